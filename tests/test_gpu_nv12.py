"""GPU: NV12 as a frame format (dvsg_frames_nv12_to_rgb_u8, dvsg_frames_ingest_nv12, dvsg_tps_render_nv12,
OnlineStabilizer(frame_format="nv12")).

Every new kernel is defined as a composition of entry points that are pinned elsewhere, so the bar is BIT equality
throughout: the conversion against the int32 restatement of tests/nv12_ref.py (all 2^24 triples), the ingest against
convert + dvsg_frames_ingest_u8, the render against dvsg_tps_warp_f32 on each plane with the byte rules written in torch.
Output buffers are pre-filled with a poison byte or NaN and nothing outside the documented region may change."""
import numpy as np
import pytest

import inputs
import nv12_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5


@pytest.fixture(scope="module")
def net(synthetic_weights):
    import torch
    assert torch.cuda.is_available()
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def _call(name, *args):
    import torch
    from coupe.dvsg_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _equal(got, want, what):
    import torch
    if got.dtype.is_floating_point:   # bitwise, NaN included
        got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError("%s: %d values differ, max %g" % (what, int((d > 0).sum()), float(d.max())))


def _dev(batch):
    import torch
    return torch.from_numpy(batch.buf).cuda()


def _convert(batch, buf, matrix, flip):
    """dvsg_frames_nv12_to_rgb_u8 of a batch on the device -> (dst [n,H,W,3] with one poisoned frame behind it)."""
    import torch
    n, H, W = batch.n, batch.H, batch.W
    dst = torch.full((n + 1, H, W, 3), POISON, dtype=torch.uint8, device="cuda")
    _call("dvsg_frames_nv12_to_rgb_u8", _ptr(buf), _ptr(buf) + batch.uv_offset, batch.pitch, batch.frame_stride, n, H, W,
          matrix, flip, _ptr(dst))
    return dst


# ---------------------------------------------------------------------------------------------------------------------
# 1. the conversion
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every_triple():
    """One packed 4096 x 4096 frame in which every (Y, U, V) occurs exactly once: 2 x 2 block (bi, bj) carries
    U = bi % 256, V = bj % 256, and its four pixels are Y = 4 * (8 * (bi // 256) + bj // 256) + 2 * (i % 2) + j % 2."""
    N = 4096
    b = nv12_ref.Batch(0, 1, N, N, fill=0)
    bi, bj = np.meshgrid(np.arange(N // 2), np.arange(N // 2), indexing="ij")
    sub = 4 * (8 * (bi // 256) + bj // 256)
    y, uv = b.planes()
    for di in (0, 1):
        for dj in (0, 1):
            y[0, di::2, dj::2] = sub + 2 * di + dj
    uv[0, :, 0::2] = bi % 256
    uv[0, :, 1::2] = bj % 256
    key = (y[0].astype(np.int64) << 16) | (np.repeat(np.repeat(uv[0, :, 0::2], 2, 0), 2, 1).astype(np.int64) << 8) \
        | np.repeat(np.repeat(uv[0, :, 1::2], 2, 0), 2, 1)
    assert (np.bincount(key.ravel(), minlength=1 << 24) == 1).all()
    return b


@pytest.mark.parametrize("matrix", [nv12_ref.BT601, nv12_ref.BT709])
def test_convert_exhaustive(every_triple, matrix):
    import torch
    b = every_triple
    dst = _convert(b, _dev(b), matrix, 0)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[1] == POISON).all()
    y, uv = b.planes()
    for r in range(0, b.H, 512):   # slabs on the host
        want = nv12_ref.nv12_to_rgb(y[0, r:r + 512], uv[0, r // 2:r // 2 + 256], matrix)
        assert np.array_equal(got[0, r:r + 512], want), "rows %d.." % r


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("n,H,W,pitch,uv_row", [(3, 6, 10, 10, 6), (2, 34, 70, 128, 48), (1, 4, 4, 4, 4),
                                                (2, 6, 10, 11, 7)])   # the last: rows at odd addresses, scalar loads
def test_convert_layouts(n, H, W, pitch, uv_row, flip):
    import torch
    b = nv12_ref.Batch(100 + H + pitch, n, H, W, pitch, uv_row)
    for matrix in (nv12_ref.BT601, nv12_ref.BT709):
        got = _convert(b, _dev(b), matrix, flip).cpu().numpy()
        assert (got[n] == POISON).all()
        assert np.array_equal(got[:n], nv12_ref.nv12_to_rgb(*b.planes(), matrix, flip))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ingest == convert + dvsg_frames_ingest_u8
# ---------------------------------------------------------------------------------------------------------------------
MODEL = (38, 54)   # the 37 x 53 of tests/test_gpu_source_res.py, rounded to even (the same-size path needs an even size)


INGEST_LAYOUTS = [
    (MODEL, MODEL, 54, 38), (MODEL, MODEL, 64, 40),            # same size: / 255.
    ((68, 102), MODEL, 102, 68), ((68, 102), MODEL, 128, 72),   # down-scale
    ((20, 32), MODEL, 32, 20), ((20, 32), (37, 53), 33, 21),    # up-scale; an odd model size and odd row addresses
]


@pytest.mark.parametrize("n,src,dst,pitch,uv_row", [(n,) + c for c in INGEST_LAYOUTS for n in (1, 3)] +
                         [(1, (1080, 1920), (288, 512), 1920, 1080)])
def test_ingest_is_convert_then_ingest_u8(n, src, dst, pitch, uv_row):
    import torch
    (H0, W0), (h, w) = src, dst
    n_pool = n + 2
    slots = np.array([n + 1, 0, 2][:n] if n > 1 else [1], dtype=np.int32)
    if n > 1:
        slots[1] = n_pool + 3   # out of range: that frame is skipped
    slots_d = torch.from_numpy(slots).cuda()
    b = nv12_ref.Batch(200 + H0 + pitch + n, n, H0, W0, pitch, uv_row)
    buf = _dev(b)
    for matrix in (nv12_ref.BT601, nv12_ref.BT709):
        got = torch.full((n_pool, h, w, 3), float("nan"), device="cuda")
        want = got.clone()
        _call("dvsg_frames_ingest_nv12", _ptr(buf), _ptr(buf) + b.uv_offset, b.pitch, b.frame_stride, n, H0, W0, matrix,
              _ptr(got), n_pool, _ptr(slots_d), h, w)
        rgb = _convert(b, buf, matrix, 0)
        _call("dvsg_frames_ingest_u8", _ptr(rgb), n, H0, W0, 0, _ptr(want), n_pool, _ptr(slots_d), h, w, 0, 0, 0)
        torch.cuda.synchronize()
        _equal(got, want, "pool (matrix %d)" % matrix)
        written = [int(s) for s in slots if 0 <= s < n_pool]
        assert len(written) == (n if n == 1 else n - 1)
        for s in range(n_pool):
            assert bool(torch.isnan(got[s]).all()) == (s not in written), "pool frame %d" % s
            assert s not in written or bool(torch.isfinite(got[s]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. render == dvsg_tps_warp_f32 on each plane, with the byte rules of the header
# ---------------------------------------------------------------------------------------------------------------------
def _coord(n):
    import torch
    from coupe.dvsg_amd.model import V_SRC
    return torch.from_numpy(np.ascontiguousarray(np.tile(V_SRC[None], (n, 1, 1)))).cuda()


def _render(handle, F, b, buf, ob, out):
    """dvsg_tps_render_nv12 of batch b (device bytes buf) into `out`, a device buffer laid out as batch ob -> T."""
    import torch
    T = torch.full((b.n, 2, 28), float("nan"), device="cuda")
    _call("dvsg_tps_render_nv12", handle, _ptr(F), _ptr(buf), _ptr(buf) + b.uv_offset, b.pitch, b.frame_stride, b.n, b.H,
          b.W, _ptr(T), _ptr(out), _ptr(out) + ob.uv_offset, ob.pitch, ob.frame_stride)
    return T


def _warp(U, T, x_s=None, y_s=None):
    """dvsg_tps_warp_f32 of U [n,h,w,C] at its own size (U None: the grid only)."""
    import torch
    n, h, w = (int(v) for v in (U.shape[:3] if U is not None else x_s.shape))
    C = int(U.shape[3]) if U is not None else 1
    out = torch.full_like(U, float("nan")) if U is not None else None
    _call("dvsg_tps_warp_f32", _ptr(U), _ptr(_coord(n)), _ptr(T), n, h, w, C, 25, h, w, _ptr(out), _ptr(x_s), _ptr(y_s))
    return out


def _planes_by_definition(b, buf, T):
    """The two planes as the header defines them, in torch: (luma [n,H,W] uint8, chroma [n,H/2,W] uint8)."""
    import torch
    n, H, W = b.n, b.H, b.W
    y = buf[:, :H, :W]
    uv = buf[:, b.uv_row:b.uv_row + H // 2, :W]
    Yf = (y.double() / 255.0).float().reshape(n, H, W, 1).contiguous()
    Cf = ((uv.double() - 128.0) / 255.0).float().reshape(n, H // 2, W // 2, 2).contiguous()
    luma = (_warp(Yf, T).double() * 255.0).clamp(0, 255).to(torch.uint8).reshape(n, H, W)   # truncation, saturating
    chroma = torch.floor(_warp(Cf, T).double() * 255.0 + 128.5).clamp(0, 255).to(torch.uint8).reshape(n, H // 2, W)
    return luma, chroma


@pytest.mark.parametrize("n,H,W,pitch,uv_row,opitch,ouv_row", [
    (3, 68, 102, 102, 68, 128, 72), (1, 20, 32, 40, 24, 33, 21), (1, 4, 6, 6, 4, 8, 4), (1, 1080, 1920, 1920, 1080, 2048, 1088),
    (2, 12, 516, 516, 12, 516, 12),   # more than one column block in the luma plane, exactly one in the chroma plane
])
def test_render_is_the_composition(net, n, H, W, pitch, uv_row, opitch, ouv_row):
    import torch
    b = nv12_ref.Batch(300 + H + W, n, H, W, pitch, uv_row)
    ob = nv12_ref.Batch(0, n, H, W, opitch, ouv_row, fill=POISON)
    buf, out = _dev(b), _dev(ob)
    F = torch.from_numpy(inputs.control_vectors(310 + W, n)).cuda()
    T = _render(net.handle, F, b, buf, ob, out)
    # T is dvsg_tps_render_u8's for the same F_t
    T8 = torch.full_like(T, float("nan"))
    rgb = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    f32 = torch.empty((n, H, W, 3), device="cuda")
    _call("dvsg_tps_render_u8", net.handle, _ptr(F), _ptr(rgb), n, H, W, 0, _ptr(T8), _ptr(f32), 0, 0, 0)
    luma, chroma = _planes_by_definition(b, buf, T8)
    torch.cuda.synchronize()
    assert torch.isfinite(T).all()
    _equal(T, T8, "T")
    _equal(out[:, :H, :W], luma, "luma plane")
    _equal(out[:, ouv_row:ouv_row + H // 2, :W], chroma, "chroma plane")
    got = out.cpu().numpy()
    assert (ob.outside(got) == POISON).all(), "bytes outside the two planes changed"
    assert np.array_equal(buf.cpu().numpy(), b.buf), "the source changed"


# ---------------------------------------------------------------------------------------------------------------------
# 4. the border is neutral
# ---------------------------------------------------------------------------------------------------------------------
def _invalid(x_s, y_s, H, W):
    """not sample_a_valid: float32 x = ((x_s + 1) W) / 2, valid iff 0 <= x < W - 1 and 0 <= y < H - 1 (NaN invalid)."""
    x = ((x_s + np.float32(1.0)) * np.float32(W)) / np.float32(2.0)
    y = ((y_s + np.float32(1.0)) * np.float32(H)) / np.float32(2.0)
    assert x.dtype == np.float32 and y.dtype == np.float32
    x0, y0 = np.floor(x), np.floor(y)
    valid = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
    return ~valid


def test_border_is_neutral(net):
    import torch
    n, H, W = 2, 36, 52
    b = nv12_ref.Batch(400, n, H, W)
    ob = nv12_ref.Batch(0, n, H, W, fill=POISON)
    buf, out = _dev(b), _dev(ob)
    Fh = np.zeros((n, 25, 2), np.float32)
    Fh[:, :, 0] = 0.3
    T = _render(net.handle, torch.from_numpy(Fh).cuda(), b, buf, ob, out)
    grids = []
    for h, w in ((H, W), (H // 2, W // 2)):
        xs, ys = torch.empty((n, h, w), device="cuda"), torch.empty((n, h, w), device="cuda")
        _warp(None, T, xs, ys)
        grids.append(_invalid(xs.cpu().numpy(), ys.cpu().numpy(), h, w))
    both = grids[0] & np.repeat(np.repeat(grids[1], 2, axis=1), 2, axis=2)
    assert both.any() and not both.all(), "%d of %d pixels" % (both.sum(), both.size)
    y, uv = ob.planes(out.cpu().numpy())
    U, V = (np.repeat(np.repeat(uv[:, :, k::2], 2, axis=1), 2, axis=2) for k in (0, 1))
    assert (y[both] == 0).all() and (U[both] == 128).all() and (V[both] == 128).all()
    assert (y[~grids[0]] != 0).any()   # and the inside is a picture


# ---------------------------------------------------------------------------------------------------------------------
# 5. online
# ---------------------------------------------------------------------------------------------------------------------
def _model(weights, H, W):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights)
    model.get_evaluation_model(7)
    model.precision = "f32"
    return model


@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
def test_online_nv12(synthetic_weights, matrix):
    """Two streams of different source sizes, 3 steps: pool and F_t are those of an RGB source_res run fed the converted
    frames, each output is dvsg_tps_render_nv12 called directly with the step's F_t row, NumPy in gives NumPy out, and
    stabilize_clips on the two clips is the per-stream pushes."""
    import torch
    from coupe.dvsg_amd.online import YUV_MATRICES, OnlineStabilizer, stabilize_clips
    model = _model(synthetic_weights, 37, 53)
    sizes = [(68, 102), (20, 32)]
    clips = [nv12_ref.smooth_batch(500 + i, 3, H0, W0) for i, (H0, W0) in enumerate(sizes)]
    on = OnlineStabilizer(model, max_streams=2, frame_format="nv12", yuv_matrix=matrix)
    off = OnlineStabilizer(model, max_streams=2, source_res=True)
    assert on.source_res and on._T is not None
    on.pool.zero_()
    off.pool.zero_()
    sid_on, sid_off = [on.open(), on.open()], [off.open(), off.open()]
    m = YUV_MATRICES[matrix]
    outs = [[], []]
    for k in range(3):
        dev = [torch.from_numpy(c.buf[k]).cuda() for c in clips]
        rgb = [_convert(nv12_ref.Batch(0, 1, *sizes[i], fill=0), dev[i], m, 0)[0] for i in range(2)]
        res = on.step({sid_on[i]: dev[i] for i in range(2)})
        off.step({sid_off[i]: rgb[i] for i in range(2)})
        _equal(on._F, off._F, "F_t of step %d" % k)
        _equal(on.pool, off.pool, "pool after step %d" % k)
        for row, i in enumerate(sorted(range(2), key=lambda i: sizes[i])):   # batch order: by source size
            H0, W0 = sizes[i]
            got = res[sid_on[i]]
            assert isinstance(got, torch.Tensor) and tuple(got.shape) == (3 * H0 // 2, W0) and got.dtype == torch.uint8
            one = nv12_ref.Batch(0, 1, H0, W0, fill=POISON)
            alone = _dev(one)
            _render(model.locnet.handle, on._F[row:row + 1].clone(), one, dev[i][None].contiguous(), one, alone)
            _equal(got, alone[0], "output of stream %d, step %d" % (i, k))
            outs[i].append(got.cpu().numpy())
    torch.cuda.synchronize()
    # NumPy in -> NumPy out, through push; the same bits
    host = OnlineStabilizer(model, frame_format="nv12", yuv_matrix=matrix)
    sid = host.open()
    for k in range(3):
        got = host.push(sid, clips[1].buf[k])
        assert isinstance(got, np.ndarray) and np.array_equal(got, outs[1][k])
    both = stabilize_clips(model, [c.buf for c in clips], frame_format="nv12", yuv_matrix=matrix)
    for i in range(2):
        assert isinstance(both[i], np.ndarray) and both[i].dtype == np.uint8
        assert np.array_equal(both[i], np.stack(outs[i])), "clip %d" % i


def test_online_nv12_rejects_bad_frames(synthetic_weights):
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(synthetic_weights, 37, 53)
    on = OnlineStabilizer(model, frame_format="nv12")
    sid = on.open()
    with pytest.raises(ValueError, match="float"):
        on.push(sid, np.zeros((30, 32), np.float32))
    for shape in [(30, 31), (31, 32), (3, 2)]:   # odd W0, rows that are no 3 H0 / 2 of an even H0, too small
        with pytest.raises(ValueError, match="odd"):
            on.push(sid, np.zeros(shape, np.uint8))
    with pytest.raises(ValueError, match="NV12 frame must be"):
        on.push(sid, np.zeros((30, 32, 3), np.uint8))
    assert on._streams[sid][1] == 0   # no step was taken
    assert on.push(sid, np.full((30, 32), 128, np.uint8)).shape == (30, 32)
