"""GPU: the crop of live streams -- dvsg_tps_render_zoom_nv12, dvsg_crop_ratchet_f32, dvsg_tps_coefficients_f32 and
OnlineStabilizer(crop=...).

Every new kernel is a composition of pinned entry points or has a NumPy restatement (tests/ratchet_ref.py), so the bar is
BIT equality throughout.  Output buffers are pre-filled with a poison byte or NaN and nothing outside the documented region
may change."""
import ctypes

import numpy as np
import pytest

import crop_ref
import inputs
import nv12_ref
import ratchet_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
F32 = np.float32
INT32_MAX = 2 ** 31 - 1


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
    return None if t is None else t.data_ptr()


def _equal(got, want, what):
    import torch
    if got.dtype.is_floating_point:   # bitwise, NaN included
        it = torch.int32 if got.dtype == torch.float32 else torch.int64
        got, want = got.contiguous().view(it), want.contiguous().view(it)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError("%s: %d values differ, max %g" % (what, int((d > 0).sum()), float(d.max())))


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.buf if isinstance(x, nv12_ref.Batch) else x)).cuda()


def _coord(n):
    from coupe.dvsg_amd.model import V_SRC
    return _dev(np.tile(V_SRC[None], (n, 1, 1)))


def _render_nv12(handle, F, b, buf, ob, out, zoom="plain"):
    """dvsg_tps_render_zoom_nv12 (zoom a device tensor or None = NULL) or, with zoom="plain", dvsg_tps_render_nv12 -> T"""
    import torch
    T = torch.full((b.n, 2, 28), float("nan"), device="cuda")
    head = (handle, _ptr(F), _ptr(buf), _ptr(buf) + b.uv_offset, b.pitch, b.frame_stride, b.n, b.H, b.W)
    tail = (_ptr(T), _ptr(out), _ptr(out) + ob.uv_offset, ob.pitch, ob.frame_stride)
    if isinstance(zoom, str):
        _call("dvsg_tps_render_nv12", *head, *tail)
    else:
        _call("dvsg_tps_render_zoom_nv12", *head, _ptr(zoom), *tail)
    return T


def _warp_zoom(U, T, zoom):
    """dvsg_tps_warp_zoom_f32 of U [n,h,w,C] at its own size"""
    import torch
    n, h, w, C = (int(v) for v in U.shape)
    out = torch.full_like(U, float("nan"))
    _call("dvsg_tps_warp_zoom_f32", _ptr(U), _ptr(_coord(n)), _ptr(T), _ptr(zoom), n, h, w, C, 25, h, w, _ptr(out), None, None)
    return out


def _T_of_render_u8(handle, F, n, H, W):
    import torch
    T8 = torch.full((n, 2, 28), float("nan"), device="cuda")
    rgb = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    f32 = torch.empty((n, H, W, 3), device="cuda")
    _call("dvsg_tps_render_u8", handle, _ptr(F), _ptr(rgb), n, H, W, 0, _ptr(T8), _ptr(f32), None, 0, 0)
    return T8


def _planes_by_definition(b, buf, T, zoom):
    """The two planes as the header defines them, in torch: (luma [n,H,W] uint8, chroma [n,H/2,W] uint8)."""
    import torch
    n, H, W = b.n, b.H, b.W
    y = buf[:, :H, :W]
    uv = buf[:, b.uv_row:b.uv_row + H // 2, :W]
    Yf = (y.double() / 255.0).float().reshape(n, H, W, 1).contiguous()
    Cf = ((uv.double() - 128.0) / 255.0).float().reshape(n, H // 2, W // 2, 2).contiguous()
    luma = (_warp_zoom(Yf, T, zoom).double() * 255.0).clamp(0, 255).to(torch.uint8).reshape(n, H, W)   # truncation, saturating
    chroma = torch.floor(_warp_zoom(Cf, T, zoom).double() * 255.0 + 128.5).clamp(0, 255).to(torch.uint8).reshape(n, H // 2, W)
    return luma, chroma


# ---------------------------------------------------------------------------------------------------------------------
# 1. the zoomed NV12 render == dvsg_tps_warp_zoom_f32 on each plane, with the byte rules of the header
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,pitch,uv_row,opitch,ouv_row", [
    (1, 4, 6, 6, 4, 8, 4), (1, 20, 32, 40, 24, 33, 21),   # the second: odd row addresses
    (2, 12, 516, 516, 12, 516, 12),                       # several column blocks in the luma plane, one in the chroma plane
    (3, 68, 102, 102, 68, 128, 72),
])
def test_zoomed_render_is_the_composition(net, n, H, W, pitch, uv_row, opitch, ouv_row):
    import torch
    b = nv12_ref.Batch(700 + H + W, n, H, W, pitch, uv_row)
    ob = nv12_ref.Batch(0, n, H, W, opitch, ouv_row, fill=POISON)
    buf = _dev(b)
    F = _dev(inputs.control_vectors(710 + W, n))
    T8 = _T_of_render_u8(net.handle, F, n, H, W)
    zoom = _dev(np.array([1.0, 0.93, 0.5], dtype=F32)[:n] if n > 1 else np.array([0.93], dtype=F32))
    out = _dev(ob)
    T = _render_nv12(net.handle, F, b, buf, ob, out, zoom)
    luma, chroma = _planes_by_definition(b, buf, T8, zoom)
    torch.cuda.synchronize()
    assert torch.isfinite(T).all()
    _equal(T, T8, "T")
    _equal(out[:, :H, :W], luma, "luma plane")
    _equal(out[:, ouv_row:ouv_row + H // 2, :W], chroma, "chroma plane")
    assert (ob.outside(out.cpu().numpy()) == POISON).all(), "bytes outside the two planes changed"
    assert np.array_equal(buf.cpu().numpy(), b.buf), "the source changed"
    # zoom == 1.0f and zoom == NULL: dvsg_tps_render_nv12's bytes
    plain = _dev(ob)
    _render_nv12(net.handle, F, b, buf, ob, plain)
    for z in (torch.ones(n, device="cuda"), None):
        one = _dev(ob)
        T1 = _render_nv12(net.handle, F, b, buf, ob, one, z)
        _equal(one, plain, "zoom %s against dvsg_tps_render_nv12" % ("1" if z is not None else "NULL"))
        _equal(T1, T8, "T")
    if n > 1:
        assert not torch.equal(out[1:], plain[1:]), "a zoom below 1 must change the picture"
        _equal(out[0], plain[0], "frame 0 has zoom 1")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the ratchet == its NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def _gpu_ratchet(state_d, slots, ka, Da, kb, Db, margin, crop_min, recover):
    import torch
    n = len(slots)
    zoom = torch.full((n + 1,), float("nan"), device="cuda")
    free = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    ka_d, kb_d = _dev(np.asarray(ka, np.int32)), (_dev(np.asarray(kb, np.int32)) if kb is not None else None)
    slots_d = _dev(np.asarray(slots, np.int32))
    _call("dvsg_crop_ratchet_f32", _ptr(ka_d), Da, _ptr(kb_d), Db, _ptr(slots_d), n, _ptr(state_d),
          int(state_d.numel()) - 1, margin, crop_min, recover, _ptr(zoom), _ptr(free))
    torch.cuda.synchronize()
    return zoom.cpu().numpy(), free.cpu().numpy()


@pytest.mark.parametrize("recover", [0.0, 0.03])
@pytest.mark.parametrize("two_planes", [False, True])
def test_ratchet_is_its_numpy_restatement(two_planes, recover):
    """Three calls in a row on one state tensor (the second and third start from what the one before left): keys 0, D,
    above D and INT32_MAX, permuted slots, one slot out of range on either side, crop_min binding (key 0 and small
    keys), untouched state entries and the element behind every output keeping their bits."""
    import torch
    Da, Db = 35 * 63, 17 * 31
    n_state = 9
    rng = np.random.default_rng(17 + two_planes)
    state = np.concatenate([rng.uniform(0.55, 1.0, n_state).astype(F32), np.array([np.nan], F32)])   # [n_state] + a guard
    state[2] = F32(1.0)
    state_d = _dev(state)
    ref = state[:n_state].copy()
    margin, crop_min = 2.0 / 17, 0.5
    slots = [[4, 0, 7, n_state, 2, -1, 8, 5], [8, 7, 5, 4, 2, 0, 1, 3], [1, 2, 0, 3, 6, 4, 5, 7]]
    for k, sl in enumerate(slots):
        ka = np.array([0, Da, Da + 5, INT32_MAX, int(0.9 * Da), int(0.62 * Da), int(0.55 * Da), Da - 1], np.int64)
        kb = np.array([Db, int(0.8 * Db), INT32_MAX, 0, Db + 1, int(0.97 * Db), Db - 1, int(0.3 * Db)], np.int64)
        ka, kb = np.roll(ka, k), np.roll(kb, 3 * k)
        want_z, want_f, written = ratchet_ref.ratchet(ref, sl, ka, Da, kb if two_planes else None, Db, margin, crop_min, recover)
        got_z, got_f = _gpu_ratchet(state_d, sl, ka, Da, kb if two_planes else None, Db, margin, crop_min, recover)
        assert written.sum() == (6 if k == 0 else 8)
        assert got_z[:-1].tobytes() == want_z.tobytes(), (k, got_z, want_z)
        assert got_f[:-1].tobytes() == want_f.tobytes(), (k, got_f, want_f)
        assert np.isnan(got_z[-1]) and np.isnan(got_f[-1]), "wrote past an output"
        got_state = state_d.cpu().numpy()
        assert got_state[:n_state].tobytes() == ref.tobytes(), (k, got_state, ref)
        assert np.isnan(got_state[n_state]), "wrote past the state"
        if k == 0:   # slots 1, 3, 6 were not named: their bits are the seeded ones
            assert got_state[[1, 3, 6]].tobytes() == state[[1, 3, 6]].tobytes()
            assert (want_z[written] == F32(crop_min)).any(), "crop_min was meant to bind"
        if recover == 0.0:
            assert (ref <= state[:n_state]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. scan -> ratchet -> zoomed render leaves no border in either plane
# ---------------------------------------------------------------------------------------------------------------------
def _scan(net, F, gh, gw, zoom=None):
    """dvsg_tps_coverage_net_f32 with source and output grid (gh, gw) -> (n_border, key_min) int32 [n] on the device"""
    import torch
    n = int(F.shape[0])
    need = ctypes.c_size_t()
    from coupe.dvsg_amd import _lib
    _lib.call("dvsg_tps_coverage_workspace_bytes", n, gh, gw, ctypes.byref(need))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
    res = torch.full((2, n), -7, dtype=torch.int32, device="cuda")
    T = torch.empty((n, 2, 28), device="cuda")
    _call("dvsg_tps_coverage_net_f32", net.handle, _ptr(F), _ptr(zoom), n, gh, gw, gh, gw, _ptr(T), _ptr(res[0]), _ptr(res[1]),
          _ptr(ws), ws.numel() * 8)
    return res[0], res[1]


@pytest.mark.parametrize("H,W", [(36, 64), (72, 128)])
def test_chain_leaves_no_border_in_either_plane(net, H, W):
    """Every draw of ratchet_ref.BORDER_FREE_DRAWS at this size, none left out: |F_t| <= 0.1 because DESIGN section
    5.00000's smooth-map caveat bounds what the margin can promise (a map that bends by much less than a pixel over one
    cell).  The draws were chosen on the CPU so that the oracle's restatement gives 0 on both grids
    (tests/test_online_crop_cpu.py).  Scan both planes, ratchet from 1.0 with the chroma margin, render; a second pair of
    scans at the rendered zoom reports 0 border pixels for luma and for chroma, and the rendered luma holds no black pixel
    (the source's luma is >= 16) where the plain render has some."""
    import torch
    draws = [d for d in ratchet_ref.BORDER_FREE_DRAWS if d[:2] == (H, W)]
    n = len(draws)
    assert n >= 10
    F = _dev(np.concatenate([ratchet_ref.draw_F(seed, a) for _, _, seed, a in draws]))
    (lh, lw), (ch, cw) = ratchet_ref.plane_grids(H, W)
    nb_l, key_l = _scan(net, F, lh, lw)
    nb_c, key_c = _scan(net, F, ch, cw)
    state = torch.ones(n, device="cuda")
    slots = torch.arange(n, dtype=torch.int32, device="cuda")
    zoom = torch.full((n,), float("nan"), device="cuda")
    free = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    _call("dvsg_crop_ratchet_f32", _ptr(key_l), (lh - 1) * (lw - 1), _ptr(key_c), (ch - 1) * (cw - 1), _ptr(slots), n,
          _ptr(state), n, ratchet_ref.nv12_margin(H, W), 0.5, 0.0, _ptr(zoom), _ptr(free))
    b = nv12_ref.smooth_batch(800 + H, n, H, W)
    ob = nv12_ref.Batch(0, n, H, W, fill=POISON)
    buf, out, plain = _dev(b), _dev(ob), _dev(ob)
    _render_nv12(net.handle, F, b, buf, ob, out, zoom)
    _render_nv12(net.handle, F, b, buf, ob, plain)
    left_l, _ = _scan(net, F, lh, lw, zoom)
    left_c, _ = _scan(net, F, ch, cw, zoom)
    torch.cuda.synchronize()
    z = zoom.cpu().numpy()
    print("H=%d W=%d zoom %s free %s" % (H, W, z.tolist(), free.cpu().numpy().tolist()))
    assert (nb_l > 0).all() and (nb_c > 0).all(), "the plain grids have a border"
    assert ((z > 0.5) & (z < 1.0)).all(), "a draw hit crop_min or kept zoom 1: it says nothing about the margin"
    want = ratchet_ref.free_of_keys(key_l.cpu().numpy(), key_c.cpu().numpy(), H, W)
    assert free.cpu().numpy().tobytes() == want.tobytes()
    assert left_l.cpu().tolist() == [0] * n, "luma border pixels at the rendered zoom"
    assert left_c.cpu().tolist() == [0] * n, "chroma border pixels at the rendered zoom"
    y, _ = ob.planes(out.cpu().numpy())
    y_plain, _ = ob.planes(plain.cpu().numpy())
    assert (y != 0).all() and all((y_plain[i] == 0).any() for i in range(n))


# ---------------------------------------------------------------------------------------------------------------------
# 4. online, NV12, crop="auto"
# ---------------------------------------------------------------------------------------------------------------------
def _model(weights, H, W):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights)
    model.get_evaluation_model(7)
    model.precision = "f32"
    return model


def test_online_nv12_auto(synthetic_weights):
    """Two streams of different even sizes, 40 frames each (the ring of 34 wraps): the pool and every step's F_t are those
    of a run with crop=None; a stream's zoom never increases; each output is dvsg_tps_render_zoom_nv12 called with the step's
    recorded zoom; the final zoom is crop_zoom of the recorded F_t's frees (the smaller of the two planes', from crop_scan)."""
    import torch
    from coupe.dvsg_amd.clip import crop_scan, crop_zoom
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    model = _model(synthetic_weights, 37, 53)
    sizes = [(68, 102), (20, 32)]
    N = 40
    clips = [nv12_ref.smooth_batch(900 + i, N, H0, W0) for i, (H0, W0) in enumerate(sizes)]
    on = OnlineStabilizer(model, max_streams=2, frame_format="nv12", crop="auto")
    off = OnlineStabilizer(model, max_streams=2, frame_format="nv12")
    assert on.span + 2 < N
    on.pool.zero_()
    off.pool.zero_()
    sid_on, sid_off = [on.open(), on.open()], [off.open(), off.open()]
    for i in range(2):
        st = on.crop_state(sid_on[i])
        assert st["zoom"] == F32(1.0) and st["zoom"].dtype == np.float32 and st["free"] is None
    zooms, Fs, outs = [[], []], [[], []], [[], []]
    order = sorted(range(2), key=lambda i: sizes[i])   # batch order: by source size
    for k in range(N):
        dev = [_dev(c.buf[k]) for c in clips]
        res = on.step({sid_on[i]: dev[i] for i in range(2)})
        res_off = off.step({sid_off[i]: dev[i] for i in range(2)})
        _equal(on._F, off._F, "F_t of step %d" % k)
        _equal(on.pool, off.pool, "pool after step %d" % k)
        for row, i in enumerate(order):
            H0, W0 = sizes[i]
            st = on.crop_state(sid_on[i])
            zooms[i].append(st["zoom"])
            Fs[i].append(on._F[row].cpu().numpy())
            got = res[sid_on[i]]
            assert isinstance(got, torch.Tensor) and tuple(got.shape) == (3 * H0 // 2, W0) and got.dtype == torch.uint8
            one = nv12_ref.Batch(0, 1, H0, W0, fill=POISON)
            alone = _dev(one)
            _render_nv12(model.locnet.handle, on._F[row:row + 1].clone(), one, dev[i][None].contiguous(), one, alone,
                         _dev(np.array([st["zoom"]], dtype=F32)))
            _equal(got, alone[0], "output of stream %d, step %d" % (i, k))
            outs[i].append(got.cpu().numpy())
            if st["zoom"] < 1.0:
                assert not torch.equal(got, res_off[sid_off[i]]), "a cropped frame differs from the plain one"
    torch.cuda.synchronize()
    for i, (H0, W0) in enumerate(sizes):
        z = np.array(zooms[i], dtype=np.float64)
        print("stream %d %dx%d zoom %s" % (i, H0, W0, [round(float(v), 4) for v in zooms[i]]))
        assert (np.diff(z) <= 0).all() and z[0] < 1.0
        F = np.stack(Fs[i])
        (lh, lw), (ch, cw) = ratchet_ref.plane_grids(H0, W0)
        free = np.minimum(crop_scan(model, F, (lh, lw))["free"], crop_scan(model, F, (ch, cw))["free"])
        want = crop_zoom(free, ratchet_ref.nv12_margin(H0, W0), 0.5)
        got = on.crop_state(sid_on[i])
        assert got["zoom"].tobytes() == want.tobytes(), (got, want)
        assert got["free"] == free[-1]
    # stabilize_clips passes crop through: frame k of a clip at the zoom the ratchet has reached at frame k
    both = stabilize_clips(model, [c.buf for c in clips], frame_format="nv12", crop="auto")
    for i in range(2):
        assert isinstance(both[i], np.ndarray) and np.array_equal(both[i], np.stack(outs[i])), "clip %d" % i


# ---------------------------------------------------------------------------------------------------------------------
# 5. online, RGB
# ---------------------------------------------------------------------------------------------------------------------
def _tps_launches(fn):
    """the number of profiled launch groups of the TPS warp class (renders, warps and coverage scans) that fn() issues"""
    from coupe.dvsg_amd import _lib
    _lib.call("dvsg_prof_begin", 6)
    fn()
    ms, n, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    _lib.call("dvsg_prof_end", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by))
    return n.value


def test_online_source_res_u8(synthetic_weights):
    """source_res uint8 frames: every output is dvsg_tps_render_zoom_u8 with the step's recorded zoom; pool and F_t are
    those of a run without crop; crop=0.9 renders every frame at np.float32(0.9) and launches no scan; crop_start=0.8
    starts there; a closed and reopened stream starts at crop_start again."""
    import torch
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(synthetic_weights, 37, 53)
    H0, W0, N = 40, 60, 5
    frames = _dev((inputs.smooth_frames(31, N, H0, W0) * 255).astype(np.uint8))
    kw = dict(source_res=True, as_uint8=True)
    auto = OnlineStabilizer(model, crop="auto", crop_start=0.8, crop_margin=0.25, **kw)   # free - 0.25 < 0.8: the zoom moves
    fixed = OnlineStabilizer(model, crop=0.9, **kw)
    off = OnlineStabilizer(model, **kw)
    for s in (auto, fixed, off):
        s.pool.zero_()
    sa, sf, so = auto.open(), fixed.open(), off.open()
    assert auto.crop_state(sa)["zoom"] == F32(0.8) and fixed.crop_state(sf) == dict(zoom=F32(0.9), free=None)
    counts = []
    prev = F32(0.8)
    for k in range(N):
        res = {}
        counts.append([_tps_launches(lambda s=s, sid=sid, name=name: res.__setitem__(name, s.push(sid, frames[k])))
                       for s, sid, name in ((auto, sa, "auto"), (fixed, sf, "fixed"), (off, so, "off"))])
        for s in (auto, fixed):
            _equal(s._F, off._F, "F_t of step %d" % k)
            _equal(s.pool, off.pool, "pool after step %d" % k)
        za, zf = auto.crop_state(sa)["zoom"], fixed.crop_state(sf)["zoom"]
        assert zf.tobytes() == F32(0.9).tobytes() and za <= prev
        prev = za
        for name, z, s in (("auto", za, auto), ("fixed", zf, fixed)):
            want = torch.full((1, H0, W0, 3), POISON, dtype=torch.uint8, device="cuda")
            T = torch.empty((1, 2, 28), device="cuda")
            F1, z1 = s._F[:1].clone(), _dev(np.array([z], dtype=F32))   # named: they must outlive the launch
            _call("dvsg_tps_render_zoom_u8", model.locnet.handle, _ptr(F1), _ptr(frames[k:k + 1]), 1, H0, W0, 0, _ptr(z1),
                  _ptr(T), None, _ptr(want), W0, 0)
            _equal(res[name], want[0], "%s output of step %d" % (name, k))
        assert not torch.equal(res["fixed"], res["off"])
    torch.cuda.synchronize()
    # per step: the stabilise call's warp and the render, plus ONE scan with "auto" and none with a fixed zoom
    assert all(c[1] == c[2] and c[0] == c[2] + 1 for c in counts), counts
    assert prev < F32(0.8), "the ratchet was meant to move below crop_start"
    auto.close(sa)
    sb = auto.open()
    assert auto._streams[sb][0] == 0, "the reopened stream takes the same ring"
    assert auto.crop_state(sb) == dict(zoom=F32(0.8), free=None)
    auto.push(sb, frames[0])
    assert auto.crop_state(sb)["zoom"] <= F32(0.8) and auto.crop_state(sb)["free"] is not None


@pytest.mark.parametrize("crop", ["auto", 0.9])
def test_online_model_size(synthetic_weights, crop):
    """Model-size output: the float path is dvsg_tps_warp_zoom_f32 of the step's input slot with the T of
    dvsg_tps_render_u8 for its F_t and the recorded zoom; with side_by_side and as_uint8 the left half stays the uncropped
    source and the right half is the cropped frame's bytes.  Two streams, uint8 frames of the model's size and larger."""
    import torch
    from coupe.dvsg_amd.online import OnlineStabilizer
    h, w = 37, 53
    model = _model(synthetic_weights, h, w)
    N = 4
    clips = [_dev((inputs.smooth_frames(41, N, h, w) * 255).astype(np.uint8)),
             _dev((inputs.smooth_frames(42, N, 50, 70) * 255).astype(np.uint8))]
    on = OnlineStabilizer(model, max_streams=2, crop=crop)
    side = OnlineStabilizer(model, max_streams=2, crop=crop, side_by_side=True, as_uint8=True)
    off = OnlineStabilizer(model, max_streams=2, side_by_side=True, as_uint8=True)
    for s in (on, side, off):
        s.pool.zero_()
    sids = {s: [s.open(), s.open()] for s in (on, side, off)}
    for k in range(N):
        res = {s: s.step({sids[s][i]: clips[i][k] for i in range(2)}) for s in (on, side, off)}
        for s in (on, side):
            _equal(s._F, off._F, "F_t of step %d" % k)
            _equal(s.pool, off.pool, "pool after step %d" % k)
        T8 = _T_of_render_u8(model.locnet.handle, on._F.clone(), 2, h, w)
        _equal(on._T, T8, "T of step %d" % k)
        for row, i in enumerate((1, 0)):   # batch order: resized uint8 first, then same-size uint8
            z = on.crop_state(sids[on][i])["zoom"]
            assert side.crop_state(sids[side][i])["zoom"].tobytes() == z.tobytes()
            if crop != "auto":
                assert z.tobytes() == F32(0.9).tobytes()
            ring = on._streams[sids[on][i]][0]
            u = on.pool[ring * on.frames_per_stream + on.span + 1][None].clone()
            want = _warp_zoom(u, T8[row:row + 1].clone(), _dev(np.array([z], dtype=F32)))[0]
            got = res[on][sids[on][i]]
            assert got.dtype == torch.float32 and tuple(got.shape) == (h, w, 3)
            _equal(got, want, "float output of stream %d, step %d" % (i, k))
            o8, sd = res[side][sids[side][i]]
            _, sd_off = res[off][sids[off][i]]
            want8 = (want.double() * 255.0).clamp(0, 255).to(torch.uint8)
            _equal(o8, want8, "uint8 output of stream %d, step %d" % (i, k))
            _equal(sd[:, :w], sd_off[:, :w], "unstable half of stream %d, step %d" % (i, k))
            _equal(sd[:, w:], want8, "stabilised half of stream %d, step %d" % (i, k))
    torch.cuda.synchronize()
