"""GPU: the bicubic render filter of a view (include/dvsg_amd.h, "Views and the render filter") against its NumPy restatement
tests/bicubic_ref.py, byte for byte and -- out_f32 -- bit for bit, no pixel masked or left out.  The map's x_s, y_s come from
the grid-only form of dvsg_tps_warp_zoom_f32 at each plane's size, as the header defines them.  Synthetic weights, f32."""
import ctypes
import io

import numpy as np
import pytest

import bicubic_ref as R
import inputs
import nv12_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
ZOOM = (1.0, 0.7, 0.9)
_CACHE = {}


def _torch():
    import torch
    return torch


def _call(name, *args):
    from coupe.dvsg_amd import _lib
    _lib.call(name, *args)


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(nbytes):
    import test_conv_gemm_f64 as f64
    g = f64.Guarded(nbytes, _torch().device("cuda:0"))
    g.body.fill_(POISON)
    return g


@pytest.fixture(scope="module")
def net(synthetic_weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def vectors(n=3):
    """F_t of n = 3 frames: zero, uniform +-0.05, uniform +-0.3 (the last leaves valid and invalid pixels on every plane)"""
    rng = np.random.default_rng(77)
    F = np.zeros((n, 25, 2), np.float32)
    F[1] = rng.uniform(-0.05, 0.05, (25, 2))
    F[2] = rng.uniform(-0.3, 0.3, (25, 2))
    return F


def grid(T, zoom, n, ph, pw):
    """x_s, y_s [n, ph, pw] of the grid-only dvsg_tps_warp_zoom_f32 (U == NULL, out == NULL) with coord = V_src"""
    torch = _torch()
    V = _dev(inputs.v_src(n))
    xs = torch.empty((n, ph, pw), device="cuda")
    ys = torch.empty_like(xs)
    _call("dvsg_tps_warp_zoom_f32", None, V.data_ptr(), T.data_ptr(), zoom.data_ptr() if zoom is not None else None, n, 1, 1, 3,
          25, ph, pw, None, xs.data_ptr(), ys.data_ptr(), _stream())
    return xs.cpu().numpy(), ys.cpu().numpy()


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %r want %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def render_u8(handle, F, src, flip, zoom, want_f32, want_u8, u8_W, u8_x0):
    """One render call into guarded, poisoned outputs -> (T, out_f32 or None, the whole uint8 image or None)"""
    torch = _torch()
    n, H, W = src.shape[:3]
    T = torch.empty((n, 2, 28), device="cuda")
    gf = _guarded(n * H * W * 12) if want_f32 else None
    gu = _guarded(n * H * u8_W * 3) if want_u8 else None
    args = [handle, F.data_ptr(), src.data_ptr(), n, H, W, flip]
    if zoom is not None:
        args.append(zoom.data_ptr())
    args += [T.data_ptr(), gf.ptr() if gf else None, gu.ptr() if gu else None, u8_W, u8_x0, _stream()]
    _call("dvsg_tps_render_zoom_u8" if zoom is not None else "dvsg_tps_render_u8", *args)
    torch.cuda.synchronize()
    assert (gf is None or gf.intact()) and (gu is None or gu.intact()), "a guard byte was written"
    f32 = gf.view(torch.float32, (n, H, W, 3)).cpu().numpy() if gf else None
    u8 = gu.view(torch.uint8, (n, H, u8_W, 3)).cpu().numpy() if gu else None
    return T, f32, u8


@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("H,W", [(7, 9), (12, 21), (5, 515)])
def test_rgb_render_is_the_reference(net, H, W, zoomed):
    """dvsg_tps_render_u8 / dvsg_tps_render_zoom_u8 through a bicubic view.  7 x 9 and 12 x 21: x0 = 0 and x0 = pw - 2 occur,
    a row of 3 W bytes starts at every byte alignment, and neither width is a multiple of any vector.  5 x 515: three column
    tiles of 256 with a partial last one (blockIdx.x > 0), one partial 4-row tile, rows of 1545 bytes."""
    n = 3
    view = net.view("bicubic")
    src_h = np.random.default_rng(H * W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    src, F = _dev(src_h), _dev(vectors(n))
    zoom = _dev(np.float32(ZOOM)) if zoomed else None
    want = None
    for flip in (0, 1):
        for want_f32, want_u8, u8_W, u8_x0 in ((True, False, W, 0), (False, True, W, 0), (True, True, W, 0), (True, True, 2 * W, W)):
            T, f32, u8 = render_u8(view, F, src, flip, zoom, want_f32, want_u8, u8_W, u8_x0)
            if want is None:
                xs, ys = grid(T, zoom, n, H, W)
                ok = R.valid(H, W, xs[2], ys[2])
                assert ok.any() and (~ok).any(), "the +-0.3 frame must leave valid and invalid pixels"
                assert R.valid(H, W, xs[0], ys[0])[:-1, :-1].all()
                want = np.stack([R.render_f32(src_h[b], xs[b], ys[b]) for b in range(n)])
                assert np.abs(want).max() > 0.5
            what = "%dx%d flip=%d f32=%d u8=%d u8_W=%d" % (H, W, flip, want_f32, want_u8, u8_W)
            if want_f32:
                same_bits(f32, want[..., ::-1] if flip else want, what + " out_f32")
            if want_u8:
                same_bits(u8[:, :, u8_x0:u8_x0 + W], R.to_u8(want), what + " out_u8")
                rest = np.delete(u8, np.s_[u8_x0:u8_x0 + W], axis=2)
                assert (rest == POISON).all(), what + ": bytes of the uint8 row beyond the W columns were written"


def render_nv12(handle, F, b, buf, ob, zoom):
    torch = _torch()
    n, H, W = b.n, b.H, b.W
    T = torch.empty((n, 2, 28), device="cuda")
    g = _guarded(ob.buf.size)
    args = [handle, F.data_ptr(), buf.data_ptr(), buf.data_ptr() + b.uv_offset, b.pitch, b.frame_stride, n, H, W]
    if zoom is not None:
        args.append(zoom.data_ptr())
    args += [T.data_ptr(), g.ptr(), g.ptr() + ob.uv_offset, ob.pitch, ob.frame_stride, _stream()]
    _call("dvsg_tps_render_zoom_nv12" if zoom is not None else "dvsg_tps_render_nv12", *args)
    torch.cuda.synchronize()
    assert g.intact(), "a guard byte was written"
    return T, g.view(torch.uint8, ob.buf.shape).cpu().numpy()


def nv12_reference(b, T, zoom):
    """(y [n,H,W], uv [n,H/2,W]) bytes of the reference, and the luma / chroma validity of the last frame"""
    n, H, W = b.n, b.H, b.W
    y, uv = b.planes()
    xl, yl = grid(T, zoom, n, H, W)
    xc, yc = grid(T, zoom, n, H // 2, W // 2)
    wy = np.stack([R.to_u8(R.render_f32(y[i][..., None], xl[i], yl[i]))[..., 0] for i in range(n)])
    wc = np.stack([R.to_u8(R.render_f32(uv[i].reshape(H // 2, W // 2, 2), xc[i], yc[i], chroma=True), chroma=True).reshape(H // 2, W)
                   for i in range(n)])
    return wy, wc, R.valid(H, W, xl[-1], yl[-1]), R.valid(H // 2, W // 2, xc[-1], yc[-1])


@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("H,W,pitch", [(8, 12, 16), (10, 36, 48), (10, 520, 528)])
def test_nv12_render_is_the_reference(net, H, W, pitch, zoomed):
    """dvsg_tps_render_nv12 / dvsg_tps_render_zoom_nv12 through a bicubic view, pitch > W and a padded frame_stride (the UV
    plane starts two rows behind the luma).  The 8 x 12 chroma plane is 4 x 6: nearly every tap row clamps.  10 x 520: luma
    over three 256-column tiles, chroma over two, both planes end in a partial 4-row tile."""
    n = 3
    view = net.view("bicubic")
    b = nv12_ref.Batch(H + W, n, H, W, pitch, H + 2)
    ob = nv12_ref.Batch(0, n, H, W, pitch + 16, H + 1, fill=POISON)
    buf, F = _dev(b.buf), _dev(vectors(n))
    zoom = _dev(np.float32(ZOOM)) if zoomed else None
    T, out = render_nv12(view, F, b, buf, ob, zoom)
    wy, wc, ok_l, ok_c = nv12_reference(b, T, zoom)
    assert ok_l.any() and (~ok_l).any() and ok_c.any() and (~ok_c).any()
    gy, gc = ob.planes(out)
    same_bits(gy, wy, "luma")
    same_bits(gc, wc, "chroma")
    assert (gc[-1].reshape(H // 2, W // 2, 2)[~ok_c] == 128).all() and (gy[-1][~ok_l] == 0).all()
    assert (ob.outside(out) == POISON).all(), "bytes beyond W or between the planes were written"


@pytest.mark.parametrize("zoomed", [False, True])
def test_planes_narrower_than_a_tap_row(net, zoomed):
    """pw < 4: a row holds no 4-tap window, so the kernels take one clamped byte load per tap component.  RGB 5 x 3 and
    6 x 2; NV12 4 x 6 and 6 x 4, whose chroma planes are 2 x 3 and 3 x 2 (the luma plane of 6 x 4 is the narrowest that
    still takes the window).  F_t = 0 leaves valid pixels on every one of them."""
    n = 3
    view = net.view("bicubic")
    F = _dev(vectors(n))
    zoom = _dev(np.float32(ZOOM)) if zoomed else None
    for H, W in ((5, 3), (6, 2)):
        src_h = np.random.default_rng(H + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        T, f32, u8 = render_u8(view, F, _dev(src_h), 0, zoom, True, True, W, 0)
        xs, ys = grid(T, zoom, n, H, W)
        assert R.valid(H, W, xs[0], ys[0]).any()
        want = np.stack([R.render_f32(src_h[b], xs[b], ys[b]) for b in range(n)])
        same_bits(f32, want, "%dx%d out_f32" % (H, W))
        same_bits(u8, R.to_u8(want), "%dx%d out_u8" % (H, W))
    for H, W in ((4, 6), (6, 4)):
        b = nv12_ref.Batch(H * W, n, H, W, W + 3, H + 1)
        ob = nv12_ref.Batch(0, n, H, W, W + 5, H, fill=POISON)
        T, out = render_nv12(view, F, b, _dev(b.buf), ob, zoom)
        wy, wc, _, _ = nv12_reference(b, T, zoom)
        gy, gc = ob.planes(out)
        same_bits(gy, wy, "%dx%d luma" % (H, W))
        same_bits(gc, wc, "%dx%d chroma" % (H, W))
        assert (gy[0] != 0).any() and (gc[0] != 128).any()
        assert (ob.outside(out) == POISON).all()


def test_views_queries_T_and_bilinear_views(net):
    """T through a view is the parent's; a bilinear view renders the parent's bytes; the queries; a view of a view."""
    from coupe.dvsg_amd import _lib
    lib = _lib.load()
    n, H, W = 3, 12, 21
    src = _dev(np.random.default_rng(5).integers(0, 256, (n, H, W, 3), dtype=np.uint8))
    F = _dev(vectors(n))
    zoom = _dev(np.float32(ZOOM))
    cubic = net.view("bicubic")
    assert net.view("bicubic") is cubic and net.view("bilinear") is net.handle
    plain = ctypes.c_void_p()
    _call("dvsg_locnet_view_create", net.handle, 0, ctypes.byref(plain))
    nested = ctypes.c_void_p()
    _call("dvsg_locnet_view_create", cubic, 0, ctypes.byref(nested))       # a view of a view: of the parent, own filter
    try:
        assert [lib.dvsg_locnet_render_filter(h) for h in (net.handle, cubic, plain, nested)] == [0, 1, 0, 0]
        assert [lib.dvsg_locnet_in_channels(h) for h in (net.handle, cubic, plain, nested)] == [21] * 4
        T0, f0, u0 = render_u8(net.handle, F, src, 1, zoom, True, True, W, 0)
        for h, what in ((plain, "bilinear view"), (nested, "bilinear view of a bicubic view")):
            T1, f1, u1 = render_u8(h, F, src, 1, zoom, True, True, W, 0)
            same_bits(T1.cpu().numpy(), T0.cpu().numpy(), what + " T")
            same_bits(f1, f0, what + " out_f32")
            same_bits(u1, u0, what + " out_u8")
        T2, f2, _ = render_u8(cubic, F, src, 1, zoom, True, True, W, 0)
        same_bits(T2.cpu().numpy(), T0.cpu().numpy(), "bicubic view T")
        assert not np.array_equal(f2, f0), "the bicubic view must not render sampler A's values"
        b = nv12_ref.Batch(9, n, 10, 36, 48, 12)
        ob = nv12_ref.Batch(0, n, 10, 36, 40, 10, fill=POISON)
        buf = _dev(b.buf)
        Ta, oa = render_nv12(net.handle, F, b, buf, ob, None)
        Tb, obv = render_nv12(plain, F, b, buf, ob, None)
        same_bits(Tb.cpu().numpy(), Ta.cpu().numpy(), "NV12 T")
        same_bits(obv, oa, "NV12 bilinear view")
        # calibrating through a view is refused before anything runs
        ws = _torch().empty(1 << 10, dtype=_torch().uint8, device="cuda")
        assert lib.dvsg_locnet_calibrate_f16(cubic, None, 0, 0, 0, ws.data_ptr(), ws.numel(), None) == -1
        assert b"view" in lib.dvsg_last_error_string()
    finally:
        assert lib.dvsg_locnet_destroy(nested) == 0 and lib.dvsg_locnet_destroy(plain) == 0


def test_destroy_order(synthetic_weights):
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    lib = _lib.load()
    parent = LocNet(synthetic_weights)
    view = ctypes.c_void_p()
    _call("dvsg_locnet_view_create", parent.handle, 1, ctypes.byref(view))
    assert lib.dvsg_locnet_destroy(parent.handle) == -1                    # refused: nothing is destroyed
    assert b"view" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_in_channels(parent.handle) == 21 and lib.dvsg_locnet_render_filter(view) == 1
    F = _dev(vectors()[1:2])
    T = _torch().empty((1, 2, 28), device="cuda")
    _call("dvsg_tps_coefficients_f32", view, F.data_ptr(), 1, T.data_ptr(), _stream())   # the parent is still whole
    _torch().cuda.synchronize()
    assert np.isfinite(T.cpu().numpy()).all()
    assert lib.dvsg_locnet_destroy(view) == 0
    assert lib.dvsg_locnet_destroy(parent.handle) == 0
    parent.handle = None


def test_a_view_sees_its_parents_later_calibration(synthetic_weights):
    """A view resolves to its parent at call time: made BEFORE dvsg_locnet_calibrate_f16 of the parent, it runs the float16
    network on the re-rounded weights afterwards (the parent's F_t bit for bit, and not the F_t from before)."""
    from coupe.dvsg_amd.networks import LocNet
    torch = _torch()
    loc = LocNet(synthetic_weights)
    view = loc.view("bicubic")
    x = _dev(inputs.window_frames(3, 1, 64, 96))
    ws, nbytes = loc.workspace(1, 64, 96)

    def f16(handle):
        F = torch.empty((1, 25, 2), device="cuda")
        _call("dvsg_locnet_forward_f16", handle, x.data_ptr(), 1, 64, 96, F.data_ptr(), ws.data_ptr(), nbytes, _stream())
        torch.cuda.synchronize()
        return F.cpu().numpy()
    before = f16(view)
    same_bits(before, f16(loc.handle), "F_t before the calibration")
    loc.calibrate_f16(x)
    after = f16(view)
    same_bits(after, f16(loc.handle), "F_t after the calibration")
    assert not np.array_equal(after, before), "the calibration must move the float16 F_t"


def test_network_through_a_view_is_the_parents():
    """dvsg_stabilize_ring_inplace_f32 (B = 2, 38 x 54, skip (0, 2, 3), a 9-channel checkpoint) through a bicubic view: the
    parent's pool, F_t, x_s and y_s, bit for bit."""
    import test_gpu_pipe as pipe
    torch = _torch()
    model = pipe.model()
    loc = model.locnet
    B, (H, W) = 2, pipe.MODEL
    pool0 = _dev(inputs.smooth_frames(31, 10, H, W))
    table = _dev(np.int32([[0, 1, 2], [5, 6, 7]]))
    slots = _dev(np.int32([3, 8]))
    ws, nbytes = loc.workspace(B, H, W)
    got = []
    for handle in (loc.handle, loc.view("bicubic")):
        pool = pool0.clone()
        F = torch.empty((B, 25, 2), device="cuda")
        xs, ys = torch.empty((B, H, W), device="cuda"), torch.empty((B, H, W), device="cuda")
        _call("dvsg_stabilize_ring_inplace_f32", handle, 0, pool.data_ptr(), 10, table.data_ptr(), slots.data_ptr(), B, H, W,
              F.data_ptr(), xs.data_ptr(), ys.data_ptr(), ws.data_ptr(), nbytes, _stream())
        torch.cuda.synchronize()
        got.append([t.cpu().numpy() for t in (pool, F, xs, ys)])
    assert not np.array_equal(got[0][0], pool0.cpu().numpy())
    for a, b, what in zip(got[0], got[1], ("pool", "F_t", "x_s", "y_s")):
        same_bits(b, a, what)


def _online(fmt, render_filter, sizes):
    """Two streams of 6 frames at two source sizes through OnlineStabilizer(crop="auto"): per step the outputs, F_t and the
    zoom of every stream; then the pool and the crop states."""
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd.online import OnlineStabilizer
    torch = _torch()
    kw = dict(frame_format="nv12") if fmt == "nv12" else dict(source_res=True, as_uint8=True)
    on = OnlineStabilizer(pipe.model(), max_streams=2, skip_length=pipe.SKIP, crop="auto", render_filter=render_filter, **kw)
    if fmt == "nv12":
        clips = [nv12_ref.smooth_batch(800 + i, 6, *s).buf for i, s in enumerate(sizes)]
    else:
        clips = [(inputs.smooth_frames(810 + i, 6, *s) * 255).astype(np.uint8) for i, s in enumerate(sizes)]
    sids = [on.open(), on.open()]
    order = sorted(range(2), key=lambda i: sizes[i])       # a step's batch rows run by source size
    steps = []
    for k in range(6):
        outs = on.step({sid: clips[i][k] for i, sid in enumerate(sids)})
        F = on._F[:2].cpu().numpy()
        steps.append([(outs[sids[i]], F[order.index(i)], on.crop_state(sids[i])["zoom"]) for i in range(2)])
    torch.cuda.synchronize()
    return clips, steps, on.pool.cpu().numpy(), [on.crop_state(s) for s in sids], on.model.locnet


@pytest.mark.parametrize("fmt", ["nv12", "rgb"])
def test_online_stabilizer_end_to_end(fmt):
    """OnlineStabilizer(render_filter="bicubic", crop="auto"), NV12 and source_res + as_uint8: every output is the reference
    applied to the stabiliser's own F_t and zoom; the pool and the crop states are the bilinear run's."""
    sizes = [(64, 96), (20, 32)]
    clips, steps, pool, crop, loc = _online(fmt, "bicubic", sizes)
    _, steps_bl, pool_bl, crop_bl, _ = _online(fmt, "bilinear", sizes)
    same_bits(pool, pool_bl, "pool")
    assert crop == crop_bl
    moved = False
    for k in range(6):
        for i, (H0, W0) in enumerate(sizes):
            out, F, z = steps[k][i]
            same_bits(F, steps_bl[k][i][1], "F_t")
            assert z == steps_bl[k][i][2]
            moved = moved or not np.array_equal(out, steps_bl[k][i][0])
            Fd, T, zoom = _dev(F[None]), _torch().empty((1, 2, 28), device="cuda"), _dev(np.float32([z]))
            _call("dvsg_tps_coefficients_f32", loc.handle, Fd.data_ptr(), 1, T.data_ptr(), _stream())
            if fmt == "nv12":
                b = nv12_ref.Batch(0, 1, H0, W0)
                b.buf = clips[i][k][None]
                wy, wc, _, _ = nv12_reference(b, T, zoom)
                same_bits(out[:H0], wy[0], "step %d stream %d luma" % (k, i))
                same_bits(out[H0:], wc[0], "step %d stream %d chroma" % (k, i))
            else:
                xs, ys = grid(T, zoom, 1, H0, W0)
                same_bits(out, R.to_u8(R.render_f32(clips[i][k], xs[0], ys[0])), "step %d stream %d" % (k, i))
    assert moved, "the two filters must differ somewhere"


def test_pipes_take_the_option():
    """stabilize_pipes with one Y4M source and render_filter="bicubic" writes the bytes of stabilize_clips with the option."""
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd import y4m
    from coupe.dvsg_amd.online import stabilize_clips
    clip, i420 = pipe.clips()["single"][:6], pipe.clips()["single_i420"][:6]
    want = stabilize_clips(pipe.model(), [clip], frame_format="nv12", skip_length=pipe.SKIP,
                           yuv_matrix=y4m.default_yuv_matrix(pipe.BIG[0]), render_filter="bicubic")[0]
    out = io.BytesIO()
    src = y4m.Y4MReader(io.BytesIO(pipe.y4m_bytes(i420)))
    pipe.run([src], [y4m.Y4MWriter(out, src.width, src.height, src.fps)], render_filter="bicubic")
    got, _ = pipe.nv12_frames_of_y4m(out.getvalue())
    pipe.same(got, want, "the one source, bicubic")
    plain = stabilize_clips(pipe.model(), [clip], frame_format="nv12", skip_length=pipe.SKIP,
                            yuv_matrix=y4m.default_yuv_matrix(pipe.BIG[0]))[0]
    assert not np.array_equal(want, plain)


def test_bicubic_is_sharper(net):
    """One case: a 24 x 96 NV12 frame whose luma is 0.5 + 0.4 sin(2 pi x / 6) in every row, F_t = all 25 points displaced by
    5 / 96 in x (a pure translation worth 2.5 source pixels, the worst phase for a 4-tap blend).  Both filters' luma against
    the analytically shifted signal over the pixels valid in both: bicubic's mean absolute error is the smaller, no margin.
    On the two NumPy references alone (tests/test_bicubic_cpu.py) the figures are 0.0066 against 0.0229, i.e. 1.5 % amplitude
    overshoot against 8.5 % amplitude loss."""
    import test_bicubic_cpu as cpu
    plane, _, _, sig, d = cpu.sharpness_case()
    H, W = plane.shape[:2]
    b = nv12_ref.Batch(0, 1, H, W, fill=128)
    b.buf[0, :H] = plane[..., 0]
    F = np.zeros((1, 25, 2), np.float32)
    F[..., 0] = d
    buf, Fd = _dev(b.buf), _dev(F)
    ob = nv12_ref.Batch(0, 1, H, W, fill=POISON)
    T, out_bc = render_nv12(net.view("bicubic"), Fd, b, buf, ob, None)
    _, out_bl = render_nv12(net.handle, Fd, b, buf, ob, None)
    xs, ys = grid(T, None, 1, H, W)
    ok = R.valid(H, W, xs[0], ys[0])
    x, _ = R.coords(H, W, xs[0], ys[0])
    assert ok.sum() > 2000 and np.abs(x[ok] - (np.arange(W)[None] * W / (W - 1.0) + 2.5).repeat(H, 0)[ok]).max() < 1e-2
    truth = sig(x.astype(np.float64))
    e_bc = np.abs(out_bc[0, :H] / 255.0 - truth)[ok].mean()
    e_bl = np.abs(out_bl[0, :H] / 255.0 - truth)[ok].mean()
    print("mean |error|: bicubic %.5f bilinear %.5f" % (e_bc, e_bl))
    assert e_bc < e_bl
