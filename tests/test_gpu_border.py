"""GPU: the border modes of the four source-size renders (include/dvsg_amd.h, "Border modes") against their NumPy restatement
tests/border_ref.py.  Valid samples are the DVSG_BORDER_BLACK render's, bit for bit; invalid ones are the restatement's, byte
for byte and -- out_f32 -- bit for bit, no sample masked or left out.  x_s, y_s come from the grid-only form of
dvsg_tps_warp_zoom_f32 at each plane's size, as the header defines them.  Every render writes into PRE-FILLED outputs (seeded
bytes, floats in [2, 3)), so what "keep" leaves and what no mode may touch are both visible.  Synthetic weights, f32.

Shapes: RGB 7 x 10, 16 x 24, 1 x 5 and 5 x 515 (three 256-column tiles, the last one partial); NV12 8 x 12, 4 x 4 (a 2 x 2 chroma
plane: the byte-tap path), 16 x 20 (pitch 32, the UV plane three rows behind the luma, out_pitch > W) and 10 x 520 (pitch 528:
luma over three column tiles, chroma over two, both planes end in a partial 4-row tile).  Each test asserts about its own inputs that every side of every plane has a
full row or column of invalid samples in some frame, and that at least a quarter of all its samples (all shapes, planes and
frames of the launch) are valid.  The quarter is taken over the test's inputs as a whole: a plane with ph == 1 (RGB 1 x 5) has no
valid sample by the header's rule and the 2 x 2 chroma plane has at most one per frame, so neither can hold it alone."""
import ctypes
import io

import numpy as np
import pytest

import bicubic_ref as R
import border_ref as BR
import inputs
import nv12_ref
import test_gpu_bicubic as B

pytestmark = pytest.mark.gpu

RGB_SHAPES = ((7, 10), (16, 24), (1, 5), (5, 515))
NV12_SHAPES = ((8, 12, 12, 8, 12), (4, 4, 4, 4, 4), (16, 20, 32, 19, 28), (10, 520, 528, 11, 524))    # H, W, pitch, uv_row, out_pitch
ZOOM = (1.0, 0.8, 0.6)
BORDERS = ("replicate", "mirror", "keep")
FILTERS = ("bilinear", "bicubic")
U8_PAD, U8_X0 = 3, 2
_CACHE = {}

_dev, _call, _stream, grid, same_bits = B._dev, B._call, B._stream, B.grid, B.same_bits


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def net(synthetic_weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def vectors(kind):
    """F_t of a launch of three frames.  "launch": uniform (+0.4, +0.4), uniform (-0.4, -0.4), per-point random in +-0.25;
    "turned": the same frames in another order (another valid set per frame); "far": uniform (-2.5, +2.5), where the clamp
    behind the one reflection is reached; "nan": "launch" with one NaN component in frame 1."""
    F = np.zeros((3, 25, 2), np.float32)
    if kind == "far":
        F[..., 0], F[..., 1] = -2.5, 2.5
        return F
    F[0], F[1] = 0.4, -0.4
    F[2] = np.random.default_rng(41).uniform(-0.25, 0.25, (25, 2))
    if kind == "turned":
        F = np.ascontiguousarray(F[[2, 0, 1]])
    if kind == "nan":
        F[1, 7, 0] = np.nan
    return F


def _guarded(a):
    import test_conv_gemm_f64 as f64
    return f64.Guarded.of(_dev(a))


# ---------------------------------------------------------------------------------------------------------------------
# one launch of each format into pre-filled outputs -> T and the outputs as NumPy
# ---------------------------------------------------------------------------------------------------------------------
def rgb_source(H, W):
    return np.random.default_rng(100 * H + W).integers(0, 256, (3, H, W, 3), dtype=np.uint8)


def rgb_prefill(H, W, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(2.0, 3.0, (3, H, W, 3)).astype(np.float32),
            rng.integers(0, 256, (3, H, W + U8_PAD, 3), dtype=np.uint8))


def rgb_render(handle, F, src, flip, zoom, pre):
    torch = _torch()
    n, H, W = src.shape[:3]
    T = torch.empty((n, 2, 28), device="cuda")
    gf, gu = _guarded(pre[0]), _guarded(pre[1])
    Fd, srcd = _dev(F), _dev(src)      # (held until the launch has run)
    args = [handle, Fd.data_ptr(), srcd.data_ptr(), n, H, W, flip]
    if zoom is not None:
        args.append(zoom.data_ptr())
    args += [T.data_ptr(), gf.ptr(), gu.ptr(), W + U8_PAD, U8_X0, _stream()]
    _call("dvsg_tps_render_zoom_u8" if zoom is not None else "dvsg_tps_render_u8", *args)
    torch.cuda.synchronize()
    assert gf.intact() and gu.intact(), "a guard byte was written"
    return T, gf.view(torch.float32, pre[0].shape).cpu().numpy(), gu.view(torch.uint8, pre[1].shape).cpu().numpy()


def nv12_source(H, W, pitch, uv_row):
    return nv12_ref.Batch(H * 31 + W, 3, H, W, pitch, uv_row)


def nv12_prefill(H, W, uv_row, out_pitch, seed=2):
    return nv12_ref.Batch(seed + H, 3, H, W, out_pitch, uv_row)


def nv12_render(handle, F, b, zoom, pre):
    torch = _torch()
    T = torch.empty((b.n, 2, 28), device="cuda")
    buf, g, Fd = _dev(b.buf), _guarded(pre.buf), _dev(F)
    args = [handle, Fd.data_ptr(), buf.data_ptr(), buf.data_ptr() + b.uv_offset, b.pitch, b.frame_stride, b.n, b.H, b.W]
    if zoom is not None:
        args.append(zoom.data_ptr())
    args += [T.data_ptr(), g.ptr(), g.ptr() + pre.uv_offset, pre.pitch, pre.frame_stride, _stream()]
    _call("dvsg_tps_render_zoom_nv12" if zoom is not None else "dvsg_tps_render_nv12", *args)
    torch.cuda.synchronize()
    assert g.intact(), "a guard byte was written"
    return T, g.view(torch.uint8, pre.buf.shape).cpu().numpy()


def _zoom(zoomed):
    return _dev(np.float32(ZOOM)) if zoomed else None


def check_inputs(masks):
    """masks: the validity [n, ph, pw] of every plane of a test's three-frame launches"""
    for ok in masks:
        bad = ~ok
        sides = (bad[:, 0, :].all(axis=1), bad[:, -1, :].all(axis=1), bad[:, :, 0].all(axis=1), bad[:, :, -1].all(axis=1))
        assert all(s.any() for s in sides), "plane %s: a side has no fully invalid row / column in any frame" % (ok.shape,)
    total, good = sum(ok.size for ok in masks), sum(int(ok.sum()) for ok in masks)
    assert 4 * good >= total, "%d of %d samples valid" % (good, total)


def expected(plane, xs, ys, border, bicubic, chroma, before_f32, before_u8, flip=0):
    """what a render leaves in a pre-filled plane: (float32 values or None, bytes), from the restatement"""
    n = len(plane)
    f, u = [], []
    for i in range(n):
        v, written = BR.render(plane[i], xs[i], ys[i], border, bicubic, chroma)
        w = written[..., None]
        if before_f32 is not None:
            f.append(np.where(w, v[..., ::-1] if flip else v, before_f32[i]))
        u.append(np.where(w, BR.to_u8(v, bicubic, chroma), before_u8[i]))
    return (np.stack(f) if before_f32 is not None else None), np.stack(u)


def compare(got, black, want, ok, what):
    """valid samples: the BLACK render's bits; invalid ones: the restatement's"""
    same_bits(got[ok], black[ok], what + ", valid samples against DVSG_BORDER_BLACK")
    same_bits(got[~ok], want[~ok], what + ", invalid samples against border_ref")


# ---------------------------------------------------------------------------------------------------------------------
# 1. every border against both filters, all four entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("border", BORDERS)
def test_rgb_borders(net, border, filt, zoomed):
    """dvsg_tps_render_u8 / dvsg_tps_render_zoom_u8: out_f32 and out_u8 (columns [2, 2 + W) of rows of W + 3 pixels; 16 x 24 with
    channel_flip), for the three-frame launch, the far launch and the launch with a NaN."""
    bicubic = filt == "bicubic"
    view, plain = net.view(filt, border), net.view(filt, "black")
    zoom = _zoom(zoomed)
    masks = []
    for H, W in RGB_SHAPES:
        src, pre = rgb_source(H, W), rgb_prefill(H, W)
        flip = 1 if (H, W) == (16, 24) else 0
        cols = np.s_[:, :, U8_X0:U8_X0 + W]
        for kind in ("launch", "far", "nan"):
            F = vectors(kind)
            T, f32, u8 = rgb_render(view, F, src, flip, zoom, pre)
            key = ("rgb", H, W, filt, zoomed, kind)
            if key not in _CACHE:
                _, bf, bu = rgb_render(plain, F, src, flip, zoom, pre)
                xs, ys = grid(T, zoom, 3, H, W)
                _CACHE[key] = (bf, bu, xs, ys, np.stack([R.valid(H, W, xs[i], ys[i]) for i in range(3)]))
            bf, bu, xs, ys, ok = _CACHE[key]
            if kind == "launch":
                masks.append(ok)
            elif kind == "far":
                assert not ok.any()
            else:
                assert np.isnan(xs[1]).all() and not ok[1].any() and ok[0].any() == (H > 1)
            wf, wu = expected(src, xs, ys, border, bicubic, False, pre[0], pre[1][cols], flip)
            what = "%s %s %dx%d %s zoom=%d" % (border, filt, H, W, kind, zoomed)
            compare(f32, bf, wf, ok, what + " out_f32")
            compare(u8[cols], bu[cols], wu, ok, what + " out_u8")
            rest = np.delete(u8, np.s_[U8_X0:U8_X0 + W], axis=2)
            assert np.array_equal(rest, np.delete(pre[1], np.s_[U8_X0:U8_X0 + W], axis=2)), what + ": columns outside were written"
            if kind == "nan" and border != "keep":
                assert (f32[1] == 0).all() and (u8[cols][1] == 0).all(), what + ": a NaN coordinate gives black"
            if kind == "far" and border != "keep" and H > 1:
                assert (u8[cols] != 0).any(), what + ": the far launch is filled from the source's edge"
    check_inputs(masks)


def _nv12_planes(b, buf=None):
    y, uv = b.planes(buf)
    return y[..., None], uv.reshape(b.n, b.H // 2, b.W // 2, 2)


@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("border", BORDERS)
def test_nv12_borders(net, border, filt, zoomed):
    """dvsg_tps_render_nv12 / dvsg_tps_render_zoom_nv12: both planes, each on its own validity; the bytes of the output buffer that
    belong to neither plane (pitch padding, the rows between the planes) stay as they were."""
    bicubic = filt == "bicubic"
    view, plain = net.view(filt, border), net.view(filt, "black")
    zoom = _zoom(zoomed)
    masks = []
    for H, W, pitch, uv_row, out_pitch in NV12_SHAPES:
        b, pre = nv12_source(H, W, pitch, uv_row), nv12_prefill(H, W, uv_row, out_pitch)
        src = _nv12_planes(b)
        before = _nv12_planes(pre)
        for kind in ("launch", "far", "nan"):
            F = vectors(kind)
            T, out = nv12_render(view, F, b, zoom, pre)
            key = ("nv12", H, W, filt, zoomed, kind)
            if key not in _CACHE:
                _, bo = nv12_render(plain, F, b, zoom, pre)
                g = [grid(T, zoom, 3, H, W), grid(T, zoom, 3, H // 2, W // 2)]
                ok = [np.stack([R.valid(ph, pw, x[i], y[i]) for i in range(3)]) for (x, y), (ph, pw) in zip(g, ((H, W), (H // 2, W // 2)))]
                _CACHE[key] = (bo, g, ok)
            bo, g, ok = _CACHE[key]
            if kind == "launch":
                masks += ok
            got, black = _nv12_planes(pre, out), _nv12_planes(pre, bo)
            for p, name in enumerate(("luma", "chroma")):
                _, want = expected(src[p], g[p][0], g[p][1], border, bicubic, p == 1, None, before[p])
                what = "%s %s %dx%d %s zoom=%d %s" % (border, filt, H, W, kind, zoomed, name)
                compare(got[p], black[p], want, ok[p], what)
                if kind == "nan" and border != "keep":
                    assert (got[p][1] == (128 if p else 0)).all(), what + ": a NaN coordinate gives black"
            assert np.array_equal(pre.outside(out), pre.outside()), "bytes beyond W or between the planes were written"
    check_inputs(masks)


# ---------------------------------------------------------------------------------------------------------------------
# 2. keep: a second render into the same output; the zoomed entry at zoom 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_keep_renders_twice_into_one_output(net, filt):
    """Two launches into one pre-filled output, the second with the frames' F_t in another order: after it, a sample invalid
    in the second launch holds what the first left there (its render where that was valid, else the pre-fill), and the padding
    holds the pre-fill."""
    view, plain = net.view(filt, "keep"), net.view(filt, "black")
    masks = []
    H, W = 16, 24
    src, pre = rgb_source(H, W), rgb_prefill(H, W, seed=9)
    cols = np.s_[:, :, U8_X0:U8_X0 + W]
    state = pre
    for kind in ("launch", "turned"):
        F = vectors(kind)
        T, f32, u8 = rgb_render(view, F, src, 0, None, state)
        _, bf, bu = rgb_render(plain, F, src, 0, None, state)
        xs, ys = grid(T, None, 3, H, W)
        ok = np.stack([R.valid(H, W, xs[i], ys[i]) for i in range(3)])
        masks.append(ok)
        same_bits(f32, np.where(ok[..., None], bf, state[0]), "rgb %s out_f32" % kind)
        wu = state[1].copy()
        wu[cols] = np.where(ok[..., None], bu[cols], state[1][cols])
        same_bits(u8, wu, "rgb %s out_u8 and its padding" % kind)
        state = (f32, u8)
    first, second = masks
    assert (first & ~second).any() and (~first & ~second).any(), "the second launch must leave both kinds of earlier bytes"
    H, W, pitch, uv_row, out_pitch = NV12_SHAPES[2]
    b, pre = nv12_source(H, W, pitch, uv_row), nv12_prefill(H, W, uv_row, out_pitch, seed=9)
    for kind in ("launch", "turned"):
        F = vectors(kind)
        T, out = nv12_render(view, F, b, None, pre)
        _, bo = nv12_render(plain, F, b, None, pre)
        want = pre.buf.copy()
        for p, (ph, pw) in enumerate(((H, W), (H // 2, W // 2))):
            xs, ys = grid(T, None, 3, ph, pw)
            ok = np.stack([R.valid(ph, pw, xs[i], ys[i]) for i in range(3)])
            masks.append(ok)
            w, k = _nv12_planes(pre, want)[p], _nv12_planes(pre, bo)[p]    # views of `want` and of the black render
            w[ok] = k[ok]
        same_bits(out, want, "nv12 %s, planes and padding" % kind)
        pre = nv12_ref.Batch(0, 3, H, W, out_pitch, uv_row)
        pre.buf = out
    check_inputs(masks)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", FILTERS)
def test_zoom_one_is_the_plain_entry(net, filt, border):
    view = net.view(filt, border)
    ones = _dev(np.ones(3, np.float32))
    F = vectors("launch")
    H, W = 7, 10
    src, pre = rgb_source(H, W), rgb_prefill(H, W)
    T0, f0, u0 = rgb_render(view, F, src, 1, None, pre)
    T1, f1, u1 = rgb_render(view, F, src, 1, ones, pre)
    same_bits(T1.cpu().numpy(), T0.cpu().numpy(), "T")
    same_bits(f1, f0, "out_f32")
    same_bits(u1, u0, "out_u8")
    xs, ys = grid(T0, None, 3, H, W)
    masks = [np.stack([R.valid(H, W, xs[i], ys[i]) for i in range(3)])]
    H, W, pitch, uv_row, out_pitch = NV12_SHAPES[0]
    b, pre = nv12_source(H, W, pitch, uv_row), nv12_prefill(H, W, uv_row, out_pitch)
    T0, o0 = nv12_render(view, F, b, None, pre)
    _, o1 = nv12_render(view, F, b, ones, pre)
    same_bits(o1, o0, "nv12")
    for ph, pw in ((H, W), (H // 2, W // 2)):
        xs, ys = grid(T0, None, 3, ph, pw)
        masks.append(np.stack([R.valid(ph, pw, xs[i], ys[i]) for i in range(3)]))
    check_inputs(masks)


# ---------------------------------------------------------------------------------------------------------------------
# 3. views
# ---------------------------------------------------------------------------------------------------------------------
def test_views_with_border_zero_and_the_query(net):
    """..._border(f, 0) renders the bytes of dvsg_locnet_view_create(f); dvsg_locnet_render_border reports each view's value,
    nested views (a view of a view: of the parent, nothing inherited) included; LocNet.view caches per pair."""
    from coupe.dvsg_amd import _lib
    lib = _lib.load()
    assert net.view("bilinear", "black") is net.handle and net.view("bicubic", "mirror") is net.view("bicubic", "mirror")
    assert net.view("bicubic", "black") is net.view("bicubic") and net.view("bicubic", "mirror") is not net.view("bilinear", "mirror")
    made = []

    def make(parent, f, border=None):
        v = ctypes.c_void_p()
        if border is None:
            _call("dvsg_locnet_view_create", parent, f, ctypes.byref(v))
        else:
            _call("dvsg_locnet_view_create_border", parent, f, border, ctypes.byref(v))
        made.append(v)
        return v
    try:
        mirror = make(net.handle, 1, 2)
        nested_plain = make(mirror, 0)              # a view of a view through the old constructor: border 0
        nested_keep = make(mirror, 0, 3)
        nested_of_nested = make(nested_keep, 1, 1)
        handles = (net.handle, None, mirror, nested_plain, nested_keep, nested_of_nested, net.view("bicubic"))
        assert [lib.dvsg_locnet_render_border(h) for h in handles] == [0, 0, 2, 0, 3, 1, 0]
        assert [lib.dvsg_locnet_render_filter(h) for h in handles] == [0, 0, 1, 0, 0, 1, 1]
        assert [lib.dvsg_locnet_in_channels(h) for h in handles if h is not None] == [21] * 6
        F = vectors("launch")
        H, W = 16, 24
        src, pre = rgb_source(H, W), rgb_prefill(H, W)
        b, npre = nv12_source(*NV12_SHAPES[2][:4]), nv12_prefill(16, 20, 19, 28)
        for f in (0, 1):
            old, new = make(net.handle, f), make(mirror, f, 0)
            T0, f0, u0 = rgb_render(old, F, src, 0, _zoom(True), pre)
            T1, f1, u1 = rgb_render(new, F, src, 0, _zoom(True), pre)
            same_bits(T1.cpu().numpy(), T0.cpu().numpy(), "T")
            same_bits(f1, f0, "filter %d out_f32" % f)
            same_bits(u1, u0, "filter %d out_u8" % f)
            same_bits(nv12_render(new, F, b, None, npre)[1], nv12_render(old, F, b, None, npre)[1], "filter %d nv12" % f)
        # the nested views render like views of the parent with the same pair
        _, fa, ua = rgb_render(nested_keep, F, src, 0, None, pre)
        _, fb, ub = rgb_render(net.view("bilinear", "keep"), F, src, 0, None, pre)
        same_bits(fa, fb, "nested keep out_f32")
        same_bits(ua, ub, "nested keep out_u8")
        ws = _torch().empty(1 << 10, dtype=_torch().uint8, device="cuda")
        assert lib.dvsg_locnet_calibrate_f16(mirror, None, 0, 0, 0, ws.data_ptr(), ws.numel(), None) == -1
        assert b"view" in lib.dvsg_last_error_string()
    finally:
        for v in made:
            assert lib.dvsg_locnet_destroy(v) == 0


def test_destroying_a_parent_with_a_border_view_is_refused(synthetic_weights):
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    lib = _lib.load()
    parent = LocNet(synthetic_weights)
    view = ctypes.c_void_p()
    _call("dvsg_locnet_view_create_border", parent.handle, 0, 3, ctypes.byref(view))
    assert lib.dvsg_locnet_destroy(parent.handle) == -1
    assert b"view" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_render_border(view) == 3
    assert lib.dvsg_locnet_destroy(view) == 0
    assert lib.dvsg_locnet_destroy(parent.handle) == 0
    parent.handle = None


# ---------------------------------------------------------------------------------------------------------------------
# 4. OnlineStabilizer
# ---------------------------------------------------------------------------------------------------------------------
SIZES = ((44, 60), (40, 58))      # a little larger than the 38 x 54 model; two sizes in one step
STEPS = 4


def _clip(fmt, i, n=STEPS, sizes=SIZES):
    if fmt == "nv12":
        return nv12_ref.smooth_batch(900 + i, n, *sizes[i]).buf
    return (inputs.smooth_frames(910 + i, n, *sizes[i]) * 255).astype(np.uint8)


def _online(fmt, border, filt, events=(), crop=None, as_uint8=True, scene=None, clips=None, sizes=SIZES):
    """Two streams (one per size) through OnlineStabilizer for STEPS steps: per step every stream's output, F_t and zoom; then
    the pool and the crop state.  events: {step: "reset"} applies reset() to stream 0 before that step."""
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd.online import OnlineStabilizer
    kw = dict(frame_format="nv12") if fmt == "nv12" else dict(source_res=True, as_uint8=as_uint8)
    if scene is not None:
        kw.update(scene_cut=scene)
    on = OnlineStabilizer(pipe.model(), max_streams=2, skip_length=pipe.SKIP, crop=crop, render_filter=filt, border=border, **kw)
    clips = clips or [_clip(fmt, 0, sizes=sizes), _clip(fmt, 1, sizes=sizes)]
    sids = [on.open(), on.open()]
    order = sorted(range(2), key=lambda i: sizes[i])      # (stable: equal sizes keep the streams' order)
    steps = []
    for k in range(len(clips[0])):
        if dict(events).get(k) == "reset":
            on.reset(sids[0])
        outs = on.step({sid: clips[i][k] for i, sid in enumerate(sids)})
        F = on._F[:2].cpu().numpy()
        z = [on.crop_state(s)["zoom"] if crop is not None else None for s in sids]
        steps.append([(outs[sids[i]].copy(), F[order.index(i)], z[i]) for i in range(2)])
    _torch().cuda.synchronize()
    state = (on.pool.cpu().numpy(), on._F.cpu().numpy(), None if crop is None else on._crop_zoom.cpu().numpy())
    return clips, steps, state


def _valid_planes(fmt, F, z, H0, W0):
    """validity of every plane of one frame rendered with F_t and zoom z: [(ok, rows, C)] -- luma / chroma rows of the surface"""
    import test_gpu_pipe as pipe
    torch = _torch()
    Fd, T = _dev(F[None]), torch.empty((1, 2, 28), device="cuda")
    _call("dvsg_tps_coefficients_f32", pipe.model().locnet.handle, Fd.data_ptr(), 1, T.data_ptr(), _stream())
    zoom = None if z is None else _dev(np.float32([z]))
    out = []
    for ph, pw in (((H0, W0), (H0 // 2, W0 // 2)) if fmt == "nv12" else ((H0, W0),)):
        xs, ys = grid(T, zoom, 1, ph, pw)
        out.append(R.valid(ph, pw, xs[0], ys[0]))
    return out


def _merge(fmt, ok, new, old):
    """where(valid, new, old) on a frame in its own layout"""
    if fmt != "nv12":
        return np.where(ok[0][..., None], new, old)
    H0 = ok[0].shape[0]
    out = old.copy()
    out[:H0] = np.where(ok[0], new[:H0], old[:H0])
    c = np.repeat(ok[1], 2, axis=1)
    out[H0:] = np.where(c, new[H0:], old[H0:])
    return out


@pytest.mark.parametrize("fmt", ["nv12", "rgb"])
@pytest.mark.parametrize("border", BORDERS)
def test_online_sequences_share_the_recurrence(fmt, border):
    """Each border against border="black" over a few steps, with crop="auto" and without crop: the pool, _F and the crop state
    are equal, and the outputs agree on every valid sample.  Without crop some invalid sample differs (the last row and column
    are invalid at any F_t); with it the zoom may have removed them all.  (bicubic for nv12, bilinear for rgb: both filters run.)"""
    filt = "bicubic" if fmt == "nv12" else "bilinear"
    for crop in ("auto", None):
        key = ("online", fmt, filt, crop)
        if key not in _CACHE:
            _CACHE[key] = _online(fmt, "black", filt, crop=crop)
        _, base, state0 = _CACHE[key]
        _, steps, state = _online(fmt, border, filt, crop=crop)
        for a, b, what in zip(state, state0, ("pool", "_F", "crop zoom")):
            if a is not None:
                same_bits(a, b, what)
        differ = False
        for k in range(STEPS):
            for i, (H0, W0) in enumerate(SIZES):
                out, F, z = steps[k][i]
                same_bits(F, base[k][i][1], "F_t")
                assert z == base[k][i][2]
                ok = _valid_planes(fmt, F, z, H0, W0)
                assert ok[0].any()
                same_bits(_merge(fmt, ok, out, base[k][i][0]), base[k][i][0], "crop=%s step %d stream %d: valid samples" % (crop, k, i))
                differ = differ or not np.array_equal(out, base[k][i][0])
        assert differ or crop is not None, "border=%r must change some invalid sample" % border


def _keep_expectation(fmt, clips, base, restarts, sizes=SIZES):
    """out_k = where(valid_k, black_k, out_{k-1}) per stream, out_{-1} (and after a restart at k) the source bytes of frame k"""
    want = []
    prev = [None, None]
    for k in range(len(base)):
        row = []
        for i, (H0, W0) in enumerate(sizes):
            black, F, z = base[k][i]
            if prev[i] is None or (i == 0 and k in restarts):
                prev[i] = clips[i][k]
            ok = _valid_planes(fmt, F, z, H0, W0)
            prev[i] = _merge(fmt, ok, black, prev[i])
            row.append(prev[i])
        want.append(row)
    return want


@pytest.mark.parametrize("fmt", ["nv12", "rgb"])
def test_keep_across_steps_and_after_reset(fmt):
    """Two streams of different source sizes in one step keep separate surfaces; step k's output is where(valid_k, black render_k,
    out_{k-1}) with out_{-1} the source bytes of step 0, and again from the frame that follows reset(sid)."""
    for events in ((), ((2, "reset"),)):
        clips, base, _ = _online(fmt, "black", "bilinear", events)
        _, steps, _ = _online(fmt, "keep", "bilinear", events)
        want = _keep_expectation(fmt, clips, base, {k for k, _ in events})
        carried = False
        for k in range(STEPS):
            for i in range(2):
                same_bits(steps[k][i][0], want[k][i], "events %s step %d stream %d" % (events, k, i))
                if k > 0:
                    ok = _valid_planes(fmt, steps[k][i][1], None, *SIZES[i])
                    carried = carried or not np.array_equal(_merge(fmt, ok, steps[k][i][0], clips[i][k]), steps[k][i][0])
        assert carried, "some invalid sample must show an earlier frame, not its own source"


@pytest.mark.parametrize("fmt", ["nv12", "rgb"])
def test_keep_two_streams_of_one_size_share_a_launch(fmt):
    """Two streams of ONE source size are rendered by one launch of two frames, into a stacked copy of their surfaces that is
    stored back: the outputs are the same recurrence per stream, through a reset of stream 0."""
    sizes, events = (SIZES[0], SIZES[0]), ((2, "reset"),)
    clips, base, _ = _online(fmt, "black", "bilinear", events, sizes=sizes)
    _, steps, _ = _online(fmt, "keep", "bilinear", events, sizes=sizes)
    want = _keep_expectation(fmt, clips, base, {2}, sizes)
    assert not np.array_equal(clips[0], clips[1])
    for k in range(STEPS):
        for i in range(2):
            same_bits(steps[k][i][0], want[k][i], "step %d stream %d" % (k, i))


def test_keep_float_output_restarts_from_the_source_over_255():
    clips, base, _ = _online("rgb", "black", "bilinear", as_uint8=False)
    _, steps, _ = _online("rgb", "keep", "bilinear", as_uint8=False)
    first = [c.astype(np.float32) / np.float32(255) for c in clips]
    want = _keep_expectation("rgb", first, base, set())
    for k in range(STEPS):
        for i in range(2):
            assert steps[k][i][0].dtype == np.float32
            same_bits(steps[k][i][0], want[k][i], "step %d stream %d" % (k, i))


@pytest.mark.parametrize("kind", ["u8_source_res", "nv12"])
def test_keep_restarts_at_a_device_detected_cut(synthetic_weights, kind):
    """Scene A then scene B through one stream with scene_cut (the clips of tests/test_gpu_scene.py): from the cut frame on the
    outputs are those of a fresh border="keep" stream fed B alone -- the old scene's bytes are gone -- and before it those of a
    stream without scene_cut."""
    import test_gpu_scene as scene
    from coupe.dvsg_amd.online import OnlineStabilizer
    A, Bc, kw = scene._clips(kind, n=4)
    if kind == "u8_source_res":
        kw = dict(kw, as_uint8=True)
    model = scene._model(synthetic_weights, 32, 48)
    on = OnlineStabilizer(model, scene_cut=scene.THR, border="keep", **kw)
    off = OnlineStabilizer(model, border="keep", **kw)
    fresh = OnlineStabilizer(model, border="keep", **kw)
    s_on, s_off, s_fresh = on.open(), off.open(), fresh.open()
    got = scene._push_all(on, s_on, np.concatenate([A, Bc]))
    assert on.scene_state(s_on)["cuts"] == 1
    scene._same(got[:4], scene._push_all(off, s_off, A), "scene A against scene_cut=None")
    scene._same(got[4:], scene._push_all(fresh, s_fresh, Bc), "scene B against a fresh stream")
    carried = off.push(s_off, Bc[0])
    assert carried.tobytes() != got[4].tobytes(), "without the restart the cut frame's border shows scene A"


def test_pipes_give_the_same_bytes_at_depth_1_and_3():
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd import y4m
    from coupe.dvsg_amd.online import stabilize_clips
    i420 = pipe.clips()["single_i420"][:5]
    got = []
    for depth in (1, 3):
        out = io.BytesIO()
        src = y4m.Y4MReader(io.BytesIO(pipe.y4m_bytes(i420)))
        pipe.run([src], [y4m.Y4MWriter(out, src.width, src.height, src.fps)], depth=depth, border="mirror")
        got.append(pipe.nv12_frames_of_y4m(out.getvalue())[0])
    pipe.same(got[0], got[1], "depth 1 against depth 3")
    want = stabilize_clips(pipe.model(), [pipe.clips()["single"][:5]], frame_format="nv12", skip_length=pipe.SKIP,
                           yuv_matrix=y4m.default_yuv_matrix(pipe.BIG[0]), border="mirror")[0]
    pipe.same(got[1], want, "stabilize_pipes against stabilize_clips")
    assert not np.array_equal(want, pipe.reference("single")[0][:5]), "mirror must differ from black"
