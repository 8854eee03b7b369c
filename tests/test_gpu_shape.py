"""GPU: warp shaping (include/dvsg_amd.h, "Warp shaping").  The contract is an identity: an entry point given a shaped view and
F_t writes and uses what it would if given the unshaped view of the same filter and border and F' = tests/shape_ref.py's
restatement of the rule on F_t -- T, every output byte and float, bit for bit, nothing masked.  So every case here runs the
entry point twice, once through the shaped view on F and once through the unshaped view on shape_ref(F), into outputs that
were filled with the same seeded bytes behind guards.  Synthetic weights, f32.

F is three frames of uniform +-0.05 (seeded, distinct per frame); the NaN cases use a copy with one NaN in frame 1.  Sizes: RGB
6 x 10 and 1 x 5, NV12 4 x 4, NV12 8 x 12 with pitch 16, the UV plane one row behind the luma and an output pitch of 20."""
import ctypes
import gc
import io

import numpy as np
import pytest

import bicubic_ref as R
import nv12_ref
import ratchet_ref
import shape_ref as S
import test_gpu_bicubic as B
import test_gpu_border as Bd

pytestmark = pytest.mark.gpu

SETS = (("affine", 0.5, 0.0), ("affine", 1.0, 1.0), ("similarity", 0.25, 0.75), ("translation", 1.0, 1.0), ("affine", 0.0, 0.0))
SET_IDS = ["%s-%g-%g" % s for s in SETS]
LOOKS = (("bilinear", "black"), ("bicubic", "mirror"), ("bilinear", "keep"))
RGB_SHAPES = ((6, 10), (1, 5))
NV12_SHAPES = ((4, 4, 4, 4, 4), (8, 12, 16, 9, 20))     # H, W, pitch, uv_row, out_pitch
ZOOM = 0.8
_CACHE = {}

_dev, _call, _stream, grid, same_bits = B._dev, B._call, B._stream, B.grid, B.same_bits


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def net(synthetic_weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def vectors(nan=False):
    F = np.random.default_rng(2024).uniform(-0.05, 0.05, (3, 25, 2)).astype(np.float32)
    if nan:
        F[1, 7, 0] = np.nan
    return F


def shaped_F(shape, nan=False):
    """shape_ref of the test's F, once per set"""
    key = ("F'", shape, nan)
    if key not in _CACHE:
        _CACHE[key] = S.shape(vectors(nan), *shape)
    return _CACHE[key]


def coefficients(handle, F):
    torch = _torch()
    Fd = _dev(F)
    T = torch.full((len(F), 2, 28), -7.0, device="cuda")
    _call("dvsg_tps_coefficients_f32", handle, Fd.data_ptr(), len(F), T.data_ptr(), _stream())
    torch.cuda.synchronize()
    return T.cpu().numpy()


def same_bits_nan(got, want, what):
    """bit for bit, except that a NaN matches any NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": the NaNs sit elsewhere"
    same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), what)


def _zoom(zoomed):
    return _dev(np.full(3, ZOOM, np.float32)) if zoomed else None


def shaped(shape):
    return shape[1:] != (1.0, 0.0) and shape[1] != 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. dvsg_tps_coefficients_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SETS, ids=SET_IDS)
def test_coefficients_are_the_parents_on_the_shaped_field(net, shape):
    model, s, rho = shape
    for nan in (False, True):
        F, Fp = vectors(nan), shaped_F(shape, nan)
        for filt, border in LOOKS[:2]:       # the coefficients read neither
            got = coefficients(net.view(filt, border, s, rho, model), F)
            want = coefficients(net.handle, Fp)
            same_bits_nan(got, want, "%s nan=%d" % (shape, nan))
        if nan:
            assert np.isnan(got[1, 0]).all() and not np.isnan(got[[0, 2]]).any()
            assert np.isnan(got[1, 1]).all() == (model == "similarity")
        elif shaped(shape):
            assert not np.array_equal(got, coefficients(net.handle, F)), "the shape must move T"
    if s == 0.0:       # strength 0 is the identity map's T, whatever F
        same_bits(got[[0, 2]], coefficients(net.handle, np.zeros((2, 25, 2), np.float32)), "strength 0")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the four renders
# ---------------------------------------------------------------------------------------------------------------------
def check_validity(masks, what):
    total, good = sum(ok.size for ok in masks), sum(int(ok.sum()) for ok in masks)
    assert 4 * good >= total, "%s: %d of %d samples valid" % (what, good, total)


@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("look", LOOKS, ids=["%s-%s" % l for l in LOOKS])
@pytest.mark.parametrize("shape", SETS, ids=SET_IDS)
def test_renders_are_the_unshaped_views_on_the_shaped_field(net, shape, look, zoomed):
    """dvsg_tps_render_u8 / _zoom_u8 (out_f32 and out_u8 in columns [2, 2 + W) of rows of W + 3 pixels; 6 x 10 channel-flipped)
    and dvsg_tps_render_nv12 / _zoom_nv12: T, both RGB outputs, both NV12 planes, and every byte around them."""
    model, s, rho = shape
    filt, border = look
    view, plain = net.view(filt, border, s, rho, model), net.view(filt, border)
    assert shape[1:] == (1.0, 0.0) or view is not plain
    F, Fp = vectors(), shaped_F(shape)
    zoom = _zoom(zoomed)
    masks, moved = [], False
    for H, W in RGB_SHAPES:
        src, pre = Bd.rgb_source(H, W), Bd.rgb_prefill(H, W)
        flip = 1 if (H, W) == (6, 10) else 0
        T, f32, u8 = Bd.rgb_render(view, F, src, flip, zoom, pre)
        T0, f0, u0 = Bd.rgb_render(plain, Fp, src, flip, zoom, pre)
        what = "%s %s rgb %dx%d zoom=%d" % (shape, look, H, W, zoomed)
        same_bits(T.cpu().numpy(), T0.cpu().numpy(), what + " T")
        same_bits(f32, f0, what + " out_f32")
        same_bits(u8, u0, what + " out_u8, the columns outside included")
        rest = np.delete(u8, np.s_[Bd.U8_X0:Bd.U8_X0 + W], axis=2)
        assert np.array_equal(rest, np.delete(pre[1], np.s_[Bd.U8_X0:Bd.U8_X0 + W], axis=2)), what + ": columns outside were written"
        xs, ys = grid(T0, zoom, 3, H, W)
        masks.append(np.stack([R.valid(H, W, xs[i], ys[i]) for i in range(3)]))
        moved = moved or not np.array_equal(T.cpu().numpy(), coefficients(net.handle, F))
    for H, W, pitch, uv_row, out_pitch in NV12_SHAPES:
        b, pre = Bd.nv12_source(H, W, pitch, uv_row), Bd.nv12_prefill(H, W, uv_row, out_pitch)
        T, out = Bd.nv12_render(view, F, b, zoom, pre)
        T0, out0 = Bd.nv12_render(plain, Fp, b, zoom, pre)
        what = "%s %s nv12 %dx%d zoom=%d" % (shape, look, H, W, zoomed)
        same_bits(T.cpu().numpy(), T0.cpu().numpy(), what + " T")
        same_bits(out, out0, what + " planes and padding")
        assert np.array_equal(pre.outside(out), pre.outside()), what + ": bytes beyond W or between the planes were written"
        assert not np.array_equal(out, pre.buf), what + ": nothing was rendered"
        for ph, pw in ((H, W), (H // 2, W // 2)):
            xs, ys = grid(T0, zoom, 3, ph, pw)
            masks.append(np.stack([R.valid(ph, pw, xs[i], ys[i]) for i in range(3)]))
    if shaped(shape):
        assert moved, "%s: the shaped T is the parent's T on the raw F" % (shape,)
        check_validity(masks, "%s %s zoom=%d" % (shape, look, zoomed))


@pytest.mark.parametrize("shape", SETS[:3], ids=SET_IDS[:3])
def test_renders_with_a_nan_frame(net, shape):
    """The set with a NaN in frame 1: the same identity; the frame is rendered all invalid (black / unwritten), the others are not."""
    model, s, rho = shape
    F, Fp = vectors(True), shaped_F(shape, True)
    assert np.isnan(Fp[1, :, 0]).all() and not np.isnan(Fp[[0, 2]]).any()
    view, plain = net.view("bilinear", "black", s, rho, model), net.handle
    H, W = RGB_SHAPES[0]
    src, pre = Bd.rgb_source(H, W), Bd.rgb_prefill(H, W)
    T, f32, u8 = Bd.rgb_render(view, F, src, 0, None, pre)
    T0, f0, u0 = Bd.rgb_render(plain, Fp, src, 0, None, pre)
    same_bits_nan(T.cpu().numpy(), T0.cpu().numpy(), "T")
    same_bits_nan(f32, f0, "out_f32")      # (a NaN's sign and payload are not pinned: the frame's samples compare as NaN)
    same_bits(u8, u0, "out_u8")
    cols = np.s_[:, :, Bd.U8_X0:Bd.U8_X0 + W]
    assert (np.isnan(f32[1]) | (f32[1] == 0)).all() and (u8[cols][1] == 0).all(), "no sample of the NaN frame shows the source"
    assert (f32[0] > 0).any() and (f32[2] > 0).any()
    H, W, pitch, uv_row, out_pitch = NV12_SHAPES[1]
    b, pre = Bd.nv12_source(H, W, pitch, uv_row), Bd.nv12_prefill(H, W, uv_row, out_pitch)
    same_bits(Bd.nv12_render(view, F, b, _zoom(True), pre)[1], Bd.nv12_render(plain, Fp, b, _zoom(True), pre)[1], "nv12")


# ---------------------------------------------------------------------------------------------------------------------
# 3. dvsg_tps_coverage_net_f32
# ---------------------------------------------------------------------------------------------------------------------
def scan(handle, F, gh, gw, zoom=None):
    """dvsg_tps_coverage_net_f32 with source and output grid (gh, gw) -> n_border, key_min int32 [n], T (NumPy)"""
    torch = _torch()
    n = len(F)
    need = ctypes.c_size_t()
    _call("dvsg_tps_coverage_workspace_bytes", n, gh, gw, ctypes.byref(need))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
    res = torch.full((2, n), -7, dtype=torch.int32, device="cuda")
    T = torch.full((n, 2, 28), -7.0, device="cuda")
    Fd = F if isinstance(F, torch.Tensor) else _dev(F)
    _call("dvsg_tps_coverage_net_f32", handle, Fd.data_ptr(), zoom.data_ptr() if zoom is not None else None, n, gh, gw, gh, gw,
          T.data_ptr(), res[0].data_ptr(), res[1].data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream())
    torch.cuda.synchronize()
    return res[0].cpu().numpy(), res[1].cpu().numpy(), T.cpu().numpy()


@pytest.mark.parametrize("shape", SETS, ids=SET_IDS)
def test_coverage_scans_the_shaped_warp(net, shape):
    """n_border, key_min and T through the shaped view are the parent's on shape_ref(F): the scan counts the border that the
    shaped render draws.  Grids 6 x 10, 8 x 12 and the 4 x 6 chroma grid of the latter, plain and at zoom 0.8."""
    model, s, rho = shape
    view = net.view("bicubic", "mirror", s, rho, model)
    differs = False
    for nan in (False, True):
        F, Fp = vectors(nan), shaped_F(shape, nan)
        for gh, gw in ((6, 10), (8, 12), (4, 6)):
            for zoomed in (False, True):
                nb, key, T = scan(view, F, gh, gw, _zoom(zoomed))
                nb0, key0, T0 = scan(net.handle, Fp, gh, gw, _zoom(zoomed))
                what = "%s %dx%d zoom=%d nan=%d" % (shape, gh, gw, zoomed, nan)
                assert np.array_equal(nb, nb0) and np.array_equal(key, key0), what
                same_bits_nan(T, T0, what + " T")
                assert (nb[[0, 2]] < gh * gw).all() and (zoomed or (nb > 0).all()), what
                if nan:
                    assert nb[1] == gh * gw, "a NaN frame is all border"
                else:
                    raw = scan(net.handle, F, gh, gw, _zoom(zoomed))
                    differs = differs or not np.array_equal(nb, raw[0]) or not np.array_equal(key, raw[1])
    # (the grids are coarse: the count need not move for every set, but the unshaped map must never be what was scanned)
    print("%s: scan differs from the raw field's: %s" % (shape, differs))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the unshaped view of every model; views and their reports on a real handle
# ---------------------------------------------------------------------------------------------------------------------
def test_unshaped_views_render_the_border_views_bytes(net):
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import SHAPE_MODELS
    lib = _lib.load()
    F = vectors()
    made = []

    def make(parent, f, b, m, s, rho):
        v = ctypes.c_void_p()
        _call("dvsg_locnet_view_create_shaped", parent, f, b, m, s, rho, ctypes.byref(v))
        made.append(v)
        return v

    def report(h):
        m, s, r = ctypes.c_int(-7), ctypes.c_float(-7), ctypes.c_float(-7)
        assert lib.dvsg_locnet_render_shape(h, ctypes.byref(m), ctypes.byref(s), ctypes.byref(r)) == 0
        return m.value, s.value, r.value
    try:
        H, W = RGB_SHAPES[0]
        src, pre = Bd.rgb_source(H, W), Bd.rgb_prefill(H, W)
        b, npre = Bd.nv12_source(*NV12_SHAPES[1][:4]), Bd.nv12_prefill(8, 12, 9, 20)
        for f, bo in ((0, 0), (1, 2), (0, 3)):
            old = ctypes.c_void_p()
            _call("dvsg_locnet_view_create_border", net.handle, f, bo, ctypes.byref(old))
            made.append(old)
            assert report(old) == (0, 1.0, 0.0)
            T0, f0, u0 = Bd.rgb_render(old, F, src, 0, _zoom(True), pre)
            n0 = Bd.nv12_render(old, F, b, None, npre)[1]
            for m in SHAPE_MODELS.values():
                new = make(net.handle, f, bo, m, 1.0, 0.0)
                assert report(new) == (m, 1.0, 0.0)
                assert (lib.dvsg_locnet_render_filter(new), lib.dvsg_locnet_render_border(new)) == (f, bo)
                T1, f1, u1 = Bd.rgb_render(new, F, src, 0, _zoom(True), pre)
                same_bits(T1.cpu().numpy(), T0.cpu().numpy(), "T")
                same_bits(f1, f0, "out_f32")
                same_bits(u1, u0, "out_u8")
                same_bits(Bd.nv12_render(new, F, b, None, npre)[1], n0, "nv12")
                same_bits(coefficients(new, F), coefficients(net.handle, F), "coefficients")
        # reports on a real network: the handle, its views, a view of a shaped view (nothing inherited)
        assert report(net.handle) == (0, 1.0, 0.0) and report(net.view("bicubic", "mirror")) == (0, 1.0, 0.0)
        sv = make(net.handle, 1, 2, 1, 0.25, 0.75)
        assert report(sv) == (1, 0.25, 0.75)
        nested = make(sv, 0, 0, 2, 0.5, 1.0)
        assert report(nested) == (2, 0.5, 1.0) and lib.dvsg_locnet_render_border(nested) == 0
        border_of_shaped = ctypes.c_void_p()
        _call("dvsg_locnet_view_create_border", sv, 0, 1, ctypes.byref(border_of_shaped))
        made.append(border_of_shaped)
        assert report(border_of_shaped) == (0, 1.0, 0.0)
        same_bits(coefficients(border_of_shaped, F), coefficients(net.handle, F), "a view of a shaped view is unshaped")
        same_bits(coefficients(nested, F), coefficients(net.handle, S.shape(F, "translation", 0.5, 1.0)), "nested shaped view")
        assert lib.dvsg_locnet_in_channels(sv) == 21
        # the other entry points see the parent: calibrating through a shaped view is refused like through any view
        ws = _torch().empty(1 << 10, dtype=_torch().uint8, device="cuda")
        assert lib.dvsg_locnet_calibrate_f16(sv, None, 0, 0, 0, ws.data_ptr(), ws.numel(), None) == -1
        assert b"view" in lib.dvsg_last_error_string()
        assert lib.dvsg_locnet_destroy(net.handle) == -1 and b"view" in lib.dvsg_last_error_string()
    finally:
        for v in made:
            assert lib.dvsg_locnet_destroy(v) == 0
    # LocNet.view: cached on all five values; an unshaped request is the two-argument view whatever its model
    assert net.view("bilinear", "black", 1.0, 0.0, "translation") is net.handle
    assert net.view("bicubic", "mirror", 1.0, 0.0, "similarity") is net.view("bicubic", "mirror")
    a = net.view("bilinear", "black", 0.5, 0.0, "affine")
    assert a is net.view("bilinear", "black", 0.5) and a is not net.handle
    assert a is not net.view("bilinear", "black", 0.5, 0.0, "similarity") and a is not net.view("bicubic", "black", 0.5)
    assert a is not net.view("bilinear", "black", 0.5, 0.25)
    assert report(net.view("bilinear", "keep", 0.1, 1, "translation")) == (2, float(np.float32(0.1)), 1.0)


def test_forward_through_a_shaped_view_is_the_parents(net):
    """dvsg_locnet_forward_* does not read the shape: F_t through a shaped view is the parent's, bit for bit."""
    import inputs
    torch = _torch()
    H, W, n = 64, 96, 2
    x = _dev(inputs.window_frames(7, n, H, W))
    need = ctypes.c_size_t()
    _call("dvsg_locnet_workspace_bytes", net.handle, n, H, W, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    out = []
    for h in (net.handle, net.view("bilinear", "black", 0.25, 1.0, "translation")):
        F = torch.full((n, 25, 2), -7.0, device="cuda")
        _call("dvsg_locnet_forward_f32", h, x.data_ptr(), n, H, W, F.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        out.append(F.cpu().numpy())
    same_bits(out[1], out[0], "F_t")
    assert np.abs(out[0]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the recurrence is untouched; scan, crop and render see one warp
# ---------------------------------------------------------------------------------------------------------------------
ONLINE = dict(strength=0.5, rigidity=1.0, shape_model="similarity")
ONLINE_SET = ("similarity", 0.5, 1.0)
SRC = (44, 60)
STEPS = 6


def test_online_nv12_shaped_stream_shares_the_recurrence():
    """Two OnlineStabilizers on the same 6 NV12 frames of 44 x 60 (model 38 x 54, the pipe tests'), crop="auto", one shaped.  The pool
    and F_t are the same bits after every step.  Each shaped output is dvsg_tps_render_zoom_nv12 of the unshaped view on
    shape_ref(F_t) with the zoom the stream reports, and that zoom is the ratchet (tests/ratchet_ref.py) on the scans of both
    planes through the shaped view."""
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd.online import OnlineStabilizer
    torch = _torch()
    model = pipe.model()
    H0, W0 = SRC
    clip = nv12_ref.smooth_batch(930, STEPS, H0, W0).buf
    on = OnlineStabilizer(model, skip_length=pipe.SKIP, frame_format="nv12", crop="auto", **ONLINE)
    off = OnlineStabilizer(model, skip_length=pipe.SKIP, frame_format="nv12", crop="auto")
    on.pool.zero_()
    off.pool.zero_()
    s_on, s_off = on.open(), off.open()
    view = model.locnet.view("bilinear", "black", ONLINE["strength"], ONLINE["rigidity"], ONLINE["shape_model"])
    state = np.ones(1, np.float32)
    moved = False
    for k in range(STEPS):
        got = on.push(s_on, clip[k])
        base = off.push(s_off, clip[k])
        same_bits(on._F.cpu().numpy(), off._F.cpu().numpy(), "F_t of step %d" % k)
        same_bits(on.pool.cpu().numpy(), off.pool.cpu().numpy(), "pool after step %d" % k)
        F = on._F[:1].cpu().numpy()
        z = on.crop_state(s_on)["zoom"]
        # the zoom: the ratchet on the scan of the SHAPED view, both planes
        (lh, lw), (ch, cw) = ratchet_ref.plane_grids(H0, W0)
        _, key_l, _ = scan(view, F, lh, lw)
        _, key_c, _ = scan(view, F, ch, cw)
        want_z, _, _ = ratchet_ref.ratchet(state, [0], key_l, (lh - 1) * (lw - 1), key_c, (ch - 1) * (cw - 1),
                                           ratchet_ref.nv12_margin(H0, W0), 0.5, 0.0)
        assert z.tobytes() == want_z[0].tobytes(), "step %d: zoom %r, the ratchet on the shaped scan gives %r" % (k, z, want_z[0])
        # the output: the unshaped view on shape_ref(F_t) at that zoom
        Fp = S.shape(F, *ONLINE_SET)
        b = nv12_ref.Batch(0, 1, H0, W0)
        b.buf = clip[k][None]
        _, alone = Bd.nv12_render(model.locnet.handle, Fp, b, _dev(np.float32([z])), nv12_ref.Batch(0, 1, H0, W0, fill=0xA5))
        same_bits(got, alone[0], "output of step %d" % k)
        moved = moved or not np.array_equal(got, base)
        print("step %d: zoom shaped %r, unshaped %r" % (k, z, off.crop_state(s_off)["zoom"]))
    assert moved, "the shaped stream must render something else than the unshaped one"
    torch.cuda.synchronize()


def test_stabilize_clip_is_the_shaped_online_stream():
    """RGB at source size, as the source_res tests pair them.  Without crop: the clip's frames are the online stream's.  With
    crop="auto": the clip's one zoom is the zoom the online ratchet has reached after the last frame -- both scan the shaped
    view: it is crop_zoom of the `free` that a scan through that view reports --, and every frame is dvsg_tps_render_zoom_u8 of
    the unshaped view on shape_ref(F_t) at that zoom."""
    import inputs
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd.clip import crop_zoom, stabilize_clip
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = pipe.model()
    H0, W0 = SRC
    frames = (inputs.smooth_frames(940, STEPS, H0, W0) * 255).astype(np.uint8)
    kw = dict(source_res=True, as_uint8=True, render_filter="bicubic", border="replicate", **ONLINE)
    on = OnlineStabilizer(model, skip_length=pipe.SKIP, **kw)
    sid = on.open()
    got, Fs = [], []
    for k in range(STEPS):
        got.append(on.push(sid, frames[k]))
        Fs.append(on._F[:1].cpu().numpy())
    want = stabilize_clip(model, None, frames, skip_length=pipe.SKIP, **kw)
    same_bits(want, np.stack(got), "stabilize_clip against the online stream")
    plain = stabilize_clip(model, None, frames, skip_length=pipe.SKIP, source_res=True, as_uint8=True, render_filter="bicubic",
                           border="replicate")
    assert not np.array_equal(plain, want)
    # crop="auto"
    auto = OnlineStabilizer(model, skip_length=pipe.SKIP, crop="auto", **kw)
    sid = auto.open()
    for k in range(STEPS):
        auto.push(sid, frames[k])
    info = {}
    cropped = stabilize_clip(model, None, frames, skip_length=pipe.SKIP, crop="auto", crop_info=info, **kw)
    assert np.float32(info["zoom"]).tobytes() == auto.crop_state(sid)["zoom"].tobytes()
    F = np.concatenate(Fs)
    view = model.locnet.view("bicubic", "replicate", ONLINE["strength"], ONLINE["rigidity"], ONLINE["shape_model"])
    _, key, _ = scan(view, F, H0, W0)
    D = (H0 - 1) * (W0 - 1)
    free = np.minimum(key.astype(np.int64), D).astype(np.float64) / D
    assert np.array_equal(info["free"], free)
    assert np.float32(info["zoom"]) == crop_zoom(free, out_hw=(H0, W0))
    Fp = S.shape(F, *ONLINE_SET)
    zoom = _dev(np.full(STEPS, info["zoom"], np.float32))
    torch = _torch()
    T = torch.empty((STEPS, 2, 28), device="cuda")
    out = torch.zeros((STEPS, H0, W0, 3), dtype=torch.uint8, device="cuda")
    Fd, srcd = _dev(Fp), _dev(frames)
    _call("dvsg_tps_render_zoom_u8", model.locnet.view("bicubic", "replicate"), Fd.data_ptr(), srcd.data_ptr(), STEPS, H0, W0, 0,
          zoom.data_ptr(), T.data_ptr(), None, out.data_ptr(), W0, 0, _stream())
    torch.cuda.synchronize()
    same_bits(cropped, out.cpu().numpy(), "stabilize_clip(crop='auto') against the unshaped view on shape_ref(F_t)")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the stream contract for the new launch
# ---------------------------------------------------------------------------------------------------------------------
class NV12Call(object):
    """dvsg_tps_render_nv12 through a shaped view with its own inputs and outputs on the device"""

    def __init__(self, handle, seed):
        torch = _torch()
        H, W, pitch, uv_row, out_pitch = 16, 20, 32, 19, 28
        self.handle = handle
        self.b = nv12_ref.Batch(seed, 3, H, W, pitch, uv_row)
        self.ob = nv12_ref.Batch(0, 3, H, W, out_pitch, uv_row, fill=0xA5)
        self.buf = _dev(self.b.buf)
        self.F = torch.zeros((3, 25, 2), device="cuda")
        self.T = torch.empty((3, 2, 28), device="cuda")
        self.out = _dev(self.ob.buf)

    def fill(self, seed):
        self.F.copy_(_dev(np.random.default_rng(seed).uniform(-0.05, 0.05, (3, 25, 2)).astype(np.float32)))
        self.out.fill_(0xA5)
        self.T.fill_(-7.0)

    def issue(self, s):
        b, ob = self.b, self.ob
        _call("dvsg_tps_render_nv12", self.handle, self.F.data_ptr(), self.buf.data_ptr(), self.buf.data_ptr() + b.uv_offset,
              b.pitch, b.frame_stride, 3, b.H, b.W, self.T.data_ptr(), self.out.data_ptr(), self.out.data_ptr() + ob.uv_offset,
              ob.pitch, ob.frame_stride, s)

    def snapshot(self):
        return self.T.cpu().numpy(), self.out.cpu().numpy()

    def same(self, want, what):
        got = self.snapshot()
        same_bits(got[0], want[0], what + ": T")
        same_bits(got[1], want[1], what + ": planes")


def test_shaped_render_replays_from_a_captured_graph(net):
    """One capture on a side stream, one linear chain of two launches, replayed on two fresh F_t."""
    torch = _torch()
    c = NV12Call(net.view("bicubic", "mirror", 0.25, 0.75, "similarity"), 5)
    side = torch.cuda.Stream()
    s = side.cuda_stream
    c.fill(0)
    torch.cuda.synchronize()
    c.issue(s)                          # warm up
    side.synchronize()
    want = []
    for seed in (1, 2):
        c.fill(seed)
        torch.cuda.synchronize()
        c.issue(s)
        side.synchronize()
        want.append(c.snapshot())
    assert not np.array_equal(want[0][1], want[1][1])
    c.fill(0)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.issue(s)
    finally:
        gc.enable()
    torch.cuda.synchronize()
    for k, seed in enumerate((1, 2)):
        c.fill(seed)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.same(want[k], "replay %d" % (k + 1))
    # and the eager values are the contract's
    Fp = S.shape(c.F.cpu().numpy(), "similarity", 0.25, 0.75)
    c.handle = net.view("bicubic", "mirror")
    c.F.copy_(_dev(Fp))
    c.out.fill_(0xA5)
    c.issue(s)
    side.synchronize()
    c.same(want[1], "the unshaped view on shape_ref(F)")


def test_shaped_render_on_two_streams_of_one_handle(net):
    import test_gpu_streams as ts
    torch = _torch()
    view = net.view("bilinear", "black", 0.5, 1.0, "affine")
    a, b = NV12Call(view, 6), NV12Call(view, 7)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    want = []
    for c, seed, st in ((a, 1, s1), (b, 2, s2)):
        c.fill(seed)
        torch.cuda.synchronize()
        c.issue(st.cuda_stream)
        st.synchronize()
        want.append(c.snapshot())
    delay = ts.Delay()

    def run(scale):
        a.fill(1)
        b.fill(2)
        torch.cuda.synchronize()
        ev = delay.enqueue(delay.stream, scale)
        s1.wait_event(ev)
        s2.wait_event(ev)
        a.issue(s1.cuda_stream)
        b.issue(s2.cuda_stream)
        return ev.query()
    ts.behind_delay(delay, run, "shaped dvsg_tps_render_nv12 twice")
    a.same(want[0], "first call")
    b.same(want[1], "second call")
    assert not np.array_equal(want[0][1], want[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# 7. the pipe front end
# ---------------------------------------------------------------------------------------------------------------------
def test_pipes_pass_the_shape_on():
    import test_gpu_pipe as pipe
    from coupe.dvsg_amd import y4m
    from coupe.dvsg_amd.online import OnlineStabilizer
    i420 = pipe.clips()["single_i420"][:3]
    out = io.BytesIO()
    src = y4m.Y4MReader(io.BytesIO(pipe.y4m_bytes(i420)))
    pipe.run([src], [y4m.Y4MWriter(out, src.width, src.height, src.fps)], strength=0.5)
    got = pipe.nv12_frames_of_y4m(out.getvalue())[0]
    on = OnlineStabilizer(pipe.model(), frame_format="nv12", skip_length=pipe.SKIP, yuv_matrix=y4m.default_yuv_matrix(pipe.BIG[0]),
                          strength=0.5)
    sid = on.open()
    want = np.stack([on.push(sid, f) for f in pipe.clips()["single"][:3]])
    pipe.same(got, want, "stabilize_pipes against OnlineStabilizer")
    assert not np.array_equal(want, pipe.reference("single")[0][:3]), "strength 0.5 must differ from the full warp"
