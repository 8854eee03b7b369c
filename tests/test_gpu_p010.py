"""GPU: P010 frames (include/dvsg_amd.h, "P010 frames") -- the surface format of a view, the two NV12 renders on 10-bit
surfaces, OnlineStabilizer(frame_format="p010") and 10-bit pipes.  Everything compares bit for bit.  Outputs are pre-filled
(seeded bytes or a poison byte) and nothing beyond 2 W bytes of a row, between the planes or between the frames may change.

Shapes: (4, 4) -- chroma 2 x 2, the bicubic pw < 4 path; (6, 8) -- chroma pw = 4, the packed window fills the row; (10, 520) --
luma over three 256-column tiles, chroma over two, both planes end in a partial 4-row tile.  n = 2, frame_stride larger than
the frame, input pitch 2 W + 6 (even, no multiple of 4: words off the dword grid), another output pitch.  The border tests
also run the three-frame launches of tests/test_gpu_border.py ("launch", "far", "nan") with its zoom.  COVERED names a test
for each of the sixteen p010_render_kernel<kZoom, kCubic, kBorder> instantiations."""
import ctypes
import io
import threading

import numpy as np
import pytest

import bicubic_ref as R
import border_ref
import inputs
import nv12_ref
import p010_ref
import shape_ref
import test_gpu_bicubic as B
import test_gpu_border as GB

pytestmark = pytest.mark.gpu

POISON = 0xA5
NEUTRAL = 512 << 6
ZOOM = (0.9, 0.9)
#        H   W   uv_row  low bits  out pitch
SHAPES = [(4, 4, 4, 0, 2 * 4 + 2), (6, 8, 7, 0x2B, 2 * 8 + 4), (10, 520, 10, 0, 2 * 520 + 2)]
_CACHE = {}

_dev, _call, _stream, grid, same_bits = B._dev, B._call, B._stream, B.grid, B.same_bits


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def net(synthetic_weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def vectors():
    """F_t as tests/test_gpu_nv12.py draws it, scaled by 2: with and without ZOOM every plane of every shape then has valid
    and invalid samples at least 0.02 of a sample away from the edge of validity (asserted where the grids are known)."""
    return (np.float32(2.0) * inputs.control_vectors(905, 2)).astype(np.float32)


def source(H, W, uv_row, low, n=2):
    return p010_ref.P010Batch(100 * H + W, n, H, W, 2 * W + 6, uv_row, tail=1, low=low)


def prefill(H, W, uv_row, out_pitch, n=2):
    b = p010_ref.P010Batch(0, n, H, W, out_pitch, uv_row + 1, tail=2, fill=POISON)
    b.buf[:] = np.random.default_rng(7 * H + W).integers(0, 256, b.buf.shape, dtype=np.uint8)
    return b


def render(handle, F, b, zoom, pre, name="p010"):
    """One launch of dvsg_tps_render_nv12 / _zoom_nv12 of batch b into a guarded copy of `pre` -> (T, the output's bytes)"""
    import test_conv_gemm_f64 as f64
    torch = _torch()
    T = torch.full((b.n, 2, 28), float("nan"), device="cuda")
    buf, g, Fd = _dev(b.buf), f64.Guarded.of(_dev(pre.buf)), _dev(F)
    args = [handle, Fd.data_ptr(), buf.data_ptr(), buf.data_ptr() + b.uv_offset, b.pitch, b.frame_stride, b.n, b.H, b.W]
    if zoom is not None:
        args.append(zoom.data_ptr())
    args += [T.data_ptr(), g.ptr(), g.ptr() + pre.uv_offset, pre.pitch, pre.frame_stride, _stream()]
    _call("dvsg_tps_render_zoom_nv12" if zoom is not None else "dvsg_tps_render_nv12", *args)
    torch.cuda.synchronize()
    assert g.intact(), "%s: a guard byte was written" % name
    assert np.array_equal(buf.cpu().numpy(), b.buf), "%s: the source changed" % name
    return T, g.view(torch.uint8, pre.buf.shape).cpu().numpy()


def _zoom(zoomed):
    return _dev(np.float32(ZOOM)) if zoomed else None


def grids(T, zoom, H, W):
    """per plane: (x_s, y_s, valid) [2, ph, pw] of the grid-only dvsg_tps_warp_zoom_f32"""
    out = []
    for ph, pw in ((H, W), (H // 2, W // 2)):
        xs, ys = grid(T, zoom, 2, ph, pw)
        ok = np.stack([R.valid(ph, pw, xs[i], ys[i]) for i in range(2)])
        assert ok.any() and not ok.all(), "plane %d x %d: %d of %d samples valid" % (ph, pw, ok.sum(), ok.size)
        out.append((xs, ys, ok))
    return out


# The three-frame launches of tests/test_gpu_border.py -- "launch" (every side of every plane fully invalid in some frame),
# "far" (the clamp behind the one reflection is reached) and "nan" (one NaN component in frame 1) -- with its zoom.
KINDS = ("launch", "far", "nan")


def launch(kind, shape, zoomed):
    """(source, pre-filled output, F_t, zoom) of a three-frame launch of `kind` at a row of SHAPES"""
    H, W, uv_row, low, out_pitch = shape
    return (source(H, W, uv_row, low, 3), prefill(H, W, uv_row, out_pitch, 3), GB.vectors(kind),
            _dev(np.float32(GB.ZOOM)) if zoomed else None)


def plane_grids(T, zoom, n, H, W):
    """per plane: (x_s, y_s, valid) [n, ph, pw] of the grid-only dvsg_tps_warp_zoom_f32"""
    out = []
    for ph, pw in ((H, W), (H // 2, W // 2)):
        xs, ys = grid(T, zoom, n, ph, pw)
        out.append((xs, ys, np.stack([R.valid(ph, pw, xs[i], ys[i]) for i in range(n)])))
    return out


def black_and_grids(net, filt, kind, shape, zoomed):
    """(the two planes' words of the black-border P010 render of the launch, its plane_grids), once per launch"""
    key = ("black", filt, kind, shape, zoomed)
    if key not in _CACHE:
        b, pre, F, zoom = launch(kind, shape, zoomed)
        T, out = render(net.view(filt, "black", surface="p010"), F, b, zoom, pre)
        _CACHE[key] = (pre.words(out), plane_grids(T, zoom, 3, shape[0], shape[1]))
    return _CACHE[key]


def check_launch_inputs(net, zoomed):
    """tests/test_gpu_border.py's two assertions about the "launch" kind's masks, over all SHAPES and both planes"""
    if ("masks", zoomed) not in _CACHE:
        GB.check_inputs([ok for shape in SHAPES for _, _, ok in black_and_grids(net, "bilinear", "launch", shape, zoomed)[1]])
        _CACHE[("masks", zoomed)] = True


def check_kind(kind, xs, ys, ok, what):
    if kind == "far":
        assert not ok.any(), what
    elif kind == "nan":
        assert (np.isnan(xs[1]) | np.isnan(ys[1])).all() and not ok[1].any() and ok[0].any(), what


def warp_plane(s, T, zoom):
    """dvsg_tps_warp_f32 / dvsg_tps_warp_zoom_f32 of the float image s [n, ph, pw, C] at its own size"""
    torch = _torch()
    n, ph, pw, C = s.shape
    U, V = _dev(s), _dev(inputs.v_src(n))
    out = torch.full_like(U, float("nan"))
    if zoom is None:
        _call("dvsg_tps_warp_f32", U.data_ptr(), V.data_ptr(), T.data_ptr(), n, ph, pw, C, 25, ph, pw, out.data_ptr(), None,
              None, _stream())
    else:
        _call("dvsg_tps_warp_zoom_f32", U.data_ptr(), V.data_ptr(), T.data_ptr(), zoom.data_ptr(), n, ph, pw, C, 25, ph, pw,
              out.data_ptr(), None, None, _stream())
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. bilinear, black border: each plane is the sample rule, dvsg_tps_warp(_zoom)_f32 on the float image, the word rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("H,W,uv_row,low,out_pitch", SHAPES)
def test_bilinear_render_is_the_composition(net, H, W, uv_row, low, out_pitch, zoomed):
    torch = _torch()
    view = net.view(surface="p010")
    b, pre = source(H, W, uv_row, low), prefill(H, W, uv_row, out_pitch)
    for plane in b.words():
        s = plane >> 6
        assert s.min() == 0 and s.max() == 1023 and ((plane & 0x3F) == low).all()
    F, zoom = vectors(), _zoom(zoomed)
    T, out = render(view, F, b, zoom, pre)
    # T is dvsg_tps_render_u8's
    T8 = torch.full_like(T, float("nan"))
    rgb = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    f32 = torch.empty((2, H, W, 3), device="cuda")
    _call("dvsg_tps_render_u8", net.handle, _dev(F).data_ptr(), rgb.data_ptr(), 2, H, W, 0, T8.data_ptr(), f32.data_ptr(), None,
          0, 0, _stream())
    torch.cuda.synchronize()
    same_bits(T.cpu().numpy(), T8.cpu().numpy(), "T")
    got = pre.words(out)
    for p, (name, (xs, ys, ok)) in enumerate(zip(("luma", "chroma"), grids(T, zoom, H, W))):
        v = warp_plane(p010_ref.samples(b.words()[p], p == 1), T8, zoom)
        same_bits(got[p], p010_ref.to_word(v, p == 1), "%s %dx%d zoom=%d" % (name, H, W, zoomed))
        assert (got[p][~ok] == (NEUTRAL if p else 0)).all(), "%s: the border is not neutral" % name
        assert ((got[p] & 0x3F) == 0).all(), "%s: low bits were written" % name
    assert np.array_equal(pre.outside(out), pre.outside()), "bytes beyond 2 W, between the planes or the frames were written"


# ---------------------------------------------------------------------------------------------------------------------
# 2. bicubic x every border x zoom against p010_ref
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("border", ["black", "replicate", "mirror", "keep"])
@pytest.mark.parametrize("H,W,uv_row,low,out_pitch", SHAPES[1:])
def test_bicubic_borders_are_the_reference(net, H, W, uv_row, low, out_pitch, border, zoomed):
    view = net.view("bicubic", border, surface="p010")
    b, pre = source(H, W, uv_row, low), prefill(H, W, uv_row, out_pitch)
    F, zoom = vectors(), _zoom(zoomed)
    T, out = render(view, F, b, zoom, pre)
    key = (H, W, zoomed)
    if key not in _CACHE:
        _CACHE[key] = grids(T, zoom, H, W)
    got, before, src = pre.words(out), pre.words(), b.words()
    for p, (name, (xs, ys, ok)) in enumerate(zip(("luma", "chroma"), _CACHE[key])):
        want = np.empty_like(got[p])
        for i in range(2):
            v, written = p010_ref.render_bicubic(src[p][i], xs[i], ys[i], border, p == 1)
            want[i] = np.where(written[..., None], p010_ref.to_word(v, p == 1), before[p][i])
            assert border != "keep" or np.array_equal(written, ok[i])
        same_bits(got[p], want, "%s %s %dx%d zoom=%d" % (border, name, H, W, zoomed))
        if border == "keep":
            assert np.array_equal(got[p][~ok], before[p][~ok]), "%s: keep wrote an invalid sample" % name
    assert np.array_equal(pre.outside(out), pre.outside()), "bytes beyond 2 W, between the planes or the frames were written"
    # the far launch and the launch with a NaN (three frames): every sample is the restatement's; in the frame with the NaN
    # coordinate every written luma word is 0 and every chroma word 512 << 6, and keep writes nothing
    shape = (H, W, uv_row, low, out_pitch)
    for kind in KINDS[1:]:
        b, pre, F, zoom = launch(kind, shape, zoomed)
        T, out = render(view, F, b, zoom, pre)
        key = (H, W, zoomed, kind)
        if key not in _CACHE:
            _CACHE[key] = plane_grids(T, zoom, 3, H, W)
        got, before, src = pre.words(out), pre.words(), b.words()
        for p, (name, (xs, ys, ok)) in enumerate(zip(("luma", "chroma"), _CACHE[key])):
            what = "%s %s %s %dx%d zoom=%d" % (kind, border, name, H, W, zoomed)
            check_kind(kind, xs, ys, ok, what)
            want = np.empty_like(got[p])
            for i in range(3):
                v, written = p010_ref.render_bicubic(src[p][i], xs[i], ys[i], border, p == 1)
                want[i] = np.where(written[..., None], p010_ref.to_word(v, p == 1), before[p][i])
                assert np.array_equal(written, ok[i] if border == "keep" else np.ones_like(ok[i]))
            same_bits(got[p], want, what)
            if kind == "nan":
                blank = before[p][1] if border == "keep" else np.full_like(before[p][1], NEUTRAL if p else 0)
                same_bits(got[p][1], blank, what + ": the frame with a NaN coordinate")
        assert np.array_equal(pre.outside(out), pre.outside()), "%s: bytes outside the planes were written" % kind


# ---------------------------------------------------------------------------------------------------------------------
# 2b. bilinear x replicate, mirror, keep x zoom: render_plane<C, false, kBorder, uint16_t> against p010_ref.render_bilinear
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("border", ["replicate", "mirror", "keep"])
@pytest.mark.parametrize("H,W,uv_row,low,out_pitch", SHAPES)
def test_bilinear_borders_are_the_reference(net, H, W, uv_row, low, out_pitch, border, zoomed, kind):
    """Valid samples are the bits of the black-border P010 render of the same launch; invalid ones are
    to_word(p010_ref.render_bilinear), word for word; keep leaves the pre-filled words.  (4, 4): in the 2 x 2 chroma plane
    x1 = min(x0 + 1, pw - 1) clips at once."""
    shape = (H, W, uv_row, low, out_pitch)
    b, pre, F, zoom = launch(kind, shape, zoomed)
    T, out = render(net.view("bilinear", border, surface="p010"), F, b, zoom, pre)
    black, g = black_and_grids(net, "bilinear", kind, shape, zoomed)
    if kind == "launch":
        check_launch_inputs(net, zoomed)
    got, before, src = pre.words(out), pre.words(), b.words()
    for p, (name, (xs, ys, ok)) in enumerate(zip(("luma", "chroma"), g)):
        what = "%s %s %s %dx%d zoom=%d" % (kind, border, name, H, W, zoomed)
        check_kind(kind, xs, ys, ok, what)
        want, wrote = np.empty_like(got[p]), np.empty_like(ok)
        for i in range(3):
            v, wrote[i] = p010_ref.render_bilinear(src[p][i], xs[i], ys[i], border, p == 1)
            want[i] = np.where(wrote[i][..., None], p010_ref.to_word(v, p == 1), before[p][i])
        assert np.array_equal(wrote, ok if border == "keep" else np.ones_like(ok))
        same_bits(got[p][ok], black[p][ok], what + ", valid samples against the black border")
        same_bits(got[p][~ok], want[~ok], what + ", invalid samples against p010_ref.render_bilinear")
        assert ((got[p][wrote] & 0x3F) == 0).all(), what + ": low bits were written"
        if border == "keep":
            assert np.array_equal(got[p][~ok], before[p][~ok]) and (before[p][~ok] & 0x3F).any(), what + ": keep wrote an invalid sample"
        elif kind == "nan":
            assert (got[p][1] == (NEUTRAL if p else 0)).all(), what + ": a NaN coordinate gives the black value"
    assert np.array_equal(pre.outside(out), pre.outside()), "bytes beyond 2 W, between the planes or the frames were written"


@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("border", ["replicate", "mirror"])
def test_far_launch_writes_one_corner_sample(net, border, filt, zoomed):
    """A known answer that no restatement enters.  F_t = (-2.5, +2.5) at all 25 points moves every coordinate of every plane
    out through the left side (x < 0) and the bottom side (y > ph - 1).  Replicate clamps each to (0, ph - 1): every word of
    a frame's plane is that plane's BOTTOM-LEFT sample with the low bits cleared.  Mirror reflects once (x -> -x, y -> 2 (ph - 1)
    - y) and clamps what is still outside, so wherever the coordinate lies beyond the one reflection on both axes --
    x <= -(pw - 1) and y >= 2 (ph - 1), read off the grid alone -- the word is the TOP-RIGHT sample; samples within one
    reflection on an axis are blends and are left to the restatement tests.  On the clamped coordinate the bilinear weights
    are 1, 0, 0, 0 and the bicubic ones 0, 1, 0, 0 on each axis, exactly (t = 0; tests/test_p010_cpu.py checks both
    restatements), so both filters are held exactly."""
    F = GB.vectors("far")
    assert (F[..., 0] < 0).all() and (F[..., 1] > 0).all()
    for shape in SHAPES:
        H, W = shape[:2]
        b, pre, F, zoom = launch("far", shape, zoomed)
        T, out = render(net.view(filt, border, surface="p010"), F, b, zoom, pre)
        got, src = pre.words(out), b.words()
        for p, (xs, ys, ok) in enumerate(plane_grids(T, zoom, 3, H, W)):
            ph, pw = ok.shape[1:]
            x, y = border_ref.coords(ph, pw, xs, ys, np.float64)
            assert (x < 0).all() and (y > ph - 1).all()
            sel = np.ones_like(ok) if border == "replicate" else (x <= -(pw - 1)) & (y >= 2 * (ph - 1))
            for i in range(3):
                assert sel[i].any(), "no sample of frame %d of the %d x %d plane lies beyond the reflection" % (i, ph, pw)
                corner = src[p][i, ph - 1, 0] if border == "replicate" else src[p][i, 0, pw - 1]
                bad = (got[p][i][sel[i]] != (corner & 0xFFC0)).any(axis=-1)
                assert not bad.any(), "%s %s %dx%d plane %d frame %d zoom=%d: %d of %d words are not the corner sample" % (
                    border, filt, H, W, p, i, zoomed, bad.sum(), bad.size)


# (kZoom, kCubic, kBorder) of p010_render_kernel -> the test that launches it, from the parametrisations above
COVERED = {}
for _z in (False, True):
    COVERED[(_z, False, "black")] = "test_bilinear_render_is_the_composition"
    for _b in ("replicate", "mirror", "keep"):
        COVERED[(_z, False, _b)] = "test_bilinear_borders_are_the_reference"
    for _b in ("black", "replicate", "mirror", "keep"):
        COVERED[(_z, True, _b)] = "test_bicubic_borders_are_the_reference"


def _parametrised(test):
    """the set of (zoomed, border or None) over the parametrize marks of a test function"""
    values = {m.args[0]: m.args[1] for m in test.pytestmark if m.name == "parametrize"}
    return {(z, bd) for z in values["zoomed"] for bd in values.get("border", [None])}


def test_every_p010_render_instantiation_has_a_test():
    """2 x 2 x 4 instantiations of p010_render_kernel<kZoom, kCubic, kBorder>, each named with a test whose parameters reach it"""
    assert len(COVERED) == 16 and set(COVERED) == {(z, c, bd) for z in (False, True) for c in (False, True)
                                                   for bd in border_ref.BORDERS}
    for (z, cubic, bd), name in COVERED.items():
        cases = _parametrised(globals()[name])
        assert (z, bd) in cases or (z, None) in cases and bd == "black", (z, cubic, bd, name)
        assert ("bicubic" in name) == cubic


def test_bicubic_tiny_plane(net):
    """(4, 4): chroma is 2 x 2, one load per tap component"""
    H, W, uv_row, low, out_pitch = SHAPES[0]
    b, pre = source(H, W, uv_row, low), prefill(H, W, uv_row, out_pitch)
    for border in ("black", "mirror"):
        T, out = render(net.view("bicubic", border, surface="p010"), vectors(), b, None, pre)
        got, src = pre.words(out), b.words()
        for p, (xs, ys, ok) in enumerate(grids(T, None, H, W)):
            want = np.stack([p010_ref.to_word(p010_ref.render_bicubic(src[p][i], xs[i], ys[i], border, p == 1)[0], p == 1)
                             for i in range(2)])
            same_bits(got[p], want, "%s plane %d" % (border, p))
        assert np.array_equal(pre.outside(out), pre.outside())


# ---------------------------------------------------------------------------------------------------------------------
# 3. a shaped view
# ---------------------------------------------------------------------------------------------------------------------
def test_shaped_view(net):
    H, W, uv_row, low, out_pitch = SHAPES[1]
    b, pre = source(H, W, uv_row, low), prefill(H, W, uv_row, out_pitch)
    F, zoom = vectors(), _zoom(True)
    shaped = net.view("bilinear", "black", 0.5, 1.0, "similarity", surface="p010")
    T, out = render(shaped, F, b, zoom, pre)
    Fp = shape_ref.shape(F, "similarity", 0.5, 1.0)
    T0, out0 = render(net.view(surface="p010"), Fp, b, zoom, pre)
    same_bits(T.cpu().numpy(), T0.cpu().numpy(), "T against the unshaped view given F'")
    assert np.array_equal(out, out0), "the planes of the shaped view are not the unshaped view's given F'"
    nb = nv12_ref.Batch(3, 2, H, W)
    Tn, _ = render(net.view("bilinear", "black", 0.5, 1.0, "similarity"), F, nb, zoom, nv12_ref.Batch(4, 2, H, W), "nv12")
    same_bits(T.cpu().numpy(), Tn.cpu().numpy(), "T against the shaped NV12 view")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the property: argument checks, inheritance, and what does not read it
# ---------------------------------------------------------------------------------------------------------------------
def _surface_view(handle, fmt):
    v = ctypes.c_void_p()
    _call("dvsg_locnet_view_create_surface", handle, fmt, ctypes.byref(v))
    return v


def test_argument_checks_and_what_reads_the_property(net):
    from coupe.dvsg_amd import _lib
    torch = _torch()
    lib = _lib.load()
    H, W = 6, 8
    p010 = _surface_view(net.handle, 1)
    back = _surface_view(p010, 0)   # a view of a view is a view of the parent
    mirror = _surface_view(net.view("bicubic", "mirror"), 1)
    shaped = _surface_view(net.view("bilinear", "keep", 0.5, 0.25, "translation"), 1)
    try:
        assert [lib.dvsg_locnet_render_surface(h) for h in (p010, back, net.handle, net.view("bicubic", "mirror"), mirror)] == \
            [1, 0, 0, 0, 1]
        assert (lib.dvsg_locnet_render_filter(mirror), lib.dvsg_locnet_render_border(mirror)) == (1, 2)   # inherited
        assert (lib.dvsg_locnet_render_filter(p010), lib.dvsg_locnet_render_border(p010)) == (0, 0)
        m, s, r = ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
        lib.dvsg_locnet_render_shape(shaped, ctypes.byref(m), ctypes.byref(s), ctypes.byref(r))
        assert (m.value, s.value, r.value, lib.dvsg_locnet_render_border(shaped)) == (2, 0.5, 0.25, 3)
        assert lib.dvsg_locnet_destroy(net.handle) == -1 and b"view" in lib.dvsg_last_error_string()
        # argument checks, before any device work: T keeps its NaN
        F = _dev(vectors())
        T = torch.full((2, 2, 28), float("nan"), device="cuda")
        buf = torch.zeros(4 * 9 * 32 + 8, dtype=torch.uint8, device="cuda")
        out = torch.full_like(buf, POISON)
        y, o = buf.data_ptr(), out.data_ptr()
        assert y % 4 == 0 and o % 4 == 0

        def status(pitch=2 * W, opitch=2 * W, dy=0, duv=0, doy=0, douv=0, stride=9 * 2 * W):
            return lib.dvsg_tps_render_nv12(p010, F.data_ptr(), y + dy, y + H * pitch + duv, pitch, stride, 2, H, W, T.data_ptr(),
                                            o + doy, o + H * opitch + douv, opitch, 9 * opitch, _stream())
        for kw, word in ((dict(pitch=2 * W - 2), b"source pitch=14 < 2 W = 16"), (dict(opitch=2 * W - 2), b"output pitch=14"),
                         (dict(pitch=2 * W + 1), b"source pitch=17 is odd"), (dict(opitch=2 * W + 3), b"output pitch=19 is odd"),
                         (dict(dy=1), b"source y plane pointer"), (dict(duv=1), b"source uv plane pointer"),
                         (dict(doy=1), b"output y plane pointer"), (dict(douv=1), b"output uv plane pointer"),
                         (dict(stride=9 * 2 * W + 1), b"source frame_stride")):
            assert status(**kw) == -1, kw
            assert word in lib.dvsg_last_error_string(), (kw, lib.dvsg_last_error_string())
        zoom = _dev(np.float32(ZOOM))
        assert lib.dvsg_tps_render_zoom_nv12(p010, F.data_ptr(), y, y + H * 14, 14, 9 * 14, 2, H, W, zoom.data_ptr(), T.data_ptr(), o,
                                             o + H * 16, 16, 9 * 16, _stream()) == -1
        assert b"dvsg_tps_render_zoom_nv12" in lib.dvsg_last_error_string() and b"pitch" in lib.dvsg_last_error_string()
        torch.cuda.synchronize()
        assert torch.isnan(T).all() and (out == POISON).all(), "a refused call did device work"
        assert status() == 0
        # the same network without the property still renders NV12, pitch = W included, with the parent's bytes
        nb, npre = nv12_ref.Batch(5, 2, H, W), nv12_ref.Batch(6, 2, H, W, W + 3)
        Tb, ob = render(back, vectors(), nb, None, npre, "nv12")
        Tp, op = render(net.handle, vectors(), nb, None, npre, "nv12")
        same_bits(Tb.cpu().numpy(), Tp.cpu().numpy(), "T")
        assert np.array_equal(ob, op)
        # dvsg_tps_render_u8 does not read it
        src = _dev(np.random.default_rng(8).integers(0, 256, (2, H, W, 3), dtype=np.uint8))
        for with_p, without in ((p010, net.handle), (mirror, net.view("bicubic", "mirror"))):
            a = B.render_u8(with_p, F, src, 0, None, True, True, W, 0)
            c = B.render_u8(without, F, src, 0, None, True, True, W, 0)
            same_bits(a[0].cpu().numpy(), c[0].cpu().numpy(), "T of dvsg_tps_render_u8")
            same_bits(a[1], c[1], "out_f32")
            same_bits(a[2], c[2], "out_u8")
        Tc = torch.empty((2, 2, 28), device="cuda")
        _call("dvsg_tps_coefficients_f32", shaped, F.data_ptr(), 2, Tc.data_ptr(), _stream())
        Td = torch.empty((2, 2, 28), device="cuda")
        _call("dvsg_tps_coefficients_f32", net.view("bilinear", "keep", 0.5, 0.25, "translation"), F.data_ptr(), 2, Td.data_ptr(),
              _stream())
        torch.cuda.synchronize()
        same_bits(Tc.cpu().numpy(), Td.cpu().numpy(), "dvsg_tps_coefficients_f32")
    finally:
        for v in (p010, back, mirror, shaped):
            lib.dvsg_locnet_destroy(v)


# ---------------------------------------------------------------------------------------------------------------------
# 5. online, 6. pipes: model 38 x 54, the 9-channel synthetic checkpoint with skip_length (0, 2, 3)
# ---------------------------------------------------------------------------------------------------------------------
MODEL, SKIP = (38, 54), (0, 2, 3)
SIZES = [(20, 32), (64, 96)]


def model():
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if "model" not in _CACHE:
        m = StabNet(*MODEL).load_weights(make_synthetic_weights(seed=0, c_in=3 * len(SKIP)))
        m.get_evaluation_model(len(SKIP))
        m.precision = "f32"
        _CACHE["model"] = m
    return _CACHE["model"]


def clips():
    """per size: (NV12 clip [9, 3 H0 / 2, W0], P010 clip uint8 [9, 3 H0 / 2, 2 W0] whose words' high bytes are the NV12 clip's
    and whose next two bits are seeded: all ten bits are used)"""
    if "clips" not in _CACHE:
        out = []
        for i, (H0, W0) in enumerate(SIZES):
            nv12 = nv12_ref.smooth_batch(800 + i, 9, H0, W0).buf
            two = np.random.default_rng(810 + i).integers(0, 4, nv12.shape, dtype=np.uint16)
            words = (nv12.astype(np.uint16) << 8) | (two << 6)
            out.append((nv12, words.astype("<u2").view(np.uint8).reshape(9, 3 * H0 // 2, 2 * W0)))
        _CACHE["clips"] = out
    return _CACHE["clips"]


def test_online_p010():
    """The pool, F_t and the crop state are those of an NV12 run fed the words' high bytes; each output is a direct render
    through the P010 view with the step's F_t row and the stream's zoom; uint16 in gives uint16 out."""
    torch = _torch()
    from coupe.dvsg_amd.online import OnlineStabilizer
    m = model()
    kw = dict(max_streams=2, skip_length=SKIP, crop="auto", yuv_matrix="bt601")
    on, off = OnlineStabilizer(m, frame_format="p010", **kw), OnlineStabilizer(m, frame_format="nv12", **kw)
    on.pool.zero_()
    off.pool.zero_()
    sid_on, sid_off = [on.open(), on.open()], [off.open(), off.open()]
    view = m.locnet.view(surface="p010")
    outs = [[], []]
    for k in range(9):
        dev = [_dev(c[1][k]) for c in clips()]
        res = on.step({sid_on[i]: dev[i] for i in range(2)})
        off.step({sid_off[i]: _dev(clips()[i][0][k]) for i in range(2)})
        same_bits(on._F.cpu().numpy(), off._F.cpu().numpy(), "F_t of step %d" % k)
        same_bits(on.pool.cpu().numpy(), off.pool.cpu().numpy(), "pool after step %d" % k)
        for row, i in enumerate(sorted(range(2), key=lambda i: SIZES[i])):   # batch order: by source size
            H0, W0 = SIZES[i]
            a, c = on.crop_state(sid_on[i]), off.crop_state(sid_off[i])
            assert a["zoom"] == c["zoom"] and a["free"] == c["free"], "crop state of stream %d, step %d" % (i, k)
            got = res[sid_on[i]]
            assert isinstance(got, torch.Tensor) and tuple(got.shape) == (3 * H0 // 2, 2 * W0) and got.dtype == torch.uint8
            one = p010_ref.P010Batch(0, 1, H0, W0, fill=POISON)
            one.buf[:] = clips()[i][1][k]
            _, alone = render(view, on._F[row:row + 1].cpu().numpy(), one, _dev(np.float32([a["zoom"]])),
                              p010_ref.P010Batch(0, 1, H0, W0, fill=POISON))
            assert np.array_equal(got.cpu().numpy(), alone[0]), "output of stream %d, step %d" % (i, k)
            outs[i].append(got.cpu().numpy())
    assert on.crop_state(sid_on[1])["zoom"] < 1.0
    # NumPy uint16 in -> NumPy uint16 out, the same bits
    host = OnlineStabilizer(m, frame_format="p010", **kw)
    sid = host.open()
    for k in range(4):
        got = host.push(sid, clips()[0][1][k].view("<u2"))
        assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and got.shape == (30, 32)
        assert np.array_equal(got.view(np.uint8), outs[0][k]), "uint16 frame %d" % k
    with pytest.raises(ValueError, match="odd"):
        host.push(sid, np.zeros((30, 62), np.uint8))


def run_pipes(sources, sinks, **kw):
    from coupe.dvsg_amd.pipe import stabilize_pipes
    box = {}

    def target():
        try:
            _torch().cuda.set_device(0)
            box["stats"] = stabilize_pipes(model(), sources, sinks, skip_length=SKIP, **kw)
        except BaseException as e:
            box["error"] = e
    model()
    t = threading.Thread(target=target, name="test-caller")
    t.start()
    t.join(60.0)
    assert not t.is_alive(), "stabilize_pipes did not return"
    if "error" in box:
        raise box["error"]
    return box["stats"]


def test_pipes_ten_bit():
    """One C420p10 source, depth 3: the output is stabilize_clips(frame_format="p010") on the repacked frames, byte for byte
    after the repack, under a header that repeats C420p10 and the X tags; raw P010 in and out gives the same frames."""
    torch = _torch()
    from coupe.dvsg_amd import y4m
    from coupe.dvsg_amd.online import stabilize_clips
    H0, W0 = SIZES[0]
    p010 = clips()[0][1]
    want = stabilize_clips(model(), [p010], frame_format="p010", skip_length=SKIP, yuv_matrix=y4m.default_yuv_matrix(H0))[0]
    assert want.dtype == np.uint8 and want.shape == p010.shape and not np.array_equal(want, p010)
    planar = y4m.p010_to_i420p10(torch.from_numpy(p010.copy())).numpy()
    head = b"YUV4MPEG2 W32 H20 F30000:1001 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\n"
    src = y4m.Y4MReader(io.BytesIO(head + b"".join(b"FRAME\n" + f.tobytes() for f in planar)), depths=(8, 10))
    out = io.BytesIO()
    snk = y4m.Y4MWriter(out, W0, H0, src.fps, aspect=src.aspect, colorspace=src.colorspace, tags=src.tags, interlace=src.interlace)
    stats = run_pipes([src], [snk], depth=3)
    assert stats[0]["frames"] == 9 and stats[0]["high_water"] <= 3
    data = out.getvalue()
    assert data.startswith(head)
    got = np.stack(list(y4m.Y4MReader(io.BytesIO(data), depths=(8, 10))))
    assert np.array_equal(y4m.i420p10_to_p010(torch.from_numpy(got)).numpy(), want)
    raw = io.BytesIO()
    stats = run_pipes([y4m.RawP010Reader(io.BytesIO(p010.tobytes()), W0, H0)], [y4m.RawP010Writer(raw, W0, H0)], depth=3)
    assert stats[0]["frames"] == 9 and raw.getvalue() == want.tobytes()
