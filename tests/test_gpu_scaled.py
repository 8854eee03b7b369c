"""GPU: the renders at a delivery size (include/dvsg_amd.h, "Output size") -- a view of dvsg_locnet_view_create_scaled given to
dvsg_tps_render_u8, dvsg_tps_render_zoom_u8, dvsg_tps_render_nv12 and dvsg_tps_render_zoom_nv12 -- against their NumPy
restatement tests/scaled_ref.py, bit for bit: out_f32 bits, bytes and P010 words, no tolerance.  x_s, y_s of the virtual
samples come from the grid-only form of dvsg_tps_warp_zoom_f32 at each plane's VIRTUAL grid, as the header defines them.
Every render writes into outputs pre-filled with a sentinel, so what must not be written is visible.  Synthetic weights, f32.

Then OnlineStabilizer(out_size=...) and stabilize_pipes(out_size=...) against the direct render calls."""
import ctypes
import io

import numpy as np
import pytest

import bicubic_ref as R
import inputs
import nv12_ref
import p010_ref
import scaled_ref as S

pytestmark = pytest.mark.gpu

POISON = 0xA5
F32 = np.float32
FILTERS = ("bilinear", "bicubic")
BORDERS = ("black", "replicate", "mirror")
OUT_SIZES = ((12, 20), (8, 14), (6, 10), (24, 10), (36, 60))    # of a (24, 40) source: factors 2x2, 3x3, 4x4, 1x4, 1x1
SURFACE_CASES = [((24, 40), o) for o in OUT_SIZES] + [((26, 44), (12, 20))]   # the last: 3x3, a ratio that does not divide
U8_PAD, U8_X0 = 5, 2


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _lib():
    from coupe.dvsg_amd import _lib
    return _lib


def _call(name, *args):
    _lib().call(name, *args, _stream())


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def net(synthetic_weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype,
                                                                                            want.shape, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32) if got.dtype == np.float32 else got != want
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %r want %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def vectors(seed=5):
    """F_t of two frames: a uniform shift of (+0.45, -0.35) plus +-0.05 per point -- a wide band of invalid samples on two
    sides -- and +-0.25 per point"""
    rng = np.random.default_rng(seed)
    F = np.zeros((2, 25, 2), F32)
    F[0, :, 0], F[0, :, 1] = 0.45, -0.35
    F[0] += rng.uniform(-0.05, 0.05, (25, 2)).astype(F32)
    F[1] = rng.uniform(-0.25, 0.25, (25, 2))
    return F


def zooms():
    """zoom absent, and per frame 1.0 / 0.8"""
    return (None, _dev(np.array([1.0, 0.8], F32)))


def grid(T, zoom, n, gh, gw):
    """x_s, y_s [n, gh, gw] of the grid-only dvsg_tps_warp_zoom_f32 (U == NULL, out == NULL) with coord = V_src"""
    torch = _torch()
    V = _dev(inputs.v_src(n))
    xs = torch.empty((n, gh, gw), device="cuda")
    ys = torch.empty_like(xs)
    _call("dvsg_tps_warp_zoom_f32", None, _ptr(V), _ptr(T), _ptr(zoom), n, 1, 1, 3, 25, gh, gw, None, _ptr(xs), _ptr(ys))
    return xs.cpu().numpy(), ys.cpu().numpy()


def check_coverage(counts, total):
    """the reference shows an output pixel with all sub-samples valid, one with none and -- where a pixel has more than one -- a
    mixed one"""
    c = np.concatenate([np.asarray(x).ravel() for x in counts])
    assert (c == total).any(), "no output pixel with all %d sub-samples valid" % total
    assert (c == 0).any(), "no output pixel with all sub-samples invalid"
    assert total == 1 or ((c > 0) & (c < total)).any(), "no output pixel with valid and invalid sub-samples"


# ---------------------------------------------------------------------------------------------------------------------
# one launch of each format into pre-filled outputs
# ---------------------------------------------------------------------------------------------------------------------
def rgb_source(n, H, W):
    return np.random.default_rng(100 * H + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def rgb_render(handle, F, src, flip, zoom, oh, ow, status=False):
    """-> (T, out_f32 [n,oh,ow,3], the whole uint8 image [n,oh,ow + U8_PAD,3], the two tails behind the outputs)"""
    torch = _torch()
    n, H, W = src.shape[:3]
    T = torch.full((n, 2, 28), float("nan"), device="cuda")
    nf, nu = n * oh * ow * 3, n * oh * (ow + U8_PAD) * 3
    f32 = torch.full((nf + 64,), 7.0, device="cuda")
    u8 = torch.full((nu + 64,), POISON, dtype=torch.uint8, device="cuda")
    Fd, srcd = _dev(F), _dev(src)
    args = [handle, _ptr(Fd), _ptr(srcd), n, H, W, flip]
    if zoom is not None:
        args.append(_ptr(zoom))
    args += [_ptr(T), _ptr(f32), _ptr(u8), ow + U8_PAD, U8_X0, _stream()]
    name = "dvsg_tps_render_zoom_u8" if zoom is not None else "dvsg_tps_render_u8"
    if status:
        rc = getattr(_lib().load(), name)(*args)
        err = _lib().load().dvsg_last_error_string()
    else:
        _lib().call(name, *args)
    torch.cuda.synchronize()
    assert (f32[nf:] == 7.0).all() and (u8[nu:] == POISON).all(), "bytes behind an output were written"
    res = (T.cpu().numpy(), f32[:nf].view(n, oh, ow, 3).cpu().numpy(), u8[:nu].view(n, oh, ow + U8_PAD, 3).cpu().numpy())
    return (rc, err) + res if status else (T,) + res[1:]


def surface_render(handle, F, b, zoom, ob, status=False):
    """b, ob: nv12_ref.Batch or p010_ref.P010Batch of the source and of the pre-filled output -> (T, the output buffer)"""
    torch = _torch()
    T = torch.full((b.n, 2, 28), float("nan"), device="cuda")
    buf, Fd = _dev(b.buf), _dev(F)
    out = torch.cat([_dev(ob.buf).reshape(-1), torch.full((64,), POISON, dtype=torch.uint8, device="cuda")])
    args = [handle, _ptr(Fd), _ptr(buf), _ptr(buf) + b.uv_offset, b.pitch, b.frame_stride, b.n, b.H, b.W]
    if zoom is not None:
        args.append(_ptr(zoom))
    args += [_ptr(T), _ptr(out), _ptr(out) + ob.uv_offset, ob.pitch, ob.frame_stride, _stream()]
    name = "dvsg_tps_render_zoom_nv12" if zoom is not None else "dvsg_tps_render_nv12"
    if status:
        rc = getattr(_lib().load(), name)(*args)
        err = _lib().load().dvsg_last_error_string()
    else:
        _lib().call(name, *args)
    torch.cuda.synchronize()
    assert (out[ob.buf.size:] == POISON).all(), "bytes behind the output were written"
    got = out[:ob.buf.size].view(ob.buf.shape).cpu().numpy()
    return (rc, err, T.cpu().numpy(), got) if status else (T, got)


def surface_batches(p010, H, W, oh, ow, n=2):
    """a seeded source with a pitch above its width and a UV plane behind a gap, and a poisoned output likewise"""
    if p010:
        return (p010_ref.P010Batch(H * 31 + W, n, H, W, pitch=2 * W + 6, uv_row=H + 1, tail=1, low=0x15),
                p010_ref.P010Batch(0, n, oh, ow, pitch=2 * ow + 10, uv_row=oh + 2, tail=1, fill=POISON))
    return nv12_ref.Batch(H * 31 + W, n, H, W, W + 3, H + 1), nv12_ref.Batch(0, n, oh, ow, ow + 5, oh + 2, fill=POISON)


def surface_planes(batch, p010, buf=None):
    """(luma [n, H, W, 1], chroma [n, H / 2, W / 2, 2]) of a batch's buffer, bytes or words"""
    if p010:
        return batch.words(buf)
    y, uv = batch.planes(buf)
    return y[..., None], uv.reshape(batch.n, batch.H // 2, batch.W // 2, 2)


def coefficients(handle, F):
    """T of dvsg_tps_coefficients_f32: what every render writes for F_t (each render's own T is compared with it)"""
    T = _torch().full((len(F), 2, 28), float("nan"), device="cuda")
    Fd = _dev(F)
    _call("dvsg_tps_coefficients_f32", handle, _ptr(Fd), len(F), _ptr(T))
    _torch().cuda.synchronize()
    return T


def expected_planes(b, p010, T, zoom, oh, ow, border, bicubic):
    """the two planes of every frame by the restatement, and the valid counts of their output samples"""
    sy, sx = S.factors((b.H, b.W), (oh, ow))
    want, counts = [], []
    for chroma, plane in enumerate(surface_planes(b, p010)):
        ph, pw = plane.shape[1:3]
        po, qo = (oh // 2, ow // 2) if chroma else (oh, ow)
        xs, ys = grid(T, zoom, b.n, sy * po, sx * qo)
        want.append(np.stack([S.render(plane[i], xs[i], ys[i], sy, sx, border, bicubic, bool(chroma), p010)[1]
                              for i in range(b.n)]))
        counts += [S.coverage((ph, pw), xs[i], ys[i], sy, sx) for i in range(b.n)]
    return want, counts, sy * sx


# ---------------------------------------------------------------------------------------------------------------------
# 6. identity: a scaled view at the source's size, or (0, 0), is the view without the property
# ---------------------------------------------------------------------------------------------------------------------
def _scaled_zero(inner):
    v = ctypes.c_void_p()
    _lib().call("dvsg_locnet_view_create_scaled", inner, 0, 0, ctypes.byref(v))
    return v


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("border", BORDERS + ("keep",))
def test_identity_rgb(net, filt, border):
    H, W = 24, 40
    src, F = rgb_source(2, H, W), vectors()
    plain, zero = net.view(filt, border), _scaled_zero(net.view(filt, border))
    try:
        for zoom in zooms():
            want = rgb_render(plain, F, src, 1, zoom, H, W)
            for name, view in (("(H, W)", net.view(filt, border, out_size=(H, W))), ("(0, 0)", zero)):
                got = rgb_render(view, F, src, 1, zoom, H, W)
                for g, w, what in zip(got, want, ("T", "out_f32", "out_u8")):
                    same(g.cpu().numpy() if what == "T" else g, w.cpu().numpy() if what == "T" else w,
                         "%s %s size %s zoom=%s %s" % (filt, border, name, zoom is not None, what))
    finally:
        _lib().load().dvsg_locnet_destroy(zero)


@pytest.mark.parametrize("p010", [False, True], ids=["nv12", "p010"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("border", BORDERS + ("keep",))
def test_identity_surfaces(net, filt, border, p010):
    H, W = 24, 40
    surface = "p010" if p010 else "nv12"
    b, ob = surface_batches(p010, H, W, H, W)
    F = vectors()
    plain, zero = net.view(filt, border, surface=surface), _scaled_zero(net.view(filt, border, surface=surface))
    try:
        for zoom in zooms():
            T0, want = surface_render(plain, F, b, zoom, ob)
            for name, view in (("(H, W)", net.view(filt, border, surface=surface, out_size=(H, W))), ("(0, 0)", zero)):
                T1, got = surface_render(view, F, b, zoom, ob)
                what = "%s %s %s size %s zoom=%s" % (surface, filt, border, name, zoom is not None)
                same(T1.cpu().numpy(), T0.cpu().numpy(), what + " T")
                same(got, want, what)
            assert (want != POISON).any()
    finally:
        _lib().load().dvsg_locnet_destroy(zero)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the rule, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _check_rgb(net, H, W, oh, ow, filt, border, flip):
    bicubic = filt == "bicubic"
    src, F = rgb_source(2, H, W), vectors()
    view = net.view(filt, border, out_size=(oh, ow))
    sy, sx = S.factors((H, W), (oh, ow))
    # the reference first: its inputs show an all-valid, an all-invalid and a mixed output pixel before anything is compared
    Tp = coefficients(net.view(filt, border), F)
    grids = [grid(Tp, zoom, 2, sy * oh, sx * ow) for zoom in zooms()]
    check_coverage([S.coverage((H, W), xs[i], ys[i], sy, sx) for xs, ys in grids for i in range(2)], sy * sx)
    want = [[S.render(src[i], xs[i], ys[i], sy, sx, border, bicubic) for i in range(2)] for xs, ys in grids]
    for zoom, w in zip(zooms(), want):
        T, f32, u8 = rgb_render(view, F, src, flip, zoom, oh, ow)
        same(T.cpu().numpy(), Tp.cpu().numpy(), "T")
        what = "rgb %dx%d -> %dx%d %s %s zoom=%s" % (H, W, oh, ow, filt, border, zoom is not None)
        for i in range(2):
            wf, wu = w[i]
            same(f32[i], wf[..., ::-1] if flip else wf, what + " out_f32 frame %d" % i)
            same(u8[i, :, U8_X0:U8_X0 + ow], wu, what + " out_u8 frame %d" % i)
        assert (np.delete(u8, np.s_[U8_X0:U8_X0 + ow], axis=2) == POISON).all(), what + ": columns outside were written"


@pytest.mark.parametrize("out", OUT_SIZES)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("border", BORDERS)
def test_rule_rgb(net, border, filt, out):
    _check_rgb(net, 24, 40, out[0], out[1], filt, border, flip=1 if out == (8, 14) else 0)


def _check_surface(net, p010, H, W, oh, ow, filt, border):
    surface = "p010" if p010 else "nv12"
    b, ob = surface_batches(p010, H, W, oh, ow)
    F = vectors()
    view = net.view(filt, border, surface=surface, out_size=(oh, ow))
    # the reference first, as in _check_rgb
    Tp = coefficients(net.view(filt, border), F)
    refs = [expected_planes(b, p010, Tp, zoom, oh, ow, border, filt == "bicubic") for zoom in zooms()]
    check_coverage([c for _, counts, _ in refs for c in counts], refs[0][2])
    for zoom, (want, _, _) in zip(zooms(), refs):
        T, out = surface_render(view, F, b, zoom, ob)
        same(T.cpu().numpy(), Tp.cpu().numpy(), "T")
        what = "%s %dx%d -> %dx%d %s %s zoom=%s" % (surface, H, W, oh, ow, filt, border, zoom is not None)
        for got, w, name in zip(surface_planes(ob, p010, out), want, ("luma", "chroma")):
            same(got, w, what + " " + name)
        assert (ob.outside(out) == POISON).all(), what + ": bytes beyond the width or between the planes were written"


@pytest.mark.parametrize("p010", [False, True], ids=["nv12", "p010"])
@pytest.mark.parametrize("src, out", SURFACE_CASES)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("border", BORDERS)
def test_rule_surfaces(net, border, filt, src, out, p010):
    _check_surface(net, p010, src[0], src[1], out[0], out[1], filt, border)


# ---------------------------------------------------------------------------------------------------------------------
# 8. tile seams: more than one column tile; output rows that are no multiple of the row tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt, border", [("bilinear", "black"), ("bicubic", "mirror"), ("bilinear", "replicate")])
def test_tile_seams(net, filt, border):
    _check_rgb(net, 16, 520, 8, 260, filt, border, 0)
    _check_rgb(net, 38, 24, 19, 12, filt, border, 0)
    for p010 in (False, True):
        _check_surface(net, p010, 16, 520, 8, 260, filt, border)


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals: a status, nothing launched
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(net):
    lib = _lib().load()
    F = vectors()
    src = rgb_source(2, 24, 40)
    for out, word in (((4, 20), b"out_H=4"), ((12, 7), b"out_W=7")):     # factor 6 and factor 6: above 4 on each axis
        rc, err, T, f32, u8 = rgb_render(net.view(out_size=out), F, src, 0, None, out[0], out[1], status=True)
        assert rc == -1 and word in err and b"4x" in err, err
        assert np.isnan(T).all() and (f32 == 7.0).all() and (u8 == POISON).all(), "a refused render wrote something"
        b, ob = surface_batches(False, 24, 40, *((4, 20) if out == (4, 20) else (12, 6)))
        rc, err, T, got = surface_render(net.view(out_size=(ob.H, ob.W)), F, b, None, ob, status=True)
        assert rc == -1 and (b"out_H=4" if out == (4, 20) else b"out_W=6") in err, err
        assert np.isnan(T).all() and (got == POISON).all()
    # factor 5 exactly, the first one refused, on each axis: RGB 24 -> 5 rows and 40 -> 8 columns, either entry point
    for out, word in (((5, 20), b"out_H=5"), ((12, 8), b"out_W=8")):
        assert S.factors((24, 40), out) in ((5, 2), (2, 5))
        for zoom in zooms():
            rc, err, T, f32, u8 = rgb_render(net.view(out_size=out), F, src, 0, zoom, out[0], out[1], status=True)
            assert rc == -1 and word in err and b"5x" in err and b"4x" in err, err
            assert np.isnan(T).all() and (f32 == 7.0).all() and (u8 == POISON).all(), "a refused render wrote something"
    # NV12 and P010, even sizes: 26 -> 6 rows of a (26, 44) source, 40 -> 8 columns of a (24, 40) source
    for (H, W), out, word in (((26, 44), (6, 22), b"out_H=6"), ((24, 40), (12, 8), b"out_W=8")):
        assert S.factors((H, W), out) in ((5, 2), (2, 5))
        for p010 in (False, True):
            b, ob = surface_batches(p010, H, W, out[0], out[1])
            view = net.view(surface="p010" if p010 else "nv12", out_size=out)
            for zoom in zooms():
                rc, err, T, got = surface_render(view, F, b, zoom, ob, status=True)
                assert rc == -1 and word in err and b"5x" in err and b"4x" in err, err
                assert np.isnan(T).all() and (got == POISON).all(), "a refused render wrote something"
    # ... and factor 4 on each axis is served (24 -> 6 rows, 40 -> 10 columns: test_rule_* compare those renders)
    assert S.factors((24, 40), (6, 10)) == (4, 4)
    # keep at another size (at the source's size it renders: test_identity_*)
    rc, err, T, f32, u8 = rgb_render(net.view(border="keep", out_size=(12, 20)), F, src, 0, None, 12, 20, status=True)
    assert rc == -1 and b"DVSG_BORDER_KEEP" in err and np.isnan(T).all() and (f32 == 7.0).all()
    b, ob = surface_batches(False, 24, 40, 12, 20)
    rc, err, T, got = surface_render(net.view(border="keep", out_size=(12, 20)), F, b, _dev(np.ones(2, F32)), ob, status=True)
    assert rc == -1 and b"DVSG_BORDER_KEEP" in err and b"dvsg_tps_render_zoom_nv12" in err and (got == POISON).all()
    # odd NV12 output sizes: refused by the render (the view itself may be odd: RGB renders through it)
    for out, word in (((13, 20), b"out_H=13"), ((12, 21), b"out_W=21"), ((2, 20), b"out_H=2")):
        view = net.view(out_size=out)
        ob = nv12_ref.Batch(0, 2, 14, 22, fill=POISON)
        rc, err, T, got = surface_render(view, F, surface_batches(False, 24, 40, 12, 20)[0], None, ob, status=True)
        assert rc == -1 and word in err, err
        assert np.isnan(T).all() and (got == POISON).all()
    # the constructor
    v = ctypes.c_void_p()
    assert lib.dvsg_locnet_view_create_scaled(net.handle, 0, 7, ctypes.byref(v)) == -1 and not v.value
    assert b"out_H=0" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create_scaled(net.handle, 7, 0, ctypes.byref(v)) == -1 and b"out_W=0" in lib.dvsg_last_error_string()


def _size(handle):
    h, w = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib().load().dvsg_locnet_render_size(handle, ctypes.byref(h), ctypes.byref(w)) == 0
    return h.value, w.value


def test_view_rules_and_render_size(net):
    lib = _lib().load()
    made = []

    def make(name, *args):
        v = ctypes.c_void_p()
        _lib().call(name, *args, ctypes.byref(v))
        made.append(v)
        return v
    try:
        assert _size(None) == (0, 0) and _size(net.handle) == (0, 0)
        cubic = make("dvsg_locnet_view_create_border", net.handle, 1, 2)
        scaled = make("dvsg_locnet_view_create_scaled", cubic, 12, 20)
        assert _size(scaled) == (12, 20) and lib.dvsg_locnet_render_filter(scaled) == 1 and lib.dvsg_locnet_render_border(scaled) == 2
        p010 = make("dvsg_locnet_view_create_surface", scaled, 1)
        assert _size(p010) == (12, 20) and lib.dvsg_locnet_render_surface(p010) == 1 and lib.dvsg_locnet_render_filter(p010) == 1
        again = make("dvsg_locnet_view_create_scaled", p010, 6, 10)     # a view of a view: of the parent, surface inherited
        assert _size(again) == (6, 10) and lib.dvsg_locnet_render_surface(again) == 1 and lib.dvsg_locnet_render_border(again) == 2
        back = make("dvsg_locnet_view_create_scaled", again, 0, 0)
        assert _size(back) == (0, 0)
        for name, args in (("dvsg_locnet_view_create", (scaled, 1)), ("dvsg_locnet_view_create_border", (scaled, 0, 1)),
                           ("dvsg_locnet_view_create_shaped", (scaled, 0, 0, 0, ctypes.c_float(0.5), ctypes.c_float(0.0)))):
            assert _size(make(name, *args)) == (0, 0), name
        # every view is the parent's: the parent is not destroyed while one lives, and a view does not calibrate
        assert lib.dvsg_locnet_destroy(net.handle) == -1 and b"view" in lib.dvsg_last_error_string()
        x = _torch().zeros((1, 32, 48, 21), device="cuda")
        assert lib.dvsg_locnet_calibrate_f16(scaled, _ptr(x), 1, 32, 48, _ptr(x), 8, _stream()) == -1
        assert b"view" in lib.dvsg_last_error_string()
        # the scan and the coefficient call do not read the size
        F = _dev(vectors())
        T0, T1 = _torch().empty((2, 2, 28), device="cuda"), _torch().empty((2, 2, 28), device="cuda")
        _call("dvsg_tps_coefficients_f32", cubic, _ptr(F), 2, _ptr(T0))
        _call("dvsg_tps_coefficients_f32", scaled, _ptr(F), 2, _ptr(T1))
        same(T1.cpu().numpy(), T0.cpu().numpy(), "dvsg_tps_coefficients_f32 through a scaled view")
        # ... nor does the coverage scan, which takes its grid as arguments: T, n_border and key_min through the scaled view
        # (size (12, 20)) are those through the view it was made from, on a grid that is neither size
        torch = _torch()
        zoom = _dev(np.array([1.0, 0.8], F32))
        need = ctypes.c_size_t()
        _lib().call("dvsg_tps_coverage_workspace_bytes", 2, 30, 50, ctypes.byref(need))
        scans = []
        for handle in (cubic, scaled, p010):
            ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
            Ts = torch.full((2, 2, 28), float("nan"), device="cuda")
            keys = torch.full((2, 2), -1, dtype=torch.int32, device="cuda")
            _call("dvsg_tps_coverage_net_f32", handle, _ptr(F), _ptr(zoom), 2, 24, 40, 30, 50, _ptr(Ts), _ptr(keys[0]),
                  _ptr(keys[1]), _ptr(ws), ws.numel() * 8)
            torch.cuda.synchronize()
            scans.append((Ts.cpu().numpy(), keys.cpu().numpy()))
        assert (scans[0][1][0] > 0).any(), "the scan found a border to count"
        for Ts, keys in scans[1:]:
            same(Ts, scans[0][0], "T of dvsg_tps_coverage_net_f32 through a scaled view")
            same(keys, scans[0][1], "n_border, key_min of dvsg_tps_coverage_net_f32 through a scaled view")
    finally:
        for v in reversed(made):
            lib.dvsg_locnet_destroy(v)


# ---------------------------------------------------------------------------------------------------------------------
# 10. OnlineStabilizer(out_size=...)
# ---------------------------------------------------------------------------------------------------------------------
def _model(weights, H, W):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights)
    model.get_evaluation_model(7)
    model.precision = "f32"
    return model


def _equal(got, want, what):
    torch = _torch()
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s against %s" % (what, tuple(got.shape), tuple(want.shape))
    if got.dtype.is_floating_point:
        got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    assert torch.equal(got, want), "%s: %d values differ" % (what, int((got != want).sum()))


def _scan(model, F1, zoom, src, grid_hw):
    """n_border, key_min of dvsg_tps_coverage_net_f32 for one frame"""
    torch = _torch()
    need = ctypes.c_size_t()
    _lib().call("dvsg_tps_coverage_workspace_bytes", 1, grid_hw[0], grid_hw[1], ctypes.byref(need))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
    T = torch.empty((1, 2, 28), device="cuda")
    keys = torch.empty((2,), dtype=torch.int32, device="cuda")
    _call("dvsg_tps_coverage_net_f32", model.locnet.handle, _ptr(F1), _ptr(zoom), 1, src[0], src[1], grid_hw[0], grid_hw[1],
          _ptr(T), _ptr(keys[0:1]), _ptr(keys[1:2]), _ptr(ws), ws.numel() * 8)
    return (int(v) for v in keys.tolist())


def _online(synthetic_weights, fmt, crop):
    import ratchet_ref
    torch = _torch()
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(synthetic_weights, 32, 48)
    surface = fmt == "nv12"
    sizes, out_size, N = [(40, 60), (24, 40)], (12, 20), 4
    if surface:
        clips = [_dev(nv12_ref.smooth_batch(900 + i, N, H0, W0).buf) for i, (H0, W0) in enumerate(sizes)]
        kw = dict(frame_format="nv12")
    else:
        clips = [_dev((inputs.smooth_frames(31 + i, N, H0, W0) * 255).astype(np.uint8)) for i, (H0, W0) in enumerate(sizes)]
        kw = dict(source_res=True, as_uint8=True)
    on = OnlineStabilizer(model, max_streams=2, out_size=out_size, crop=crop, **kw)
    off = OnlineStabilizer(model, max_streams=2, **kw)
    on.pool.zero_()
    off.pool.zero_()
    sid_on, sid_off = [on.open(), on.open()], [off.open(), off.open()]
    order = sorted(range(2), key=lambda i: ((0,) + sizes[i]) if not surface else sizes[i])   # batch order: by source size
    oh, ow = out_size
    view = model.locnet.view(surface="nv12", out_size=out_size)
    state = np.ones(2, F32)
    for k in range(N):
        res = on.step({sid_on[i]: clips[i][k] for i in range(2)})
        off.step({sid_off[i]: clips[i][k] for i in range(2)})
        _equal(on._F, off._F, "F_t of step %d" % k)
        _equal(on.pool, off.pool, "pool after step %d" % k)
        for row, i in enumerate(order):
            H0, W0 = sizes[i]
            F1 = on._F[row:row + 1].clone()
            sy, sx = S.factors((H0, W0), out_size)
            zoom = None
            if crop is not None:
                g = [((H0, W0), (sy * oh, sx * ow))] + ([((H0 // 2, W0 // 2), (sy * (oh // 2), sx * (ow // 2)))] if surface else [])
                keys = [list(_scan(model, F1, None, s, v))[1] for s, v in g]
                D = [(v[0] - 1) * (v[1] - 1) for _, v in g]
                z, free, _ = ratchet_ref.ratchet(state, [on._streams[sid_on[i]][0]], [keys[0]], D[0],
                                                 [keys[1]] if surface else None, D[1] if surface else 0,
                                                 margin=2.0 / (min(g[-1][1]) - 1))
                st = on.crop_state(sid_on[i])
                assert st["zoom"].tobytes() == z[0].tobytes() and st["free"] == free[0], (k, i, st, z, free)
                zoom = _dev(z)
                for s, v in g:      # no invalid virtual sample remains at the zoom the frame is rendered with
                    n_border = list(_scan(model, F1, zoom, s, v))[0]
                    print("step %d stream %d grid %s zoom %.4f: %d invalid virtual samples" % (k, i, v, z[0], n_border))
                    assert n_border == 0
            got = res[sid_on[i]]
            T = torch.empty((1, 2, 28), device="cuda")
            if surface:
                assert tuple(got.shape) == (3 * oh // 2, ow) and got.dtype == torch.uint8
                want = torch.full((1, 3 * oh // 2, ow), POISON, dtype=torch.uint8, device="cuda")
                srcf = clips[i][k][None].contiguous()
                args = [view, _ptr(F1), _ptr(srcf), _ptr(srcf) + H0 * W0, W0, 3 * H0 // 2 * W0, 1, H0, W0]
                args += [_ptr(zoom)] if crop is not None else []
                _call("dvsg_tps_render_zoom_nv12" if crop is not None else "dvsg_tps_render_nv12", *args, _ptr(T), _ptr(want),
                      _ptr(want) + oh * ow, ow, 3 * oh // 2 * ow)
            else:
                assert tuple(got.shape) == (oh, ow, 3) and got.dtype == torch.uint8
                want = torch.full((1, oh, ow, 3), POISON, dtype=torch.uint8, device="cuda")
                args = [view, _ptr(F1), _ptr(clips[i][k:k + 1]), 1, H0, W0, 0] + ([_ptr(zoom)] if crop is not None else [])
                _call("dvsg_tps_render_zoom_u8" if crop is not None else "dvsg_tps_render_u8", *args, _ptr(T), None, _ptr(want),
                      ow, 0)
            _equal(got, want[0], "%s output of stream %d, step %d" % (fmt, i, k))
    torch.cuda.synchronize()
    return model, clips, sizes, out_size


@pytest.mark.parametrize("crop", [None, "auto"])
@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_online_out_size(synthetic_weights, fmt, crop):
    """Two streams of different source sizes, 4 steps each: every output is the direct render call through
    LocNet.view(out_size=...) on that step's F_t; the pool and F_t are those of a run without out_size; with crop="auto" the
    zoom is the ratchet fed by the scan of the VIRTUAL grids and no invalid virtual sample remains at it."""
    _online(synthetic_weights, fmt, crop)


def test_online_out_size_p010_words(synthetic_weights):
    """P010 given as host uint16 words comes back as uint16 words of the delivery size, the direct render's through
    LocNet.view(surface="p010", out_size=...)"""
    torch = _torch()
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(synthetic_weights, 32, 48)
    (H0, W0), (oh, ow) = (24, 40), (12, 20)
    nv = nv12_ref.smooth_batch(960, 3, H0, W0).buf
    low = np.random.default_rng(1).integers(0, 4, nv.shape).astype(np.uint16)
    words = ((nv.astype(np.uint16) << 8) | (low << 6)).astype(np.uint16)      # 10-bit samples in the high bits
    on = OnlineStabilizer(model, frame_format="p010", out_size=(oh, ow))
    sid = on.open()
    view = model.locnet.view(surface="p010", out_size=(oh, ow))
    for k in range(3):
        got = on.push(sid, words[k])
        assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and got.shape == (3 * oh // 2, ow)
        src = _dev(np.ascontiguousarray(words[k]).view(np.uint8))[None].contiguous()
        want = torch.full((1, 3 * oh // 2, 2 * ow), POISON, dtype=torch.uint8, device="cuda")
        F1, T = on._F[:1].clone(), torch.empty((1, 2, 28), device="cuda")
        _call("dvsg_tps_render_nv12", view, _ptr(F1), _ptr(src), _ptr(src) + H0 * 2 * W0, 2 * W0, 3 * H0 // 2 * 2 * W0, 1, H0, W0,
              _ptr(T), _ptr(want), _ptr(want) + oh * 2 * ow, 2 * ow, 3 * oh // 2 * 2 * ow)
        same(got, want[0].cpu().numpy().view(np.uint16), "P010 output of step %d" % k)
        assert (got & 63 == 0).all() and len(np.unique(got)) > 8


def test_online_refusals_and_float_output(synthetic_weights):
    torch = _torch()
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(synthetic_weights, 32, 48)
    on = OnlineStabilizer(model, source_res=True, out_size=(12, 20))
    sid = on.open()
    frame = _dev((inputs.smooth_frames(3, 1, 40, 60)[0] * 255).astype(np.uint8))
    out = on.push(sid, frame)
    assert tuple(out.shape) == (12, 20, 3) and out.dtype == torch.float32
    with pytest.raises(ValueError, match="4x"):
        on.push(sid, _dev(np.zeros((61, 60, 3), np.uint8)))
    assert on._streams[sid][1] == 1, "a refused frame leaves the stream as it was"


# ---------------------------------------------------------------------------------------------------------------------
# 11. stabilize_pipes, memory to memory
# ---------------------------------------------------------------------------------------------------------------------
def test_pipe_out_size(synthetic_weights):
    """a 6-frame Y4M at (24, 40) with --out-size 20x12 -> a well-formed Y4M of that size whose frames are those of
    stabilize_clips(frame_format="nv12", out_size=(12, 20)) on the same frames"""
    torch = _torch()
    from coupe.dvsg_amd import pipe, y4m
    from coupe.dvsg_amd.online import stabilize_clips
    model = _model(synthetic_weights, 32, 48)
    nv12 = nv12_ref.smooth_batch(950, 6, 24, 40).buf
    i420 = y4m.nv12_to_i420(torch.from_numpy(nv12)).numpy()
    data = b"YUV4MPEG2 W40 H24 F25:1 Ip A1:1 C420jpeg\n" + b"".join(b"FRAME\n" + f.tobytes() for f in i420)
    args = pipe._arguments(["--synthetic-weights", "--out-size", "20x12"])
    src = y4m.Y4MReader(io.BytesIO(data))
    out = io.BytesIO()
    oh, ow = args.out_size
    sink = y4m.Y4MWriter(out, ow, oh, src.fps, aspect=pipe.output_aspect(src.aspect, (src.height, src.width), (oh, ow)),
                         colorspace=src.colorspace)
    stats = pipe.stabilize_pipes(model, [src], [sink], out_size=args.out_size)
    assert stats[0]["frames"] == 6
    r = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    frames = list(r)
    assert (r.width, r.height) == (20, 12) and r.aspect == (1, 1) and len(frames) == 6
    got = y4m.i420_to_nv12(torch.from_numpy(np.stack(frames))).numpy()
    want = stabilize_clips(model, [nv12], frame_format="nv12", out_size=(12, 20), yuv_matrix=y4m.default_yuv_matrix(24))[0]
    assert want.shape == (6, 18, 20)
    same(got, want, "the pipe's frames")
    assert len(np.unique(want)) > 8, "the frames carry a picture"
