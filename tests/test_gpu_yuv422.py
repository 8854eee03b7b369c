"""GPU: 4:2:2 frames (include/dvsg_amd.h, "Chroma sampling") -- the chroma format of a view, the two NV12 renders on NV16 and
P210 frames at source size and at a delivery size, OnlineStabilizer(frame_format="nv16" | "p210"), stabilize_clips and 4:2:2
pipes.  Everything compares bit for bit: whole buffers between guard bytes, outputs pre-filled with a poison byte, and
nothing beyond the used bytes of a row, between the planes or between the frames may change.

Luma is held to the SAME call through the same view without the property (the Y plane does not move); chroma to the
per-plane references of tests/border_ref.py, tests/p010_ref.py and tests/scaled_ref.py on the (H, W / 2) plane, with x_s, y_s
from the grid-only form of dvsg_tps_warp_zoom_f32.

Render shapes: (4, 4) -- the minimum, chroma 4 x 2; (6, 8) with an offset UV plane -- a chroma plane of one full and one
partial group of 4 rows, where 4:2:0 has a single partial one; (10, 520) -- chroma columns cross the 256-thread tile.  Three
frames per launch ("launch" of tests/test_gpu_border.py), zoom (1.0, 0.8, 0.6): one frame's zoom is exactly 1.0f."""
import ctypes
import io

import numpy as np
import pytest

import bicubic_ref as R
import border_ref
import nv12_ref
import p010_ref
import scaled_ref as S
import test_gpu_border as GB
import test_gpu_p010 as GP
import test_gpu_scaled as GS
import yuv422_ref as Y

pytestmark = pytest.mark.gpu

POISON = 0xA5
FILTERS = ("bilinear", "bicubic")
SURFACES = ("nv12", "p010")
FORMATS = {"nv12": "nv16", "p010": "p210"}
#          H   W   uv_row  low bits
SHAPES = [(4, 4, 4, 0), (6, 8, 9, 0x2B), (10, 520, 10, 0)]
_CACHE = {}

_dev, _call, _stream, grid, same_bits, render = GP._dev, GP._call, GP._stream, GP.grid, GP.same_bits, GP.render


def _torch():
    import torch
    return torch


def _lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def net(synthetic_weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def _poison(words):
    return np.uint16(POISON * 0x0101) if words else np.uint8(POISON)


def source(H, W, uv_row, low, words, n=3):
    """seeded frames with a pitch beyond the used bytes (bytes: odd), the UV plane at row uv_row and a row behind the frame"""
    return Y.Batch422(100 * H + W, n, H, W, words, pitch=(2 * W + 6) if words else (W + 3), uv_row=uv_row, tail=1, low=low)


def prefill(H, W, uv_row, words, n=3):
    """a poisoned output of another pitch, with its UV plane one row further down"""
    return Y.Batch422(0, n, H, W, words, pitch=(2 * W + 10) if words else (W + 5), uv_row=uv_row + 1, tail=2, fill=POISON)


def chroma_samples(plane, words):
    """the float32 image dvsg_tps_warp_f32 is given for a chroma plane, by the surface format's sample rule"""
    return p010_ref.samples(plane, True) if words else R.samples(np.asarray(plane), True, np.float32)


def chroma_bytes(v, bicubic, words):
    return p010_ref.to_word(v, True) if words else border_ref.to_u8(v, bicubic, True)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the render at source size
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoomed", [False, True])
@pytest.mark.parametrize("border", ["black", "replicate", "mirror", "keep"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("H,W,uv_row,low", SHAPES)
def test_render(net, H, W, uv_row, low, surface, filt, border, zoomed):
    torch = _torch()
    words, bicubic = surface == "p010", filt == "bicubic"
    b, pre = source(H, W, uv_row, low if words else 0, words), prefill(H, W, uv_row, words)
    F = GB.vectors("launch")
    zoom = _dev(np.float32(GB.ZOOM)) if zoomed else None
    assert GB.ZOOM[0] == 1.0
    with422, without = net.view(filt, border, surface=surface, chroma="422"), net.view(filt, border, surface=surface)
    assert _lib().dvsg_locnet_render_chroma(with422) == 1 and _lib().dvsg_locnet_render_chroma(without) == 0
    T, out = render(with422, F, b, zoom, pre, FORMATS[surface])
    what = "%s %s %s %dx%d zoom=%d" % (FORMATS[surface], filt, border, H, W, zoomed)
    # T's bits are dvsg_tps_render_u8's
    T8 = torch.full_like(T, float("nan"))
    rgb = torch.zeros((3, H, W, 3), dtype=torch.uint8, device="cuda")
    f32 = torch.empty((3, H, W, 3), device="cuda")
    _call("dvsg_tps_render_u8", net.handle, _dev(F).data_ptr(), rgb.data_ptr(), 3, H, W, 0, T8.data_ptr(), f32.data_ptr(), None,
          0, 0, _stream())
    torch.cuda.synchronize()
    same_bits(T.cpu().numpy(), T8.cpu().numpy(), what + ": T")
    # luma: the same call through the same view without the property, on the same Y plane
    T0, out0 = render(without, F, b, zoom, pre, surface)
    same_bits(T.cpu().numpy(), T0.cpu().numpy(), what + ": T against the 4:2:0 view")
    got_y, got_c = pre.planes(out)
    same_bits(got_y, pre.planes(out0)[0], what + ": luma against the view without the property")
    assert (got_y != _poison(words)).any()
    # chroma: the reference on the (H, W / 2) plane
    xs, ys = grid(T, zoom, 3, H, W // 2)
    ok = np.stack([R.valid(H, W // 2, xs[i], ys[i]) for i in range(3)])
    assert ok.any() and not ok.all(), "%s: %d of %d chroma samples valid" % (what, ok.sum(), ok.size)
    src_c, before = b.planes()[1], pre.planes()[1]
    want = np.empty_like(got_c)
    for i in range(3):
        s, written = Y.render_chroma(src_c[i], xs[i], ys[i], border, bicubic, words)
        assert np.array_equal(written, ok[i] if border == "keep" else np.ones_like(ok[i]))
        want[i] = np.where(written[..., None], s, before[i])
    same_bits(got_c, want, what + ": chroma")
    if border == "keep":
        assert (got_c[~ok] == _poison(words)).all(), what + ": keep wrote an invalid sample"
    if border == "black" and not bicubic:   # dvsg_tps_warp_f32 / _zoom_f32 on a grid of the plane's size, bit for bit
        v = GP.warp_plane(chroma_samples(src_c, words), T8, zoom)
        same_bits(got_c, chroma_bytes(v, False, words), what + ": chroma against dvsg_tps_warp_f32")
    assert np.array_equal(pre.outside(out), pre.outside()), what + ": bytes outside the planes were written"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the render at a delivery size
# ---------------------------------------------------------------------------------------------------------------------
SCALED_CASES = [((24, 40), (12, 20)), ((24, 40), (8, 14)), ((24, 40), (6, 10)), ((24, 40), (24, 10)), ((26, 44), (12, 20))]


def scaled_batches(words, H, W, oh, ow, n=2):
    return (Y.Batch422(H * 31 + W, n, H, W, words, pitch=(2 * W + 6) if words else (W + 3), uv_row=H + 1, tail=1, low=0x15 if words else 0),
            Y.Batch422(0, n, oh, ow, words, pitch=(2 * ow + 10) if words else (ow + 5), uv_row=oh + 2, tail=1, fill=POISON))


@pytest.mark.parametrize("border", ["black", "replicate", "mirror"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("src, out", SCALED_CASES)
def test_scaled(net, src, out, surface, filt, border):
    (H, W), (oh, ow) = src, out
    words, bicubic = surface == "p010", filt == "bicubic"
    b, ob = scaled_batches(words, H, W, oh, ow)
    F = GS.vectors()
    with422 = net.view(filt, border, surface=surface, out_size=out, chroma="422")
    without = net.view(filt, border, surface=surface, out_size=out)
    sy, sx = S.factors(src, out)
    Tp = GS.coefficients(net.view(filt, border), F)
    src_c = b.planes()[1]
    # the reference first: the chroma plane (H, W / 2) -> (oh, ow / 2) on the virtual grid (sy oh, sx ow / 2)
    refs, counts = [], []
    for zoom in GS.zooms():
        xs, ys = GS.grid(Tp, zoom, 2, sy * oh, sx * (ow // 2))
        refs.append(np.stack([Y.render_chroma_scaled(src_c[i], xs[i], ys[i], sy, sx, border, bicubic, words) for i in range(2)]))
        counts += [S.coverage((H, W // 2), xs[i], ys[i], sy, sx) for i in range(2)]
    GS.check_coverage(counts, sy * sx)
    for zoom, want in zip(GS.zooms(), refs):
        what = "%s %dx%d -> %dx%d %s %s zoom=%s" % (FORMATS[surface], H, W, oh, ow, filt, border, zoom is not None)
        T, got = GS.surface_render(with422, F, b, zoom, ob)
        T0, got0 = GS.surface_render(without, F, b, zoom, ob)
        GS.same(T.cpu().numpy(), Tp.cpu().numpy(), what + " T")
        GS.same(T0.cpu().numpy(), Tp.cpu().numpy(), what + " T of the 4:2:0 view")
        GS.same(ob.planes(got)[0], ob.planes(got0)[0], what + " luma against the view without the property")
        GS.same(ob.planes(got)[1], want, what + " chroma")
        assert (ob.outside(got) == POISON).all(), what + ": bytes beyond the width or between the planes were written"


@pytest.mark.parametrize("border", ["black", "replicate", "mirror", "keep"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("surface", SURFACES)
def test_scaled_identity(net, surface, filt, border):
    """a scaled 4:2:2 view at the source's size, or (0, 0), gives the unscaled 4:2:2 view's bytes"""
    H, W = 24, 40
    b, ob = scaled_batches(surface == "p010", H, W, H, W)
    F = GS.vectors()
    plain = net.view(filt, border, surface=surface, chroma="422")
    zero = ctypes.c_void_p()
    GS._lib().call("dvsg_locnet_view_create_scaled", plain, 0, 0, ctypes.byref(zero))
    try:
        assert _lib().dvsg_locnet_render_chroma(zero) == 1
        for zoom in GS.zooms():
            T0, want = GS.surface_render(plain, F, b, zoom, ob)
            for name, view in (("(H, W)", net.view(filt, border, surface=surface, out_size=(H, W), chroma="422")), ("(0, 0)", zero)):
                T1, got = GS.surface_render(view, F, b, zoom, ob)
                what = "%s %s %s size %s zoom=%s" % (FORMATS[surface], filt, border, name, zoom is not None)
                GS.same(T1.cpu().numpy(), T0.cpu().numpy(), what + " T")
                GS.same(got, want, what)
            assert (ob.planes(want)[1] != _poison(surface == "p010")).any()
    finally:
        _lib().dvsg_locnet_destroy(zero)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the property: inheritance, what reads it, argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _make(name, handle, *args):
    v = ctypes.c_void_p()
    GS._lib().call(name, handle, *(args + (ctypes.byref(v),)))
    return v


def _props(h):
    lib = _lib()
    oh, ow = ctypes.c_int(), ctypes.c_int()
    lib.dvsg_locnet_render_size(h, ctypes.byref(oh), ctypes.byref(ow))
    return (lib.dvsg_locnet_render_filter(h), lib.dvsg_locnet_render_border(h), lib.dvsg_locnet_render_surface(h),
            (oh.value, ow.value), lib.dvsg_locnet_render_chroma(h))


def test_the_property_is_inherited_and_read_by_the_nv12_renders_alone(net):
    torch = _torch()
    lib = _lib()
    made = []

    def make(name, handle, *args):
        made.append(_make(name, handle, *args))
        return made[-1]
    try:
        inner = net.view("bicubic", "mirror")
        # chroma first, then surface, then size -- and the other way round
        c = make("dvsg_locnet_view_create_chroma", inner, 1)
        cs = make("dvsg_locnet_view_create_surface", c, 1)
        css = make("dvsg_locnet_view_create_scaled", cs, 12, 20)
        assert [_props(h) for h in (c, cs, css)] == [(1, 2, 0, (0, 0), 1), (1, 2, 1, (0, 0), 1), (1, 2, 1, (12, 20), 1)]
        s = make("dvsg_locnet_view_create_scaled", inner, 12, 20)
        ss = make("dvsg_locnet_view_create_surface", s, 1)
        ssc = make("dvsg_locnet_view_create_chroma", ss, 1)
        assert [_props(h) for h in (s, ss, ssc)] == [(1, 2, 0, (12, 20), 0), (1, 2, 1, (12, 20), 0), (1, 2, 1, (12, 20), 1)]
        back = make("dvsg_locnet_view_create_chroma", ssc, 0)      # a view of a view is a view of the parent
        assert _props(back) == (1, 2, 1, (12, 20), 0)
        # the three plain constructors give 4:2:0, from a 4:2:2 view too
        plain = [make("dvsg_locnet_view_create", c, 1), make("dvsg_locnet_view_create_border", c, 0, 2),
                 make("dvsg_locnet_view_create_shaped", c, 0, 1, 1, ctypes.c_float(0.5), ctypes.c_float(0.25))]
        assert [lib.dvsg_locnet_render_chroma(h) for h in plain + [net.handle, inner]] == [0] * 5
        assert lib.dvsg_locnet_destroy(net.handle) == -1 and b"view" in lib.dvsg_last_error_string()
        # both orders render alike at the delivery size (the chroma view of a scaled view is in the size table)
        b, ob = scaled_batches(True, 24, 40, 12, 20)
        F = GS.vectors()
        _, one = GS.surface_render(css, F, b, None, ob)
        _, two = GS.surface_render(ssc, F, b, None, ob)
        _, three = GS.surface_render(net.view("bicubic", "mirror", surface="p010", out_size=(12, 20), chroma="422"), F, b, None, ob)
        GS.same(one, two, "chroma -> surface -> scaled against scaled -> surface -> chroma")
        GS.same(one, three, "against LocNet.view")
        assert (ob.planes(one)[1] != _poison(True)).any()
        # a 4:2:0 view made by the constructor gives the parent's NV12 bytes
        H, W = 6, 8
        zero = make("dvsg_locnet_view_create_chroma", net.handle, 0)
        nb, npre = nv12_ref.Batch(5, 2, H, W), nv12_ref.Batch(6, 2, H, W, W + 3)
        Tz, oz = render(zero, GP.vectors(), nb, None, npre, "nv12")
        Tp, op = render(net.handle, GP.vectors(), nb, None, npre, "nv12")
        same_bits(Tz.cpu().numpy(), Tp.cpu().numpy(), "T")
        assert np.array_equal(oz, op)
        # dvsg_tps_render_u8 / _zoom_u8, the coverage scan and the coefficients do not read it
        F2 = _dev(GP.vectors())
        src = _dev(np.random.default_rng(8).integers(0, 256, (2, H, W, 3), dtype=np.uint8))
        zoom = _dev(np.float32([1.0, 0.8]))
        c0 = make("dvsg_locnet_view_create_chroma", net.handle, 1)
        for with_c, without in ((c0, net.handle), (c, inner)):
            for z in (None, zoom):
                a = GP.B.render_u8(with_c, F2, src, 0, z, True, True, W, 0)
                d = GP.B.render_u8(without, F2, src, 0, z, True, True, W, 0)
                same_bits(a[0].cpu().numpy(), d[0].cpu().numpy(), "T of dvsg_tps_render_u8")
                same_bits(a[1], d[1], "out_f32")
                same_bits(a[2], d[2], "out_u8")
        shaped = net.view("bilinear", "keep", 0.5, 0.25, "translation")
        shaped_c = make("dvsg_locnet_view_create_chroma", shaped, 1)
        res = []
        for h in (shaped_c, shaped):
            Tc = torch.full((2, 2, 28), float("nan"), device="cuda")
            _call("dvsg_tps_coefficients_f32", h, F2.data_ptr(), 2, Tc.data_ptr(), _stream())
            need = ctypes.c_size_t()
            GS._lib().call("dvsg_tps_coverage_workspace_bytes", 2, 12, 10, ctypes.byref(need))
            ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
            Ts = torch.full((2, 2, 28), float("nan"), device="cuda")
            keys = torch.full((2, 2), -1, dtype=torch.int32, device="cuda")
            _call("dvsg_tps_coverage_net_f32", h, F2.data_ptr(), None, 2, 12, 10, 12, 10, Ts.data_ptr(), keys[0].data_ptr(),
                  keys[1].data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream())
            torch.cuda.synchronize()
            res.append((Tc.cpu().numpy(), Ts.cpu().numpy(), keys.cpu().numpy()))
        for a, d, name in zip(res[0], res[1], ("dvsg_tps_coefficients_f32", "T of the coverage scan", "the scan's keys")):
            same_bits(a, d, name)
        # argument errors are returned before any byte of the outputs is written
        T = torch.full((2, 2, 28), float("nan"), device="cuda")
        buf = torch.zeros(2 * 13 * 32 + 8, dtype=torch.uint8, device="cuda")
        out = torch.full_like(buf, POISON)
        y, o = buf.data_ptr(), out.data_ptr()

        def status(handle, H=H, W=W, pitch=W, opitch=W, duv=0, stride=13 * W, n=2):
            return lib.dvsg_tps_render_nv12(handle, F2.data_ptr(), y, y + H * pitch + duv, pitch, stride, n, H, W, T.data_ptr(),
                                            o, o + H * opitch, opitch, 13 * opitch, _stream())
        c0p = make("dvsg_locnet_view_create_surface", c0, 1)
        for handle, kw, word in ((c0, dict(pitch=W - 1), b"source pitch=7 < W=8"), (c0, dict(opitch=W - 2), b"output pitch=6"),
                                 (c0, dict(H=5), b"H=5"), (c0, dict(W=6, H=2), b"H=2"), (c0, dict(stride=6 * W - 1), b"frame_stride"),
                                 (c0, dict(n=0), b"n=0"), (c0p, dict(pitch=2 * W - 2, opitch=2 * W), b"pitch=14 < 2 W = 16"),
                                 (c0p, dict(pitch=2 * W, opitch=2 * W, duv=1), b"source uv plane pointer")):
            assert status(handle, **kw) == -1, kw
            assert word in lib.dvsg_last_error_string(), (kw, lib.dvsg_last_error_string())
        assert lib.dvsg_tps_render_zoom_nv12(c0, F2.data_ptr(), y, y + H * 7, 7, 13 * 7, 2, H, W, zoom.data_ptr(), T.data_ptr(), o,
                                             o + H * W, W, 13 * W, _stream()) == -1
        assert b"dvsg_tps_render_zoom_nv12" in lib.dvsg_last_error_string()
        torch.cuda.synchronize()
        assert torch.isnan(T).all() and (out == POISON).all(), "a refused call did device work"
        assert status(c0) == 0 and status(c0p, pitch=2 * W, opitch=2 * W, stride=13 * 2 * W) == 0
    finally:
        for v in reversed(made):
            lib.dvsg_locnet_destroy(v)


# ---------------------------------------------------------------------------------------------------------------------
# 4. online: model 38 x 54, the 9-channel synthetic checkpoint with skip_length (0, 2, 3)
# ---------------------------------------------------------------------------------------------------------------------
SKIP, SIZES, N = GP.SKIP, GP.SIZES, 9
OUT_SIZE = (16, 24)    # factors 2 x 2 of (20, 32) and 4 x 4 of (64, 96)
model = GP.model


def clips(fmt):
    """per size: (the NV12 clip [9, 3 H0 / 2, W0] the network is to see, the 4:2:2 clip uint8 [9, 2 H0, bps W0]).  The EVEN
    chroma rows are the NV12 clip's, the odd ones come from another seed: they matter to the render and not to the ingest.
    P210: the words' high bytes are those samples and the next two bits are seeded."""
    if ("clips", fmt) not in _CACHE:
        out = []
        for i, (H0, W0) in enumerate(SIZES):
            nv12 = nv12_ref.smooth_batch(800 + i, N, H0, W0).buf
            odd = nv12_ref.smooth_batch(830 + i, N, H0, W0).buf
            nv16 = np.empty((N, 2 * H0, W0), np.uint8)
            nv16[:, :H0] = nv12[:, :H0]
            nv16[:, H0::2], nv16[:, H0 + 1::2] = nv12[:, H0:], odd[:, H0:]
            assert not np.array_equal(nv16[:, H0::2], nv16[:, H0 + 1::2])
            if fmt == "p210":
                two = np.random.default_rng(810 + i).integers(0, 4, nv16.shape, dtype=np.uint16)
                words = (nv16.astype(np.uint16) << 8) | (two << 6)
                clip = words.astype("<u2").view(np.uint8).reshape(N, 2 * H0, 2 * W0)
            else:
                clip = nv16
            assert np.array_equal(Y.even_rows_surface(clip, fmt == "p210"), nv12)
            out.append((nv12, clip))
        _CACHE[("clips", fmt)] = out
    return _CACHE[("clips", fmt)]


def _one(H, W, words, frame=None):
    """a packed one-frame batch [1, 2 H, bps W]: poison, or the bytes of `frame`"""
    one = Y.Batch422(0, 1, H, W, words, fill=POISON)
    if frame is not None:
        one.buf[0] = frame
    return one


def run_online(fmt, variant):
    """9 steps of two streams with crop="auto"; returns the outputs per stream.  variant "plain" (with scene_cut), "keep" or
    "out_size".  Every step: _F, the pool and the scene state are an "nv12" run's fed the even-row surfaces; every output is
    one direct render through the view with the step's F_t row and the stream's zoom."""
    if ("online", fmt, variant) in _CACHE:
        return _CACHE[("online", fmt, variant)]
    torch = _torch()
    from coupe.dvsg_amd.online import OnlineStabilizer
    m, words, surface = model(), fmt == "p210", "p010" if fmt == "p210" else "nv12"
    kw = dict(max_streams=2, skip_length=SKIP, crop="auto", yuv_matrix="bt601")
    extra, view_kw = {}, {}
    if variant == "plain":
        kw["scene_cut"] = 0.75
    elif variant == "keep":
        extra, view_kw = dict(border="keep"), dict(border="keep")
    else:
        extra, view_kw = dict(out_size=OUT_SIZE), dict(out_size=OUT_SIZE)
    on, off = OnlineStabilizer(m, frame_format=fmt, **kw, **extra), OnlineStabilizer(m, frame_format="nv12", **kw, **extra)
    on.pool.zero_()
    off.pool.zero_()
    sid_on, sid_off = [on.open(), on.open()], [off.open(), off.open()]
    view = m.locnet.view(surface=surface, chroma="422", **view_kw)
    assert _lib().dvsg_locnet_render_chroma(view) == 1
    outs, kept = [[], []], [None, None]
    cl = clips(fmt)
    for k in range(N):
        res = on.step({sid_on[i]: _dev(cl[i][1][k]) for i in range(2)})
        off.step({sid_off[i]: _dev(cl[i][0][k]) for i in range(2)})
        same_bits(on._F.cpu().numpy(), off._F.cpu().numpy(), "F_t of step %d" % k)
        same_bits(on.pool.cpu().numpy(), off.pool.cpu().numpy(), "pool after step %d" % k)
        if variant == "plain":
            assert torch.equal(on._scene, off._scene), "scene state after step %d" % k
        for row, i in enumerate(sorted(range(2), key=lambda i: SIZES[i])):   # batch order: by source size
            H0, W0 = SIZES[i]
            oh, ow = OUT_SIZE if variant == "out_size" else (H0, W0)
            a = on.crop_state(sid_on[i])   # (the 4:2:0 run scans another chroma grid: its zoom is its own)
            got = res[sid_on[i]]
            assert isinstance(got, torch.Tensor) and tuple(got.shape) == (2 * oh, (2 if words else 1) * ow) and got.dtype == torch.uint8
            pre = _one(oh, ow, words, kept[i] if variant == "keep" and k > 0 else cl[i][1][k] if variant == "keep" else None)
            _, alone = render(view, on._F[row:row + 1].cpu().numpy(), _one(H0, W0, words, cl[i][1][k]),
                              _dev(np.float32([a["zoom"]])), pre, fmt)
            assert np.array_equal(got.cpu().numpy(), alone[0]), "%s %s: output of stream %d, step %d" % (fmt, variant, i, k)
            kept[i] = alone[0]
            outs[i].append(got.cpu().numpy())
    zooms = [float(on.crop_state(s)["zoom"]) for s in sid_on]
    assert min(zooms) < 1.0, "no stream ends with zoom < 1 (%s): the crop path proves nothing" % (zooms,)
    _CACHE[("online", fmt, variant)] = [np.stack(o) for o in outs]
    return _CACHE[("online", fmt, variant)]


@pytest.mark.parametrize("variant", ["plain", "keep", "out_size"])
@pytest.mark.parametrize("fmt", ["nv16", "p210"])
def test_online(fmt, variant):
    outs = run_online(fmt, variant)
    bps = 2 if fmt == "p210" else 1
    for (H0, W0), o in zip(SIZES, outs):
        oh, ow = OUT_SIZE if variant == "out_size" else (H0, W0)
        assert o.shape == (N, 2 * oh, bps * ow) and len(np.unique(o)) > 8


def test_online_scans_the_chroma_grid():
    """crop="auto" scans (H0, W0 / 2) for chroma, not (H0 / 2, W0 / 2), and with out_size the virtual grid (sy oh, sx ow / 2)"""
    from coupe.dvsg_amd.online import OnlineStabilizer
    m = model()
    on = OnlineStabilizer(m, frame_format="nv16", skip_length=SKIP, crop="auto")
    assert on._scan_grids(20, 32, True) == [(20, 32), (20, 16)]
    assert OnlineStabilizer(m, frame_format="p010", skip_length=SKIP, crop="auto")._scan_grids(20, 32, True) == [(20, 32), (10, 16)]
    on = OnlineStabilizer(m, frame_format="p210", skip_length=SKIP, crop="auto", out_size=OUT_SIZE)
    assert on._scan_grids(64, 96, True) == [(64, 96, 64, 96), (64, 48, 64, 48)]
    assert on._scan_grids(20, 32, True) == [(20, 32, 32, 48), (20, 16, 32, 24)]


def test_online_words_in_words_out():
    """NumPy uint16 in -> NumPy uint16 out, the bits of the uint8 form; reset() and a refused frame"""
    from coupe.dvsg_amd.online import OnlineStabilizer
    want = run_online("p210", "plain")[0]
    host = OnlineStabilizer(model(), frame_format="p210", max_streams=2, skip_length=SKIP, crop="auto", yuv_matrix="bt601",
                            scene_cut=0.75)
    sid = host.open()
    H0, W0 = SIZES[0]
    for k in range(4):
        got = host.push(sid, clips("p210")[0][1][k].view("<u2"))
        assert isinstance(got, np.ndarray) and got.dtype == np.uint16 and got.shape == (2 * H0, W0)
        assert np.array_equal(got.view(np.uint8), want[k]), "uint16 frame %d" % k
    host.reset(sid)
    got = host.push(sid, clips("p210")[0][1][0].view("<u2"))
    assert np.array_equal(got.view(np.uint8), want[0]), "the first frame after reset() is a step 0"
    with pytest.raises(ValueError, match="odd"):
        host.push(sid, np.zeros((42, 64), np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 5. clips and pipes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv16", "p210"])
def test_stabilize_clips_is_the_online_run(fmt):
    from coupe.dvsg_amd.online import stabilize_clips
    want = run_online(fmt, "plain")
    cl = [c[1] for c in clips(fmt)]
    got = stabilize_clips(model(), cl, frame_format=fmt, skip_length=SKIP, crop="auto", yuv_matrix="bt601", scene_cut=0.75)
    for i in range(2):
        assert isinstance(got[i], np.ndarray) and got[i].dtype == np.uint8
        assert np.array_equal(got[i], want[i]), "clip %d" % i
    if fmt == "p210":   # uint16 clips come back as words
        got = stabilize_clips(model(), [c.view("<u2") for c in cl], frame_format=fmt, skip_length=SKIP, crop="auto",
                              yuv_matrix="bt601", scene_cut=0.75)
        for i in range(2):
            assert got[i].dtype == np.uint16 and np.array_equal(got[i].view(np.uint8), want[i])
    with pytest.raises(ValueError, match=r"2\*H0"):
        stabilize_clips(model(), [cl[0][0]], frame_format=fmt, skip_length=SKIP)


@pytest.mark.parametrize("fmt", ["nv16", "p210"])
def test_pipes(fmt):
    """One C422 / C422p10 source, depth 3: the output is stabilize_clips on the repacked frames, byte for byte after the
    repack, under a header that repeats the C tag and the X tags; raw NV16 / P210 in and out gives the same frames."""
    torch = _torch()
    from coupe.dvsg_amd import y4m
    from coupe.dvsg_amd.online import stabilize_clips
    H0, W0 = SIZES[0]
    ten = fmt == "p210"
    semi = clips(fmt)[0][1]
    want = stabilize_clips(model(), [semi], frame_format=fmt, skip_length=SKIP, yuv_matrix=y4m.default_yuv_matrix(H0))[0]
    assert want.dtype == np.uint8 and want.shape == semi.shape and not np.array_equal(want, semi)
    to_planar, to_semi = (y4m.p210_to_i422p10, y4m.i422p10_to_p210) if ten else (y4m.nv16_to_i422, y4m.i422_to_nv16)
    planar = to_planar(torch.from_numpy(semi.copy())).numpy()
    assert np.array_equal(planar[0], (Y.p210_to_i422p10 if ten else Y.nv16_to_i422)(semi[0]))
    tag = b"C422p10 XYSCSS=422P10" if ten else b"C422 XYSCSS=422"
    head = b"YUV4MPEG2 W32 H20 F30000:1001 Ip A1:1 " + tag + b" XCOLORRANGE=LIMITED\n"
    both = ("420", "422")
    src = y4m.Y4MReader(io.BytesIO(head + b"".join(b"FRAME\n" + f.tobytes() for f in planar)), depths=(8, 10), chromas=both)
    out = io.BytesIO()
    snk = y4m.Y4MWriter(out, W0, H0, src.fps, aspect=src.aspect, colorspace=src.colorspace, tags=src.tags, interlace=src.interlace,
                        chromas=both)
    stats = GP.run_pipes([src], [snk], depth=3)
    assert stats[0]["frames"] == N and stats[0]["high_water"] <= 3
    data = out.getvalue()
    assert data.startswith(head)
    got = np.stack(list(y4m.Y4MReader(io.BytesIO(data), depths=(8, 10), chromas=both)))
    assert np.array_equal(to_semi(torch.from_numpy(got)).numpy(), want)
    Reader, Writer = (y4m.RawP210Reader, y4m.RawP210Writer) if ten else (y4m.RawNV16Reader, y4m.RawNV16Writer)
    raw = io.BytesIO()
    stats = GP.run_pipes([Reader(io.BytesIO(semi.tobytes()), W0, H0)], [Writer(raw, W0, H0)], depth=3)
    assert stats[0]["frames"] == N and raw.getvalue() == want.tobytes()


def test_front_end_on_a_422_file(tmp_path):
    """python -m coupe.dvsg_amd.pipe on a tiny C422 file: the output header repeats the C tag and the X tags"""
    import subprocess
    import sys
    from coupe.dvsg_amd import y4m
    H0, W0 = SIZES[0]
    planar = y4m.nv16_to_i422(_torch().from_numpy(clips("nv16")[0][1][:3].copy())).numpy()
    head = b"YUV4MPEG2 W32 H20 F25:1 Ip A1:1 C422 XCOLORRANGE=LIMITED\n"
    (tmp_path / "in.y4m").write_bytes(head + b"".join(b"FRAME\n" + f.tobytes() for f in planar))
    run = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--synthetic-weights", "--model-size", "54x38",
                          "--skip-length", "0,2,3", "--input", str(tmp_path / "in.y4m"), "--output", str(tmp_path / "out.y4m")],
                         capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    data = (tmp_path / "out.y4m").read_bytes()
    assert data.startswith(head)
    r = y4m.Y4MReader(io.BytesIO(data), chromas=("420", "422"))
    assert r.layout == "i422" and len(list(r)) == 3
