"""Host-side checks of the 10-bit path (include/dvsg_amd.h, "P010 frames"): the sample and word rules over all 1024 values,
the surface-format view's argument checks, C420p10 over Y4M, the two repacks, stabilize_pipes at 10 bits with the step
replaced by the identity, and OnlineStabilizer's option checks for frame_format="p010".  Nothing here needs a device."""
import ctypes
import io
import os
import threading

import numpy as np
import pytest

from coupe.dvsg_amd import y4m
from coupe.dvsg_amd.pipe import stabilize_pipes

f32 = np.float32
S = np.arange(1024)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sample and word rules
# ---------------------------------------------------------------------------------------------------------------------
def test_float32_division_is_the_rounded_float64_quotient():
    q = S.astype(f32) / f32(1023.0)
    assert q.dtype == f32
    assert np.array_equal(q, (S.astype(np.float64) / 1023.0).astype(f32))
    c = (S - 512).astype(f32) / f32(1023.0)
    assert np.array_equal(c, ((S - 512).astype(np.float64) / 1023.0).astype(f32))


def test_luma_rounds_to_nearest_because_truncation_is_no_round_trip():
    """NV12 luma truncates and round-trips all 256 bytes; at 10 bits truncation comes back one low for 519 values."""
    v = S.astype(f32) / f32(1023.0)
    trunc = np.floor(v.astype(np.float64) * 1023.0)
    low = trunc != S
    assert int(low.sum()) == 519
    assert np.array_equal(trunc[low], S[low] - 1)
    near = np.clip(np.floor(v.astype(np.float64) * 1023.0 + 0.5), 0, 1023)
    assert np.array_equal(near, S)
    b = np.arange(256)
    assert np.array_equal(np.floor((b.astype(f32) / f32(255.0)).astype(np.float64) * 255.0), b)   # the 8-bit rule's reason


def test_chroma_rule_is_exact():
    v = (S - 512).astype(f32) / f32(1023.0)
    assert np.array_equal(np.clip(np.floor(v.astype(np.float64) * 1023.0 + 512.5), 0, 1023), S)
    assert v[512] == 0.0   # the neutral value is the filters' exact zero


def test_p010_ref_restates_the_rules():
    import p010_ref
    words = (S << 6).astype(np.uint16)
    noisy = words | np.uint16(0x3F)   # the low 6 bits are ignored
    for chroma in (False, True):
        v = p010_ref.samples(noisy, chroma)
        assert v.dtype == f32 and np.array_equal(v, p010_ref.samples(words, chroma))
        assert np.array_equal(p010_ref.to_word(v, chroma), words)
    assert p010_ref.to_word(f32([np.nan, -1.0, 2.0]), False).tolist() == [0, 0, 1023 << 6]
    assert p010_ref.to_word(f32([np.nan, -1.0, 2.0]), True).tolist() == [0, 0, 1023 << 6]
    assert p010_ref.to_word(f32([0.0]), True).tolist() == [512 << 6]


# ---------------------------------------------------------------------------------------------------------------------
# 2. dvsg_locnet_view_create_surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.dvsg_last_error_string()


def test_view_create_surface_rejects_bad_arguments(lib):
    f = lib.dvsg_locnet_view_create_surface
    view = ctypes.c_void_p(5)
    assert f(None, 1, ctypes.byref(view)) == -1 and b"NULL net" in _err(lib)
    assert b"dvsg_locnet_view_create_surface" in _err(lib)
    assert f(8, 1, None) == -1 and b"NULL view" in _err(lib)
    for bad in (2, -1, 7):   # decided before the handle (here not even a handle) is read
        view = ctypes.c_void_p(5)
        assert f(8, bad, ctypes.byref(view)) == -1
        assert ("surface_format=%d" % bad).encode() in _err(lib)
        assert view.value is None
    assert lib.dvsg_locnet_render_surface(None) == 0


def test_python_view_checks_the_surface_name():
    from coupe.dvsg_amd.networks import SURFACES, check_surface
    assert SURFACES == {"nv12": 0, "p010": 1}
    assert check_surface("p010") == "p010"
    for bad in ("P010", "p016", 1, None):
        with pytest.raises(ValueError, match="surface"):
            check_surface(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. C420p10 over Y4M
# ---------------------------------------------------------------------------------------------------------------------
W, H = 8, 6
HEAD10 = b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\n" % (W, H)


def frames10(seed, n, W, H):
    """n C420p10 frames as the stream's bytes, uint8 [n, 3 H / 2, 2 W]: samples in [0, 1023], 0 and 1023 among them"""
    s = np.random.default_rng(seed).integers(0, 1024, (n, 3 * H // 2, W), dtype=np.uint16)
    s[:, 0, 0], s[:, 0, 1], s[:, -1, -1] = 0, 1023, 1023
    return s.astype("<u2").view(np.uint8)


def stream10(frames):
    return HEAD10 + b"".join(b"FRAME\n" + f.tobytes() for f in frames)


def test_y4m_420p10_is_parsed_when_asked_for():
    fr = frames10(1, 3, W, H)
    r = y4m.Y4MReader(io.BytesIO(stream10(fr)), depths=(8, 10))
    assert (r.width, r.height, r.fps, r.aspect, r.interlace, r.colorspace) == (W, H, (30000, 1001), (1, 1), "p", "420p10")
    assert r.layout == "i420p10" and r.frame_shape == (3 * H // 2, 2 * W) and r.frame_bytes == 3 * W * H
    assert r.tags == ("XYSCSS=420P10", "XCOLORRANGE=LIMITED")
    got = list(r)
    assert len(got) == 3 and all(g.dtype == np.uint8 and np.array_equal(g, f) for g, f in zip(got, fr))
    # an 8-bit stream through the same reader is what it was
    r8 = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1 C420jpeg\n"), depths=(8, 10))
    assert r8.layout == "i420" and r8.frame_shape == (9, 8) and y4m.Y4MReader.layout == "i420"


def test_y4m_default_still_refuses_420p10():
    for kw in ({}, dict(depths=(8,))):
        with pytest.raises(y4m.Y4MError, match="C420p10"):
            y4m.Y4MReader(io.BytesIO(stream10(frames10(1, 1, W, H))), **kw)
    for tag in ("C422", "C444", "C444p16", "C420p12", "C422p10"):   # and ten-bit readers refuse everything else still
        with pytest.raises(y4m.Y4MError, match=tag):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1 %s\n" % tag.encode()), depths=(8, 10))
    with pytest.raises(y4m.Y4MError, match="C420jpeg"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1 C420jpeg\n"), depths=(10,))
    for bad in ((), (12,), (8, 16)):
        with pytest.raises(ValueError, match="depths"):
            y4m.Y4MReader(io.BytesIO(HEAD10), depths=bad)


def test_y4m_420p10_writer_round_trip():
    fr = frames10(2, 4, W, H)
    out = io.BytesIO()
    w = y4m.Y4MWriter(out, W, H, (30000, 1001), aspect=(1, 1), colorspace="420p10", tags=("XYSCSS=420P10", "XCOLORRANGE=LIMITED"))
    assert w.layout == "i420p10" and w.frame_shape == (3 * H // 2, 2 * W) and w.frame_bytes == 3 * W * H
    for f in fr:
        w.write(f)
    w.flush()
    assert out.getvalue() == stream10(fr)
    assert y4m.Y4MWriter(io.BytesIO(), W, H, 25).layout == "i420"   # the class default is untouched
    with pytest.raises(ValueError, match="bytes"):
        w.write(np.zeros((3 * H // 2, W), np.uint8))
    with pytest.raises(y4m.Y4MError, match="422p10"):
        y4m.Y4MWriter(io.BytesIO(), W, H, 25, colorspace="422p10")


@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 5, 6, 7])
def test_y4m_420p10_from_a_pipe_with_short_reads(chunk):
    fr = frames10(3, 2, W, H)
    data = stream10(fr)
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb", buffering=0) as f:
            for i in range(0, len(data), chunk):
                f.write(data[i:i + chunk])
    t = threading.Thread(target=feed)
    t.start()
    try:
        with os.fdopen(rd, "rb", buffering=0) as f:
            got = list(y4m.Y4MReader(f, depths=(8, 10)))
    finally:
        t.join(30)
    assert len(got) == 2 and all(np.array_equal(g, f) for g, f in zip(got, fr))


def test_y4m_420p10_truncated_frame_names_the_byte_counts():
    data = stream10(frames10(4, 3, W, H))
    per = len(b"FRAME\n") + 3 * W * H
    assert 3 * W * H == 144
    r = y4m.Y4MReader(io.BytesIO(data[:len(HEAD10) + 2 * per + 6 + 42]), depths=(8, 10))
    assert r.read() is not None and r.read() is not None
    with pytest.raises(y4m.Y4MError, match=r"frame 2 .*\b42 of 144 bytes"):
        r.read()
    raw = y4m.RawP010Reader(io.BytesIO(bytes(144 + 143)), W, H)
    assert raw.layout == "p010" and raw.frame_shape == (9, 16) and raw.read() is not None
    with pytest.raises(y4m.Y4MError, match=r"frame 1 .*\b143 of 144 bytes"):
        raw.read()


def test_raw_p010_writer():
    out = io.BytesIO()
    w = y4m.RawP010Writer(out, W, H)
    fr = frames10(5, 2, W, H)
    for f in fr:
        w.write(f)
    assert w.layout == "p010" and out.getvalue() == fr.tobytes() and w.frames_written == 2
    with pytest.raises(y4m.Y4MError, match="7"):
        y4m.RawP010Writer(io.BytesIO(), 7, 4)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the repacks against their index formula
# ---------------------------------------------------------------------------------------------------------------------
def every_value_frame():
    """One 32 x 32 frame whose Y plane holds every 10-bit value once and whose U and V planes hold 256 values each, 0 and
    1023 among them: planar samples uint16 [48, 32]"""
    Hh = Ww = 32
    s = np.empty((3 * Hh // 2, Ww), np.uint16)
    s[:Hh] = np.random.default_rng(6).permutation(1024).reshape(Hh, Ww)
    c = np.random.default_rng(7).permutation(1024)[:512]
    c[0], c[511] = 0, 1023
    s[Hh:] = c.reshape(Hh // 2, Ww)
    return s, Hh, Ww


def p010_by_index(s, Hh, Ww):
    """P010[i][j] of planar samples s: Y as it is, UV row i = U row i and V row i interleaved, every word << 6 (mod 2^16)"""
    q = Hh * Ww // 4
    flat = s.reshape(-1).astype(np.uint32)
    u, v = flat[Hh * Ww:Hh * Ww + q], flat[Hh * Ww + q:]
    out = np.empty_like(flat)
    out[:Hh * Ww] = flat[:Hh * Ww]
    out[Hh * Ww + 0::2][:q] = u
    out[Hh * Ww + 1::2][:q] = v
    return ((out << 6) & 0xFFFF).astype(np.uint16).reshape(s.shape)


def test_repacks_against_the_index_formula():
    import torch
    s, Hh, Ww = every_value_frame()
    assert np.array_equal(np.sort(s[:Hh].ravel()), S) and s.max() == 1023 and s.min() == 0
    want = p010_by_index(s, Hh, Ww)
    assert (want >= 0x8000).any(), "no word has its top bit set"
    src = torch.from_numpy(s.astype("<u2").view(np.uint8).copy())
    got = y4m.i420p10_to_p010(src)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (48, 64)
    assert np.array_equal(got.numpy().view("<u2"), want)
    back = y4m.p010_to_i420p10(got)
    assert np.array_equal(back.numpy().view("<u2"), s)
    # a batch, into a caller's buffer; low bits of P010 words and high bits of planar samples are dropped
    batch = torch.stack([src, src.flip(0).contiguous()])
    out = torch.empty_like(batch)
    assert y4m.i420p10_to_p010(batch, out=out) is out and torch.equal(out[0], got)
    dirty = torch.from_numpy((want | np.uint16(0x3F)).astype("<u2").view(np.uint8).copy())
    assert np.array_equal(y4m.p010_to_i420p10(dirty).numpy().view("<u2"), s)
    high = torch.from_numpy((s | np.uint16(0xFC00)).astype("<u2").view(np.uint8).copy())
    assert np.array_equal(y4m.i420p10_to_p010(high).numpy().view("<u2"), want)
    with pytest.raises(ValueError, match="not be src"):
        y4m.i420p10_to_p010(src, out=src)
    with pytest.raises(ValueError, match="uint8"):
        y4m.i420p10_to_p010(src.view(torch.int16))
    with pytest.raises(ValueError, match="out"):
        y4m.p010_to_i420p10(src, out=torch.empty((48, 32), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 5. stabilize_pipes at 10 bits, the step replaced by the identity
# ---------------------------------------------------------------------------------------------------------------------
def identity(frames):
    return dict(frames)


def call(*args, **kw):
    box = {}

    def target():
        try:
            box["result"] = stabilize_pipes(*args, **kw)
        except BaseException as e:
            box["error"] = e
    t = threading.Thread(target=target, name="test-caller")
    t.start()
    t.join(30.0)
    assert not t.is_alive(), "stabilize_pipes did not return"
    return box.get("result"), box.get("error")


@pytest.mark.parametrize("depth", [1, 3])
def test_a_ten_bit_source_passes_through_bit_for_bit(depth):
    fr = frames10(8, 5, W, H)
    out, raw = io.BytesIO(), io.BytesIO()
    src = y4m.Y4MReader(io.BytesIO(stream10(fr)), depths=(8, 10))
    snk = y4m.Y4MWriter(out, W, H, src.fps, aspect=src.aspect, colorspace=src.colorspace, tags=src.tags)
    seen = []

    def step(frames):
        seen.extend(f.cpu().numpy().copy() for f in frames.values())
        return dict(frames)
    # a second lane: the same frames as raw P010 in and out, nothing repacked
    p010 = y4m.i420p10_to_p010(__import__("torch").from_numpy(fr.copy())).numpy()
    stats, err = call(None, [src, y4m.RawP010Reader(io.BytesIO(p010.tobytes()), W, H)], [snk, y4m.RawP010Writer(raw, W, H)],
                      depth=depth, _step_fn=step)
    assert err is None and [s["frames"] for s in stats] == [5, 5]
    assert out.getvalue() == stream10(fr)
    assert raw.getvalue() == p010.tobytes()
    assert len(seen) == 10 and all(np.array_equal(a, p010[k // 2]) for k, a in enumerate(seen))   # the step saw P010


def test_mixed_depths_are_refused_before_any_read():
    class Source(object):
        width, height, frame_shape, layout = W, H, (3 * H // 2, 2 * W), "i420p10"
        reads = 0

        def readinto(self, buf):
            Source.reads += 1
            return False
    eight = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1\n"))
    with pytest.raises(ValueError, match="bit depth"):
        stabilize_pipes(None, [Source()], [y4m.Y4MWriter(io.BytesIO(), W, H, 25)], _step_fn=identity)
    with pytest.raises(ValueError, match="bit depth"):
        stabilize_pipes(None, [eight, Source()], [y4m.RawNV12Writer(io.BytesIO(), W, H), y4m.RawP010Writer(io.BytesIO(), W, H)],
                        _step_fn=identity)
    with pytest.raises(ValueError, match="bit depth"):
        stabilize_pipes(None, [eight], [y4m.RawP010Writer(io.BytesIO(), W, H)], _step_fn=identity)
    assert Source.reads == 0 and eight.frames_read == 0
    assert [t.name for t in threading.enumerate() if t.name.startswith("stabilize_pipes")] == []


def test_front_end_knows_p010():
    from coupe.dvsg_amd import pipe
    args = pipe._arguments(["--synthetic-weights", "--format", "p010", "--size", "8x6"])
    assert args.format == "p010" and args.output_format == "p010" and args.size == (8, 6)
    with pytest.raises(pipe._UsageError, match="--size"):
        pipe._arguments(["--synthetic-weights", "--format", "p010"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. OnlineStabilizer's option checks
# ---------------------------------------------------------------------------------------------------------------------
def test_online_p010_options_raise_before_the_device():
    from coupe.dvsg_amd._lib import DvsgError
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    model = StabNet(32, 48)
    for kw, name in [(dict(side_by_side=True), "side_by_side"), (dict(as_uint8=True), "as_uint8"),
                     (dict(channel_order="bgr"), "channel_order")]:
        with pytest.raises(ValueError, match=name):
            OnlineStabilizer(model, frame_format="p010", **kw)
    with pytest.raises(ValueError, match="yuv_matrix"):
        OnlineStabilizer(model, frame_format="p010", yuv_matrix="bt2020")
    with pytest.raises(ValueError, match="'rgb', 'nv12' or 'p010'"):
        OnlineStabilizer(model, frame_format="i420")
    with pytest.raises(ValueError, match="'rgb', 'nv12' or 'p010'"):
        OnlineStabilizer(model, frame_format="p016")
    # the source-size options are accepted as for "nv12": the first thing missing is the weights
    with pytest.raises(DvsgError, match="weights"):
        OnlineStabilizer(model, frame_format="p010", render_filter="bicubic", border="keep", strength=0.5, rigidity=1.0,
                         shape_model="similarity", crop="auto")
    assert stabilize_clips(model, [], frame_format="p010") == []


# ---------------------------------------------------------------------------------------------------------------------
# 7. the bilinear restatement p010_ref.render_bilinear: known answers, torch's grid_sample, float32 against float64
# ---------------------------------------------------------------------------------------------------------------------
LOW = 0x3F
U24 = 2.0 ** -24


def tps_grids(F, ph, pw):
    """x_s, y_s [n, ph, pw] float32 of the map of F_t at a plane's size, from oracle.thin_plate_spline"""
    import inputs
    from oracle import thin_plate_spline as otps
    F = np.asarray(F, f32)
    V = inputs.v_src(len(F))
    with np.errstate(invalid="ignore"):
        T = otps.solve_system(V, (V + F).astype(f32))
        xs, ys = otps.source_coords(T, V, ph, pw)
    return xs.reshape(len(F), ph, pw), ys.reshape(len(F), ph, pw)


def border_vectors(kind):
    import test_gpu_border
    return test_gpu_border.vectors(kind)


def _words(s):
    return ((np.asarray(s, np.uint16) << 6) | np.uint16(LOW)).astype(np.uint16)


# samples of the hand-derived planes
L2 = [[100, 300], [500, 900]]
U2, V2 = [[512, 613], [412, 1023]], [[0, 512], [256, 768]]
L34 = [[0, 64, 128, 192], [256, 320, 384, 448], [512, 640, 768, 1023]]
# (x, y), valid, luma value in codes under replicate, mirror, (U, V) under replicate, mirror.  With wx0 = (x0 + 1) - xc, wx1 =
# xc - x0 and the same for y, a code is wx0 wy0 s(y0, x0) + wx0 wy1 s(y1, x0) + wx1 wy0 s(y0, x1) + wx1 wy1 s(y1, x1) (chroma:
# on s - 512, plus 512); the word holds it rounded to nearest, and no case is a tie.  E.g. (0.25, 0.5): .375 * 100 + .375 * 500 + .125 * 300 +
# .125 * 900 = 375; (-0.5, 0.5): replicate xc = 0 -> .5 * 100 + .5 * 500 = 300, mirror xc = 0.5 -> (100 + 500 + 300 + 900) / 4;
# (1, 1): on the last sample, x0 = x1 = 1 with weight 1 -> 900; (-3, 0.5): mirror reflects to 3 and clamps to 1 -> column 1.
KNOWN_2X2 = [
    ((0.25, 0.5), True, 375, 375, (551, 256), (551, 256)),        # interior
    ((-0.5, 0.5), False, 300, 450, (462, 128), (640, 384)),       # left
    ((1.5, 0.5), False, 600, 450, (818, 640), (640, 384)),        # right
    ((0.25, -0.5), False, 150, 375, (537.25, 128), (551, 256)),   # above: 0.25 * 101 + 512 = 537.25
    ((0.25, 1.5), False, 600, 375, (564.75, 384), (551, 256)),    # below: -75 + 127.75 + 512
    ((-0.5, -0.5), False, 100, 450, (512, 0), (640, 384)),        # a corner
    ((1.5, 1.5), False, 900, 450, (1023, 768), (640, 384)),       # the opposite corner
    ((1.0, 1.0), False, 900, 900, (1023, 768), (1023, 768)),      # exactly on the last sample
    ((-3.0, 0.5), False, 300, 600, (462, 128), (818, 640)),       # beyond the one reflection
]
# 3 x 4 luma: (1.5, 0.75) = .125 * 64 + .375 * 320 + .125 * 128 + .375 * 384 = 288; (1.5, 2.25): replicate yc = 2 -> (640 + 768) / 2,
# mirror yc = 1.75 -> .125 * 320 + .375 * 640 + .125 * 384 + .375 * 768 = 616
KNOWN_3X4 = [
    ((1.5, 0.75), True, 288, 288),
    ((-1.0, 0.75), False, 192, 256),
    ((4.5, 0.75), False, 384, 288),
    ((1.5, -0.75), False, 96, 288),
    ((1.5, 2.25), False, 704, 616),
    ((4.5, 2.25), False, 1023, 616),
    ((-1.0, -0.75), False, 0, 256),
    ((3.0, 0.75), False, 384, 384),                               # exactly on the last column
    ((-7.0, 0.75), False, 192, 384),
]


def _known_coords(points, ph, pw):
    import bicubic_ref as R
    xy = np.asarray([p[0] for p in points], np.float64)
    x_s, y_s = (2.0 * xy[:, 0] / pw - 1.0).astype(f32)[None], (2.0 * xy[:, 1] / ph - 1.0).astype(f32)[None]
    x, y = R.coords(ph, pw, x_s, y_s)
    assert np.array_equal(x[0], xy[:, 0]) and np.array_equal(y[0], xy[:, 1]), "the coordinates are exact in float32"
    assert R.valid(ph, pw, x_s, y_s)[0].tolist() == [p[1] for p in points]
    return x_s, y_s


@pytest.mark.parametrize("border", ["black", "replicate", "mirror", "keep"])
def test_render_bilinear_known_answers(border):
    import p010_ref
    cases = [(_words(L2)[..., None], False, KNOWN_2X2, lambda p: (p[2], p[3])),
             (np.stack([_words(U2), _words(V2)], axis=-1), True, KNOWN_2X2, lambda p: (p[4], p[5])),
             (_words(L34)[..., None], False, KNOWN_3X4, lambda p: (p[2], p[3]))]
    for plane, chroma, points, codes in cases:
        ph, pw = plane.shape[:2]
        assert ((plane & LOW) == LOW).all()
        x_s, y_s = _known_coords(points, ph, pw)
        v, written = p010_ref.render_bilinear(plane, x_s, y_s, border, chroma)
        assert v.dtype == f32 and v.shape == (1, len(points), plane.shape[2]) and written.shape == (1, len(points))
        valid = np.array([p[1] for p in points])
        assert np.array_equal(written[0], valid if border == "keep" else np.ones_like(valid))
        black = 512 if chroma else 0
        want = np.array([np.broadcast_to(codes(p)[border == "mirror"] if (p[1] or border in ("replicate", "mirror")) else black,
                                         plane.shape[2:]) for p in points])
        code = np.floor(want + 0.5).astype(np.uint16)
        assert np.array_equal(p010_ref.to_word(v, chroma)[0], code << 6), (border, chroma, plane.shape)
        assert np.abs(v[0].astype(np.float64) - (want - black) / 1023.0).max() <= 2e-7
        if border in ("black", "keep"):
            assert (v[0][~valid] == 0).all() and not np.signbit(v[0][~valid]).any()
    # a NaN coordinate: the black value, written under replicate / mirror
    nan = f32([[np.nan, 0.0]])
    for plane, chroma in ((cases[0][0], False), (cases[1][0], True)):
        for x_s, y_s in ((nan, nan[:, ::-1].copy()), (nan[:, ::-1].copy(), nan)):
            v, written = p010_ref.render_bilinear(plane, x_s, y_s, border, chroma)
            assert (v == 0).all() and written.tolist() == [[border != "keep"] * 2]
            assert (p010_ref.to_word(v, chroma) == ((512 << 6) if chroma else 0)).all()


def _noise_plane(seed, ph, pw, C):
    return _words(np.random.default_rng(seed).integers(0, 1024, (ph, pw, C)))


@pytest.mark.parametrize("border,mode", [("replicate", "border"), ("mirror", "reflection")])
def test_render_bilinear_f64_is_grid_sample(border, mode):
    """The float64 form against torch.nn.functional.grid_sample(mode="bilinear", align_corners=True) in float64 at the grid
    value 2 x / (pw - 1) - 1 of the UNMOVED float64 coordinate: an implementation that shares no text with the restatement.
    padding_mode="border" is the clamp; "reflection" reflects about the centres of the first and last sample, as `move` does,
    but as often as it takes, so the comparison covers the samples within ONE reflection, -(n - 1) <= x <= 2 (n - 1) on both
    axes.  1e-12 absolute: both sides are float64 evaluations of about twenty operations on values of magnitude <= 1."""
    import torch
    import bicubic_ref as R
    import border_ref as BR
    import p010_ref
    F = border_vectors("launch")
    for (ph, pw), C in (((6, 8), 1), ((5, 4), 2), ((6, 8), 2), ((5, 4), 1)):
        plane = np.stack([_noise_plane(10 * ph + pw + i, ph, pw, C) for i in range(len(F))])
        xs, ys = tps_grids(F, ph, pw)
        ok = np.stack([R.valid(ph, pw, xs[i], ys[i]) for i in range(len(F))])
        bad = ~ok
        for side in (bad[:, 0, :], bad[:, -1, :], bad[:, :, 0], bad[:, :, -1]):
            assert side.any(), "every side has invalid samples"
        x, y = BR.coords(ph, pw, xs, ys, np.float64)
        near = (x >= -(pw - 1)) & (x <= 2 * (pw - 1)) & (y >= -(ph - 1)) & (y <= 2 * (ph - 1))
        assert 2 * int((near & bad).sum()) >= int(bad.sum()) > 0, "%d of %d invalid samples lie within one reflection" % (
            (near & bad).sum(), bad.sum())
        for i in range(len(F)):
            v, _ = p010_ref.render_bilinear(plane[i], xs[i], ys[i], border, C == 2, dtype=np.float64)
            assert v.dtype == np.float64
            img = torch.from_numpy(p010_ref.samples(plane[i], C == 2, np.float64)).permute(2, 0, 1)[None]
            g = torch.from_numpy(np.stack([2.0 * x[i] / (pw - 1) - 1.0, 2.0 * y[i] / (ph - 1) - 1.0], axis=-1))[None]
            ref = torch.nn.functional.grid_sample(img, g, mode="bilinear", padding_mode=mode, align_corners=True)
            ref = ref[0].permute(1, 2, 0).numpy()
            err = np.abs(v - ref)[near[i]].max()
            assert err <= 1e-12, (border, ph, pw, C, i, err)


def _codes64(v, chroma):
    return np.clip(np.floor(v * 1023.0 + (512.5 if chroma else 0.5)), 0.0, 1023.0)


def _local_differences(s, xc, yc, n=4):
    """(Dx, Dy) [oh, ow]: the largest |difference of two neighbouring samples| along x (along y) over the n x n samples around
    the cell of (xc, yc), indices edge-replicated, all components: n = 4 holds the taps of the bilinear filter in every
    cell the two evaluations can fall in (a floor on the other side of an integer), n = 6 those of the bicubic one"""
    ph, pw = s.shape[:2]
    x0, y0 = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    cols = [np.clip(x0 - (n // 2 - 1) + k, 0, pw - 1) for k in range(n)]
    rows = [np.clip(y0 - (n // 2 - 1) + k, 0, ph - 1) for k in range(n)]
    Dx, Dy = np.zeros(xc.shape), np.zeros(xc.shape)
    for a in range(n):
        for b in range(n - 1):
            Dx = np.maximum(Dx, np.abs(s[rows[a], cols[b + 1]] - s[rows[a], cols[b]]).max(axis=-1))
            Dy = np.maximum(Dy, np.abs(s[rows[b + 1], cols[a]] - s[rows[b], cols[a]]).max(axis=-1))
    return Dx, Dy


def _coordinate_error(x, xc, mirror):
    """u (2 |x| + |xc|): x = ((x_s + 1) pw) / 2 carries two float32 roundings of relative size u = 2^-24 each (the division by 2
    is exact), mirror's (m + m) - x a third of at most u |(m + m) - x| = u |xc| where it is not clamped away (-x is exact);
    the clamp moves nothing further apart."""
    return U24 * (2.0 * np.abs(x) + (np.abs(xc) if mirror else 0.0))


@pytest.mark.parametrize("border", ["replicate", "mirror"])
@pytest.mark.parametrize("H,W", [(4, 4), (6, 8)])
def test_render_bilinear_f32_against_f64_in_codes(H, W, border):
    """For every sample of both planes, to_word of the float32 value is one of the codes that v64 - E ... v64 + E round to, and
    |v32 - v64| <= E, with E derived per sample, u = 2^-24, samples of magnitude <= 1:

      coordinates  |dx| <= u (2 |x| + |xc|) (_coordinate_error), the same for y.  The bilinear surface is continuous and
                   piecewise linear; along x its slope is a convex combination of differences of horizontally neighbouring
                   samples, so moving the coordinate by dx, dy changes the value by at most Dx |dx| + Dy |dy| with Dx, Dy
                   the largest such differences around the cell (_local_differences: wide enough for a floor that falls
                   on the other side of an integer).
      weights      at the float32 coordinate xc - x0f is exact (Sterbenz) and (x0f + 1) - xc is off by at most u, so each
                   product of two weights is off by at most u + u + u = 3 u (two inputs times a factor <= 1, one rounding).
      blend        the float32 sample is off by u |s|; a product w s by (3 + w + w) u |s| (the weight's error, the sample's
                   and its own rounding); the four products by (12 + 2) u since the weights sum to 1; the three additions
                   add u each on partial sums of magnitude <= 1: 17 u.  One more u covers the second-order terms: 18 u.

    Nothing is fitted: the worst ratio |v32 - v64| / E is printed.  At most 5 % of a case's samples may have two codes."""
    import bicubic_ref as R
    import border_ref as BR
    import p010_ref
    F = border_vectors("launch")
    worst, two, total = 0.0, 0, 0
    for p, (ph, pw, C) in enumerate(((H, W, 1), (H // 2, W // 2, 2))):
        xs, ys = tps_grids(F, ph, pw)
        for i in range(len(F)):
            plane = _noise_plane(1000 * H + 10 * W + 3 * p + i, ph, pw, C)
            v32, _ = p010_ref.render_bilinear(plane, xs[i], ys[i], border, p == 1)
            v64, _ = p010_ref.render_bilinear(plane, xs[i], ys[i], border, p == 1, dtype=np.float64)
            x, y = BR.coords(ph, pw, xs[i], ys[i], np.float64)
            xc, yc = BR.move(x, pw, border, np.float64), BR.move(y, ph, border, np.float64)
            Dx, Dy = _local_differences(p010_ref.samples(plane, p == 1, np.float64), xc, yc)
            E = (Dx * _coordinate_error(x, xc, border == "mirror") + Dy * _coordinate_error(y, yc, border == "mirror")
                 + 18 * U24)[..., None]
            worst = max(worst, float((np.abs(v32.astype(np.float64) - v64) / E).max()))
            lo, hi = _codes64(v64 - E, p == 1), _codes64(v64 + E, p == 1)
            got = (p010_ref.to_word(v32, p == 1) >> 6).astype(np.float64)
            assert ((lo <= got) & (got <= hi)).all(), (border, H, W, p, i)
            assert (hi - lo <= 1).all()
            two += int((hi != lo).sum())
            total += lo.size
        assert not R.valid(ph, pw, xs, ys).all()
    print("render_bilinear %s %dx%d: worst |v32 - v64| / E = %.3f, %d of %d samples have two codes" % (border, H, W, worst, two, total))
    assert worst <= 1.0
    assert 20 * two <= total, "%d of %d samples have a two-code set" % (two, total)


CUBIC_ABS = 1.375      # sum |w_k(t)| <= 1 + 2 * 0.75 t (1 - t) <= 1.375: w0 and w3 are the negative lobes A t (1 - t)^2, A t^2 (1 - t)
CUBIC_SLOPE = 2.625    # sum_j |sum_{k > j} w_k'(t)| <= 0.75 + 1.125 + 0.75: |w0'|, |w3'| <= 0.75 and (w2 + w3)' = -1.5 t^2 + 1.5 t + 0.75


def _cubic_weight_error(t):
    """The running error bound of bicubic_ref.weights_f32 at t (float64, exact), summed over the four weights, first order
    in u = 2^-24: every float32 operation's rounding is at most u |its result|, carried to the weight through the
    multiplications by the argument that follow it; t + 1 and 1 - t are each off by at most u, times the weight's slope; w3 =
    ((1 - w0) - w1) - w2 inherits the three errors and adds three roundings (the four polynomials sum to 1 exactly)."""
    import bicubic_ref as R
    u = t + 1.0
    s1 = -0.75 * u
    s2 = s1 + 3.75
    s3 = s2 * u
    s4 = s3 - 6.0
    s5 = s4 * u
    s6 = s5 + 3.0
    e0 = U24 * (np.abs(s1) * u * u + np.abs(s2) * u * u + np.abs(s3) * u + np.abs(s4) * u + np.abs(s5) + np.abs(s6)
                + np.abs(0.75 * (3.0 * t * t - 4.0 * t + 1.0)))

    def inner(t, slope):
        s1 = 1.25 * t
        s2 = s1 - 2.25
        s3 = s2 * t
        s4 = s3 * t
        return U24 * (np.abs(s1) * t * t + np.abs(s2) * t * t + np.abs(s3) * t + np.abs(s4) + np.abs(s4 + 1.0) + slope)
    v = 1.0 - t
    e1, e2 = inner(t, 0.0), inner(v, np.abs(3.75 * v * v - 4.5 * v))
    w = R.weights_f64(t)
    e3 = e0 + e1 + e2 + U24 * (np.abs(1.0 - w[0]) + np.abs(1.0 - w[0] - w[1]) + np.abs(w[3]))
    return e0 + e1 + e2 + e3


@pytest.mark.parametrize("border", ["replicate", "mirror"])
@pytest.mark.parametrize("H,W", [(4, 4), (6, 8)])
def test_render_bicubic_f32_against_f64_in_codes(H, W, border):
    """The bicubic restatement held the same way, with E per sample, u = 2^-24, samples of magnitude <= 1:

      coordinates  |dx|, |dy| as for the bilinear filter.  The cubic-convolution surface (edge-replicated taps) is C1; with
                   d_j the differences of neighbouring taps, dh/dx = sum_j (sum_{k > j} w_k') d_j, so |dv/dx| <= CUBIC_ABS
                   CUBIC_SLOPE Dx and the same along y, Dx, Dy over the 6 x 6 samples both evaluations can touch.
      weights      t = xc - floor(xc) is exact; _cubic_weight_error(t) bounds the sum of the four weights' errors, Ex and Ey.
                   They enter the value times |sample| <= 1 and times the other axis' sum |w| <= CUBIC_ABS.
      blend        a row: the sample's rounding and the product's, 2 u |w p| each term, and three additions on partial sums
                   <= CUBIC_ABS: 5 CUBIC_ABS u.  The column blend multiplies that by CUBIC_ABS and adds its own four
                   products and three additions on values <= CUBIC_ABS^2: 9 CUBIC_ABS^2 u = 17.02 u; 18 u with the
                   second-order terms.

    The worst ratio |v32 - v64| / E is printed; at most 5 % of a case's samples may have two codes."""
    import border_ref as BR
    import p010_ref
    F = border_vectors("launch")
    mirror = border == "mirror"
    worst, two, total = 0.0, 0, 0
    for p, (ph, pw, C) in enumerate(((H, W, 1), (H // 2, W // 2, 2))):
        xs, ys = tps_grids(F, ph, pw)
        for i in range(len(F)):
            plane = _noise_plane(2000 * H + 10 * W + 3 * p + i, ph, pw, C)
            v32, _ = p010_ref.render_bicubic(plane, xs[i], ys[i], border, p == 1)
            v64, _ = p010_ref.render_bicubic(plane, xs[i], ys[i], border, p == 1, dtype=np.float64)
            x, y = BR.coords(ph, pw, xs[i], ys[i], np.float64)
            xc, yc = BR.move(x, pw, border, np.float64), BR.move(y, ph, border, np.float64)
            x32, y32 = BR.coords(ph, pw, xs[i], ys[i])
            xc32, yc32 = BR.move(x32, pw, border).astype(np.float64), BR.move(y32, ph, border).astype(np.float64)
            Dx, Dy = _local_differences(p010_ref.samples(plane, p == 1, np.float64), xc, yc, n=6)
            E = (CUBIC_ABS * CUBIC_SLOPE * (Dx * _coordinate_error(x, xc, mirror) + Dy * _coordinate_error(y, yc, mirror))
                 + CUBIC_ABS * (_cubic_weight_error(xc32 - np.floor(xc32)) + _cubic_weight_error(yc32 - np.floor(yc32)))
                 + 18 * U24)[..., None]
            worst = max(worst, float((np.abs(v32.astype(np.float64) - v64) / E).max()))
            lo, hi = _codes64(v64 - E, p == 1), _codes64(v64 + E, p == 1)
            got = (p010_ref.to_word(v32, p == 1) >> 6).astype(np.float64)
            assert ((lo <= got) & (got <= hi)).all(), (border, H, W, p, i)
            assert (hi - lo <= 1).all()
            two += int((hi != lo).sum())
            total += lo.size
    print("render_bicubic %s %dx%d: worst |v32 - v64| / E = %.3f, %d of %d samples have two codes" % (border, H, W, worst, two, total))
    assert worst <= 1.0
    assert 20 * two <= total, "%d of %d samples have a two-code set" % (two, total)


@pytest.mark.parametrize("border", ["replicate", "mirror"])
def test_far_launch_gives_one_corner_in_the_restatement(border):
    """F_t = (-2.5, +2.5) at all 25 points moves every coordinate out through the left and the bottom side.  Replicate clamps
    each to (0, ph - 1): the bottom-left sample.  Mirror reflects once, and where the coordinate lies beyond that reflection
    (x <= -(pw - 1), y >= 2 (ph - 1)) the clamp lands on the opposite side: the top-right sample.  There the bilinear weights are
    1, 0, 0, 0 and the bicubic ones 0, 1, 0, 0 in both directions, exactly (t = 0: every polynomial of cubic_weights is exact), so
    BOTH restatements give the corner sample itself, bit for bit."""
    import border_ref as BR
    import p010_ref
    F = border_vectors("far")
    for ph, pw, C in ((6, 8, 1), (3, 4, 2), (2, 2, 2), (10, 520, 1)):
        plane = _noise_plane(ph + pw, ph, pw, C)
        xs, ys = tps_grids(F[:1], ph, pw)
        x, y = BR.coords(ph, pw, xs[0], ys[0], np.float64)
        assert (x < 0).all() and (y > ph - 1).all()
        sel = np.ones(x.shape, bool) if border == "replicate" else (x <= -(pw - 1)) & (y >= 2 * (ph - 1))
        assert sel.any()
        corner = plane[ph - 1, 0] if border == "replicate" else plane[0, pw - 1]
        for render in (p010_ref.render_bilinear, p010_ref.render_bicubic):
            v, _ = render(plane, xs[0], ys[0], border, C == 2)
            assert np.array_equal(v[sel], np.broadcast_to(p010_ref.samples(corner, C == 2), v[sel].shape)), (render.__name__, ph, pw)
            assert (p010_ref.to_word(v, C == 2)[sel] == (corner & ~np.uint16(LOW))).all()
