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
