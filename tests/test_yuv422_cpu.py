"""No-GPU checks of 4:2:2 frames (include/dvsg_amd.h, "Chroma sampling"): the view constructor's argument checks and the
getter, the Python names, what `plan_step` decides for "nv16" and "p210", C422 / C422p10 over Y4M as an opt-in, the four
repacks against tests/yuv422_ref.py's index formulas, and the pipe's refusal of mixed chroma samplings."""
import ctypes
import io
import os
import threading

import numpy as np
import pytest
import torch

import yuv422_ref as Y
from coupe.dvsg_amd import y4m
from coupe.dvsg_amd.online import plan_step
from coupe.dvsg_amd.pipe import stabilize_pipes


# ---------------------------------------------------------------------------------------------------------------------
# 1. dvsg_locnet_view_create_chroma / dvsg_locnet_render_chroma
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def test_view_create_chroma_rejects_bad_arguments(lib):
    f = lib.dvsg_locnet_view_create_chroma
    view = ctypes.c_void_p(5)
    assert f(None, 1, ctypes.byref(view)) == -1 and b"NULL net" in lib.dvsg_last_error_string()
    assert b"dvsg_locnet_view_create_chroma" in lib.dvsg_last_error_string()
    assert f(8, 1, None) == -1 and b"NULL view" in lib.dvsg_last_error_string()
    for bad in (-1, 2, 7):   # decided before the handle (here not even a handle) is read
        view = ctypes.c_void_p(5)
        assert f(8, bad, ctypes.byref(view)) == -1
        err = lib.dvsg_last_error_string()
        assert ("chroma_format=%d" % bad).encode() in err and b"dvsg_locnet_view_create_chroma" in err
        assert view.value is None
    assert lib.dvsg_locnet_render_chroma(None) == 0
    assert lib.dvsg_abi_version() == 1


def test_python_names():
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import CHROMAS, SURFACES, check_chroma
    assert CHROMAS == {"420": 0, "422": 1} and SURFACES == {"nv12": 0, "p010": 1}
    assert check_chroma("422") == "422" and check_chroma("420") == "420"
    for bad in ("444", "4:2:2", 422, 1, None):
        with pytest.raises(ValueError, match="chroma"):
            check_chroma(bad)
    assert {"dvsg_locnet_view_create_chroma", "dvsg_locnet_render_chroma"} <= set(_lib.SIGNATURES)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dvsg_amd.h")).read()
    assert "#define DVSG_CHROMA_420 0" in header and "#define DVSG_CHROMA_422 1" in header and "Chroma sampling" in header


# ---------------------------------------------------------------------------------------------------------------------
# 2. plan_step for the two formats
# ---------------------------------------------------------------------------------------------------------------------
H, W = 32, 48


def _streams(sids):
    table = {sid: [ring, 10 * ring + 3] for ring, sid in enumerate(sids)}
    return table, table.__getitem__


def test_plan_step_keys_and_run_order():
    feed = {"big": np.zeros((2 * 64, 96), np.uint8), "small_a": torch.zeros((2 * 20, 32), dtype=torch.uint8),
            "small_b": np.zeros((2 * 20, 32), np.uint8)}
    rows, runs = plan_step(feed, _streams(list(feed))[1], H, W, frame_format="nv16", source_res=True)
    assert [r.sid for r in rows] == ["small_a", "small_b", "big"] and runs == [(0, 2), (2, 3)]
    assert [r.key for r in rows] == [(20, 32), (20, 32), (64, 96)] and not any(r.words for r in rows)
    assert [r.host for r in rows] == [False, True, True]
    # P210: the uint8 form [2 H0, 2 W0] and uint16 words [2 H0, W0] are one key; the word form is flagged
    feed = {"bytes": np.zeros((2 * 20, 2 * 32), np.uint8), "words": np.zeros((2 * 20, 32), np.uint16)}
    rows, runs = plan_step(feed, _streams(list(feed))[1], H, W, frame_format="p210", source_res=True)
    assert [r.key for r in rows] == [(20, 32), (20, 32)] and runs == [(0, 2)]
    assert [r.words for r in rows] == [False, True] and all(r.t.dtype == torch.uint8 and tuple(r.t.shape) == (40, 64) for r in rows)
    # the same rows are another size as 4:2:0: [48, 32] is H0 = 24 for nv16 and H0 = 32 for nv12
    f = {"a": np.zeros((48, 32), np.uint8)}
    assert plan_step(f, _streams(["a"])[1], H, W, frame_format="nv16", source_res=True)[0][0].key == (24, 32)
    assert plan_step(f, _streams(["a"])[1], H, W, frame_format="nv12", source_res=True)[0][0].key == (32, 32)
    # out_size: the factors are those of the luma size
    with pytest.raises(ValueError, match="minification"):
        plan_step({"a": np.zeros((2 * 64, 96), np.uint8)}, _streams(["a"])[1], H, W, frame_format="nv16", source_res=True,
                  out_size=(12, 20))


@pytest.mark.parametrize("fmt, frame, exc, message", [
    ("nv16", np.zeros((2 * 21, 32), np.uint8), ValueError, r"\[2\*H0, W0\] needs even H0, W0 >= 4"),        # odd H0
    ("nv16", np.zeros((41, 32), np.uint8), ValueError, r"\[2\*H0, W0\]"),                                    # odd rows
    ("nv16", np.zeros((40, 31), np.uint8), ValueError, r"\[2\*H0, W0\] needs even H0, W0 >= 4"),
    ("nv16", np.zeros((4, 32), np.uint8), ValueError, r"even H0, W0 >= 4"),                                  # H0 = 2
    ("p210", np.zeros((40, 62), np.uint8), ValueError, r"\[2\*H0, 2\*W0\] needs even H0, W0 >= 4"),          # W0 = 31
    ("p210", np.zeros((42, 32), np.uint16), ValueError, r"\[2\*H0, 2\*W0\]"),                                # odd H0, as words
    ("nv16", np.zeros((40, 32), np.float32), ValueError, "not float frames"),
    ("p210", np.zeros((40, 64), np.float64), ValueError, "not float frames"),
    ("nv16", np.zeros((40, 32, 3), np.uint8), ValueError, r"an NV16 frame must be \[2\*H0, W0\]"),
    ("p210", np.zeros((40,), np.uint8), ValueError, r"a P210 frame must be \[2\*H0, 2\*W0\]"),
    ("nv16", np.zeros((40, 32), np.uint16), TypeError, "NV16 frames must be uint8, got"),
    ("p210", np.zeros((40, 32), np.int32), TypeError, "P210 frames must be uint8 or uint16"),
])
def test_plan_step_refusals(fmt, frame, exc, message):
    table, stream_of = _streams(["ok", "bad"])
    good = np.zeros((40, 64 if fmt == "p210" else 32), np.uint8)
    with pytest.raises(exc, match=message):
        plan_step({"ok": good, "bad": frame}, stream_of, H, W, frame_format=fmt, source_res=True)
    assert table == {"ok": [0, 3], "bad": [1, 13]}


def test_online_options_raise_before_the_device():
    from coupe.dvsg_amd._lib import DvsgError
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    model = StabNet(32, 48)
    for fmt in ("nv16", "p210"):
        for kw, name in [(dict(side_by_side=True), "side_by_side"), (dict(as_uint8=True), "as_uint8"),
                         (dict(channel_order="bgr"), "channel_order"), (dict(out_size=(11, 20)), "even"),
                         (dict(out_size=(12, 20), border="keep"), "keep")]:
            with pytest.raises(ValueError, match=name):
                OnlineStabilizer(model, frame_format=fmt, **kw)
        with pytest.raises(DvsgError, match="weights"):   # the source-size options are accepted as for "nv12"
            OnlineStabilizer(model, frame_format=fmt, render_filter="bicubic", border="keep", strength=0.5, rigidity=1.0,
                             shape_model="similarity", crop="auto")
        assert stabilize_clips(model, [], frame_format=fmt) == []
    with pytest.raises(ValueError, match="'nv16' or 'p210'"):
        OnlineStabilizer(model, frame_format="nv24")


# ---------------------------------------------------------------------------------------------------------------------
# 3. C422 and C422p10 over Y4M: an opt-in
# ---------------------------------------------------------------------------------------------------------------------
FW, FH = 8, 6
HEAD8 = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C422 XYSCSS=422 XCOLORRANGE=FULL\n" % (FW, FH)
HEAD10 = b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C422p10 XYSCSS=422P10\n" % (FW, FH)
BOTH = ("420", "422")


def frames8(seed, n):
    """n C422 frames as the stream's bytes, uint8 [n, 2 H, W]"""
    return np.random.default_rng(seed).integers(0, 256, (n, 2 * FH, FW), dtype=np.uint8)


def frames10(seed, n):
    """n C422p10 frames as the stream's bytes, uint8 [n, 2 H, 2 W]: samples in [0, 1023], 0 and 1023 among them"""
    s = np.random.default_rng(seed).integers(0, 1024, (n, 2 * FH, FW), dtype=np.uint16)
    s[:, 0, 0], s[:, 0, 1], s[:, -1, -1] = 0, 1023, 1023
    return s.astype("<u2").view(np.uint8)


def stream(head, frames):
    return head + b"".join(b"FRAME\n" + f.tobytes() for f in frames)


def test_y4m_422_is_parsed_when_asked_for():
    fr = frames8(1, 3)
    r = y4m.Y4MReader(io.BytesIO(stream(HEAD8, fr)), chromas=BOTH)
    assert (r.width, r.height, r.fps, r.colorspace, r.layout) == (FW, FH, (25, 1), "422", "i422")
    assert r.frame_shape == (2 * FH, FW) and r.frame_bytes == 2 * FW * FH and r.tags == ("XYSCSS=422", "XCOLORRANGE=FULL")
    got = list(r)
    assert len(got) == 3 and all(g.dtype == np.uint8 and np.array_equal(g, f) for g, f in zip(got, fr))
    fr = frames10(2, 2)
    r = y4m.Y4MReader(io.BytesIO(stream(HEAD10, fr)), depths=(8, 10), chromas=BOTH)
    assert (r.colorspace, r.layout, r.frame_shape, r.frame_bytes) == ("422p10", "i422p10", (2 * FH, 2 * FW), 4 * FW * FH)
    assert all(np.array_equal(g, f) for g, f in zip(list(r), fr))
    # 4:2:0 through the same reader is what it was
    r = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1 C420jpeg\n"), depths=(8, 10), chromas=BOTH)
    assert r.layout == "i420" and r.frame_shape == (9, 8) and y4m.Y4MReader.layout == "i420"
    r = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1\n"), chromas=BOTH)
    assert r.layout == "i420" and r.frame_shape == (9, 8)
    assert y4m.LAYOUT_BITS["i422"] == 8 and y4m.LAYOUT_BITS["p210"] == 10 and set(y4m.LAYOUT_CHROMA) == set(y4m.LAYOUT_BITS)
    assert {k for k, v in y4m.LAYOUT_CHROMA.items() if v == "422"} == {"i422", "i422p10", "nv16", "p210"}


def test_y4m_defaults_and_partial_opt_ins_still_refuse():
    for kw in ({}, dict(depths=(8, 10)), dict(chromas=("420",)), dict(depths=(8, 10), chromas=("420",))):
        with pytest.raises(y4m.Y4MError, match="C422"):
            y4m.Y4MReader(io.BytesIO(stream(HEAD8, frames8(1, 1))), **kw)
        with pytest.raises(y4m.Y4MError, match="C422p10"):
            y4m.Y4MReader(io.BytesIO(stream(HEAD10, frames10(1, 1))), **kw)
    with pytest.raises(y4m.Y4MError, match="C422p10"):       # 4:2:2 asked for, ten bits not
        y4m.Y4MReader(io.BytesIO(HEAD10), chromas=BOTH)
    with pytest.raises(y4m.Y4MError, match="C420jpeg"):      # 4:2:2 only
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1 C420jpeg\n"), chromas=("422",))
    with pytest.raises(y4m.Y4MError, match="no C tag"):
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1\n"), chromas=("422",))
    for tag in ("C444", "C444p10", "C411", "C422p12", "Cmono"):
        with pytest.raises(y4m.Y4MError, match=tag):
            y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1 %s\n" % tag.encode()), depths=(8, 10), chromas=BOTH)
    with pytest.raises(y4m.Y4MError, match="H7"):            # odd heights are out of scope for 4:2:2 too
        y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H7 F25:1 C422\n"), chromas=BOTH)
    for bad in ((), ("444",), ("420", "411"), (422,)):
        with pytest.raises(ValueError, match="chromas"):
            y4m.Y4MReader(io.BytesIO(HEAD8), chromas=bad)
        with pytest.raises(ValueError, match="chromas"):
            y4m.Y4MWriter(io.BytesIO(), FW, FH, 25, chromas=bad)
    with pytest.raises(ValueError, match="422"):
        y4m.Y4MWriter(io.BytesIO(), FW, FH, 25, colorspace="422")
    with pytest.raises(y4m.Y4MError, match="422p10"):
        y4m.Y4MWriter(io.BytesIO(), FW, FH, 25, colorspace="422p10")
    with pytest.raises(y4m.Y4MError, match="444"):
        y4m.Y4MWriter(io.BytesIO(), FW, FH, 25, colorspace="444", chromas=BOTH)


def test_y4m_422_writer_round_trip():
    for head, fr, cs, layout, shape in ((HEAD8, frames8(3, 4), "422", "i422", (2 * FH, FW)),
                                        (HEAD10, frames10(4, 4), "422p10", "i422p10", (2 * FH, 2 * FW))):
        src = y4m.Y4MReader(io.BytesIO(head), depths=(8, 10), chromas=BOTH)
        out = io.BytesIO()
        w = y4m.Y4MWriter(out, FW, FH, src.fps, aspect=src.aspect, colorspace=cs, tags=src.tags, chromas=BOTH)
        assert (w.layout, w.frame_shape, w.frame_bytes) == (layout, shape, shape[0] * shape[1])
        for f in fr:
            w.write(f)
        w.flush()
        assert out.getvalue() == stream(head, fr)
        with pytest.raises(ValueError, match="bytes"):
            w.write(np.zeros((3 * FH // 2, shape[1]), np.uint8))
    assert y4m.Y4MWriter(io.BytesIO(), FW, FH, 25, chromas=BOTH).layout == "i420"   # the default colorspace stays 4:2:0


@pytest.mark.parametrize("chunk", [1, 3, 7])
@pytest.mark.parametrize("ten", [False, True], ids=["C422", "C422p10"])
def test_y4m_422_from_a_pipe_with_short_reads(ten, chunk):
    fr = frames10(5, 2) if ten else frames8(5, 2)
    data = stream(HEAD10 if ten else HEAD8, fr)
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb", buffering=0) as f:
            for i in range(0, len(data), chunk):
                f.write(data[i:i + chunk])
    t = threading.Thread(target=feed)
    t.start()
    try:
        with os.fdopen(rd, "rb", buffering=0) as f:
            got = list(y4m.Y4MReader(f, depths=(8, 10), chromas=BOTH))
    finally:
        t.join(30)
    assert len(got) == 2 and all(np.array_equal(g, f) for g, f in zip(got, fr))


def test_truncated_frames_name_the_index_and_the_byte_counts():
    data = stream(HEAD8, frames8(6, 3))
    per = len(b"FRAME\n") + 2 * FW * FH
    assert 2 * FW * FH == 96
    r = y4m.Y4MReader(io.BytesIO(data[:len(HEAD8) + 2 * per + 6 + 42]), chromas=BOTH)
    assert r.read() is not None and r.read() is not None
    with pytest.raises(y4m.Y4MError, match=r"frame 2 .*\b42 of 96 bytes"):
        r.read()
    data = stream(HEAD10, frames10(6, 2))
    r = y4m.Y4MReader(io.BytesIO(data[:len(HEAD10) + 6 + 192 + 6 + 100]), depths=(8, 10), chromas=BOTH)
    assert r.read() is not None
    with pytest.raises(y4m.Y4MError, match=r"frame 1 .*\b100 of 192 bytes"):
        r.read()
    raw = y4m.RawNV16Reader(io.BytesIO(bytes(96 + 95)), FW, FH)
    assert raw.layout == "nv16" and raw.frame_shape == (12, 8) and raw.read() is not None
    with pytest.raises(y4m.Y4MError, match=r"frame 1 .*\b95 of 96 bytes"):
        raw.read()
    raw = y4m.RawP210Reader(io.BytesIO(bytes(192 + 191)), FW, FH)
    assert raw.layout == "p210" and raw.frame_shape == (12, 16) and raw.read() is not None
    with pytest.raises(y4m.Y4MError, match=r"frame 1 .*\b191 of 192 bytes"):
        raw.read()


def test_raw_writers():
    for cls, layout, fr in ((y4m.RawNV16Writer, "nv16", frames8(7, 2)), (y4m.RawP210Writer, "p210", frames10(7, 2))):
        out = io.BytesIO()
        w = cls(out, FW, FH)
        for f in fr:
            w.write(f)
        assert w.layout == layout and out.getvalue() == fr.tobytes() and w.frames_written == 2
        with pytest.raises(y4m.Y4MError, match="7"):
            cls(io.BytesIO(), 7, 4)
        with pytest.raises(ValueError, match="bytes"):
            w.write(np.zeros((3 * FH // 2, fr.shape[2]), np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the four repacks against the index formulas
# ---------------------------------------------------------------------------------------------------------------------
def test_the_index_formulas_are_inverse_and_place_known_samples():
    Hh, Ww = 4, 6
    planar = np.arange(2 * Hh * Ww, dtype=np.uint8).reshape(2 * Hh, Ww)
    semi = Y.i422_to_nv16(planar)
    assert np.array_equal(semi[:Hh], planar[:Hh])
    u, v = planar.reshape(-1)[Hh * Ww:Hh * Ww + Hh * Ww // 2].reshape(Hh, Ww // 2), planar.reshape(-1)[Hh * Ww + Hh * Ww // 2:].reshape(Hh, Ww // 2)
    assert np.array_equal(semi[Hh:, 0::2], u) and np.array_equal(semi[Hh:, 1::2], v)   # UV row r = U row r, V row r
    assert np.array_equal(Y.nv16_to_i422(semi), planar)


def test_repacks_against_the_index_formulas():
    Hh, Ww = 6, 10
    rng = np.random.default_rng(8)
    p8 = rng.integers(0, 256, (2, 2 * Hh, Ww), dtype=np.uint8)
    src = torch.from_numpy(p8.copy())
    got = y4m.i422_to_nv16(src)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 12, 10)
    assert np.array_equal(got.numpy(), np.stack([Y.i422_to_nv16(f) for f in p8]))
    assert np.array_equal(y4m.nv16_to_i422(got).numpy(), p8)
    assert np.array_equal(y4m.nv16_to_i422(src).numpy(), np.stack([Y.nv16_to_i422(f) for f in p8]))
    assert np.array_equal(y4m.i422_to_nv16(src[0]).numpy(), Y.i422_to_nv16(p8[0]))   # one frame
    out = torch.empty_like(src)
    assert y4m.i422_to_nv16(src, out=out) is out and torch.equal(out, got)
    assert y4m.nv16_to_i422(got, out=out) is out and torch.equal(out, src)
    for f in (y4m.i422_to_nv16, y4m.nv16_to_i422):
        with pytest.raises(ValueError, match="not be src"):
            f(src, out=src)
        with pytest.raises(ValueError, match="out"):
            f(src, out=torch.empty((2, 12, 12), dtype=torch.uint8))
        with pytest.raises(ValueError, match="even H"):
            f(torch.zeros((10, 10), dtype=torch.uint8))   # H = 5
    # ten bits: every value; high bits of planar samples and low bits of P210 words are dropped
    s = rng.integers(0, 1024, (2 * Hh, Ww), dtype=np.uint16)
    s.reshape(-1)[:4] = (0, 1023, 512, 1)
    planar = s.astype("<u2").view(np.uint8)
    want = Y.i422p10_to_p210(planar)
    assert (want.view("<u2") >= 0x8000).any(), "no word has its top bit set"
    src = torch.from_numpy(planar.copy())
    got = y4m.i422p10_to_p210(src)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (12, 20) and np.array_equal(got.numpy(), want)
    assert np.array_equal(y4m.p210_to_i422p10(got).numpy(), planar) and np.array_equal(Y.p210_to_i422p10(want), planar)
    dirty = torch.from_numpy((want.view("<u2") | np.uint16(0x3F)).astype("<u2").view(np.uint8).copy())
    assert np.array_equal(y4m.p210_to_i422p10(dirty).numpy(), planar)
    high = torch.from_numpy((s | np.uint16(0xFC00)).astype("<u2").view(np.uint8).copy())
    assert np.array_equal(y4m.i422p10_to_p210(high).numpy(), want)
    batch = torch.stack([src, src.flip(0).contiguous()])
    out = torch.empty_like(batch)
    assert y4m.i422p10_to_p210(batch, out=out) is out and torch.equal(out[0], got)
    for f in (y4m.i422p10_to_p210, y4m.p210_to_i422p10):
        with pytest.raises(ValueError, match="not be src"):
            f(src, out=src)
        with pytest.raises(ValueError, match="uint8"):
            f(src.view(torch.int16))
        with pytest.raises(ValueError, match="out"):
            f(src, out=torch.empty((12, 10), dtype=torch.uint8))


def test_even_rows_surface():
    b = Y.Batch422(3, 2, 6, 8)
    luma, chroma = b.planes()
    seen = Y.even_rows_surface(b.buf)
    assert seen.shape == (2, 9, 8) and np.array_equal(seen[:, :6], luma[..., 0])
    assert np.array_equal(seen[:, 6:].reshape(2, 3, 4, 2), chroma[:, 0::2])
    w = Y.Batch422(4, 2, 6, 8, words=True, low=0x2B)
    luma, chroma = w.planes()
    seen = Y.even_rows_surface(w.buf, words=True)
    assert seen.shape == (2, 9, 8) and np.array_equal(seen[:, :6], (luma[..., 0] >> 8).astype(np.uint8))
    assert np.array_equal(seen[:, 6:].reshape(2, 3, 4, 2), (chroma[:, 0::2] >> 8).astype(np.uint8))
    # a batch with a pitch, an offset UV plane and a tail keeps its planes apart from everything else
    p = Y.Batch422(5, 3, 6, 8, words=True, pitch=22, uv_row=7, tail=1, fill=0xA5)
    assert p.buf.shape == (3, 14, 22) and p.frame_stride == 14 * 22 and p.uv_offset == 7 * 22
    assert p.outside().size == 3 * (14 * 22 - 2 * 6 * 16) and p.planes()[1].shape == (3, 6, 4, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 5. stabilize_pipes: a 4:2:2 run with the step replaced by the identity, and the mixed-sampling refusal
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


@pytest.mark.parametrize("ten", [False, True], ids=["C422", "C422p10"])
def test_a_422_source_passes_through_bit_for_bit(ten):
    head, fr = (HEAD10, frames10(9, 5)) if ten else (HEAD8, frames8(9, 5))
    out, raw = io.BytesIO(), io.BytesIO()
    src = y4m.Y4MReader(io.BytesIO(stream(head, fr)), depths=(8, 10), chromas=BOTH)
    snk = y4m.Y4MWriter(out, FW, FH, src.fps, aspect=src.aspect, colorspace=src.colorspace, tags=src.tags, chromas=BOTH)
    seen = []

    def step(frames):
        seen.extend(f.cpu().numpy().copy() for f in frames.values())
        return dict(frames)
    semi = np.stack([(Y.i422p10_to_p210 if ten else Y.i422_to_nv16)(f) for f in fr])
    Reader, Writer = (y4m.RawP210Reader, y4m.RawP210Writer) if ten else (y4m.RawNV16Reader, y4m.RawNV16Writer)
    stats, err = call(None, [src, Reader(io.BytesIO(semi.tobytes()), FW, FH)], [snk, Writer(raw, FW, FH)], depth=3, _step_fn=step)
    assert err is None and [s["frames"] for s in stats] == [5, 5]
    assert out.getvalue() == stream(head, fr) and raw.getvalue() == semi.tobytes()
    assert len(seen) == 10 and all(np.array_equal(a, semi[k // 2]) for k, a in enumerate(seen))   # the step saw NV16 / P210


def test_mixed_chroma_samplings_are_refused_before_any_read():
    class Source(object):
        width, height, frame_shape, layout = FW, FH, (2 * FH, FW), "i422"
        reads = 0

        def readinto(self, buf):
            Source.reads += 1
            return False
    plain = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1\n"))
    with pytest.raises(ValueError, match=r"sink 0 is 4:2:0 \(i420\) in a 4:2:2 run.*chroma sampling"):
        stabilize_pipes(None, [Source()], [y4m.Y4MWriter(io.BytesIO(), FW, FH, 25)], _step_fn=identity)
    with pytest.raises(ValueError, match=r"source 1 is 4:2:2 \(i422\) in a 4:2:0 run"):
        stabilize_pipes(None, [plain, Source()], [y4m.RawNV12Writer(io.BytesIO(), FW, FH), y4m.RawNV16Writer(io.BytesIO(), FW, FH)],
                        _step_fn=identity)
    with pytest.raises(ValueError, match=r"sink 0 is 4:2:2 \(nv16\)"):
        stabilize_pipes(None, [plain], [y4m.RawNV16Writer(io.BytesIO(), FW, FH)], _step_fn=identity)
    with pytest.raises(ValueError, match="bit depth"):     # the depth is still checked, and first
        stabilize_pipes(None, [Source()], [y4m.RawP210Writer(io.BytesIO(), FW, FH)], _step_fn=identity)
    with pytest.raises(ValueError, match=r"frame_shape .* is not \[2 H, W\]"):
        class Wrong(Source):
            frame_shape = (3 * FH // 2, FW)
        stabilize_pipes(None, [Wrong()], [y4m.RawNV16Writer(io.BytesIO(), FW, FH)], _step_fn=identity)
    assert Source.reads == 0 and plain.frames_read == 0
    assert [t.name for t in threading.enumerate() if t.name.startswith("stabilize_pipes")] == []


def test_front_end_arguments():
    from coupe.dvsg_amd import pipe
    for fmt in ("nv16", "p210"):
        args = pipe._arguments(["--synthetic-weights", "--format", fmt, "--size", "8x6"])
        assert args.format == fmt and args.output_format == fmt and args.size == (8, 6)
        with pytest.raises(pipe._UsageError, match="--size"):
            pipe._arguments(["--synthetic-weights", "--format", fmt])
        args = pipe._arguments(["--synthetic-weights", "--format", "y4m", "--output-format", fmt])
        assert args.output_format == fmt
    with pytest.raises(pipe._UsageError, match="nv24"):
        pipe._arguments(["--synthetic-weights", "--format", "nv24", "--size", "8x6"])
    assert pipe._RAW_COLORSPACE == {"p010": "420p10", "nv16": "422", "p210": "422p10"}
    assert pipe._FRAME_FORMAT == {(8, "420"): "nv12", (10, "420"): "p010", (8, "422"): "nv16", (10, "422"): "p210"}
