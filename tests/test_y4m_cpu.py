"""CPU: the Y4M / raw NV12 framing of coupe/dvsg_amd/y4m.py against bytes written out by hand, short reads, the writer ->
reader round trip, and the I420 <-> NV12 repack against its index formula."""
import io
import os
import threading

import numpy as np
import pytest

from coupe.dvsg_amd import y4m
from coupe.dvsg_amd.y4m import Y4MError


def payload(seed, W, H, n=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 3 * H // 2, W), dtype=np.uint8)


def stream(header, frames, frame_header=b"FRAME\n"):
    return header + b"".join(frame_header + f.tobytes() for f in frames)


FULL_HEADER = b"YUV4MPEG2 W8 H6 F30000:1001 Ip A128:117 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\n"


def test_header_with_all_tags():
    frames = payload(1, 8, 6, 3)
    r = y4m.Y4MReader(io.BytesIO(stream(FULL_HEADER, frames)))
    assert (r.width, r.height) == (8, 6) and r.frame_shape == (9, 8) and r.frame_bytes == 72 and r.layout == "i420"
    assert tuple(r.fps) == (30000, 1001) and tuple(r.aspect) == (128, 117)
    assert r.interlace == "p" and r.colorspace == "420mpeg2"
    assert r.tags == ("XYSCSS=420MPEG2", "XCOLORRANGE=FULL")          # verbatim, in order
    got = list(r)
    assert len(got) == 3
    for g, f in zip(got, frames):
        assert g.dtype == np.uint8 and g.shape == (9, 8) and g.tobytes() == f.tobytes()


def test_no_c_tag_no_i_tag_and_frame_parameters():
    frames = payload(2, 4, 4, 2)
    r = y4m.Y4MReader(io.BytesIO(stream(b"YUV4MPEG2 W4 H4 F25:1\n", frames, b"FRAME Ip Xsomething=1\n")))
    assert r.colorspace is None and r.interlace is None and r.aspect is None and r.tags == ()
    assert [g.tobytes() for g in r] == [f.tobytes() for f in frames]


@pytest.mark.parametrize("c", ["420", "420jpeg", "420mpeg2", "420paldv"])
def test_every_8_bit_420_form_is_accepted(c):
    r = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 F25:1 I? C" + c.encode() + b"\n"))
    assert r.colorspace == c and r.interlace == "?"


@pytest.mark.parametrize("header,tag", [
    (b"YUV4MPEG2 W8 H6 F25:1 C422\n", "C422"),
    (b"YUV4MPEG2 W8 H6 F25:1 C444\n", "C444"),
    (b"YUV4MPEG2 W8 H6 F25:1 Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W8 H6 F25:1 C420p10\n", "C420p10"),
    (b"YUV4MPEG2 W8 H6 F25:1 C444p16\n", "C444p16"),
    (b"YUV4MPEG2 W8 H6 F25:1 It\n", "It"),
    (b"YUV4MPEG2 W8 H6 F25:1 Ib\n", "Ib"),
    (b"YUV4MPEG2 W8 H6 F25:1 Im\n", "Im"),
    (b"YUV4MPEG2 W7 H6 F25:1\n", "W7"),
    (b"YUV4MPEG2 W8 H5 F25:1\n", "H5"),
    (b"YUV4MPEG2 W2 H6 F25:1\n", "W2"),
    (b"YUV4MPEG2 W8 H2 F25:1\n", "H2"),
    (b"YUV4MPEG2 H6 F25:1\n", "no W tag"),
    (b"YUV4MPEG2 W8 F25:1\n", "no H tag"),
    (b"YUV4MPEG3 W8 H6 F25:1\n", "YUV4MPEG2"),
    (b"RIFF....AVI LIST\n", "YUV4MPEG2"),
])
def test_refusals_name_the_tag_before_any_frame_is_read(header, tag):
    f = io.BytesIO(stream(header, payload(3, 8, 6, 1)))
    with pytest.raises(Y4MError, match=tag) as e:
        y4m.Y4MReader(f)
    assert isinstance(e.value, ValueError)
    assert f.tell() <= len(header)


def test_a_stream_that_ends_after_the_header_has_no_frames():
    r = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W8 H6 F25:1\n"))
    assert list(r) == [] and r.read() is None
    assert not r.readinto(np.empty((9, 8), np.uint8))


def test_a_truncated_last_frame_names_its_index_and_the_bytes_received():
    data = stream(b"YUV4MPEG2 W8 H6 F25:1\n", payload(4, 8, 6, 3))
    r = y4m.Y4MReader(io.BytesIO(data[:-30]))
    assert r.read() is not None and r.read() is not None
    with pytest.raises(Y4MError, match=r"frame 2 .*\b42 of 72 bytes"):
        r.read()
    raw = y4m.RawNV12Reader(io.BytesIO(payload(4, 8, 6, 2).tobytes()[:-1]), 8, 6)
    assert raw.read() is not None
    with pytest.raises(Y4MError, match=r"frame 1 .*\b71 of 72 bytes"):
        raw.read()


def test_a_frame_that_does_not_start_with_FRAME():
    r = y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 F25:1\nFRAMES" + bytes(24)))
    with pytest.raises(Y4MError, match="frame 0"):
        r.read()


def test_writer_to_reader_round_trip():
    frames = payload(5, 12, 8, 4)
    f = io.BytesIO()
    w = y4m.Y4MWriter(f, 12, 8, (30000, 1001), aspect=(1, 1), colorspace="420paldv", tags=("XCOLORRANGE=LIMITED", "XFOO=bar"))
    for fr in frames:
        w.write(fr)
    assert f.getvalue().startswith(b"YUV4MPEG2 W12 H8 F30000:1001 Ip A1:1 C420paldv XCOLORRANGE=LIMITED XFOO=bar\nFRAME\n")
    r = y4m.Y4MReader(io.BytesIO(f.getvalue()))
    assert (r.width, r.height, tuple(r.fps), tuple(r.aspect), r.colorspace) == (12, 8, (30000, 1001), (1, 1), "420paldv")
    assert r.tags == ("XCOLORRANGE=LIMITED", "XFOO=bar")
    assert [g.tobytes() for g in r] == [fr.tobytes() for fr in frames]
    # a second generation written from the reader's fields is the same stream
    f2 = io.BytesIO()
    w2 = y4m.Y4MWriter(f2, r.width, r.height, r.fps, aspect=r.aspect, colorspace=r.colorspace, tags=r.tags, interlace=r.interlace)
    for fr in frames:
        w2.write(fr)
    assert f2.getvalue() == f.getvalue()


def test_writer_arguments():
    import fractions
    f = io.BytesIO()
    y4m.Y4MWriter(f, 4, 4, fractions.Fraction(30000, 1001), colorspace=None, interlace=None)
    assert f.getvalue() == b"YUV4MPEG2 W4 H4 F30000:1001\n"
    f = io.BytesIO()
    y4m.Y4MWriter(f, 4, 4, "24")
    assert f.getvalue() == b"YUV4MPEG2 W4 H4 F24:1 Ip C420jpeg\n"
    with pytest.raises(ValueError, match="422"):
        y4m.Y4MWriter(io.BytesIO(), 4, 4, 25, colorspace="422")
    with pytest.raises(ValueError, match="5"):
        y4m.Y4MWriter(io.BytesIO(), 5, 4, 25)
    with pytest.raises(ValueError, match="bytes"):
        y4m.Y4MWriter(io.BytesIO(), 4, 4, 25).write(np.zeros((6, 6), np.uint8))


def test_raw_nv12_round_trip():
    frames = payload(6, 8, 6, 3)
    f = io.BytesIO()
    w = y4m.RawNV12Writer(f, 8, 6)
    for fr in frames:
        w.write(fr)
    assert f.getvalue() == frames.tobytes() and w.layout == "nv12"
    r = y4m.RawNV12Reader(io.BytesIO(f.getvalue()), 8, 6)
    assert r.layout == "nv12" and r.frame_shape == (9, 8)
    assert [g.tobytes() for g in r] == [fr.tobytes() for fr in frames]
    with pytest.raises(Y4MError, match="7"):
        y4m.RawNV12Reader(io.BytesIO(), 7, 6)


class Trickle(object):
    """A file object that hands out 1 to 7 bytes per call, whatever is asked for."""

    def __init__(self, data, seed, with_readinto):
        self.f, self.rng = io.BytesIO(data), np.random.default_rng(seed)
        if with_readinto:
            self.readinto = self._readinto

    def read(self, n=-1):
        k = int(self.rng.integers(1, 8))
        return self.f.read(k if n < 0 else min(n, k))

    def _readinto(self, buf):
        chunk = self.read(len(buf))
        buf[:len(chunk)] = chunk
        return len(chunk)


@pytest.mark.parametrize("with_readinto", [False, True])
def test_short_reads_from_a_wrapper(with_readinto):
    frames = payload(7, 8, 6, 3)
    data = stream(FULL_HEADER, frames, b"FRAME Xp=1\n")
    r = y4m.Y4MReader(Trickle(data, 1, with_readinto))
    assert r.tags == ("XYSCSS=420MPEG2", "XCOLORRANGE=FULL")
    assert [g.tobytes() for g in r] == [f.tobytes() for f in frames]
    raw = y4m.RawNV12Reader(Trickle(frames.tobytes(), 2, with_readinto), 8, 6)
    assert [g.tobytes() for g in raw] == [f.tobytes() for f in frames]


def test_short_reads_from_a_real_pipe():
    frames = payload(8, 8, 6, 3)
    data = stream(FULL_HEADER, frames)
    rd, wr = os.pipe()

    def feed():
        rng = np.random.default_rng(3)
        i = 0
        while i < len(data):
            k = int(rng.integers(1, 8))
            os.write(wr, data[i:i + k])
            i += k
        os.close(wr)
    t = threading.Thread(target=feed)
    t.start()
    try:
        with os.fdopen(rd, "rb", buffering=0) as f:       # unbuffered: every read is the pipe's own short read
            r = y4m.Y4MReader(f)
            into = np.empty((3,) + r.frame_shape, np.uint8)
            assert all(r.readinto(into[k]) for k in range(3)) and not r.readinto(np.empty(r.frame_shape, np.uint8))
    finally:
        t.join(30)
    assert not t.is_alive()
    assert into.tobytes() == frames.tobytes()


def test_readinto_checks_the_buffer():
    r = y4m.Y4MReader(io.BytesIO(stream(b"YUV4MPEG2 W8 H6 F25:1\n", payload(9, 8, 6, 1))))
    with pytest.raises(ValueError, match="bytes"):
        r.readinto(np.empty((9, 9), np.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        r.readinto(np.empty((9, 16), np.uint8)[:, ::2])


# ---- the repack

def nv12_of_i420(a):
    """The index formula: NV12[H + i, 2 j] = U[i, j] and NV12[H + i, 2 j + 1] = V[i, j], with U and V the H/2 x W/2 planes
    that follow Y in the I420 bytes."""
    R, W = a.shape[-2:]
    H = 2 * R // 3
    flat = a.reshape(a.shape[:-2] + (R * W,))
    out = np.empty_like(flat)
    out[..., :H * W] = flat[..., :H * W]
    q = H * W // 4
    for i in range(H // 2):
        for j in range(W // 2):
            out[..., H * W + i * W + 2 * j] = flat[..., H * W + i * (W // 2) + j]
            out[..., H * W + i * W + 2 * j + 1] = flat[..., H * W + q + i * (W // 2) + j]
    return out.reshape(a.shape)


@pytest.mark.parametrize("W,H", [(8, 6), (4, 4), (12, 10), (6, 8)])   # H / 2 odd: a chroma plane ends inside a row
def test_repack_is_the_index_formula_and_its_own_inverse(W, H):
    import torch
    a = payload(10, W, H, 3)
    want = nv12_of_i420(a)
    t = torch.from_numpy(a)
    got = y4m.i420_to_nv12(t)
    assert got.dtype == torch.uint8 and got.shape == t.shape and np.array_equal(got.numpy(), want)
    assert np.array_equal(y4m.i420_to_nv12(t[1]).numpy(), want[1])                     # single-frame form
    assert np.array_equal(y4m.nv12_to_i420(got).numpy(), a)
    assert np.array_equal(y4m.nv12_to_i420(got[2]).numpy(), a[2])
    assert np.array_equal(y4m.i420_to_nv12(y4m.nv12_to_i420(t)).numpy(), a)            # inverse the other way round
    # the U and V of NV12 as planes
    uv = want[:, H:].reshape(3, H // 2, W // 2, 2)
    assert np.array_equal(uv[..., 0].reshape(3, -1), a.reshape(3, -1)[:, H * W:H * W + H * W // 4])


def test_repack_fills_out_in_place():
    import torch
    a = payload(11, 8, 6, 2)
    t = torch.from_numpy(a)
    out = torch.zeros_like(t)
    p = out.data_ptr()
    assert y4m.i420_to_nv12(t, out=out) is out and out.data_ptr() == p and np.array_equal(out.numpy(), nv12_of_i420(a))
    back = torch.zeros((4, 9, 8), dtype=torch.uint8)
    y4m.nv12_to_i420(out, out=back[1:3])                                               # a slice of a larger buffer
    assert np.array_equal(back[1:3].numpy(), a) and not back[0].any() and not back[3].any()
    single = torch.zeros((9, 8), dtype=torch.uint8)
    y4m.i420_to_nv12(t[0], out=single)
    assert np.array_equal(single.numpy(), nv12_of_i420(a[0]))
    with pytest.raises(ValueError, match="out"):
        y4m.i420_to_nv12(t, out=torch.zeros((2, 9, 10), dtype=torch.uint8))
    with pytest.raises(ValueError, match="not be src"):
        y4m.i420_to_nv12(t, out=t)
    with pytest.raises(ValueError, match="even"):
        y4m.i420_to_nv12(torch.zeros((9, 7), dtype=torch.uint8))


def test_default_yuv_matrix():
    assert y4m.default_yuv_matrix(719) == "bt601"
    assert y4m.default_yuv_matrix(720) == "bt709"
    assert y4m.default_yuv_matrix(2160) == "bt709"
