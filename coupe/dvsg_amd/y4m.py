"""Uncompressed video over pipes: YUV4MPEG2 (Y4M) and header-less NV12 readers and writers, and the planar <-> semi-planar
chroma repack between them.  No codec: a decoder and an encoder sit at either end of a pipe and speak these two formats
(`ffmpeg -f yuv4mpegpipe -pix_fmt yuv420p`, `ffmpeg -f rawvideo -pix_fmt nv12`).

A Y4M stream is one header line

    YUV4MPEG2 W<width> H<height> F<num>:<den> [I<p|?>] [A<num>:<den>] [C<chroma>] [X<anything> ...]\\n

followed by frames, each `FRAME[ params]\\n` and W H 3 / 2 bytes: H rows of Y, then the U plane and the V plane, each
H/2 x W/2 (I420).  `Y4MReader` hands a frame over as one uint8 array [3 H / 2, W] holding those bytes as they lie in the
stream; `OnlineStabilizer(frame_format="nv12")` wants the two chroma planes interleaved, which is `i420_to_nv12` (on the
device, in the pipeline).  `RawNV12Reader` yields NV12 [3 H / 2, W] directly, and nothing is repacked.

Chroma siting and range tags are carried through unchanged and interpreted nowhere: `C420jpeg`, `C420mpeg2` and `C420paldv`
differ in where the chroma samples sit, `XCOLORRANGE=FULL` says the bytes span [0, 255] instead of [16, 235].  The render
warps the Y plane and the UV plane directly (`dvsg_tps_render_nv12`), so an output pixel keeps the range and the siting of
the input, and a writer that repeats the input's tags describes the output correctly.  The YUV matrix (`yuv_matrix`, limited
range) only decides what the CNN sees at the model's size; Y4M carries no matrix, so `default_yuv_matrix` picks one by height
as players do.  Full-range footage therefore reaches the CNN through a limited-range matrix (slightly more contrast, clipped
at both ends); its effect on F_t has not been measured.

Readers and writers share one small interface, which `pipe.stabilize_pipes` relies on: `width`, `height`, `layout` ("i420"
or "nv12"), `frame_shape` ([3 H / 2, W]), `frame_bytes`; a reader has `readinto(buf) -> bool` (False at a clean end of the
stream) and iterates over fresh arrays; a writer has `write(frame)` and `flush()`.

Ten bits.  `Y4MReader(f, depths=(8, 10))` also takes `C420p10` (`ffmpeg -pix_fmt yuv420p10le -strict -1 -f yuv4mpegpipe`): the
same three planes with 2 bytes per sample, little-endian, the value in the LOW 10 bits; `layout` is then "i420p10" and a frame
is the stream's bytes, uint8 [3 H / 2, 2 W] (3 W H bytes).  `Y4MWriter(colorspace="420p10")` writes it.  `RawP010Reader` and
`RawP010Writer` are header-less P010 (`-f rawvideo -pix_fmt p010le`, `layout` "p010"): Y and interleaved U V as 16-bit
little-endian words with the value in the HIGH 10 bits -- what `OnlineStabilizer(frame_format="p010")` takes.
`i420p10_to_p010` and `p010_to_i420p10` repack between the two on the device.  The default `depths=(8,)` refuses `C420p10`.

4:2:2.  `Y4MReader(f, chromas=("420", "422"))` also takes `C422` (`ffmpeg -pix_fmt yuv422p -f yuv4mpegpipe`) and, with 10
among `depths`, `C422p10` (`-pix_fmt yuv422p10le -strict -1`): H rows of Y, then the U plane and the V plane of H x W / 2
each, so a frame is uint8 [2 H, W] ([2 H, 2 W] at ten bits, the value in the LOW 10 bits); `layout` is "i422" / "i422p10".
`Y4MWriter(colorspace="422" | "422p10", chromas=("420", "422"))` writes them.  `RawNV16Reader` / `RawNV16Writer` and
`RawP210Reader` / `RawP210Writer` are header-less NV16 and P210 (`-f rawvideo -pix_fmt nv16`, `p210le`): Y and H rows of
interleaved U V, what `OnlineStabilizer(frame_format="nv16" | "p210")` takes.  `i422_to_nv16`, `nv16_to_i422`,
`i422p10_to_p210` and `p210_to_i422p10` repack on the device.  The default `chromas=("420",)` refuses 4:2:2 as before; H and W
are even and at least 4 here too.  `LAYOUT_CHROMA` names every layout's chroma sampling beside `LAYOUT_BITS`.
"""
import numpy as np

MAGIC = b"YUV4MPEG2"
FRAME_MAGIC = b"FRAME"
CHROMA_420 = ("420", "420jpeg", "420mpeg2", "420paldv")   # 8-bit 4:2:0; they differ in chroma siting only
CHROMA_420_P10 = ("420p10",)                               # 10-bit 4:2:0, 2 bytes per sample
CHROMA_422 = ("422",)                                      # 8-bit 4:2:2: chroma planes of H x W / 2
CHROMA_422_P10 = ("422p10",)                               # 10-bit 4:2:2, 2 bytes per sample
# the layouts of this module, their bit depth and their chroma sampling
LAYOUT_BITS = {"i420": 8, "nv12": 8, "i420p10": 10, "p010": 10, "i422": 8, "nv16": 8, "i422p10": 10, "p210": 10}
LAYOUT_CHROMA = {"i420": "420", "nv12": "420", "i420p10": "420", "p010": "420",
                 "i422": "422", "nv16": "422", "i422p10": "422", "p210": "422"}
MAX_HEADER = 4096                                          # bytes of one header line, the newline included


class Y4MError(ValueError):
    """A stream that is not the Y4M / raw NV12 this module reads: a malformed or unsupported header, or a truncated frame."""


def _read_exact(f, view):
    """Fill the writable byte view from `f`, across short reads; returns the bytes received (less than asked for at the end
    of the stream only)."""
    n, got = len(view), 0
    readinto = getattr(f, "readinto", None)
    while got < n:
        if readinto is not None:
            k = readinto(view[got:])
        else:
            chunk = f.read(n - got)
            k = None if chunk is None else len(chunk)
            if k:
                view[got:got + k] = chunk
        if k is None:
            raise Y4MError("the stream is in non-blocking mode and has no data: give the reader a blocking file object")
        if k == 0:
            break
        got += k
    return got


def _read_line(f, first=b""):
    """The bytes up to and without the next newline, read one at a time (a pipe cannot be given anything back); None at the
    end of the stream before any byte."""
    line = bytearray(first)
    one = bytearray(1)
    while True:
        if _read_exact(f, memoryview(one)) == 0:
            if not line:
                return None
            raise Y4MError("the stream ends inside a header line: %r" % bytes(line[:40]))
        if one == b"\n":
            return bytes(line)
        line += one
        if len(line) >= MAX_HEADER:
            raise Y4MError("a header line of more than %d bytes: %r ..." % (MAX_HEADER, bytes(line[:40])))


def _ratio(tag):
    """'F30000:1001' -> (30000, 1001)"""
    try:
        num, den = tag[1:].split(":")
        num, den = int(num), int(den)
    except ValueError:
        raise Y4MError("tag %s: expected %s<num>:<den>" % (tag, tag[:1])) from None
    if num < 0 or den < 0:
        raise Y4MError("tag %s: negative ratio" % tag)
    return num, den


def _as_ratio(value, what):
    """A Fraction, (num, den), an int or 'N/D' / 'N:D' / 'N' -> (num, den)"""
    if isinstance(value, str):
        parts = value.replace(":", "/").split("/")
        try:
            value = (int(parts[0]), int(parts[1]) if len(parts) > 1 else 1)
            if len(parts) > 2:
                raise ValueError
        except (ValueError, IndexError):
            raise ValueError("%s must be N or N/D, got %r" % (what, value)) from None
    elif hasattr(value, "numerator"):
        value = (int(value.numerator), int(value.denominator))
    num, den = (int(v) for v in value)
    if num < 0 or den < 0:
        raise ValueError("%s must not be negative, got %d:%d" % (what, num, den))
    return num, den


def check_size(width, height, wtag="width", htag="height"):
    """OnlineStabilizer's NV12 rule: both even and at least 4."""
    for tag, v in ((wtag, width), (htag, height)):
        if v % 2 or v < 4:
            raise Y4MError("%s%d: 4:2:0 frames need an even width and height of at least 4" % (tag, v))


def _check_chromas(chromas):
    chromas = tuple(chromas)
    if not chromas or any(c not in ("420", "422") for c in chromas):
        raise ValueError("chromas must be a non-empty subset of ('420', '422'), got %r" % (chromas,))
    return chromas


def _frame_rows(height, chroma):
    """The rows of a frame of `height`: Y, then the chroma of H / 2 rows' worth (4:2:0) or H rows' worth (4:2:2)."""
    return 2 * height if chroma == "422" else 3 * height // 2


def _frame_view(buf, nbytes):
    """`buf` (anything with the buffer protocol, a pinned tensor's .numpy() included) as a flat byte view of nbytes."""
    view = memoryview(buf)
    if not view.contiguous:
        raise ValueError("a frame buffer must be contiguous")
    view = view.cast("B") if view.ndim != 1 or view.format != "B" else view
    if len(view) != nbytes:
        raise ValueError("a frame buffer of %d bytes, the frame has %d" % (len(view), nbytes))
    return view


class _Reader(object):
    layout = None

    def _init_frames(self, fileobj, width, height, sample_bytes=1, chroma="420"):
        self.fileobj, self.width, self.height = fileobj, int(width), int(height)
        self.frame_shape = (_frame_rows(self.height, chroma), sample_bytes * self.width)
        self.frame_bytes = self.frame_shape[0] * self.frame_shape[1]
        self.frames_read = 0

    def _payload(self, view):
        got = _read_exact(self.fileobj, view)
        if got != len(view):
            raise Y4MError("frame %d is truncated: %d of %d bytes received" % (self.frames_read, got, len(view)))

    def read(self):
        """The next frame as a fresh uint8 array of `frame_shape`, or None at the end of the stream."""
        frame = np.empty(self.frame_shape, dtype=np.uint8)
        return frame if self.readinto(frame) else None

    def __iter__(self):
        return self

    def __next__(self):
        frame = self.read()
        if frame is None:
            raise StopIteration
        return frame


class Y4MReader(_Reader):
    """Y4M from any binary file object, a pipe that returns short reads included.  The header is parsed on construction:
    `width`, `height`, `fps` and `aspect` ((num, den) as written, None without the tag), `interlace` ("p", "?" or None),
    `colorspace` (the C tag's value, None without one: 4:2:0 by default) and `tags`, every other tag verbatim and in order
    (the X tags, `XCOLORRANGE=FULL` among them).  Frames are I420, [3 H / 2, W] uint8: H rows of Y, then the U plane and the
    V plane as they lie in the stream.  `readinto(buf)` fills a caller's buffer of `frame_bytes` (pinned memory, say) without
    a copy.

    Accepted: C420, C420jpeg, C420mpeg2, C420paldv or no C tag; Ip, I? or no I tag.  Everything else -- another chroma
    format or bit depth, interlaced material, an odd or tiny or missing W / H, a wrong magic -- raises Y4MError naming the
    tag, before any frame is read.  A stream that ends inside a frame raises Y4MError with the frame's index and the bytes
    received; one that ends after the header yields no frames.

    depths: the bit depths the caller is ready for, a subset of (8, 10).  With 10 among them C420p10 is accepted as well:
    `layout` is "i420p10", `colorspace` "420p10", and a frame is uint8 [3 H / 2, 2 W], every sample 2 bytes little-endian
    with its value in the low 10 bits.  The default (8,) refuses it like any other format.

    chromas: the chroma samplings the caller is ready for, a subset of ("420", "422").  With "422" among them C422 (and, with
    10 among depths, C422p10) is accepted as well: `layout` is "i422" / "i422p10" and a frame is uint8 [2 H, W] / [2 H, 2 W],
    H rows of Y, then the U plane and the V plane of H x W / 2 each.  The default ("420",) refuses them like any other
    format."""
    layout = "i420"

    def __init__(self, fileobj, depths=(8,), chromas=("420",)):
        depths = tuple(depths)
        if not depths or any(d not in (8, 10) for d in depths):
            raise ValueError("depths must be a non-empty subset of (8, 10), got %r" % (depths,))
        chromas = _check_chromas(chromas)
        accepted = ()
        if "420" in chromas:
            accepted += (CHROMA_420 if 8 in depths else ()) + (CHROMA_420_P10 if 10 in depths else ())
        if "422" in chromas:
            accepted += (CHROMA_422 if 8 in depths else ()) + (CHROMA_422_P10 if 10 in depths else ())
        sampling = " and ".join("4:2:" + c[2] for c in sorted(chromas))
        sample_bytes = 1 if 8 in depths else 2   # without a C tag a stream is 8-bit 4:2:0
        line = _read_line(fileobj)
        if line is None:
            raise Y4MError("an empty stream: no YUV4MPEG2 header")
        tokens = [t for t in line.split(b" ") if t]
        if not tokens or tokens[0] != MAGIC:
            raise Y4MError("not a Y4M stream: it starts with %r, not YUV4MPEG2" % bytes(line[:16]))
        width = height = None
        self.fps = self.aspect = self.interlace = self.colorspace = None
        tags = []
        for tok in tokens[1:]:
            tag = tok.decode("latin-1")
            key = tag[0]
            try:
                if key == "W":
                    width = int(tag[1:])
                elif key == "H":
                    height = int(tag[1:])
            except ValueError:
                raise Y4MError("tag %s: not a size" % tag) from None
            if key == "F":
                self.fps = _ratio(tag)
            elif key == "A":
                self.aspect = _ratio(tag)
            elif key == "I":
                if tag[1:] not in ("p", "?"):
                    raise Y4MError("tag %s: interlaced material is not supported (progressive Ip or I? only)" % tag)
                self.interlace = tag[1:]
            elif key == "C":
                if tag[1:] not in accepted:
                    raise Y4MError("tag %s: only %s %s is supported (%s)" % (tag, " and ".join("%d-bit" % d for d in sorted(depths)),
                                                                             sampling, ", ".join("C" + c for c in accepted)))
                self.colorspace = tag[1:]
                sample_bytes = 2 if tag[1:] in CHROMA_420_P10 + CHROMA_422_P10 else 1
            elif key not in "WH":
                tags.append(tag)
        if width is None or height is None:
            raise Y4MError("the Y4M header has no %s tag: %r" % ("W" if width is None else "H", line[:80]))
        check_size(width, height, "W", "H")
        if self.colorspace is None and 8 not in depths:
            raise Y4MError("the Y4M header has no C tag, which means 8-bit 4:2:0, and depths=%r does not take it" % (depths,))
        if self.colorspace is None and "420" not in chromas:
            raise Y4MError("the Y4M header has no C tag, which means 8-bit 4:2:0, and chromas=%r does not take it" % (chromas,))
        self.tags = tuple(tags)
        chroma = "422" if self.colorspace in CHROMA_422 + CHROMA_422_P10 else "420"
        self.layout = ("i422" if chroma == "422" else "i420") + ("p10" if sample_bytes == 2 else "")
        self._init_frames(fileobj, width, height, sample_bytes, chroma)

    def readinto(self, buf):
        view = _frame_view(buf, self.frame_bytes)
        head = bytearray(len(FRAME_MAGIC) + 1)
        got = _read_exact(self.fileobj, memoryview(head))
        if got == 0:
            return False
        if got < len(head):
            raise Y4MError("frame %d is truncated: the stream ends inside its FRAME header (%d bytes received)"
                           % (self.frames_read, got))
        if head[:-1] != FRAME_MAGIC or head[-1:] not in (b"\n", b" "):
            raise Y4MError("frame %d does not start with FRAME: %r" % (self.frames_read, bytes(head)))
        if head[-1:] == b" " and _read_line(self.fileobj, b" ") is None:   # frame parameters: accepted and ignored
            raise Y4MError("frame %d is truncated: the stream ends inside its FRAME header" % self.frames_read)
        self._payload(view)
        self.frames_read += 1
        return True


class RawNV12Reader(_Reader):
    """Header-less NV12 (`-f rawvideo -pix_fmt nv12`): frames of W H 3 / 2 bytes, [3 H / 2, W] uint8 with H rows of Y and H / 2
    rows of interleaved U V.  The size comes from the caller; the interface is Y4MReader's."""
    layout = "nv12"
    fps = aspect = interlace = colorspace = None
    tags = ()

    def __init__(self, fileobj, width, height):
        check_size(int(width), int(height))
        self._init_frames(fileobj, width, height)

    def readinto(self, buf):
        view = _frame_view(buf, self.frame_bytes)
        got = _read_exact(self.fileobj, view)
        if got == 0:
            return False
        if got != self.frame_bytes:
            raise Y4MError("frame %d is truncated: %d of %d bytes received" % (self.frames_read, got, self.frame_bytes))
        self.frames_read += 1
        return True


class RawP010Reader(RawNV12Reader):
    """Header-less P010 (`-f rawvideo -pix_fmt p010le`): frames of 3 W H bytes, uint8 [3 H / 2, 2 W] -- H rows of Y and H / 2
    rows of interleaved U V, every sample a 16-bit little-endian word with its value in the high 10 bits.  RawNV12Reader's
    interface."""
    layout = "p010"

    def __init__(self, fileobj, width, height):
        check_size(int(width), int(height))
        self._init_frames(fileobj, width, height, 2)


class RawNV16Reader(RawNV12Reader):
    """Header-less NV16 (`-f rawvideo -pix_fmt nv16`): frames of 2 W H bytes, [2 H, W] uint8 with H rows of Y and H rows of
    interleaved U V.  RawNV12Reader's interface."""
    layout = "nv16"

    def __init__(self, fileobj, width, height):
        check_size(int(width), int(height))
        self._init_frames(fileobj, width, height, 1, "422")


class RawP210Reader(RawNV12Reader):
    """Header-less P210 (`-f rawvideo -pix_fmt p210le`): frames of 4 W H bytes, uint8 [2 H, 2 W] -- H rows of Y and H rows of
    interleaved U V, every sample a 16-bit little-endian word with its value in the high 10 bits.  RawNV12Reader's
    interface."""
    layout = "p210"

    def __init__(self, fileobj, width, height):
        check_size(int(width), int(height))
        self._init_frames(fileobj, width, height, 2, "422")


class _Writer(object):
    layout = None

    def _init_frames(self, fileobj, width, height, sample_bytes=1, chroma="420"):
        self.fileobj, self.width, self.height = fileobj, int(width), int(height)
        check_size(self.width, self.height)
        self.frame_shape = (_frame_rows(self.height, chroma), sample_bytes * self.width)
        self.frame_bytes = self.frame_shape[0] * self.frame_shape[1]
        self.frames_written = 0

    def _write_all(self, data):
        view = memoryview(data)
        while len(view):           # a raw file object may take less than it is given
            k = self.fileobj.write(view)
            if k is None:
                k = len(view)
            view = view[k:]

    def flush(self):
        flush = getattr(self.fileobj, "flush", None)
        if flush is not None:
            flush()


class Y4MWriter(_Writer):
    """Writes the stream header once, then `FRAME\\n` and the I420 bytes per `write(frame)`.  fps and aspect are a
    Fraction, (num, den), an int or "N/D"; aspect, interlace and colorspace of None leave their tag out; `tags` are appended
    verbatim (a reader's `tags`, to carry XCOLORRANGE and the like through).  colorspace="420p10": 10-bit frames, uint8
    [3 H / 2, 2 W] as Y4MReader hands them over; `layout` is then "i420p10".  chromas: with "422" among them
    colorspace="422" and "422p10" are written too (frames [2 H, W] / [2 H, 2 W], `layout` "i422" / "i422p10"); the default
    ("420",) refuses them."""
    layout = "i420"

    def __init__(self, fileobj, width, height, fps, aspect=None, colorspace="420jpeg", tags=(), interlace="p", chromas=("420",)):
        chromas = _check_chromas(chromas)
        written = (CHROMA_420 + CHROMA_420_P10 if "420" in chromas else ()) + (CHROMA_422 + CHROMA_422_P10 if "422" in chromas else ())
        if colorspace is None and "420" not in chromas:
            raise Y4MError("colorspace None means 8-bit 4:2:0, and chromas=%r does not write it" % (chromas,))
        if colorspace is not None and colorspace not in written:
            raise Y4MError("colorspace %r: only 8-bit and 10-bit %s is written (%s)"
                           % (colorspace, " and ".join("4:2:" + c[2] for c in sorted(chromas)), ", ".join(written)))
        p10, chroma = colorspace in CHROMA_420_P10 + CHROMA_422_P10, "422" if colorspace in CHROMA_422 + CHROMA_422_P10 else "420"
        self.layout = ("i422" if chroma == "422" else "i420") + ("p10" if p10 else "")
        self._init_frames(fileobj, width, height, 2 if p10 else 1, chroma)
        self.fps = _as_ratio(fps, "fps")
        self.aspect = None if aspect is None else _as_ratio(aspect, "aspect")
        if interlace not in (None, "p", "?"):
            raise Y4MError("interlace %r: progressive only ('p', '?' or None)" % (interlace,))
        self.colorspace, self.interlace, self.tags = colorspace, interlace, tuple(tags)
        for t in self.tags:
            if not t or any(c in t for c in " \n"):
                raise Y4MError("tag %r: a tag is one word" % (t,))
        head = ["YUV4MPEG2", "W%d" % self.width, "H%d" % self.height, "F%d:%d" % self.fps]
        if interlace is not None:
            head.append("I" + interlace)
        if self.aspect is not None:
            head.append("A%d:%d" % self.aspect)
        if colorspace is not None:
            head.append("C" + colorspace)
        self._write_all((" ".join(head + list(self.tags)) + "\n").encode("latin-1"))

    def write(self, frame):
        view = _frame_view(frame, self.frame_bytes)
        self._write_all(b"FRAME\n")
        self._write_all(view)
        self.frames_written += 1


class RawNV12Writer(_Writer):
    """Header-less NV12: `write(frame)` writes the W H 3 / 2 bytes of an NV12 frame [3 H / 2, W]."""
    layout = "nv12"

    def __init__(self, fileobj, width, height):
        self._init_frames(fileobj, width, height)

    def write(self, frame):
        self._write_all(_frame_view(frame, self.frame_bytes))
        self.frames_written += 1


class RawP010Writer(_Writer):
    """Header-less P010: `write(frame)` writes the 3 W H bytes of a P010 frame, uint8 [3 H / 2, 2 W]."""
    layout = "p010"

    def __init__(self, fileobj, width, height):
        self._init_frames(fileobj, width, height, 2)

    def write(self, frame):
        self._write_all(_frame_view(frame, self.frame_bytes))
        self.frames_written += 1


class RawNV16Writer(_Writer):
    """Header-less NV16: `write(frame)` writes the 2 W H bytes of an NV16 frame [2 H, W]."""
    layout = "nv16"

    def __init__(self, fileobj, width, height):
        self._init_frames(fileobj, width, height, 1, "422")

    def write(self, frame):
        self._write_all(_frame_view(frame, self.frame_bytes))
        self.frames_written += 1


class RawP210Writer(_Writer):
    """Header-less P210: `write(frame)` writes the 4 W H bytes of a P210 frame, uint8 [2 H, 2 W]."""
    layout = "p210"

    def __init__(self, fileobj, width, height):
        self._init_frames(fileobj, width, height, 2, "422")

    def write(self, frame):
        self._write_all(_frame_view(frame, self.frame_bytes))
        self.frames_written += 1


def _planes_422(t):
    """`_planes` for 4:2:2: a frame [2 H, W] or a batch [n, 2 H, W] as views (y [n, H W], chroma [n, H W], H, W)."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("a frame is [2 H, W] and a batch [n, 2 H, W], got %s" % (tuple(t.shape),))
    n, R, W = (int(v) for v in t.shape)
    H = R // 2
    if R % 2 or H % 2 or W % 2:
        raise ValueError("4:2:2 frames [2 H, W] need even H and W, got %s" % (tuple(t.shape),))
    if n > 0 and (t.stride(2) != 1 or t.stride(1) != W):
        raise ValueError("the rows of a frame must be contiguous (strides %s)" % (tuple(t.stride()),))
    flat = t.as_strided((n, R * W), (t.stride(0), 1), t.storage_offset())
    return flat[:, :H * W], flat[:, H * W:], H, W


def _planes(t):
    """A frame [3 H / 2, W] or a batch [n, 3 H / 2, W] as views: (y [n, H W], chroma [n, H W / 2], H, W)."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("a frame is [3 H / 2, W] and a batch [n, 3 H / 2, W], got %s" % (tuple(t.shape),))
    n, R, W = (int(v) for v in t.shape)
    H = 2 * R // 3
    if R % 3 or H % 2 or W % 2:
        raise ValueError("4:2:0 frames [3 H / 2, W] need even H and W, got %s" % (tuple(t.shape),))
    if n > 0 and (t.stride(2) != 1 or t.stride(1) != W):
        raise ValueError("the rows of a frame must be contiguous (strides %s)" % (tuple(t.stride()),))
    flat = t.as_strided((n, R * W), (t.stride(0), 1), t.storage_offset())
    return flat[:, :H * W], flat[:, H * W:], H, W


def _repack_out(src, out):
    import torch
    if out is None:
        out = torch.empty(src.shape, dtype=src.dtype, device=src.device)
    elif out.shape != src.shape or out.dtype != src.dtype or out.device != src.device:
        raise ValueError("out must have the shape, dtype and device of src: %s %s %s against %s %s %s"
                         % (tuple(out.shape), out.dtype, out.device, tuple(src.shape), src.dtype, src.device))
    if out.data_ptr() == src.data_ptr() and src.numel():
        raise ValueError("out must not be src: the repack is not done in place")
    return out


def _repack(src, out, to_nv12, given=None, planes=_planes):
    """The two strided copies; given: the caller's own `out` (already checked) in the place of the check here.  planes:
    `_planes`, or `_planes_422` for frames whose chroma planes have H rows."""
    out = _repack_out(src, out) if given is None else out
    sy, sc, H, W = planes(src)
    oy, oc, _, _ = planes(out)
    n, q = int(sy.shape[0]), int(sc.shape[1]) // 2   # the samples of one chroma plane
    oy.copy_(sy)
    if to_nv12:   # U plane | V plane -> U0 V0 U1 V1 ...
        oc.view(n, q, 2).copy_(sc.view(n, 2, q).transpose(1, 2))
    else:
        oc.view(n, 2, q).copy_(sc.view(n, q, 2).transpose(1, 2))
    return out


def i420_to_nv12(src, out=None):
    """I420 (Y, the U plane, the V plane) -> NV12 (Y, interleaved U V) for a uint8 tensor [3 H / 2, W] or a batch
    [n, 3 H / 2, W] on any device: two strided copies on the current stream, no synchronise, and no allocation when `out`
    (same shape, not `src` itself) is given.  Returns out."""
    return _repack(src, out, True)


def nv12_to_i420(src, out=None):
    """The inverse of `i420_to_nv12`, with the same contract."""
    return _repack(src, out, False)


def _words(t, what, layout=("4:2:0", "3 H / 2")):
    """A 10-bit frame or batch, uint8 [..., 3 H / 2, 2 W], as int16 words [..., 3 H / 2, W] over the same memory (int16: the
    16-bit type every torch has; the bits are what matters).  layout: the names its message uses."""
    import torch
    if t.dtype != torch.uint8 or t.dim() not in (2, 3) or int(t.shape[-1]) % 4:
        raise ValueError("%s: a 10-bit %s frame is uint8 [%s, 2 W] with even W (a batch [n, %s, 2 W]), got %s %s"
                         % (what, layout[0], layout[1], layout[1], t.dtype, tuple(t.shape)))
    if t.numel() and (t.stride(-1) != 1 or any(s % 2 for s in t.stride()[:-1]) or t.data_ptr() % 2):
        raise ValueError("%s: the rows of a frame must be contiguous and 2-byte aligned (strides %s)" % (what, tuple(t.stride())))
    return t.view(torch.int16)


def i420p10_to_p010(src, out=None):
    """C420p10 frames as Y4MReader(depths=(8, 10)) yields them (uint8 [3 H / 2, 2 W] or a batch: Y, the U plane, the V plane,
    16-bit little-endian, value in the low 10 bits) -> P010 (Y, interleaved U V, value in the HIGH 10 bits):
    word_out = (word_in << 6) mod 2^16, so the upper 6 bits of a C420p10 sample are dropped.  Two strided copies and one
    in-place shift on the current stream, no synchronise, no allocation when `out` is given.  Returns out."""
    out = _repack_out(src, out)
    o16 = _words(out, "out")
    _repack(_words(src, "src"), o16, True, given=out)
    o16.bitwise_left_shift_(6)   # int16: the bits of a word with the top bit set survive (no arithmetic is done on them)
    return out


def p010_to_i420p10(src, out=None):
    """The inverse for P010 words: word_out = word_in >> 6 as an UNSIGNED shift (int16's >> is arithmetic, so the sign
    copies are masked off), then U and V split into planes.  The low 6 bits of a P010 word are dropped."""
    out = _repack_out(src, out)
    o16 = _words(out, "out")
    _repack(_words(src, "src"), o16, False, given=out)
    o16.bitwise_right_shift_(6).bitwise_and_(0x03FF)
    return out


def i422_to_nv16(src, out=None):
    """I422 (Y, the U plane, the V plane of H x W / 2 each) -> NV16 (Y, H rows of interleaved U V) for a uint8 tensor
    [2 H, W] or a batch [n, 2 H, W]: `i420_to_nv12`'s contract at the 4:2:2 plane size."""
    return _repack(src, out, True, planes=_planes_422)


def nv16_to_i422(src, out=None):
    """The inverse of `i422_to_nv16`, with the same contract."""
    return _repack(src, out, False, planes=_planes_422)


_L422 = ("4:2:2", "2 H")


def i422p10_to_p210(src, out=None):
    """C422p10 frames as Y4MReader(depths=(8, 10), chromas=("420", "422")) yields them (uint8 [2 H, 2 W] or a batch, value in
    the low 10 bits) -> P210 (Y, interleaved U V, value in the HIGH 10 bits): `i420p10_to_p010`'s contract at the 4:2:2
    plane size."""
    out = _repack_out(src, out)
    o16 = _words(out, "out", _L422)
    _repack(_words(src, "src", _L422), o16, True, given=out, planes=_planes_422)
    o16.bitwise_left_shift_(6)
    return out


def p210_to_i422p10(src, out=None):
    """The inverse for P210 words, as `p010_to_i420p10`: an unsigned shift by 6, then U and V split into planes."""
    out = _repack_out(src, out)
    o16 = _words(out, "out", _L422)
    _repack(_words(src, "src", _L422), o16, False, given=out, planes=_planes_422)
    o16.bitwise_right_shift_(6).bitwise_and_(0x03FF)
    return out


def default_yuv_matrix(height):
    """Y4M names no matrix: "bt709" from 720 rows up and "bt601" below, as players assume."""
    return "bt709" if int(height) >= 720 else "bt601"
