"""How shaky is a clip?  A no-reference figure from the pictures themselves: the global motion between consecutive luma planes
by block matching on the device (`dvsg_shake_measure_u8`, include/dvsg_amd.h "SHAKE"; tests/shake_ref.py restates the rule in
NumPy and the kernels equal it bit for bit), and from those vectors how fast the picture moves and how much that motion
changes from one frame to the next.  Measure the input and the output of a stabilisation and compare:

    python -m coupe.dvsg_amd.shake before.y4m after.y4m

    ffmpeg -i in.mp4 -f yuv4mpegpipe -pix_fmt yuv420p - | tee before.y4m \\
      | python -m coupe.dvsg_amd.pipe --ckpt DIR > after.y4m && python -m coupe.dvsg_amd.shake before.y4m after.y4m

`measure` gives a `Track` (one row [gx, gy, n_valid, ok] per pair of frames, sixteenths of a reduced pixel per frame),
`summary` the figures of one track, `compare` those of two and `jitter_ratio = jitter_b / jitter_a`.  The matcher is a GPU job
and there is no CPU fallback, as everywhere in this package.

The median sees translation only.  `measure_motion` (`dvsg_shake_motion_u8`, "SHAKE MOTION"; tests/shake_motion_ref.py) also
fits a similarity -- translation, roll and zoom -- to the blocks that agree with the median, and gives a `MotionTrack` of
exact integer sums; `motion_figures` makes roll, zoom and wobble (what the similarity leaves unexplained) of one pair,
`motion_summary` the figures of a clip and `compare_motion` those of two with `roll_jitter_ratio` and `wobble_ratio`:

    python -m coupe.dvsg_amd.shake --motion before.y4m after.y4m

Wobble is what `rigidity` and `shape_model` of the renders exist to prevent: measure it before and after to see what they buy.

What the figures are NOT:
  - Motion beyond the radius (radius x factor source pixels per frame) is lost, not measured: such pairs count as `lost`.
  - A zoomed or cropped output scales its motion by 1 / zoom, so compare like with like (crop both, or neither).
  - The black border of an uncropped output moves with the warp; the margin (an eighth of each side by default) exists to
    keep it out of the blocks.
  - A scene cut produces one meaningless row (usually a lost one).
  - No threshold for "steady" is offered, because none has been measured.
  - Roll, zoom and wobble are a similarity's: perspective and rolling shutter count as wobble.  The matcher has a wobble
    floor of its own (motion inside a block and the parabola step: 0.07 - 0.16 reduced pixels on synthetic planes), and no
    threshold for "wobbly" is offered either.
"""
import argparse
import collections
import ctypes
import fractions
import json
import math
import sys

import numpy as np

from . import _lib

PROG = "coupe.dvsg_amd.shake"
CHUNK = 64          # frames per call of measure's default chunking
MAX_FRAMES = 4096   # per call of dvsg_shake_measure_u8

# vectors int64 [n - 1, 4]; factor; size (H, W) of the source planes; blocks int64 [n - 1, n_blk, 3] or None
Track = collections.namedtuple("Track", ["vectors", "factor", "size", "blocks"])
# rows int64 [n - 1, 13]; factor; size (H, W); grid (ny, nx) of the blocks; blocks int64 [n - 1, n_blk, 3] or None
MotionTrack = collections.namedtuple("MotionTrack", ["rows", "factor", "size", "grid", "blocks"])


def geometry(H, W, factor=None, radius=12, margin=0.125):
    """(factor, margin_y, margin_x) of `measure`: the default factor is max(1, ceil(W / 512)), the margins are
    max(radius, ceil(margin * h)) and max(radius, ceil(margin * w)) on the reduced plane."""
    f = max(1, -(-int(W) // 512)) if factor is None else int(factor)
    if f < 1:
        raise ValueError("factor must be at least 1, got %d" % f)
    h, w = int(H) // f, int(W) // f
    return f, max(int(radius), math.ceil(margin * h)), max(int(radius), math.ceil(margin * w))


def chunk_ranges(n, chunk):
    """[(first, last + 1), ...] of the calls for n frames: chunks of at most `chunk` frames that overlap by one frame, so
    every pair lies in exactly one of them."""
    if chunk < 2:
        raise ValueError("chunk must be at least 2 frames, got %d" % chunk)
    out, a = [], 0
    while a < n - 1:
        b = min(a + chunk, n)
        out.append((a, b))
        a = b - 1
    return out


def _device_planes(luma):
    """-> (tensor that keeps the memory alive, pointer, pitch, frame_stride, n, H, W) on the device"""
    import torch
    from ._tensor import device
    if isinstance(luma, tuple):
        t, pitch, frame_stride = luma
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3):
            raise ValueError("a (tensor, pitch, frame_stride) view needs a uint8 device tensor of shape [n, H, W]")
        n, H, W = t.shape
        pitch, frame_stride = int(pitch), int(frame_stride)
        have = t.untyped_storage().nbytes() - t.storage_offset()
        if pitch < W or frame_stride < (H - 1) * pitch + W or (n - 1) * frame_stride + (H - 1) * pitch + W > have:
            raise ValueError("pitch=%d, frame_stride=%d do not describe %d planes of %dx%d inside the tensor's %d bytes"
                             % (pitch, frame_stride, n, H, W, have))
        return t, t.data_ptr(), pitch, frame_stride, n, H, W
    dev = device()
    t = luma if isinstance(luma, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(luma))
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError("luma must be uint8 [n, H, W], got %s %s" % (t.dtype, tuple(t.shape)))
    if t.device.type != "cuda":
        t = t.to(dev)
    n, H, W = t.shape
    s0, s1, s2 = t.stride()
    if not (s2 == 1 and s1 >= W and (n == 1 or s0 >= (H - 1) * s1 + W)):   # anything but rows of bytes: one copy
        t = t.contiguous()
        s0, s1, s2 = t.stride()
    return t, t.data_ptr(), s1, s0, n, H, W


def _measure_chunks(luma, factor, radius, margin, texture, min_blocks, blocks, chunk, gate):
    """The chunked calls behind `measure` (gate None: dvsg_shake_measure_u8, int32 rows of 4) and `measure_motion`
    (dvsg_shake_motion_u8, int64 rows of 13) -> (rows int64, f, (H, W), (ny, nx), blocks int64 or None)"""
    import torch
    keep, base, pitch, frame_stride, n, H, W = _device_planes(luma)
    if n < 2:
        raise ValueError("a measurement needs at least 2 frames, got %d" % n)
    f, my, mx = geometry(H, W, factor, radius, margin)
    h, w = H // f, W // f
    grid = ((h - 2 * my) // 16, (w - 2 * mx) // 16)
    chunk = min(int(chunk), MAX_FRAMES)
    query = "dvsg_shake_workspace_bytes" if gate is None else "dvsg_shake_motion_workspace_bytes"
    rows, block_rows = [], []
    workspace = None
    for a, b in chunk_ranges(n, chunk):
        m = b - a
        need = ctypes.c_size_t()
        _lib.call(query, m, H, W, f, int(radius), my, mx, ctypes.byref(need))
        if workspace is None or workspace.numel() < need.value:
            workspace = torch.empty(need.value, dtype=torch.uint8, device=keep.device)
        v = np.empty((m - 1, 4), dtype=np.int32) if gate is None else np.empty((m - 1, 13), dtype=np.int64)
        blk = np.empty((m - 1, grid[0] * grid[1], 3), dtype=np.int32) if blocks else None
        head = (base + a * frame_stride, pitch, frame_stride, m, H, W, f, int(radius), my, mx, int(texture), int(min_blocks))
        tail = (v.ctypes.data, None if blk is None else blk.ctypes.data, workspace.data_ptr(), workspace.numel())
        if gate is None:
            _lib.call("dvsg_shake_measure_u8", *(head + tail))
        else:
            _lib.call("dvsg_shake_motion_u8", *(head + (int(gate),) + tail))
        rows.append(v)
        block_rows.append(blk)
    return (np.concatenate(rows).astype(np.int64), f, (H, W), grid,
            np.concatenate(block_rows).astype(np.int64) if blocks else None)


def measure(luma, factor=None, radius=12, margin=0.125, texture=256, min_blocks=8, blocks=False, chunk=CHUNK):
    """The global motion of every pair of consecutive planes.  luma: uint8 [n, H, W] as a device tensor (rows of bytes at any
    pitch are read where they lie, `luma_of`'s Y rows included) or a NumPy array (copied to the device), or a
    (tensor, pitch, frame_stride) view of a surface batch: a uint8 device tensor whose shape is [n, H, W] and whose rows lie
    at data_ptr + t * frame_stride + i * pitch inside its storage.

    factor: the reduction (None: max(1, ceil(W / 512))).  radius: the search radius in reduced pixels, 1 .. 16.  margin: the
    share of each side kept out of the blocks (`geometry`).  texture: the least SAD curvature of a valid block.  min_blocks:
    the valid blocks a pair needs to count.  blocks=True also returns every block's (vx, vy, valid).  Clips longer than
    `chunk` frames are fed in chunks that overlap by one frame, which changes no row.

    Returns Track(vectors int64 [n - 1, 4], factor, size (H, W), blocks int64 [n - 1, n_blk, 3] or None); a row is
    [gx, gy, n_valid, ok] in sixteenths of a reduced pixel per frame: the content of frame t came from (gy, gx) / 16 in
    frame t - 1.  Synchronous: the call waits for the device."""
    vectors, f, size, _, block_rows = _measure_chunks(luma, factor, radius, margin, texture, min_blocks, blocks, chunk, None)
    return Track(vectors, f, size, block_rows)


def measure_motion(luma, factor=None, radius=12, margin=0.125, texture=256, min_blocks=8, gate=64, blocks=False, chunk=CHUNK):
    """`measure` with the sums of a similarity fit (translation + roll + zoom) over the blocks that agree with the median
    (`dvsg_shake_motion_u8`, include/dvsg_amd.h "SHAKE MOTION").  The same inputs, options and chunking as `measure`.  gate, in
    sixteenths of a reduced pixel: how far a block's vector may lie from the pair's median, per axis, and still enter the
    fit; 64 keeps moving objects out and lets through what about 1.3 degrees of roll per frame spread over a 1080p picture.

    Returns MotionTrack(rows int64 [n - 1, 13], factor, size (H, W), grid (ny, nx), blocks int64 [n - 1, n_blk, 3] or None); a
    row is [gx, gy, n_valid, ok, n_in, Sx, Sy, Su, Sv, Sxx, Sxu, Sxv, Suu], and rows[:, :4] is what `measure` returns.
    `motion_figures` makes roll, zoom and wobble of one row, `motion_summary` the figures of a clip."""
    return MotionTrack(*_measure_chunks(luma, factor, radius, margin, texture, min_blocks, blocks, chunk, gate))


def luma_of(frames, frame_format):
    """The 8-bit luma planes [n, H, W] of a batch of frames (a torch tensor, or a NumPy array, which becomes a CPU tensor).
    "nv12" [n, 3 H / 2, W] / "nv16" [n, 2 H, W]: the Y rows, no copy.  "p010" / "p210", uint8 [n, rows, 2 W] (the words' bytes,
    low byte first) or uint16 [n, rows, W]: the high byte of each Y word, the same definition the ingest uses
    (online.OnlineStabilizer), a strided view.  "rgb" uint8 [n, H, W, 3]: (77 R + 150 G + 29 B + 128) >> 8, with integer
    torch operations."""
    import torch
    t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.asarray(frames))
    if frame_format == "rgb":
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError("rgb frames must be uint8 [n, H, W, 3], got %s %s" % (t.dtype, tuple(t.shape)))
        c = t.to(torch.int32)
        return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).to(torch.uint8)
    if frame_format not in ("nv12", "nv16", "p010", "p210"):
        raise ValueError("frame_format must be 'nv12', 'nv16', 'p010', 'p210' or 'rgb', got %r" % (frame_format,))
    if t.dim() != 3:
        raise ValueError("%s frames must be [n, rows, W], got %s" % (frame_format, tuple(t.shape)))
    rows = t.shape[1]
    if frame_format in ("nv12", "p010"):
        if rows % 3:
            raise ValueError("%s frames have 3 H / 2 rows, got %d" % (frame_format, rows))
        H = 2 * rows // 3
    else:
        if rows % 2:
            raise ValueError("%s frames have 2 H rows, got %d" % (frame_format, rows))
        H = rows // 2
    if frame_format in ("nv12", "nv16"):
        if t.dtype != torch.uint8:
            raise ValueError("%s frames must be uint8, got %s" % (frame_format, t.dtype))
        return t[:, :H, :]
    if t.dtype != torch.uint8:                      # 16-bit words: their bytes, low byte first
        if t.element_size() != 2:
            raise ValueError("%s frames must be uint8 [n, rows, 2 W] or 16-bit words [n, rows, W], got %s" % (frame_format, t.dtype))
        t = t.contiguous().view(torch.uint8)
    if t.shape[2] % 2:
        raise ValueError("%s frames as bytes have 2 W columns, got %d" % (frame_format, t.shape[2]))
    return t[:, :H, 1::2]


def summary(track):
    """The figures of one track, from exact integer sums, then one division and one square root each:
      frames, pairs, lost (the pairs that are not ok);
      speed_rms = (f / 16) sqrt(sum(gx^2 + gy^2) / n_ok) over the ok pairs, in source pixels per frame;
      jitter_rms: the same over the differences of consecutive rows that are both ok -- how much the motion changes from one
      frame to the next, which is what a viewer sees as shake;
      speed_pct, jitter_pct: both as a percentage of the frame width.
    A figure with nothing to average is None."""
    rows = [[int(v) for v in r] for r in track.vectors]
    f, width = track.factor, track.size[1]
    ok = [r for r in rows if r[3]]
    speed_sum = sum(r[0] * r[0] + r[1] * r[1] for r in ok)
    jitter_sum = jitter_n = 0
    for a, b in zip(rows[:-1], rows[1:]):
        if a[3] and b[3]:
            jitter_sum += (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
            jitter_n += 1
    speed = f / 16 * math.sqrt(speed_sum / len(ok)) if ok else None
    jitter = f / 16 * math.sqrt(jitter_sum / jitter_n) if jitter_n else None
    return dict(frames=len(rows) + 1, pairs=len(rows), lost=len(rows) - len(ok), speed_rms=speed, jitter_rms=jitter,
                speed_pct=None if speed is None else 100 * speed / width,
                jitter_pct=None if jitter is None else 100 * jitter / width)


def compare(a, b):
    """{"a": summary(a), "b": summary(b), "jitter_ratio": jitter_b / jitter_a} of two tracks (None where either jitter is
    missing or a's is 0): below 1, b is the steadier clip."""
    sa, sb = summary(a), summary(b)
    ja, jb = sa["jitter_rms"], sb["jitter_rms"]
    return dict(a=sa, b=sb, jitter_ratio=jb / ja if ja and jb is not None else None)


def _fit(row, min_blocks):
    """(N, Pn, Rn, Qn, rss as a Fraction) of a fit pair, None of any other: exact, from the row's integer sums"""
    gx, gy, n_valid, ok, N, Sx, Sy, Su, Sv, Sxx, Sxu, Sxv, Suu = (int(v) for v in row)
    Qn = N * Sxx - Sx * Sx - Sy * Sy
    if not ok or N < max(int(min_blocks), 3) or Qn <= 0:
        return None
    Pn = N * Sxu - Sx * Su - Sy * Sv
    Rn = N * Sxv - Sx * Sv + Sy * Su
    Vn = N * Suu - Su * Su - Sv * Sv
    return N, Pn, Rn, Qn, max(fractions.Fraction(Vn * Qn - Pn * Pn - Rn * Rn, N * Qn), fractions.Fraction(0))


def motion_figures(row, factor=1, min_blocks=8):
    """dict(fit, zoom, roll, wobble) of one row of a MotionTrack: the least-squares similarity over the inliers, from exact
    integer sums, then one division (and for the wobble one square root) each.
      fit: the pair is ok, has n_in >= max(min_blocks, 3) inliers and they do not lie on one point;
      zoom: the fractional size change per frame;  roll: radians per frame (small angles: exactly scale x sin), in the
      vectors' convention, cur[y][x] looks like prev[y + dy][x + dx];
      wobble: (factor / 16) sqrt(rss / n_in), the RMS distance of an inlier's vector from the fitted similarity, in source
      pixels (factor=1: in reduced pixels).
    The three are None for a pair that is not fit."""
    fit = _fit(row, min_blocks)
    if fit is None:
        return dict(fit=False, zoom=None, roll=None, wobble=None)
    N, Pn, Rn, Qn, rss = fit
    return dict(fit=True, zoom=float(fractions.Fraction(Pn, 128 * Qn)), roll=float(fractions.Fraction(Rn, 128 * Qn)),
                wobble=factor / 16 * math.sqrt(float(rss / N)))


def motion_summary(track, min_blocks=8):
    """The figures of one MotionTrack (min_blocks: the one it was measured with):
      frames, pairs, unfit (the pairs that are not fit, `motion_figures`);
      roll_rms_deg: the RMS of roll over the fit pairs, in degrees per frame;
      roll_jitter_deg: the RMS of the difference of roll between consecutive pairs that are both fit -- roll shake;
      zoom_jitter_pct: the same for zoom, in per cent -- breathing;
      wobble_rms = (f / 16) sqrt(sum rss / sum n_in) over the fit pairs, in source pixels: the motion a similarity does
      not explain.
    Each pair's roll, zoom and rss is one exact division; the sums over pairs are math.fsum's (exactly rounded, whatever
    the order).  A figure with nothing to average is None."""
    fits = [_fit(r, min_blocks) for r in track.rows]
    roll = [None if x is None else float(fractions.Fraction(x[2], 128 * x[3])) for x in fits]
    zoom = [None if x is None else float(fractions.Fraction(x[1], 128 * x[3])) for x in fits]
    have = [x for x in fits if x is not None]
    both = [k for k in range(1, len(fits)) if fits[k - 1] is not None and fits[k] is not None]
    rms = lambda values: math.sqrt(math.fsum(v * v for v in values) / len(values)) if values else None
    roll_rms, roll_jitter = rms([r for r in roll if r is not None]), rms([roll[k] - roll[k - 1] for k in both])
    zoom_jitter = rms([zoom[k] - zoom[k - 1] for k in both])
    wobble = track.factor / 16 * math.sqrt(math.fsum(float(x[4]) for x in have) / sum(x[0] for x in have)) if have else None
    return dict(frames=len(fits) + 1, pairs=len(fits), unfit=len(fits) - len(have),
                roll_rms_deg=None if roll_rms is None else math.degrees(roll_rms),
                roll_jitter_deg=None if roll_jitter is None else math.degrees(roll_jitter),
                zoom_jitter_pct=None if zoom_jitter is None else 100 * zoom_jitter, wobble_rms=wobble)


def compare_motion(a, b, min_blocks=8):
    """{"a": motion_summary(a), "b": motion_summary(b), "roll_jitter_ratio", "wobble_ratio"} of two MotionTracks, the ratios
    b over a (None where either side is missing or a's is 0): below 1, b rolls or wobbles less."""
    sa, sb = motion_summary(a, min_blocks), motion_summary(b, min_blocks)
    ratio = lambda key: sb[key] / sa[key] if sa[key] and sb[key] is not None else None
    return dict(a=sa, b=sb, roll_jitter_ratio=ratio("roll_jitter_deg"), wobble_ratio=ratio("wobble_rms"))


# ---- the command line ---------------------------------------------------------------------------------------------

class _UsageError(Exception):
    pass


def _parser():
    ap = argparse.ArgumentParser(prog="python -m " + PROG, description="Measure the frame-to-frame motion of one clip, or of two "
                                 "(before and after stabilisation) and their jitter ratio.  Only the Y plane is used.")
    ap.add_argument("clips", nargs="+", metavar="FILE", help="one clip, or two of the same frame size (A, then B)")
    ap.add_argument("--format", default="y4m", choices=["y4m", "nv12", "p010", "nv16", "p210"],
                    help="of the files (nv12, p010, nv16, p210: header-less, need --size; y4m: C420, C420p10, C422, C422p10)")
    ap.add_argument("--size", default=None, metavar="WxH", help="frame size of header-less files")
    ap.add_argument("--radius", type=int, default=12, help="search radius in reduced pixels, 1 .. 16")
    ap.add_argument("--factor", type=int, default=None, help="reduction (default: max(1, ceil(W / 512)))")
    ap.add_argument("--margin", type=float, default=0.125, help="share of each side kept out of the blocks")
    ap.add_argument("--texture", type=int, default=256, help="least SAD curvature of a valid block")
    ap.add_argument("--min-blocks", type=int, default=8, help="valid blocks a pair needs to count")
    ap.add_argument("--motion", action="store_true", help="also fit roll and zoom to the blocks: roll, roll jitter, zoom jitter "
                    "and wobble (what a similarity does not explain) of each clip")
    ap.add_argument("--gate", type=int, default=None, metavar="N", help="with --motion: how far a block may lie from the median "
                    "and enter the fit, in sixteenths of a reduced pixel (default: 64)")
    ap.add_argument("--json", action="store_true", help="print one JSON object")
    return ap


def _open(path, args):
    from . import y4m
    from .pipe import _RAW
    f = open(path, "rb")
    try:
        if args.format == "y4m":
            return f, y4m.Y4MReader(f, depths=(8, 10), chromas=("420", "422"))
        return f, _RAW[args.format][0](f, *args.size)
    except Exception:
        f.close()
        raise


def _luma_rows(frames, layout, H):
    """uint8 [n, H, W] of a chunk of frames as the readers hand them over (y4m.LAYOUT_BITS): the Y rows; of 10-bit samples
    the top 8 bits -- the high byte of a P010 / P210 word, bits 9 .. 2 of a planar (low-aligned) one."""
    y = frames[:, :H]
    if layout in ("p010", "p210"):
        return np.ascontiguousarray(y[:, :, 1::2])
    if layout in ("i420p10", "i422p10"):
        return ((y[:, :, 1::2] << 6) | (y[:, :, 0::2] >> 2)).astype(np.uint8)
    return y


def _measure_file(reader, args):
    """measure() over a file, CHUNK frames at a time with one frame of overlap, so a long clip needs no more memory.  With
    --motion it is measure_motion(): (Track, MotionTrack) from the same rows; without, (Track, None)."""
    kw = dict(factor=args.factor, radius=args.radius, margin=args.margin, texture=args.texture, min_blocks=args.min_blocks)
    if args.motion:
        kw["gate"] = 64 if args.gate is None else args.gate
    vectors, rows, grid, last, factor = [], [], None, None, None
    while True:
        frames = [] if last is None else [last]
        while len(frames) < CHUNK:
            frame = reader.read()
            if frame is None:
                break
            frames.append(frame)
        if len(frames) < 2:
            break
        planes = _luma_rows(np.stack(frames), reader.layout, reader.height)
        if args.motion:
            track = measure_motion(planes, **kw)
            rows.append(track.rows)
            vectors.append(track.rows[:, :4])
            grid = track.grid
        else:
            track = measure(planes, **kw)
            vectors.append(track.vectors)
        factor, last = track.factor, frames[-1]
        if len(frames) < CHUNK:
            break
    if not vectors:
        raise _UsageError("%d frame(s): a measurement needs at least 2" % reader.frames_read)
    size = (reader.height, reader.width)
    motion = MotionTrack(np.concatenate(rows), factor, size, grid, None) if args.motion else None
    return Track(np.concatenate(vectors), factor, size, None), motion


def _line(path, s, size):
    fmt = lambda v, unit: "n/a" if v is None else "%.3f %s" % (v, unit)
    return "%s: %d frames %dx%d, %d pairs, %d lost, speed %s (%s of width), jitter %s (%s of width)" % (
        path, s["frames"], size[1], size[0], s["pairs"], s["lost"], fmt(s["speed_rms"], "px/frame"), fmt(s["speed_pct"], "%"),
        fmt(s["jitter_rms"], "px/frame"), fmt(s["jitter_pct"], "%"))


def _motion_line(path, s):
    fmt = lambda v, unit: "n/a" if v is None else "%.4f %s" % (v, unit)
    return "%s: roll %s, roll jitter %s, zoom jitter %s, wobble %s, %d unfit" % (
        path, fmt(s["roll_rms_deg"], "deg/frame"), fmt(s["roll_jitter_deg"], "deg/frame"), fmt(s["zoom_jitter_pct"], "%/frame"),
        fmt(s["wobble_rms"], "px"), s["unfit"])


def _run(args):
    from .pipe import _size
    if len(args.clips) > 2:
        raise _UsageError("one clip or two, got %d" % len(args.clips))
    if args.gate is not None and not args.motion:
        raise _UsageError("--gate belongs to --motion")
    if args.size is not None:
        try:
            args.size = _size(args.size, "--size")
        except Exception as e:
            raise _UsageError(str(e)) from None
    if args.format != "y4m" and args.size is None:
        raise _UsageError("--format %s has no header: --size WxH is required" % args.format)
    files, readers = [], []
    try:
        for path in args.clips:
            f, r = _open(path, args)
            files.append(f)
            readers.append(r)
        sizes = [(r.width, r.height) for r in readers]
        if len(set(sizes)) > 1:   # decided from the headers, before any device work
            raise _UsageError("the clips differ in size (%dx%d and %dx%d): motion scales with the picture, compare like with like"
                              % (sizes[0] + sizes[1]))
        measured = [_measure_file(r, args) for r in readers]
        tracks, motions = [m[0] for m in measured], [m[1] for m in measured]
    finally:
        for f in files:
            f.close()
    if len(tracks) == 2:
        result = compare(*tracks)
        result.update(files=list(args.clips), factor=tracks[0].factor)
    else:
        result = dict(a=summary(tracks[0]), files=list(args.clips), factor=tracks[0].factor)
    if args.motion and len(tracks) == 2:
        m = compare_motion(motions[0], motions[1], args.min_blocks)
        result.update(motion_a=m["a"], motion_b=m["b"], roll_jitter_ratio=m["roll_jitter_ratio"], wobble_ratio=m["wobble_ratio"])
    elif args.motion:
        result.update(motion_a=motion_summary(motions[0], args.min_blocks))
    if args.json:
        print(json.dumps(result))
        return 0
    for key, path, track in zip("ab", args.clips, tracks):
        print(_line(path, result[key], track.size))
        if args.motion:
            print(_motion_line(path, result["motion_" + key]))
    if len(tracks) == 2:
        ratio = result["jitter_ratio"]
        print("jitter ratio B / A: %s" % ("n/a" if ratio is None else "%.3f" % ratio))
        if args.motion:
            for name, key in (("roll jitter", "roll_jitter_ratio"), ("wobble", "wobble_ratio")):
                print("%s ratio B / A: %s" % (name, "n/a" if result[key] is None else "%.3f" % result[key]))
    return 0


def main(argv=None):
    """The front end; returns the exit status.  A bad option, a malformed stream, a missing file and clips of different
    sizes end with status 1 and one line on stderr."""
    from .y4m import Y4MError
    args = _parser().parse_args(argv)
    try:
        return _run(args)
    except (_UsageError, Y4MError, ValueError, OSError, _lib.DvsgError) as e:
        sys.stderr.write("%s: error: %s\n" % (PROG, " ".join(str(e).split())))
    return 1


if __name__ == "__main__":
    sys.exit(main())
