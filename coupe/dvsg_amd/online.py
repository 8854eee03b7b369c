"""eval.py:93-124 online: one frame in, its stabilised frame out, for several streams that share one GPU.

The reference's driver is causal -- the output for frame k depends on frames up to k and on earlier outputs only -- so
it does not need the whole clip.  `clip.stabilize_clip` keeps a clip of N frames in a pool of 2 N; here every stream
owns a RING of span + 2 pool frames (span = skip_length[-1] = 32) from `base`:

  * span + 1 history slots: stabilised frame j lives in base + j % (span + 1);
  * one input slot base + span + 1: the unstable frame of the current step.

The window of step k (`stream_window_row`) names the input slot in its last entry and, for k >= 1, the history slot of
stabilised frame max(k + skip[s] - span, 0) in entry s: eval.py's padded history list, whose 32 prepended copies of
frame 0 are the unstable frame 0 at step 0 (every entry the input slot, eval.py:93-94) and the stabilised frame 0
afterwards (the write-back of :118-120).  Step k writes its result into the history slot of frame k; that slot held
frame k - span - 1, which no window of step k reads (they read frames k - span .. k - 1).

`OnlineStabilizer.step` runs every stream that has a frame in ONE `dvsg_stabilize_ring_inplace_f32` call (B = number
of those streams), whose warp stores each result straight into its stream's history slot: independent streams keep
their own lag-1 recurrence and still share batched CNN launches.  The pool never grows with the length of a stream.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib   # binds the library on the first call, not here: importing this module needs neither it nor a device
from ._tensor import device, ptr, stream
from .clip import SKIP_LENGTH, _check_crop, _check_crop_grid, _check_window, check_skip_length, render_source_into


YUV_MATRICES = {"bt601": 0, "bt709": 1}   # DVSG_YUV_BT601_LIMITED, DVSG_YUV_BT709_LIMITED
SURFACE_FORMATS = ("nv12", "p010", "nv16", "p210")   # frame formats that are decoder surfaces: two planes, a source-size render
# a surface format's sample type and chroma sampling, by the names `LocNet.view` gives them (surface=, chroma=)
SURFACE_OF = {"nv12": ("nv12", "420"), "p010": ("p010", "420"), "nv16": ("nv12", "422"), "p210": ("p010", "422")}
WORD_FORMATS = ("p010", "p210")            # surfaces of 16-bit words: uint8 [.., 2 W0] or uint16 [.., W0], returned as given
SCENE_STATE_INTS = 68                     # DVSG_SCENE_STATE_INTS: k, cuts, S, 0, the previous histogram [64]


def _check_scene_cut(scene_cut):
    """scene_cut argument of OnlineStabilizer -> None or a float64 threshold in (0, 1]"""
    if scene_cut is None:
        return None
    if isinstance(scene_cut, (str, bytes, bool)) or not np.isscalar(scene_cut):
        raise ValueError("scene_cut must be None or a threshold in (0, 1], got %r" % (scene_cut,))
    t = float(scene_cut)
    if not (t > 0.0 and t <= 1.0):       # NaN fails both
        raise ValueError("scene_cut must be None or a threshold in (0, 1], got %r" % (scene_cut,))
    return t


def scene_threshold_count(threshold, h, w):
    """thr_count of dvsg_scene_step_f32: ceil(threshold * 2 h w) in float64, an int in [1, 2 h w]."""
    return int(np.ceil(np.float64(threshold) * np.float64(2 * int(h) * int(w))))


def stream_window_row(k, base, skip_length=SKIP_LENGTH):
    """Window of step k of a stream whose ring starts at pool frame `base`: (row int32 [S], out_slot), where row[s] is
    the pool frame window slot s reads (eval.py:103's `sample_idx` on the ring) and out_slot the history slot that
    receives stabilised frame k (eval.py:116)."""
    skip = check_skip_length(skip_length)
    k, base = int(k), int(base)
    if k < 0 or base < 0:
        raise ValueError("step k and base must be >= 0, got k=%d base=%d" % (k, base))
    span = int(skip[-1])
    hist = span + 1
    if k == 0:
        row = np.full(skip.size, base + hist, dtype=np.int32)          # 32 copies of unstable frame 0 (eval.py:93-94)
    else:
        row = (base + np.maximum(k + skip - span, 0) % hist).astype(np.int32)
        row[-1] = base + hist                                           # the unstable frame k (eval.py:103)
    return row, base + k % hist


# One frame of a step.  key: what rows of one ingest and render launch share (`_rgb_key`, `_surface_key`); host: the frame
# came from NumPy; t: the frame as a tensor, surfaces in the uint8 form; ring, k: the stream's ring and step count; words: the
# output goes back as 16-bit words.
Row = namedtuple("Row", "key sid host t ring k words")

# The slot rows of a step on the device: table int32 [B,S], out_slots and in_slots int32 [B]; rings int32 [B] with
# scene_cut (table and out_slots are then written by `dvsg_scene_step_f32`), else None.
SlotTables = namedtuple("SlotTables", "table out_slots in_slots rings")


def _words_to_bytes(x, what):
    """P010 given as 16-bit words -- host uint16, or torch.uint16 where this torch has it -- as the uint8 form, the words'
    bytes as they lie in memory: (x, whether it was words).  Anything else comes back as it is."""
    if isinstance(x, torch.Tensor):
        u16 = getattr(torch, "uint16", None)
        return (x.contiguous().view(torch.uint8), True) if u16 is not None and x.dtype == u16 else (x, False)
    if np.asarray(x).dtype != np.uint16:
        return x, False
    if not np.little_endian:
        raise ValueError("%s: P010 words are little-endian; pass the uint8 form on this host" % (what,))
    return np.ascontiguousarray(x).view(np.uint8), True


def _bytes_to_words(x):
    """A result in the uint8 form back as 16-bit words, NumPy or device tensor."""
    return x.view(np.uint16) if isinstance(x, np.ndarray) else x.view(torch.uint16)


def _rgb_key(sid, t, h, w, source_res, crop):
    """Check an RGB frame; its sort key: resized uint8 (0, H0, W0), same-size uint8 (1,), float32 (2,), float64 (3,)."""
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("stream %r: a frame must be [h,w,3], got %s" % (sid, tuple(t.shape)))
    if t.dtype == torch.uint8:
        if crop and source_res:
            _check_crop_grid(int(t.shape[0]), int(t.shape[1]))
        return (0, int(t.shape[0]), int(t.shape[1])) if tuple(t.shape[:2]) != (h, w) else (1,)
    if not t.dtype.is_floating_point:
        raise TypeError("stream %r: frames must be uint8 or floating point, got %s" % (sid, t.dtype))
    if source_res:
        raise ValueError("stream %r: source_res renders the uint8 source frame; a float frame has no source "
                         "beyond the model's size" % (sid,))
    if tuple(t.shape[:2]) != (h, w):
        raise ValueError("stream %r: float frames must already be [%d,%d,3] (StabNet(h, w) fixes the STN "
                         "out_size), got %s" % (sid, h, w, tuple(t.shape)))
    return (3,) if t.dtype == torch.float64 else (2,)


def _surface_rows(name, H0):
    """The rows of a packed surface of height H0: H0 of Y, then the UV plane's H0 / 2 (4:2:0) or H0 (4:2:2)."""
    return 2 * H0 if SURFACE_OF[name][1] == "422" else 3 * H0 // 2


def _surface_key(sid, t, name):
    """Check an NV12, P010, NV16 or P210 surface in the uint8 form; its sort key (H0, W0)."""
    bps = 2 if name in WORD_FORMATS else 1   # the bytes of a sample
    c422 = SURFACE_OF[name][1] == "422"      # R rows are H0 of Y and H0 / 2 (4:2:0) or H0 (4:2:2) of UV
    layout = "[%s, %sW0]" % ("2*H0" if c422 else "3*H0/2", "2*" if bps == 2 else "")
    article = "a" if bps == 2 else "an"
    if t.dtype.is_floating_point:
        raise ValueError("stream %r: frame_format=%r takes uint8 surfaces, not float frames (%s)" % (sid, name, t.dtype))
    if t.dtype != torch.uint8:
        raise TypeError("stream %r: %s frames must be uint8%s, got %s"
                        % (sid, name.upper(), " or uint16" if bps == 2 else "", t.dtype))
    if t.dim() != 2:
        raise ValueError("stream %r: %s %s frame must be %s, got %s" % (sid, article, name.upper(), layout, tuple(t.shape)))
    R, W0 = int(t.shape[0]), int(t.shape[1]) // bps
    H0 = R // 2 if c422 else 2 * R // 3
    if R % (2 if c422 else 3) or H0 % 2 or W0 % 2 or H0 < 4 or W0 < 4 or int(t.shape[1]) % bps:
        raise ValueError("stream %r: %s %s%s frame %s needs even H0, W0 >= 4 (odd sizes have no chroma layout), got %s"
                         % (sid, article, name.upper(), " uint8" if bps == 2 else "", layout, tuple(t.shape)))
    return (H0, W0)


def plan_step(frames, stream_of, h, w, frame_format="rgb", source_res=False, crop=False, out_size=None):
    """What a step of `frames` ({sid: frame}) will do, decided without a device: (rows, runs).  rows: one `Row` per frame in
    BATCH ORDER -- resized uint8 by source size, same-size uint8, float32, float64; surfaces by source size; equal keys in
    feed order -- and runs: the maximal ranges (i, j) of rows of one key, each one ingest and one render launch.
    stream_of(sid) -> (ring, count) of an open stream; h, w: the model's size; crop: whether the step crops.  Every frame is
    checked here, before the first launch: a bad frame raises and leaves every stream as it was.  out_size (H, W): the
    size every source-size render of the step writes; a frame it minifies more than 4x is a ValueError (`scaled_factors`).
    The grouping key stays the SOURCE size: frames of one source size share their factors too."""
    from .networks import scaled_factors
    rows = []
    for sid, fr in frames.items():
        ring, k = stream_of(sid)
        host, words = not isinstance(fr, torch.Tensor), False
        if frame_format in WORD_FORMATS:
            fr, words = _words_to_bytes(fr, "stream %r" % (sid,))
        t = torch.as_tensor(np.ascontiguousarray(fr)) if host else fr
        key = _surface_key(sid, t, frame_format) if frame_format in SURFACE_FORMATS else \
            _rgb_key(sid, t, h, w, source_res, crop)
        if out_size is not None:
            src = key if frame_format in SURFACE_FORMATS else tuple(int(v) for v in t.shape[:2])
            try:
                scaled_factors(src, out_size)
            except ValueError as e:
                raise ValueError("stream %r: %s" % (sid, e))
        rows.append(Row(key, sid, host, t, ring, k, words))
    rows.sort(key=lambda r: r.key)   # stable
    runs, i = [], 0
    while i < len(rows):
        j = i + 1
        while j < len(rows) and rows[j].key == rows[i].key:
            j += 1
        runs.append((i, j))
        i = j
    return rows, runs


class OnlineStabilizer(object):
    """eval.py:93-124 for up to `max_streams` live streams, one step at a time.

    stab = OnlineStabilizer(model, max_streams=4)
    sid = stab.open()
    out = stab.push(sid, frame)                    # or stab.step({sid: frame, sid2: frame2, ...}) -> {sid: out}
    stab.close(sid)                                # its ring is handed to the next open()

    Frames are [h0,w0,3] and take the formats of `clip.stabilize_clip`: uint8 (resized to the model's (w, h) and
    BGR-flipped with channel_order="bgr" as eval.py:79-80 does), or float RGB in [0,1] of the model's size (float64
    renders the unstable half of side_by_side from float64).  The output of a stream is its stabilised frame [h,w,3]
    float32, or uint8 with as_uint8, and with side_by_side the pair (out, side [h,2w,3] uint8).  NumPy in -> NumPy out
    after a synchronise; device tensors in -> device tensors out with nothing synchronised.  model.precision selects
    the precision.

    One step: one `dvsg_frames_ingest_u8` launch per distinct uint8 source size (a float frame is copied into its
    input slot), ONE `dvsg_stabilize_ring_inplace_f32` call for all streams in the step, then the uint8 egress
    (`dvsg_frames_f32_to_u8_slots`) when asked for.  Streams may open and close at any step and a step may leave
    a stream out; each stream's step count advances only with its own frames.

    source_res=True: the output of a stream is rendered at the size of its uint8 frame [H0,W0,3] instead of the model's:
    the step's F_t warps the source frame itself (`dvsg_tps_render_u8`, one launch per distinct source size, reading the
    device copy ingest made), float32 [H0,W0,3] or uint8 with as_uint8, and side [H0,2 W0,3] = (source bytes | render)
    with side_by_side.  The recurrence is unchanged: the pool, F_t and the model-size history are those of a run
    without it.  Float frames carry no source beyond the model's size and raise ValueError.

    frame_format="nv12": frames arrive and leave as a decoder's NV12 surfaces, a 2-D uint8 array or device tensor
    [3 H0 / 2, W0] (H0 rows of Y, then H0 / 2 rows of interleaved UV; H0, W0 even), converted with yuv_matrix ("bt709" or
    "bt601", limited range).  source_res is implied: the output of a stream is its stabilised frame in the same layout
    at source size.  Per distinct source size one `dvsg_frames_ingest_nv12` launch converts and resizes straight into
    the input slots and one `dvsg_tps_render_nv12` launch warps both planes of the device copy ingest read; the step
    itself is still the one `dvsg_stabilize_ring_inplace_f32` call, on the same pool of model-size float RGB frames.
    side_by_side, as_uint8, channel_order="bgr", float frames and odd sizes raise ValueError.

    frame_format="p010": the same for 10-bit surfaces (include/dvsg_amd.h, "P010 frames"): a Y plane and an interleaved UV
    plane of 16-bit little-endian words, the sample in the high 10 bits.  A frame is a 2-D array or device tensor in one of
    two forms and comes back in the form it was given: uint8 [3 H0 / 2, 2 W0] (the words' bytes, low byte first), or uint16
    [3 H0 / 2, W0] (NumPy uint16, or torch.uint16 where this torch has it); internally it is the uint8 form.  The options,
    checks and results are those of "nv12" (even H0, W0 >= 4; no side_by_side, as_uint8 or channel_order; crop, scene_cut,
    border="keep" surfaces, strength and rigidity as there; the coverage scan's grids stay (H0, W0) and (H0 / 2, W0 / 2)).
    What the network sees is DEFINED as the NV12 surface made of each word's HIGH BYTE (word >> 8, the sample's top 8
    bits): one strided copy per source-size group, `src[..., 1::2]`, into a buffer this object owns, then the same
    `dvsg_frames_ingest_nv12`.  The pool, F_t and the crop state are therefore those of an "nv12" run fed those bytes.  The
    render goes through `LocNet.view(..., surface="p010")` with pitch = 2 W0 and warps the 10-bit planes themselves.

    frame_format="nv16" / "p210": 4:2:2 footage (camera originals, mezzanine files; include/dvsg_amd.h, "Chroma sampling"),
    8-bit and 10-bit.  A frame is H0 rows of Y, then H0 rows of interleaved UV: uint8 [2 H0, W0] for "nv16"; for "p210"
    uint8 [2 H0, 2 W0] or uint16 [2 H0, W0], returned in the form given, exactly as "p010".  The options, checks and results
    are those of "nv12" / "p010".  What the network sees is DEFINED as the NV12 surface made of the Y plane and the EVEN
    chroma rows (for "p210" the high byte of each of those words): one strided device copy per source-size run into the
    buffer this object owns, then the unchanged `dvsg_frames_ingest_nv12`.  The pool, F_t, scene cuts and the crop's inputs
    are therefore those of an "nv12" run fed that surface, bit for bit.  The render goes through
    `LocNet.view(..., surface=, chroma="422", out_size=)` and warps every chroma row; crop="auto" scans the chroma grid
    (H0, W0 / 2), with out_size the virtual grid (sy H, sx W / 2), and the default crop_margin stays one pixel of that
    grid's shorter axis.

    render_filter: the filter of the source-size render (source_res=True or frame_format="nv12", with and without crop).
    "bilinear" (default) is sampler A; "bicubic" gives the render calls a view of the network with that filter
    (`LocNet.view`, include/dvsg_amd.h "Views and the render filter": 16 taps, OpenCV's INTER_CUBIC weights, bytes rounded
    to nearest, the same black border).  The pool, F_t, the history and the crop's zoom are identical for both.  "bicubic"
    without a source-size render (RGB at the model's size) raises ValueError, as does a float frame pushed into it.

    border: what the source-size render (source_res=True or frame_format="nv12", either filter, with and without crop)
    makes of a sample whose taps leave the source (include/dvsg_amd.h, "Border modes").  "black" (default): 0, luma 0 /
    chroma 128.  "replicate" / "mirror": the filter evaluated at the coordinate clamped into / reflected once about the
    edge of the source; they only select the view the render calls are given (`LocNet.view`).  "keep": such a sample is
    not written, so it keeps what the stream showed there before.  Each ring owns a persistent output surface at its
    source size (allocated on first use, again when the stream's source size changes); a step renders into it and returns
    a fresh copy.  The surface restarts from the source bytes of frame f (float32 outputs: `dvsg_frames_u8_to_f32` of them,
    in the output's channel order) before f is rendered on the stream's step 0, after `reset(sid)`, and after a device-detected
    scene cut at f -- the last decided on the device from `dvsg_scene_step_f32`'s `cut` output by a masked copy, nothing
    synchronised.  The valid samples, the pool, F_t, the history and the crop's zoom are identical for every border; crop
    composes as it is, the border mode fills whatever the zoom leaves.  A border other than "black" without a
    source-size render raises ValueError, as does "keep" with side_by_side.

    strength, rigidity, shape_model: how much of the network's warp the source-size render applies (source_res=True or
    frame_format="nv12"; every filter and border, with and without crop and scene_cut; include/dvsg_amd.h, "Warp shaping").
    strength in [0, 1] scales the correction (0: the source as it is, for A/B viewing; 1, the default: all of it);
    rigidity in [0, 1] pulls the 25 control points' displacements towards their least-squares fit by shape_model --
    "affine" (default), "similarity" or "translation" -- so that rigidity=1 renders a warp that cannot wobble.  They only
    select the view (`LocNet.view`) that the render, the coverage scan of crop="auto" and the coefficient call are given, so
    the zoom is that of the border the shaped render draws, and they cost no launch.  The recurrence is untouched: the
    network was trained on its own full-strength history, so the pool, F_t and the model-size history are those of a run
    without shaping.  Anything but (1, 0) without a source-size render raises ValueError.

    crop: every output frame has a black border (luma 0 / chroma 128 in NV12) wherever sampler A's taps leave the source.
    None (default) returns the frames as they are.  A zoom z in (0, 1] renders every frame of every stream on the output
    grid scaled by z about its centre; nothing is scanned.  "auto" keeps ONE zoom per stream on the device and lowers it
    as the stream goes: per step and per source-size group, after the one stabilise call, the coverage scan of the
    step's F_t on the output's own grid (`dvsg_tps_coverage_net_f32`), the ratchet (`dvsg_crop_ratchet_f32`:
    z = min(max(free - crop_margin, crop_min), 1, z_before + crop_recover)) on the stream's entry of a [max_streams]
    state tensor, and the zoomed render -- `dvsg_tps_render_zoom_u8` (source_res), `dvsg_tps_render_zoom_nv12` (NV12) or,
    at the model's size, `dvsg_tps_warp_zoom_f32` from a gathered copy of the step's input slots (then
    `dvsg_frames_f32_to_u8` with as_uint8).  Device tensors in still means nothing synchronised.  With crop_recover = 0
    (default) the zoom of a stream never grows, so the picture never pumps; after the last frame it equals
    `clip.crop_zoom` of all the stream's frames.  `open()` starts a stream at crop_start.  NV12 scans both planes --
    chroma leaves the source one luma pixel before luma does -- and takes the smaller `free`; its default crop_margin is
    one pixel of the chroma grid's shorter axis, otherwise that of `clip.crop_zoom`.  The recurrence is untouched: the
    history slots keep uncropped frames, and the pool and F_t are those of a run without crop.  The unstable half of
    side_by_side stays the uncropped source.  `crop_state(sid)` reports a stream's zoom.

    out_size=(H, W): every stream's output has that size whatever its source size -- RGB [H, W, 3] (source_res=True),
    NV12 [3 H / 2, W], P010 in the form it was given -- rendered straight at that size by the scaled view of the render's
    handle (`LocNet.view(..., out_size=)`; include/dvsg_amd.h, "Output size"): each output sample is the float32 average of
    sy x sx samples of the TPS map on the virtual grid (sy H, sx W), sy = max(1, ceil(H0 / H)), sx = max(1, ceil(W0 / W)),
    so a 4K stream leaves at 1080p without a second resampling pass and without aliasing.  crop composes: a fixed zoom is
    passed through; "auto" scans the VIRTUAL grids ((sy H, sx W) and, for surfaces, (sy H / 2, sx W / 2)), so the zoom it
    settles on leaves no invalid virtual sample, and its default crop_margin is one pixel of the virtual (chroma) grid's
    shorter axis.  The recurrence is untouched: the pool, F_t, the history and scene_cut are those of a run without it.
    Without a source-size render (source_res=False with RGB), with border="keep", with side_by_side, with odd sizes for a
    surface format, or for a pushed frame it would minify more than 4x it raises ValueError.

    scene_cut: a live stream cuts, and after a cut the window would mix two scenes for `span` steps (and crop="auto" would keep
    the old scene's zoom for good).  None (default) leaves the caller to close() and open(); a step launches what it
    launches without the option.  A threshold in (0, 1] makes every stream notice its own cuts on the device: per step,
    after ingest and before the one stabilise call, ONE `dvsg_scene_step_f32` call takes the 64-bin luma histogram of each
    stream's input slot, S = the L1 distance to the histogram of the stream's previous frame, and declares a cut when
    S >= ceil(threshold * 2 h w) and at least max(1, scene_min_len) frames have passed since the ring's last start.  A cut
    at frame f is close(sid) + open() onto the same ring + push(f): f is step 0 of eval.py:93-94, the windows that follow count
    from f, and with crop="auto" the ring's zoom restarts at crop_start.  History slots that still hold the old scene are
    never read.  The step count lives in a [max_streams, 68] int32 state tensor on the device and the step's `table` and
    `out_slots` are written by that call -- the host uploads ring numbers and input slots only, and its per-stream counter
    is "frames pushed", nothing more.  Device tensors in still means nothing synchronised.  The statistic is taken from
    the float32 RGB pool at the model's size, so it is the same for uint8, float and NV12 sources.  There is no default
    threshold (none has been measured on real footage); hard cuts only -- a fade or a dissolve changes the histogram a
    little per frame and passes.  `scene_state(sid)` reports a stream's cuts; `reset(sid)` is the caller's own cut (a
    decoder's or an edit list's), with or without scene_cut: the stream's next frame is step 0."""

    def __init__(self, model, max_streams=1, skip_length=SKIP_LENGTH, channel_order="rgb", side_by_side=False,
                 as_uint8=False, source_res=False, frame_format="rgb", yuv_matrix="bt709", crop=None, crop_margin=None,
                 crop_min=0.5, crop_start=1.0, crop_recover=0.0, scene_cut=None, scene_min_len=1, render_filter="bilinear",
                 border="black", strength=1.0, rigidity=0.0, shape_model="affine", out_size=None):
        from .networks import check_border, check_out_size, check_render_filter, check_shape
        surface = frame_format in SURFACE_FORMATS
        out_size = check_out_size(out_size, bool(source_res) or surface, surface)
        if out_size is not None and border == "keep":
            raise ValueError("out_size has no border='keep': the surface a stream keeps has no counterpart at another size")
        if out_size is not None and side_by_side:
            raise ValueError("out_size has no side_by_side layout: the source half keeps the source's size")
        check_render_filter(render_filter, bool(source_res) or surface)
        check_border(border, bool(source_res) or surface)
        shape = check_shape(strength, rigidity, shape_model, bool(source_res) or surface)
        if border == "keep" and side_by_side:
            raise ValueError("border='keep' has no side_by_side layout: the surface a stream keeps is its output frame")
        crop = _check_crop(crop)
        scene_cut = _check_scene_cut(scene_cut)
        if isinstance(scene_min_len, bool) or not isinstance(scene_min_len, (int, np.integer)) or scene_min_len < 0:
            raise ValueError("scene_min_len must be an integer >= 0, got %r" % (scene_min_len,))
        if crop_margin is not None and not float(crop_margin) >= 0.0:
            raise ValueError("crop_margin must be None or >= 0, got %r" % (crop_margin,))
        if not 0.0 < float(crop_min) <= 1.0 or not 0.0 < float(crop_start) <= 1.0:
            raise ValueError("crop_min and crop_start must be in (0, 1], got %r and %r" % (crop_min, crop_start))
        if not float(crop_recover) >= 0.0:
            raise ValueError("crop_recover must be >= 0, got %r" % (crop_recover,))
        if channel_order not in ("rgb", "bgr"):
            raise ValueError("channel_order must be 'rgb' or 'bgr'")
        if frame_format not in ("rgb",) + SURFACE_FORMATS:
            raise ValueError("frame_format must be 'rgb', 'nv12' or 'p010', or for 4:2:2 'nv16' or 'p210', got %r"
                             % (frame_format,))
        if yuv_matrix not in YUV_MATRICES:
            raise ValueError("yuv_matrix must be 'bt709' or 'bt601', got %r" % (yuv_matrix,))
        if surface:
            if side_by_side:
                raise ValueError("frame_format=%r has no side_by_side layout: such a frame has two planes" % (frame_format,))
            if as_uint8:
                raise ValueError("frame_format=%r always returns frames in the layout it is given: as_uint8 does not apply"
                                 % (frame_format,))
            if channel_order != "rgb":
                raise ValueError("frame_format=%r has no channel_order: the pool is RGB, got %r" % (frame_format, channel_order))
            source_res = True
        if model.locnet is None:
            raise _lib.DvsgError("StabNet has no weights: call load_weights()/load_ckpt() first")
        skip = check_skip_length(skip_length)
        _check_window(model, skip.size)
        if int(max_streams) < 1:
            raise ValueError("max_streams must be >= 1, got %r" % (max_streams,))
        self.model = model
        self.skip_length = tuple(int(s) for s in skip)
        self.max_streams = int(max_streams)
        self.span = int(skip[-1])
        self.frames_per_stream = self.span + 2
        self.h, self.w = model.h, model.w
        self.flip = 1 if channel_order == "bgr" else 0
        self.side_by_side, self.as_uint8, self.source_res = bool(side_by_side), bool(as_uint8), bool(source_res)
        self.frame_format, self.yuv_matrix = frame_format, YUV_MATRICES[yuv_matrix]
        self.render_filter, self.border, self.out_size = render_filter, border, out_size
        self.strength, self.rigidity, self.shape_model = shape
        self._keep = {}           # border="keep": ring -> the stream's persistent output surface, at its source size
        self._keep_fresh = set()  # rings whose next frame is a step 0: the surface restarts from that frame's source bytes
        # frame_format="p010", "nv16", "p210": (H0, W0) -> (uint8 [max_streams, 3 H0 / 2, W0], the NV12 surface the network sees:
        # the words' high bytes, the even chroma rows, or both; for 4:2:2 the rows it is gathered from, else None)
        self._hi = {}
        self._cut = None          # int32 [B] on the device: the `cut` output of this step's dvsg_scene_step_f32
        dev = device()
        self.pool = torch.empty((self.max_streams * self.frames_per_stream, self.h, self.w, 3), dtype=torch.float32,
                                device=dev)
        self._F = torch.empty((self.max_streams, model.param_dim, 2), dtype=torch.float32, device=dev)
        # the TPS coefficients of a source-size render ([n,2,P+3], written by dvsg_tps_render_u8)
        self._T = torch.empty((self.max_streams, 2, model.param_dim + 3), dtype=torch.float32, device=dev) \
            if self.source_res or crop is not None else None
        self.crop, self._crop_auto = crop, isinstance(crop, str)
        self.crop_margin = None if crop_margin is None else float(crop_margin)
        self.crop_min, self.crop_start, self.crop_recover = float(crop_min), float(crop_start), float(crop_recover)
        self._crop_zoom = None    # float32 [max_streams]: "auto": the zoom of the stream that owns ring r; else the fixed zoom
        self._crop_last = {}      # sid -> (free float64 [n] of the stream's last step, its row)
        self._V = None            # V_src per frame, for the model-size zoomed warp
        if crop is not None:
            self._crop_zoom = torch.full((self.max_streams,), self.crop_start if isinstance(crop, str) else float(crop),
                                         dtype=torch.float32, device=dev)
            if not self.source_res:
                from .model import V_SRC
                _check_crop_grid(self.h, self.w)
                self._V = torch.from_numpy(V_SRC).to(dev).unsqueeze(0).repeat(self.max_streams, 1, 1).contiguous()
        self.scene_cut, self.scene_min_len = scene_cut, int(scene_min_len)
        self._scene = None        # int32 [max_streams, 68]: the scene state of the stream that owns ring r (dvsg_scene_step_f32)
        if scene_cut is not None:
            if 2 * self.h * self.w > 2 ** 31 - 1:
                raise ValueError("scene_cut: a frame of %d x %d is too large (2 h w must stay below 2^31)" % (self.h, self.w))
            self._scene_thr = scene_threshold_count(scene_cut, self.h, self.w)
            self._scene_skip = (ctypes.c_int32 * len(self.skip_length))(*self.skip_length)
            self._scene = torch.zeros((self.max_streams, SCENE_STATE_INTS), dtype=torch.int32, device=dev)
        self._free = list(range(self.max_streams))   # rings no open stream owns
        # sid -> [ring, count].  Without scene_cut the count is the stream's step k since open() / reset(); with it k lives on
        # the device (a cut resets it there) and the count is "frames pushed", which no window is derived from.
        self._streams = {}
        self._next_sid = 0

    @property
    def open_streams(self):
        return sorted(self._streams)

    def open(self):
        """Start a stream (its first frame is step 0 of eval.py) and return its id."""
        if not self._free:
            raise RuntimeError("all %d streams of this OnlineStabilizer are open: close one first" % self.max_streams)
        ring = self._free.pop(0)
        sid = self._next_sid
        self._next_sid += 1
        self._streams[sid] = [ring, 0]
        self._restart(ring)
        return sid

    def _restart(self, ring):
        """The device state of `ring` as a stream's first frame wants it: device fills, nothing synchronised."""
        if self._crop_auto:
            self._crop_zoom[ring] = self.crop_start
        if self._scene is not None:
            self._scene[ring].zero_()
        if self.border == "keep":
            self._keep_fresh.add(ring)

    def reset(self, sid):
        """The caller's own cut (a decoder's flag, an edit list): the next frame of the stream is step 0 of eval.py, as if the
        stream had been closed and opened onto the same ring.  With crop="auto" its zoom restarts at crop_start; with
        scene_cut its device state (frames since the cut, cuts, score, histogram) is zeroed like open() does."""
        st = self._stream(sid)
        if self._scene is None:
            st[1] = 0
        self._crop_last.pop(sid, None)
        self._restart(st[0])

    def close(self, sid):
        ring, _ = self._stream(sid)
        del self._streams[sid]
        self._crop_last.pop(sid, None)
        self._keep.pop(ring, None)
        self._free.append(ring)
        self._free.sort()

    def _stream(self, sid):
        st = self._streams.get(sid)
        if st is not None:
            return st
        if isinstance(sid, (int, np.integer)) and 0 <= sid < self._next_sid:
            raise ValueError("stream %d is closed" % sid)
        raise ValueError("stream %r was never opened" % (sid,))

    @property
    def _render_options(self):
        """The five options that select the view of a source-size render, by the names `LocNet.view` gives them."""
        return dict(render_filter=self.render_filter, border=self.border, strength=self.strength, rigidity=self.rigidity,
                    shape_model=self.shape_model)

    def _view(self, scan=False):
        """The handle a surface render is given, `LocNet.view(..., surface=frame_format)`, asked for at call time: the cache
        is LocNet's.  scan=True: the handle every call that only turns F_t into T is given (the coverage scan,
        `dvsg_tps_coefficients_f32`): the view the render uses without the surface, so that scan, crop and render see one
        warp; the network itself when nothing is shaped (the scan does not read a filter or a border)."""
        if not scan:
            surface, chroma = SURFACE_OF[self.frame_format]
            return self.model.locnet.view(surface=surface, out_size=self.out_size, chroma=chroma, **self._render_options)
        if self.strength == 1.0 and self.rigidity == 0.0:
            return self.model.locnet.handle
        return self.model.locnet.view(**self._render_options)

    def push(self, sid, frame):
        """`step` for a single stream: its output for `frame`."""
        return self.step({sid: frame})[sid]

    def crop_state(self, sid):
        """dict(zoom, free) of an open stream, after a synchronise: zoom np.float32, the zoom its last frame was rendered
        with (crop_start before the first; the fixed zoom with crop=z), and free, the `free` of `clip.crop_scan` for its
        last frame (NV12: the smaller of the luma and the chroma plane's), None before the first frame or with crop=z."""
        ring, _ = self._stream(sid)
        if self.crop is None:
            raise ValueError("this OnlineStabilizer was made without crop")
        last = self._crop_last.get(sid)
        return dict(zoom=np.float32(self._crop_zoom[ring].item()), free=None if last is None else float(last[0][last[1]].item()))

    def scene_state(self, sid):
        """dict(frames_since_cut, cuts, score) of an open stream, after a synchronise: the frames since the ring's last start
        (open, reset or a detected cut; the cut frame counts), the cuts detected since open() / reset(), and
        score = S / (2 h w) of its last frame in [0, 1] (0.0 before the second frame of a run)."""
        ring, _ = self._stream(sid)
        if self._scene is None:
            raise ValueError("this OnlineStabilizer was made without scene_cut")
        k, cuts, S = (int(v) for v in self._scene[ring, :3].tolist())
        return dict(frames_since_cut=k, cuts=cuts, score=S / float(2 * self.h * self.w))

    def _step_zoom(self, rows, i, j, grids):
        """The zoom of batch rows [i, j) -> float32 [j - i] on the device.  crop=z: the constant.  "auto": one coverage
        scan of the rows' F_t per grid of `grids` (one (H, W), or the luma and the chroma plane's), each with the source
        and the output of that size -- or, an entry (src_h, src_w, gh, gw), a source of one size scanned on the grid of
        another (out_size: the virtual grid) -- then the ratchet on the rows' streams; T rows [i, j) are written."""
        n = j - i
        if not self._crop_auto:
            return self._crop_zoom[:n]
        dev = device()
        rings = np.array([r.ring for r in rows[i:j]], dtype=np.int32)
        if np.unique(rings).size != n:
            raise ValueError("two frames of one step share a crop state slot")
        keys = torch.empty((len(grids), 2, n), dtype=torch.int32, device=dev)   # per grid: n_border | key_min
        grids = [g if len(g) == 4 else (g[0], g[1], g[0], g[1]) for g in grids]
        for g, (sh, sw, gh, gw) in enumerate(grids):
            need = ctypes.c_size_t()
            _lib.call("dvsg_tps_coverage_workspace_bytes", n, gh, gw, ctypes.byref(need))
            ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=dev)
            _lib.call("dvsg_tps_coverage_net_f32", self._view(scan=True), ptr(self._F[i:j]), None, n, sh, sw, gh, gw,
                      ptr(self._T[i:j]), ptr(keys[g, 0]), ptr(keys[g, 1]), ptr(ws), ws.numel() * 8, stream())
        slots = torch.from_numpy(rings).pin_memory().to(dev, non_blocking=True)
        zoom = torch.empty((n,), dtype=torch.float32, device=dev)
        free = torch.empty((n,), dtype=torch.float64, device=dev)
        D = [(gh - 1) * (gw - 1) for _, _, gh, gw in grids]
        margin = 2.0 / (min(grids[-1][2:]) - 1) if self.crop_margin is None else self.crop_margin
        _lib.call("dvsg_crop_ratchet_f32", ptr(keys[0, 1]), D[0], ptr(keys[1, 1]) if len(grids) > 1 else None,
                  D[1] if len(grids) > 1 else 0, ptr(slots), n, ptr(self._crop_zoom), self.max_streams, margin, self.crop_min,
                  self.crop_recover, ptr(zoom), ptr(free), stream())
        for b in range(i, j):
            self._crop_last[rows[b].sid] = (free, b - i)
        return zoom

    def _input_slot(self, ring):
        """The pool frame that holds the unstable frame of the step of the stream on `ring`."""
        return ring * self.frames_per_stream + self.span + 1

    def _slot_tables(self, rows):
        """The step's `SlotTables` for `rows` in batch order.  Without scene_cut one upload [table B*S | out slots B | input
        slots B] from the host's step counts.  With it the step count is the device's: the upload is [rings B | input slots B],
        and table and out slots are device buffers that `_scene_step` fills after ingest."""
        B, S = len(rows), len(self.skip_length)
        if self._scene is not None:
            rings = np.array([r.ring for r in rows], dtype=np.int32)
            if np.unique(rings).size != B:
                raise ValueError("two frames of one step share a ring")
            up = torch.from_numpy(np.concatenate([rings, self._input_slot(rings)])).pin_memory().to(device(), non_blocking=True)
            return SlotTables(torch.empty((B, S), dtype=torch.int32, device=device()),
                              torch.empty((B,), dtype=torch.int32, device=device()), up[B:], up[:B])
        host = np.empty(B * S + 2 * B, dtype=np.int32)     # [table B*S | out slots B | input slots B]
        for i, r in enumerate(rows):
            host[i * S:(i + 1) * S], host[B * S + i] = stream_window_row(r.k, r.ring * self.frames_per_stream, self.skip_length)
            host[B * S + B + i] = self._input_slot(r.ring)
        # a fresh pinned buffer per step: the caching host allocator does not hand it out again before this copy is done
        idx = torch.from_numpy(host).pin_memory().to(device(), non_blocking=True)
        return SlotTables(idx[:B * S].view(B, S), idx[B * S:B * S + B], idx[B * S + B:], None)

    def _scene_step(self, rings, table, out_slots):
        """scene_cut: the one `dvsg_scene_step_f32` call of a step, between ingest and the stabilise call.  It reads the step's
        input slots, decides every stream's cut and writes `table` and `out_slots`; only crop="auto" hands it the zoom
        state to restart."""
        B, S = int(table.shape[0]), len(self.skip_length)
        need = ctypes.c_size_t()
        _lib.call("dvsg_scene_workspace_bytes", B, ctypes.byref(need))
        ws = torch.empty((need.value + 3) // 4, dtype=torch.int32, device=device())
        cut = torch.empty((B,), dtype=torch.int32, device=device())
        _lib.call("dvsg_scene_step_f32", ptr(self.pool), int(self.pool.shape[0]), self.h, self.w, ptr(rings), B,
                  self._scene_skip, S, ptr(self._scene), self.max_streams, self._scene_thr, self.scene_min_len,
                  ptr(self._crop_zoom) if self._crop_auto else None, self.crop_start, ptr(table), ptr(out_slots), ptr(cut),
                  ptr(ws), ws.numel() * 4, stream())
        self._cut = cut

    def _keep_surfaces(self, rows, i, j, first):
        """border="keep": the output surfaces of batch rows [i, j) as one tensor to render into, and what to do after the
        render.  first [n, ...]: what a row's surface restarts from (its source frame in the output's form).  A surface is
        (re)started here on the host's word -- a new ring, reset(), another source size -- or, after a device-detected cut,
        by a masked copy on this step's `cut` flags.  Returns (out, done): render into out [n, ...], then done() gives the
        fresh copies to hand out (and stores the rendered rows back into their surfaces)."""
        surfs = []
        for b in range(i, j):
            ring, f = rows[b].ring, first[b - i]
            s = self._keep.get(ring)
            if s is None or s.shape != f.shape or s.dtype != f.dtype or ring in self._keep_fresh:
                s = self._keep[ring] = f.clone(memory_format=torch.contiguous_format)
                self._keep_fresh.discard(ring)
            elif self._cut is not None:
                s.copy_(torch.where(self._cut[b] != 0, f, s))
            surfs.append(s)
        if len(surfs) == 1:   # the surface itself is the launch's output
            out = surfs[0].unsqueeze(0)
            return out, out.clone
        out = torch.stack(surfs)

        def done():
            for s, o in zip(surfs, out):
                s.copy_(o)
            return out
        return out, done

    def step(self, frames):
        """One step of every stream in `frames` ({sid: frame}); returns {sid: output}.  What depends on the frame format is
        the check (`_rgb_key`, `_surface_key` under `plan_step`), the ingest of a run and its render."""
        if not frames:
            return {}
        rows, runs = plan_step(frames, self._stream, self.h, self.w, self.frame_format, self.source_res, self.crop is not None,
                               self.out_size)
        B = len(rows)
        if self.frame_format in SURFACE_FORMATS:
            ingest, render = self._ingest_surface, self._render_surface
        else:
            ingest = self._ingest_rgb
            render = self._render_source if self.source_res else self._egress_plain if self.crop is None else self._egress_cropped
        slots = self._slot_tables(rows)
        side = torch.empty((B, self.h, 2 * self.w, 3), dtype=torch.uint8, device=device()) \
            if self.side_by_side and not self.source_res else None
        # ---- ingest: the unstable frames into their input slots (eval.py:79-80); what a run's render reads, per run
        srcs = [ingest(rows, i, j, slots.in_slots, side) for i, j in runs]
        if side is not None:
            self._side_from_slots(rows, slots.in_slots, side)
        for size in set(self._hi).difference(r.key for r in rows):   # P010: a source size no stream of this step has
            del self._hi[size]
        # ---- the step: every stream's window from its ring, every result into its history slot (eval.py:101-120)
        if slots.rings is not None:
            self._scene_step(slots.rings, slots.table, slots.out_slots)
        self.model.locnet.stabilize_ring_inplace(self.pool, slots.table, slots.out_slots, self._F[:B],
                                                 precision=self.model.precision)
        for r in rows:
            self._streams[r.sid][1] += 1
        # ---- egress (eval.py:112-113): per run at source size, else the whole batch as one range; every range is handed
        # out before the next is rendered
        res = {}
        for (i, j), src in zip(runs, srcs) if self.source_res else [((0, B), None)]:
            out, sd = render(rows, i, j, src, slots, side)
            self._hand_out(res, rows[i:j], out, sd)
        return {sid: res[sid] for sid in frames}

    def _hand_out(self, res, rows, out, side=None):
        """res[sid] for `rows`, whose outputs are out[0], out[1], ... (and side[...], with side_by_side): NumPy for a row that
        came from the host -- one `.cpu()` per tensor, only if there is such a row -- else views of the device tensors; a
        row that came as 16-bit words leaves as such."""
        dev = (out,) if side is None else (out, side)
        cpu = tuple(t.cpu().numpy() for t in dev) if any(r.host for r in rows) else None
        for b, r in enumerate(rows):
            ts = cpu if r.host else dev
            o = _bytes_to_words(ts[0][b]) if r.words else ts[0][b]
            res[r.sid] = o if side is None else (o, ts[1][b])

    def _ingest_rgb(self, rows, i, j, in_slots, side):
        """Ingest of an RGB run: uint8 frames by one `dvsg_frames_ingest_u8` launch, which also writes the unstable half of
        `side` for resized frames; returns them on the device, [j-i,H0,W0,3].  Float frames are copied into their input slots
        (None); a float64 frame's half of `side` is rendered from the float64."""
        dev, h, w, kind = device(), self.h, self.w, rows[i].key[0]
        if kind <= 1:
            ts = [r.t.to(dev) for r in rows[i:j]]
            src = ts[0].contiguous() if j - i == 1 else torch.stack(ts)
            u8 = side[i:j] if side is not None and kind == 0 else None
            _lib.call("dvsg_frames_ingest_u8", ptr(src), j - i, int(src.shape[-3]), int(src.shape[-2]), self.flip,
                      ptr(self.pool), int(self.pool.shape[0]), ptr(in_slots[i:j]), h, w, ptr(u8), 2 * w, 0, stream())
            return src.view(j - i, *src.shape[-3:])
        for b in range(i, j):
            t = rows[b].t.to(dev)
            self.pool[self._input_slot(rows[b].ring)].copy_(t)   # one rounding to float32 (the feed cast)
            if side is not None and kind == 3:
                t = t.contiguous()
                _lib.call("dvsg_frames_f64_to_u8", ptr(t), 1, h, w, self.flip, ptr(side[b]), 2 * w, 0, stream())
        return None

    def _side_from_slots(self, rows, in_slots, side):
        """The unstable halves of `side` that ingest left: same-size uint8 and float32 rows, rendered from their float32
        input slots -- one contiguous range of the batch order."""
        left = [b for b, r in enumerate(rows) if r.key in ((1,), (2,))]
        if left:
            a, b = left[0], left[-1] + 1
            _lib.call("dvsg_frames_f32_to_u8_slots", ptr(self.pool), int(self.pool.shape[0]), ptr(in_slots[a:b]), b - a,
                      self.h, self.w, self.flip, ptr(side[a:b]), 2 * self.w, 0, stream())

    def _egress_plain(self, rows, i, j, src, slots, side):
        """Egress of a model-size step without crop, the whole batch: the history slots the step wrote.  `side` arrives with
        its unstable half written."""
        B, h, w, flip, n_pool = len(rows), self.h, self.w, self.flip, int(self.pool.shape[0])
        if side is not None:
            _lib.call("dvsg_frames_f32_to_u8_slots", ptr(self.pool), n_pool, ptr(slots.out_slots), B, h, w, flip, ptr(side),
                      2 * w, w, stream())
        if self.as_uint8:
            out = torch.empty((B, h, w, 3), dtype=torch.uint8, device=self.pool.device)
            _lib.call("dvsg_frames_f32_to_u8_slots", ptr(self.pool), n_pool, ptr(slots.out_slots), B, h, w, flip, ptr(out),
                      w, 0, stream())
        else:
            out = self.pool.index_select(0, slots.out_slots)   # the ring slot is overwritten span + 1 steps later
        return out, side

    def _egress_cropped(self, rows, i, j, src, slots, side):
        """Egress of a model-size step with crop, the whole batch: the step's unstable frames (a gathered copy of the input
        slots) warped once more by the step's own T on the zoomed grid (`dvsg_tps_warp_zoom_f32`); the history slots keep
        the uncropped frames.  `side` arrives with its unstable half written."""
        B, h, w, flip = len(rows), self.h, self.w, self.flip
        zoom = self._step_zoom(rows, 0, B, [(h, w)])
        if not self._crop_auto:   # no scan has written T
            _lib.call("dvsg_tps_coefficients_f32", self._view(scan=True), ptr(self._F[:B]), B, ptr(self._T[:B]), stream())
        u = self.pool.index_select(0, slots.in_slots)
        out = torch.empty_like(u)
        _lib.call("dvsg_tps_warp_zoom_f32", ptr(u), ptr(self._V[:B]), ptr(self._T[:B]), ptr(zoom), B, h, w, 3,
                  self.model.param_dim, h, w, ptr(out), None, None, stream())
        if side is not None:
            _lib.call("dvsg_frames_f32_to_u8", ptr(out), B, h, w, flip, ptr(side), 2 * w, w, stream())
        if self.as_uint8:
            f32, out = out, torch.empty((B, h, w, 3), dtype=torch.uint8, device=out.device)
            _lib.call("dvsg_frames_f32_to_u8", ptr(f32), B, h, w, flip, ptr(out), w, 0, stream())
        return out, side

    def _render_source(self, rows, i, j, src, slots, side):
        """Egress of a source_res run: one `dvsg_tps_render_u8` launch that warps the uint8 frames `src` by this step's F_t
        rows [i, j) at their own size."""
        n, H0, W0 = j - i, int(src.shape[1]), int(src.shape[2])
        done = None
        if self.border == "keep":   # (no side_by_side): the streams' own surfaces, restarted from the source where due
            first = src
            if not self.as_uint8:   # the float32 frame the render's own samples are taken from (torch's / is not that)
                first = torch.empty((n, H0, W0, 3), dtype=torch.float32, device=src.device)
                _lib.call("dvsg_frames_u8_to_f32", ptr(src), n * H0 * W0, self.flip, ptr(first), stream())
            out, done = self._keep_surfaces(rows, i, j, first)
        else:
            oh, ow = (H0, W0) if self.out_size is None else self.out_size
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8 if self.as_uint8 else torch.float32, device=src.device)
        side = torch.empty((n, H0, 2 * W0, 3), dtype=torch.uint8, device=src.device) if self.side_by_side else None
        zoom = self._step_zoom(rows, i, j, self._scan_grids(H0, W0, False)) if self.crop is not None else None
        render_source_into(self.model, src, self._F[i:j], self._T[i:j], self.flip, out, side, zoom, out_size=self.out_size,
                           **self._render_options)
        return (out if done is None else done()), side

    def _scan_grids(self, H0, W0, surface):
        """The grids crop="auto" scans for a source of (H0, W0): the output's own -- with out_size the VIRTUAL grid
        (sy H, sx W) against the source's size, so that no virtual sample of the render is left invalid -- and for a
        surface the chroma plane's too: (H0 / 2, W0 / 2), or (H0, W0 / 2) for a 4:2:2 format."""
        c422 = surface and SURFACE_OF[self.frame_format][1] == "422"
        if self.out_size is None:
            return [(H0, W0), (H0 if c422 else H0 // 2, W0 // 2)] if surface else [(H0, W0)]
        from .networks import scaled_factors
        (oh, ow), (sy, sx) = self.out_size, scaled_factors((H0, W0), self.out_size)
        luma = (H0, W0, sy * oh, sx * ow)
        chroma = (H0, W0 // 2, sy * oh, sx * (ow // 2)) if c422 else (H0 // 2, W0 // 2, sy * (oh // 2), sx * (ow // 2))
        return [luma, chroma] if surface else [luma]

    def _ingest_surface(self, rows, i, j, in_slots, side):
        """Ingest of a run of surfaces of one size: one `dvsg_frames_ingest_nv12` launch; returns the frames on the device,
        [j-i, R, bps W0] (R: the format's rows, 3 H0 / 2 or 2 H0; bps: the bytes of a sample; words are handled as their bytes)."""
        dev, (H0, W0) = device(), rows[i].key
        src = torch.stack([r.t.to(dev) for r in rows[i:j]]).contiguous()
        seen = src
        if self.frame_format != "nv12":
            # the network sees an NV12 surface: the words' high bytes (P010, P210), the Y plane and the EVEN chroma rows
            # (NV16, P210): one strided copy into a buffer this object owns -- for 4:2:2 one gather of the rows 0 .. H0 - 1,
            # H0, H0 + 2, .. by an index kept beside the buffer
            buf, picked = self._hi.get((H0, W0), (None, None))
            if buf is None:
                buf = torch.empty((self.max_streams, 3 * H0 // 2, W0), dtype=torch.uint8, device=dev)
                if SURFACE_OF[self.frame_format][1] == "422":
                    # made on the device: a copy of a host index would wait for the caller's stream
                    picked = torch.cat([torch.arange(H0, device=dev), torch.arange(H0, 2 * H0, 2, device=dev)])
                self._hi[(H0, W0)] = (buf, picked)
            seen = buf[:j - i]
            hi = src[..., 1::2] if self.frame_format in WORD_FORMATS else src
            if picked is not None:
                torch.index_select(hi, 1, picked, out=seen)
            else:
                seen.copy_(hi)
        _lib.call("dvsg_frames_ingest_nv12", ptr(seen), ptr(seen) + H0 * W0, W0, 3 * H0 // 2 * W0, j - i, H0, W0,
                  self.yuv_matrix, ptr(self.pool), int(self.pool.shape[0]), ptr(in_slots[i:j]), self.h, self.w, stream())
        return src

    def _render_surface(self, rows, i, j, src, slots, side):
        """Egress of a run of surfaces: one `dvsg_tps_render_nv12` (or `_zoom_nv12`) launch that warps both planes of `src`."""
        (H0, W0), net = rows[i].key, self._view()
        pitch = int(src.shape[2])   # bps W0: rows are packed; the UV plane follows the Y plane
        oh, ow = (H0, W0) if self.out_size is None else self.out_size
        R0, ro = _surface_rows(self.frame_format, H0), _surface_rows(self.frame_format, oh)   # a frame's rows, in and out
        if self.border == "keep":
            out, done = self._keep_surfaces(rows, i, j, src)
        else:
            out, done = torch.empty((j - i, ro, pitch // W0 * ow), dtype=src.dtype, device=src.device), None
        opitch = int(out.shape[2])
        if self.crop is None:
            _lib.call("dvsg_tps_render_nv12", net, ptr(self._F[i:j]), ptr(src), ptr(src) + H0 * pitch, pitch,
                      R0 * pitch, j - i, H0, W0, ptr(self._T[i:j]), ptr(out), ptr(out) + oh * opitch, opitch,
                      ro * opitch, stream())
        else:   # chroma leaves the source first: both planes are scanned, each on its own grid
            zoom = self._step_zoom(rows, i, j, self._scan_grids(H0, W0, True))
            _lib.call("dvsg_tps_render_zoom_nv12", net, ptr(self._F[i:j]), ptr(src),
                      ptr(src) + H0 * pitch, pitch, R0 * pitch, j - i, H0, W0, ptr(zoom), ptr(self._T[i:j]),
                      ptr(out), ptr(out) + oh * opitch, opitch, ro * opitch, stream())
        return (out if done is None else done()), None


def stabilize_clips(model, clips, batch=None, **kw):
    """eval.py:76-124 for K whole clips at once: the clips run through one `OnlineStabilizer` of `batch` streams
    (default K) in lockstep, so each step is one batched call and every clip keeps its own recurrence exactly.  Clips
    may differ in length (a finished clip's ring goes to the next waiting clip).  `kw` are OnlineStabilizer's options,
    scene_cut and scene_min_len among them: every clip then restarts its own history at its own cuts; strength, rigidity
    and shape_model shape every clip's source-size render alike.
    Returns a list with, per clip, what `clip.stabilize_clip` returns for it (NumPy for NumPy clips).  With
    frame_format="nv12" a clip is [N,3*H0/2,W0] uint8 and so is its result; with "p010" [N,3*H0/2,2*W0] uint8 or
    [N,3*H0/2,W0] uint16, likewise; with "nv16" / "p210" the same with 2*H0 rows.  crop=... is OnlineStabilizer's: frame k of a
    clip is rendered with the zoom the ratchet has reached at frame k, NOT with `stabilize_clip`'s one clip-wide zoom
    (the two agree from the frame on that sets the clip's minimum)."""
    K = len(clips)
    if K == 0:
        return []
    batch = K if batch is None else max(1, min(int(batch), K))
    dev = device()
    host = [not isinstance(c, torch.Tensor) for c in clips]
    dclips, words = [], []
    for c, hst in zip(clips, host):
        fmt = kw.get("frame_format", "rgb")
        words.append(False)
        if fmt in WORD_FORMATS:   # uint16 clips run in the uint8 form and come back as words
            c, words[-1] = _words_to_bytes(c, "clip %d" % len(dclips))
        t = (torch.as_tensor(np.ascontiguousarray(c)) if hst else c).to(dev).contiguous()
        if fmt in SURFACE_FORMATS:
            if t.dim() != 3 or t.shape[0] < 1:
                raise ValueError("every %s clip must be [N,%s,%sW0] with N >= 1, got %s"
                                 % (fmt.upper(), "2*H0" if SURFACE_OF[fmt][1] == "422" else "3*H0/2",
                                    "2*" if fmt in WORD_FORMATS else "", tuple(t.shape)))
        elif t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
            raise ValueError("every clip must be [N,h,w,3] with N >= 1, got %s" % (tuple(t.shape),))
        dclips.append(t)
    on = OnlineStabilizer(model, max_streams=batch, **kw)
    outs = [[] for _ in range(K)]
    waiting = list(range(K))
    active = {}   # sid -> [clip, next frame]
    while waiting or active:
        while waiting and len(active) < batch:
            active[on.open()] = [waiting.pop(0), 0]
        res = on.step({sid: dclips[c][k] for sid, (c, k) in active.items()})
        for sid, r in res.items():
            c = active[sid][0]
            outs[c].append(r)
            active[sid][1] += 1
            if active[sid][1] == dclips[c].shape[0]:
                on.close(sid)
                del active[sid]
    result = []
    for c in range(K):
        if on.side_by_side:
            o = (torch.stack([r[0] for r in outs[c]]), torch.stack([r[1] for r in outs[c]]))
            o = tuple(x.cpu().numpy() for x in o) if host[c] else o
        else:
            o = torch.stack(outs[c])
            o = o.cpu().numpy() if host[c] else o
            if words[c]:
                o = _bytes_to_words(o)
        result.append(o)
    return result
