"""Stabilise video that arrives over pipes: Y4M or raw NV12 in, the same out, with reading, upload, the step, download and
writing overlapped.

    ffmpeg -i shaky.mp4 -f yuv4mpegpipe -pix_fmt yuv420p - \\
      | python -m coupe.dvsg_amd.pipe --ckpt DIR --crop auto --scene-cut 0.75 \\
      | ffmpeg -i - -c:v libx264 steady.mp4

`stabilize_pipes` is `online.stabilize_clips` for sources whose length nobody knows in advance: one
`OnlineStabilizer(frame_format="nv12")`, the same schedule, and around each step three stages per source that keep `depth`
frames in flight.  The GPU work is OnlineStabilizer's own; the only device work added is the planar <-> semi-planar chroma
repack of `y4m`, two strided copies per frame.

A source owns `depth` SLOTS, each a pinned host input buffer with its device copy and a pinned host output buffer (with
device buffers for the two repacks where the source or the sink is Y4M).  A slot goes round three stations:

  (a) the source's reader thread fills the slot's pinned input buffer from the file object (`readinto`);
  (b) the calling thread uploads it on a copy stream (non_blocking, one event), makes the compute stream wait on that
      event, repacks I420 -> NV12 where the source is Y4M, runs ONE `OnlineStabilizer.step` for all sources of the step with
      device tensors in -> device tensors out (nothing synchronised), repacks NV12 -> I420 where the sink is Y4M, and
      downloads into the slot's pinned output buffer on a second copy stream behind an event;
  (c) the source's writer thread waits on that event -- the only host-side wait on the device -- writes the frame and hands
      the slot back to the reader.

Ten-bit runs (`C420p10` Y4M or raw P010 at every end) are the same loop around one `OnlineStabilizer(frame_format="p010")`:
frames are uint8 [3 H / 2, 2 W], the repacks are `y4m.i420p10_to_p010` and `y4m.p010_to_i420p10`.  All ends of one call share
a bit depth.

4:2:2 runs (`C422` / `C422p10` Y4M, raw NV16 or raw P210 at every end) are the same loop again around one
`OnlineStabilizer(frame_format="nv16")` or `("p210")`: frames are uint8 [2 H, W] or [2 H, 2 W], the repacks are
`y4m.i422_to_nv16` / `nv16_to_i422` and `y4m.i422p10_to_p210` / `p210_to_i422p10`.  All ends of one call share their chroma
sampling as they share their bit depth.

A slot is not refilled before its frame is written, so a source never has more than `depth` frames between `readinto` and
`write` (back-pressure: a slow sink stalls its reader, memory does not grow), and every reuse hazard is covered by the order
of the stations: when a slot returns to (a) its download has finished, hence the step that read its device input, hence its
upload.  `depth=1` is the serial loop -- read, upload, step, download, write -- through the same code.
"""
import collections
import queue
import sys
import threading
import time

from . import y4m

_POLL = 0.05    # seconds between looks at the abort flag while a thread waits on a queue
_END = object()


class _Abort(Exception):
    """Raised inside the loop when another thread has failed; never leaves stabilize_pipes."""


class _Failure(object):
    def __init__(self, exc):
        self.exc = exc


class _Slot(object):
    __slots__ = ("host_in", "dev_in", "nv12_in", "dev_out", "host_out", "e_up", "e_step", "e_down")


class _Staging(object):
    """Where the frames are staged: a HIP device with two copy streams and events, or (only under an injected step, for the
    tests of the loop's mechanics) the host, where every copy is synchronous and no event exists."""

    def __init__(self, use_device):
        import torch
        self.torch = torch
        self.cuda = bool(use_device)
        if self.cuda:
            from ._tensor import device
            self.device = device()
            self.copy_in, self.copy_out = torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
        else:
            self.device = torch.device("cpu")

    def host(self, shape):
        return self.torch.empty(shape, dtype=self.torch.uint8, pin_memory=self.cuda)

    def dev(self, shape):
        return self.torch.empty(shape, dtype=self.torch.uint8, device=self.device)

    def event(self):
        return self.torch.cuda.Event() if self.cuda else None

    def fence(self):
        """Fresh device buffers may be memory that work already queued on the compute stream still uses: the upload stream,
        which the allocator knows nothing of, waits for that work (on the device; the host goes on)."""
        if self.cuda:
            e = self.torch.cuda.Event()
            e.record(self.torch.cuda.current_stream())
            self.copy_in.wait_event(e)

    def drain(self):
        """After the loop: nothing is left on the copy streams when the buffers go back to the allocator."""
        if self.cuda:
            self.copy_in.synchronize()
            self.copy_out.synchronize()

    def upload(self, slot):
        """host_in -> dev_in on the copy stream; the compute stream waits for it."""
        if not self.cuda:
            slot.dev_in.copy_(slot.host_in)
            return
        torch = self.torch
        with torch.cuda.stream(self.copy_in):
            slot.dev_in.copy_(slot.host_in, non_blocking=True)
            slot.e_up.record(self.copy_in)
        torch.cuda.current_stream().wait_event(slot.e_up)

    def download(self, slot, src):
        """src (written on the compute stream) -> host_out on the other copy stream, behind e_down."""
        if not self.cuda:
            slot.host_out.copy_(src)
            return
        torch = self.torch
        slot.e_step.record(torch.cuda.current_stream())
        self.copy_out.wait_event(slot.e_step)
        with torch.cuda.stream(self.copy_out):
            slot.host_out.copy_(src, non_blocking=True)
            slot.e_down.record(self.copy_out)
        if src is not slot.dev_out:
            src.record_stream(self.copy_out)    # the step's own output tensor: its memory is not reused before the copy


# the planar layouts and their repacks to and from what OnlineStabilizer takes
_PLANAR = {"i420": (y4m.i420_to_nv12, y4m.nv12_to_i420), "i420p10": (y4m.i420p10_to_p010, y4m.p010_to_i420p10),
           "i422": (y4m.i422_to_nv16, y4m.nv16_to_i422), "i422p10": (y4m.i422p10_to_p210, y4m.p210_to_i422p10)}
# the OnlineStabilizer frame format of a run, by (bit depth, chroma sampling)
_FRAME_FORMAT = {(8, "420"): "nv12", (10, "420"): "p010", (8, "422"): "nv16", (10, "422"): "p210"}


def _frame_shape(height, width, bits, chroma):
    """[3 H / 2, W] of a 4:2:0 frame or [2 H, W] of a 4:2:2 one; a 10-bit row is 2 W bytes."""
    return (y4m._frame_rows(int(height), chroma), (2 if bits == 10 else 1) * int(width))


class _Lane(object):
    """One source, its sink, its slots and its two threads."""

    def __init__(self, index, source, sink, depth, staging, shared, out_shape=None):
        self.index, self.source, self.sink, self.depth = index, source, sink, depth
        self.staging, self.shared = staging, shared
        self.frames = 0          # frames written
        self.in_flight = 0       # frames between readinto and write
        self.high_water = 0
        self.lock = threading.Lock()
        self.write_failed = False
        self.finished = False
        self.state = None        # device snapshots of the stream's crop / scene state, taken when it closes
        self.t0 = time.perf_counter()
        self.seconds = None
        shape = tuple(source.frame_shape)
        out_shape = shape if out_shape is None else tuple(out_shape)   # out_size: the stabilised frames have another size
        self.free = queue.Queue(maxsize=depth)          # slots the reader may fill
        self.filled = queue.Queue(maxsize=depth + 1)    # slots with a frame, then _END or a _Failure
        self.towrite = queue.Queue(maxsize=depth + 1)   # slots with a stabilised frame on its way, then _END
        for _ in range(depth):
            s = _Slot()
            s.host_in, s.dev_in = staging.host(shape), staging.dev(shape)
            s.nv12_in = staging.dev(shape) if source.layout in _PLANAR else None
            s.dev_out = staging.dev(out_shape) if sink.layout in _PLANAR else None
            s.host_out = staging.host(out_shape)
            s.e_up, s.e_step, s.e_down = staging.event(), staging.event(), staging.event()
            self.free.put(s)
        staging.fence()
        name = "stabilize_pipes-%d" % index
        self.reader = threading.Thread(target=self._read_loop, name=name + "-reader", daemon=True)
        self.writer = threading.Thread(target=self._write_loop, name=name + "-writer", daemon=True)
        self.reader.start()
        self.writer.start()

    # ---- (a)
    def _read_loop(self):
        stop = self.shared.stop
        try:
            while True:
                slot = None
                while slot is None:
                    if stop.is_set():
                        return
                    try:
                        slot = self.free.get(timeout=_POLL)
                    except queue.Empty:
                        pass
                if not self.source.readinto(slot.host_in.numpy()):
                    self.filled.put(_END)
                    return
                with self.lock:
                    self.in_flight += 1
                    self.high_water = max(self.high_water, self.in_flight)
                self.filled.put(slot)
        except BaseException as e:   # handed to the loop in stream order: the frames before it are still stabilised
            self.filled.put(_Failure(e))

    def next_slot(self):
        """The slot of the source's next frame, or None at its end; raises what the reader raised."""
        while True:
            if self.shared.failed.is_set():
                raise _Abort()
            try:
                item = self.filled.get(timeout=_POLL)
            except queue.Empty:
                continue
            if item is _END:
                return None
            if isinstance(item, _Failure):
                raise item.exc
            return item

    # ---- (b)
    def upload(self, slot):
        """The slot's frame on the device as NV12 [3 H / 2, W] (10-bit: P010 [3 H / 2, 2 W]), ordered on the compute stream."""
        self.staging.upload(slot)
        if slot.nv12_in is None:
            return slot.dev_in
        return _PLANAR[self.source.layout][0](slot.dev_in, out=slot.nv12_in)

    def submit(self, slot, out):
        """The stabilised NV12 frame `out` (device) on its way to the sink."""
        if tuple(out.shape) != tuple(slot.host_out.shape):
            raise ValueError("source %d: the step returned %s for a frame of %s" % (self.index, tuple(out.shape),
                                                                                  tuple(slot.host_out.shape)))
        src = out if slot.dev_out is None else _PLANAR[self.sink.layout][1](out, out=slot.dev_out)
        self.staging.download(slot, src)
        self.towrite.put(slot)

    # ---- (c)
    def _write_loop(self):
        while True:
            slot = self.towrite.get()
            if slot is _END:
                break
            try:
                if not self.write_failed:    # after a failed write the slots only go round, so that nothing blocks
                    if slot.e_down is not None:
                        slot.e_down.synchronize()
                    self.sink.write(slot.host_out.numpy())
                    self.frames += 1
            except BaseException as e:
                self.write_failed = True
                self.shared.fail(e)
            finally:
                with self.lock:
                    self.in_flight -= 1
                self.free.put(slot)
        try:
            if not self.write_failed and hasattr(self.sink, "flush"):
                self.sink.flush()
        except BaseException as e:
            self.shared.fail(e)
        self.seconds = time.perf_counter() - self.t0

    def finish(self):
        """No more frames will be submitted: the writer ends after those it has."""
        if not self.finished:
            self.finished = True
            self.towrite.put(_END)

    def join(self):
        self.reader.join()
        self.writer.join()


class _Shared(object):
    def __init__(self):
        self.stop = threading.Event()      # readers: read nothing more
        self.failed = threading.Event()    # the loop: stop stepping
        self.lock = threading.Lock()
        self.errors = []

    def fail(self, exc):
        with self.lock:
            self.errors.append(exc)
        self.failed.set()


class _NoRings(object):
    """open() / close() for an injected step, which owns no rings."""

    def __init__(self):
        self.n = 0

    def open(self):
        self.n += 1
        return self.n - 1

    def close(self, sid):
        pass


def _snapshot(on, sid):
    """The stream's zoom and scene state as device copies, ordered on the compute stream: nothing synchronised."""
    state = {}
    if getattr(on, "crop", None) is not None:
        state["zoom"] = on._crop_zoom[on._stream(sid)[0]].clone()
    if getattr(on, "_scene", None) is not None:
        state["cuts"] = on._scene[on._stream(sid)[0], 1].clone()
    return state


def _ends_format(sources, sinks, out_size=None):
    """Everything that can be said of the ends before a frame is read; returns the run's (bit depth, chroma sampling),
    (8, "420") without sources.  out_size (H, W): what every sink that states a size must state instead of its source's."""
    if len(sources) != len(sinks):
        raise ValueError("stabilize_pipes needs one sink per source, got %d sources and %d sinks" % (len(sources), len(sinks)))
    bits = chroma = None
    for i, (src, snk) in enumerate(zip(sources, sinks)):
        for end, what in ((src, "source"), (snk, "sink")):
            layout = getattr(end, "layout", None)
            if layout not in y4m.LAYOUT_BITS:
                raise ValueError("%s %d: layout must be 'i420' or 'nv12' (10-bit: 'i420p10' or 'p010'; 4:2:2: 'i422', 'nv16', 'i422p10' "
                                 "or 'p210'), got %r" % (what, i, layout))
            bits = y4m.LAYOUT_BITS[layout] if bits is None else bits
            if y4m.LAYOUT_BITS[layout] != bits:
                raise ValueError("%s %d is %d-bit (%s) in a %d-bit run: all sources and sinks of one call share a bit depth"
                                 % (what, i, y4m.LAYOUT_BITS[layout], layout, bits))
            chroma = y4m.LAYOUT_CHROMA[layout] if chroma is None else chroma
            if y4m.LAYOUT_CHROMA[layout] != chroma:
                raise ValueError("%s %d is 4:2:%s (%s) in a 4:2:%s run: all sources and sinks of one call share their chroma "
                                 "sampling" % (what, i, y4m.LAYOUT_CHROMA[layout][2], layout, chroma[2]))
        y4m.check_size(int(src.width), int(src.height))
        if tuple(src.frame_shape) != _frame_shape(src.height, src.width, bits, chroma):
            raise ValueError("source %d: frame_shape %s is not [%s, %sW] of %d x %d"
                             % (i, tuple(src.frame_shape), "2 H" if chroma == "422" else "3 H / 2", "2 " if bits == 10 else "",
                                src.width, src.height))
        want = (src.width, src.height) if out_size is None else (out_size[1], out_size[0])
        size = (getattr(snk, "width", want[0]), getattr(snk, "height", want[1]))
        if size != want and out_size is not None:
            raise ValueError("sink %d is %d x %d but out_size is %d x %d" % ((i,) + size + want))
        if size != want:
            raise ValueError("sink %d is %d x %d but its source is %d x %d: the output has the size of the input"
                             % ((i,) + size + (src.width, src.height)))
    return bits or 8, chroma or "420"


def _check_ends(sources, sinks, out_size=None):
    """`_ends_format`'s checks; returns the run's bit depth alone."""
    return _ends_format(sources, sinks, out_size)[0]


def stabilize_pipes(model, sources, sinks, batch=None, depth=3, _step_fn=None, **online_kw):
    """Stabilise every source into its sink: sink i receives exactly the stabilised frames of source i, in order.

    sources, sinks: equal-length lists of `y4m` readers and writers, or any objects with their small interface --
        a source: `width`, `height`, `frame_shape` ((3 H / 2, W)), `layout` ("i420": Y, U plane, V plane; "nv12": Y,
            interleaved U V) and `readinto(buf) -> bool`, which fills the uint8 array `buf` [3 H / 2, W] with the next frame
            and returns False at the end of the stream instead;
        a sink: `layout`, `write(frame)` for a uint8 array [3 H / 2, W] that is only valid during the call, and optionally
            `flush()`, `width` and `height` (which must then be the source's).
        Sources may differ in size, layout and length; a sink may have another layout than its source.
        Ten bits: layouts "i420p10" (Y4M C420p10: planar, value in the low 10 bits of a little-endian word) and "p010"
        (semi-planar, value in the high 10 bits), frames uint8 [3 H / 2, 2 W].  All sources and sinks of one call share a
        bit depth; a mix raises ValueError before any frame is read.  A 10-bit run goes through one
        `OnlineStabilizer(frame_format="p010")`; an 8-bit run is what it was.
        4:2:2: layouts "i422" / "i422p10" (Y4M C422 / C422p10) and "nv16" / "p210", frames uint8 [2 H, W] / [2 H, 2 W].  All
        sources and sinks of one call share their chroma sampling too; a mix raises ValueError naming the end before any
        frame is read.  Such a run goes through `OnlineStabilizer(frame_format="nv16")` or `("p210")`.
    batch: streams per step (default: all sources).  depth: frames in flight per source, >= 1.
    online_kw: OnlineStabilizer's crop, crop_*, scene_cut, scene_min_len, skip_length, render_filter, border, strength, rigidity,
        shape_model, out_size and yuv_matrix, passed through.  out_size=(H, W): every sink receives frames of that size
        ([3 H / 2, W], 10-bit [3 H / 2, 2 W]) whatever its source's; a sink that states a size must state that one.
        yuv_matrix defaults to "auto" here: `y4m.default_yuv_matrix` of the first source's height, resolved per call.

    One `OnlineStabilizer(model, max_streams=batch, frame_format="nv12")` serves all sources on `stabilize_clips`' own
    schedule: sources are opened in order while a ring is free, every step takes one frame from every open source, and a
    source that ends closes and hands its ring to the next one waiting.  Every step's batch is therefore the one
    `stabilize_clips` runs on the same clips with the same `batch`, and the bytes are the same for every `depth`.

    The stages and their overlap are the module docstring's.  In steady state the host synchronises nothing: the writer
    threads wait on the download events of the buffers they are about to write, and that is all.

    Failure: when a reader, a writer or the step raises, the loop stops taking frames, the frames already stabilised are
    still written where their sink works, every thread is joined and the first exception is re-raised.  A reader's exception
    surfaces in stream order, after the frames before it have gone through.  No thread outlives the call; a thread blocked
    inside a source's own `readinto` is waited for, so a source must end or fail, not stall for ever.

    Returns a list with, per source, dict(frames written, high_water: the most frames it ever had between readinto and
    write (<= depth), seconds from its opening to its last write, zoom with crop and cuts with scene_cut, else None)."""
    sources, sinks = list(sources), list(sinks)
    out_size = online_kw.get("out_size")
    if out_size is not None:
        from .networks import check_out_size
        out_size = check_out_size(out_size, True, True)
    bits, chroma = _ends_format(sources, sinks, out_size)
    K = len(sources)
    if isinstance(depth, bool) or int(depth) != depth or depth < 1:
        raise ValueError("depth must be an integer >= 1, got %r" % (depth,))
    depth = int(depth)
    if K == 0:
        return []
    batch = K if batch is None else max(1, min(int(batch), K))
    if _step_fn is None:
        from .online import OnlineStabilizer
        kw = dict(online_kw)
        if kw.get("yuv_matrix", "auto") == "auto":
            kw["yuv_matrix"] = y4m.default_yuv_matrix(sources[0].height)
        on = OnlineStabilizer(model, max_streams=batch, frame_format=_FRAME_FORMAT[(bits, chroma)], **kw)
        step, staging = on.step, _Staging(True)
    else:
        import torch
        if online_kw:
            raise ValueError("an injected step takes no OnlineStabilizer options: %s" % sorted(online_kw))
        on, step, staging = _NoRings(), _step_fn, _Staging(torch.cuda.is_available())
    shared = _Shared()
    lanes = []                            # every lane ever started, in source order
    waiting = list(range(K))
    active = collections.OrderedDict()    # sid -> (lane, the slot of its next frame)

    def close(sid, lane):
        if _step_fn is None:
            lane.state = _snapshot(on, sid)
        on.close(sid)
        lane.finish()

    try:
        while waiting or active:
            for sid, (lane, slot) in list(active.items()):      # every open source's next frame, or its end
                slot = lane.next_slot()
                if slot is None:
                    del active[sid]
                    close(sid, lane)
                else:
                    active[sid] = (lane, slot)
            while waiting and len(active) < batch:
                i = waiting.pop(0)
                lane = _Lane(i, sources[i], sinks[i], depth, staging, shared,
                             None if out_size is None else _frame_shape(out_size[0], out_size[1], bits, chroma))
                lanes.append(lane)
                sid = on.open()
                slot = lane.next_slot()
                if slot is None:                                 # a stream without frames
                    close(sid, lane)
                else:
                    active[sid] = (lane, slot)
            if not active:
                continue
            res = step({sid: lane.upload(slot) for sid, (lane, slot) in active.items()})
            for sid, (lane, slot) in active.items():
                lane.submit(slot, res[sid])
    except _Abort:
        pass
    except BaseException as e:
        shared.fail(e)
    finally:
        shared.stop.set()
        for lane in lanes:
            lane.finish()
        for lane in lanes:
            lane.join()
        try:
            staging.drain()
        except BaseException as e:
            shared.fail(e)
    if shared.errors:
        raise shared.errors[0]
    stats = []
    by_index = {lane.index: lane for lane in lanes}
    for i in range(K):
        lane = by_index[i]
        state = lane.state or {}
        stats.append(dict(frames=lane.frames, high_water=lane.high_water, seconds=lane.seconds,
                          zoom=float(state["zoom"].item()) if "zoom" in state else None,
                          cuts=int(state["cuts"].item()) if "cuts" in state else None))
    return stats


def output_aspect(aspect, source_size, out_size):
    """The `A` tag of a Y4M output of (H, W) = out_size made from a source of source_size: the source's pixel aspect where
    the two sizes have the same shape (out_W src_H == out_H src_W: square pixels stay square), else unknown, (0, 0) ->
    "A0:0" -- a scaled picture of another shape has pixels of another shape, which nobody stated."""
    (sh, sw), (oh, ow) = source_size, out_size
    return aspect if ow * sh == oh * sw else (0, 0)


# ---- python -m coupe.dvsg_amd.pipe -----------------------------------------------------------------------------------
PROG = "coupe.dvsg_amd.pipe"


class _UsageError(Exception):
    pass


def _parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def error(self, message):     # one line and status 1, not argparse's usage block and status 2
            raise _UsageError(message)

    ap = Parser(prog=PROG, description="Stabilise uncompressed video from files or pipes (Y4M, raw NV12, P010, NV16 or P210).")
    ap.add_argument("--input", action="append", metavar="PATH|-", help="repeatable; default: stdin")
    ap.add_argument("--output", action="append", metavar="PATH|-", help="repeatable, one per input; default: stdout")
    ap.add_argument("--format", default="y4m", choices=["y4m", "nv12", "p010", "nv16", "p210"],
                    help="of the inputs (nv12, p010, 4:2:2 nv16, p210: header-less, need --size; y4m: C420, C420p10, C422, C422p10)")
    ap.add_argument("--output-format", default=None, choices=["y4m", "nv12", "p010", "nv16", "p210"],
                    help="of the outputs (default: --format); of the inputs' bit depth and chroma sampling")
    ap.add_argument("--size", default=None, metavar="WxH", help="frame size of raw NV12 / P010 / NV16 / P210 inputs")
    ap.add_argument("--fps", default="25", metavar="N[/D]", help="frame rate written to a Y4M output of a raw NV12 input")
    w = ap.add_mutually_exclusive_group(required=True)
    w.add_argument("--ckpt", metavar="DIR", help="reference checkpoint directory (with its `checkpoints` index)")
    w.add_argument("--npz", metavar="FILE", help="one reference checkpoint file")
    w.add_argument("--synthetic-weights", action="store_true", help="the seeded test checkpoint: for demos and tests only")
    ap.add_argument("--model-size", default="512x288", metavar="WxH", help="the CNN's frame size (config.py:12-13)")
    ap.add_argument("--precision", default="f32", choices=["f32", "f32x3", "f32s", "f16"])
    ap.add_argument("--skip-length", default=None, metavar="A,B,...", help="the window's frame offsets (default: the "
                    "reference's 0,16,24,28,30,31,32); their number is fixed by the checkpoint")
    ap.add_argument("--crop", default=None, metavar="auto|Z")
    ap.add_argument("--crop-min", type=float, default=None)
    ap.add_argument("--crop-margin", type=float, default=None)
    ap.add_argument("--crop-recover", type=float, default=None)
    ap.add_argument("--render-filter", default=None, choices=["bilinear", "bicubic"],
                    help="filter of the source-size render (default: bilinear)")
    ap.add_argument("--border", default=None, choices=["black", "replicate", "mirror", "keep"],
                    help="what the render makes of samples outside the source: black (default), the source's edge "
                    "replicated or mirrored, or keep what the stream showed there before")
    ap.add_argument("--strength", type=float, default=None, metavar="S",
                    help="fraction of the network's warp that is rendered, in [0, 1] (default 1; 0 shows the source)")
    ap.add_argument("--rigidity", type=float, default=None, metavar="R",
                    help="pull of the rendered warp towards its --shape-model fit, in [0, 1] (default 0: the free spline; "
                    "1 cannot wobble)")
    ap.add_argument("--shape-model", default=None, choices=["affine", "similarity", "translation"],
                    help="the rigid motion --rigidity pulls towards (default: affine)")
    ap.add_argument("--out-size", default=None, metavar="WxH",
                    help="render every output at this size (even, at most 4x smaller than its input per axis) with an area "
                         "filter, instead of at the input's size")
    ap.add_argument("--scene-cut", type=float, default=None, metavar="THR")
    ap.add_argument("--scene-min-len", type=int, default=None, metavar="N")
    ap.add_argument("--yuv-matrix", default="auto", choices=["auto", "bt709", "bt601"])
    ap.add_argument("--batch", type=int, default=None, help="streams per step (default: all inputs)")
    ap.add_argument("--depth", type=int, default=3, help="frames in flight per input (1: the serial loop)")
    ap.add_argument("--stats", action="store_true", help="frames, frames/s, final zoom and cuts per input, on stderr")
    return ap


# the header-less formats of --format / --output-format: (reader, writer)
_RAW = {"nv12": (y4m.RawNV12Reader, y4m.RawNV12Writer), "p010": (y4m.RawP010Reader, y4m.RawP010Writer),
        "nv16": (y4m.RawNV16Reader, y4m.RawNV16Writer), "p210": (y4m.RawP210Reader, y4m.RawP210Writer)}
# the C tag of a Y4M output of a raw source
_RAW_COLORSPACE = {"p010": "420p10", "nv16": "422", "p210": "422p10"}


def _size(text, option):
    try:
        w, h = (int(v) for v in text.lower().split("x"))
        if w < 1 or h < 1:
            raise ValueError
    except ValueError:
        raise _UsageError("%s must be WxH, got %r" % (option, text)) from None
    return w, h


def _arguments(argv):
    """Parse and check everything that can be checked without a device or a stream; raises _UsageError."""
    args = _parser().parse_args(argv)
    args.input = args.input or ["-"]
    args.output = args.output or ["-"]
    if len(args.input) != len(args.output):
        raise _UsageError("%d --input but %d --output: give one output per input" % (len(args.input), len(args.output)))
    if args.input.count("-") > 1 or args.output.count("-") > 1:
        raise _UsageError("stdin and stdout can serve one stream each")
    args.output_format = args.output_format or args.format
    args.size = _size(args.size, "--size") if args.size is not None else None
    if args.format in _RAW and args.size is None:
        raise _UsageError("--format %s has no header: --size WxH is required" % args.format)
    args.model_size = _size(args.model_size, "--model-size")
    try:
        args.fps = y4m._as_ratio(args.fps, "--fps")
    except ValueError as e:
        raise _UsageError(str(e)) from None
    try:
        args.skip_length = tuple(int(v) for v in args.skip_length.split(",")) if args.skip_length else None
    except ValueError:
        raise _UsageError("--skip-length takes integers A,B,..., got %r" % args.skip_length) from None
    try:
        args.crop = args.crop if args.crop in (None, "auto") else float(args.crop)
    except ValueError:
        raise _UsageError("--crop takes 'auto' or a zoom in (0, 1], got %r" % args.crop) from None
    if args.out_size is not None:
        from .networks import check_out_size
        ow, oh = _size(args.out_size, "--out-size")
        if args.border == "keep":
            raise _UsageError("--border keep has no --out-size: the kept surface has no counterpart at another size")
        try:
            args.out_size = check_out_size((oh, ow), True, True)
        except ValueError as e:
            raise _UsageError("--out-size %s: %s" % (args.out_size, e)) from None
    if args.depth < 1 or (args.batch is not None and args.batch < 1):
        raise _UsageError("--depth and --batch must be at least 1")
    return args


def _run(args, note):
    from .clip import SKIP_LENGTH
    from .model import StabNet
    from . import weights as _weights
    files = []
    stdout = None
    try:
        sources = []
        for path in args.input:
            f = sys.stdin.buffer if path == "-" else open(path, "rb")
            files.append(f)
            sources.append(y4m.Y4MReader(f, depths=(8, 10), chromas=("420", "422")) if args.format == "y4m" else
                           _RAW[args.format][0](f, *args.size))
        for path, src in zip(args.input, sources):
            if any(t.upper() == "XCOLORRANGE=FULL" for t in src.tags):
                note("%s: full-range video goes through unchanged; the CNN sees it through a limited-range matrix" % path)
        skip = args.skip_length or SKIP_LENGTH
        S = len(skip)
        if args.synthetic_weights:
            note("--synthetic-weights: a seeded test checkpoint, not a trained model")
            weights = _weights.make_synthetic_weights(seed=0, c_in=3 * S)
        elif args.ckpt:
            weights = _weights.load_ckpt_dir(args.ckpt)
        else:
            weights = _weights.load_npz(args.npz)
        w, h = args.model_size
        model = StabNet(h, w).load_weights(weights)
        model.get_evaluation_model(S)
        model.precision = args.precision
        kw = dict(skip_length=skip, yuv_matrix=args.yuv_matrix)
        for key in ("crop", "crop_min", "crop_margin", "crop_recover", "scene_cut", "scene_min_len", "render_filter", "border",
                    "strength", "rigidity", "shape_model", "out_size"):
            if getattr(args, key) is not None:
                kw[key] = getattr(args, key)
        sinks = []
        for path, src in zip(args.output, sources):
            if path == "-":
                f = stdout = sys.stdout.buffer
                sys.stdout = sys.stderr     # nothing but video goes to the real stdout
            else:
                f = open(path, "wb")
            files.append(f)
            out_h, out_w = args.out_size or (src.height, src.width)
            if args.output_format in _RAW:
                sinks.append(_RAW[args.output_format][1](f, out_w, out_h))
            else:   # a Y4M header repeats the source's C tag (C420p10, C422, C422p10 for a raw P010, NV16, P210 source) and its X tags
                sinks.append(y4m.Y4MWriter(f, out_w, out_h, src.fps or args.fps,
                                           aspect=output_aspect(src.aspect, (src.height, src.width), (out_h, out_w)),
                                           colorspace=_RAW_COLORSPACE.get(src.layout, src.colorspace), tags=src.tags,
                                           interlace=src.interlace, chromas=("420", "422")))
        stats = stabilize_pipes(model, sources, sinks, batch=args.batch, depth=args.depth, **kw)
        if args.stats:
            for path, st in zip(args.input, stats):
                line = "%s: %d frames, %.1f frames/s" % (path, st["frames"], st["frames"] / max(st["seconds"], 1e-9))
                if st["zoom"] is not None:
                    line += ", zoom %.4f" % st["zoom"]
                if st["cuts"] is not None:
                    line += ", %d cut(s)" % st["cuts"]
                note(line)
    finally:
        for f in files:
            try:
                if f is stdout:
                    f.flush()
                elif f is not sys.stdin.buffer:
                    f.close()
            except OSError:
                pass
    return 0


def main(argv=None):
    """The front end; returns the exit status.  A bad option, a malformed or truncated stream, a missing file or checkpoint
    and a checkpoint of another window length end with status 1 and one line on stderr."""
    from ._lib import DvsgError

    def note(text):
        sys.stderr.write("%s: %s\n" % (PROG, " ".join(str(text).split())))
        sys.stderr.flush()
    try:
        return _run(_arguments(argv), note)
    except _UsageError as e:
        note("error: %s" % e)
    except (ValueError, OSError, DvsgError) as e:
        note("error: %s" % (e,))
    return 1


if __name__ == "__main__":
    sys.exit(main())
