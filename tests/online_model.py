"""An unbounded-history model of `coupe.dvsg_amd.online.OnlineStabilizer`, and the schedules that drive both.

The product keeps every stream in a RING of 34 pool slots, hands rings from closed streams to new ones, keeps per-ring state on
the device and lets a kernel write the step table.  The model keeps none of that: every stream owns a Python list that is
eval.py:93-124's `total_frames` restated literally (`History`), a scene state machine written out in a few lines
(`SceneState`), a NumPy zoom state for `ratchet_ref.ratchet` and its own border="keep" surface.  One step gathers the fed
rows' windows from a scratch pool filled from those lists (`dvsg_window_gather_f32`) and runs ONE non-ring
`LocNet.stabilize` call at the same B and in the batch order `OnlineStabilizer.step` documents, so the CNN's float32
association is the product's (tests/test_gpu_ring.py::test_stabilize_ring_is_gather_plus_stabilize,
tests/test_gpu_online.py::test_inplace_ring_is_the_contiguous_ring) and every output must match BIT FOR BIT at every step.
What differs between the two is the bookkeeping, which is the subject.

Nothing here imports `coupe.dvsg_amd.online`: no `stream_window_row`, no slot, count or state rule of the product.  Ingest
and egress go through the plain C entry points the fused ones are pinned against (tests/test_gpu_online.py,
tests/test_gpu_nv12.py), one row (n = 1) at a time.  frame_format="p010": the network sees the NV12 surface of word >> 8,
computed on the words, through the NV12 ingest; the render is one n = 1 call through `LocNet.view(..., surface="p010")` at
pitch 2 W0; a frame that came as 16-bit words leaves as such.

`make_schedule(name)` / `coverage(schedule)`: deterministic schedules of open / close / reset / feed events with a content
of its own for every stream, and the facts tests/test_online_model_cpu.py asserts about them so that a later edit cannot
silently lose a case."""
import ctypes

import numpy as np

import inputs
import ratchet_ref
import scene_ref

F32 = np.float32
SKIP = (0, 16, 24, 28, 30, 31, 32)        # config.py:48
THRESHOLD = scene_ref.THRESHOLD           # 0.75
MIN_LEN = 3                               # scene_min_len of every scene schedule
MODEL_H, MODEL_W = 32, 48
YUV_MATRICES = {"bt601": 0, "bt709": 1}
FILTERS = ("bilinear", "bicubic")
BORDERS = ("black", "replicate", "mirror", "keep")


# ---------------------------------------------------------------------------------------------------------------------
# the history of one stream: eval.py:93-124's list
# ---------------------------------------------------------------------------------------------------------------------
class History(object):
    """eval.py's `total_frames` of one stream, one frame at a time.  `window(frame)` is :93-94 (on a run's first frame) or the
    clip's next frame appended, then :103; `write_back(result)` is :116-120 and moves on to the next step.  Entries that no
    later window can read (index < k) are dropped; the list is never a ring.  Items are opaque: device tensors in the
    model, integer labels in the CPU test."""

    def __init__(self, skip=SKIP):
        self.skip = tuple(int(s) for s in skip)
        self.span = self.skip[-1]
        self.restart()

    def restart(self):
        self.total, self.k, self.dropped = [], 0, 0

    def window(self, frame):
        if self.k == 0:
            self.total = [frame] * self.span + [frame]            # 32 copies of the unstable frame plus that frame itself
            self.dropped = 0
        else:
            self.total.append(frame)                              # total[k + 32]: the unstable frame of step k
        return [self.total[self.k + s - self.dropped] for s in self.skip]

    def write_back(self, result):
        self.total[self.k + self.span - self.dropped] = result    # :116
        if self.k == 0:
            for i in range(self.span):                            # :118-120
                self.total[i] = result
        self.k += 1
        del self.total[:self.k - self.dropped]                    # step k' >= k reads total[k' + skip] only
        self.dropped = self.k


class SceneState(object):
    """The scene-cut decision of one stream (include/dvsg_amd.h, "ONLINE streams, SCENE CUTS"): k frames since the last start,
    the cuts so far, the last S and the previous histogram.  A cut iff k >= max(1, min_len) and S >= thr_count."""

    def __init__(self, thr_count, min_len):
        self.thr_count, self.min_len = int(thr_count), int(min_len)
        self.restart()

    def restart(self):
        self.k, self.cuts, self.S, self.prev = 0, 0, 0, None

    def step(self, hist):
        """hist: the 64-bin histogram of the stream's current frame -> True when this frame is a cut"""
        S = 0 if self.k == 0 else scene_ref.distance(hist, self.prev)
        cut = self.k >= max(1, self.min_len) and S >= self.thr_count
        if cut:
            self.k = 0
            self.cuts += 1
        self.k, self.S, self.prev = self.k + 1, S, hist
        return cut


class _Stream(object):
    def __init__(self, skip):
        self.hist = History(skip)
        self.scene = None
        self.zoom = None      # crop="auto": float32 [1], the state ratchet_ref.ratchet updates
        self.free = None
        self.keep = None      # border="keep": the stream's own surface
        self.fresh = True     # the surface restarts from the next frame's source


class _Row(object):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
class UnboundedStreams(object):
    """The surface of OnlineStabilizer the tests need -- open, close, reset, step, push, crop_state, scene_state -- with the same
    constructor options.  `cut_log` collects (step number, sid) of every detected cut, `k_of(sid)` is a stream's next step."""

    def __init__(self, model, max_streams=1, skip_length=SKIP, channel_order="rgb", side_by_side=False, as_uint8=False,
                 source_res=False, frame_format="rgb", yuv_matrix="bt709", crop=None, crop_margin=None, crop_min=0.5,
                 crop_start=1.0, crop_recover=0.0, scene_cut=None, scene_min_len=1, render_filter="bilinear", border="black",
                 strength=1.0, rigidity=0.0, shape_model="affine"):
        assert channel_order in ("rgb", "bgr") and frame_format in ("rgb", "nv12", "p010")
        assert render_filter in FILTERS and border in BORDERS
        self.model, self.net = model, model.locnet
        self.h, self.w = model.h, model.w
        self.max_streams = int(max_streams)
        self.skip = tuple(int(s) for s in skip_length)
        self.flip = 1 if channel_order == "bgr" else 0
        self.p010 = frame_format == "p010"              # 10-bit surfaces: the network sees the NV12 surface of word >> 8
        self.nv12 = frame_format in ("nv12", "p010")    # two planes, a source-size render
        self.matrix = YUV_MATRICES[yuv_matrix]
        self.side_by_side, self.as_uint8 = bool(side_by_side), bool(as_uint8)
        self.source_res = bool(source_res) or self.nv12
        self.crop = None if crop is None else (crop if isinstance(crop, str) else F32(crop))
        self.crop_auto = isinstance(crop, str)
        self.crop_margin = None if crop_margin is None else float(crop_margin)
        self.crop_min, self.crop_start, self.crop_recover = float(crop_min), float(crop_start), float(crop_recover)
        self.scene_thr = None if scene_cut is None else \
            int(np.ceil(np.float64(scene_cut) * np.float64(2 * self.h * self.w)))
        self.scene_min_len = int(scene_min_len)
        self.view_args = (render_filter, border, strength, rigidity, shape_model)
        self.keep = border == "keep"
        self._streams = {}
        self._next_sid = 0
        self.steps = 0
        self.cut_log = []

    # ---- streams
    def open(self):
        if len(self._streams) >= self.max_streams:
            raise RuntimeError("all %d streams are open" % self.max_streams)
        sid = self._next_sid
        self._next_sid += 1
        st = self._streams[sid] = _Stream(self.skip)
        if self.scene_thr is not None:
            st.scene = SceneState(self.scene_thr, self.scene_min_len)
        self._restart(st)
        return sid

    def _restart(self, st):
        """The next frame of the stream is step 0: history, zoom and surface start over (open, reset and a cut alike)."""
        st.hist.restart()
        if self.crop_auto:
            st.zoom = np.array([self.crop_start], dtype=F32)
        st.fresh = True

    def reset(self, sid):
        st = self._streams[sid]
        self._restart(st)
        st.free = None
        if st.scene is not None:
            st.scene.restart()

    def close(self, sid):
        del self._streams[sid]

    @property
    def open_streams(self):
        return sorted(self._streams)

    def k_of(self, sid):
        return self._streams[sid].hist.k

    def crop_state(self, sid):
        st = self._streams[sid]
        if self.crop is None:
            raise ValueError("made without crop")
        return dict(zoom=F32(st.zoom[0]) if self.crop_auto else F32(self.crop), free=st.free)

    def scene_state(self, sid):
        st = self._streams[sid]
        if st.scene is None:
            raise ValueError("made without scene_cut")
        return dict(frames_since_cut=st.scene.k, cuts=st.scene.cuts, score=st.scene.S / float(2 * self.h * self.w))

    def push(self, sid, frame):
        return self.step({sid: frame})[sid]

    # ---- one step
    def step(self, frames):
        import torch
        from coupe.dvsg_amd import _lib
        self.steps += 1
        if not frames:
            return {}
        h, w = self.h, self.w
        rows = []
        for sid, fr in frames.items():
            r = _Row()
            r.sid, r.st = sid, self._streams[sid]
            r.host = not isinstance(fr, torch.Tensor)
            r.words = False
            if self.p010:
                fr = self._p010(r, fr)
            r.t = (torch.as_tensor(np.ascontiguousarray(fr)) if r.host else fr).cuda().contiguous()
            if self.nv12:
                assert r.t.dtype == torch.uint8 and r.t.dim() == 2
                r.key = (2 * int(r.t.shape[0]) // 3, int(r.t.shape[1]))
            elif r.t.dtype == torch.uint8:
                r.key = (0, int(r.t.shape[0]), int(r.t.shape[1])) if tuple(r.t.shape[:2]) != (h, w) else (1,)
            else:
                assert tuple(r.t.shape) == (h, w, 3) and not self.source_res
                r.key = (3,) if r.t.dtype == torch.float64 else (2,)
            rows.append(r)
        # the documented batch order: resized uint8 grouped by source size, same-size uint8, float32, float64 (NV12: by
        # source size); stable in feed order within a group
        rows.sort(key=lambda r: r.key)
        B = len(rows)
        for r in rows:
            self._ingest(r)
        if self.scene_thr is not None:
            for r in rows:                                        # a cut is a reset of that stream before its row is gathered
                if r.st.scene.step(scene_ref.histogram(r.u.cpu().numpy())):
                    self._restart(r.st)
                    self.cut_log.append((self.steps - 1, r.sid))
        windows = [r.st.hist.window(r.u) for r in rows]
        S = len(self.skip)
        pool = torch.stack([f for win in windows for f in win])   # the scratch pool of this step
        table = torch.arange(B * S, dtype=torch.int32, device=pool.device).view(B, S)
        x = torch.empty((B, h, w, 3 * S), dtype=torch.float32, device=pool.device)
        _lib.call("dvsg_window_gather_f32", pool.data_ptr(), B * S, h, w, table.data_ptr(), B, S, x.data_ptr(), _stream())
        u = torch.stack([r.u for r in rows])
        out = torch.empty((B, h, w, 3), dtype=torch.float32, device=pool.device)
        F = torch.empty((B, self.model.param_dim, 2), dtype=torch.float32, device=pool.device)
        self.net.stabilize(x, u, out, F, precision=self.model.precision)
        res = {}
        for b, r in enumerate(rows):
            r.st.hist.write_back(out[b].clone())                  # the history keeps the uncropped model-size frame
            o = self._egress(r, out[b:b + 1], F[b:b + 1].contiguous())
            if r.host:
                o = tuple(p.cpu().numpy() for p in o) if isinstance(o, tuple) else o.cpu().numpy()
            if r.words:                                           # a frame that came as 16-bit words leaves as such
                o = o.view(np.uint16) if r.host else o.view(torch.uint16)
            res[r.sid] = o
        return {sid: res[sid] for sid in frames}

    def _p010(self, r, fr):
        """A P010 frame -- uint8 [3 H0 / 2, 2 W0], the words' bytes, or uint16 [3 H0 / 2, W0], host or device: r.p010 keeps its
        bytes on the device for the render, r.words whether it came as words; returns the NV12 surface the network sees,
        uint8 [3 H0 / 2, W0] = word >> 8, computed on the words."""
        import torch
        a = fr.cpu().numpy() if isinstance(fr, torch.Tensor) else np.ascontiguousarray(fr)
        r.words = a.dtype == np.uint16
        assert a.dtype in (np.uint8, np.uint16) and a.ndim == 2 and np.little_endian
        words = a if r.words else a.view("<u2")
        r.p010 = torch.from_numpy(words.view(np.uint8).copy()).cuda()
        hi = (words >> np.uint16(8)).astype(np.uint8)
        return hi if r.host else torch.from_numpy(hi).cuda()

    def _ingest(self, r):
        """r.u: the unstable frame at the model's size, float32 [h,w,3] RGB; r.src: the uint8 source [1,H0,W0,3] (NV12:
        [1,3 H0/2,W0]); r.left: the unstable half of a model-size side_by_side frame."""
        import torch
        from coupe.dvsg_amd import _lib
        h, w, t = self.h, self.w, r.t
        dev = t.device
        r.src = r.left = None
        flip = self.flip
        want_left = self.side_by_side and not self.source_res
        left = torch.empty((1, h, 2 * w, 3), dtype=torch.uint8, device=dev) if want_left else None
        if self.nv12:
            H0, W0 = r.key
            nv = t.unsqueeze(0)
            r.src = r.p010.unsqueeze(0) if self.p010 else nv    # what the render warps
            rgb = torch.empty((1, H0, W0, 3), dtype=torch.uint8, device=dev)
            _lib.call("dvsg_frames_nv12_to_rgb_u8", nv.data_ptr(), nv.data_ptr() + H0 * W0, W0, 3 * H0 // 2 * W0, 1, H0, W0,
                      self.matrix, 0, rgb.data_ptr(), _stream())
            t, flip = rgb[0], 0                                   # convert, then the RGB path
        if t.dtype == torch.uint8:
            H0, W0 = int(t.shape[0]), int(t.shape[1])
            if not self.nv12:
                r.src = t.unsqueeze(0)
            r.u = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            if (H0, W0) == (h, w):
                _lib.call("dvsg_frames_u8_to_f32", t.data_ptr(), h * w, flip, r.u.data_ptr(), _stream())
            else:
                _lib.call("dvsg_frames_resize_u8_f32", t.data_ptr(), 1, H0, W0, flip, r.u.data_ptr(), h, w,
                          left.data_ptr() if left is not None else 0, 2 * w, 0, _stream())
                r.left = left
        elif t.dtype == torch.float64:
            r.u = t.to(torch.float32)                             # one rounding
            if want_left:
                _lib.call("dvsg_frames_f64_to_u8", t.data_ptr(), 1, h, w, flip, left.data_ptr(), 2 * w, 0, _stream())
                r.left = left
        else:
            r.u = t.clone()
        if want_left and r.left is None:                          # the float32 frame holds the unstable frame exactly
            _lib.call("dvsg_frames_f32_to_u8", r.u.data_ptr(), 1, h, w, flip, left.data_ptr(), 2 * w, 0, _stream())
            r.left = left

    def _zoom(self, r, F, T, grids):
        """crop -> float32 [1] on the device (None without crop); T [1,2,28] is written with crop="auto"."""
        import torch
        from coupe.dvsg_amd import _lib
        if self.crop is None:
            return None
        if not self.crop_auto:
            return torch.full((1,), float(self.crop), dtype=torch.float32, device=F.device)
        view = self.net.view(*self.view_args)
        keys, D = [], []
        for gh, gw in grids:
            need = ctypes.c_size_t()
            _lib.call("dvsg_tps_coverage_workspace_bytes", 1, gh, gw, ctypes.byref(need))
            ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=F.device)
            res = torch.empty((2, 1), dtype=torch.int32, device=F.device)
            _lib.call("dvsg_tps_coverage_net_f32", view, F.data_ptr(), None, 1, gh, gw, gh, gw, T.data_ptr(), res[0].data_ptr(),
                      res[1].data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream())
            keys.append(res[1].cpu().numpy())
            D.append((gh - 1) * (gw - 1))
        margin = 2.0 / (min(grids[-1]) - 1) if self.crop_margin is None else self.crop_margin
        two = len(grids) > 1
        zoom, free, _ = ratchet_ref.ratchet(r.st.zoom, [0], keys[0], D[0], keys[1] if two else None, D[1] if two else 0,
                                            margin, self.crop_min, self.crop_recover)
        r.st.free = float(free[0])
        return torch.from_numpy(zoom.copy()).to(F.device)

    def _surface(self, r, first):
        """border="keep": the stream's own surface, restarted from `first` where due; without it a fresh tensor."""
        import torch
        if not self.keep:
            return torch.empty_like(first)
        st = r.st
        if st.keep is None or st.fresh or st.keep.shape != first.shape or st.keep.dtype != first.dtype:
            st.keep = first.clone()
            st.fresh = False
        return st.keep

    def _egress(self, r, s, F):
        """s [1,h,w,3]: the stabilised model-size frame of row r, F [1,25,2] its F_t -> the stream's output."""
        import torch
        from coupe.dvsg_amd import _lib
        h, w, flip, dev = self.h, self.w, self.flip, s.device
        T = torch.empty((1, 2, self.model.param_dim + 3), dtype=torch.float32, device=dev)
        view = self.net.view(*self.view_args)
        if self.nv12:
            H0, W0 = r.key
            src = r.src
            zoom = self._zoom(r, F, T, [(H0, W0), (H0 // 2, W0 // 2)])
            out = self._surface(r, src)
            pitch = 2 * W0 if self.p010 else W0                   # rows are packed; P010: one n = 1 call through a P010 view
            if self.p010:
                assert tuple(src.shape) == (1, 3 * H0 // 2, pitch) and src.dtype == torch.uint8
                view = self.net.view(*self.view_args, surface="p010")
            args = (r.src.data_ptr(), r.src.data_ptr() + H0 * pitch, pitch, 3 * H0 // 2 * pitch, 1, H0, W0)
            tail = (T.data_ptr(), out.data_ptr(), out.data_ptr() + H0 * pitch, pitch, 3 * H0 // 2 * pitch, _stream())
            if zoom is None:
                _lib.call("dvsg_tps_render_nv12", view, F.data_ptr(), *(args + tail))
            else:
                _lib.call("dvsg_tps_render_zoom_nv12", view, F.data_ptr(), *(args + (zoom.data_ptr(),) + tail))
            return out[0].clone()
        if self.source_res:
            src = r.src
            H0, W0 = int(src.shape[1]), int(src.shape[2])
            zoom = self._zoom(r, F, T, [(H0, W0)])
            first = src
            if not self.as_uint8:
                first = torch.empty((1, H0, W0, 3), dtype=torch.float32, device=dev)
                if self.keep:
                    _lib.call("dvsg_frames_u8_to_f32", src.data_ptr(), H0 * W0, flip, first.data_ptr(), _stream())
            out = self._surface(r, first)
            side = None
            if self.side_by_side:
                side = torch.empty((1, H0, 2 * W0, 3), dtype=torch.uint8, device=dev)
                side[:, :, :W0] = src                             # the unstable half is the source bytes
            if self.as_uint8:
                f32, u8, u8_W, u8_x0 = None, out, W0, 0
            else:
                f32, u8, u8_W, u8_x0 = out, side, 2 * W0, W0
            p = lambda a: 0 if a is None else a.data_ptr()
            if zoom is None:
                _lib.call("dvsg_tps_render_u8", view, F.data_ptr(), src.data_ptr(), 1, H0, W0, flip, T.data_ptr(), p(f32), p(u8),
                          u8_W, u8_x0, _stream())
            else:
                _lib.call("dvsg_tps_render_zoom_u8", view, F.data_ptr(), src.data_ptr(), 1, H0, W0, flip, zoom.data_ptr(),
                          T.data_ptr(), p(f32), p(u8), u8_W, u8_x0, _stream())
            if side is not None and self.as_uint8:
                side[:, :, W0:] = out
            o = out[0].clone()
            return (o, side[0]) if self.side_by_side else o
        # ---- the model's size
        stab = s
        if self.crop is not None:
            from coupe.dvsg_amd.model import V_SRC
            zoom = self._zoom(r, F, T, [(h, w)])
            if not self.crop_auto:
                _lib.call("dvsg_tps_coefficients_f32", view, F.data_ptr(), 1, T.data_ptr(), _stream())
            V = torch.from_numpy(np.ascontiguousarray(V_SRC, dtype=F32)).to(dev).unsqueeze(0).contiguous()
            stab = torch.empty_like(s)
            u = r.u.unsqueeze(0).contiguous()
            _lib.call("dvsg_tps_warp_zoom_f32", u.data_ptr(), V.data_ptr(), T.data_ptr(), zoom.data_ptr(), 1, h, w, 3,
                      self.model.param_dim, h, w, stab.data_ptr(), None, None, _stream())
        o = stab[0]
        if self.as_uint8:
            o8 = torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev)
            _lib.call("dvsg_frames_f32_to_u8", stab.data_ptr(), 1, h, w, flip, o8.data_ptr(), w, 0, _stream())
            o = o8[0]
        if self.side_by_side:
            _lib.call("dvsg_frames_f32_to_u8", stab.data_ptr(), 1, h, w, flip, r.left.data_ptr(), 2 * w, w, _stream())
            return o, r.left[0]
        return o


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_clips(streams, clips, batch):
    """K whole clips through `streams` (an UnboundedStreams of `batch` streams) in lockstep: as many clips as there are free
    streams start, every running clip is fed its next frame each step, and a finished clip's place goes to the next waiting
    clip before the next step.  Returns, per clip, the list of its outputs."""
    outs = [[] for _ in clips]
    waiting, active = list(range(len(clips))), {}
    while waiting or active:
        while waiting and len(active) < batch:
            active[streams.open()] = [waiting.pop(0), 0]
        res = streams.step({sid: clips[c][k] for sid, (c, k) in active.items()})
        for sid, o in res.items():
            c = active[sid][0]
            outs[c].append(o)
            active[sid][1] += 1
            if active[sid][1] == len(clips[c]):
                streams.close(sid)
                del active[sid]
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------------------------------------------------
N_STEPS = 90
MAX_STREAMS = 3
SIZES = {"u8a": (45, 70), "u8b": (40, 64), "u8s": (MODEL_H, MODEL_W), "nva": (40, 48), "nvb": (36, 64), "pa": (40, 48),
         "pb": (36, 64)}

# name -> (opened before step, closed before step or None, steps it is open in but NOT fed, resets before steps,
#          planted scene changes at these frame numbers of the stream)
_SKELETON = {
    "a": (0, 76, (7, 20, 50, 61, 63), (), (12, 50)),            # 71 frames: a ring wraps twice; a cut at k = 38
    "b": (0, None, (3, 30, 31, 61, 64, 80), (6, 50), (12, 47, 49, 66)),
    "c": (0, 2, (0,), (), ()),                                  # opened and not fed; one frame; closed before step 2 ...
    "d": (2, 31, (10,), (), (15,)),                             # ... where d takes its ring
    "e": (32, 61, (45,), (), ()),
    "g": (62, None, (70,), (), (10,)),
    "f": (76, None, (85,), (), ()),                             # takes a's ring
}
# the kinds of the streams per schedule; the feed order of a step is the order of this table, which is NOT the batch order
_KINDS = {
    "rgb": {"b": "f32", "a": "u8a", "c": "f32", "d": "u8b", "e": "u8s", "f": "u8s", "g": "f64"},
    "source_res": {"a": "u8a", "b": "u8b", "c": "u8a", "d": "u8b", "e": "u8a", "f": "u8b", "g": "u8b"},
    "nv12": {"a": "nva", "b": "nvb", "c": "nvb", "d": "nva", "e": "nvb", "f": "nvb", "g": "nva"},
    "model_size": {"b": "f32", "a": "f32", "c": "f32", "d": "f64", "e": "f32", "f": "f64", "g": "f32"},
    # a is left out of step 50 while b and e (one size) are fed: the other size is gone for a step and comes back
    "p010": {"a": "pa", "b": "pb", "c": "pb", "d": "pa", "e": "pb", "f": "pb", "g": "pa"},
}
_FEED_ORDER = {"rgb": "fgbadce", "source_res": "abcdefg", "nv12": "abcdefg", "model_size": "gfbadce", "p010": "abcdefg"}
_HOST = {"rgb": "acdfg", "source_res": "bdf", "nv12": "a", "model_size": "adg", "p010": "ad"}   # NumPy in; the others device tensors
# the form a P010 stream's frames arrive in: 16-bit words or their bytes, from the host or on the device ("dev_u16" only
# where the installed torch has torch.uint16; the other streams are "dev_u8")
_P010_FORMS = {"a": "host_u16", "d": "host_u8", "b": "dev_u16"}


def _has_torch_uint16():
    try:
        import torch
    except ImportError:
        return False
    return hasattr(torch, "uint16")
_SEED = {n: 5100 + 7 * i for i, n in enumerate("abcdefg")}


class Schedule(list):
    """A list of steps, each a list of events ("open" | "close" | "reset" | "feed", stream name), with the streams' content
    specs in `.streams`, whether the schedule is run with scene cuts in `.scene` and its name."""


def make_schedule(name):
    assert name in _KINDS, name
    sched = Schedule([] for _ in range(N_STEPS))
    sched.name, sched.scene, sched.max_streams = name, name != "rgb", MAX_STREAMS
    sched.streams = {}
    order = _FEED_ORDER[name]
    for n in sorted(_SKELETON, key=lambda n: (_SKELETON[n][0], n)):
        first, last, _, resets, _ = _SKELETON[n]
        if last is not None:
            sched[last].append(("close", n))
    for n in sorted(_SKELETON, key=lambda n: (_SKELETON[n][0], n)):
        first, last, _, resets, _ = _SKELETON[n]
        sched[first].append(("open", n))
        for t in resets:
            sched[t].append(("reset", n))
    for n in order:
        first, last, out, resets, planted = _SKELETON[n]
        fed = [t for t in range(first, N_STEPS if last is None else last) if t not in out]
        for t in fed:
            sched[t].append(("feed", n))
        scenes, cur = [], 0
        for j in range(len(fed)):
            cur ^= int(j in planted)
            scenes.append(cur)
        sched.streams[n] = dict(kind=_KINDS[name][n], seed=_SEED[n], n=len(fed), scenes=scenes, host=n in _HOST[name])
        if name == "p010":
            form = _P010_FORMS.get(n, "dev_u8")
            if form == "dev_u16" and not _has_torch_uint16():
                form = "dev_u8"
            assert form.startswith("host") == (n in _HOST[name])
            sched.streams[n]["form"] = form
    return sched


def _levels(seed, n, H, W, scenes, C=3):
    """Scene 0's values in [0.05, 0.45], scene 1's in [0.55, 0.95] (scene_ref.scene_a / scene_b): no histogram bin is shared."""
    lo = np.where(np.asarray(scenes) == 0, F32(0.05), F32(0.55)).astype(F32).reshape(-1, 1, 1, 1)
    return (lo + F32(0.4) * inputs.smooth_frames(seed, n, H, W, C=C)).astype(F32)


def stream_frames(spec):
    """The frames of one stream, a NumPy array [n, ...], from its own seed at its own size."""
    kind, seed, n, scenes = spec["kind"], spec["seed"], spec["n"], spec["scenes"]
    if kind == "f32":
        return _levels(seed, n, MODEL_H, MODEL_W, scenes)
    if kind == "f64":
        # values float32 does not hold: np.uint8(v * 255.) of the float64 and of the rounded float32 differ in about half the
        # bytes, so the unstable half of side_by_side shows which of the two it was rendered from
        q = np.floor(_levels(seed, n, MODEL_H, MODEL_W, scenes).astype(np.float64) * 254.0)
        return (q + (1.0 - 2.0 ** -30)) / 255.0
    if kind.startswith("u8"):
        H, W = SIZES[kind]
        return np.round(_levels(seed, n, H, W, scenes) * 255).astype(np.uint8)
    H, W = SIZES[kind]
    if kind in ("pa", "pb"):
        # 10-bit codes: luma 64 + 876 level (its high byte is the NV12 schedule's 16 + 219 level, so the two scenes keep
        # disjoint high-byte histograms), chroma around 512; seeded NON-ZERO bits in the low 6 of every word.  uint16 words
        # [n, 3 H / 2, W], or their bytes [n, 3 H / 2, 2 W] for a stream fed in the uint8 form.
        y = np.round(64 + 876 * _levels(seed, n, H, W, scenes, C=1)[..., 0]).astype(np.uint16)
        uv = np.round(512 + 48 * (inputs.smooth_frames(seed + 500, n, H // 2, W // 2, C=2) - 0.5)).astype(np.uint16)
        code = np.concatenate([y, uv.reshape(n, H // 2, W)], axis=1)
        low = np.random.default_rng(seed + 900).integers(1, 64, code.shape, dtype=np.uint16)
        words = ((code << 6) | low).astype("<u2")
        return words.view(np.uint16) if spec.get("form", "host_u16").endswith("u16") else words.view(np.uint8)
    y = np.round(16 + 219 * _levels(seed, n, H, W, scenes, C=1)[..., 0]).astype(np.uint8)
    uv = np.round(128 + 12 * (inputs.smooth_frames(seed + 500, n, H // 2, W // 2, C=2) - 0.5)).astype(np.uint8)
    return np.concatenate([y, uv.reshape(n, H // 2, W)], axis=1)


def coverage(sched):
    """The facts about a schedule that the CPU test asserts.  k is a stream's frames since its last start: open, reset or --
    in a scene schedule -- a planted cut that fires (k >= MIN_LEN frames after the last start; a planted change before that
    is suppressed, and on a start's own frame there is nothing to compare with)."""
    open_, frames, k, ever = {}, {}, {}, {}
    just_reset = set()
    facts = dict(longest=0, reuse_after_long=False, reuse_after_one_frame=False, close_and_open_before_one_step=False,
                 left_out=set(), streams=set(), opened_not_fed=False, empty_step=False, batch_sizes=set(), reset_k=[],
                 max_groups=0, max_sizes=0, cut_alone=False, two_cuts=False, suppressed=0, cut_k=[], planted_after_reset=0,
                 max_open=0, cuts=[], forms=set(), shared_launch=False, size_returns=False)
    before, gone = set(), False      # the source sizes of the last step that fed something; a size it had is missing now
    freed = []                       # frames of the closed streams whose place nobody has taken yet, oldest first
    for t, events in enumerate(sched):
        fed, opened, closed_now = [], [], False
        for what, n in events:
            if what == "open":
                assert n not in ever
                open_[n], frames[n], k[n], ever[n] = True, 0, 0, True
                opened.append(n)
                if freed:            # the lowest free ring goes first; with one free ring at a time this is that ring
                    assert len(freed) == 1
                    last = freed.pop(0)
                    facts["reuse_after_long"] |= last >= 70
                    facts["reuse_after_one_frame"] |= last == 1
                    facts["close_and_open_before_one_step"] |= closed_now
            elif what == "close":
                del open_[n]
                freed.append(frames[n])
                closed_now = True
            elif what == "reset":
                facts["reset_k"].append(k[n])
                k[n] = 0
                just_reset.add(n)
            else:
                assert what == "feed" and n in open_ and n not in fed
                fed.append(n)
        facts["max_open"] = max(facts["max_open"], len(open_))
        facts["streams"] |= set(open_)
        facts["empty_step"] |= not fed
        if fed:
            facts["batch_sizes"].add(len(fed))
            facts["left_out"] |= set(open_) - set(fed)
            facts["opened_not_fed"] |= bool(set(opened) - set(fed))
            kinds = [sched.streams[n]["kind"] for n in fed]
            facts["max_groups"] = max(facts["max_groups"], len(set(kinds)))
            sized = [SIZES[c] for c in kinds if c in SIZES and c != "u8s"]
            facts["max_sizes"] = max(facts["max_sizes"], len(set(sized)))
            facts["forms"] |= set(sched.streams[n].get("form") for n in fed)
            facts["shared_launch"] |= len(sized) > len(set(sized))        # two rows of one key: one run, one launch
            now = set(sized)
            facts["size_returns"] |= gone and len(now) >= 2                # ... and a later step feeds both again
            gone |= len(before) >= 2 and len(now) == 1 and now < before    # one of two sizes after a step that fed both ...
            before = now
        cuts = []
        for n in fed:
            j, sc = frames[n], sched.streams[n]["scenes"]
            if sched.scene and j >= 1 and sc[j] != sc[j - 1]:
                if k[n] == 0:
                    facts["planted_after_reset"] += int(n in just_reset)
                elif k[n] < MIN_LEN:
                    facts["suppressed"] += 1
                else:
                    facts["cut_k"].append(k[n])
                    cuts.append(n)
                    k[n] = 0
            frames[n] += 1
            k[n] += 1
            just_reset.discard(n)
            facts["longest"] = max(facts["longest"], frames[n])
        facts["cuts"] += [(t, n) for n in cuts]
        facts["cut_alone"] |= len(cuts) == 1 and len(fed) > 1
        facts["two_cuts"] |= len(cuts) >= 2
    return facts
