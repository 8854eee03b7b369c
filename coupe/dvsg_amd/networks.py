"""Drop-in for the inference part of the reference's networks.py on MI355X.

`scale_RGB(rgb)` (networks.py:6-16) and `localizationNet(input, param_dim, is_train=False,
reuse=False, scope=...) -> [B, param_dim, 2]` (networks.py:30-46).  The reference builds TF
variables under a scope and fills them from a checkpoint through the session; here the
scope maps to a `LocNet` handle created from the same checkpoint arrays
(`load_localizationNet`).  Training (`is_train=True`) and the correlationNet branch are out
of scope.
"""
import ctypes

import numpy as np

from . import _lib, weights as _weights
from ._tensor import as_dev, device, empty, like_input, ptr, stream

_nets = {}


def scale_RGB(rgb):
    """networks.py:6-16 (standalone op; inside localizationNet it is fused into conv1)."""
    t = as_dev(rgb)
    B, H, W, C = t.shape
    out = empty(t.shape, t)
    _lib.call("dvsg_scale_rgb_f32", ptr(t), B, H, W, C, ptr(out), stream())
    return like_input(out, rgb)


def _entry(base, precision):
    """C entry point for a precision: "f32" (exact float32 matrix cores, the reference's arithmetic),
    "f32s" (float32 storage and accumulation, products from two float16 pieces per operand: 22 significant
    bits for |x| >= 2^-3, an absolute step of 2^-24 below -- include/dvsg_amd.h), "f32x3" (float32 tensors and accumulation,
    conv products from three bfloat16 pieces per operand: all 24 bits of both operands at any magnitude) or "f16" (float16
    activations, hi / lo float16 weight pairs)."""
    if precision not in ("f32", "f32s", "f32x3", "f16"):
        raise ValueError("precision must be 'f32', 'f32s', 'f32x3' or 'f16', got %r" % (precision,))
    return "%s_%s" % (base, precision)


RENDER_FILTERS = {"bilinear": 0, "bicubic": 1}     # DVSG_RENDER_BILINEAR, DVSG_RENDER_BICUBIC


def check_render_filter(render_filter, source_size_render=True):
    """render_filter argument -> its name.  "bicubic" where no source-size render happens (RGB at the model's size, float
    frames) is a ValueError that names source_res: only the source-size renders have a filter."""
    if not isinstance(render_filter, str) or render_filter not in RENDER_FILTERS:
        raise ValueError("render_filter must be 'bilinear' or 'bicubic', got %r" % (render_filter,))
    if render_filter != "bilinear" and not source_size_render:
        raise ValueError("render_filter=%r filters the source-size render only: it needs source_res=True (uint8 frames) or "
                         "frame_format='nv12'; frames at the model's size are warped by sampler A" % (render_filter,))
    return render_filter


RENDER_BORDERS = {"black": 0, "replicate": 1, "mirror": 2, "keep": 3}   # DVSG_BORDER_BLACK, _REPLICATE, _MIRROR, _KEEP


def check_border(border, source_size_render=True):
    """border argument -> its name.  Any border but "black" where no source-size render happens (RGB at the model's size,
    float frames) is a ValueError that names source_res: only the source-size renders have a border mode."""
    if not isinstance(border, str) or border not in RENDER_BORDERS:
        raise ValueError("border must be 'black', 'replicate', 'mirror' or 'keep', got %r" % (border,))
    if border != "black" and not source_size_render:
        raise ValueError("border=%r fills the border of the source-size render only: it needs source_res=True (uint8 frames) "
                         "or frame_format='nv12'; frames at the model's size keep sampler A's black border" % (border,))
    return border


SHAPE_MODELS = {"affine": 0, "similarity": 1, "translation": 2}   # DVSG_SHAPE_AFFINE, _SIMILARITY, _TRANSLATION


def check_shape(strength=1.0, rigidity=0.0, shape_model="affine", source_size_render=True):
    """strength, rigidity and shape_model arguments -> (strength, rigidity, shape_model) with the two numbers as the float32
    values the library receives.  Each number must lie in [0, 1] (NaN is refused).  Any shape but the unshaped
    (strength 1, rigidity 0) where no source-size render happens (RGB at the model's size, float frames) is a ValueError that
    names source_res: only what is rendered at source size is shaped, the recurrence never is."""
    if not isinstance(shape_model, str) or shape_model not in SHAPE_MODELS:
        raise ValueError("shape_model must be 'affine', 'similarity' or 'translation', got %r" % (shape_model,))
    out = []
    for name, v in (("strength", strength), ("rigidity", rigidity)):
        if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("%s must be a number in [0, 1], got %r" % (name, v))
        f = float(np.float32(v))
        if not 0.0 <= f <= 1.0:   # (NaN fails both comparisons)
            raise ValueError("%s must be a number in [0, 1], got %r" % (name, v))
        out.append(f)
    if (out[0] != 1.0 or out[1] != 0.0) and not source_size_render:
        raise ValueError("strength=%r, rigidity=%r shape the source-size render only: they need source_res=True (uint8 frames) "
                         "or frame_format='nv12'; frames at the model's size feed the recurrence and stay unshaped"
                         % (strength, rigidity))
    return out[0], out[1], shape_model


SURFACES = {"nv12": 0, "p010": 1}   # DVSG_SURFACE_NV12, DVSG_SURFACE_P010


def check_surface(surface):
    if not isinstance(surface, str) or surface not in SURFACES:
        raise ValueError("surface must be 'nv12' or 'p010', got %r" % (surface,))
    return surface


CHROMAS = {"420": 0, "422": 1}   # DVSG_CHROMA_420, DVSG_CHROMA_422


def check_chroma(chroma):
    if not isinstance(chroma, str) or chroma not in CHROMAS:
        raise ValueError("chroma must be '420' or '422', got %r" % (chroma,))
    return chroma


MAX_SCALED_FACTOR = 4   # virtual samples per axis and output sample that the scaled renders serve


def scaled_factors(source_size, out_size):
    """(H, W), (oh, ow) -> (sy, sx), the supersampling factors of a render at a delivery size: max(1, ceil(H / oh)) and
    max(1, ceil(W / ow)), from the two sizes alone (include/dvsg_amd.h, "Output size").  ValueError above 4: more than 4x
    minification is not served.  Pure: no device."""
    (H, W), (oh, ow) = source_size, out_size
    if min(H, W, oh, ow) < 1:
        raise ValueError("sizes must be positive, got source %r and out_size %r" % (tuple(source_size), tuple(out_size)))
    sy, sx = max(1, -(-int(H) // int(oh))), max(1, -(-int(W) // int(ow)))
    if sy > MAX_SCALED_FACTOR or sx > MAX_SCALED_FACTOR:
        raise ValueError("out_size=%dx%d (H x W) is a %dx%d minification of a %dx%d source; more than %dx is not served"
                         % (oh, ow, sy, sx, H, W, MAX_SCALED_FACTOR))
    return sy, sx


def check_out_size(out_size, source_size_render=True, surface=False):
    """out_size argument -> None or (H, W) as two ints >= 1.  An out_size where no source-size render happens (RGB at the
    model's size, float frames) is a ValueError that names source_res: only the source-size renders have an output size.
    surface: the frames are NV12 / P010, whose planes need even sizes of at least 4."""
    if out_size is None:
        return None
    try:
        ok = len(out_size) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in out_size)
    except TypeError:
        ok = False
    if not ok or min(out_size) < 1:
        raise ValueError("out_size must be (H, W), two integers >= 1, got %r" % (out_size,))
    if not source_size_render:
        raise ValueError("out_size=%r sizes the source-size render only: it needs source_res=True (uint8 frames) or "
                         "frame_format='nv12'; frames at the model's size are warped at that size" % (tuple(out_size),))
    oh, ow = int(out_size[0]), int(out_size[1])
    if surface and (oh % 2 or ow % 2 or oh < 4 or ow < 4):
        raise ValueError("out_size=%r: NV12 / P010 frames are even-sized and at least 4x4" % ((oh, ow),))
    return oh, ow


class LocNet(object):
    """Owns the device-side network (`dvsg_locnet_t`) and one growable workspace per stream that uses it."""

    def __init__(self, weights):
        device()
        # the window length is the checkpoint's own: conv1/weights [7,7,3S,64] fixes the channel count every other array is
        # checked against; which counts load is the library's decision (dvsg_locnet_create: 3 S, S <= 16)
        conv1 = _weights.normalize_names(weights).get(_weights.PREFIX + "resnet_v1_50/conv1/weights")
        w = _weights.validate(weights, int(conv1.shape[2]) if conv1 is not None and conv1.ndim == 4 else 21)
        names = sorted(w)
        n = len(names)
        self._keep = [np.ascontiguousarray(w[k], dtype=np.float32) for k in names]
        c_names = (ctypes.c_char_p * n)(*[k.encode() for k in names])
        c_data = (ctypes.c_void_p * n)(*[a.ctypes.data for a in self._keep])
        c_nd = (ctypes.c_int * n)(*[a.ndim for a in self._keep])
        dims = np.ones((n, 4), dtype=np.int64)
        for i, a in enumerate(self._keep):
            dims[i, :a.ndim] = a.shape
        handle = ctypes.c_void_p()
        _lib.call("dvsg_locnet_create", n, c_names, c_data, c_nd,
                  dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(handle))
        self.handle = handle
        self._views = {}   # (render filter, border, strength, rigidity, shape model, surface[, out_size[, chroma]]) -> view
                           # handle, made on first use (view())
        self._keep = None  # the library copied everything to the device
        self._ws = None
        self.in_channels = _lib.load().dvsg_locnet_in_channels(self.handle)

    def view(self, render_filter="bilinear", border="black", strength=1.0, rigidity=0.0, shape_model="affine", surface="nv12",
             out_size=None, chroma="420"):
        """The handle the source-size renders, the coverage scan and `dvsg_tps_coefficients_f32` take for `render_filter`,
        `border` and the warp shape: this network itself for ("bilinear", "black") unshaped, else a view of it
        (`dvsg_locnet_view_create_border`, or `dvsg_locnet_view_create_shaped` when strength != 1 or rigidity != 0: the same
        network, nothing copied, its own filter, border mode and shape), made once per set of five values and kept until the
        network goes.  An unshaped view is the same whatever its shape_model.  surface="p010": the view of that handle
        whose NV12 renders read and write P010 surfaces (`dvsg_locnet_view_create_surface`: filter, border and shape
        inherited); no other entry point reads it.  out_size=(H, W): the view of THAT handle whose four renders write frames
        of this size (`dvsg_locnet_view_create_scaled`: everything else inherited); no other entry point reads it.  chroma="422": the view of
        THAT handle whose NV12 renders read and write 4:2:2 frames, a UV plane of H rows (`dvsg_locnet_view_create_chroma`:
        everything else inherited; include/dvsg_amd.h, "Chroma sampling"); no other entry point reads it."""
        check_chroma(chroma)
        out_size = check_out_size(out_size)
        check_surface(surface)
        check_render_filter(render_filter)
        check_border(border)
        key = (render_filter, border, strength, rigidity, shape_model)   # as given: what the layers above the base are kept by
        strength, rigidity, shape_model = check_shape(strength, rigidity, shape_model)
        # the base: filter, border and shape by value, on the network itself
        shaped = strength != 1.0 or rigidity != 0.0
        if not shaped:
            shape_model = "affine"
        base = (render_filter, border, strength, rigidity, shape_model, "nv12")   # (these five as the library receives them)
        if shaped:
            v = self._view(base, "dvsg_locnet_view_create_shaped", self.handle, RENDER_FILTERS[render_filter],
                           RENDER_BORDERS[border], SHAPE_MODELS[shape_model], strength, rigidity)
        elif render_filter != "bilinear" or border != "black":
            v = self._view(base, "dvsg_locnet_view_create_border", self.handle, RENDER_FILTERS[render_filter],
                           RENDER_BORDERS[border])
        else:
            v = self.handle
        # then one layer per inherited property, each a view of the handle so far: (value, its default, constructor, arguments)
        for value, default, constructor, args in (
                (surface, "nv12", "dvsg_locnet_view_create_surface", (SURFACES[surface],)),
                (out_size, None, "dvsg_locnet_view_create_scaled", out_size),
                (chroma, "420", "dvsg_locnet_view_create_chroma", (CHROMAS[chroma],))):
            key += (value,)
            if value != default:
                v = self._view(key, constructor, v, *args)
        return v

    def _view(self, key, constructor, *args):
        """The view kept under `key`, made on first use by `constructor(*args, &view)`."""
        v = self._views.get(key)
        if v is None:
            v = ctypes.c_void_p()
            _lib.call(constructor, *(args + (ctypes.byref(v),)))
            self._views[key] = v
        return v

    def __del__(self):
        try:
            for v in getattr(self, "_views", {}).values():   # views first: a parent with views is not destroyed
                _lib.load().dvsg_locnet_destroy(v)
            self._views = {}
            if getattr(self, "handle", None):
                _lib.load().dvsg_locnet_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def workspace(self, B, H, W, slot=0, stream=None):
        """(buffer, bytes needed) for a [B,H,W,c_in] batch.  Buffers are PER STREAM: the C ABI lets calls on distinct streams
        run concurrently only on distinct workspaces (include/dvsg_amd.h, Conventions), so the buffer is keyed by
        (slot, the stream it will be used on) -- `stream`, a torch stream, default the current one -- and two callers that
        share this LocNet under two streams never share scratch.  It is allocated with that stream current, so the caching
        allocator orders a later free behind the work queued there.  The same stream gets the same buffer back (it grows,
        never shrinks); memory grows only for callers that really use several streams."""
        import torch
        need = ctypes.c_size_t()
        _lib.call("dvsg_locnet_workspace_bytes", self.handle, B, H, W, ctypes.byref(need))
        if self._ws is None:
            self._ws = {}
        s = torch.cuda.current_stream() if stream is None else stream
        key = (slot, s.device_index, s.cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need.value:
            self._ws[key] = None
            with torch.cuda.stream(s):
                ws = self._ws[key] = torch.empty(need.value, dtype=torch.uint8, device=device())
        return ws, need.value

    def stabilize(self, patches, u_t, out, F, xs=None, ys=None, n_streams=1, precision="f32", mask=None):
        """`dvsg_stabilize_f32` on device tensors (with `mask` [B,H,W]: `dvsg_stabilize_masked_f32`, eval_train.py's
        graph -- the plane multiplies the 3 (S - 1) history channels inside conv1's load stage), optionally with the batch split over
        `n_streams` side streams: every conv launch covers the chip in a few rounds of tiles and
        its last round is only partly full; launches from two independent half batches fill each
        other's tails (+4 % at B=16 720p before the stream-K tail, <1 % since).  Results do not
        depend on the split beyond float32 re-association (samples are independent); the
        caller's stream sees one fork / join."""
        import torch
        fn = _entry("dvsg_stabilize", precision)
        if u_t.dim() != 4 or u_t.shape[3] != 3:
            raise ValueError("u_t must be [B,H,W,3], got %s" % (tuple(u_t.shape),))
        B, H, W, _ = u_t.shape
        # the C entry point takes no channel count: conv1 reads `in_channels` floats per pixel, so a
        # narrower window (e.g. a 5-entry skip_length) would be read past its end
        if tuple(patches.shape) != (B, H, W, self.in_channels):
            raise ValueError("patches_t must be [%d,%d,%d,%d] (conv1 of the loaded checkpoint has %d input "
                             "channels), got %s" % (B, H, W, self.in_channels, self.in_channels, tuple(patches.shape)))
        if tuple(out.shape) != (B, H, W, 3) or F.numel() != B * 50:
            raise ValueError("out must be [B,H,W,3] and F_t [B,25,2]")
        for name, t, n in (("patches_t", patches, None), ("u_t", u_t, None), ("s_t_pred", out, None), ("F_t", F, None),
                           ("x_s", xs, B * H * W), ("y_s", ys, B * H * W)):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
            if n is not None and t.numel() != n:
                raise ValueError("%s must hold B*H*W = %d values" % (name, n))
        if mask is not None:
            self._check_mask(mask, B, H, W)
            ws, nbytes = self.workspace(B, H, W)
            _lib.call("dvsg_stabilize_masked_f32", self.handle, self._PRECISION_CODE[precision], ptr(patches), ptr(u_t),
                      ptr(mask), B, H, W, ptr(out), ptr(F), ptr(xs), ptr(ys), ptr(ws), nbytes, stream())
            return
        if n_streams <= 1 or B < 2 * n_streams:
            ws, nbytes = self.workspace(B, H, W)
            _lib.call(fn, self.handle, ptr(patches), ptr(u_t), B, H, W, ptr(out), ptr(F),
                      ptr(xs), ptr(ys), ptr(ws), nbytes, stream())
            return
        if getattr(self, "_side", None) is None or len(self._side) != n_streams:
            self._side = [torch.cuda.Stream() for _ in range(n_streams)]
        cur = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(cur)
        per = -(-B // n_streams)
        for i, side in enumerate(self._side):
            b0, b1 = i * per, min(B, (i + 1) * per)
            if b0 >= b1:
                break
            side.wait_event(fork)
            ws, nbytes = self.workspace(b1 - b0, H, W, slot=1 + i, stream=side)
            _lib.call(fn, self.handle, ptr(patches[b0:b1]), ptr(u_t[b0:b1]), b1 - b0, H, W,
                      ptr(out[b0:b1]), ptr(F[b0:b1]), ptr(xs[b0 * H * W:b1 * H * W]) if xs is not None else 0,
                      ptr(ys[b0 * H * W:b1 * H * W]) if ys is not None else 0, ptr(ws), nbytes, side.cuda_stream)
            join = torch.cuda.Event()
            join.record(side)
            cur.wait_event(join)

    _PRECISION_CODE = {"f32": 0, "f16": 1, "f32s": 2, "f32x3": 3}   # DVSG_PRECISION_* of include/dvsg_amd.h

    def _check_ring(self, pool, table):
        import torch
        S = self.in_channels // 3   # the window length is the checkpoint's: conv1 reads table rows of S entries
        if pool.dim() != 4 or pool.shape[3] != 3 or pool.dtype not in (torch.float32, torch.uint8) \
                or not pool.is_cuda or not pool.is_contiguous():
            raise ValueError("pool must be a contiguous [n,H,W,3] float32 or uint8 device tensor")
        if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != S or not table.is_cuda \
                or not table.is_contiguous():
            raise ValueError("table must be a contiguous [B,%d] int32 device tensor (clip.window_index_table; conv1 of the "
                             "loaded checkpoint has %d input channels)" % (S, self.in_channels))
        return int(table.shape[0]), int(pool.shape[1]), int(pool.shape[2])

    @staticmethod
    def _check_mask(mask, B, H, W):
        import torch
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32 or not mask.is_cuda or not mask.is_contiguous() \
                or tuple(mask.shape) != (B, H, W):
            raise ValueError("mask must be a contiguous float32 device tensor [%d,%d,%d] (random_mask_plane)" % (B, H, W))

    def random_mask_plane(self, H_theta, h, w):
        """`dvsg_random_mask_plane_f32`: model.py:156-167 / eval_train.py:53-64's mask for homographies H_theta [B,8]
        (the value after the scale and identity offset of :162-163) as ONE plane [B,h,w] -- the projective warp of an
        all-ones image is the same in each of the 3 (S - 1) history channels."""
        return random_mask_plane(H_theta, h, w)

    def stabilize_ring(self, pool, table, out, F, xs=None, ys=None, precision="f32", mask=None):
        """`dvsg_stabilize_ring_f32` / `_u8`: the evaluation graph on windows assembled inside conv1's load stage
        from the frame pool [n,H,W,3] (float32 in [0,1], or raw uint8) through the index table [B,S],
        S = in_channels / 3 (eval.py:103-104 and, for uint8, the / 255. of :80, fused); u_t of window b is pool frame table[b,S-1].
        With `mask` [B,H,W] (`random_mask_plane`): `dvsg_stabilize_ring_masked_*`, eval_train.py's graph."""
        import torch
        B, H, W = self._check_ring(pool, table)
        if precision not in self._PRECISION_CODE:
            raise ValueError("precision must be 'f32', 'f32s', 'f32x3' or 'f16', got %r" % (precision,))
        if tuple(out.shape) != (B, H, W, 3) or F.numel() != B * 50:
            raise ValueError("out must be [B,H,W,3] and F_t [B,25,2]")
        for name, t, n in (("s_t_pred", out, None), ("F_t", F, None), ("x_s", xs, B * H * W), ("y_s", ys, B * H * W)):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
            if n is not None and t.numel() != n:
                raise ValueError("%s must hold B*H*W = %d values" % (name, n))
        ws, nbytes = self.workspace(B, H, W)
        if mask is not None:
            self._check_mask(mask, B, H, W)
            fn = "dvsg_stabilize_ring_masked_u8" if pool.dtype == torch.uint8 else "dvsg_stabilize_ring_masked_f32"
            _lib.call(fn, self.handle, self._PRECISION_CODE[precision], ptr(pool), int(pool.shape[0]), ptr(table), ptr(mask),
                      B, H, W, ptr(out), ptr(F), ptr(xs), ptr(ys), ptr(ws), nbytes, stream())
            return
        fn = "dvsg_stabilize_ring_u8" if pool.dtype == torch.uint8 else "dvsg_stabilize_ring_f32"
        _lib.call(fn, self.handle, self._PRECISION_CODE[precision], ptr(pool), int(pool.shape[0]), ptr(table), B, H, W,
                  ptr(out), ptr(F), ptr(xs), ptr(ys), ptr(ws), nbytes, stream())

    def stabilize_ring_inplace(self, pool, table, out_slots, F, xs=None, ys=None, precision="f32"):
        """`dvsg_stabilize_ring_inplace_f32`: `stabilize_ring` on a float32 pool whose result for window b is written
        into pool frame out_slots[b] (int32 [B] on the device) -- the history write-back of eval.py:116 for online
        streams (coupe.dvsg_amd.online).  The out slots must be distinct and no entry of `table` may name one of them
        (not checked on the device)."""
        import torch
        B, H, W = self._check_ring(pool, table)
        if pool.dtype != torch.float32:
            raise ValueError("an in-place ring holds the stabilised history: pool must be float32")
        if precision not in self._PRECISION_CODE:
            raise ValueError("precision must be 'f32', 'f32s', 'f32x3' or 'f16', got %r" % (precision,))
        if out_slots.dtype != torch.int32 or out_slots.dim() != 1 or out_slots.shape[0] != B or not out_slots.is_cuda \
                or not out_slots.is_contiguous():
            raise ValueError("out_slots must be a contiguous int32 device tensor [%d]" % B)
        if F.numel() != B * 50:
            raise ValueError("F_t must be [B,25,2]")
        for name, t, n in (("F_t", F, None), ("x_s", xs, B * H * W), ("y_s", ys, B * H * W)):
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("%s must be a contiguous float32 device tensor" % name)
            if n is not None and t.numel() != n:
                raise ValueError("%s must hold B*H*W = %d values" % (name, n))
        ws, nbytes = self.workspace(B, H, W)
        _lib.call("dvsg_stabilize_ring_inplace_f32", self.handle, self._PRECISION_CODE[precision], ptr(pool),
                  int(pool.shape[0]), ptr(table), ptr(out_slots), B, H, W, ptr(F), ptr(xs), ptr(ys), ptr(ws), nbytes,
                  stream())

    def forward_masked(self, src, mask, table=None, precision="f32", stage=-1):
        """`dvsg_locnet_forward_masked`: F_t [B,25,2] (stage -1) or the parity tap of `stage` (0 conv1, 1 pool1) with
        the mask plane [B,H,W] multiplied into the history channels in conv1's load stage.  `src` is a window tensor
        [B,H,W,in_channels] (table None) or a frame pool [n,H,W,3] float32 / uint8 with its index table [B,in_channels/3]."""
        import torch
        if table is None:
            t = as_dev(src)
            B, H, W, C = t.shape
            if C != self.in_channels:
                raise ValueError("a masked window has %d channels (conv1 of the loaded checkpoint), got %d" % (self.in_channels, C))
            kind, n_pool = 0, 0
        else:
            t = src
            B, H, W = self._check_ring(t, table)
            kind, n_pool = (2 if t.dtype == torch.uint8 else 1), int(t.shape[0])
        self._check_mask(mask, B, H, W)
        if stage > 1:
            raise ValueError("forward_masked taps stages 0 (conv1) and 1 (pool1); later stages do not depend on the source")
        ws, nbytes = self.workspace(B, H, W)
        dims = (ctypes.c_int * 3)()
        if stage < 0:
            buf = torch.empty((B, 25, 2), dtype=torch.float32, device=t.device)
        else:
            h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            buf = torch.empty((B * max(h1 * w1 * 64, 2048),), dtype=torch.float32, device=t.device)
        _lib.call("dvsg_locnet_forward_masked", self.handle, self._PRECISION_CODE[precision], ptr(t), kind, n_pool,
                  ptr(table), ptr(mask), B, H, W, int(stage), ptr(buf), buf.numel() * 4, dims, ptr(ws), nbytes, stream())
        if stage < 0:
            return buf
        h, w, c = dims[0], dims[1], dims[2]
        return buf[:B * h * w * c].reshape(B, h, w, c)

    def forward_ring(self, pool, table, precision="f32", stage=-1):
        """`dvsg_locnet_forward_ring`: F_t [B,25,2] (stage -1) or the parity tap of `stage` from a frame ring."""
        import torch
        B, H, W = self._check_ring(pool, table)
        ws, nbytes = self.workspace(B, H, W)
        dims = (ctypes.c_int * 3)()
        if stage < 0:
            buf = torch.empty((B, 25, 2), dtype=torch.float32, device=pool.device)
        else:
            h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            buf = torch.empty((B * max(h1 * w1 * 64, 2048),), dtype=torch.float32, device=pool.device)
            if stage > 1:
                raise ValueError("forward_ring taps stages 0 (conv1) and 1 (pool1); later stages do not depend on the source")
        _lib.call("dvsg_locnet_forward_ring", self.handle, self._PRECISION_CODE[precision], ptr(pool),
                  1 if pool.dtype == torch.uint8 else 0, int(pool.shape[0]), ptr(table), B, H, W, int(stage), ptr(buf),
                  buf.numel() * 4, dims, ptr(ws), nbytes, stream())
        if stage < 0:
            return buf
        h, w, c = dims[0], dims[1], dims[2]
        return buf[:B * h * w * c].reshape(B, h, w, c)

    def calibrate_f16(self, patches):
        """`dvsg_locnet_calibrate_f16`: measure the mean activation of every convolution input on the calibration windows
        `patches` [B,H,W,in_channels] (a few frames of the clip about to be stabilised) and re-round the plain float16 weights of
        blocks 2-4 with error feedback, after which precision="f16" runs those blocks without the lo weight piece: 22 %
        less time, F_t within 1e-6 of the paired mode on frames of the calibration windows' statistics.  `None` undoes it."""
        if patches is None:
            ws, nbytes = self.workspace(1, 64, 64)
            _lib.call("dvsg_locnet_calibrate_f16", self.handle, 0, 0, 0, 0, ptr(ws), nbytes, stream())
            self.f16_calibrated = False
            return self
        t = as_dev(patches)
        B, H, W, C = t.shape
        if C != self.in_channels:
            raise ValueError("calibration windows must have %d channels, got %d" % (self.in_channels, C))
        ws, nbytes = self.workspace(B, H, W)
        _lib.call("dvsg_locnet_calibrate_f16", self.handle, ptr(t), B, H, W, ptr(ws), nbytes, stream())
        self.f16_calibrated = True
        return self

    def forward(self, patches, param_dim=25, precision="f32"):
        t = as_dev(patches)
        B, H, W, C = t.shape
        if C != self.in_channels:
            raise ValueError("localizationNet was loaded for %d input channels, got %d" % (self.in_channels, C))
        if param_dim != 25:
            raise ValueError("the reference's dense4 has 50 outputs: param_dim must be 25")
        ws, nbytes = self.workspace(B, H, W)
        F = empty((B, param_dim, 2), t)
        _lib.call(_entry("dvsg_locnet_forward", precision), self.handle, ptr(t), B, H, W, ptr(F), ptr(ws), nbytes,
                  stream())
        return F

    def tap(self, patches, stage, precision="f32"):
        """Parity hook: activation after `stage` (0 conv1, 1 pool1, 2..17 units, 18 pool5), float32."""
        t = as_dev(patches)
        B, H, W, C = t.shape
        ws, nbytes = self.workspace(B, H, W)
        h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        h, w = (h1 + 1) // 2, (w1 + 1) // 2
        cap = max(h1 * w1 * 64, h * w * 64)
        for base, units, last_stride in ((64, 3, 2), (128, 4, 2), (256, 6, 2), (512, 3, 1)):
            for u in range(1, units + 1):   # tiny frames: h*w*depth does not shrink monotonically
                s = last_stride if u == units else 1
                h, w = (h - 1) // s + 1, (w - 1) // s + 1
                cap = max(cap, h * w * base * 4)
        cap *= B
        buf = empty((cap,), t)
        dims = (ctypes.c_int * 3)()
        _lib.call(_entry("dvsg_locnet_forward_tap", precision), self.handle, ptr(t), B, H, W, int(stage), ptr(buf), cap * 4,
                  dims, ptr(ws), nbytes, stream())
        h, w, c = dims[0], dims[1], dims[2]
        return buf[:B * h * w * c].reshape(B, h, w, c)


def random_mask_plane(H_theta, h, w):
    """model.py:156-167 / eval_train.py:53-64: ProjectiveTransformer([h, w]).transform(ones, H_theta)[..., 0] for
    H_theta [B,8] (after the scale and identity offset of :162-163), float32 [B,h,w] on the device."""
    tt = as_dev(H_theta)
    if tt.dim() != 2 or tt.shape[1] != 8:
        raise ValueError("H must be [B,8], got %s" % (tuple(tt.shape),))
    B = int(tt.shape[0])
    out = empty((B, int(h), int(w)), tt)
    _lib.call("dvsg_random_mask_plane_f32", ptr(tt), B, int(h), int(w), ptr(out), stream())
    return out


def load_localizationNet(weights, scope="stabNet/localizationNet"):
    """Create (or replace) the network living under `scope` from checkpoint arrays keyed by
    the reference's variable names (ckpt_manager.py:33)."""
    _nets[scope] = LocNet(weights)
    return _nets[scope]


def localizationNet(input, param_dim, is_train=False, reuse=False, scope="stabNet/localizationNet"):
    """networks.py:30-46."""
    if is_train:
        raise NotImplementedError("training graph is out of scope; is_train must be False (model.py:99)")
    key = scope if isinstance(scope, str) else getattr(scope, "name", str(scope))
    if key not in _nets:
        raise _lib.DvsgError("no weights loaded for scope %r: call load_localizationNet(weights) first "
                             "(the reference would silently run on random weights, ckpt_manager.py:21-22)" % key)
    F = _nets[key].forward(input, param_dim)
    return like_input(F, input)
