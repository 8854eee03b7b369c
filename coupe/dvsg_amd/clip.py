"""Callers of the hot path: the eval.py clip loop and the multi-GPU window sharding.

* `stabilize_clip` reproduces the reference driver's frame loop (eval.py:76-124) with the clip
  resident in HBM from the uint8 frames in to the uint8 frames out: 32 copies of frame 0 are
  prepended, each step feeds the 7-frame dilated window k + [0,16,24,28,30,31,32]
  (config.py:48), and the stabilised frame is written back into the history (eval.py:116-120).
  That write-back makes frame t depend on stabilised frame t-1, so ONE clip cannot be sharded
  across GPUs ("replicas only": different clips on different GPUs).
* `shard_range` / `sharded_map` / `stabilize_windows_sharded` cover the case that does shard:
  independent windows (BASELINE.json configs[3]).  Rank r owns a contiguous block of windows,
  there is no data-path collective, and the stabilised frames are gathered to one rank at the end
  (RCCL over xGMI on GPUs; any torch.distributed backend works -- the CPU tests use gloo).
* `stabilize_clip_teacher_forced` is the reference's other driver, eval_train.py:115-165, whose
  history frames come from the ground-truth stable clip: its windows ARE independent, so a clip
  runs batched and sharded over the GPUs of a node.  That driver evaluates eval_train.py's OWN graph
  (:25-51), whose CNN input is multiplied by a random projective mask (:43-45, 53-64): `mask_H`.
"""
import numpy as np
import torch

SKIP_LENGTH = (0, 16, 24, 28, 30, 31, 32)   # config.py:48
RENDER_BATCH_BYTES = 1 << 28                # output bytes per source-size render launch (stabilize_clip(source_res=True))


def shard_range(n, world, rank):
    """Contiguous block [lo, hi) of `n` windows owned by `rank` (sizes differ by at most 1)."""
    if not (0 <= rank < world):
        raise ValueError("rank %d outside world of %d" % (rank, world))
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def sharded_map(n, batch, produce, frame_shape, like, group=None, dst=0):
    """Run `produce(b0, b1) -> [b1-b0, *frame_shape]` over this rank's contiguous share of `n`
    independent units in batches of at most `batch`, then gather the results, in unit order, on
    rank `dst` (None elsewhere).  No collective on the data path; one exchange at the end, which every rank of
    the group must reach (ranks whose shard is empty included: they join its opening all-reduce and send nothing)."""
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, hi = shard_range(n, world, rank)
    outs = []
    for b0 in range(lo, hi, batch):
        outs.append(torch.as_tensor(produce(b0, min(hi, b0 + batch))))
    ref = outs[0] if outs else like
    local = torch.cat(outs, 0) if outs else ref.new_zeros((0,) + tuple(frame_shape))
    if world == 1:
        return local
    # One exchange at the end, only real rows: every rank that owns windows sends its slab straight
    # to `dst` (its own xGMI link on RCCL), which receives each slab in place -- no padding to a
    # common shard size, no copy after the receive.
    on_host = local.is_cuda and dist.get_backend(group) != "nccl"
    back = local.device
    # EVERY rank enters one cheap collective first, whatever it owns.  A rank with an empty shard (n < world,
    # e.g. a 2-window clip on 8 GPUs) takes no part in the point-to-point exchange below, and on NCCL / RCCL a
    # `batch_isend_irecv` that is the FIRST communication of a group must be entered by all of its ranks (it
    # creates the communicator; otherwise the behaviour is undefined and can hang).  The all-reduce creates the
    # communicator with everybody present and doubles as a consistency check of the sharding: the shard sizes
    # the ranks computed must add up to n.
    # (its device follows the BACKEND, not `local`: a rank with an empty shard may hold a CPU `like` while the populated
    # ranks hold device tensors, and a CPU tensor in an NCCL / RCCL collective raises on that rank and hangs the others)
    if dist.get_backend(group) == "nccl":
        count_dev = torch.device("cuda", torch.cuda.current_device())
        if not local.is_cuda:
            local = local.to(count_dev)
            back = count_dev
    else:
        count_dev = torch.device("cpu")
    count = torch.tensor([local.shape[0]], dtype=torch.int64, device=count_dev)
    dist.all_reduce(count, op=dist.ReduceOp.SUM, group=group)
    if int(count.item()) != n:
        raise RuntimeError("sharded_map: the ranks hold %d units in total, expected %d (every rank must pass the "
                           "same n)" % (int(count.item()), n))
    if on_host:
        local = local.cpu()   # rehearsal backends (gloo) exchange through host memory; RCCL stays on the device
    peer = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    if rank != dst:
        if local.shape[0]:
            for req in dist.batch_isend_irecv([dist.P2POp(dist.isend, local.contiguous(), peer(dst), group)]):
                req.wait()
        return None
    full = local.new_empty((n,) + tuple(frame_shape))
    ops = []
    for r in range(world):
        rlo, rhi = shard_range(n, world, r)
        if r == dst:
            full[rlo:rhi] = local
        elif rhi > rlo:
            ops.append(dist.P2POp(dist.irecv, full[rlo:rhi], peer(r), group))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    return full.to(back) if on_host else full


def stabilize_windows_sharded(run_fn, patches_t, u_t, batch=16, group=None, dst=0):
    """Stabilise `patches_t` [N,H,W,3S] / `u_t` [N,H,W,3] (every rank passes the same N) with
    the windows sharded over the ranks of `group`; returns [N,H,W,3] on rank `dst`, None
    elsewhere.  `run_fn(patches, u) -> [b,H,W,3]` is the per-batch hot path (e.g.
    `lambda p, u: sess.run(outputs['s_t_pred'], {inputs['patches_t']: p, inputs['u_t']: u})`)."""
    return sharded_map(patches_t.shape[0], batch, lambda b0, b1: run_fn(patches_t[b0:b1], u_t[b0:b1]),
                       (u_t.shape[1], u_t.shape[2], 3), torch.as_tensor(u_t[:0]), group, dst)


def check_skip_length(skip_length):
    """skip_length (config.py:48) as int64: it must start at 0 and increase strictly."""
    skip = np.asarray(skip_length, dtype=np.int64)
    if skip.ndim != 1 or skip.size < 1 or skip[0] != 0 or np.any(np.diff(skip) <= 0):
        raise ValueError("skip_length must start at 0 and increase strictly (config.py:48)")
    return skip


def window_index_table(n_frames, skip_length=SKIP_LENGTH):
    """The frame loop of eval.py:93-124 as an index table.  With the clip kept in a pool of
    2 N frames -- [0, N) the unstable inputs, [N, 2 N) the stabilised outputs -- entry [k, s] is
    the pool frame that window slot s holds at step k: slot k + skip[s] of the reference's
    padded history list, which is
      * the unstable frame k for the last slot (eval.py:103, sample_idx[-1]);
      * a stabilised frame for every slot the write-back of eval.py:116 already replaced;
      * one of the 32 prepended copies of frame 0 (eval.py:93-94) otherwise -- the unstable
        frame 0 at step 0, the stabilised frame 0 afterwards (eval.py:118-120).
    Returns int32 [N, S]."""
    skip = check_skip_length(skip_length)
    N = int(n_frames)
    span = int(skip[-1])
    k = np.arange(N, dtype=np.int64)[:, None]
    j = k + skip[None, :]                                    # slot in the padded history
    table = np.where(j >= span, N + (j - span), np.where(k == 0, 0, N))
    table[:, -1] = k[:, 0]
    return table.astype(np.int32)


def _check_window(model, S):
    """A window of S frames is 3 S channels; conv1 of the loaded checkpoint fixes that number."""
    if 3 * S != model.locnet.in_channels:
        raise ValueError("skip_length has %d entries (%d channels) but conv1 of the loaded checkpoint has %d "
                         "input channels" % (S, 3 * S, model.locnet.in_channels))


INT32_MAX = 2 ** 31 - 1


def _check_crop_grid(out_h, out_w):
    """The host-side shape rules of dvsg_tps_coverage_f32, raised as ValueError before any launch; returns D."""
    out_h, out_w = int(out_h), int(out_w)
    if out_h < 2 or out_w < 2:
        raise ValueError("a crop needs an output grid of at least 2 x 2, got %d x %d" % (out_h, out_w))
    D = (out_h - 1) * (out_w - 1)
    if D >= INT32_MAX or out_h * out_w >= 2 ** 31:
        raise ValueError("output grid %d x %d too large for the coverage scan: (out_h - 1)(out_w - 1) must stay below 2^31 - 1"
                         % (out_h, out_w))
    return D


def _zoom_tensor(zoom, n, dev):
    """None, a scalar or n values -> None or float32 [n] on the device"""
    if zoom is None:
        return None
    if isinstance(zoom, torch.Tensor):
        z = zoom.to(dev, torch.float32).reshape(-1)
    else:
        z = torch.from_numpy(np.asarray(zoom, dtype=np.float32).reshape(-1)).to(dev)
    if z.numel() == 1:
        z = z.expand(n)
    if z.numel() != n:
        raise ValueError("zoom must be a scalar or one value per frame (%d), got %d" % (n, z.numel()))
    return z.contiguous()


def _coverage(model, F, src_hw, out_hw, zoom, T=None, net=None):
    """`dvsg_tps_coverage_net_f32` over all rows of F [N,25,2] (device), 65535 at a time -> int32 [2,N] on the device
    (n_border | key_min); T [N,2,28], if given, receives the TPS coefficients.  net: the handle the scan is given (default the
    network itself); a shaped view (`LocNet.view`) scans the warp its render draws."""
    import ctypes
    from . import _lib
    from ._tensor import ptr, stream
    N = int(F.shape[0])
    (sh, sw), (oh, ow) = src_hw, out_hw
    res = torch.empty((2, N), dtype=torch.int32, device=F.device)
    if T is None:
        T = torch.empty((N, 2, model.param_dim + 3), dtype=torch.float32, device=F.device)
    need = ctypes.c_size_t()
    _lib.call("dvsg_tps_coverage_workspace_bytes", min(N, 65535), oh, ow, ctypes.byref(need))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=F.device)
    for b0 in range(0, N, 65535):
        b1 = min(N, b0 + 65535)
        _lib.call("dvsg_tps_coverage_net_f32", model.locnet.handle if net is None else net, ptr(F[b0:b1]), ptr(zoom[b0:b1]) if zoom is not None else None,
                  b1 - b0, int(sh), int(sw), oh, ow, ptr(T[b0:b1]), ptr(res[0, b0:b1]), ptr(res[1, b0:b1]), ptr(ws),
                  ws.numel() * 8, stream())
    return res


def crop_scan(model, F, src_hw, out_hw=None, zoom=None):
    """How much of each stabilised frame is border?  F [N,25,2]: the F_t of every frame (NumPy or torch); src_hw = (H, W) of
    the frame sampler A reads; out_hw the output grid (default src_hw); zoom: None, a scalar or [N] float32, the zoom of the
    grid about its centre.  One fused launch pair (`dvsg_tps_coverage_net_f32`: map, validity predicate and reduction; x_s /
    y_s never reach memory) and ONE device -> host read.  Returns a dict of NumPy arrays with one entry per frame:
      border_pixels  int: output pixels that sampler A leaves black (two of its taps coincide and their weights cancel);
      key_min        int: the smallest key max(|2j - (w-1)| (h-1), |2i - (h-1)| (w-1)) over them, 2^31 - 1 if there is none;
      free           float64 min(key_min, D) / D, D = (h-1)(w-1): the centred rectangle of the frame's aspect ratio scaled
                     by `free` is the largest one that holds no border pixel (1.0: nothing but the outermost ring, if that)."""
    from . import _lib
    from ._tensor import device
    if model.locnet is None:
        raise _lib.DvsgError("StabNet has no weights: call load_weights()/load_ckpt() first")
    out_hw = tuple(src_hw) if out_hw is None else tuple(out_hw)
    D = _check_crop_grid(*out_hw)
    if int(src_hw[0]) < 1 or int(src_hw[1]) < 1:
        raise ValueError("src_hw must be positive, got %s" % (tuple(src_hw),))
    dev = device()
    Ft = (F if isinstance(F, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(F, dtype=np.float32)))
    Ft = Ft.to(dev, torch.float32).contiguous()
    if Ft.dim() != 3 or tuple(Ft.shape[1:]) != (model.param_dim, 2) or Ft.shape[0] < 1:
        raise ValueError("F must be [N,%d,2]" % model.param_dim)
    res = _coverage(model, Ft, src_hw, (int(out_hw[0]), int(out_hw[1])), _zoom_tensor(zoom, int(Ft.shape[0]), dev)).cpu().numpy()
    key = res[1].astype(np.int64)
    return dict(free=np.minimum(key, D).astype(np.float64) / D, border_pixels=res[0].astype(np.int64), key_min=key)


def crop_zoom(free, margin=None, crop_min=0.5, out_hw=None):
    """The clip's ONE zoom from the per-frame `free` of `crop_scan` (a zoom per frame would put the jitter back):
        z = max(min(free) - margin, crop_min), at most 1, rounded once to float32.
    margin: default 2 / (min(out_h, out_w) - 1) -- one pixel of the shorter axis in the grid's units, which needs out_hw.
    `free` is measured on the pixels of the UNZOOMED grid; the zoomed grid's pixels lie between them, and a border that is
    not straight can reach one of them although both of its neighbours on the old grid were valid: the margin pays for that."""
    free = np.asarray(free, dtype=np.float64).reshape(-1)
    if free.size < 1 or not np.all(np.isfinite(free)) or free.min() < 0.0:
        raise ValueError("free must hold at least one finite value >= 0")
    if margin is None:
        if out_hw is None:
            raise ValueError("the default margin is one pixel of the shorter axis: pass out_hw or margin")
        _check_crop_grid(*out_hw)
        margin = 2.0 / (min(int(out_hw[0]), int(out_hw[1])) - 1)
    margin, crop_min = float(margin), float(crop_min)
    if not (margin >= 0.0) or not (0.0 < crop_min <= 1.0):
        raise ValueError("margin must be >= 0 and crop_min in (0, 1]")
    return np.float32(min(max(float(free.min()) - margin, crop_min), 1.0))


def _check_crop(crop):
    """crop argument of stabilize_clip -> None, "auto" or a float32 in (0, 1]"""
    if crop is None or (isinstance(crop, str) and crop == "auto"):
        return crop
    if isinstance(crop, (str, bytes, bool)) or not np.isscalar(crop):
        raise ValueError("crop must be None, 'auto' or a zoom in (0, 1], got %r" % (crop,))
    z = np.float32(crop)
    if not (z > 0.0 and z <= 1.0):       # NaN fails both
        raise ValueError("crop must be None, 'auto' or a zoom in (0, 1], got %r" % (crop,))
    return z


def stabilize_clip(model, session, frames, skip_length=SKIP_LENGTH, side_by_side=False, channel_order="rgb",
                   as_uint8=False, source_res=False, crop=None, crop_margin=None, crop_min=0.5, crop_info=None,
                   render_filter="bilinear", border="black", strength=1.0, rigidity=0.0, shape_model="affine"):
    """eval.py:76-124 for one clip, entirely on the device.

    frames: [N,h0,w0,3], NumPy or torch.
      * uint8 -- raw decoded frames.  They are converted as eval.py:79-80 does (optional
        BGR->RGB with channel_order="bgr", / 255. in float64, cv2.resize to the model's (w, h)
        when the size differs) by `dvsg_frames_u8_to_f32` / `dvsg_frames_resize_u8_f32`;
      * float -- RGB in [0,1], already (model.h, model.w); rounded to float32 once, which is the
        cast TF applies to the fed window (eval.py:106-110).
    Video decode / encode (cv2.VideoCapture / VideoWriter) is host I/O and out of scope.

    The clip lives in one HBM pool [2N,h,w,3] float32 (unstable | stabilised).  Each step is ONE call,
    `dvsg_stabilize_ring_f32`: conv1 assembles the 3S-channel window of eval.py:103-104 in its load stage
    from the pool frames `window_index_table` names, and the result is written straight into its pool
    slot; the write-back of eval.py:116-120 is the index table, not a copy.  `session` is accepted for call-site
    symmetry with eval.py and not used.

    Returns the stabilised frames [N,h,w,3] -- float32, or uint8 (np.uint8(x * 255.),
    eval.py:112) with as_uint8 -- and, with side_by_side, also the reference's output video
    frames uint8 [N,h,2w,3] (unstable | stabilised, eval.py:112; BGR if channel_order="bgr",
    eval.py:113).  NumPy in -> NumPy out.

    source_res=True (uint8 frames only): the outputs are at the frames' own size [N,h0,w0,3] (side [N,h0,2 w0,3], the
    unstable half the source bytes): after the loop, each frame's F_t warps its source frame (`dvsg_tps_render_u8`, in
    launches of at most RENDER_BATCH_BYTES of output).  The loop itself is unchanged.
    render_filter="bicubic" (source_res only, else ValueError) renders them with the bicubic filter of a view
    (`LocNet.view`: 16 taps, bytes rounded to nearest; include/dvsg_amd.h, "Views and the render filter"); the default
    "bilinear" is sampler A.  F_t, the pool and the crop's zoom do not depend on it.
    border="replicate" / "mirror" (source_res only, else ValueError) fill the black border of those renders from the
    source's edge (include/dvsg_amd.h, "Border modes"; `LocNet.view`); with crop they fill whatever the zoom leaves.
    border="keep" is a ValueError here: it carries each frame's border over from the frame before, and these renders run
    after the loop in launches of many frames at once, not one frame at a time in order -- `OnlineStabilizer(border="keep")`
    (or `online.stabilize_clips`) renders frame by frame and takes it.
    strength, rigidity, shape_model (source_res only, else ValueError): how much of each frame's warp those renders apply
    (include/dvsg_amd.h, "Warp shaping"; `OnlineStabilizer` describes them).  They select the view the renders AND the
    scans of crop are given, so the clip's one zoom of crop="auto" is the zoom of the shaped warps.  The loop, F_t and the
    pool do not depend on them.

    crop: every stabilised frame has a black border wherever sampler A's taps leave the frame (at F_t = 0 already its last
    row and column).  None (default) returns the frames as the reference does.  "auto" or a zoom z in (0, 1] renders them
    WITHOUT it: the loop runs unchanged -- it must keep feeding back uncropped frames --, then `crop_scan` measures every
    frame, `crop_zoom(free, crop_margin, crop_min)` picks one z for the clip ("auto"), and every frame is rendered again
    from its unstable frame and its F_t on the output grid scaled by z about its centre (`dvsg_tps_warp_zoom_f32` from the
    float32 pool, `dvsg_tps_render_zoom_u8` from the uint8 source with source_res): still one interpolation per pixel.
    crop_info, if a dict, receives zoom, cropping_ratio (= zoom), free [N], border_pixels [N] of the rendered crop (a
    second scan at z; all 0 unless crop_min or an explicit z cut the zoom short) and limited: the frames whose
    free - margin < crop_min.
    """
    crop = _check_crop(crop)
    from . import _lib
    from ._tensor import device, ptr, stream
    from .networks import check_border, check_render_filter, check_shape
    check_render_filter(render_filter, bool(source_res))
    strength, rigidity, shape_model = check_shape(strength, rigidity, shape_model, bool(source_res))
    if check_border(border, bool(source_res)) == "keep":
        raise ValueError("border='keep' needs renders that run one frame at a time in order; stabilize_clip renders its "
                         "frames in batches after the loop: use OnlineStabilizer(border='keep') or online.stabilize_clips")
    if channel_order not in ("rgb", "bgr"):
        raise ValueError("channel_order must be 'rgb' or 'bgr'")
    if model.locnet is None:
        raise _lib.DvsgError("StabNet has no weights: call load_weights()/load_ckpt() first")
    flip = 1 if channel_order == "bgr" else 0
    host = not isinstance(frames, torch.Tensor)
    dev = device()
    fr = torch.as_tensor(np.ascontiguousarray(frames)) if host else frames
    if fr.dim() != 4 or fr.shape[3] != 3 or fr.shape[0] < 1:
        raise ValueError("frames must be [N,h,w,3]")
    N, h, w = int(fr.shape[0]), model.h, model.w
    S = len(skip_length)
    _check_window(model, S)
    table = torch.from_numpy(window_index_table(N, skip_length)).to(dev)
    pool = torch.empty((2 * N, h, w, 3), dtype=torch.float32, device=dev)
    fr = fr.to(dev).contiguous()
    if source_res and fr.dtype != torch.uint8:
        raise ValueError("source_res renders the uint8 source frames; float frames have no source beyond the model's size")
    # the unstable half of the output video is np.uint8(float64 frame * 255.) (eval.py:112): rendered
    # from float64 wherever the float32 pool would not hold the same value
    side = torch.empty((N, h, 2 * w, 3), dtype=torch.uint8, device=dev) if side_by_side and not source_res else None
    left_done = False
    if fr.dtype == torch.uint8:
        if tuple(fr.shape[1:3]) == (h, w):
            _lib.call("dvsg_frames_u8_to_f32", ptr(fr), N * h * w, flip, ptr(pool), stream())
        else:
            _lib.call("dvsg_frames_resize_u8_f32", ptr(fr), N, int(fr.shape[1]), int(fr.shape[2]), flip, ptr(pool),
                      h, w, ptr(side), 2 * w, 0, stream())
            left_done = side is not None
    elif fr.dtype.is_floating_point:
        if tuple(fr.shape[1:3]) != (h, w):
            raise ValueError("float frames must already be [N,%d,%d,3] (StabNet(h, w) fixes the STN out_size)" % (h, w))
        pool[:N] = fr        # one rounding to float32 (the feed cast); a plain device copy for float32 input
        if side_by_side and fr.dtype == torch.float64:
            _lib.call("dvsg_frames_f64_to_u8", ptr(fr), N, h, w, flip, ptr(side), 2 * w, 0, stream())
            left_done = True
    else:
        raise TypeError("frames must be uint8 or floating point, got %s" % fr.dtype)
    F = torch.empty((N, model.param_dim, 2), dtype=torch.float32, device=dev)   # F_t of every frame
    # one call per frame: conv1 picks the S window frames out of the pool through table[k] (eval.py:103-104 fused
    # into its load stage: no window tensor, no gather launch), the warp reads u_t = pool[table[k, S - 1]] = pool[k],
    # and the result lands in its history slot pool[N + k] (:116), which no slot of window k reads
    for k in range(N):                                                             # eval.py:101
        model.locnet.stabilize_ring(pool, table[k:k + 1], pool[N + k:N + k + 1], F[k:k + 1],
                                    precision=model.precision)                    # :106-110
    zoom = None
    if crop is not None:
        out_hw = (int(fr.shape[1]), int(fr.shape[2])) if source_res else (h, w)
        shaped = strength != 1.0 or rigidity != 0.0   # the scans take the view the renders take
        zoom, T_all = _choose_zoom(model, F, out_hw, crop, crop_margin, crop_min, crop_info,
                                   model.locnet.view(render_filter, border, strength, rigidity, shape_model) if shaped else None)
    if source_res:   # eval.py:112-113 at the frames' own size, in launches of at most RENDER_BATCH_BYTES of output
        H0, W0 = int(fr.shape[1]), int(fr.shape[2])
        out = torch.empty((N, H0, W0, 3), dtype=torch.uint8 if as_uint8 else torch.float32, device=dev)
        side = torch.empty((N, H0, 2 * W0, 3), dtype=torch.uint8, device=dev) if side_by_side else None
        batch = max(1, min(N, 65535, RENDER_BATCH_BYTES // (H0 * W0 * 3 * (out.element_size() + int(side_by_side)))))
        T = torch.empty((batch, 2, model.param_dim + 3), dtype=torch.float32, device=dev)
        for b0 in range(0, N, batch):
            b1 = min(N, b0 + batch)
            render_source_into(model, fr[b0:b1], F[b0:b1], T, flip, out[b0:b1], side[b0:b1] if side is not None else None,
                               zoom[b0:b1] if zoom is not None else None, render_filter, border, strength, rigidity,
                               shape_model)
        if host:
            out = out.cpu().numpy()
            side = side.cpu().numpy() if side is not None else None
        return (out, side) if side_by_side else out
    stab = pool[N:]
    if zoom is not None:   # the cropped frames: every unstable frame warped once more, on the zoomed grid, by its own T
        from .model import V_SRC
        stab = torch.empty((N, h, w, 3), dtype=torch.float32, device=dev)
        V = torch.from_numpy(V_SRC).to(dev).unsqueeze(0).repeat(min(N, 65535), 1, 1).contiguous()
        for b0 in range(0, N, 65535):
            b1 = min(N, b0 + 65535)
            _lib.call("dvsg_tps_warp_zoom_f32", ptr(pool[b0:b1]), ptr(V), ptr(T_all[b0:b1]), ptr(zoom[b0:b1]), b1 - b0, h, w, 3,
                      model.param_dim, h, w, ptr(stab[b0:b1]), None, None, stream())
    if side_by_side:                                                               # eval.py:112-113
        if not left_done:   # uint8 / float32 input: the float32 pool holds the frame exactly
            _lib.call("dvsg_frames_f32_to_u8", ptr(pool), N, h, w, flip, ptr(side), 2 * w, 0, stream())
        _lib.call("dvsg_frames_f32_to_u8", ptr(stab), N, h, w, flip, ptr(side), 2 * w, w, stream())
    if as_uint8:
        out = torch.empty((N, h, w, 3), dtype=torch.uint8, device=dev)
        _lib.call("dvsg_frames_f32_to_u8", ptr(stab), N, h, w, flip, ptr(out), w, 0, stream())
    else:
        out = stab.clone() if zoom is None else stab
    if host:
        out = out.cpu().numpy()
        side = side.cpu().numpy() if side is not None else None
    return (out, side) if side_by_side else out


def _choose_zoom(model, F, out_hw, crop, crop_margin, crop_min, crop_info, net=None):
    """The crop of stabilize_clip: scan every frame's F_t on the plain grid, pick the clip's zoom ("auto") or take the
    caller's, scan again at that zoom for the report.  net: the handle the scans are given (`_coverage`).  Returns (zoom
    float32 [N] on the device, T [N,2,28])."""
    N = int(F.shape[0])
    D = _check_crop_grid(*out_hw)
    margin = 2.0 / (min(out_hw) - 1) if crop_margin is None else float(crop_margin)
    T = torch.empty((N, 2, model.param_dim + 3), dtype=torch.float32, device=F.device)
    key = _coverage(model, F, out_hw, out_hw, None, T, net)[1].cpu().numpy().astype(np.int64)
    free = np.minimum(key, D).astype(np.float64) / D
    z = crop_zoom(free, margin, crop_min) if isinstance(crop, str) else crop
    zoom = torch.full((N,), float(z), dtype=torch.float32, device=F.device)
    if isinstance(crop_info, dict):
        left = _coverage(model, F, out_hw, out_hw, zoom, None, net)[0].cpu().numpy().astype(np.int64)
        crop_info.update(zoom=float(z), cropping_ratio=float(z), free=free, border_pixels=left,
                         limited=np.nonzero(free - margin < float(crop_min))[0])
    return zoom, T


def render_source_into(model, src, F, T, flip, out, side=None, zoom=None, render_filter="bilinear", border="black",
                       strength=1.0, rigidity=0.0, shape_model="affine", out_size=None):
    """`dvsg_tps_render_u8` for the uint8 frames src [n,H0,W0,3] (device) and their F_t rows F [n,25,2]: the stabilised
    frames at source size into `out` [n,H0,W0,3] (float32, or uint8: np.uint8(x * 255.) in the channel order of src)
    and, if given, `side` [n,H0,2 W0,3] uint8 = (source bytes | uint8 render).  T [n,2,28] receives the TPS
    coefficients.  One render launch; a uint8 `out` is copied into the right half of `side`.  zoom float32 [n] (device):
    `dvsg_tps_render_zoom_u8`, the render on the grid scaled by zoom[i] about its centre.  render_filter, border: the filter
    and the border mode of the handle the render is given (`LocNet.view`).  border="keep" is accepted: this is ONE launch,
    and the samples it leaves unwritten keep what the caller put into `out` (frame i of the launch does not see frame
    i - 1: a caller that wants the previous output there renders one frame at a time, as OnlineStabilizer does); with
    `side` it is a ValueError naming border.  strength, rigidity, shape_model: the warp shape of that handle -- the render
    applies F' of include/dvsg_amd.h, "Warp shaping", and T receives its coefficients.  out_size=(H, W): the render goes
    through the scaled view of that handle and `out` is [n,H,W,3] (include/dvsg_amd.h, "Output size"); with `side` it is a
    ValueError naming out_size."""
    from . import _lib
    from ._tensor import ptr, stream
    from .networks import check_border
    if check_border(border) == "keep" and side is not None:
        raise ValueError("border='keep' has no side_by_side layout: the unwritten samples are the caller's `out`")
    if out_size is not None and side is not None:
        raise ValueError("out_size has no side_by_side layout: the source half keeps the source's size")
    net = model.locnet.view(render_filter, border, strength, rigidity, shape_model, out_size=out_size)
    n, H0, W0 = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    if side is not None:
        side[:, :, :W0] = src   # np.uint8(v / 255. * 255.) == v for every byte: the unstable half is the source
    if out.dtype == torch.uint8:
        f32, u8, u8_W, u8_x0 = None, out, int(out.shape[2]), 0
    else:                       # one launch writes the float32 render and the right half of side
        f32, u8, u8_W, u8_x0 = out, side, 2 * W0, W0
    if zoom is not None:
        _lib.call("dvsg_tps_render_zoom_u8", net, ptr(F), ptr(src), n, H0, W0, flip, ptr(zoom), ptr(T), ptr(f32),
                  ptr(u8), u8_W, u8_x0, stream())
    else:
        _lib.call("dvsg_tps_render_u8", net, ptr(F), ptr(src), n, H0, W0, flip, ptr(T), ptr(f32), ptr(u8),
                  u8_W, u8_x0, stream())
    if side is not None and out.dtype == torch.uint8:
        side[:, :, W0:] = out


def teacher_forced_index_table(n_frames, skip_length=SKIP_LENGTH):
    """eval_train.py:137-165 as an index table.  There the history is never the network's own
    output: the first 32 unstable frames are replaced by the stable (ground-truth) ones up front
    (:137-138) and every processed unstable frame is replaced by its stable twin (:162), so step k
    (frame k + 32) sees stable frames in every slot but the last.  With a pool of 2 N frames --
    [0, N) unstable, [N, 2N) stable -- entry [k, s] = N + k + skip[s], and [k, -1] = k + 32.
    The windows do not depend on each other: they shard over GPUs.  Returns int32 [N-32, S]."""
    skip = check_skip_length(skip_length)
    N, span = int(n_frames), int(skip[-1])
    if N <= span:
        raise ValueError("eval_train.py needs more than %d frames, got %d" % (span, N))
    k = np.arange(N - span, dtype=np.int64)[:, None]
    table = N + k + skip[None, :]
    table[:, -1] = k[:, 0] + span
    return table.astype(np.int32)


def _frames_to_pool(fr, pool, h, w, flip, what):
    """uint8 / float frames [n,h0,w0,3] on the device -> float32 [n,h,w,3] slice of the pool."""
    from . import _lib
    from ._tensor import ptr, stream
    n = int(fr.shape[0])
    if fr.dtype == torch.uint8:
        if tuple(fr.shape[1:3]) == (h, w):
            _lib.call("dvsg_frames_u8_to_f32", ptr(fr), n * h * w, flip, ptr(pool), stream())
        else:
            _lib.call("dvsg_frames_resize_u8_f32", ptr(fr), n, int(fr.shape[1]), int(fr.shape[2]), flip, ptr(pool),
                      h, w, 0, 0, 0, stream())
    elif fr.dtype.is_floating_point:
        if tuple(fr.shape[1:3]) != (h, w):
            raise ValueError("float %s frames must already be [N,%d,%d,3]" % (what, h, w))
        pool.copy_(fr)
    else:
        raise TypeError("%s frames must be uint8 or floating point, got %s" % (what, fr.dtype))


def _mask_homographies(mask_H, n, dev):
    """eval_train.py:55-57 for the n steps of a clip: [n,8] float32 on `dev`, or None (no mask)."""
    from .model import draw_random_H
    if mask_H is None:
        return None
    if isinstance(mask_H, str):
        if mask_H != "random":
            raise ValueError("mask_H must be None, 'random', a torch.Generator or an [N-32,8] array")
        return draw_random_H(n, dev)
    if isinstance(mask_H, torch.Generator):
        return draw_random_H(n, dev, mask_H)
    Ht = torch.as_tensor(np.asarray(mask_H, dtype=np.float32) if not isinstance(mask_H, torch.Tensor) else mask_H)
    if tuple(Ht.shape) != (n, 8):
        raise ValueError("mask_H must be [%d,8] (one homography per stabilised frame), got %s" % (n, tuple(Ht.shape)))
    return Ht.to(dev, torch.float32).contiguous()


def stabilize_clip_teacher_forced(model, unstable, stable, batch=16, skip_length=SKIP_LENGTH, channel_order="rgb",
                                  as_uint8=False, group=None, dst=0, mask_H="random"):
    """eval_train.py:115-165 for one pair of clips: every unstable frame k >= 32 is stabilised from
    the window [stable k-32, k-16, k-8, k-4, k-2, k-1 | unstable k].  The windows are independent,
    so they run in batches of `batch` and -- with torch.distributed initialised -- shard over the
    ranks of `group` with no data-path collective; the stabilised frames are gathered on rank
    `dst` (BASELINE.json configs[3]).  Every rank passes the same clips (frame formats as in
    `stabilize_clip`) and keeps the whole pool in its HBM.

    mask_H: eval_train.py evaluates its OWN graph (:25-51, :86), in which the six history frames the CNN sees
    are multiplied by `random_mask` (:43-45, 53-64) -- a fresh random near-identity homography per `sess.run`.
      * "random" (default: what eval_train.py does) -- drawn with torch.rand per step (other VALUES than
        tf.random_uniform would give, the same distribution); a `torch.Generator` -- the same, reproducibly
        (a CPU generator seeded alike on every rank gives every rank the same table);
      * an array [N-32,8] -- the homography of each step, AFTER the scale / identity offset of :56-57 (the parity
        tests pin the loop against the oracle this way);
      * None -- no mask: model.py's graph (model.py:98-123) on the teacher-forced windows.  NOT what eval_train.py
        computes; kept for callers that want the regressor's unmasked prediction on ground-truth history.
    The mask is ONE [b,h,w] plane per batch (`dvsg_random_mask_plane_f32`), multiplied into the history channels
    inside conv1's load stage (`dvsg_stabilize_ring_masked_{f32,u8}`); the warp samples the unmasked frame (:48).

    Returns [N-32,h,w,3] float32 (or uint8 with as_uint8) on rank `dst` -- NumPy if the clips were
    NumPy -- and None on the other ranks."""
    from . import _lib
    from ._tensor import device, ptr, stream
    from .networks import random_mask_plane
    if channel_order not in ("rgb", "bgr"):
        raise ValueError("channel_order must be 'rgb' or 'bgr'")
    if model.locnet is None:
        raise _lib.DvsgError("StabNet has no weights: call load_weights()/load_ckpt() first")
    flip = 1 if channel_order == "bgr" else 0
    host = not isinstance(unstable, torch.Tensor)
    dev = device()
    un = (torch.as_tensor(np.ascontiguousarray(unstable)) if host else unstable).to(dev).contiguous()
    st = (torch.as_tensor(np.ascontiguousarray(stable)) if not isinstance(stable, torch.Tensor) else stable).to(dev).contiguous()
    if un.dim() != 4 or un.shape[3] != 3 or st.shape != un.shape:
        raise ValueError("unstable and stable clips must both be [N,h,w,3]")
    N, h, w, S = int(un.shape[0]), model.h, model.w, len(skip_length)
    _check_window(model, S)
    span = int(skip_length[-1])
    table = torch.from_numpy(teacher_forced_index_table(N, skip_length)).to(dev)
    Ht = _mask_homographies(mask_H, N - span, dev)
    if un.dtype == torch.uint8 and st.dtype == torch.uint8 and tuple(un.shape[1:3]) == (h, w) and not flip:
        pool = torch.cat([un, st], 0)        # the raw frames ARE the ring: 3 bytes per pixel in HBM
    else:
        pool = torch.empty((2 * N, h, w, 3), dtype=torch.float32, device=dev)
        _frames_to_pool(un, pool[:N], h, w, flip, "unstable")
        _frames_to_pool(st, pool[N:], h, w, flip, "stable")
    F = torch.empty((batch, model.param_dim, 2), dtype=torch.float32, device=dev)

    def produce(b0, b1):
        b = b1 - b0
        out = torch.empty((b, h, w, 3), dtype=torch.float32, device=dev)
        # windows b0..b1 straight from the pool (uint8 when the clips came as same-size RGB uint8 frames: the / 255. of
        # eval_train.py's frame reader happens in conv1's load stage); u_t of window k is pool frame table[k, S - 1] = k + skip_length[-1]
        plane = random_mask_plane(Ht[b0:b1], h, w) if Ht is not None else None      # eval_train.py:43 (one plane per window)
        model.locnet.stabilize_ring(pool, table[b0:b1], out, F[:b], precision=model.precision, mask=plane)
        if not as_uint8:
            return out
        out8 = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
        _lib.call("dvsg_frames_f32_to_u8", ptr(out), b, h, w, flip, ptr(out8), w, 0, stream())
        return out8

    like = torch.empty((0, h, w, 3), dtype=torch.uint8 if as_uint8 else torch.float32, device=dev)
    res = sharded_map(N - span, batch, produce, (h, w, 3), like, group, dst)
    if res is not None and host:
        res = res.cpu().numpy()
    return res


def score_clip_teacher_forced(model, unstable, stable, flows, surfs=None, surfs_dim=None, batch=16, mask_H="random",
                              precision=None, loss_applied=None, coefs=None, group=None, skip_length=SKIP_LENGTH,
                              channel_order="rgb"):
    """The checkpoint score of main.py:198-221 on one pair of clips: `trainer.build_loss_train` on the two-frame graph of
    model.py:59-96, averaged over the steps of the clip.  The windows are those of `teacher_forced_index_table` (n = N - 32 of
    them); step k = 1 .. n-1 takes window k-1 as frame t-1 and window k as frame t, the stable clip's frames k+31 and k+32
    as s_t_1_gt / s_t_gt, and
      flows[k]     [h,w,2] float32 in pixels (data_loader.py:239), `flows` being [n,h,w,2] (entry 0 is not read);
      surfs[k-1], surfs[k]          int32 [2,Ns,2] matched points of the two frames, `surfs` being [n,2,Ns,2], and
      surfs_dim[k-1], surfs_dim[k]  their counts [n] -- without `surfs` the `surf` term is not applied.
    mask_H: the two `random_mask` draws of each step (model.py:71-72): "random", a torch.Generator, or an array [n-1,2,8]
    (t-1 first) after the scale / offset of :162-163.  precision: `model.precision` unless given.  loss_applied / coefs as in
    `build_loss_train` (default: every term the data allows, `cor` never).

    A step's value is the loss of that step alone (batch 1 of the reference's loop); `batch` steps run through the kernels
    together and their per-sample values are taken, so the score does not depend on `batch` beyond the network's own
    batching.  With torch.distributed initialised the steps shard over the ranks of `group` like the windows of
    `stabilize_clip_teacher_forced`; each rank adds its steps up in float64, in step order, and ONE all-reduce of those
    sums follows.  Returns an OrderedDict of Python floats on every rank: the per-term means over the steps, and `total`
    (errs_total_test of main.py:198-215)."""
    import collections
    import torch.distributed as dist
    from . import _lib, trainer
    from ._tensor import device
    from .model import V_SRC
    from .networks import random_mask_plane
    if channel_order not in ("rgb", "bgr"):
        raise ValueError("channel_order must be 'rgb' or 'bgr'")
    if model.locnet is None:
        raise _lib.DvsgError("StabNet has no weights: call load_weights()/load_ckpt() first")
    if loss_applied is None:
        loss_applied = [k for k in ('image', 'identity', 'temporal', 'surf', 'distortion') if k != 'surf' or surfs is not None]
    applied = trainer.applied_keys(loss_applied)
    if 'surf' in applied and (surfs is None or surfs_dim is None):
        raise ValueError("the surf term needs surfs [n,2,Ns,2] and surfs_dim [n]")
    flip = 1 if channel_order == "bgr" else 0
    dev = device()
    to_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))).to(dev).contiguous()
    un, st = to_dev(unstable), to_dev(stable)
    if un.dim() != 4 or un.shape[3] != 3 or st.shape != un.shape:
        raise ValueError("unstable and stable clips must both be [N,h,w,3]")
    N, h, w, S = int(un.shape[0]), model.h, model.w, len(skip_length)
    _check_window(model, S)
    span = int(skip_length[-1])
    table = torch.from_numpy(teacher_forced_index_table(N, skip_length)).to(dev)
    n = N - span
    steps = n - 1
    if steps < 1:
        raise ValueError("a score needs two windows: more than %d frames, got %d" % (span + 1, N))
    fl = to_dev(flows).to(torch.float32)
    if tuple(fl.shape) != (n, h, w, 2):
        raise ValueError("flows must be [%d,%d,%d,2] (one per window, entry 0 unused), got %s" % (n, h, w, tuple(fl.shape)))
    if 'surf' in applied:
        sf, sd = to_dev(surfs).to(torch.float32), to_dev(surfs_dim).to(torch.float32).reshape(-1)
        if sf.dim() != 4 or sf.shape[0] != n or sf.shape[1] != 2 or sf.shape[3] != 2 or sd.numel() != n:
            raise ValueError("surfs must be [%d,2,Ns,2] and surfs_dim [%d]" % (n, n))
    if mask_H is None:
        Ht = None
    elif isinstance(mask_H, (str, torch.Generator)):
        Ht = _mask_homographies(mask_H, 2 * steps, dev).reshape(steps, 2, 8)
    else:
        Ht = torch.as_tensor(np.asarray(mask_H, dtype=np.float32) if not isinstance(mask_H, torch.Tensor) else mask_H)
        if tuple(Ht.shape) != (steps, 2, 8):
            raise ValueError("mask_H must be [%d,2,8] (the t-1 and the t draw of each step), got %s" % (steps, tuple(Ht.shape)))
        Ht = Ht.to(dev, torch.float32).contiguous()
    pool = torch.empty((2 * N, h, w, 3), dtype=torch.float32, device=dev)
    _frames_to_pool(un, pool[:N], h, w, flip, "unstable")
    _frames_to_pool(st, pool[N:], h, w, flip, "stable")
    V = torch.from_numpy(V_SRC).to(dev).unsqueeze(0)
    prec = model.precision if precision is None else precision
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    lo, hi = shard_range(steps, world, rank)
    keys = applied + ['total']
    sums = torch.zeros(len(keys), dtype=torch.float64)
    for b0 in range(lo, hi, batch):             # steps b0 .. b1-1, i.e. k = b0+1 .. b1: window k-1 = row b0 .. of the table
        b1 = min(hi, b0 + batch)
        b = b1 - b0
        if Ht is None:
            plane = torch.ones((2 * b, h, w), dtype=torch.float32, device=dev)
        else:
            plane = random_mask_plane(torch.cat([Ht[b0:b1, 0], Ht[b0:b1, 1]], 0).contiguous(), h, w)
        table2 = torch.cat([table[b0:b1], table[b0 + 1:b1 + 1]], 0).contiguous()      # ONE batch of 2 b: t-1 first
        F2 = model.locnet.forward_masked(pool, plane, table=table2, precision=prec).reshape(2 * b, model.param_dim, 2)
        values = dict(u_t_1=pool[span + b0:span + b1], u_t=pool[span + b0 + 1:span + b1 + 1],
                      s_t_1_gt=pool[N + span + b0:N + span + b1], s_t_gt=pool[N + span + b0 + 1:N + span + b1 + 1],
                      of_t=fl[b0 + 1:b1 + 1])
        if 'surf' in applied:
            values.update(surfs_t_1=sf[b0:b1], surfs_t=sf[b0 + 1:b1 + 1], surfs_dim_t_1=sd[b0:b1], surfs_dim_t=sd[b0 + 1:b1 + 1])
        loss = trainer.loss_terms(values, dict(F_t_1=F2[:b].contiguous(), F_t=F2[b:].contiguous(), V_src=V,
                                               num_control_points=model.num_control_points), applied, per_sample=True)
        trainer.add_total(loss, coefs)
        rows = torch.stack([loss[k].reshape(b) for k in keys], 1).to(torch.float64).cpu()   # [b, K+1], float32 values
        for r in range(b):                      # fixed order: step by step, as main.py:210 accumulates
            sums += rows[r]
    if world > 1:
        red = sums.to(dev) if dist.get_backend(group) == "nccl" else sums
        dist.all_reduce(red, op=dist.ReduceOp.SUM, group=group)
        sums = red.cpu()
    return collections.OrderedDict((k, float(sums[i]) / steps) for i, k in enumerate(keys))     # main.py:215
