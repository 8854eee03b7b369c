"""Drop-in for the test-time losses of the reference's trainer.py on MI355X: the score that ranks checkpoints.

Reference surface kept (trainer.py:95-123, 233-323, 363-386), names and argument order:

    masked_MSE(pred, gt, mask)
    temporal_loss(pred, gt, mask_pred, mask_gt, of, h, w)
    distortion_loss(V_src, V, num_control_points)
    get_surf_loss(surf, T, coord, max_dim_per_batch, batch_size, w, h)
    build_loss_train(inputs, outputs, loss_applied, coefs)

Forward only: no gradients, no optimiser, no coefficient schedule.  The `cor` term needs correlationNet (a ResNet-v2-101)
and raises NotImplementedError.  Compute: the `dvsg_loss_*` entries of include/dvsg_amd.h -- one fused kernel per term, sums
in float64 in a fixed order.  Torch tensors in -> 0-dim torch tensors out; NumPy in -> NumPy float32 out.

Two departures from the reference's signatures, both because a tensor of the graph never exists here:
  * masks are PLANES [B,H,W].  A [B,H,W,3] mask is accepted by temporal_loss and its first channel taken (the reference's
    three channels are the warp of the same ones and equal each other); `stats['mask3']` counts how often that happened.
  * get_surf_loss takes the thin-plate-spline map itself -- T [B,2,P+3] and coord [B,P,2] -- where the reference takes
    x_offset / y_offset: the map is evaluated at the SURF points only.
"""
import collections

import numpy as np
import torch

from . import _lib
from .ThinPlateSpline import _solve
from ._tensor import as_dev, empty, is_host, ptr, stream

LOSS_KEYS = ('image', 'identity', 'temporal', 'surf', 'cor', 'distortion')   # trainer.py:100-117, in the dict's order
# what this module's calls allocated: 'mask3' counts [B,H,W,3] masks (built or taken apart), 'pred' the optional
# [B,H,W,3] prediction outputs of image_loss; tests assert on these instead of timing
stats = collections.Counter()


def _out(t, ref):
    return np.float32(t.item()) if is_host(ref) else t.reshape(())


def _workspace(B, H, W, like):
    import ctypes
    n = ctypes.c_size_t()
    _lib.call("dvsg_loss_workspace_bytes", B, H, W, ctypes.byref(n))
    return torch.empty((n.value + 7) // 8, dtype=torch.float64, device=like.device)


def _plane(mask, B, H, W, what):
    m = as_dev(mask, what)
    if m.dim() == 4 and m.shape[3] == 3:
        stats['mask3'] += 1
        if not (torch.equal(m[..., 0], m[..., 1]) and torch.equal(m[..., 0], m[..., 2])):
            raise ValueError("%s [B,H,W,3] must hold three equal channels (the kernels take one plane)" % what)
        m = m[..., 0].contiguous()
    if tuple(m.shape) != (B, H, W):
        raise ValueError("%s must be a plane [B,H,W] (or [B,H,W,3] with equal channels)" % what)
    return m


def masked_mse_terms(pred, gt, mask):
    """`masked_MSE` with everything it computes: (mean [1], per_sample [B], sums [B,2] float64)."""
    p, g, m = as_dev(pred, "pred"), as_dev(gt, "gt"), as_dev(mask, "mask")
    if p.dim() != 4 or g.shape != p.shape:
        raise ValueError("pred and gt must be [B,H,W,C] of one shape")
    B, H, W, C = p.shape
    if tuple(m.shape) == (B, H, W):
        plane = 1
    elif m.shape == p.shape:
        plane = 0
    else:
        raise ValueError("mask must be [B,H,W,C] like pred, or a plane [B,H,W]")
    ps, mean = empty((B,), p), empty((1,), p)
    sums = torch.empty((B, 2), dtype=torch.float64, device=p.device)
    ws = _workspace(B, H, W, p)
    _lib.call("dvsg_loss_masked_mse_f32", ptr(p), ptr(g), ptr(m), B, H, W, C, plane, ptr(ps), ptr(mean), ptr(sums),
              ptr(ws), ws.numel() * 8, stream())
    return mean, ps, sums


def masked_MSE(pred, gt, mask, name=None):
    """trainer.py:233-243."""
    return _out(masked_mse_terms(pred, gt, mask)[0], pred)


def temporal_terms(pred, gt, mask_pred, mask_gt, of):
    p, g, f = as_dev(pred, "pred"), as_dev(gt, "gt"), as_dev(of, "of")
    if p.dim() != 4 or p.shape[3] != 3 or g.shape != p.shape:
        raise ValueError("pred and gt must be [B,H,W,3]")
    B, H, W, _ = p.shape
    if tuple(f.shape) != (B, H, W, 2):
        raise ValueError("of must be [B,H,W,2] in pixels")
    mp, mg = _plane(mask_pred, B, H, W, "mask_pred"), _plane(mask_gt, B, H, W, "mask_gt")
    ps, mean = empty((B,), p), empty((1,), p)
    sums = torch.empty((B, 2), dtype=torch.float64, device=p.device)
    ws = _workspace(B, H, W, p)
    _lib.call("dvsg_loss_temporal_f32", ptr(p), ptr(mp), ptr(f), ptr(g), ptr(mg), B, H, W, ptr(ps), ptr(mean), ptr(sums),
              ptr(ws), ws.numel() * 8, stream())
    return mean, ps, sums


def temporal_loss(pred, gt, mask_pred, mask_gt, of, h, w, name=None):
    """trainer.py:245-250; h, w must be the frames' size (tf_warp's out_height / out_width there too)."""
    if tuple(np.shape(pred)[1:3]) != (int(h), int(w)):
        raise ValueError("h, w must equal the frame size %s" % (tuple(np.shape(pred)[1:3]),))
    return _out(temporal_terms(pred, gt, mask_pred, mask_gt, of)[0], pred)


def grid_terms(V_src, V, num_control_points):
    """identity and distortion of one frame: (identity_mean, distortion_mean, identity [B], distortion [B])."""
    n = int(num_control_points)
    F = as_dev(V, "V").reshape(-1, n * n, 2)
    B = F.shape[0]
    vs = as_dev(V_src, "V_src").reshape(-1, n * n, 2)
    if vs.shape[0] == 1 and B > 1:
        vs = vs.expand(B, -1, -1).contiguous()
    if vs.shape[0] != B:
        raise ValueError("V_src must be [B,%d,2] with the batch of V" % (n * n))
    ident, dist = empty((B,), F), empty((B,), F)
    im, dm = empty((1,), F), empty((1,), F)
    _lib.call("dvsg_loss_grid_f32", ptr(vs), ptr(F), B, n, ptr(ident), ptr(im), ptr(dist), ptr(dm), stream())
    return im, dm, ident, dist


def distortion_loss(V_src, V, num_control_points, name=None):
    """trainer.py:252-323, as written (0.125 at V = 0 on the 5 x 5 grid: see include/dvsg_amd.h)."""
    return _out(grid_terms(V_src, V, num_control_points)[1], V)


def identity_loss(F):
    """tl.cost.absolute_difference_error(F, zeros, is_mean=True) of trainer.py:105-106."""
    F_ = as_dev(F, "F")
    n = int(round(F_.shape[1] ** 0.5))
    return _out(grid_terms(torch.zeros_like(F_), F_, n)[0], F)


def solve_T(V_src, F):
    """T [B,2,P+3] of ThinPlateSpline(., V_src, F, .) (ThinPlateSpline.py:143-166)."""
    c, v = as_dev(V_src, "V_src"), as_dev(F, "F")
    B, P, _ = v.shape
    if c.shape[0] == 1 and B > 1:
        c = c.expand(B, -1, -1).contiguous()
    T = empty((B, 2, P + 3), v)
    _solve(c, v, True, B, P, T)
    return c, T


def image_terms(u, gt, coord, T, want_pred=False):
    """masked_MSE(TPS(u), gt, TPS(ones)) fused: (mean, per_sample, sums, pred | None, mask plane | None)."""
    U, g = as_dev(u, "u"), as_dev(gt, "gt")
    if U.dim() != 4 or U.shape[3] != 3 or g.shape != U.shape:
        raise ValueError("u and gt must be [B,H,W,3] of one shape")
    B, H, W, _ = U.shape
    P = coord.shape[1]
    ps, mean = empty((B,), U), empty((1,), U)
    sums = torch.empty((B, 2), dtype=torch.float64, device=U.device)
    pred = mask = None
    if want_pred:
        stats['pred'] += 1
        pred, mask = empty((B, H, W, 3), U), empty((B, H, W), U)
    ws = _workspace(B, H, W, U)
    _lib.call("dvsg_loss_image_f32", ptr(U), ptr(coord), ptr(T), ptr(g), B, H, W, P, ptr(pred), ptr(mask), ptr(ps), ptr(mean),
              ptr(sums), ptr(ws), ws.numel() * 8, stream())
    return mean, ps, sums, pred, mask


def surf_terms(surf, T, coord, max_dim_per_batch, w, h, want_coords=False):
    s = surf if isinstance(surf, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(surf))
    s = as_dev(s.to(torch.float32), "surf")     # int32 in the reference's feed (model.py:51), cast at trainer.py:366: exact
    if s.dim() != 4 or s.shape[1] != 2 or s.shape[3] != 2:
        raise ValueError("surf must be [B,2,N,2]")
    B, _, N, _ = s.shape
    Tt, c = as_dev(T, "T"), as_dev(coord, "coord")
    P = c.shape[1]
    if tuple(Tt.shape) != (B, 2, P + 3) or tuple(c.shape) != (B, P, 2):
        raise ValueError("T must be [B,2,P+3] and coord [B,P,2] with the batch of surf")
    d = as_dev(max_dim_per_batch, "max_dim_per_batch").reshape(-1)
    if d.numel() != B:
        raise ValueError("max_dim_per_batch must hold one value per sample")
    ps, mean = empty((B,), s), empty((1,), s)
    sums = torch.empty((B,), dtype=torch.float64, device=s.device)
    coords = empty((B, N, 2), s) if want_coords else None
    _lib.call("dvsg_loss_surf_f32", ptr(s), ptr(d), ptr(c), ptr(Tt), B, N, int(h), int(w), P, ptr(coords), ptr(ps), ptr(mean),
              ptr(sums), stream())
    return mean, ps, sums, coords


def get_surf_loss(surf, T, coord, max_dim_per_batch, batch_size, w, h):
    """trainer.py:363-386 with (T, coord) in the place of (x_offset, y_offset)."""
    return _out(surf_terms(surf, T, coord, max_dim_per_batch, w, h)[0], surf)


def loss_terms(inputs, outputs, applied, per_sample=False):
    """The applied terms of trainer.py:100-117 on VALUES, in the reference's order, without `total`: 1-element batch means, or
    -- per_sample -- the [B] values whose batch mean they are (what a driver that averages over steps adds up)."""
    n = int(outputs['num_control_points'])
    i = 1 if per_sample else 0
    loss = collections.OrderedDict()
    if any(k in applied for k in ('image', 'temporal', 'surf')):
        c_t, T_t = solve_T(outputs['V_src'], outputs['F_t'])
        c_1, T_1 = solve_T(outputs['V_src'], outputs['F_t_1'])
    if 'image' in applied or 'temporal' in applied:
        keep = 'temporal' in applied
        r1 = image_terms(inputs['u_t_1'], inputs['s_t_1_gt'], c_1, T_1, keep)
        r0 = image_terms(inputs['u_t'], inputs['s_t_gt'], c_t, T_t, keep)
        if 'image' in applied:
            loss['image'] = r1[i] + r0[i]                                                           # :100-101
    if 'identity' in applied or 'distortion' in applied:
        g0 = grid_terms(outputs['V_src'], outputs['F_t'], n)
        g1 = grid_terms(outputs['V_src'], outputs['F_t_1'], n)
        if 'identity' in applied:
            loss['identity'] = g0[2 * i] + g1[2 * i]                                                # :105-106
    if 'temporal' in applied:
        loss['temporal'] = temporal_terms(r0[3], r1[3], r0[4], r1[4], inputs['of_t'])[i]            # :108
    if 'surf' in applied:
        H, W = as_dev(inputs['u_t']).shape[1:3]
        s1 = surf_terms(inputs['surfs_t_1'], T_1, c_1, inputs['surfs_dim_t_1'], W, H)[i]
        s0 = surf_terms(inputs['surfs_t'], T_t, c_t, inputs['surfs_dim_t'], W, H)[i]
        loss['surf'] = s1 + s0                                                                      # :110-111
    if 'distortion' in applied:
        loss['distortion'] = g1[1 + 2 * i] + g0[1 + 2 * i]                                          # :116-117
    return loss


def add_total(loss, coefs=None):
    """loss['total'] = sum coefs[k] * loss[k] in the dict's order (:120; coefs default to 1)."""
    coefs = coefs or {}
    total = None
    for k, v in list(loss.items()):
        term = v * float(coefs.get(k, 1.0))
        total = term if total is None else total + term
    loss['total'] = total
    return loss


def applied_keys(loss_applied):
    unknown = [k for k in loss_applied if k not in LOSS_KEYS]
    if unknown:
        raise KeyError("unknown loss keys %s: trainer.py:100-117 builds %s" % (unknown, list(LOSS_KEYS)))
    applied = [k for k in LOSS_KEYS if k in loss_applied]
    if 'cor' in applied:
        raise NotImplementedError("loss['cor'] needs correlationNet (trainer.py:113-114): not built")
    return applied


def build_loss_train(inputs, outputs, loss_applied=('image', 'identity', 'temporal', 'surf', 'distortion'), coefs=None):
    """trainer.py:95-123.  Returns an OrderedDict of the applied terms in the reference's order, and `total` =
    sum coefs[k] * loss[k] (:120; coefs default to 1).

    On the GRAPH -- `inputs`, `outputs` of `StabNet.init_train_inputs` / `get_train_model(False)` -- the values are fetches:
    `Session.run(loss, feed)` (a dict, as main.py:208 runs `trainer.loss_test`) or of any of its entries evaluates the
    localisation net on the two masked windows as one batch and then the fused entries below.
    On VALUES -- `inputs` holds u_t, u_t_1, s_t_gt, s_t_1_gt, of_t, surfs_t, surfs_t_1, surfs_dim_t, surfs_dim_t_1
    (model.py:36-58), `outputs` F_t, F_t_1, V_src and num_control_points -- the terms are computed at once.
    Either way the warped frames and masks the reference's dict carries are produced inside the fused image term and kept
    only when the temporal term needs them; a three-channel mask is never built."""
    applied = applied_keys(loss_applied)
    from .model import Fetch
    if isinstance(outputs['F_t'], Fetch):
        model = outputs['F_t'].model
        model.loss_applied, model.loss_coefs = applied, dict(coefs or {})
        return collections.OrderedDict((k, Fetch(model, 'loss/' + k)) for k in applied + ['total'])
    host = is_host(outputs['F_t'])
    loss = loss_terms(inputs, outputs, applied)
    for k in loss:
        loss[k] = loss[k].reshape(())
    add_total(loss, coefs)
    if host:
        for k in loss:
            loss[k] = np.float32(loss[k].item())
    return loss
