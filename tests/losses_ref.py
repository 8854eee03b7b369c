"""NumPy restatement of the reference's five test-time loss terms (trainer.py), written from its text for the tests.

`dtype=np.float64` gives the arithmetic yardstick; `dtype=np.float32` forms every per-element term in float32 op by op in
the reference's order and sums the terms in float64 (what tests/test_gpu_losses.py compares the kernels' sums with).
No product imports, no oracle imports: callers pass the warped tensors in."""
import numpy as np


def div_no_nan(a, b):
    """tf.div_no_nan: 0 where the divisor is 0."""
    a, b = np.asarray(a), np.asarray(b)
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.result_type(a, b))
    np.divide(a, b, out=out, where=(b != 0))
    return out


def masked_mse_sums(pred, gt, mask, dtype=np.float64):
    """trainer.py:234-237, 242: per sample (sum squared_difference(pred * mask, gt * mask), sum mask, sum |mask|), the
    terms in `dtype`, the sums in float64 (the squares are their own absolute values).  `mask` [B,H,W,C] or a plane [B,H,W] counted C times."""
    pred, gt, mask = (np.asarray(a, dtype=dtype) for a in (pred, gt, mask))
    if mask.ndim == pred.ndim - 1:
        mask = np.broadcast_to(mask[..., None], pred.shape)
    pm = pred * mask                      # :234
    gm = gt * mask                        # :235
    d = pm - gm
    sq = d * d                            # :237
    ax = tuple(range(1, pred.ndim))
    num = sq.astype(np.float64).sum(axis=ax)
    den = mask.astype(np.float64).sum(axis=ax)   # :242
    return num, den, np.abs(mask).astype(np.float64).sum(axis=ax)


def masked_MSE(pred, gt, mask, dtype=np.float64):
    """trainer.py:233-243."""
    num, den, _ = masked_mse_sums(pred, gt, mask, dtype)
    return float(np.mean(div_no_nan(num, den)))   # :242-243


def temporal_loss(pred_warped, gt, mask_pred_warped, mask_gt, dtype=np.float64):
    """trainer.py:245-250 behind the two tf_warp calls, which the caller makes."""
    m = np.asarray(mask_pred_warped, dtype=dtype) * np.asarray(mask_gt, dtype=dtype)   # :250
    return masked_MSE(pred_warped, gt, m, dtype)


def identity_loss(F, dtype=np.float64):
    """trainer.py:105-106, one of its two summands: tl.cost.absolute_difference_error(F, 0, is_mean=True)."""
    F = np.asarray(F, dtype=dtype)
    return float(np.mean(np.mean(np.abs(F - 0), axis=(1, 2))))


def _sp_term(v_src, v_src_0, v_src_1, v, v_0, v_1):
    """get_sp_term, trainer.py:253-267."""
    s = (np.sqrt(np.sum((v_src - v_src_1) ** 2, axis=3)) / np.sqrt(np.sum((v_src_0 - v_src_1) ** 2, axis=3)))[..., None]  # :254
    M_rot = np.array([[0., 1.], [-1., 0.]], dtype=v.dtype)     # :255
    v_0_1 = v_0 - v_1                                          # :256
    R = np.einsum('ij,bhwj->bhwi', M_rot, v_0_1)               # :259-264
    return np.mean(np.sum((v - v_1 - s * R) ** 2, axis=3), axis=(1, 2))   # :266


def distortion_per_sample(V_src, V, n, dtype=np.float64):
    Vs = (np.asarray(V_src, dtype=dtype).reshape(-1, n, n, 2) + 1.0) / 2.0   # :272
    Vv = Vs + np.asarray(V, dtype=dtype).reshape(-1, n, n, 2)                # :273
    a = lambda X: X[:, :-1, :-1]   # noqa: E731  (i, j)
    b = lambda X: X[:, :-1, 1:]    # noqa: E731  (i, j+1)
    c = lambda X: X[:, 1:, :-1]    # noqa: E731  (i+1, j)
    d = lambda X: X[:, 1:, 1:]     # noqa: E731  (i+1, j+1)
    t1 = _sp_term(a(Vs), d(Vs), c(Vs), a(Vv), d(Vv), c(Vv))   # :275-285
    t2 = _sp_term(b(Vs), c(Vs), d(Vs), b(Vv), c(Vv), d(Vv))   # :287-297
    t3 = _sp_term(c(Vs), b(Vs), a(Vs), c(Vv), b(Vv), a(Vv))   # :299-309
    t4 = _sp_term(d(Vs), a(Vs), b(Vs), d(Vv), a(Vv), b(Vv))   # :311-321
    return (t1 + t2 + t3 + t4) / 4.0


def distortion_loss(V_src, V, n, dtype=np.float64):
    """trainer.py:252-323."""
    return float(np.mean(distortion_per_sample(V_src, V, n, dtype)))   # :323


def surf_sums(surf, x_offset, y_offset, w, h, dtype=np.float64):
    """trainer.py:364-383: per sample sum of squared differences (float64 sum of `dtype` terms), and the gathered [B,N,2]."""
    surf = np.asarray(surf)
    B = surf.shape[0]
    xo = np.concatenate([np.asarray(x_offset, dtype=dtype).reshape(B, -1), -np.ones((B, 1), dtype)], axis=1)   # :364
    yo = np.concatenate([np.asarray(y_offset, dtype=dtype).reshape(B, -1), -np.ones((B, 1), dtype)], axis=1)   # :365
    un = surf[:, 0].astype(np.float32).astype(dtype)                   # :368
    ux = (un[:, :, 0] / dtype(w - 1)) * dtype(2) - dtype(1)            # :369
    uy = (un[:, :, 1] / dtype(h - 1)) * dtype(2) - dtype(1)            # :370
    st = surf[:, 1].astype(np.float32)                                 # :374-376
    idx = (st[:, :, 0] + st[:, :, 1] * np.float32(w)).astype(np.int32)   # :377
    tx = np.take_along_axis(xo, idx, axis=1)                           # :379
    ty = np.take_along_axis(yo, idx, axis=1)                           # :380
    dx, dy = tx - ux, ty - uy
    sq = np.stack([dx * dx, dy * dy], axis=2)                          # :383
    return sq.astype(np.float64).sum(axis=(1, 2)), np.stack([tx, ty], axis=2)


def get_surf_loss(surf, x_offset, y_offset, max_dim_per_batch, w, h, dtype=np.float64):
    """trainer.py:363-386."""
    num, _ = surf_sums(surf, x_offset, y_offset, w, h, dtype)
    return float(np.mean(div_no_nan(num, np.asarray(max_dim_per_batch, dtype=np.float64).reshape(-1))))   # :384-386
