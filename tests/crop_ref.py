"""NumPy reference of the crop (crop_kernels.hip, coupe.dvsg_amd.clip.crop_scan / crop_zoom): sampler A's validity predicate
in float32 op by op, the integer key, the per-frame scan, `free`, `crop_zoom`, and a float64 evaluation of the TPS map on a
zoomed grid.  `mut` names a simulated wrong kernel; the CPU tests require the reference to tell each from the right one."""
import numpy as np

F32 = np.float32
INT32_MAX = 2 ** 31 - 1
EPS32 = float(F32(1e-6))
MUTANTS = ("rows_past", "x_lt_W", "no_aspect")


def pixel_coords(xs, ys, H, W):
    """sample_a_load's float32 pixel coordinate ((x_s + 1) W) / 2: three separately rounded operations"""
    x = (((np.asarray(xs, dtype=F32) + F32(1.0)).astype(F32) * F32(W)).astype(F32) / F32(2.0)).astype(F32)
    y = (((np.asarray(ys, dtype=F32) + F32(1.0)).astype(F32) * F32(H)).astype(F32) / F32(2.0)).astype(F32)
    return x, y


def _index(v):
    """floorf, then f2i's guarded conversion (clamped to +-2^30 while still a float; NaN is the caller's)"""
    f = np.clip(np.floor(np.nan_to_num(v, nan=0.0)), F32(-1073741824.0), F32(1073741824.0))
    return f.astype(np.int64)


def valid(xs, ys, H, W, mut=None):
    """bool, the shape of xs: sampler A blends four distinct taps there -- (x1 - x0)(y1 - y0) == 1 after the clip"""
    x, y = pixel_coords(xs, ys, H, W)
    nan = np.isnan(x) | np.isnan(y)
    x0, y0 = _index(x), _index(y)
    hi_x = W if mut == "x_lt_W" else W - 1          # the wrong clip lets x in [W-1, W) through
    x0c, x1c = np.clip(x0, 0, hi_x), np.clip(x0 + 1, 0, hi_x)
    y0c, y1c = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    return ((x1c - x0c) * (y1c - y0c) == 1) & ~nan


def keys(out_h, out_w, mut=None):
    """int64 [out_h,out_w]: max(|2j - (w-1)| (h-1), |2i - (h-1)| (w-1))"""
    i = np.arange(out_h, dtype=np.int64)[:, None]
    j = np.arange(out_w, dtype=np.int64)[None, :]
    fx, fy = (1, 1) if mut == "no_aspect" else (out_h - 1, out_w - 1)
    return np.maximum(np.abs(2 * j - (out_w - 1)) * fx, np.abs(2 * i - (out_h - 1)) * fy)


def scan(xs, ys, H, W, out_h, out_w, mut=None, xs_past=None, ys_past=None):
    """(n_border, key_min) int64 [B] of source coordinates xs, ys [B, out_h * out_w] (any shape of that size) for a source
    of H x W.  mut == "rows_past": the rows of the last partial 4-row group behind out_h -- their coordinates come in
    xs_past, ys_past [B, r, out_w] -- are counted too, with the key of their row index."""
    xs = np.asarray(xs, dtype=F32).reshape(-1, out_h, out_w)
    ys = np.asarray(ys, dtype=F32).reshape(-1, out_h, out_w)
    bad = ~valid(xs, ys, H, W, mut)
    k = np.broadcast_to(keys(out_h, out_w, mut)[None], bad.shape)
    n = bad.reshape(bad.shape[0], -1).sum(1).astype(np.int64)
    kmin = np.where(bad, k, INT32_MAX).reshape(bad.shape[0], -1).min(1).astype(np.int64)
    if mut == "rows_past" and xs_past is not None and np.asarray(xs_past).size:
        r = np.asarray(xs_past).shape[1]
        badp = ~valid(xs_past, ys_past, H, W)
        i = np.arange(out_h, out_h + r, dtype=np.int64)[:, None]
        j = np.arange(out_w, dtype=np.int64)[None, :]
        kp = np.maximum(np.abs(2 * j - (out_w - 1)) * (out_h - 1), np.abs(2 * i - (out_h - 1)) * (out_w - 1))
        n = n + badp.reshape(badp.shape[0], -1).sum(1)
        kmin = np.minimum(kmin, np.where(badp, kp[None], INT32_MAX).reshape(badp.shape[0], -1).min(1))
    return n, kmin


def free(key_min, out_h, out_w):
    D = (out_h - 1) * (out_w - 1)
    return np.minimum(np.asarray(key_min, dtype=np.int64), D).astype(np.float64) / D


def crop_zoom(free_values, margin=None, crop_min=0.5, out_hw=None):
    """z = max(min(free) - margin, crop_min), at most 1, rounded once to float32; the default margin is one pixel of the
    shorter axis, 2 / (min(out_h, out_w) - 1)"""
    if margin is None:
        margin = 2.0 / (min(out_hw) - 1)
    z = max(float(np.min(np.asarray(free_values, dtype=np.float64))) - float(margin), float(crop_min))
    return F32(min(z, 1.0))


def linspace32(n):
    """tf.linspace(-1, 1, n) as the kernels form it: -1.0f + step * (float)i, step = 2.0f / (n - 1)"""
    step = F32(F32(2.0) / F32(n - 1)) if n > 1 else F32(0.0)
    return (F32(-1.0) + (step * np.arange(n, dtype=F32)).astype(F32)).astype(F32)


def zoomed_axes(out_h, out_w, z, rows=None):
    """(X [out_w], Y [rows]) float64: float64(float32(z)) times the float32 grid values, the product exact in float64"""
    z = np.float64(F32(z))
    i = np.arange(out_h) if rows is None else np.asarray(rows)
    step = F32(F32(2.0) / F32(out_h - 1)) if out_h > 1 else F32(0.0)
    yl = (F32(-1.0) + (step * i.astype(F32)).astype(F32)).astype(F32)
    return z * linspace32(out_w).astype(np.float64), z * yl.astype(np.float64)


def map_f64(T, coord, out_h, out_w, z=1.0, rows=None):
    """(x_s, y_s) float64 [B, rows, out_w]: the thin-plate-spline map (ThinPlateSpline.py:92-134) of float32 T [B,2,P+3] and
    float32 control points [B or 1,P,2] on the grid zoomed by z (scalar or [B]), every operation in float64"""
    T = np.asarray(T, dtype=np.float64)
    c = np.asarray(coord, dtype=F32).astype(np.float64)
    B, P = T.shape[0], T.shape[2] - 3
    zs = np.broadcast_to(np.asarray(z, dtype=F32).reshape(-1), (B,)) if np.ndim(z) else np.full(B, F32(z), dtype=F32)
    out = []
    for b in range(B):
        X, Y = zoomed_axes(out_h, out_w, zs[b], rows)
        X, Y = X[None, :], Y[:, None]
        cb = c[b % c.shape[0]]
        acc = [T[b, k, 0] + T[b, k, 1] * X + T[b, k, 2] * Y for k in range(2)]
        for q in range(P):
            d2 = np.square(X - cb[q, 0]) + np.square(Y - cb[q, 1])
            r = d2 * np.log(d2 + EPS32)
            for k in range(2):
                acc[k] = acc[k] + T[b, k, 3 + q] * r
        out.append(acc)
    out = np.asarray(out)
    return out[:, 0], out[:, 1]
