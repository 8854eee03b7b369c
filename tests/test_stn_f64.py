"""Samplers B and C, the STN grids, the mask plane and the strip kernel of warp_kernels.hip pinned to float64, every pixel.

No pixel is masked or left out anywhere in this file.  u = 2^-24; every bound carries the factor SECOND = 1.01 of
test_tps_f64.py for the second-order terms ((1 + u)^k - 1 <= 1.01 k u, k <= 70); nothing here was fitted to a GPU result.
x_t, y_t are tf.linspace's own float32 operations on both sides (bit-identical inputs, -1 + step j).

1.  Grids (stn_kernel<kAffine | kProjective | kElastic>, x_s / y_s; the image-less call and the call with an image must
    write the same bits).
    Affine: fl(fl(fl(t0 x_t) + fl(t1 y_t)) + t2), the oracle's seq_matmul_small in k order: bit equality with
    oracle.spatial_transformer.AffineTransformer._transform, and against float64 the two products pass three roundings
    each (product, two sums), t2 one:   E_aff = u (3 |t0 x_t| + 3 |t1 y_t| + |t2|).
    Projective: xq, yq, zq are three such sums.  THE DIVISION IS CORRECTLY ROUNDED: build.sh passes no -ffast-math and
    hipcc's default is -fhip-fp32-correctly-rounded-divide-sqrt; in the shipped object every `/` of
    stn_kernel<kProjective, *> and mask_plane_kernel is the IEEE sequence v_div_scale_f32 x 2, v_rcp_f32, three v_fma_f32 +
    two v_fmac_f32 (Newton steps and residual), v_div_fmas_f32, v_div_fixup_f32 -- 4 divisions in the two-row kernel (8, 4, 12,
    8, 4, 4 of those instructions), 2 in the mask plane; a bare v_rcp_f32 + v_mul_f32 quotient does not occur.  So x_s, y_s
    are asserted bit-equal to the oracle's _transform (np.array_equal) and nothing else is tightened; zq == 0 gives
    exactly 0 (tf.div_no_nan), asserted on the column j = 0 of theta[6] = 1, theta[7] = 0.  The float64 quotient is held
    too, where it is defined: |x_s - xq/zq| <= (E_x + |q| E_z) / (|zq| - E_z) + u (|q| + that), infinite where |zq| <= E_z
    (a sign change of zq inside the frame has such pixels; bit equality with the oracle still holds there).
    Elastic: coefficients = theta @ L_inv, acc = th_0 L_0q, then acc + th_k L_kq: a term passes at most n roundings,
        E_c = n u sum_k |th_k L_kq|.
    The kernel keeps the coefficients in LDS and never writes them, so on the GPU this link is asserted through the map
    (below) and, separately, in the CPU replay.  The map: dx, dy one rounding each; dx dx, dy dy 3u each; rsq (1 + 4u), all
    terms positive; ln moves by 4u absolutely; logf (OCML, no fast-math) within 1 ulp = 2u |ln rsq|; rsq logf rounds once:
        Dr_k = u (4 rsq (|L| + 1) + 3 |r|),  L = ln rsq, r = rsq L;  rsq == 0 gives exactly 0 on both sides
    (a difference of two float32 values is 0 only if they are equal), and the accumulation (c0 x_t + c1 y_t) + c2, then
    + c_{3+k} u_k in k order, rounds each of its n + 3 terms at most n + 3 times:
        E_map = sum_k |c_k| Dr_k + (n + 3) u S,   S = |c0 x_t| + |c1 y_t| + |c2| + sum_k |c_{3+k} r_k|.
    Asserted twice on the GPU: against the float64 map of the float32 coefficients of the replay (the kernel's, if it
    does what its text says; E_map alone), and against the float64 map of the float64 coefficients with
    E_map(|c| + E_c) + sum_k E_c,k |basis_k|, which does not depend on the replay.

2.  Sampler B (stn_kernel<kCoords>, padded_geom + sample_padded_blend) at given float32 coordinates.  The pixel coordinate
    x = ((x_s + 1) / 2) (W - 1), the clamp to [-1, W] and the + 1 into the zero-ringed image are float32 operations that
    the reference restates in float32 (three roundings; the clamp is exact), so kernel and reference always pick the
    same cell.  From the float32 x the weights' factors are exact in float64, and in the kernel x - x0 is exact (same
    binade or Sterbenz) and x1 - x rounds at most once (only in the cell [0, 1)): a factor once, the weight once, the
    product once, and the first term passes three additions:
        ref = sum_i w_i I_i,   |out - ref| <= g u sum_i |w_i| |I_i| + 4 x 2^-126,   g = 2 + 1 + 1 + 3 = 7 = G_BLEND.
    The extra + 1 and the (x + 1) / 2 (W - 1) scale sit in front of the float32 x that both sides share; they add
    nothing to g.  Bit equality with oracle.bilinear_interp / padded_bilinear is asserted as well.  The taps on the ring
    read 0 (never the clamped pixel), which the frame "corners" (only the four corners and the last row and column
    non-zero) shows.  NaN coordinates are out of scope: NumPy's clip propagates NaN, the kernel's fmaxf(NaN, -1) is -1 by
    definition.  +-Inf and +-3e38 are in scope wherever the scale does not form Inf x 0 (W, H >= 2).

3.  Sampler C (dvsg_flow_warp_f32): x = j + flow_x in float32 on both sides, then bound 2.  flow_tiled = 0 (gather
    kernel), 1 and 2 (strip kernel, two dispatch orders) are compared bit for bit with each other AND with oracle.tf_warp
    AND held to the float64 bound at every shape, the multi-band ones included.  SEAMS restates the launch formula of
    dvsg_flow_warp_f32 (a CPU test recomputes it and checks the formula's text in the source).

4.  The mask plane (mask_plane_kernel): bound 2 on an all-ones image at link 1's float32 coordinates; bit for bit with
    stn_kernel<kProjective, 1> on ones and (the division being correctly rounded) with the oracle.

CPU tests: float32 NumPy replays of the grids and of padded_geom + blend pass the same checking functions at every case up
to 72 x 128; twelve simulated wrong kernels are each rejected with a stated floor (MUTANT_FLOOR).  Two readings are fixed
here: "weights taken after the clip" forms the weights from the tap indices clamped into the image (sampler A's way), since
moving padded_geom's own min() in front of the weights changes no value -- the min() acts only at x == W exactly, where
both x taps lie on the zero ring; and "the upper index not min()-ed" reads one element past the ringed image, modelled as
NaN (0 x NaN = NaN) for the same reason.

Measured on one MI355X (profiles/r09_stn_f64.log; worst |got - ref| / bound; the 92 GPU cases of this file run in 5 s):
    grids        affine 0.14-0.85, projective up to 0.79 (0 values off the oracle's bits), elastic 0.007-0.37 of E_map and
                 0.002-0.10 of the chained bound
    sampler B    up to 0.33 at given coordinates, up to 0.50 in the image calls of the grids
    sampler C    up to 0.51; flow_tiled 0, 1, 2 and the oracle bit-equal on all 53 million values
    mask plane   up to 0.22
No kernel defect was found.  Mutations of the real kernels on a scratch copy: DESIGN.md section 5.0e.
"""
import os
import re

import numpy as np
import pytest

import test_conv_gemm_f64 as f64
import test_tps_f64 as tps

Guarded, TINY = f64.Guarded, f64.TINY
F32, U24, SECOND, G_BLEND = tps.F32, tps.U24, tps.SECOND, tps.G_BLEND
check_grid = tps.check_grid

HERE = os.path.dirname(os.path.abspath(__file__))
WARP_SRC = os.path.join(os.path.dirname(HERE), "coupe", "dvsg_amd", "csrc", "warp_kernels.hip")
PPT_GRID, PPT_MEM = 2, 4                          # rows per thread: grid sources / flow and explicit coordinates


def _lin(n):
    from oracle.tfops import tf_linspace
    return tf_linspace(-1.0, 1.0, n)


def _xy64(oh, ow):
    return _lin(ow).astype(np.float64)[None, None, :], _lin(oh).astype(np.float64)[None, :, None]


def _xy32(oh, ow):
    return _lin(ow)[None, None, :], _lin(oh)[None, :, None]


# ---------------------------------------------------------------------------------------------------------------------
# link 1: grids

def _aff64(t, X, Y):
    """float64 value and bound of fl(fl(fl(t0 X) + fl(t1 Y)) + t2), t [B,3]"""
    t = np.asarray(t, dtype=F32).astype(np.float64)
    p0, p1, t2 = t[:, 0, None, None] * X, t[:, 1, None, None] * Y, t[:, 2, None, None]
    return p0 + p1 + t2, SECOND * U24 * (3.0 * np.abs(p0) + 3.0 * np.abs(p1) + np.abs(t2))


def _aff32(t, X, Y):
    t = np.asarray(t, dtype=F32)
    s = ((t[:, 0, None, None] * X).astype(F32) + (t[:, 1, None, None] * Y).astype(F32)).astype(F32)
    return (s + t[:, 2, None, None]).astype(F32)


def affine_reference(theta, oh, ow):
    """(ref, E) [B,2,oh,ow] float64 for theta [B,6] float32"""
    X, Y = _xy64(oh, ow)
    th = np.asarray(theta, dtype=F32).reshape(-1, 2, 3)
    a, b = _aff64(th[:, 0], X, Y), _aff64(th[:, 1], X, Y)
    return np.stack([a[0], b[0]], 1), np.stack([a[1], b[1]], 1)


def replay_affine(theta, oh, ow, mut=None):
    X, Y = _xy32(oh, ow)
    th = np.asarray(theta, dtype=F32).reshape(-1, 2, 3)
    if mut == "affine_rows_swapped":
        th = th[:, ::-1]
    return _aff32(th[:, 0], X, Y), _aff32(th[:, 1], X, Y)


def _theta9(theta):
    th = np.asarray(theta, dtype=F32).reshape(-1, 8)
    return np.concatenate([th, np.ones((th.shape[0], 1), dtype=F32)], 1).reshape(-1, 3, 3)


def projective_reference(theta, oh, ow):
    """(ref, E) [B,2,oh,ow]: the float64 quotient; where the float32 zq is 0 the value is exactly 0 (E = 0); where
    |zq| <= E_z the quotient is not defined to any precision (E = inf)"""
    X, Y = _xy64(oh, ow)
    th = _theta9(theta)
    (xq, Ex), (yq, Ey), (zq, Ez) = (_aff64(th[:, r], X, Y) for r in range(3))
    X32, Y32 = _xy32(oh, ow)
    z32 = _aff32(th[:, 2], X32, Y32)
    ref, E = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for q, Eq in ((xq, Ex), (yq, Ey)):
            v = q / zq
            e = (Eq + np.abs(v) * Ez) / (np.abs(zq) - Ez)
            e = SECOND * (e + U24 * (np.abs(v) + e))
            e = np.where(np.abs(zq) > Ez, e, np.inf)
            ref.append(np.where(z32 == 0, 0.0, np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)))
            E.append(np.where(z32 == 0, 0.0, e))
    return np.stack(ref, 1), np.stack(E, 1)


def replay_projective(theta, oh, ow, mut=None):
    X, Y = _xy32(oh, ow)
    th = _theta9(theta)
    xq, yq, zq = (_aff32(th[:, r], X, Y) for r in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        if mut == "zq0_gives_inf":
            return (xq / zq).astype(F32), (yq / zq).astype(F32)
        nz = zq != 0
        safe = np.where(nz, zq, F32(1))
        return np.where(nz, (xq / safe).astype(F32), F32(0)), np.where(nz, (yq / safe).astype(F32), F32(0))


_ELASTIC = {}


def elastic_constants(g):
    """(source_points [2,n], L_inv [n,n+3]) float32 of the library's host function (no GPU involved)"""
    from coupe.dvsg_amd import _lib
    if g not in _ELASTIC:
        n = g * g
        src, linv = np.empty((2, n), dtype=F32), np.empty((n, n + 3), dtype=F32)
        _lib.call("dvsg_elastic_constants_f32", g, src.ctypes.data, linv.ctypes.data)
        _ELASTIC[g] = (src, linv)
    return _ELASTIC[g]


def elastic_theta(g, B, scale, seed):
    src, _ = elastic_constants(g)
    v = np.random.default_rng(seed).standard_normal((B, 2, g * g)) * scale
    return (src[None] + v.astype(F32)).astype(F32)


def coeff_reference(theta, L_inv):
    """(c64, E_c) [B,2,n+3] of float32 theta [B,2,n] and L_inv [n,n+3]"""
    t, L = np.asarray(theta, dtype=F32).astype(np.float64), np.asarray(L_inv, dtype=F32).astype(np.float64)
    return t @ L, SECOND * t.shape[2] * U24 * (np.abs(t) @ np.abs(L))


def replay_coeff(theta, L_inv, mut=None):
    t, L = np.asarray(theta, dtype=F32), np.asarray(L_inv, dtype=F32)
    acc = (t[:, :, 0, None] * L[None, None, 0]).astype(F32)
    for k in range(1, t.shape[2]):
        acc = (acc + (t[:, :, k, None] * L[None, None, k]).astype(F32)).astype(F32)
    return acc


def elastic_reference(c, Ec, src, oh, ow):
    """(ref, E) [B,2,oh,ow]: the float64 map of coefficients c [B,2,n+3] known to within Ec (0: the float32 values)"""
    c = np.asarray(c).astype(np.float64)
    Ec = np.zeros_like(c) if Ec is None else Ec
    s = np.asarray(src, dtype=F32).astype(np.float64)
    n = s.shape[1]
    X, Y = _xy64(oh, ow)
    X, Y = X[None], Y[None]                                                # [1,1,*,*] against c[..., k, None, None] [B,2,1,1]
    ca = np.abs(c) + Ec
    col = lambda a, k: a[:, :, k, None, None]
    acc = col(c, 0) * X + col(c, 1) * Y + col(c, 2)
    S = col(ca, 0) * np.abs(X) + col(ca, 1) * np.abs(Y) + col(ca, 2)
    Cb = col(Ec, 0) * np.abs(X) + col(Ec, 1) * np.abs(Y) + col(Ec, 2)
    D = 0.0
    for k in range(n):
        rsq = np.square(X - s[0, k]) + np.square(Y - s[1, k])
        with np.errstate(divide="ignore", invalid="ignore"):
            L = np.where(rsq > 0, np.log(np.where(rsq > 0, rsq, 1.0)), 0.0)
        r = rsq * L
        acc = acc + col(c, 3 + k) * r
        S = S + col(ca, 3 + k) * np.abs(r)
        D = D + col(ca, 3 + k) * U24 * (4.0 * rsq * (np.abs(L) + 1.0) + 3.0 * np.abs(r))
        Cb = Cb + col(Ec, 3 + k) * np.abs(r)
    return acc, Cb + SECOND * (D + (n + 3) * U24 * S)


def replay_elastic(c, src, oh, ow, mut=None):
    """stn_kernel<kElastic>'s map in NumPy float32, one rounding per operation, ln correctly rounded"""
    c, s = np.asarray(c, dtype=F32), np.asarray(src, dtype=F32)
    X, Y = _xy32(oh, ow)
    X, Y = X[None], Y[None]
    col = lambda k: c[:, :, k, None, None]
    acc = (((col(0) * X).astype(F32) + (col(1) * Y).astype(F32)).astype(F32) + col(2)).astype(F32)
    acc = acc + np.zeros((1, 1, oh, ow), dtype=F32)
    for k in range(s.shape[1]):
        dx, dy = (X - s[0, k]).astype(F32), (Y - s[1, k]).astype(F32)
        rsq = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = (np.log2 if mut == "log2_for_ln" else np.log)(rsq.astype(np.float64)).astype(F32)
            u = (rsq * lg).astype(F32)                                     # 0 x -inf = NaN where rsq == 0
        if mut != "rsq0_gives_nan":
            u = np.where(rsq == 0, F32(0), u)
        acc = (acc + (col(3 + k) * u).astype(F32)).astype(F32)
    if mut == "last_row_dropped" and oh % PPT_GRID:
        acc = acc.copy()
        acc[:, :, oh - 1] = np.nan                                         # the sentinel of a row that was never written
    return acc[:, 0], acc[:, 1]


# ---------------------------------------------------------------------------------------------------------------------
# links 2-4: padded_geom + blend

def stn_pixel(xs, ys, H, W, mut=None):
    """stn_kernel's `x = ((xs + 1.0f) / 2.0f) * ((float)p.W - 1.0f)` and the same for y, in float32"""
    wm, hm = (F32(W), F32(H)) if mut == "scale_W_for_Wm1" else (F32(F32(W) - F32(1)), F32(F32(H) - F32(1)))
    with np.errstate(invalid="ignore", over="ignore"):
        x = (((np.asarray(xs, dtype=F32) + F32(1)).astype(F32) / F32(2)).astype(F32) * wm).astype(F32)
        y = (((np.asarray(ys, dtype=F32) + F32(1)).astype(F32) / F32(2)).astype(F32) * hm).astype(F32)
    return x, y


def flow_pixel(flow):
    """x = j + flow_x, y = i + flow_y in float32 -> [B,H*W] each"""
    flow = np.asarray(flow, dtype=F32)
    B, H, W, _ = flow.shape
    x = (np.arange(W, dtype=F32)[None, None, :] + flow[..., 0]).astype(F32)
    y = (np.arange(H, dtype=F32)[None, :, None] + flow[..., 1]).astype(F32)
    return x.reshape(B, -1), y.reshape(B, -1)


def pad_geom(x, n):
    """padded_geom along one axis of size n, float32: (x + 1 after the clamp, x0f, x1f, x0, x1)"""
    x = np.minimum(np.maximum(np.asarray(x, dtype=F32), F32(-1)), F32(n))
    x = (x + F32(1)).astype(F32)
    x0f = np.floor(x).astype(F32)
    x1f = (x0f + F32(1)).astype(F32)
    return x, x0f, x1f, x0f.astype(np.int64), np.minimum(x1f, F32(n) + F32(1)).astype(np.int64)


def blend_reference(im, x, y):
    """(ref, E) [B,N,C] float64 at float32 pixel coordinates x, y [B,N]"""
    im = np.asarray(im, dtype=F32)
    B, H, W, C = im.shape
    imp = np.pad(im.astype(np.float64), [[0, 0], [1, 1], [1, 1], [0, 0]])
    xp, x0f, x1f, x0, x1 = pad_geom(x, W)
    yp, y0f, y1f, y0, y1 = pad_geom(y, H)
    xd, yd = xp.astype(np.float64), yp.astype(np.float64)
    bi = np.arange(B)[:, None]
    ref = np.zeros(xp.shape + (C,))
    S = np.zeros_like(ref)
    for w, yy, xx in (((x1f - xd) * (y1f - yd), y0, x0), ((xd - x0f) * (y1f - yd), y0, x1),
                      ((x1f - xd) * (yd - y0f), y1, x0), ((xd - x0f) * (yd - y0f), y1, x1)):
        t = w[..., None] * imp[bi, yy, xx]
        ref += t
        S += np.abs(t)
    return ref, SECOND * G_BLEND * U24 * S + 4.0 * TINY


BLEND_MUTANTS = ("weights_after_clip", "taps_exchanged", "clamped_tap_as_value", "upper_index_not_min", "sums_reordered",
                 "fused_multiply_add")


def replay_blend(im, x, y, mut=None):
    """padded_geom + sample_padded_blend in NumPy float32, with a simulated defect"""
    im = np.asarray(im, dtype=F32)
    B, H, W, C = im.shape
    xp, x0f, x1f, x0, x1 = pad_geom(x, W)
    yp, y0f, y1f, y0, y1 = pad_geom(y, H)
    if mut == "clamped_tap_as_value":
        imp = np.pad(im, [[0, 0], [1, 1], [1, 1], [0, 0]], mode="edge")
    else:
        imp = np.pad(im, [[0, 0], [1, 1], [1, 1], [0, 0]])
    if mut == "upper_index_not_min":                                      # one element past the ringed image: not a pixel
        imp = np.pad(imp, [[0, 0], [0, 1], [0, 1], [0, 0]], constant_values=np.nan)
        x1, y1 = x1f.astype(np.int64), y1f.astype(np.int64)
    if mut == "weights_after_clip":                                       # from the taps clamped into the image
        x0f, x1f = (np.clip(x0 - 1, 0, W - 1) + 1).astype(F32), (np.clip(x1 - 1, 0, W - 1) + 1).astype(F32)
        y0f, y1f = (np.clip(y0 - 1, 0, H - 1) + 1).astype(F32), (np.clip(y1 - 1, 0, H - 1) + 1).astype(F32)
    bi = np.arange(B)[:, None]
    I00, I01, I10, I11 = imp[bi, y0, x0], imp[bi, y0, x1], imp[bi, y1, x0], imp[bi, y1, x1]
    if mut == "taps_exchanged":
        I01, I10 = I10, I01
    w00 = ((x1f - xp).astype(F32) * (y1f - yp).astype(F32)).astype(F32)[..., None]
    w01 = ((xp - x0f).astype(F32) * (y1f - yp).astype(F32)).astype(F32)[..., None]
    w10 = ((x1f - xp).astype(F32) * (yp - y0f).astype(F32)).astype(F32)[..., None]
    w11 = ((xp - x0f).astype(F32) * (yp - y0f).astype(F32)).astype(F32)[..., None]
    with np.errstate(invalid="ignore"):
        if mut == "fused_multiply_add":
            fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
            return fma(w11, I11, fma(w10, I10, fma(w01, I01, (w00 * I00).astype(F32))))
        t00, t01, t10, t11 = ((w * I).astype(F32) for w, I in ((w00, I00), (w01, I01), (w10, I10), (w11, I11)))
        if mut == "sums_reordered":
            return (t00 + (t01 + (t10 + t11).astype(F32)).astype(F32)).astype(F32)
        return (((t00 + t01).astype(F32) + t10).astype(F32) + t11).astype(F32)


def check_blend(out, im, x, y, oracle):
    """out [B,N,C] (any shape of that size) at float32 pixel coordinates x, y [B,N]: (values out of the float64 bound,
    worst ratio, values not bit-equal to `oracle` (+0 == -0), pixels (b, n) of either kind)"""
    ref, E = blend_reference(im, x, y)
    got = np.ascontiguousarray(out, dtype=F32).reshape(ref.shape)
    d = np.abs(got.astype(np.float64) - ref)
    bad = ~(d <= E)
    q = np.nan_to_num(d / E, nan=np.inf)
    o32 = np.ascontiguousarray(oracle, dtype=F32).reshape(ref.shape)
    neq = (got.view(np.uint32) != o32.view(np.uint32)) & ~((got == 0) & (o32 == 0))
    return int(bad.sum()), float(q.max()), int(neq.sum()), np.argwhere(bad.any(-1) | neq.any(-1))


def oracle_sample(im, xs, ys):
    from oracle import spatial_transformer as ost
    B, C = im.shape[0], im.shape[3]
    return ost.bilinear_interp(im, xs, ys, None).reshape(B, -1, C)


def oracle_padded(im, x, y):
    from oracle.warp_with_optical_flow import padded_bilinear
    return padded_bilinear(im, x, y)


REGIONS = ("x in [-1,0)", "x in [W-1,W]", "y in [-1,0)", "y in [H-1,H]", "exactly -1", "exactly W / H", "on an integer",
           "beyond left", "beyond right", "beyond top", "beyond bottom", "+-Inf", "|v| >= 3e38")
REGION_SHARE = 0.05


def region_counts(x, y, H, W, xs=None, ys=None):
    """pixel coordinates x, y (before the clamp) and the coordinates xs, ys as given to the sampler (default: x, y) ->
    (counts per REGIONS, number of samples)"""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    xs, ys = (x if xs is None else np.asarray(xs, dtype=F32)), (y if ys is None else np.asarray(ys, dtype=F32))
    huge = lambda v: np.isfinite(v) & (np.abs(v) >= 3e38)
    with np.errstate(invalid="ignore"):
        c = (((x >= -1) & (x < 0)), ((x >= W - 1) & (x <= W)), ((y >= -1) & (y < 0)), ((y >= H - 1) & (y <= H)),
             ((x == -1) | (y == -1)), ((x == W) | (y == H)),
             (np.isfinite(x) & (x == np.floor(x))) | (np.isfinite(y) & (y == np.floor(y))),
             (x < -1), (x > W), (y < -1), (y > H), np.isinf(xs) | np.isinf(ys), huge(xs) | huge(ys))
    return tuple(int(v.sum()) for v in c), x.size


def regions_ok(counts, n):
    return all(c >= REGION_SHARE * n for c in counts)


def region_text(counts, n):
    return ", ".join("%s %.1f %%" % (name, 100.0 * c / n) for name, c in zip(REGIONS, counts))


def _normalised_for(t, n):
    """float32 x_s whose float32 pixel coordinate ((x_s + 1) / 2) (n - 1) is the float32 t where an x_s within 3 ulp has
    that property (else the nearest candidate)"""
    t = np.asarray(t, dtype=F32)
    wm = F32(F32(n) - F32(1))
    base = (2.0 * t.astype(np.float64) / float(wm) - 1.0).astype(F32)
    cand = [base]
    for _ in range(3):
        cand = [np.nextafter(cand[0], F32(-np.inf))] + cand + [np.nextafter(cand[-1], F32(np.inf))]
    cand = np.stack(cand)
    fwd = (((cand + F32(1)).astype(F32) / F32(2)).astype(F32) * wm).astype(F32)
    pick = np.where((fwd == t[None]).any(0), (fwd == t[None]).argmax(0), 3)
    return np.take_along_axis(cand, pick[None], 0)[0]


def region_coords(B, N, H, W, seed, special=True):
    """normalised float32 x_s, y_s [B,N]: each axis draws one of ten kinds per sample (inside, the two border cells, the two
    clamp values exactly, an integer, beyond either side, +-Inf, +-3e38)"""
    rng = np.random.default_rng(seed)

    def axis(n):
        kind = rng.integers(0, 10 if special else 8, (B, N))
        sign = rng.choice([-1.0, 1.0], (B, N))
        u = rng.uniform(0.0, 1.0, (B, N))
        t = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7],
                      [u * (n - 1), u * 0.999 - 1.0, (n - 1) + u, -1.0 + 0 * u, n + 0 * u,
                       np.floor(u * (n + 2)) - 1.0, -1.0 - 0.01 - 5.0 * u, n + 0.01 + 5.0 * u], 0.0).astype(F32)
        v = _normalised_for(t, n)
        v = np.where(kind == 8, F32(np.inf) * sign.astype(F32), v)
        return np.where(kind == 9, F32(3.2e38) * sign.astype(F32), v).astype(F32)
    return axis(W), axis(H)


def make_frames(kind, B, H, W, C, seed):
    """smooth | noise (white, both signs) | positive (white, in [0.5, 1.5]) | corners (zero but for the four corners and the
    last row and column: a tap on the ring that read the clamped pixel would show)"""
    if kind in ("smooth", "ones"):
        return tps.make_frames(kind, B, H, W, C, seed)
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.uniform(-1.0, 1.0, (B, H, W, C)).astype(F32)
    v = rng.uniform(0.5, 1.5, (B, H, W, C)).astype(F32)
    if kind == "corners":
        keep = np.zeros((H, W), dtype=bool)
        keep[-1, :] = keep[:, -1] = keep[0, 0] = True
        v = v * keep[None, :, :, None]
    return v.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# link 3: the launch formula of dvsg_flow_warp_f32, restated (not imported)

FS_W, FS_STEP, FS_MX, FS_MY, FS_ROUNDS = 128, 16, 12, 12, 4
FS_COLS, FS_LIVE = FS_W + 2 * FS_MX + 1, FS_STEP + 2 * FS_MY + 1


def strip_launch(B, H, W, rounds=FS_ROUNDS):
    """(nstrips, nbands, band_rows) of flow_warp_strip_kernel for [B,H,W,3]"""
    nstrips = -(-W // FS_W)
    steps = -(-H // FS_STEP)
    bands = min(max(1, (rounds * 256 + nstrips * B - 1) // (nstrips * B)), max(1, steps // 8))
    band_rows = -(-steps // bands) * FS_STEP
    return nstrips, -(-H // band_rows), band_rows


# (B, H, W) -> (nstrips, nbands, band_rows): the seams of the strip kernel (written out, recomputed by a CPU test)
SEAMS = {
    (1, 256, 130): (2, 2, 128), (2, 273, 130): (2, 2, 144), (1, 305, 130): (2, 2, 160), (2, 337, 130): (2, 2, 176),
    (1, 369, 130): (2, 3, 128), (3, 273, 129): (2, 2, 144), (3, 369, 257): (3, 3, 128),
    (1, 1, 130): (2, 1, 16), (1, 16, 130): (2, 1, 16), (1, 17, 130): (2, 1, 32), (1, 33, 130): (2, 1, 48),
    (1, 49, 130): (2, 1, 64), (1, 65, 130): (2, 1, 80),
    (3, 33, 1): (1, 1, 48), (3, 33, 4): (1, 1, 48), (3, 33, 127): (1, 1, 48), (3, 33, 128): (1, 1, 48),
    (3, 33, 129): (2, 1, 48), (3, 33, 257): (3, 1, 48),
}
GATHER_SHAPES = [(2, 37, 53, 1), (2, 37, 53, 2), (2, 5, 9, 5)]           # C != 3: stn_kernel<kFlow, 1 | 0>
FLOW_CONST = [(a, v) for a in (0, 1) for v in (12.0, -12.0, 11.999, -11.999, 12.001, -12.001, 13.5, -12.5)]
# inside the window at every pixel by construction: |v| <= 12 keeps both taps within the +- 12 px margins, and + 12.001
# floors to the tap of + 12.  - 12.001 and - 12.5 floor to - 13 and leave the window in the first column of every strip but
# the first / the first row of every step but the band's first (the clamp to -1 keeps the very first inside); + 13.5 leaves
# it in the last column of a strip whose source column j + 13 is still <= W (dx == kFsCols - 1: W >= 141) / the last row
# of a step with 28 rows or more below its first (dy == kFsLive - 1).  That is one column of 128 or one row of 16 at the most.
# (13.5 and not 13: with a zero fraction the tap beyond the window carries the weight 0 and a wrong value there cannot show;
# a window row holds up to 2 floats more than its 153 pixels, so the tap at dx == kFsCols - 1 is wrong only in the rows
# whose lead-in is 3 floats -- every fourth row at W & 3 == 1.)
FLOW_CONST_INSIDE = {(a, v) for a, v in FLOW_CONST if v not in (-12.001, 13.5, -12.5)}


def const_flow_leaves_window(a, v, H, W):
    """does the constant flow v on axis a put at least one pixel of an H x W frame outside the window?"""
    if (a, v) in FLOW_CONST_INSIDE:
        return False
    if a == 0:
        return W > FS_W and (v < 0 or W >= FS_W + 13)
    return H > FS_STEP if v < 0 else H >= 28


def band_of(i, band_rows):
    i_begin = (i // band_rows) * band_rows
    return i_begin, i_begin + ((i - i_begin) // FS_STEP) * FS_STEP


def window_offsets(flow, launch):
    """(dx, dy) [B,H,W] of `inwin`: the lower tap's column and row relative to the strip kernel's LDS window"""
    flow = np.asarray(flow, dtype=F32)
    B, H, W, _ = flow.shape
    _, _, band_rows = launch
    x, y = flow_pixel(flow)
    xl = pad_geom(x, W)[3].reshape(B, H, W) - 1
    yl = pad_geom(y, H)[3].reshape(B, H, W) - 1
    j, i = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    dx = xl - ((j // FS_W) * FS_W - FS_MX)
    return dx, yl - (band_of(i, band_rows)[1] - FS_MY)


def window_share(flow, launch):
    """share of pixels whose four taps lie inside the strip kernel's LDS window (`inwin`), from the flow alone"""
    dx, dy = window_offsets(flow, launch)
    return float(((dx >= 0) & (dx <= FS_COLS - 2) & (dy >= 0) & (dy <= FS_LIVE - 2)).mean())


def flows_for(group, B, H, W, launch, seed):
    """name -> (flow [B,H,W,2] float32, expected window share: a number, a range (lo, hi) or (lo, hi, "<"): hi excluded).
    The ranges, from how each flow is drawn: the smooth flow is N(0, 24 px) box-filtered over up to 15 x 15 pixels plus 1 %
    of far pixels (>= 0.85); rint(6 N(0, 1)) reaches 13 px with probability 3.7 % per axis (>= 0.9); a component is +-Inf with
    probability 0.19, and a pixel with none keeps |flow| < 5 (>= 0.8^2 - margin = 0.6); of the four border targets, column -1
    is inside the window for the whole first strip and column W for the last (>= 2 / 3 of a quarter of the pixels at three
    strips: 0.15)."""
    import inputs as tin
    rng = np.random.default_rng(seed)
    i, j = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    zero = np.zeros((B, H, W, 2), dtype=F32)
    out = {}
    if group == "const":
        for a, v in FLOW_CONST:
            f = zero.copy()
            f[..., a] = F32(v)
            want = (0.9, 1.0, "<") if const_flow_leaves_window(a, v, H, W) else 1.0
            out["const %s %+g" % ("xy"[a], v)] = (f, want)
        return out
    _, _, band_rows = launch
    out["smooth"] = (tin.smooth_flow(seed, B, H, W), (0.85, 1.0))
    if H >= 100:                                   # the window is 41 rows high; it is 153 columns wide, which W <= 257 barely leaves
        f = rng.uniform(-8.0, 8.0, (B, H, W, 2)).astype(F32)
        a, n, pos = 1, H, i
        f[..., a] += np.where((i % 2 == 1), np.where(pos < n // 2, 40.0, -40.0), 0.0).astype(F32) + 0 * j * i
        out["mixed"] = (f, (0.3, 0.7))
    i_begin, i0 = band_of(i, band_rows)
    i_end = np.minimum(H, i_begin + band_rows)
    f = zero.copy()
    f[..., 0] = 0.25
    f[..., 1] = np.where(i >= i_end - FS_STEP, i_end - i + 0.5, 0.25) + 0 * j
    out["last step -> next band's first row"] = (f, 1.0)   # at most 16.5 rows down: dy <= 28, served by the ring
    f = zero.copy()
    f[..., 0] = -0.25
    f[..., 1] = np.where(i < i_begin + FS_STEP, i_begin - 1 - i - 0.5, -0.25) + 0 * j
    out["first step -> previous band's last row"] = (f, 1.0)   # the primed rows above the band: dy >= 0
    k = (i + j) % 4
    f = zero.copy()
    f[..., 0] = np.where(k == 0, -1.0 - j, np.where(k == 1, 1.0 * W - j, 0.0))
    f[..., 1] = np.where(k == 2, -1.0 - i, np.where(k == 3, 1.0 * H - i, 0.0))
    out["onto rows -1, H and columns -1, W"] = (f, (0.15, 1.0))
    out["integer"] = (np.rint(6.0 * rng.standard_normal((B, H, W, 2))).astype(F32), (0.9, 1.0))
    f = rng.uniform(-5.0, 5.0, (B, H, W, 2)).astype(F32)
    f[rng.uniform(size=f.shape) < 0.1] = np.inf
    f[rng.uniform(size=f.shape) < 0.1] = -np.inf
    out["+-Inf"] = (f, (0.6, 1.0))
    return out


def check_share(name, share, want):
    """every flow carries an expectation: no share is only reported"""
    if isinstance(want, tuple):
        assert want[0] <= share <= want[1] and (len(want) == 2 or share < want[1]), (name, share, want)
    else:
        assert share == want, (name, share, want)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables

# grids: (kind, out_h, out_w, B, parameter); affine / projective parameter: a theta family, elastic: (grid side, vector scale)
GRID_CASES = [
    ("affine", 37, 53, 5, "random"), ("affine", 1, 1, 1, "random"), ("affine", 1, 7, 5, "random"), ("affine", 5, 1, 1, "random"),
    ("affine", 2, 255, 1, "random"), ("affine", 3, 256, 5, "random"), ("affine", 4, 257, 1, "big"), ("affine", 72, 128, 1, "big"),
    ("projective", 37, 53, 5, "random"), ("projective", 1, 1, 1, "random"), ("projective", 1, 7, 5, "zq0"),
    ("projective", 5, 1, 1, "zq0"), ("projective", 2, 255, 1, "sign"), ("projective", 3, 256, 5, "strong"),
    ("projective", 4, 257, 1, "zq0"), ("projective", 72, 128, 1, "sign"), ("projective", 20, 4, 5, "strong"),
    ("elastic", 37, 53, 5, (4, 0.05)), ("elastic", 1, 1, 1, (2, 0.5)), ("elastic", 1, 7, 5, (3, 0.05)),
    ("elastic", 5, 1, 1, (7, 0.5)), ("elastic", 2, 255, 1, (2, 0.05)), ("elastic", 3, 256, 1, (3, 0.5)),
    ("elastic", 4, 257, 1, (4, 0.5)), ("elastic", 72, 128, 1, (7, 0.05)), ("elastic", 4, 4, 5, (4, 0.5)),
    ("elastic", 7, 7, 1, (4, 0.05)), ("elastic", 13, 19, 5, (7, 0.5)),
]
GRID_IDS = ["%s-%dx%d-B%d-%s" % (c[0], c[1], c[2], c[3], str(c[4]).replace(" ", "")) for c in GRID_CASES]
GRID_IMAGE = {"affine": (9, 14, 3), "projective": (11, 6, 18), "elastic": (8, 8, 1)}   # (H, W, C) of the image call
CPU_MAX = 72 * 128


def grid_theta(kind, B, fam, seed):
    import inputs as tin
    rng = np.random.default_rng(seed)
    if kind == "affine":
        s = 0.1 if fam == "random" else 30.0
        return (np.array([1, 0, 0, 0, 1, 0])[None] + s * rng.standard_normal((B, 6))).astype(F32)
    if fam == "random":
        return tin.mask_homographies(seed, B)
    if fam == "strong":
        return strong_homographies(seed, B)
    th = np.tile(np.array([1, 0, 0, 0, 1, 0, 1, 0], dtype=F32)[None], (B, 1))          # zq = x_t + 1: 0 on column 0
    if fam == "sign":
        th[:, 6], th[:, 7] = 2.0, 0.5                                                   # zq changes sign inside the frame
        th[:, :6] += (0.1 * rng.standard_normal((B, 6))).astype(F32)
    return th


def strong_homographies(seed, B):
    """three times the range of inputs.mask_homographies (the range of test_gpu_masked.py)"""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (B, 8)).astype(F32)
    scale = np.array([0.1, 0.1, 0.5, 0.1, 0.1, 0.5, 0.1, 0.1], dtype=F32)
    return (u * F32(3.0) * scale + np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=F32)).astype(F32)


# sampler B: (H, W, C, out_h, out_w, B, frames).  W - 1 and H - 1 are powers of two: only then does a float32 x_s exist whose
# pixel coordinate ((x_s + 1) / 2) (W - 1) is exactly -1, W or a chosen integer (1 / (W - 1) is exact).  Frames of other sizes
# meet those values through the flows of link 3, which are in pixel units, and through the image calls of link 1.
SAMPLE_CASES = [
    (33, 65, 3, 37, 53, 2, "smooth"), (9, 17, 3, 5, 300, 1, "noise"), (17, 33, 1, 6, 257, 2, "corners"),
    (17, 9, 1, 21, 19, 1, "positive"), (33, 65, 2, 7, 255, 1, "noise"), (9, 5, 4, 13, 10, 2, "corners"),
    (9, 9, 18, 9, 37, 1, "noise"), (5, 3, 64, 6, 35, 1, "positive"), (2, 2, 3, 8, 256, 1, "corners"), (65, 129, 3, 72, 128, 1, "corners"),
]
SAMPLE_IDS = ["%dx%d-C%d-%dx%d-B%d-%s" % c for c in SAMPLE_CASES]

MASK_SHAPES = [(1, 1, 2), (20, 4, 3), (37, 53, 2), (5, 301, 1), (30, 600, 2)]
MASK_FAMILIES = ("random", "strong", "identity", "zero theta", "plane 0", "zq0")


def mask_theta(fam, B, seed):
    import inputs as tin
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=F32)
    if fam == "random":
        return tin.mask_homographies(seed, B)
    if fam == "strong":
        return strong_homographies(seed, B)
    th = np.tile(ident[None], (B, 1))
    if fam == "zero theta":
        th[:] = 0
    elif fam == "plane 0":
        th[:, 2] = 5.0
    elif fam == "zq0":
        th[:, 6] = 1.0
    return th


def stn_key(src, C, ppt):
    return ("stn_kernel", src, 3 if C == 3 else (1 if C == 1 else 0), ppt)


# every stn_kernel<SRC, C, PPT> (SRC 0 flow, 1 coords, 2 affine, 3 projective, 4 elastic), the mask plane and the strip
# kernel, and the GPU tests of this file that launch it
COVERED = {
    ("stn_kernel", 0, 3, 4): ["test_flow_warp_three_forms_the_oracle_and_float64 (flow_tiled = 0)", "test_flow_warp_of_a_frame_off_the_16_byte_grid"],
    ("stn_kernel", 0, 1, 4): ["test_flow_warp_other_channel_counts (C = 1)"],
    ("stn_kernel", 0, 0, 4): ["test_flow_warp_other_channel_counts (C = 2, 5)"],
    ("stn_kernel", 1, 3, 4): ["test_sampler_b_at_given_coordinates (C = 3)"],
    ("stn_kernel", 1, 1, 4): ["test_sampler_b_at_given_coordinates (C = 1)"],
    ("stn_kernel", 1, 0, 4): ["test_sampler_b_at_given_coordinates (C = 2, 4, 18, 64)"],
    ("stn_kernel", 2, 3, 2): ["test_grid_against_float64_and_the_oracle (affine, the image call: GRID_IMAGE)"],
    ("stn_kernel", 2, 1, 2): ["test_grid_against_float64_and_the_oracle (affine, the image-less call)", "test_grid_channel_forms"],
    ("stn_kernel", 2, 0, 2): ["test_grid_channel_forms (affine, C = 4)"],
    ("stn_kernel", 3, 3, 2): ["test_grid_channel_forms (projective, C = 3)"],
    ("stn_kernel", 3, 1, 2): ["test_grid_against_float64_and_the_oracle (projective, the image-less call)",
                              "test_mask_plane_against_float64_the_image_kernel_and_the_oracle (all-ones image)"],
    ("stn_kernel", 3, 0, 2): ["test_grid_against_float64_and_the_oracle (projective, the image call, C = 18)"],
    ("stn_kernel", 4, 3, 2): ["test_grid_channel_forms (elastic, C = 3)"],
    ("stn_kernel", 4, 1, 2): ["test_grid_against_float64_and_the_oracle (elastic, both calls)"],
    ("stn_kernel", 4, 0, 2): ["test_grid_channel_forms (elastic, C = 2)"],
    ("mask_plane_kernel",): ["test_mask_plane_against_float64_the_image_kernel_and_the_oracle"],
    ("flow_warp_strip_kernel",): ["test_flow_warp_three_forms_the_oracle_and_float64 (flow_tiled = 1, 2)"],
}
SRC_OF = {"affine": 2, "projective": 3, "elastic": 4}
CHANNEL_FORMS = [("affine", 1), ("affine", 4), ("projective", 3), ("elastic", 3), ("elastic", 2)]   # test_grid_channel_forms


def grid_launched():
    """the stn_kernel<2 | 3 | 4, C, 2> that the grid tests launch, from their own tables: the image call of every kind in
    GRID_CASES (GRID_IMAGE), its image-less call (C = 1) and the channel forms"""
    kinds = {c[0] for c in GRID_CASES}
    return ({stn_key(SRC_OF[k], GRID_IMAGE[k][2], PPT_GRID) for k in kinds} | {stn_key(SRC_OF[k], 1, PPT_GRID) for k in kinds}
            | {stn_key(SRC_OF[k], C, PPT_GRID) for k, C in CHANNEL_FORMS})


_MANGLED = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+(stn_kernel|mask_plane_kernel|flow_warp_strip_kernel)(?:ILi(\d+)ELi(\d+)ELi(\d+)EE)?")


def library_instantiations():
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    return {(n.decode(),) if not a else (n.decode(), int(a), int(b), int(c)) for n, a, b, c in _MANGLED.findall(data)}


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests

# The share of a case's values that a simulated wrong kernel must put out of bounds (or off the oracle's bits), reasoned
# from how region_coords draws: per axis 10 kinds of 10 % each, of which the inside, the two border cells and part of the
# integers touch the frame -- about 12 % of the samples have a non-zero reference at all, and a defect of the scale or an
# exchange of taps can only show there (floors 0.08 and 0.05).  A ring tap read as the clamped pixel shows on every sample
# beyond the frame on one axis whose other axis touches it (0.2); an index that is not min()-ed on every sample at or
# clamped to W or H (three kinds of ten per axis: 0.2); weights from the clamped taps in the border cells and beyond
# (0.1).  A reordered sum or a fused multiply-add changes bits only where at least three taps are non-zero and the
# roundings fall differently: on the dense frames at least one value (sum) and 0.3 % of the values (FMA) where the case
# has 1000 values or more; the "corners" frame is zero on all but H + W pixels and has no floor for the two, nor for
# exchanged taps; it is there for the ring (a tap on it must read 0), which it must show in the float64 bound.
MUTANT_FLOOR = {"scale_W_for_Wm1": 0.08, "weights_after_clip": 0.1, "taps_exchanged": 0.05, "clamped_tap_as_value": 0.2,
                "upper_index_not_min": 0.2, "sums_reordered": 1e-4, "fused_multiply_add": 0.003,
                "affine_rows_swapped": 0.5, "log2_for_ln": 0.5}
ROUNDING_ONLY = ("sums_reordered", "fused_multiply_add")


def test_table_covers_every_instantiation_of_the_library():
    """15 stn_kernel<SRC, C, PPT> + 2 plain kernels when this was written; a new one without a case fails here"""
    found = library_instantiations()
    assert len(found) >= 17, sorted(found)
    assert found == set(COVERED), (sorted(found - set(COVERED)), sorted(set(COVERED) - found))
    assert {stn_key(1, c[2], PPT_MEM) for c in SAMPLE_CASES} == {k for k in COVERED if k[:2] == ("stn_kernel", 1)}
    assert {2, 4, 18, 64} <= {c[2] for c in SAMPLE_CASES}
    assert {stn_key(0, c[3], PPT_MEM) for c in GATHER_SHAPES} | {stn_key(0, 3, PPT_MEM)} == {k for k in COVERED if k[:2] == ("stn_kernel", 0)}
    assert grid_launched() == {k for k in COVERED if k[0] == "stn_kernel" and k[1] >= 2}
    names = set(globals())
    for tests in COVERED.values():
        assert all(t.split(" ")[0] in names for t in tests), tests


def test_shapes_meet_every_row_residue_partial_column_blocks_and_the_asked_sizes():
    for kind in ("affine", "projective", "elastic"):
        cs = [c for c in GRID_CASES if c[0] == kind]
        assert {0, 1} <= {c[1] % PPT_GRID for c in cs} and {1, 255, 256, 257} <= {c[2] for c in cs}
        assert {(1, 1), (1, 7), (5, 1)} <= {(c[1], c[2]) for c in cs} and {1, 5} <= {c[3] for c in cs}
        assert all((c[1], c[2]) != GRID_IMAGE[kind][:2] for c in cs)                    # out_size != (H, W)
    assert {2, 3, 4, 7} == {c[4][0] for c in GRID_CASES if c[0] == "elastic"}
    assert {0.05, 0.5} == {c[4][1] for c in GRID_CASES if c[0] == "elastic"}
    assert {("elastic", 4, 4), ("elastic", 7, 7)} <= {c[:3] for c in GRID_CASES if c[0] == "elastic" and c[4][0] == 4}
    assert {0, 1, 2, 3} <= {c[3] % PPT_MEM for c in SAMPLE_CASES} and {255, 256, 257} <= {c[4] for c in SAMPLE_CASES}
    assert {"smooth", "noise", "positive", "corners"} == {c[6] for c in SAMPLE_CASES}
    assert {(1, 1), (20, 4), (37, 53), (5, 301), (30, 600)} == {s[:2] for s in MASK_SHAPES}


def test_band_table_is_the_launch_formula_of_dvsg_flow_warp_f32():
    """the table against the formula restated above, the restatement against the source text, and the seams the table
    must hold: 2 bands of 8, 9, 10 and 11 steps, 3 bands of 8 with a short last one, 1-5 single-band steps, every W & 3"""
    src = open(WARP_SRC).read() + open(os.path.join(os.path.dirname(WARP_SRC), "common.h")).read()   # (the switches' defaults)
    for text in ("constexpr int kFsW = 128, kFsStep = 16, kFsPPT = 2;", "constexpr int kFsMX = 12, kFsMY = 12;",
                 "int flow_rounds = 4;", "q.nstrips = ceil_div(W, kFsW);", "const int steps = ceil_div(H, kFsStep);",
                 "int bands = (int)std::min<long>(std::max<long>(1, ((long)g_opt.flow_rounds * 256 + (long)q.nstrips * B - 1) / "
                 "((long)q.nstrips * B)), std::max(1, steps / 8));",
                 "const int band_steps = ceil_div(steps, bands);", "q.band_rows = band_steps * kFsStep;",
                 "q.nbands = ceil_div(H, q.band_rows);",
                 "inwin[r] = (unsigned)dx <= (unsigned)(kFsCols - 2) && (unsigned)dy <= (unsigned)(kFsLive - 2);"):
        assert text in src, "the launch formula changed: restate strip_launch / window_share (%s)" % text
    for key, want in SEAMS.items():
        assert strip_launch(*key) == want, (key, strip_launch(*key), want)
    steps = lambda B, H, W: [-(-(min(H, (b + 1) * SEAMS[B, H, W][2]) - b * SEAMS[B, H, W][2]) // FS_STEP) for b in range(SEAMS[B, H, W][1])]
    assert steps(1, 256, 130) == [8, 8] and steps(2, 273, 130) == [9, 9] and steps(1, 305, 130) == [10, 10]
    assert steps(2, 337, 130) == [11, 11] and steps(1, 369, 130) == [8, 8, 8] and 369 - 256 < 8 * FS_STEP
    assert steps(3, 273, 129) == [9, 9] and steps(3, 369, 257) == [8, 8, 8]
    assert [steps(1, H, 130) for H in (1, 16, 17, 33, 49, 65)] == [[1], [1], [2], [3], [4], [5]]
    assert {k[2] for k in SEAMS if k[0] == 3} == {1, 4, 127, 128, 129, 257} and {W & 3 for _, _, W in SEAMS} == {0, 1, 2, 3}
    for B, H, W in [k for k in SEAMS if k[0] == 3 and SEAMS[k][1] > 1]:                # multi-band, img_pix & 3 varies, W & 3 != 0
        assert len({(b * H * W) & 3 for b in range(B)}) == 3 and W & 3
    assert max(H * W * B for B, H, W in SEAMS) == 369 * 257 * 3


CPU_GRID = [c for c in GRID_CASES if c[1] * c[2] <= CPU_MAX]


def _grid_inputs(case):
    kind, oh, ow, B, par = case
    seed = oh * 31 + ow + B
    if kind == "elastic":
        g, scale = par
        src, linv = elastic_constants(g)
        return elastic_theta(g, B, scale, seed), src, linv
    return grid_theta(kind, B, par, seed), None, None


@pytest.mark.parametrize("case", CPU_GRID, ids=[i for c, i in zip(GRID_CASES, GRID_IDS) if c in CPU_GRID])
def test_grid_bounds_hold_for_the_replays_and_flag_defects(case):
    from oracle import spatial_transformer as ost
    kind, oh, ow, B, par = case
    theta, src, linv = _grid_inputs(case)
    dummy = np.zeros((B, 1, 1, 1), dtype=F32)
    n = 2 * B * oh * ow
    if kind == "affine":
        ref, E = affine_reference(theta, oh, ow)
        xs, ys = replay_affine(theta, oh, ow)
        xo, yo = ost.AffineTransformer((oh, ow))._transform(dummy, theta)
        assert np.array_equal(xs.reshape(-1), xo) and np.array_equal(ys.reshape(-1), yo)
        nbad, worst, at = check_grid(xs, ys, ref, E)
        assert nbad == 0, (worst, at)
        nb = check_grid(*replay_affine(theta, oh, ow, "affine_rows_swapped"), ref, E)[0]
        assert nb >= (MUTANT_FLOOR["affine_rows_swapped"] * n if oh * ow > 1 else 1), ("affine_rows_swapped", nb, n)
    elif kind == "projective":
        ref, E = projective_reference(theta, oh, ow)
        xs, ys = replay_projective(theta, oh, ow)
        xo, yo = ost.ProjectiveTransformer((oh, ow))._transform(dummy, theta)
        assert np.array_equal(xs.reshape(-1), xo) and np.array_equal(ys.reshape(-1), yo)
        nbad, worst, at = check_grid(xs, ys, ref, E)
        assert nbad == 0, (worst, at)
        if par == "zq0":
            assert (xs[:, :, 0] == 0).all() and (ys[:, :, 0] == 0).all() and (E[:, :, :, 0] == 0).all()
            nb = check_grid(*replay_projective(theta, oh, ow, "zq0_gives_inf"), ref, E)[0]
            assert nb >= 2 * B * oh, ("zq0_gives_inf", nb)                              # floor: the whole column j = 0
        if par == "sign":
            z = _aff64(_theta9(theta)[:, 2], *_xy64(oh, ow))[0]
            assert (z > 0).any() and (z < 0).any()
    else:
        c64, Ec = coeff_reference(theta, linv)
        c32 = replay_coeff(theta, linv)
        assert (np.abs(c32.astype(np.float64) - c64) <= Ec).all(), float((np.abs(c32 - c64) / Ec).max())
        ref, E = elastic_reference(c32, None, src, oh, ow)
        xs, ys = replay_elastic(c32, src, oh, ow)
        nbad, worst, at = check_grid(xs, ys, ref, E)
        assert nbad == 0, ("map of the float32 coefficients", worst, at)
        refc, Ecm = elastic_reference(c64, Ec, src, oh, ow)
        nbad, worst_c, at = check_grid(xs, ys, refc, Ecm)
        assert nbad == 0, ("chain from the float64 coefficients", worst_c, at)
        print("replay / bound %.3f (chain %.3f)" % (worst, worst_c))
        nb = check_grid(*replay_elastic(c32, src, oh, ow, "log2_for_ln"), ref, E)[0]
        assert nb >= MUTANT_FLOOR["log2_for_ln"] * n, ("log2_for_ln", nb, n)
        if oh % PPT_GRID:
            nb = check_grid(*replay_elastic(c32, src, oh, ow, "last_row_dropped"), ref, E)[0]
            assert nb == 2 * B * ow, ("last_row_dropped", nb)                           # floor: exactly the last row
        X, Y = _xy32(oh, ow)
        on_node = sum(int(((X == src[0, k]) & (Y == src[1, k])).sum()) for k in range(src.shape[1]))
        if (oh, ow) in ((4, 4), (7, 7)):
            assert on_node == src.shape[1] == 16                                        # every source point is a pixel
        if on_node:
            xs, ys = replay_elastic(c32, src, oh, ow, "rsq0_gives_nan")
            assert check_grid(xs, ys, ref, E)[0] >= 2 * B * on_node, "rsq0_gives_nan"   # floor: those pixels


def _sample_inputs(case):
    H, W, C, oh, ow, B, frames = case
    im = make_frames(frames, B, H, W, C, seed=H * W + C)
    xs, ys = region_coords(B, oh * ow, H, W, seed=oh * ow + C)
    return im, xs, ys


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=SAMPLE_IDS)
def test_sampler_checks_cover_the_regions_and_flag_defects(case):
    """with the oracle alone: every region holds >= 5 % of the case's samples; the oracle is inside the float64 bound
    and bit-equal to the replay; each simulated defect is rejected at or above its floor"""
    H, W, C, oh, ow, B, frames = case
    im, xs, ys = _sample_inputs(case)
    x, y = stn_pixel(xs, ys, H, W)
    counts, n = region_counts(x, y, H, W, xs, ys)
    print(region_text(counts, n))
    assert regions_ok(counts, n), region_text(counts, n)
    o32 = oracle_sample(im, xs, ys)
    assert np.array_equal(o32, oracle_padded(im, x, y))
    nbad, worst, neq, _ = check_blend(replay_blend(im, x, y), im, x, y, o32)
    assert nbad == 0 and neq == 0, (nbad, worst, neq)
    print("oracle / bound %.3f" % worst)
    for mut in ("scale_W_for_Wm1",) + BLEND_MUTANTS:
        xm, ym = stn_pixel(xs, ys, H, W, mut)
        nb, _, ne, _ = check_blend(replay_blend(im, xm, ym, mut), im, x, y, o32)
        rej = max(nb, ne)
        floor = MUTANT_FLOOR[mut]
        if frames == "corners" and mut in ROUNDING_ONLY + ("taps_exchanged",):
            floor = 0.0
        if mut in ROUNDING_ONLY and o32.size < 1000:
            floor = 0.0
        print("%s: %.4f of the values rejected (floor %.4f)" % (mut, rej / o32.size, floor))
        assert rej >= floor * o32.size and (rej > 0 or floor == 0.0), (mut, rej, o32.size)
        if mut == "clamped_tap_as_value":
            assert nb >= floor * o32.size, "a ring tap read as a value must leave the float64 bound"


CPU_FLOW = [k for k in SEAMS if k[1] * k[2] <= CPU_MAX]


@pytest.mark.parametrize("B,H,W", CPU_FLOW, ids=["B%d-%dx%d" % k for k in CPU_FLOW])
def test_flow_checks_hold_for_the_replay_and_window_shares_are_as_built(B, H, W):
    from oracle.warp_with_optical_flow import tf_warp
    im = make_frames("noise", B, H, W, 3, seed=H + W)
    for group in ("const", "edges"):
        for name, (flow, want) in flows_for(group, B, H, W, SEAMS[B, H, W], seed=H * 7 + W).items():
            check_share(name, window_share(flow, SEAMS[B, H, W]), want)
            x, y = flow_pixel(flow)
            o32 = tf_warp(im, flow, H, W)
            nbad, worst, neq, _ = check_blend(replay_blend(im, x, y), im, x, y, o32)
            assert nbad == 0 and neq == 0, (name, nbad, worst, neq)


@pytest.mark.parametrize("key", [k for k in SEAMS if SEAMS[k][1] > 1], ids=lambda k: "B%d-%dx%d" % k)
def test_window_shares_of_the_multi_band_flows(key):
    B, H, W = key
    for group in ("const", "edges"):
        flows = flows_for(group, B, H, W, SEAMS[key], seed=H * 7 + W)
        assert group == "const" or "mixed" in flows
        for name, (flow, want) in flows.items():
            share = window_share(flow, SEAMS[key])
            check_share(name, share, want)
    # the window's far edges, by construction and not by chance: + 13.5 on x puts the last column of every strip whose
    # source column is inside the frame at dx == kFsCols - 1, + 13.5 on y the last row of a step at dy == kFsLive - 1
    flows = flows_for("const", B, H, W, SEAMS[key], seed=0)
    dx, _ = window_offsets(flows["const x +13.5"][0], SEAMS[key])
    assert int((dx == FS_COLS - 1).sum()) == B * H * sum(1 for c0 in range(0, W, FS_W) if c0 + FS_W - 1 + 13 <= W and c0 + FS_W <= W)
    _, dy = window_offsets(flows["const y +13.5"][0], SEAMS[key])
    assert int((dy == FS_LIVE - 1).sum()) >= B * W * (H // FS_STEP - 2)
    assert W < FS_W + 13 or int((dx == FS_COLS - 1).sum()) > 0


@pytest.mark.parametrize("H,W,B", MASK_SHAPES, ids=["%dx%d-B%d" % s for s in MASK_SHAPES])
def test_mask_plane_reference_agrees_with_the_oracle(H, W, B):
    from oracle import spatial_transformer as ost
    ones = np.ones((B, H, W, 1), dtype=F32)
    for fam in MASK_FAMILIES:
        theta = mask_theta(fam, B, seed=H + W)
        xs, ys = (a.reshape(B, -1) for a in replay_projective(theta, H, W))
        x, y = stn_pixel(xs, ys, H, W)
        o32 = ost.ProjectiveTransformer((H, W)).transform(ones, theta).reshape(B, -1, 1)
        nbad, worst, neq, _ = check_blend(replay_blend(ones, x, y), ones, x, y, o32)
        assert nbad == 0 and neq == 0, (fam, nbad, worst, neq)
        if fam in ("identity", "zero theta") and H * W > 1:
            assert (o32 == 1.0).all(), fam
        if fam == "plane 0" and min(H, W) > 1:
            assert (o32 == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU

LOG = []


def note(line):
    LOG.append(line)
    print("STNF64 " + line)


_dev, _stream = tps._dev, tps._stream


def gpu_grid(kind, theta, im, oh, ow, src=None, linv=None, want_xy=True):
    """dvsg_grid_{affine,projective,elastic}_f32 with every output between sentinels -> (out or None, x_s, y_s [B,oh*ow])"""
    import torch
    from coupe.dvsg_amd import _lib
    B = theta.shape[0]
    t = _dev(theta)
    H, W, C = im.shape[1:] if im is not None else (1, 1, 1)
    u = _dev(im) if im is not None else None
    n = B * oh * ow
    out = Guarded(n * C * 4, t.device) if im is not None else None
    gx = Guarded(n * 4, t.device) if want_xy else None
    gy = Guarded(n * 4, t.device) if want_xy else None
    tail = (u.data_ptr() if u is not None else None, B, H, W, C, oh, ow, out.ptr() if out else None,
            gx.ptr() if gx else None, gy.ptr() if gy else None, _stream())
    if kind == "elastic":
        keep = (_dev(linv), _dev(src))
        _lib.call("dvsg_grid_elastic_f32", t.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), src.shape[1], *tail)
    else:
        _lib.call("dvsg_grid_%s_f32" % kind, t.data_ptr(), *tail)
    torch.cuda.synchronize()
    for g in (out, gx, gy):
        assert g is None or g.intact(), "wrote past an output"
    f = torch.float32
    return (out.view(f, (B, oh * ow, C)).cpu().numpy() if out else None,
            gx.view(f, (B, oh * ow)).cpu().numpy() if gx else None, gy.view(f, (B, oh * ow)).cpu().numpy() if gy else None)


def gpu_sample(im, xs, ys, oh, ow):
    import torch
    from coupe.dvsg_amd import _lib
    B, H, W, C = im.shape
    u, a, b = _dev(im), _dev(xs), _dev(ys)
    out = Guarded(B * oh * ow * C * 4, u.device)
    _lib.call("dvsg_stn_sample_f32", u.data_ptr(), a.data_ptr(), b.data_ptr(), B, H, W, C, oh, ow, out.ptr(), _stream())
    torch.cuda.synchronize()
    assert out.intact(), "wrote past the output"
    return out.view(torch.float32, (B, oh * ow, C)).cpu().numpy()


def gpu_flow(u, fl, tiled):
    """dvsg_flow_warp_f32 on device tensors u [B,H,W,C], fl [B,H,W,2] with flow_tiled = `tiled` -> device tensor"""
    import torch
    from coupe.dvsg_amd import _lib
    B, H, W, C = u.shape
    out = Guarded(B * H * W * C * 4, u.device)
    try:
        _lib.call("dvsg_debug_set_option", b"flow_tiled", tiled)
        _lib.call("dvsg_flow_warp_f32", u.data_ptr(), fl.data_ptr(), B, H, W, C, out.ptr(), _stream())
    finally:
        _lib.call("dvsg_debug_set_option", b"flow_tiled", 1)
    torch.cuda.synchronize()
    assert out.intact(), "wrote past the output"
    return out.view(torch.float32, (B, H * W, C)).clone()


def gpu_mask(theta, H, W):
    import torch
    from coupe.dvsg_amd import _lib
    B = theta.shape[0]
    t = _dev(theta)
    out = Guarded(B * H * W * 4, t.device)
    _lib.call("dvsg_random_mask_plane_f32", t.data_ptr(), B, H, W, out.ptr(), _stream())
    torch.cuda.synchronize()
    assert out.intact(), "wrote past the plane"
    return out.view(torch.float32, (B, H * W, 1)).cpu().numpy()


def judge(tag, out, im, x, y, oracle):
    nbad, worst, neq, where = check_blend(out, im, x, y, oracle)
    note("%s: blend worst / bound %.3f, %d of %d values not bit-equal to the float32 oracle" % (tag, worst, neq, np.asarray(out).size))
    assert nbad == 0, "%s: %d values out of the float64 bound, first pixels (b, n) %s" % (tag, nbad, where[:4].tolist())
    assert neq == 0, "%s: %d values differ from the oracle, first pixels (b, n) %s" % (tag, neq, where[:4].tolist())
    return worst


def _judge_grid(case, xs, ys, theta, src, linv):
    """x_s, y_s [B,oh*ow] of a grid case against link 1 -> worst ratio"""
    from oracle import spatial_transformer as ost
    kind, oh, ow, B, par = case
    dummy = np.zeros((B, 1, 1, 1), dtype=F32)
    if kind == "affine":
        ref, E = affine_reference(theta, oh, ow)
        xo, yo = ost.AffineTransformer((oh, ow))._transform(dummy, theta)
    elif kind == "projective":
        ref, E = projective_reference(theta, oh, ow)
        xo, yo = ost.ProjectiveTransformer((oh, ow))._transform(dummy, theta)
    if kind != "elastic":
        assert np.array_equal(xs.reshape(-1), xo) and np.array_equal(ys.reshape(-1), yo), "x_s, y_s are not the oracle's bits"
        nbad, worst, at = check_grid(xs, ys, ref, E)
        assert nbad == 0, (nbad, worst, at)
        if par == "zq0":
            assert (xs.reshape(B, oh, ow)[:, :, 0] == 0).all() and (ys.reshape(B, oh, ow)[:, :, 0] == 0).all()
        return worst, None
    c64, Ec = coeff_reference(theta, linv)
    ref, E = elastic_reference(replay_coeff(theta, linv), None, src, oh, ow)
    nbad, worst, at = check_grid(xs, ys, ref, E)
    assert nbad == 0, ("map of the float32 coefficients", nbad, worst, at)
    refc, Ecm = elastic_reference(c64, Ec, src, oh, ow)
    nbad, worst_c, at = check_grid(xs, ys, refc, Ecm)
    assert nbad == 0, ("chain from the float64 coefficients", nbad, worst_c, at)
    return worst, worst_c


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID_CASES, ids=GRID_IDS)
def test_grid_against_float64_and_the_oracle(case):
    """link 1 on the image-less call; the call with an image writes the same x_s, y_s bits, and its pixels are link 2 at
    those coordinates"""
    kind, oh, ow, B, par = case
    theta, src, linv = _grid_inputs(case)
    _, xs, ys = gpu_grid(kind, theta, None, oh, ow, src, linv)
    worst, worst_c = _judge_grid(case, xs, ys, theta, src, linv)
    H, W, C = GRID_IMAGE[kind]
    im = make_frames("noise", B, H, W, C, seed=oh + ow)
    out, x2, y2 = gpu_grid(kind, theta, im, oh, ow, src, linv)
    assert np.array_equal(xs.view(np.uint32), x2.view(np.uint32)) and np.array_equal(ys.view(np.uint32), y2.view(np.uint32)), \
        "x_s, y_s differ between the image call and the image-less call"
    out2, _, _ = gpu_grid(kind, theta, im, oh, ow, src, linv, want_xy=False)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), "the pixels depend on whether x_s, y_s are requested"
    x, y = stn_pixel(xs, ys, H, W)
    tag = "grid %s %dx%d B=%d %s: x_s worst / bound %.3f%s" % (kind, oh, ow, B, par, worst, "" if worst_c is None else " (chain %.3f)" % worst_c)
    assert not np.isnan(x).any() and not np.isnan(y).any()                 # W, H >= 6: no Inf x 0
    judge(tag, out, im, x, y, oracle_sample(im, xs, ys))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", CHANNEL_FORMS)
def test_grid_channel_forms(kind, C):
    """the instantiations the main grid cases do not launch: the same x_s, y_s bits as the image-less call, pixels by link 2"""
    oh, ow, B = 7, 300, 2
    case = (kind, oh, ow, B, (3, 0.5) if kind == "elastic" else "random")
    theta, src, linv = _grid_inputs(case)
    H, W = 12, 10
    im = make_frames("positive", B, H, W, C, seed=C)
    out, xs, ys = gpu_grid(kind, theta, im, oh, ow, src, linv)
    worst, _ = _judge_grid(case, xs, ys, theta, src, linv)
    _, x2, y2 = gpu_grid(kind, theta, None, oh, ow, src, linv)
    assert np.array_equal(xs.view(np.uint32), x2.view(np.uint32)) and np.array_equal(ys.view(np.uint32), y2.view(np.uint32))
    x, y = stn_pixel(xs, ys, H, W)
    judge("grid %s C=%d %dx%d: x_s %.3f" % (kind, C, oh, ow, worst), out, im, x, y, oracle_sample(im, xs, ys))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SAMPLE_CASES, ids=SAMPLE_IDS)
def test_sampler_b_at_given_coordinates(case):
    H, W, C, oh, ow, B, frames = case
    im, xs, ys = _sample_inputs(case)
    x, y = stn_pixel(xs, ys, H, W)
    counts, n = region_counts(x, y, H, W, xs, ys)
    assert regions_ok(counts, n), region_text(counts, n)                  # chosen on the CPU, before the GPU is asked
    out = gpu_sample(im, xs, ys, oh, ow)
    judge("sampler B %dx%d C=%d -> %dx%d %s" % (H, W, C, oh, ow, frames), out, im, x, y, oracle_sample(im, xs, ys))
    note("    regions: " + region_text(counts, n))


@pytest.mark.gpu
def test_sampler_b_on_a_one_pixel_frame_and_single_rows():
    """W - 1 == 0 or H - 1 == 0: the scale multiplies by 0 (finite coordinates only: Inf x 0 is NaN, out of scope)"""
    for H, W, C in ((1, 1, 3), (1, 9, 1), (7, 1, 2)):
        im = make_frames("positive", 2, H, W, C, seed=H + W)
        xs, ys = region_coords(2, 37, max(H, 2), max(W, 2), seed=W, special=False)
        x, y = stn_pixel(xs, ys, H, W)
        judge("sampler B %dx%d C=%d" % (H, W, C), gpu_sample(im, xs, ys, 1, 37), im, x, y, oracle_sample(im, xs, ys))


@pytest.mark.gpu
def test_65_channels_are_refused_without_a_launch():
    import torch
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd._lib import DvsgError
    im = _dev(np.zeros((1, 4, 4, 65), dtype=F32))
    co = _dev(np.zeros((1, 16), dtype=F32))
    out = Guarded(16 * 65 * 4, im.device)
    for name, args in (("dvsg_stn_sample_f32", (im.data_ptr(), co.data_ptr(), co.data_ptr(), 1, 4, 4, 65, 4, 4, out.ptr(), _stream())),
                       ("dvsg_flow_warp_f32", (im.data_ptr(), co.data_ptr(), 1, 4, 4, 65, out.ptr(), _stream())),
                       ("dvsg_grid_affine_f32", (co.data_ptr(), im.data_ptr(), 1, 4, 4, 65, 4, 4, out.ptr(), None, None, _stream()))):
        status = getattr(_lib.load(), name)(*args)
        assert status == -1, (name, status)                               # DVSG_ERR_INVALID_ARG
        with pytest.raises(DvsgError, match="C=65"):
            _lib.check(status, name)
    torch.cuda.synchronize()
    assert bool((out.body == f64.SENTINEL).all()) and out.intact(), "a refused call wrote to its output"


def _flow_case(B, H, W, C, group, launch, misaligned=False):
    import torch
    from oracle.warp_with_optical_flow import tf_warp
    im = make_frames("noise" if (H + W) % 2 else "smooth", B, H, W, C, seed=H + W + C)
    if misaligned:
        buf = torch.empty(B * H * W * C + 1, device="cuda")
        u = buf[1:].reshape(B, H, W, C)
        u.copy_(torch.from_numpy(im))
        assert u.data_ptr() % 16 == 4
    else:
        u = _dev(im)
    worst_all = 0.0
    for name, (flow, want) in flows_for(group, B, H, W, launch, seed=H * 7 + W).items():
        share = window_share(flow, launch)
        check_share(name, share, want)                                    # on the CPU, before the GPU is asked
        fl = _dev(flow)
        outs = [gpu_flow(u, fl, v) for v in (0, 1, 2)]
        assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), \
            (name, "flow_tiled 1 / 2 differ from 0 at %d / %d values" % (int((outs[1] != outs[0]).sum()), int((outs[2] != outs[0]).sum())))
        x, y = flow_pixel(flow)
        tag = "flow %dx%dx%d B=%d%s %s (window share %.3f)" % (H, W, C, B, " off the 16-byte grid" if misaligned else "", name, share)
        worst_all = max(worst_all, judge(tag, outs[1].cpu().numpy(), im, x, y, tf_warp(im, flow, H, W)))
    return worst_all


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["const", "edges"])
@pytest.mark.parametrize("key", list(SEAMS), ids=lambda k: "B%d-%dx%d" % k)
def test_flow_warp_three_forms_the_oracle_and_float64(key, group):
    """C = 3: the gather kernel and the strip kernel in both dispatch orders give the same bits, the oracle's bits, and
    stay inside the float64 bound -- at every seam of the strip kernel"""
    B, H, W = key
    assert strip_launch(B, H, W) == SEAMS[key]
    _flow_case(B, H, W, 3, group, SEAMS[key])


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", GATHER_SHAPES)
def test_flow_warp_other_channel_counts(B, H, W, C):
    for group in ("const", "edges"):
        _flow_case(B, H, W, C, group, strip_launch(B, H, W))


@pytest.mark.gpu
def test_flow_warp_of_a_frame_off_the_16_byte_grid():
    for group in ("const", "edges"):
        _flow_case(2, 37, 53, 3, group, strip_launch(2, 37, 53), misaligned=True)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,B", MASK_SHAPES, ids=["%dx%d-B%d" % s for s in MASK_SHAPES])
def test_mask_plane_against_float64_the_image_kernel_and_the_oracle(H, W, B):
    from oracle import spatial_transformer as ost
    ones = np.ones((B, H, W, 1), dtype=F32)
    for fam in MASK_FAMILIES:
        theta = mask_theta(fam, B, seed=H + W)
        plane = gpu_mask(theta, H, W)
        img, xs, ys = gpu_grid("projective", theta, ones, H, W)
        xr, yr = (a.reshape(B, -1) for a in replay_projective(theta, H, W))
        assert np.array_equal(xs.view(np.uint32), xr.view(np.uint32)) and np.array_equal(ys.view(np.uint32), yr.view(np.uint32))
        assert np.array_equal(plane.view(np.uint32), img.view(np.uint32)), "%s: the plane is not stn_kernel<kProjective, 1> on ones" % fam
        x, y = stn_pixel(xs, ys, H, W)
        o32 = ost.ProjectiveTransformer((H, W)).transform(ones, theta).reshape(B, -1, 1)
        judge("mask plane %dx%d B=%d %s (mean %.3f)" % (H, W, B, fam, float(plane.mean())), plane, ones, x, y, o32)
        if fam in ("identity", "zero theta") and H * W > 1:
            assert (plane == 1.0).all(), fam
        if fam == "plane 0" and min(H, W) > 1:
            assert (plane == 0.0).all()
        if fam == "zq0":
            assert (xs.reshape(B, H, W)[:, :, 0] == 0).all() and (ys.reshape(B, H, W)[:, :, 0] == 0).all()
