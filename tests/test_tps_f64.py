"""The thin-plate-spline path of warp_kernels.hip pinned to float64: solver, cached inverse, grid and sampler A, every pixel.

No pixel is masked anywhere in this file.  The kernel writes its own source coordinates x_s, y_s, so the path is cut into
three links, and each link is held to a bound of its own that is derived below from the operations of the kernel (nothing
here was fitted to a GPU result; u = 2^-24, every bound carries a factor 1.01 for the second-order terms (1 + u)^k - 1 - k u,
k <= 70):

1.  T (tps_solve_kernel, tps_apply_kernel) against oracle.thin_plate_spline.solve_system(float64) on the float32 inputs.
    The kernel forms r = d2 logf(d2 + 1e-6f) in float32 (lines 60-63) and eliminates in float64, so its T solves a system
    whose r entries are perturbed.  dx, dy: one rounding each; dx dx, dy dy: one each, so each square is 3u off; their sum:
    d2 (1 + 4u), all terms positive.  e = fl(d2 + 1e-6f) is within 5u of d2 + eps relatively (d2 / e <= 1), so ln e moves by
    5u absolutely; logf is documented at 1 ulp, 2u |ln e|; the product rounds once more:
        |r_gpu - r| <= u d2 (4 |L| + 5 + 2 |L| + |L|) = u (5 d2 (|L| + 1) + 2 |r|),   L = ln(d2 + eps):   c1 = 5, c2 = 2.
    The oracle's float64 path adds the float64 constant 1e-6, the kernel float32(1e-6): |eps - eps32| <= 2.6e-14 changes r by
    at most d2 2.6e-14 / (d2 + eps) < 3e-14, added to every entry of DW.  The p entries and the right-hand side (coord +
    vector rounded to float32 on both sides) are exact in float64.  With A = |W^-1| DW and rho = ||A||_inf (asserted < 1/2)
        |T_gpu - T_64| <= A |T_64^T| / (1 - rho)  +  8 n 2^-53 |W^-1| |W| (|T_64^T| + |W^-1| |rhs|)  +  u (|T_64| + the two before)
    (the exact perturbation series instead of a stated second-order margin; the final float32 rounding).  The middle term is
    float64 arithmetic: the kernel eliminates with partial pivoting, forward error c n u64 |W^-1| |W| |T|; the reference
    multiplies by an explicit inverse (solve_system: inv(W) @ rhs), whose forward error is c n u64 |W^-1| |W| |W^-1| |rhs|
    (Higham, Accuracy and Stability, section 14.1) -- larger than the first where T comes out of cancellation; c = 8 for
    both.  At P = 3 and 4 the r part of T is zero or small (three points define an affine map), the first term vanishes and
    the bound is the final rounding alone, u |T| to seven digits: a correctly rounded float32 then sits anywhere up to
    half an ulp = u |T| from T_64, and the worst of 72 entries measures 0.96 (P = 3) and 0.87 (P = 4), on the GPU and in
    the CPU replay alike, at the same entry T[3, 0, 1] = 1.0413.  That is the rounding of the output format, not slack
    used up by the solver.
    tps_apply_kernel multiplies the float64 columns of W^-1 that the same solver produced from
    unit right-hand sides by the float64 right-hand side: the same perturbed system, the same bound.

2.  x_s, y_s (tps_warp_kernel, lines 472-491) against the float64 map of the float32 T handed to the kernel.  x_t, y_t are
    tf.linspace's own float32 operations on both sides (bit-identical inputs).  dx, dx dx, dy, dy dy, the sum: d2 (1 + 4u);
    e within 5u; v_log_f32 at the 1 ulp the ISA guide documents (2u |log2 e|); d2 l2 rounds once; the staged coefficient
    c_k = fl(T_k kLn2) rounds once and kLn2 = 0x1.62e43p-1 is 0.0461u above ln 2:
        Dr_k = u (a d2 (|L| + 1) + b d2 + c |r|),  a = 4 (d2's error through the product and through ln's argument),
               b = 1 (the rounding of e), c = 2 + 1 + 1 + 0.0461 -> 4.05 (log, product, T_k kLn2, kLn2 itself)
    and the accumulation ((T_0 + T_1 x_t) + T_2 y_t, then P fused multiply-adds in k order) rounds each of the P + 3 terms at
    most P + 4 times:
        E = sum_k |T_k| Dr_k + (P + 4) u S,     S = |T_0| + |T_1 x_t| + |T_2 y_t| + sum_k |T_k r_k|.
    A worst case like tau(K) S: a correct kernel is expected near 0.1 of it.

3.  Sampler A (sample_a_load / sample_a_blend) at the GPU's own float32 x_s, y_s.  The pixel coordinate x = ((x_s + 1) W) / 2
    and the clipped indices are taken in float32 exactly as the kernel takes them (three roundings that the float32 oracle
    restates), so reference and kernel always pick the same cell, on the jumps too.  From there, in float64:
        ref = sum_i w_i I_i,  |out - ref| <= g u sum_i |w_i| |I_i| + 4 x 2^-126,   g = 7:
    each weight factor (x1 - x etc.) rounds once (x and the index are float32 values), the weight once, the product once,
    and the first term passes three additions: 2 + 1 + 1 + 3.  (Two roundings per factor would give 9; the coordinate is an
    input here, so 7 is what the operations give and the tighter number is used.)  Far outside the frame the two x taps
    coincide, the weights are large and cancel, and sum |w| |I| is exactly the noise floor of that cancellation.
    Bit equality with oracle.interpolate_a at the same coordinates is expected everywhere (same operations, contraction
    off) and reported per case; it is asserted too, and a case where it did not hold would name the pixels.

Inputs put pixels on purpose where the earlier, masked tests removed them: each sampler case carries samples that are
affine-only (bit-exact grid), zoomed out past all four borders, squeezed into [-0.9, 0.9] px around the left / top border
and into [W - 1.9, W - 0.1] around the right / bottom one, shifted by 1.5 (beyond the frame), and held at x == 0 exactly
(on an integer and on the jump).  The fractions per region are computed with the float32 oracle before the GPU is asked,
asserted (each >= 1 % of the case's pixels or >= 50 pixels) and printed.  dvsg_stabilize_* compute their own F_t from the
network, so their coordinates are not this file's choice: their region counts are printed, not asserted.

CPU tests (no GPU): a NumPy float32 replay of the kernel's operation order (correctly rounded log2, FMA in float64 rounded
once) and the float32 oracle stay inside bound 2 at every small shape; the same checking functions reject ten simulated
wrong kernels at every (shape, P) with a stated floor on the failing fraction; the table names every tps_* kernel of the
built library.

Measured on one MI355X (profiles/r05_tps_f64.log; worst |got - ref| / bound per link; the 55 GPU cases of this file run in 3 s):
    solver       P = 3: 0.96, 4: 0.87 (output rounding, see above), 9: 0.16, 16: 0.12, 25: 0.11, 49: 0.07, 61: 0.07
    cached W^-1  0.025-0.030 at B = 1, 5, 64 (V_src, P = 25), the same figure as dvsg_tps_solve_f32 on the same inputs
    grid         0.015-0.38 in the grid-only cases, 0.18-0.53 in the sampler cases (whose T is mostly affine, so the bound is
                 mostly the P + 4 roundings of the accumulation); 0.064 at 1280 x 720, 0.058 on the 3840 x 2160 rows.  The CPU
                 replay with a correctly rounded log2 gives 0.02-0.31 on the same grid-only cases: v_log_f32 shows no excess
                 over the 1 ulp that the bound assumes
    sampler A    at most 0.49 of the float64 bound; 0 of 1 230 870 values not bit-equal to oracle.interpolate_a
    regions      7-33 % of a case's pixels in each of the six regions in every dvsg_tps_warp_f32 case; the render cases
                 9-10 % in the y cells, 0.1-1 % (>= 50 pixels) in the x cells; the network-driven calls 0.2-1.9 % (printed only)
No kernel defect was found.  Two mutations of warp_kernels.hip on a scratch copy (the x1 clip moved after the weights for
x >= W - 1; the last row of a partial last row group not produced) fail 22 and 32 of the 55 GPU cases here.
"""
import math
import re

import numpy as np
import pytest

import test_conv_gemm_f64 as f64

Guarded, TINY = f64.Guarded, f64.TINY

F32 = np.float32
U24 = 2.0 ** -24
SECOND = 1.01                                     # (1 + u)^k - 1 <= 1.01 k u for k <= 70
KLN2 = F32(float.fromhex("0x1.62e43p-1"))
EPS32 = float(F32(1e-6))
SOLVE_C1, SOLVE_C2 = 5.0, 2.0
GRID_A, GRID_B, GRID_C = 4.0, 1.0, 4.05
G_BLEND = 7.0

assert abs(float(KLN2) / math.log(2.0) - 1.0) / U24 < 0.05      # the 0.0461 of the docstring, rounded up in GRID_C


# ---------------------------------------------------------------------------------------------------------------------
# inputs (NumPy, seeded)

def control_points(P, B, jitter, seed=0):
    """[B,P,2] float32: the first P nodes of the smallest square grid that holds P (P = 3: a triangle, 61: 8 x 8 less three),
    the same for every sample, or moved per sample by up to 0.3 of the spacing"""
    g = max(2, int(math.ceil(math.sqrt(P))))
    lin = np.linspace(-1.0, 1.0, g)
    pts = np.array([[x, y] for y in lin for x in lin])[:P]
    out = np.tile(pts[None], (B, 1, 1))
    if jitter:
        out = out + np.random.default_rng(seed).uniform(-0.3, 0.3, out.shape) * (2.0 / (g - 1))
    return np.ascontiguousarray(out, dtype=F32)


def node_points(P, B, oh, ow):
    """control points ON nodes of the float32 output grid (d2 == 0 occurs at P pixels per sample)"""
    from oracle.tfops import tf_linspace
    xl, yl = tf_linspace(-1.0, 1.0, ow), tf_linspace(-1.0, 1.0, oh)
    rng = np.random.default_rng(P * 1000 + oh * 10 + ow)
    cells = rng.choice(oh * ow, size=P, replace=oh * ow < P)
    pts = np.stack([xl[cells % ow], yl[cells // ow]], 1)
    return np.ascontiguousarray(np.tile(pts[None], (B, 1, 1)), dtype=F32)


def vectors(B, P, scale, shift, seed):
    v = np.random.default_rng(seed).standard_normal((B, P, 2)) * scale
    v[..., 0] += shift
    return v.astype(F32)


def solved_T(coord, vec):
    """float32 T of the float64 solve (P >= 3)"""
    from oracle import thin_plate_spline as otps
    rhs = (coord + vec).astype(F32)
    return otps.solve_system(coord.astype(np.float64), rhs.astype(np.float64), dtype=np.float64).astype(F32)


def grid_T(coord, scale, shift, seed):
    """T for a grid case: the solve for P >= 3, identity + scaled noise below (the solver takes P >= 3, the grid P >= 1)"""
    B, P, _ = coord.shape
    if P >= 3:
        return solved_T(coord, vectors(B, P, scale, shift, seed))
    rng = np.random.default_rng(seed)
    T = np.zeros((B, 2, P + 3))
    T[:, 0, 1] = T[:, 1, 2] = 1.0
    T += rng.standard_normal(T.shape) * scale
    T[:, 0, 0] += shift
    return T.astype(F32)


KINDS = ("affine", "zoom", "lefttop", "rightbottom", "shift", "xzero")


def sampler_T(B, P, H, W, seed):
    """[B,2,P+3] float32, sample b of kind KINDS[b % 6] (see the docstring of this file)"""
    rng = np.random.default_rng(seed)
    T = np.zeros((B, 2, P + 3))
    for b in range(B):
        kind = KINDS[b % len(KINDS)]
        wob = 0.0
        if kind == "affine":
            T[b, 0, 1] = T[b, 1, 2] = 1.0
        elif kind == "zoom":
            c, s = 1.2 * math.cos(0.1), 1.2 * math.sin(0.1)
            T[b, 0, :3] = (0.01, c, -s)
            T[b, 1, :3] = (-0.02, s, c)
            wob = 0.05
        elif kind == "lefttop":
            T[b, 0, :3] = (-1.0, 1.8 / W, 0.0)
            T[b, 1, :3] = (-1.0, 0.0, 1.8 / H)
            wob = 0.05 / max(H, W)
        elif kind == "rightbottom":
            T[b, 0, :3] = (-1.0 + 2.0 * (W - 1) / W, 1.8 / W, 0.0)
            T[b, 1, :3] = (-1.0 + 2.0 * (H - 1) / H, 0.0, 1.8 / H)
            wob = 0.05 / max(H, W)
        elif kind == "shift":
            T[b, 0, :3] = (1.5, 1.0, 0.0)
            T[b, 1, :3] = (0.0, 0.0, 1.0)
            wob = 0.05
        else:                                      # x == 0 exactly at every pixel, y the identity
            T[b, 0, :3] = (-1.0, 0.0, 0.0)
            T[b, 1, :3] = (0.0, 0.0, 1.0)
        T[b, :, 3:] = rng.standard_normal((2, P)) * wob / math.sqrt(P)
    return T.astype(F32)


def make_frames(kind, B, H, W, C, seed):
    import inputs as tin
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        return tin.smooth_frames(seed, B, H, W, C, factor=4)
    if kind == "ones":
        return np.ones((B, H, W, C), dtype=F32)
    v = rng.uniform(-1.0, 1.0, (B, H, W, C))
    return (v * (1e4 if kind == "big" else 1.0)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# link 1: T

def solve_reference(coord, rhs):
    """(T64 [B,2,n], E [B,2,n], rho) for float32 control points [B,P,2] and float32 right-hand-side points [B,P,2]"""
    from oracle import thin_plate_spline as otps
    c = np.asarray(coord, dtype=F32).astype(np.float64)
    y = np.asarray(rhs, dtype=F32).astype(np.float64)
    B, P, _ = c.shape
    n = P + 3
    T = otps.solve_system(c, y, dtype=np.float64)
    d2 = np.square(c[:, :, None, :] - c[:, None, :, :]).sum(-1)
    L = np.log(d2 + EPS32)
    r = d2 * L
    p = np.concatenate([np.ones((B, P, 1)), c], 2)
    Wm = np.zeros((B, n, n))
    Wm[:, :P, :3], Wm[:, :P, 3:], Wm[:, P:, 3:] = p, r, p.transpose(0, 2, 1)
    M = np.abs(np.linalg.inv(Wm))
    DW = np.zeros((B, n, n))
    DW[:, :P, 3:] = SECOND * U24 * (SOLVE_C1 * d2 * (np.abs(L) + 1.0) + SOLVE_C2 * np.abs(r)) + 3e-14
    A = M @ DW
    rho = float(A.sum(-1).max())
    Tt = np.abs(T).transpose(0, 2, 1)                                     # [B,n,2]
    tp = np.concatenate([np.abs(y), np.zeros((B, 3, 2))], 1)
    MW = M @ np.abs(Wm)
    E = (A @ Tt) / (1.0 - rho) + 8.0 * n * 2.0 ** -53 * (MW @ Tt + MW @ (M @ tp))
    E = E + U24 * (Tt + E)
    return T, E.transpose(0, 2, 1), rho


def check_T(T, T64, E):
    """(number of entries out of bounds, worst |T - T64| / E); NaN counts as out"""
    d = np.abs(np.asarray(T, dtype=np.float64) - T64)
    bad = ~(d <= E)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(E > 0, d / E, np.where(d > 0, np.inf, 0.0))
    return int(bad.sum()), float(np.nan_to_num(q, nan=np.inf).max())


def replay_solve(coord, rhs, mut=None):
    """the kernel's system -- r in separately rounded float32 -- solved in float64, rounded to float32"""
    c = np.asarray(coord, dtype=F32)
    B, P, _ = c.shape
    n = P + 3
    dx = (c[:, :, None, 0] - c[:, None, :, 0]).astype(F32)
    dy = (c[:, :, None, 1] - c[:, None, :, 1]).astype(F32)
    d2 = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d2 if mut == "no_eps" else (d2 + F32(1e-6)).astype(F32)
        r = (d2 * np.log(e).astype(F32)).astype(F32)
    p = np.concatenate([np.ones((B, P, 1)), c.astype(np.float64)], 2)
    Wm = np.zeros((B, n, n))
    Wm[:, :P, :3], Wm[:, :P, 3:], Wm[:, P:, 3:] = p, r.astype(np.float64), p.transpose(0, 2, 1)
    tp = np.concatenate([np.asarray(rhs, dtype=F32).astype(np.float64), np.zeros((B, 3, 2))], 1)
    if not np.isfinite(Wm).all():
        return np.full((B, 2, n), np.nan, dtype=F32)
    T = np.linalg.solve(Wm, tp).transpose(0, 2, 1)
    if mut == "swap_rows":
        T = T[:, ::-1]
    return np.ascontiguousarray(T).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# link 2: the grid

def grid_reference(T, coord, oh, ow, rows=None):
    """(ref, E) [B,2,R,ow] float64: the map of float32 T [B,2,P+3] and float32 control points [B or 1,P,2] on output rows
    `rows` (default all), and its per-pixel bound"""
    return grid_terms(T, coord, oh, ow, rows)[:2]


def grid_terms(T, coord, oh, ow, rows=None):
    """(ref, E, S) of grid_reference; T may be float64 (then S = sum_k |T_k| |basis_k| of exactly those values)"""
    from oracle.tfops import tf_linspace
    T = np.asarray(T, dtype=np.float64)
    c = np.asarray(coord, dtype=F32).astype(np.float64)
    B, P = T.shape[0], T.shape[2] - 3
    X = tf_linspace(-1.0, 1.0, ow).astype(np.float64)[None, :]
    yl = tf_linspace(-1.0, 1.0, oh).astype(np.float64)
    Y = (yl if rows is None else yl[np.asarray(rows)])[:, None]
    ref = np.empty((B, 2, Y.shape[0], ow))
    E = np.empty_like(ref)
    Ss = np.empty_like(ref)
    for b in range(B):
        cb = c[b % c.shape[0]]
        acc = [T[b, k, 0] + T[b, k, 1] * X + T[b, k, 2] * Y for k in range(2)]
        S = [np.abs(T[b, k, 0]) + np.abs(T[b, k, 1] * X) + np.abs(T[b, k, 2] * Y) for k in range(2)]
        D = [0.0, 0.0]
        for q in range(P):
            d2 = np.square(X - cb[q, 0]) + np.square(Y - cb[q, 1])
            L = np.log(d2 + EPS32)
            r = d2 * L
            dr = U24 * (GRID_A * d2 * (np.abs(L) + 1.0) + GRID_B * d2 + GRID_C * np.abs(r))
            for k in range(2):
                t = T[b, k, 3 + q]
                acc[k] = acc[k] + t * r
                S[k] = S[k] + np.abs(t * r)
                D[k] = D[k] + abs(t) * dr
        for k in range(2):
            ref[b, k] = acc[k]
            E[b, k] = SECOND * (D[k] + (P + 4) * U24 * S[k])
            Ss[b, k] = S[k]
    return ref, E, Ss


def check_grid(xs, ys, ref, E):
    """x_s, y_s [B,R*ow] (any shape of that size) against (ref, E): (number of values out of bounds, worst ratio,
    index (b, k, row, column) of the worst)"""
    got = np.stack([np.asarray(xs, dtype=np.float64).reshape(ref[:, 0].shape),
                    np.asarray(ys, dtype=np.float64).reshape(ref[:, 0].shape)], 1)
    d = np.abs(got - ref)
    bad = ~(d <= E)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(E > 0, d / E, np.where(d > 0, np.inf, 0.0))
    q = np.nan_to_num(q, nan=np.inf)
    return int(bad.sum()), float(q.max()), tuple(int(v) for v in np.unravel_index(int(q.argmax()), q.shape))


GRID_MUTANTS = ("skip_point", "swap_rows", "no_eps", "ln2_twice", "step_W", "row_off")


def replay_grid(T, coord, oh, ow, mut=None):
    """tps_warp_kernel lines 437-495 in NumPy float32, one rounding per operation, log2 correctly rounded, the fused
    multiply-add in float64 rounded once; `mut` names a simulated defect.  Returns x_s, y_s [B,oh,ow] float32."""
    T = np.asarray(T, dtype=F32)
    coord = np.asarray(coord, dtype=F32)
    B, P = T.shape[0], T.shape[2] - 3
    if mut == "swap_rows":
        T = T[:, ::-1]

    def lin(n):
        den = n if mut == "step_W" else n - 1
        step = F32(F32(2.0) / F32(den)) if n > 1 else F32(0.0)
        return (F32(-1.0) + (step * np.arange(n, dtype=F32)).astype(F32)).astype(F32)
    xl, yl = lin(ow), lin(oh)
    if mut == "row_off" and oh % 4:
        i = np.arange(oh)
        last = i >= oh - oh % 4
        step = F32(F32(2.0) / F32(oh - 1)) if oh > 1 else F32(0.0)
        yl = np.where(last, (F32(-1.0) + (step * (i + 1).astype(F32)).astype(F32)).astype(F32), yl).astype(F32)
    X, Y = xl[None, :], yl[:, None]
    out = np.empty((B, 2, oh, ow), dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            cb = coord[b % coord.shape[0]]
            acc = []
            for k in range(2):
                a = (T[b, k, 0] + (T[b, k, 1] * X).astype(F32)).astype(F32)
                acc.append((a + (T[b, k, 2] * Y).astype(F32)).astype(F32) + np.zeros((oh, ow), dtype=F32))
            for q in range(P):
                if mut == "skip_point" and q == P // 2:
                    continue
                dx = (X - cb[q, 0]).astype(F32)
                dy = (Y - cb[q, 1]).astype(F32)
                d2 = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
                e = d2 if mut == "no_eps" else (d2 + F32(1e-6)).astype(F32)
                l2 = np.log2(e.astype(np.float64)).astype(F32)
                rk = (d2 * l2).astype(F32)
                for k in range(2):
                    ck = F32(T[b, k, 3 + q] * KLN2)
                    if mut == "ln2_twice":
                        ck = F32(ck * KLN2)
                    acc[k] = (np.float64(ck) * rk.astype(np.float64) + acc[k].astype(np.float64)).astype(F32)
            out[b, 0], out[b, 1] = acc
    return out[:, 0], out[:, 1]


# ---------------------------------------------------------------------------------------------------------------------
# link 3: sampler A

def pixel_coords(xs, ys, H, W, mut=None):
    """the kernel's float32 pixel coordinate ((x_s + 1) W) / 2, lines 231-232"""
    wf, hf = (F32(W - 1), F32(H - 1)) if mut == "scale_Wm1" else (F32(W), F32(H))
    x = (((np.asarray(xs, dtype=F32) + F32(1.0)).astype(F32) * wf).astype(F32) / F32(2.0)).astype(F32)
    y = (((np.asarray(ys, dtype=F32) + F32(1.0)).astype(F32) * hf).astype(F32) / F32(2.0)).astype(F32)
    return x, y


def _cells(x, y, H, W):
    x0 = np.floor(x).astype(np.int64)
    y0 = np.floor(y).astype(np.int64)
    return (np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1), x0, y0)


def sampler_reference(U, xs, ys):
    """(ref, E) [B,N,C] float64 for frames U [B,H,W,C] float32 at float32 coordinates xs, ys [B,N]"""
    U = np.asarray(U, dtype=F32)
    B, H, W, C = U.shape
    x, y = pixel_coords(xs, ys, H, W)
    x0, x1, y0, y1, _, _ = _cells(x, y, H, W)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    bi = np.arange(B)[:, None]
    U64 = U.astype(np.float64)
    ref = np.zeros(x.shape + (C,))
    S = np.zeros_like(ref)
    for w, yy, xx in (((x1 - xd) * (y1 - yd), y0, x0), ((x1 - xd) * (yd - y0), y1, x0),
                      ((xd - x0) * (y1 - yd), y0, x1), ((xd - x0) * (yd - y0), y1, x1)):
        t = w[..., None] * U64[bi, yy, xx]
        ref += t
        S += np.abs(t)
    return ref, SECOND * G_BLEND * U24 * S + 4.0 * TINY


SAMPLER_MUTANTS = ("scale_Wm1", "weights_before_clip", "swap_taps")


def replay_sampler(U, xs, ys, mut=None):
    """sample_a_load / sample_a_blend in NumPy float32 (oracle.interpolate_a's operations; bit-identical to it without
    `mut`, which a CPU test asserts) with a simulated defect"""
    U = np.asarray(U, dtype=F32)
    B, H, W, C = U.shape
    x, y = pixel_coords(xs, ys, H, W, mut)
    x0, x1, y0, y1, fx, fy = _cells(x, y, H, W)
    if mut == "weights_before_clip":
        x0f, x1f, y0f, y1f = fx.astype(F32), (fx + 1).astype(F32), fy.astype(F32), (fy + 1).astype(F32)
    else:
        x0f, x1f, y0f, y1f = x0.astype(F32), x1.astype(F32), y0.astype(F32), y1.astype(F32)
    bi = np.arange(B)[:, None]
    Ia, Ib, Ic, Id = U[bi, y0, x0], U[bi, y1, x0], U[bi, y0, x1], U[bi, y1, x1]
    if mut == "swap_taps":
        Ib, Ic = Ic, Ib
    wa = ((x1f - x).astype(F32) * (y1f - y).astype(F32)).astype(F32)[..., None]
    wb = ((x1f - x).astype(F32) * (y - y0f).astype(F32)).astype(F32)[..., None]
    wc = ((x - x0f).astype(F32) * (y1f - y).astype(F32)).astype(F32)[..., None]
    wd = ((x - x0f).astype(F32) * (y - y0f).astype(F32)).astype(F32)[..., None]
    s = ((wa * Ia).astype(F32) + (wb * Ib).astype(F32)).astype(F32)
    s = (s + (wc * Ic).astype(F32)).astype(F32)
    return (s + (wd * Id).astype(F32)).astype(F32)


def check_sampler(out, U, xs, ys):
    """out [B,N,C] (any shape of that size) at the coordinates xs, ys [B,N] it was sampled at: (values out of the float64
    bound, worst ratio, values not bit-equal to the float32 oracle, pixels (b, n) with a value out of bounds)"""
    from oracle import thin_plate_spline as otps
    ref, E = sampler_reference(U, xs, ys)
    got = np.asarray(out, dtype=F32).reshape(ref.shape)
    d = np.abs(got.astype(np.float64) - ref)
    bad = ~(d <= E)
    q = np.nan_to_num(d / E, nan=np.inf)
    o32 = otps.interpolate_a(U, xs, ys)
    neq = got.view(np.uint32) != np.ascontiguousarray(o32, dtype=F32).view(np.uint32)
    neq &= ~((got == 0) & (o32 == 0))                                     # +0 and -0 are the same value
    return int(bad.sum()), float(q.max()), int(neq.sum()), np.argwhere(bad.any(-1) | neq.any(-1))


REGIONS = ("x in [-1,0)", "x in [W-1,W)", "y in [-1,0)", "y in [H-1,H)", "on an integer", "beyond the frame")


def region_counts(xs, ys, H, W):
    x, y = pixel_coords(xs, ys, H, W)
    return ((int(((x >= -1) & (x < 0)).sum()), int(((x >= W - 1) & (x < W)).sum()), int(((y >= -1) & (y < 0)).sum()),
             int(((y >= H - 1) & (y < H)).sum()), int(((x == np.floor(x)) | (y == np.floor(y))).sum()),
             int(((x < -1) | (x >= W) | (y < -1) | (y >= H)).sum())), x.size)


def regions_ok(counts, n):
    return all(c >= 50 or c >= 0.01 * n for c in counts)


def region_text(counts, n):
    return ", ".join("%s %.1f %%" % (name, 100.0 * c / n) for name, c in zip(REGIONS, counts))


# ---------------------------------------------------------------------------------------------------------------------
# the case tables

SOLVE_P = (3, 4, 9, 16, 25, 49, 61)
SOLVE_RHS = ((0.05, 0.0), (0.5, 0.0), (0.05, 1.5))                       # (scale, shift)

# grid: (out_h, out_w, P, B, (scale, shift), jitter, T multiplier); x_s / y_s only (U = NULL)
GRID_CASES = [
    (37, 53, 25, 2, (0.05, 0.0), False, 1.0), (72, 128, 25, 2, (0.5, 1.5), False, 1.0), (72, 128, 25, 2, (0.5, 0.0), True, 1e3),
    (1, 1, 4, 2, (0.05, 0.0), False, 1.0), (2, 2, 1, 2, (0.5, 0.0), False, 1.0), (3, 255, 16, 2, (0.05, 0.0), True, 1.0),
    (4, 256, 49, 2, (0.5, 0.0), False, 1.0), (5, 257, 61, 2, (0.05, 1.5), True, 1.0), (7, 300, 4, 6, (0.5, 0.0), True, 1.0),
    (37, 513, 16, 1, (0.05, 0.0), False, 1.0), (2, 1280, 61, 1, (0.5, 0.0), True, 1.0), (720, 1, 49, 1, (0.05, 0.0), False, 1.0),
    (5, 2, 1, 64, (0.05, 1.5), False, 1.0), (720, 1280, 25, 1, (0.05, 0.0), False, 1.0), (3, 5, 25, 64, (0.5, 0.0), True, 1.0),
]
GRID_4K = (2160, 3840, 25, 1, (0.05, 0.0), False, 1.0)
GRID_4K_ROWS = (0, 1, 2, 3, 1078, 1079, 1080, 1081, 2156, 2157, 2158, 2159)
CPU_GRID_MAX = 72 * 128                                                    # the replay runs at every case up to this size

# sampler through dvsg_tps_warp_f32: (H, W, out_h, out_w, C, P, frames)
WARP_CASES = [
    (37, 53, 37, 53, 3, 25, "smooth"), (72, 128, 72, 128, 3, 25, "noise"), (32, 64, 33, 65, 3, 16, "ones"),
    (5, 300, 7, 300, 3, 4, "noise"), (37, 53, 50, 70, 1, 49, "noise"), (72, 128, 30, 61, 1, 1, "ones"),
    (37, 53, 37, 53, 2, 25, "smooth"), (16, 24, 21, 19, 4, 61, "noise"), (37, 53, 20, 90, 5, 25, "big"),
    (16, 24, 16, 24, 18, 4, "noise"), (9, 11, 13, 10, 21, 16, "ones"), (8, 8, 9, 7, 64, 25, "noise"), (2, 3, 5, 7, 3, 1, "noise"),
]
WARP_B = 6


def warp_instantiation(C):
    return ("tps_warp_kernel", 3 if C == 3 else (1 if C == 1 else 0), "f", "f")


# every tps_* kernel of the library and the GPU tests of this file that launch it
COVERED = {
    ("tps_solve_kernel",): ["test_solver_against_float64", "test_cached_inverse_against_float64 (the handle's W^-1 columns)"],
    ("tps_apply_kernel",): ["test_cached_inverse_against_float64", "test_render_u8", "test_whole_graph"],
    ("tps_warp_kernel", 3, "f", "f"): ["test_warp_sampler (C = 3)", "test_grid", "test_ring_forms (float32, in place)"],
    ("tps_warp_kernel", 1, "f", "f"): ["test_warp_sampler (C = 1)"],
    ("tps_warp_kernel", 0, "f", "f"): ["test_warp_sampler (C = 2, 4, 5, 18, 21, 64)"],
    ("tps_warp_kernel", 3, "h", "f"): ["test_ring_forms (uint8 pool)"],
    ("tps_warp_kernel", 3, "h", "h"): ["test_render_u8"],
}

_MANGLED = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+(tps_[a-z]+_kernel)(?:ILi(\d+)E([fh])([fh])EE)?")


def library_instantiations():
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    return {(n.decode(),) if not c else (n.decode(), int(c), a.decode(), b.decode()) for n, c, a, b in _MANGLED.findall(data)}


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests

def test_table_covers_every_tps_kernel_of_the_library():
    """two plain kernels and five tps_warp_kernel<C, TU, TO> when this was written; a new one without a case fails here"""
    found = library_instantiations()
    assert len(found) >= 7, sorted(found)
    assert found == set(COVERED), (sorted(found - set(COVERED)), sorted(set(COVERED) - found))
    assert {warp_instantiation(c[4]) for c in WARP_CASES} == {k for k in COVERED if k[0] == "tps_warp_kernel" and k[2:] == ("f", "f")}
    assert {2, 4, 5, 18, 21, 64} <= {c[4] for c in WARP_CASES}


def test_shapes_meet_every_row_residue_and_a_partial_column_block():
    ohs = {c[0] for c in GRID_CASES} | {c[2] for c in WARP_CASES}
    ows = {c[1] for c in GRID_CASES} | {c[3] for c in WARP_CASES}
    assert {0, 1, 2, 3} <= {h % 4 for h in ohs} and {1, 2, 3, 4, 5, 7, 37, 72, 720} <= ohs
    assert {1, 2, 53, 255, 256, 257, 300, 513, 1280} <= ows
    assert {1, 4, 16, 25, 49, 61} <= {c[2] for c in GRID_CASES} and max(c[3] for c in GRID_CASES) == 64
    assert any((c[0], c[1]) != (c[2], c[3]) and c[2] * c[3] > c[0] * c[1] for c in WARP_CASES)
    assert any(c[2] * c[3] < c[0] * c[1] for c in WARP_CASES)


def _solve_inputs(P, jitter, scale, shift, is_vec, B=6):
    coord = control_points(P, B, jitter, seed=P)
    vec = vectors(B, P, scale, shift, seed=P * 7 + int(jitter))
    rhs_in = vec if is_vec else (coord + vec).astype(F32)
    return coord, rhs_in, (coord + rhs_in).astype(F32) if is_vec else rhs_in


@pytest.mark.parametrize("P", SOLVE_P)
def test_solver_bound_holds_for_a_float32_built_system_and_flags_defects(P):
    """the float32-built system solved in float64 (what the kernel does) is inside bound 1 at every case of the GPU test;
    swapped rows, a vector that is not added and a dropped epsilon (NaN on the diagonal) are flagged"""
    for jitter in (False, True):
        for scale, shift in SOLVE_RHS:
            coord, rhs_in, rhs = _solve_inputs(P, jitter, scale, shift, True)
            T64, E, rho = solve_reference(coord, rhs)
            assert rho < 0.5, rho
            nbad, worst = check_T(replay_solve(coord, rhs), T64, E)
            assert nbad == 0 and worst <= 1.0, (P, jitter, scale, shift, worst)
            assert check_T(replay_solve(coord, rhs, "swap_rows"), T64, E)[0] >= P, "rows swapped"
            assert check_T(replay_solve(coord, rhs_in), T64, E)[0] >= 2 * 6, "vector not added"      # the identity, B = 6
            assert check_T(replay_solve(coord, rhs, "no_eps"), T64, E)[0] == T64.size, "epsilon dropped"
            # the float32 oracle solves in float32 (LU noise of its own): not held to this bound, only finite
            assert np.isfinite(T64).all()


def _grid_inputs(case, nodes=False):
    oh, ow, P, B, (scale, shift), jitter, mult = case
    coord = control_points(P, B, jitter, seed=oh + ow)
    T = grid_T(coord, scale, shift, seed=oh * 31 + ow)
    if nodes:                                      # the same T on moved control points: the grid kernel does not care
        coord = node_points(P, B, oh, ow)
    return coord, (T.astype(np.float64) * mult).astype(F32)


CPU_GRID = [c for c in GRID_CASES if c[0] * c[1] <= CPU_GRID_MAX]
# the fraction of the case's 2 B out_h out_w values that must be out of bounds, floors from this CPU run (the measured
# fractions are 2-10 x higher; a "row_off" defect only exists where out_h % 4 != 0 and moves only the rows of the last group)
FLOOR = {"skip_point": 0.5, "swap_rows": 0.5, "ln2_twice": 0.5, "step_W": 0.25}


@pytest.mark.parametrize("case", CPU_GRID, ids=["%dx%d-P%d-B%d" % c[:4] for c in CPU_GRID])
def test_grid_bound_holds_for_replay_and_oracle_and_flags_defects(case):
    from oracle import thin_plate_spline as otps
    oh, ow, P, B, _, _, mult = case
    B = min(B, 3)
    coord, T = _grid_inputs(case)
    coord, T = coord[:B], T[:B]
    ref, E = grid_reference(T, coord, oh, ow)
    nbad, worst, at = check_grid(*replay_grid(T, coord, oh, ow), ref, E)
    assert nbad == 0, ("replay", worst, at)
    xo, yo = otps.source_coords(T, coord, oh, ow)
    nbad, worst_o, at = check_grid(xo, yo, ref, E)
    assert nbad == 0, ("oracle", worst_o, at)
    print("replay / bound %.3f, oracle / bound %.3f" % (worst, worst_o))
    n = ref.size
    for mut in GRID_MUTANTS:
        if mut == "no_eps":
            continue
        if mut == "row_off" and (oh % 4 == 0 or oh == 1):
            continue
        if mut == "step_W" and oh == 1 and ow == 1:
            continue
        nb = check_grid(*replay_grid(T, coord, oh, ow, mut), ref, E)[0]
        if mut == "row_off":
            floor = 0.5 * (oh % 4) / oh
        elif mut == "step_W":
            floor = FLOOR[mut] if min(oh, ow) > 2 else 1.0 / (4 * oh * ow)
        else:
            floor = FLOOR[mut]
        if mut == "swap_rows" and oh * ow == 1:
            floor = 0.0 if nb else 1.0            # one pixel at (-1, -1): x_s and y_s may only differ through T
            nb = max(nb, int(not np.array_equal(T[:, 0], T[:, 1])))
        assert nb >= max(1, floor * n), (mut, nb, n)
    # epsilon dropped: control points on grid nodes, d2 == 0 there, 0 x log2(0) = NaN at exactly those pixels
    if oh * ow >= P:
        cn, Tn = _grid_inputs(case, nodes=True)
        cn, Tn = cn[:B], Tn[:B]
        refn, En = grid_reference(Tn, cn, oh, ow)
        assert check_grid(*replay_grid(Tn, cn, oh, ow), refn, En)[0] == 0
        xs, ys = replay_grid(Tn, cn, oh, ow, "no_eps")
        assert np.isnan(xs).reshape(B, -1).sum(1).min() >= 1
        assert check_grid(xs, ys, refn, En)[0] >= 2 * B


def _sampler_inputs(case, B=WARP_B):
    from oracle import thin_plate_spline as otps
    H, W, oh, ow, C, P, frames = case
    coord = control_points(P, B, True, seed=H * W + C)
    T = sampler_T(B, P, H, W, seed=oh * ow + P)
    U = make_frames(frames, B, H, W, C, seed=C * 100 + H)
    xs, ys = otps.source_coords(T, coord, oh, ow)
    return U, coord, T, xs, ys


@pytest.mark.parametrize("case", WARP_CASES, ids=["%dx%d-%dx%d-C%d-P%d-%s" % c for c in WARP_CASES])
def test_sampler_checks_cover_the_regions_and_flag_defects(case):
    """on the oracle's coordinates: every region is populated, the float32 oracle is inside bound 3 and bit-equal to the
    replay, and each simulated sampler defect is flagged on at least 2 % of the values (1 % for exchanged taps, which a
    frame of ones cannot show: there the floor is 0 and the other frames carry it)"""
    from oracle import thin_plate_spline as otps
    H, W, oh, ow, C, P, frames = case
    U, coord, T, xs, ys = _sampler_inputs(case)
    counts, n = region_counts(xs, ys, H, W)
    print(region_text(counts, n))
    assert regions_ok(counts, n), region_text(counts, n)
    o32 = otps.interpolate_a(U, xs, ys)
    assert np.array_equal(replay_sampler(U, xs, ys).view(np.uint32), np.ascontiguousarray(o32).view(np.uint32))
    nbad, worst, neq, _ = check_sampler(o32, U, xs, ys)
    assert nbad == 0 and neq == 0, (nbad, worst, neq)
    for mut in SAMPLER_MUTANTS:
        nb = check_sampler(replay_sampler(U, xs, ys, mut), U, xs, ys)[0]
        floor = 0.02
        if mut == "swap_taps":
            floor = 0.0 if frames == "ones" else 0.01
        assert nb >= floor * o32.size and (nb > 0 or floor == 0.0), (mut, nb, o32.size)


def test_uint8_truncation_check_flags_rounding():
    from oracle import frames as ofr
    v = np.random.default_rng(0).uniform(0.0, 1.0, 4096).astype(F32)
    want = ofr.to_uint8(v)
    rounded = np.uint8(np.rint(v.astype(np.float64) * 255.0))
    assert (rounded != want).mean() > 0.4


# ---------------------------------------------------------------------------------------------------------------------
# GPU

LOG = []


def note(line):
    LOG.append(line)
    print("TPSF64 " + line)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def gpu_solve(coord, rhs, is_vec):
    import torch
    from coupe.dvsg_amd import _lib
    B, P, _ = coord.shape
    c, r = _dev(coord), _dev(rhs)
    T = Guarded(B * 2 * (P + 3) * 4, c.device)
    _lib.call("dvsg_tps_solve_f32", c.data_ptr(), r.data_ptr(), int(is_vec), B, P, T.ptr(), _stream())
    torch.cuda.synchronize()
    assert T.intact(), "wrote past T"
    return T.view(torch.float32, (B, 2, P + 3)).cpu().numpy()


def gpu_warp(U, coord, T, oh, ow, want_xy=True):
    """dvsg_tps_warp_f32 with every output between sentinels -> (out [B,oh,ow,C] or None, x_s, y_s [B,oh*ow] or None)"""
    import torch
    from coupe.dvsg_amd import _lib
    B, P = T.shape[0], T.shape[2] - 3
    c, t = _dev(coord), _dev(T)
    H, W, C = (U.shape[1:] if U is not None else (1, 1, 1))
    u = _dev(U) if U is not None else None
    n = B * oh * ow
    out = Guarded(n * C * 4, c.device) if U is not None else None
    gx = Guarded(n * 4, c.device) if want_xy else None
    gy = Guarded(n * 4, c.device) if want_xy else None
    _lib.call("dvsg_tps_warp_f32", u.data_ptr() if u is not None else None, c.data_ptr(), t.data_ptr(), B, H, W, C, P, oh, ow,
              out.ptr() if out else None, gx.ptr() if gx else None, gy.ptr() if gy else None, _stream())
    torch.cuda.synchronize()
    for g in (out, gx, gy):
        assert g is None or g.intact(), "wrote past an output"
    f = torch.float32
    return (out.view(f, (B, oh, ow, C)).cpu().numpy() if out else None,
            gx.view(f, (B, oh * ow)).cpu().numpy() if gx else None, gy.view(f, (B, oh * ow)).cpu().numpy() if gy else None)


_NET = {}


def _net(weights):
    from coupe.dvsg_amd.networks import LocNet
    if "net" not in _NET:
        _NET["net"] = LocNet(weights)
    return _NET["net"]


def gpu_render(net, F, src, flip, f32=True, u8_W=0, u8_x0=0):
    """dvsg_tps_render_u8 -> (T [n,2,28], out_f32 or None, out_u8 [n,H,u8_W,3] filled with the canary 0x5A first, or None)"""
    import torch
    from coupe.dvsg_amd import _lib
    n, H, W = src.shape[:3]
    Fd, s = _dev(F), _dev(src)
    T = Guarded(n * 56 * 4, s.device)
    o32 = Guarded(n * H * W * 12, s.device) if f32 else None
    o8 = Guarded(n * H * u8_W * 3, s.device) if u8_W else None
    if o8:
        o8.body.fill_(0x5A)
    _lib.call("dvsg_tps_render_u8", net.handle, Fd.data_ptr(), s.data_ptr(), n, H, W, int(flip), T.ptr(),
              o32.ptr() if o32 else None, o8.ptr() if o8 else None, u8_W, u8_x0, _stream())
    torch.cuda.synchronize()
    for g in (T, o32, o8):
        assert g is None or g.intact(), "wrote past an output"
    return (T.view(torch.float32, (n, 2, 28)).cpu().numpy(), o32.view(torch.float32, (n, H, W, 3)).cpu().numpy() if o32 else None,
            o8.view(torch.uint8, (n, H, u8_W, 3)).cpu().numpy() if o8 else None)


def T_of(net, F):
    """the T that dvsg_stabilize_* forms from F_t [n,25,2]: dvsg_tps_render_u8 returns it (tps_apply_kernel)"""
    n = F.shape[0]
    return gpu_render(net, F, np.zeros((n, 2, 2, 3), dtype=np.uint8), 0)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("P", SOLVE_P)
def test_solver_against_float64(P):
    """tps_solve_kernel, B = 6, regular and per-sample jittered control points, vector and target mode, three right-hand
    sides: every entry of T inside bound 1"""
    worst_all = 0.0
    for jitter in (False, True):
        for is_vec in (1, 0):
            for scale, shift in SOLVE_RHS:
                coord, rhs_in, rhs = _solve_inputs(P, jitter, scale, shift, is_vec)
                T64, E, rho = solve_reference(coord, rhs)
                T = gpu_solve(coord, rhs_in, is_vec)
                nbad, worst = check_T(T, T64, E)
                worst_all = max(worst_all, worst)
                assert nbad == 0, (P, jitter, is_vec, scale, shift, nbad, worst)
    note("solver P=%d: worst |T - T64| / bound %.3f" % (P, worst_all))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 64])
def test_cached_inverse_against_float64(synthetic_weights, B):
    """tps_apply_kernel on the handle's cached W^-1 columns (through dvsg_tps_render_u8, arbitrary F_t): T inside bound 1 of
    the float64 solve on V_src, and its grid agrees with the grid of dvsg_tps_solve_f32's T on the same inputs within the
    two T bounds carried through the basis plus the two grid bounds"""
    import inputs as tin
    net = _net(synthetic_weights)
    coord = tin.v_src(B)
    for scale, shift in SOLVE_RHS:
        F = vectors(B, 25, scale, shift, seed=B + int(scale * 100))
        T64, E, rho = solve_reference(coord, (coord + F).astype(F32))
        T = T_of(net, F)
        nbad, worst = check_T(T, T64, E)
        assert nbad == 0, ("apply", scale, shift, nbad, worst)
        Ts = gpu_solve(coord, F, 1)
        nbad, worst_s = check_T(Ts, T64, E)
        assert nbad == 0, ("solve", scale, shift, nbad, worst_s)
        oh, ow = 9, 14
        _, xa, ya = gpu_warp(None, coord, T, oh, ow)
        _, xb, yb = gpu_warp(None, coord, Ts, oh, ow)
        ra, Ea = grid_reference(T, coord, oh, ow)
        rb, Eb = grid_reference(Ts, coord, oh, ow)
        assert check_grid(xa, ya, ra, Ea)[0] == 0 and check_grid(xb, yb, rb, Eb)[0] == 0
        # |map(T_a) - map(T_b)| <= sum_k |T_a - T_b|_k |basis_k| <= sum_k 2 E_k |basis_k|
        basis = grid_terms(2.0 * E, coord, oh, ow)[2]
        d = np.abs(np.stack([xa, ya], 1).reshape(ra.shape).astype(np.float64) - np.stack([xb, yb], 1).reshape(ra.shape))
        assert (d <= Ea + Eb + basis).all()
        note("cached inverse B=%d scale %.2f shift %.1f: apply %.3f, solver %.3f of bound 1" % (B, scale, shift, worst, worst_s))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID_CASES, ids=["%dx%d-P%d-B%d" % c[:4] for c in GRID_CASES])
def test_grid_against_float64(case):
    """x_s, y_s alone (U = NULL) at every shape: every value inside bound 2, no mask"""
    oh, ow, P, B, _, _, mult = case
    coord, T = _grid_inputs(case)
    _, xs, ys = gpu_warp(None, coord, T, oh, ow)
    ref, E = grid_reference(T, coord, oh, ow)
    nbad, worst, at = check_grid(xs, ys, ref, E)
    note("grid %dx%d P=%d B=%d |T|max %.3g: worst / bound %.3f at (b, k, row, column) %s, bound %.2e px"
         % (oh, ow, P, B, float(np.abs(T).max()), worst, at, float(E[:, 0].max()) * ow / 2))
    assert nbad == 0, (nbad, worst, at)


@pytest.mark.gpu
def test_grid_3840x2160_on_a_band_of_rows():
    oh, ow, P, B, _, _, _ = GRID_4K
    coord, T = _grid_inputs(GRID_4K)
    _, xs, ys = gpu_warp(None, coord, T, oh, ow)
    rows = np.array(GRID_4K_ROWS)
    ref, E = grid_reference(T, coord, oh, ow, rows)
    pick = lambda a: a.reshape(B, oh, ow)[:, rows]
    nbad, worst, at = check_grid(pick(xs), pick(ys), ref, E)
    note("grid 2160x3840 rows %s: worst / bound %.3f, bound %.2e px" % ([int(r) for r in rows], worst, float(E[:, 0].max()) * ow / 2))
    assert nbad == 0, (nbad, worst, at)


@pytest.mark.gpu
@pytest.mark.parametrize("oh,ow", [(1, 1), (1, 7), (5, 1), (37, 53), (72, 128), (6, 300)])
def test_affine_only_T_gives_tf_linspace_bit_for_bit(oh, ow):
    from oracle.tfops import tf_linspace
    P, B = 25, 2
    coord = control_points(P, B, True, seed=3)
    T = np.zeros((B, 2, P + 3), dtype=F32)
    T[:, 0, 1] = T[:, 1, 2] = 1.0
    _, xs, ys = gpu_warp(None, coord, T, oh, ow)
    xl, yl = tf_linspace(-1.0, 1.0, ow), tf_linspace(-1.0, 1.0, oh)
    assert np.array_equal(xs.reshape(B, oh, ow), np.broadcast_to(xl[None, None, :], (B, oh, ow)))
    assert np.array_equal(ys.reshape(B, oh, ow), np.broadcast_to(yl[None, :, None], (B, oh, ow)))


def judge_pixels(tag, out, U, xs, ys, assert_regions):
    H, W = U.shape[1:3]
    counts, n = region_counts(xs, ys, H, W)
    nbad, worst, neq, where = check_sampler(out, U, xs, ys)
    note("%s: sampler worst / bound %.3f, %d of %d values not bit-equal to the float32 oracle; %s"
         % (tag, worst, neq, np.asarray(out).size, region_text(counts, n)))
    if assert_regions:
        assert regions_ok(counts, n), region_text(counts, n)
    assert nbad == 0, "%d values out of the float64 bound, first pixels (b, n) %s" % (nbad, where[:4].tolist())
    assert neq == 0, "%d values differ from oracle.interpolate_a, first pixels (b, n) %s" % (neq, where[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("case", WARP_CASES, ids=["%dx%d-%dx%d-C%d-P%d-%s" % c for c in WARP_CASES])
def test_warp_sampler_at_the_gpu_s_own_coordinates(case):
    """dvsg_tps_warp_f32, C = 3 / 1 / generic: the grid inside bound 2, every pixel inside bound 3 at the x_s, y_s the call
    wrote, bit-equal to the float32 oracle; the image-less call writes the same x_s, y_s"""
    H, W, oh, ow, C, P, frames = case
    U, coord, T, xo, yo = _sampler_inputs(case)
    counts, n = region_counts(xo, yo, H, W)
    assert regions_ok(counts, n), region_text(counts, n)                   # chosen on the CPU, before the GPU is asked
    out, xs, ys = gpu_warp(U, coord, T, oh, ow)
    ref, E = grid_reference(T, coord, oh, ow)
    nbad, worst, at = check_grid(xs, ys, ref, E)
    assert nbad == 0, ("grid", nbad, worst, at)
    _, x2, y2 = gpu_warp(None, coord, T, oh, ow)
    assert np.array_equal(xs, x2) and np.array_equal(ys, y2), "x_s, y_s differ between the image and the grid-only call"
    out2, _, _ = gpu_warp(U, coord, T, oh, ow, want_xy=False)
    assert np.array_equal(out, out2), "the output depends on whether x_s, y_s are requested"
    judge_pixels("warp %dx%d->%dx%d C=%d P=%d %s (grid %.3f)" % (H, W, oh, ow, C, P, frames, worst), out, U, xs, ys, True)


@pytest.mark.gpu
def test_warp_rejects_65_channels():
    from coupe.dvsg_amd._lib import DvsgError
    U = np.zeros((1, 4, 4, 65), dtype=F32)
    with pytest.raises(DvsgError):
        gpu_warp(U, control_points(4, 1, False), np.zeros((1, 2, 7), dtype=F32), 4, 4)


RING_SHAPE = (3, 64, 96)


def _ring_inputs(u8):
    B, H, W = RING_SHAPE
    n = B + 9
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if not u8:
        pool = (pool.astype(np.float64) / 255.0).astype(F32)
    table = ((np.arange(7)[None, :] + np.arange(B)[:, None] * 2) % (n - 2)).astype(np.int32)   # frames n - 2, n - 1 stay free
    table[1, 6] = n                                                       # u_t of window 1 is outside the pool: zeros
    table[2, 3] = -1
    return pool, np.ascontiguousarray(table), n


def _chain(tag, net, F, xs, ys, U, out, B, H, W):
    """F_t -> T (bound 1) -> x_s, y_s (bound 2) -> pixels (bound 3), each link against its own reference"""
    import inputs as tin
    coord = tin.v_src(1)
    T = T_of(net, F)
    T64, E, rho = solve_reference(tin.v_src(B), (tin.v_src(B) + F).astype(F32))
    nbad, wT = check_T(T, T64, E)
    assert nbad == 0, (tag, "T", nbad, wT)
    ref, Eg = grid_reference(T, coord, H, W)
    nbad, wg, at = check_grid(xs, ys, ref, Eg)
    assert nbad == 0, (tag, "grid", nbad, wg, at)
    judge_pixels("%s (T %.3f, grid %.3f, max |F_t| %.3g)" % (tag, wT, wg, float(np.abs(F).max())), out, U,
                 xs.reshape(B, -1), ys.reshape(B, -1), False)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["ring_f32", "ring_u8", "inplace"])
def test_ring_forms_against_their_own_reference(synthetic_weights, form):
    """the frame is pool[table[b, 6]] (uint8: float32(v / 255.)), zeros for an index outside the pool with x_s still
    written; in place: the named slot holds the values, every other pool byte keeps its value, an outside slot stores nothing"""
    import torch
    net = _net(synthetic_weights)
    B, H, W = RING_SHAPE
    pool, table, n = _ring_inputs(form == "ring_u8")
    pf = (pool.astype(np.float64) / 255.0).astype(F32) if pool.dtype == np.uint8 else pool
    U = np.stack([pf[table[b, 6]] if 0 <= table[b, 6] < n else np.zeros_like(pf[0]) for b in range(B)])
    dpool, dtab = _dev(pool), _dev(table)
    F = torch.full((B, 25, 2), float("nan"), device="cuda")
    xs = torch.full((B * H * W,), float("nan"), device="cuda")
    ys = torch.full((B * H * W,), float("nan"), device="cuda")
    if form == "inplace":
        slots = np.array([n - 1, -1, n - 2], dtype=np.int32)              # not named by the table; window 1 stores nothing
        assert not set(slots.tolist()) & set(table.reshape(-1).tolist()) - {-1}
        before = dpool.clone()
        net.stabilize_ring_inplace(dpool, dtab, _dev(slots), F, xs, ys)
        torch.cuda.synchronize()
        after = dpool.cpu().numpy()
        keep = [i for i in range(n) if i not in (n - 1, n - 2)]
        assert np.array_equal(after[keep].view(np.uint32), before.cpu().numpy()[keep].view(np.uint32)), "another pool frame changed"
        out = np.stack([after[n - 1], np.zeros_like(after[0]), after[n - 2]])
        Fh, xh, yh = F.cpu().numpy(), xs.cpu().numpy(), ys.cpu().numpy()
        assert np.isfinite(xh).all() and np.isfinite(yh).all(), "x_s / y_s of the window without a slot were not written"
        sel = [0, 2]
        _chain(form, net, Fh[sel], xh.reshape(B, -1)[sel], yh.reshape(B, -1)[sel], U[sel], out[sel], 2, H, W)
        T1 = T_of(net, Fh[1:2])
        ref, Eg = grid_reference(T1, __import__("inputs").v_src(1), H, W)
        assert check_grid(xh.reshape(B, -1)[1], yh.reshape(B, -1)[1], ref, Eg)[0] == 0
        return
    out = Guarded(B * H * W * 12, dpool.device)
    net.stabilize_ring(dpool, dtab, out.view(torch.float32, (B, H, W, 3)), F, xs, ys)
    torch.cuda.synchronize()
    assert out.intact()
    oh = out.view(torch.float32, (B, H, W, 3)).cpu().numpy()
    assert not oh[1].any(), "u_t outside the pool must warp a frame of zeros"
    _chain(form, net, F.cpu().numpy(), xs.cpu().numpy().reshape(B, -1), ys.cpu().numpy().reshape(B, -1), U, oh, B, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("H,W", [(37, 53), (62, 300)])
def test_render_u8_against_its_own_reference(synthetic_weights, flip, H, W):
    """tps_warp_kernel<3, uint8_t, uint8_t>: coordinates from the grid-only call with the returned T; out_f32 inside bound 3
    on float32(v / 255.) with the channels flipped; out_u8 == trunc(float64(value) x 255) in src's channel order; bytes
    outside [u8_x0, u8_x0 + W) keep the canary; each output alone gives the same bytes"""
    import inputs as tin
    from oracle import frames as ofr
    from oracle import thin_plate_spline as otps
    net = _net(synthetic_weights)
    B = 4
    rng = np.random.default_rng(H + flip)
    src = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    src[:, : H // 2, : W // 3] = 255
    F = vectors(B, 25, 0.05, 0.0, seed=W)
    F[1] = vectors(1, 25, 0.5, 0.0, seed=1)[0]
    F[2] = vectors(1, 25, 0.05, 1.5, seed=2)[0]
    F[3] += np.array([-2.0 / W, -2.0 / H], dtype=F32)                      # one pixel left / up: the [-1, 0) cells
    u8_W, u8_x0 = W + 9, 5
    T64, E, _ = solve_reference(tin.v_src(B), (tin.v_src(B) + F).astype(F32))
    counts, n = region_counts(*otps.source_coords(T64.astype(F32), tin.v_src(B), H, W), H, W)
    assert all(c >= 50 or c >= 0.01 * n for c in (counts[0], counts[2], counts[5])), region_text(counts, n)   # before the GPU
    T, o32, o8 = gpu_render(net, F, src, flip, True, u8_W, u8_x0)
    nbad, wT = check_T(T, T64, E)
    assert nbad == 0, ("T", nbad, wT)
    _, xs, ys = gpu_warp(None, tin.v_src(B), T, H, W)
    rgb = src[..., ::-1] if flip else src
    U = (rgb.astype(np.float64) / 255.0).astype(F32)
    judge_pixels("render_u8 %dx%d flip %d (T %.3f)" % (H, W, flip, wT), o32, U, xs, ys, False)
    counts, n = region_counts(xs, ys, H, W)
    assert all(c >= 50 or c >= 0.01 * n for c in (counts[0], counts[2], counts[5])), region_text(counts, n)
    want8 = ofr.to_uint8(np.clip((o32[..., ::-1] if flip else o32).astype(np.float64), 0.0, None))
    assert np.array_equal(o8[:, :, u8_x0:u8_x0 + W], want8), "uint8 output is not the truncated float64 product"
    assert (o8[:, :, :u8_x0] == 0x5A).all() and (o8[:, :, u8_x0 + W:] == 0x5A).all(), "bytes outside the columns changed"
    _, a32, none8 = gpu_render(net, F, src, flip, True)
    _, none32, a8 = gpu_render(net, F, src, flip, False, u8_W, u8_x0)
    assert none8 is None and none32 is None
    assert np.array_equal(a32.view(np.uint32), o32.view(np.uint32)) and np.array_equal(a8, o8)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_whole_graph_as_a_chain_of_bounded_links(synthetic_weights, masked):
    """dvsg_stabilize_f32 / dvsg_stabilize_masked_f32: from the call's own F_t, T by link 1, x_s by link 2 with that T, the
    pixels by link 3 with those x_s -- broadcast control points (coord_bstride = 0), no pixel masked"""
    import torch
    import inputs as tin
    from coupe.dvsg_amd.networks import random_mask_plane
    net = _net(synthetic_weights)
    B, H, W = 2, 72, 128
    x = tin.window_frames(5, B, H, W)
    u = np.ascontiguousarray(x[..., 18:])
    out = Guarded(B * H * W * 12, torch.device("cuda:0"))
    F = torch.full((B, 25, 2), float("nan"), device="cuda")
    xs = torch.full((B * H * W,), float("nan"), device="cuda")
    ys = torch.full((B * H * W,), float("nan"), device="cuda")
    mask = random_mask_plane(tin.mask_homographies(3, B), H, W) if masked else None
    net.stabilize(_dev(x), _dev(u), out.view(torch.float32, (B, H, W, 3)), F, xs, ys, mask=mask)
    torch.cuda.synchronize()
    assert out.intact()
    _chain("stabilize%s_f32 %dx%d" % ("_masked" if masked else "", H, W), net, F.cpu().numpy(), xs.cpu().numpy().reshape(B, -1),
           ys.cpu().numpy().reshape(B, -1), u, out.view(torch.float32, (B, H, W, 3)).cpu().numpy(), B, H, W)
