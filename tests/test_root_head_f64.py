"""conv1, the root max pool and the head pinned to float64, element by element.

Every conv1 instantiation of conv1_f32.hip, conv1_f16.hip and conv1_x3.hip that a public path can launch is launched on purpose by a case of CASES, which
names the launch record it expects (dvsg_debug_last_root_kernel: family, NW, TO, SRC, bands, quads per band, max pool,
average pool, dense chunks); the record must match exactly, and a CPU test checks the table against the mangled names of
the built library.  tau, bound, excess, Guarded and TINY are test_conv_gemm_f64.py's, the float16 interval check is
test_conv_f16_f64.py's.

Operands as the library holds them, reproduced in NumPy float32 with one rounding per operation:

    scale = gamma / sqrt(var + 1e-5f),  w = w_tf[kh, kw, cs, n] * scale[n],  cs = (2 - c / 7) * 7 + c % 7  (make_conv1)
    a = fl(fl(x * 255) - mean_g),  masked: fl(fl(fl(x * m) * 255) - mean_g) on channels 0..17,  uint8: x = fl(v / 255.),
    a table index outside [0, n_pool): x = 0;  on the pad ring a = 0 (not -mean).

shift = beta - mean * scale is host code that the compiler may contract into one FMA, so the bias carries one extra
2^-24 |mean * scale| in every bound (the NumPy value rounds the product first).

Bounds, per output element, K = 7 x 147 = 1029, S = conv(|a|, |w|) + |b| in float64, ref = relu(conv(a, w) + b):

    f32    |y - ref| <= tau(K) S + K 2^-126 + 2^-24 |mean scale|                                     (f64.bound "f32")
    f32x3  the same + 2^-23 S: conv1_x3_kernel follows conv_gemm_tile.h X3 -- three bfloat16 pieces hold all 24 bits of a
           and w (the reference uses w = p1 + p2 + p3 as make_conv1 packs it), six of nine cross terms are formed, the
           dropped a2 w3 + a3 w2 + a3 w3 are <= (2^-8 2^-16 + 2^-16 2^-8 + 2^-32) |a w| <= 2^-23 |a w|    (f64.bound "f32x3")
    f32s   conv1_split_kernel holds a = ahi + alo (ahi = f16(a), alo = f16(a - ahi)) and w = whi + 2^-11 wlo
           (wlo = f16((w - whi) 2^11), accumulated apart and folded in with 2^-11); the reference convolves exactly those
           sums, S = conv(|ahi| + |alo|, |whi| + 2^-11 |wlo|) + |b|.  The one dropped cross product is alo x 2^-11 wlo,
           bounded by D = conv(|alo|, 2^-11 |wlo|), computed from the pieces themselves.  The output is stored in the P format
           (hi + lo, lo rounded): 2^-22 |y| + 2^-25 as in f64.bound "f32s".  Bound: tau(K) S + K 2^-126 + D + 2^-22 S + 2^-25.
    f16    pair, marching and one-row kernels: a and w rounded to float16 in the reference (a reaches 151, a float16 ulp of
           0.125), E = tau(K) S16 + K 2^-126 + 2^-24 |mean scale|, and y must lie in [RN16(relu(pre - E)), RN16(relu(pre + E))].
           conv1_variant 2 (conv1_kernel<4, _Float16, 0>) multiplies the float32 operands and rounds the output: the same
           interval around the float32-operand reference.
ReLU is part of the reference; relu is 1-Lipschitz, so an element whose pre-activation is within the bound of 0 may be 0
or positive.  conv1's output is >= 0, so a max pool that padded with 0 instead of -inf cannot be told apart through the
network; the pool test checks the window geometry bit for bit and does not claim to cover the pad value.

Measured on one MI355X (worst |y - ref| / (tau(K) S) per family, tau(K) = 36.1 x 2^-24):
    family                                          mixed-sign frames   positive set (S = the value)
    conv1_kernel<4, float, SRC>, <8, float, 0>      0.15                0.54
    conv1_x3_kernel                                 0.05                0.40
    conv1_split_kernel                              0.07                0.52
    float16 outputs (pair, marching, one-row, <4, _Float16, 0>): every element inside its rounding interval; |y - ref|
    there is the output rounding (up to 226 x tau(K) S on the positive set, half a float16 ulp), not the accumulation.
    pool5 <= 0.46 of its bound, F_t <= 0.001 of its composed bound; pool1 bit for bit.  The file runs in 39 s.
The positive set is above half the bound in conv1_kernel and conv1_split_kernel.  Both are explained by the summation
order: all products have one sign, so every rounding acts on a partial sum that grows linearly to the value, and a chain of
n dependent float32 accumulations ends sigma = sqrt(n / 36) ulp from it.  conv1_kernel first measured 1.047 here (3 of
165 120 elements of the 10 x 516 case out of bounds, interior elements, the same bits from SRC 5 and NW 8): 518 dependent
v_mfma_f32_32x32x2_f32 steps through ONE accumulator, sigma = 3.8 ulp, the largest of 1.6e5 elements at ~4.5 sigma.  That
was a finding of this file; the kernel now keeps the even and the odd taps in two accumulators (two chains of 259 steps at
half the magnitude, added once in the epilogue), which halves it to 0.54.  conv1_split_kernel's hi x hi and lo x hi products
share one accumulator (140 MFMA steps of 16 products), and its output is rounded to the 22-bit P format.
"""
import ctypes
import math
import re

import numpy as np
import pytest

import test_conv_gemm_f64 as f64
import test_conv_f16_f64 as f16t

tau, bound, excess, Guarded, TINY = f64.tau, f64.bound, f64.excess, f64.Guarded, f64.TINY
check16, rn16 = f16t.check16, f16t.rn16

F32 = np.float32
K1 = 7 * 147
MEAN_G = (123.68, 116.779, 103.939)     # raw channel group g = c / 7 (oldest frames first) gets the mean of scaled group 2 - g
PREFIX = "stabNet/localizationNet/"
ROOT_FIELDS = ("conv1", "NW", "TO", "SRC", "bands", "quads", "maxpool", "avgpool", "dense_chunks")
PREC_CODE = {"f32": 0, "f16": 1, "f32s": 2, "f32x3": 3}
FAMILY = ("conv1_kernel", "conv1_f16_kernel", "conv1_f16_pair_kernel", "conv1_f16_march_kernel", "conv1_split_kernel",
          "conv1_x3_kernel")
POOL_OF = {"f32": 0, "f16": 2, "f32s": 3, "f32x3": 0}      # launch_maxpool
AVG_OF = {"f32": 0, "f16": 1, "f32s": 2, "f32x3": 0}       # launch_avgpool_partial
# maxpool_kernel<_Float16> cannot be launched through a public path: launch_maxpool takes it only for prec == kF16 &&
# C % 8 != 0 ("else if (prec == kF16 && C % 8 == 0) ... maxpool_h8_kernel"), and forward() always passes C = 64.
UNREACHABLE = {("maxpool_kernel", 1)}


# ---------------------------------------------------------------------------------------------------------------------
# operands, NumPy float32

def fold_conv1(weights):
    """make_conv1 / bn_fold: w [64, 21, 7, 7] (n, raw channel c, kh, kw) float32, bias [64] float32, bias slack [64] float64"""
    def get(k):
        return np.asarray(weights[PREFIX + "resnet_v1_50/conv1/" + k + ":0"], dtype=F32)
    w = get("weights")                                       # [7, 7, 21, 64] HWIO, scaled-tensor channels
    gamma, beta, mu, var = (get("BatchNorm/" + k) for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    scale = (gamma / np.sqrt((var + F32(1e-5)).astype(F32)).astype(F32)).astype(F32)
    shift = (beta - (mu * scale).astype(F32)).astype(F32)
    cs = np.array([(2 - c // 7) * 7 + c % 7 for c in range(21)])
    wf = (w[:, :, cs, :] * scale[None, None, None, :]).astype(F32)
    slack = 2.0 ** -24 * np.abs(mu.astype(np.float64) * scale.astype(np.float64))
    return np.ascontiguousarray(wf.transpose(3, 2, 0, 1)), shift, slack


def unreversed_conv1(weights):
    """the defect "group reversal not applied": raw channel c multiplies the weight of scaled channel c"""
    w, b, s = fold_conv1(weights)
    cs = np.array([(2 - c // 7) * 7 + c % 7 for c in range(21)])
    out = np.empty_like(w)
    out[:, cs] = w                                           # out[:, cs[c]] = w[:, c]  <=>  out[:, c] = w_tf[c] * scale
    return out, b, s


def bf16_rn(v):
    """float32 -> bfloat16 value (round to nearest even on the upper 16 bits), as float32"""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def held_weights(w, prec):
    """(w64 the value the kernels multiply, |w| for S, 2^-11 |wlo| for the f32s dropped term or None) as float64"""
    if prec == "f16":
        h = w.astype(np.float16).astype(np.float64)
        return h, np.abs(h), None
    if prec == "f32s":
        hi = w.astype(np.float16)
        lo = ((w - hi.astype(F32)).astype(F32) * F32(2048.0)).astype(F32).astype(np.float16)
        los = lo.astype(np.float64) / 2048.0
        return hi.astype(np.float64) + los, np.abs(hi.astype(np.float64)) + np.abs(los), np.abs(los)
    if prec == "f32x3":
        p1 = bf16_rn(w)
        r1 = (w - p1).astype(F32)
        p2 = bf16_rn(r1)
        p3 = bf16_rn((r1 - p2).astype(F32))
        h = p1.astype(np.float64) + p2.astype(np.float64) + p3.astype(np.float64)
        return h, np.abs(h), None
    return w.astype(np.float64), np.abs(w.astype(np.float64)), None


def gather_window(pool, table):
    """dvsg_window_gather_f32: pool [n, H, W, 3] float32, table [B, 7] -> window [B, H, W, 21]; outside [0, n): zeros"""
    n = pool.shape[0]
    B = table.shape[0]
    out = np.zeros((B,) + pool.shape[1:3] + (21,), dtype=F32)
    for b in range(B):
        for s in range(7):
            i = int(table[b, s])
            if 0 <= i < n:
                out[b, :, :, 3 * s:3 * s + 3] = pool[i]
    return out


def u8_to_f32(v):
    return (v.astype(np.float64) / 255.0).astype(F32)


def scaled(x, mask=None, mask_all=False):
    """the staged activation a [B, H, W, 21] float32 (inside the image) of window x, mask plane [B, H, W] or None"""
    x = np.asarray(x, dtype=F32)
    if mask is not None:
        x = x.copy()
        nm = 21 if mask_all else 18
        x[..., :nm] = (x[..., :nm] * mask[..., None].astype(F32)).astype(F32)
    mean = np.array([MEAN_G[c // 7] for c in range(21)], dtype=F32)
    return ((x * F32(255.0)).astype(F32) - mean).astype(F32)


def held_activation(a, prec):
    """(a64 as the kernel multiplies it, |a| pieces for S, |alo| or None), float32 arrays holding exact values where possible"""
    if prec == "f16":
        h = a.astype(np.float16).astype(F32)
        return h, None
    if prec == "f32s":
        hi = a.astype(np.float16).astype(F32)
        lo = (a - hi).astype(F32).astype(np.float16).astype(F32)
        return hi, lo
    return a, None


def pad3(a, ring=None):
    """[B, H, W, 21] -> torch [B, 21, H + 6, W + 6] float32; the ring is 0 (or, for the defect, `ring` per channel)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)
    p = torch.nn.functional.pad(t, (3, 3, 3, 3))
    if ring is not None:
        r = torch.from_numpy(np.asarray(ring, dtype=F32)).view(1, 21, 1, 1).expand_as(p).clone()
        r[:, :, 3:-3, 3:-3] = t
        p = r
    return p.contiguous()


def conv_region(ap, w, r0, r1, c0, c1):
    """float64 conv of padded ap [B, 21, H + 6, W + 6] with w [64, 21, 7, 7] for output rows [r0, r1), columns [c0, c1)
    -> [B, r1 - r0, c1 - c0, 64]"""
    import torch
    sl = ap[:, :, 2 * r0:2 * (r1 - 1) + 7, 2 * c0:2 * (c1 - 1) + 7].double()
    return torch.nn.functional.conv2d(sl, w, stride=2).permute(0, 2, 3, 1)


def conv_points(ap, w, b, ho, wo):
    """the same at scattered output pixels (b[i], ho[i], wo[i]) -> [N, 64]"""
    import torch
    ar = torch.arange(7)
    rows = (2 * ho)[:, None] + ar
    cols = (2 * wo)[:, None] + ar
    patch = ap[b[:, None, None, None], torch.arange(21)[None, :, None, None], rows[:, None, :, None], cols[:, None, None, :]]
    return patch.double().reshape(len(b), -1) @ w.reshape(64, -1).t()


class Operands(object):
    """conv1's operands in one precision, ready for float64 regions: pre (before ReLU), S and the tolerance pieces"""

    def __init__(self, folded, prec, a, ring=None):
        import torch
        w, bias, slack = folded
        self.prec = prec
        w64, wabs, wlo = held_weights(w, prec)
        self.w, self.wabs = torch.from_numpy(w64), torch.from_numpy(wabs)
        self.wlo = torch.from_numpy(wlo) if wlo is not None else None
        self.bias = torch.from_numpy(bias.astype(np.float64))
        self.slack = torch.from_numpy(slack)
        hi, lo = held_activation(a, prec)
        self.ap = pad3(hi, ring)
        self.alo = pad3(lo) if lo is not None else None
        self.B, self.H, self.W = a.shape[:3]
        self.Ho, self.Wo = (self.H - 1) // 2 + 1, (self.W - 1) // 2 + 1

    def _tol(self, S, D):
        t = tau(K1) * S + K1 * TINY + self.slack
        if self.prec == "f32x3":
            t = t + 2.0 ** -23 * S
        elif self.prec == "f32s":
            t = t + D + 2.0 ** -22 * S + 2.0 ** -25
        return t

    def region(self, r0, r1, c0, c1):
        """(pre, S, tol) for a rectangle of output pixels"""
        pre = conv_region(self.ap, self.w, r0, r1, c0, c1)
        S = conv_region(self.ap.abs(), self.wabs, r0, r1, c0, c1)
        D = None
        if self.alo is not None:
            pre = pre + conv_region(self.alo, self.w, r0, r1, c0, c1)
            S = S + conv_region(self.alo.abs(), self.wabs, r0, r1, c0, c1)
            D = conv_region(self.alo.abs(), self.wlo, r0, r1, c0, c1)
        pre, S = pre + self.bias, S + self.bias.abs()
        return pre, S, self._tol(S, D)

    def points(self, b, ho, wo):
        pre = conv_points(self.ap, self.w, b, ho, wo)
        S = conv_points(self.ap.abs(), self.wabs, b, ho, wo)
        D = None
        if self.alo is not None:
            pre = pre + conv_points(self.alo, self.w, b, ho, wo)
            S = S + conv_points(self.alo.abs(), self.wabs, b, ho, wo)
            D = conv_points(self.alo.abs(), self.wlo, b, ho, wo)
        pre, S = pre + self.bias, S + self.bias.abs()
        return pre, S, self._tol(S, D)

    def full(self):
        return self.region(0, self.Ho, 0, self.Wo)


def judge(prec_out, y, pre, S, tol):
    """(number of elements out of bounds, worst |y - ref| / (tau(K) S)); prec_out "f16": the interval criterion"""
    import torch
    ref = pre.clamp_min(0.0)
    unit = float(((y.double() - ref).abs() / (tau(K1) * S)).max()) if not bool(torch.isnan(y).any()) else float("inf")
    if prec_out == "f16":
        E = (tol).numpy()
        nbad, _, _ = check16(y.double().numpy(), pre.numpy(), E, True)
        return nbad, unit
    nbad, _ = excess(y, ref, tol)
    return nbad, unit


# ---------------------------------------------------------------------------------------------------------------------
# inputs (NumPy, seeded; the same on the CPU and the GPU legs)

def make_pool(kind, n, H, W, seed):
    """a frame pool [n, H, W, 3]: "u8" uint8 frames with 0 and 255 in them (mixed sign after scaling), "wide" float32
    slightly outside [0, 1] (a written-back s_t_pred), "pos" values whose scaled activation is positive (uint8 >= 160)"""
    rng = np.random.default_rng(seed)
    if kind == "wide":
        return rng.uniform(-0.05, 1.05, (n, H, W, 3)).astype(F32)
    lo = 160 if kind == "pos" else 0
    v = rng.integers(lo, 256, (n, H, W, 3), dtype=np.uint8)
    v[:, :(H + 1) // 2, :(W + 2) // 3, 0] = 255
    if kind != "pos":
        v[:, H // 2:, W // 2:, 1] = 0
    return v


def make_table(B, n, oob):
    t = (np.arange(7, dtype=np.int32)[None, :] + np.arange(B, dtype=np.int32)[:, None]) % n
    t = t[:, ::-1].copy() if B > 1 else t          # not the identity order
    if oob:
        t[0, 2] = -1
        t[B - 1, 5] = n
    return np.ascontiguousarray(t, dtype=np.int32)


def make_mask(B, H, W, seed):
    """CPU stand-in of a random_mask_plane: a fractional ramp with exact 0 and exact 1 regions"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.0, 1.0, (B, H, W)).astype(F32)
    m[:, :, :W // 3] = 1.0
    m[:, H // 2:, W - W // 4:] = 0.0
    return m


def positive_weights(weights):
    """conv1 with positive weights and a positive bias: with "pos" frames S equals the value and the bound is sharp"""
    w = dict(weights)
    s = PREFIX + "resnet_v1_50/conv1/"
    w[s + "weights:0"] = np.abs(weights[s + "weights:0"])
    w[s + "BatchNorm/beta:0"] = np.abs(weights[s + "BatchNorm/beta:0"])
    w[s + "BatchNorm/moving_mean:0"] = -np.abs(weights[s + "BatchNorm/moving_mean:0"])
    return w


# ---------------------------------------------------------------------------------------------------------------------
# the case table.  A conv1 case is (prec, variant, kind, masked, off_grid, (B, H, W), inputs, expected record head):
# kind 0 window / 1 float32 ring / 2 uint8 ring; off_grid moves the base off the 16-byte (uint8: 4-byte) grid.

A_SHAPES = [(2, 12, 256), (2, 10, 516), (2, 4, 4), (1, 20, 4), (2, 52, 20), (2, 1, 4), (1, 3, 516)]       # W % 4 == 0
U_SHAPES = [(2, 9, 253), (2, 13, 257), (2, 6, 514), (2, 1, 1), (2, 2, 3), (2, 3, 2), (1, 4, 37), (2, 50, 37), (1, 54, 255),
            (2, 7, 254)]
# Wo: 128 258 2 2 10 2 258 | 127 129 257 1 2 1 19 19 128 127;  Ho: 6 5 2 10 26 1 2 | 5 7 3 1 1 2 2 25 27 4
OFF_GRID = (2, 12, 256)     # an aligned shape run from a base off the grid: the unaligned instantiation at W % 4 == 0


def aligned_of(shape, off_grid):
    return shape[2] % 4 == 0 and not off_grid


def src_of(kind, aligned, masked):
    return 2 * kind + int(aligned) + 8 * int(masked)


def launch_of(prec, variant, kind, masked, aligned, shape):
    """launch_conv1's decision restated: (family, NW, TO, SRC, bands, quads)"""
    B, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    SRC = src_of(kind, aligned, masked)
    if prec == "f32x3":
        return (5, -1, -1, SRC, -1, -1)
    if prec == "f32s":
        return (4, -1, 0, SRC, -1, -1)
    if prec == "f16":
        if variant == 3 and not masked:
            return (1, -1, 1, SRC & 7, -1, -1)
        wtiles, quads = (Wo + 127) // 128, (Ho + 3) // 4
        bands, qpb = 0, 0
        for q in range(8, 3, -1):
            if B * wtiles * ((quads + q - 1) // q) >= 768:
                bands, qpb = (quads + q - 1) // q, q
                break
        if variant not in (2, 4) and not masked and (variant == 5 or bands > 0):
            if variant == 5:
                qpb, bands = 3, (quads + 2) // 3
            return (3, -1, -1, SRC, bands, qpb)
        if variant != 2:
            return (2, -1, 1, SRC, -1, -1)
        assert kind == 0 and not masked
        return (0, 4, 1, 0, -1, -1)
    if variant != 0 and kind == 0 and not masked:
        return (0, 8, 0, 0, -1, -1)
    return (0, 4, 0, SRC, -1, -1)


def _family_cases():
    out = []
    # (prec, variant, masks): every family at every shape, cycling through the sources so that each SRC value runs
    fams = [("f32", 0, (0, 1)), ("f16", 0, (0, 1)), ("f32s", 0, (0, 1)), ("f32x3", 0, (0, 1)),
            ("f16", 3, (0,)), ("f16", 5, (0,))]
    for prec, variant, masks in fams:
        for shapes, off in ((A_SHAPES, False), (U_SHAPES + [OFF_GRID], OFF_GRID)):
            combos = [(k, m) for m in masks for k in (0, 1, 2)]
            for i, shape in enumerate(shapes):
                for j in range(2):                       # two sources per shape: every SRC meets at least two shapes
                    kind, masked = combos[(2 * i + j) % len(combos)]
                    off_grid = off is not False and shape == off and i == len(shapes) - 1
                    inputs = "wide" if (kind != 2 and (i + j) % 3 == 0) else "u8"
                    out.append((prec, variant, kind, masked, off_grid, shape, inputs))
    # the single-instantiation A/B kernels (window, unmasked, SRC 0 whatever the alignment) at every shape
    for prec, variant in (("f32", 1), ("f16", 2)):
        for shape in A_SHAPES + U_SHAPES:
            out.append((prec, variant, 0, 0, False, shape, "u8"))
    # the masked float16 source takes the pair kernel whatever conv1_variant says
    for variant in (3, 5):
        for kind, shape in ((0, (2, 13, 257)), (1, (2, 12, 256)), (2, (2, 50, 37))):
            out.append(("f16", variant, kind, 1, False, shape, "u8"))
    # conv1_variant 4: never the marching kernel
    out.append(("f16", 4, 1, 0, False, (2, 10, 516), "u8"))
    # the positive set: S equals the value, the bound is sharp (a second network with positive conv1 weights)
    for prec, variant in (("f32", 0), ("f32", 1), ("f16", 0), ("f16", 2), ("f16", 3), ("f16", 5), ("f32s", 0), ("f32x3", 0)):
        for kind, shape in ((0, (2, 13, 257)), (2, (2, 10, 516))):
            if (prec, variant) in (("f32", 1), ("f16", 2)):
                kind = 0                                  # these two take a window tensor only
            out.append((prec, variant, kind, 0, False, shape, "pos"))
    return out


CASES = [c + (launch_of(c[0], c[1], c[2], c[3], aligned_of(c[5], c[4]), c[5]),) for c in _family_cases()]
# the marching kernel as the library selects it: B = 16 at 1280 x 720 -> 5 column tiles x 12 bands of 8 quads
MARCH_SHAPE = (16, 720, 1280)
MARCH_CASES = [("f16", 0, kind, 0, False, MARCH_SHAPE, "u8", (3, -1, -1, src_of(kind, True, 0), 12, 8)) for kind in (0, 1, 2)]
POOL_CASES = [(prec, shape) for prec in ("f32", "f16", "f32s", "f32x3")
              for shape in ((2, 9, 253), (2, 12, 256), (1, 13, 514), (2, 1, 1), (1, 4, 37), (2, 6, 3), (1, 3, 8))]
# H1 x W1: 5x127 6x128 7x257 1x1 2x19 3x2 2x4: pad_top / pad_left 1 (odd) and 0 (even)
HEAD_HW = [((1, 8, 8), 1), ((1, 32, 224), 7), ((1, 64, 128), 8), ((1, 96, 96), 9), ((1, 256, 256), 64), ((1, 720, 1280), 920)]
HEAD_B = [1, 15, 16, 17, 33]


def case_id(c):
    prec, variant, kind, masked, off, (B, H, W), inputs, exp = c
    return "%s-v%d-%s%s%s-%dx%dx%d-%s" % (prec, variant, ("win", "ringf", "ringu")[kind], "-mask" if masked else "",
                                          "-off" if off else "", B, H, W, inputs)


def instantiation(exp):
    return (FAMILY[exp[0]], exp[1], exp[2], exp[3])


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the table against the built library

_TEMPL = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+((?:conv1|maxpool)[a-z0-9_]*?_kernel)I((?:DF16_|f|Li\d+E)+)EEv")
_PLAIN = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+(maxpool[a-z0-9_]*?_kernel)EP")
_ARG = re.compile(rb"DF16_|f|Li(\d+)E")


def library_instantiations():
    """({(family, NW, TO, SRC)} of the conv1 kernels, {(pool kernel, id)}) from the mangled names in the built library"""
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    conv, pool = set(), set()
    for name, args in _TEMPL.findall(data):
        name = name.decode()
        vals = [(1 if m.group(0) == b"DF16_" else 0) if m.group(1) is None else int(m.group(1)) for m in _ARG.finditer(args)]
        if name == "maxpool_kernel":
            pool.add((name, vals[0]))
        elif name == "conv1_kernel":
            conv.add((name, vals[0], vals[1], vals[2]))
        elif name in ("conv1_f16_march_kernel", "conv1_x3_kernel"):
            conv.add((name, -1, -1, vals[0]))
        else:
            conv.add((name, -1, vals[0], vals[1]))
    for name in _PLAIN.findall(data):
        pool.add((name.decode(), {"maxpool_h8_kernel": 2, "maxpool_p_kernel": 3}[name.decode()]))
    return conv, pool


def test_table_covers_every_conv1_and_pool_instantiation():
    """62 conv1 instantiations (12 + 1 + 1 conv1_kernel, 6 one-row, 12 pair, 6 marching, 12 split, 12 x3) and four pool
    kernels when this was written: one without a case, or a case naming one that does not exist, fails here."""
    conv, pool = library_instantiations()
    assert len(conv) >= 62 and len(pool) >= 4, (len(conv), len(pool))
    covered = {instantiation(c[7]) for c in CASES + MARCH_CASES}
    assert not sorted(conv - covered), "conv1 instantiations without a case: %s" % sorted(conv - covered)
    assert covered <= conv, sorted(covered - conv)
    ids = {0: ("maxpool_kernel", 0), 1: ("maxpool_kernel", 1), 2: ("maxpool_h8_kernel", 2), 3: ("maxpool_p_kernel", 3)}
    pcov = {ids[POOL_OF[p]] for p, _ in POOL_CASES}
    assert pool - pcov == UNREACHABLE, (sorted(pool - pcov), sorted(UNREACHABLE))
    assert pcov <= pool
    # every family meets every seam class
    for fam in range(6):
        mine = [c for c in CASES if c[7][0] == fam]
        wos = {(c[5][2] - 1) // 2 + 1 for c in mine}
        hos = {(c[5][1] - 1) // 2 + 1 for c in mine}
        assert {127, 128, 129} <= wos and max(wos) >= 257, (fam, sorted(wos))
        assert any(h % 2 for h in hos) and {1, 2, 3} <= {h % 4 for h in hos}, (fam, sorted(hos))
        shapes = {c[5][1:] for c in mine}
        assert {(20, 4), (4, 37), (1, 1)} <= shapes and any(s[0] in (2, 3) or s[1] in (2, 3) for s in shapes), fam
    march5 = {((c[5][1] - 1) // 2 + 1) % 4 for c in CASES if c[7][0] == 3 and c[7][4] > 1}
    assert {1, 2, 3} <= march5, march5       # bands of three quads that end ragged, more than one band


def test_launch_table_names_the_library_s_own_choice_for_the_marching_kernel():
    assert launch_of("f16", 0, 0, 0, True, MARCH_SHAPE) == MARCH_CASES[0][7]
    assert launch_of("f16", 0, 0, 0, True, (1, 720, 1280))[0] == 2


def test_operands_reproduce_the_oracle(synthetic_weights):
    """the NumPy operands of this file against oracle.networks on a small frame: scale_RGB bit for bit (after the group
    reversal that the weights fold), and conv1 + BatchNorm + ReLU of the oracle within the float32 bound of this file"""
    import torch
    from oracle import networks as onet
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, (2, 9, 11, 21)).astype(F32)
    a = scaled(x)
    cs = np.array([(2 - c // 7) * 7 + c % 7 for c in range(21)])
    assert np.array_equal(onet.scale_RGB(x)[..., cs], a)
    scope = PREFIX + "resnet_v1_50/conv1"
    y = onet.conv2d_same_slim(onet.scale_RGB(x), onet._get(synthetic_weights, scope + "/weights"), 2)
    y = np.maximum(onet.batch_norm_inference(y, synthetic_weights, scope), 0.0)
    pre, S, tol = Operands(fold_conv1(synthetic_weights), "f32", a).full()
    # the oracle scales after the float32 GEMM (two more roundings of values <= S) and adds beta - mean * scale in parts
    nbad, worst = excess(torch.from_numpy(y), pre.clamp_min(0.0), tol + 2.0 ** -22 * S)
    assert nbad == 0, worst


# ---------------------------------------------------------------------------------------------------------------------
# CPU: every bound flags the defects it is there for, and passes a float32 evaluation of the reference

SIM_SHAPES = sorted(set(A_SHAPES + U_SHAPES))


def _sim_inputs(shape, masked, seed=3):
    B, H, W = shape
    pool = u8_to_f32(make_pool("u8", B + 6, H, W, seed))
    table = make_table(B, B + 6, False)
    x = gather_window(pool, table)
    mask = make_mask(B, H, W, seed + 1) if masked else None
    return pool, table, x, mask


def _flagged(prec, bad_pre, ops_ref):
    """does the criterion of `prec` reject the output relu(bad_pre) (float16: rounded to float16)?"""
    import torch
    pre, S, tol = ops_ref
    y = bad_pre.clamp_min(0.0)
    if prec == "f16":
        y = torch.from_numpy(rn16(y.numpy()))
    return judge(prec, y, pre, S, tol)[0] > 0


@pytest.mark.parametrize("prec", ["f32", "f16", "f32s", "f32x3"])
def test_bounds_flag_the_conv1_defects_at_every_shape_class(synthetic_weights, prec):
    """No GPU.  At every shape of the case table, in every precision's own operands and bound: a float32 evaluation of the
    reference passes; each simulated defect that changes anything at that shape is flagged."""
    import torch
    folded = fold_conv1(synthetic_weights)
    mean21 = np.array([MEAN_G[c // 7] for c in range(21)], dtype=F32)
    seen = set()
    for shape in SIM_SHAPES:
        B, H, W = shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        for masked in (False, True):
            pool, table, x, mask = _sim_inputs(shape, masked)
            a = scaled(x, mask)
            ops = Operands(folded, prec, a)
            ref = ops.full()
            pre = ref[0]
            # direction 1: the reference evaluated in float32 (accumulation error of a real kernel) passes
            y32 = (torch.nn.functional.conv2d(ops.ap.float() + (ops.alo.float() if ops.alo is not None else 0.0),
                                              ops.w.float(), stride=2).permute(0, 2, 3, 1) + ops.bias.float()).clamp_min(0.0)
            if prec == "f16":
                y32 = torch.from_numpy(rn16(y32.double().numpy()))
            assert judge(prec, y32, *ref)[0] == 0, (shape, masked, "float32 evaluation rejected")
            assert judge(prec, pre.clamp_min(0.0) if prec != "f16" else torch.from_numpy(rn16(pre.clamp_min(0.0).numpy())),
                         *ref)[0] == 0

            def other(a2=None, folded2=None, ring=None):
                return Operands(folded2 or folded, prec, a if a2 is None else a2, ring).full()[0]

            defects = {}
            w0 = folded[0].copy()
            w0[:, :, 3, :] = 0.0                                      # kernel row 3 of 7 (the one no shape pads away)
            defects["kernel row dropped"] = other(folded2=(w0, folded[1], folded[2]))
            defects["pad ring -mean"] = other(ring=-mean21)
            defects["no group reversal"] = other(folded2=unreversed_conv1(synthetic_weights))
            if masked:
                defects["mask on 18..20"] = other(a2=scaled(x, mask, mask_all=True))
                if W > 1 or H > 1:
                    defects["neighbour's mask"] = other(a2=scaled(x, np.roll(mask, 1, axis=2 if W > 1 else 1)))
            if Wo > 128:                                              # first column of the second tile, window one pixel late
                sh = other(a2=np.concatenate([a[:, :, 1:], np.zeros_like(a[:, :, :1])], axis=2))
                d = pre.clone()
                d[:, :, 128] = sh[:, :, 128]
                defects["tile seam shift"] = d
            xs = x.copy()
            xs[..., :18] = x[..., 3:]                                 # slot s reads table[b][s + 1]
            defects["window slot + 1"] = other(a2=scaled(xs, mask))
            if Ho > 1:
                d = pre.clone()
                d[:, Ho - 1] = pre[:, Ho - 2]                         # last row written twice from the row above
                defects["last row repeated"] = d
            d = pre.clone()
            d[:, Ho - 1] = float("nan")                               # last row of a ragged pair / band left unwritten
            defects["last row unwritten"] = d
            for name, bad in defects.items():
                assert _flagged(prec, bad, ref), (prec, shape, masked, name)
                seen.add(name)
    assert len(seen) == 9, sorted(seen)


def pool_ref(t, shift_left=False):
    """3 x 3 / 2 TF-SAME maximum of t [B, H1, W1, C] (torch, any float dtype); shift_left: the defect "window shifted by
    pad_left" (the window starts at 2 wo instead of 2 wo - pad_left)"""
    import torch
    B, H1, W1, C = t.shape
    Hp, Wp = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
    pt, pl = max((Hp - 1) * 2 + 3 - H1, 0) // 2, max((Wp - 1) * 2 + 3 - W1, 0) // 2
    if shift_left:
        pl = 0
    x = t.permute(0, 3, 1, 2)
    x = torch.nn.functional.pad(x, (pl, 2 * Wp + 1 - W1 - pl, pt, 2 * Hp + 1 - H1 - pt), value=float("-inf"))
    return torch.nn.functional.max_pool2d(x, 3, 2).permute(0, 2, 3, 1).contiguous()


def head_ref(x17, dense):
    """float64 head from the tap-17 tensor x17 [B, h, w, 2048]: (p, tol_p, F, tol_F given p exact).  dense: [(W, b)] x 4."""
    import torch
    B = x17.shape[0]
    flat = x17.double().reshape(B, -1, 2048)
    HW = flat.shape[1]
    p = flat.mean(1)
    tol_p = (tau(HW) + 2.0 ** -24) * flat.abs().mean(1) + TINY
    return p, tol_p


def dense_ref(p, dense, slope=0.2, e0=None):
    """F [B, 50] and its bound from the pooled features p [B, 2048] (float64, taken as exact, or known to within e0 per
    element: test_units_f64.py carries the network's composed bound into the head).  Two compositions, the
    smaller of which holds: the worst case e_next = e |W| + tau(K_l) S_l (as f64.fused_bound composes two layers; leaky
    slope <= 1 passes the error unamplified) -- which over four layers of 2048, 1024, 512 inputs grows past |F_t| itself
    and would not see a leaky slope of 0 -- and the same in quadrature, q_next = 2 sqrt(q^2 W^2) + tau(K_l) S_l: the
    errors carried by different inputs are independent roundings, tau(K) S is already the envelope of such a sum
    (sqrt(K) of them), and the factor 2 keeps the envelope's margin through the sum."""
    import torch
    x, e, q = p, torch.zeros_like(p), torch.zeros_like(p)
    if e0 is not None:
        e, q = e0.clone(), e0.clone()
    for i, (Wm, b) in enumerate(dense):
        Wm, b = Wm.double(), b.double()
        if i:
            x = torch.where(x >= 0, x, slope * x)
        K = Wm.shape[0]
        own = tau(K) * (x.abs() @ Wm.abs() + b.abs()) + K * TINY
        e = e @ Wm.abs() + own
        q = 2.0 * torch.sqrt((q * q) @ (Wm * Wm)) + own
        x = x @ Wm + b
    return x, torch.minimum(e, q)


def _dense_of(weights):
    import torch
    return [(torch.from_numpy(np.asarray(weights[PREFIX + "df/dense%d/W:0" % i], dtype=F32)),
             torch.from_numpy(np.asarray(weights[PREFIX + "df/dense%d/b:0" % i], dtype=F32))) for i in range(1, 5)]


def test_pool_and_head_checks_flag_their_defects(synthetic_weights):
    """No GPU: the bit-for-bit pool check sees a window shifted by pad_left; the pool5 bound sees a division by the padded
    slice length; the composed dense bound sees a leaky slope of 0 and a chunk that reads batch row b - 16, and passes a
    float32 evaluation of the head."""
    import torch
    g = torch.Generator().manual_seed(2)
    for shape in ((2, 5, 127, 8), (1, 7, 257, 8), (2, 1, 1, 8), (1, 3, 2, 8)):
        t = torch.rand(shape, generator=g)
        assert not torch.equal(pool_ref(t), pool_ref(t, shift_left=True)) or shape[2] % 2 == 0 or shape[2] == 1
    dense = _dense_of(synthetic_weights)
    for HW in (7, 9, 64, 920):
        x17 = torch.rand((33, HW, 1, 2048), generator=g)
        p, tol_p = head_ref(x17, dense)
        p32 = x17.reshape(33, HW, 2048).sum(1) * float(F32(1.0 / HW))
        assert excess(p32, p, tol_p)[0] == 0, HW
        per = (HW + 7) // 8
        if per * 8 != HW:
            assert excess(x17.double().reshape(33, HW, 2048).sum(1) / (per * 8), p, tol_p)[0] > 0, HW
    p = (torch.rand((33, 2048), generator=g) * 2.0).double()
    F, tol = dense_ref(p, dense)
    x = p.float()
    for i, (Wm, b) in enumerate(dense):
        if i:
            x = torch.where(x >= 0, x, 0.2 * x)
        x = x @ Wm + b
    assert excess(x, F, tol)[0] == 0
    assert excess(dense_ref(p, dense, slope=0.0)[0], F, tol)[0] > 0
    wrong = F.clone()
    wrong[16:32] = F[0:16]
    assert excess(wrong, F, tol)[0] > 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def last_root():
    from coupe.dvsg_amd import _lib
    f = (ctypes.c_int * len(ROOT_FIELDS))()
    _lib.call("dvsg_debug_last_root_kernel", f, len(ROOT_FIELDS))
    return tuple(f)


def _set_variant(v):
    from coupe.dvsg_amd import _lib
    _lib.call("dvsg_debug_set_option", b"conv1_variant", v)


_NETS = {}


def _net(weights, positive):
    from coupe.dvsg_amd.networks import LocNet
    key = (id(weights), positive)                 # (the checkpoint is kept in the entry, so its id stays its own)
    if key not in _NETS:
        _NETS[key] = (LocNet(positive_weights(weights) if positive else weights),
                      fold_conv1(positive_weights(weights) if positive else weights), weights)
    return _NETS[key][:2]


class Placed(object):
    """a host array on the device between sentinels, `off` bytes past the 256-byte grid"""

    def __init__(self, arr, dev, off=0):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
        self.n = t.numel() * t.element_size()
        self.off = off
        self.g = Guarded(self.n + 256, dev)
        self.g.body[off:off + self.n].copy_(t.view(-1).view(torch.uint8))
        self.before = self.g.body.clone()

    def ptr(self):
        return self.g.ptr() + self.off

    def unchanged(self):
        import torch
        return self.g.intact() and torch.equal(self.g.body, self.before)


def run_net(net, prec, kind, masked, src, table, mask, n_pool, B, H, W, stage, out_floats):
    """one network call (stage -1: F_t) with the output and a workspace of exactly dvsg_locnet_workspace_bytes between
    sentinels; returns (float32 output on the host, launch record)"""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    need = ctypes.c_size_t()
    _lib.call("dvsg_locnet_workspace_bytes", net.handle, B, H, W, ctypes.byref(need))
    ws = Guarded(need.value, dev)
    out = Guarded(out_floats * 4, dev)
    dims = (ctypes.c_int * 3)()
    s = torch.cuda.current_stream().cuda_stream
    code = PREC_CODE[prec]
    if masked:
        _lib.call("dvsg_locnet_forward_masked", net.handle, code, src.ptr(), kind, n_pool, table.ptr() if kind else None,
                  mask.ptr(), B, H, W, stage, out.ptr(), out_floats * 4, dims, ws.ptr(), need.value, s)
    elif kind:
        _lib.call("dvsg_locnet_forward_ring", net.handle, code, src.ptr(), int(kind == 2), n_pool, table.ptr(), B, H, W, stage,
                  out.ptr(), out_floats * 4, dims, ws.ptr(), need.value, s)
    elif stage < 0:
        _lib.call("dvsg_locnet_forward_" + prec, net.handle, src.ptr(), B, H, W, out.ptr(), ws.ptr(), need.value, s)
    else:
        _lib.call("dvsg_locnet_forward_tap_" + prec, net.handle, src.ptr(), B, H, W, stage, out.ptr(), out_floats * 4, dims,
                  ws.ptr(), need.value, s)
    rec = last_root()
    torch.cuda.synchronize()
    assert ws.intact(), "wrote past the %d-byte workspace" % need.value
    assert out.intact(), "wrote past the output"
    return out.view(torch.float32, (out_floats,)).cpu(), rec


def place_inputs(case, dev, gpu_mask=True):
    """the case's source, table and mask on the device, and the window x / mask on the host for the reference"""
    import torch
    import inputs as tin
    prec, variant, kind, masked, off_grid, (B, H, W), inputs, exp = case
    n = B + 6
    seed = 1000 * H + W
    pool = make_pool(inputs, n, H, W, seed)
    if kind != 2 and pool.dtype == np.uint8:
        pool = u8_to_f32(pool)
    table = make_table(B, n, oob=kind != 0 and inputs != "pos")
    pf = u8_to_f32(pool) if pool.dtype == np.uint8 else pool
    x = gather_window(pf, table)
    off = (1 if kind == 2 else 4) if off_grid else 0
    src = Placed(x if kind == 0 else pool, dev, off)
    tab = Placed(table, dev) if kind else None
    mask = mk = None
    if masked:
        from coupe.dvsg_amd.networks import random_mask_plane
        mk = random_mask_plane(tin.mask_homographies(seed, B), H, W).cpu().numpy()
        mask = Placed(mk, dev)
    return src, tab, mask, n, x, mk


_REF_CACHE = {}


def reference_for(case, folded, x, mk):
    prec, variant, kind, masked, off_grid, shape, inputs, exp = case
    rprec = "f32" if (prec == "f16" and variant == 2) else prec      # conv1_variant 2 multiplies the float32 operands
    key = (rprec, shape, inputs, masked, kind != 0)                   # ring tables carry two out-of-range slots
    if key not in _REF_CACHE:
        if len(_REF_CACHE) > 8:
            _REF_CACHE.clear()
        _REF_CACHE[key] = Operands(folded, rprec, scaled(x, mk)).full()
    return _REF_CACHE[key]


WORST = {}


def _note(exp, unit):
    fam = FAMILY[exp[0]] + ("<8>" if exp[1] == 8 else "") + ("<f16 out>" if exp[0] == 0 and exp[2] == 1 else "")
    WORST[fam] = max(WORST.get(fam, 0.0), unit)
    print("worst |y - ref| / (tau(K) S) so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_conv1_instantiation_against_float64(synthetic_weights, case):
    """tap 0 of one network call: the launch record names exactly the expected kernel, every element is within its float64
    bound (float16 outputs: inside the rounding interval), nothing outside the output and the workspace is written, the
    inputs keep their bytes."""
    import torch
    prec, variant, kind, masked, off_grid, (B, H, W), inputs, exp = case
    net, folded = _net(synthetic_weights, inputs == "pos")
    dev = torch.device("cuda:0")
    src, tab, mask, n, x, mk = place_inputs(case, dev)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    try:
        _set_variant(variant)
        y, rec = run_net(net, prec, kind, masked, src, tab, mask, n, B, H, W, 0, B * Ho * Wo * 64)
    finally:
        _set_variant(0)
    assert rec == exp + (-1, -1, -1), "launch record %s, expected %s" % (dict(zip(ROOT_FIELDS, rec)), exp)
    for p in (src, tab, mask):
        assert p is None or p.unchanged(), "an input changed"
    pre, S, tol = reference_for(case, folded, x, mk)
    if inputs == "pos" and prec != "f32s":      # (the f32s lo activation piece is signed: S > |pre| by conv(|alo| - alo, w))
        assert float((S - pre).abs().max()) <= 1e-9 * float(S.max()), "the positive set is not positive"
    nbad, unit = judge("f16" if prec == "f16" else prec, y.view(B, Ho, Wo, 64), pre, S, tol)
    print("%s: worst |y - ref| / (tau(K) S) = %.3f" % (case_id(case), unit))
    _note(exp, unit)
    if nbad:
        d = ((y.view(B, Ho, Wo, 64).double() - pre.clamp_min(0.0)).abs() > tol).nonzero()
        print("out of bounds at (b, ho, wo, n): first %s last %s" % (d[0].tolist(), d[-1].tolist()))
    assert nbad == 0, "%d elements out of bounds (worst %.3f x tau(K) S)" % (nbad, unit)


def march_strata(B, Ho, Wo, band_rows, seed):
    """the checked subset at the marching kernel's own size: all four borders three deep, two rows on each side of every
    band seam, two columns on each side of every column-tile seam -- as row and column strips -- and a seeded 1 % of the
    rest as points"""
    rows = set(range(3)) | set(range(Ho - 3, Ho))
    for s in range(band_rows, Ho, band_rows):
        rows |= {s - 2, s - 1, s, s + 1}
    cols = set(range(3)) | set(range(Wo - 3, Wo))
    for s in range(128, Wo, 128):
        cols |= {s - 2, s - 1, s, s + 1}
    rows, cols = sorted(rows), sorted(cols)

    def runs(v):
        out, a = [], v[0]
        for p, q in zip(v, v[1:] + [None]):
            if q != p + 1:
                out.append((a, p + 1))
                a = q
        return out
    rest = np.ones((B, Ho, Wo), dtype=bool)
    rest[:, rows] = False
    rest[:, :, cols] = False
    idx = np.argwhere(rest)
    pick = np.random.default_rng(seed).choice(len(idx), size=(len(idx) + 99) // 100, replace=False)
    return runs(rows), runs(cols), idx[np.sort(pick)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MARCH_CASES, ids=[case_id(c) for c in MARCH_CASES])
def test_marching_kernel_as_the_library_selects_it(synthetic_weights, case):
    """B = 16 at 1280 x 720, conv1_variant 0: 5 x 12 bands of 8 quads.  A full float64 reference is 2.4e11 MACs, so the
    check covers a stated subset (march_strata): the strata in full, never fewer."""
    import torch
    prec, variant, kind, masked, off_grid, (B, H, W), inputs, exp = case
    net, folded = _net(synthetic_weights, False)
    dev = torch.device("cuda:0")
    src, tab, mask, n, x, mk = place_inputs(case, dev)
    Ho, Wo = H // 2, W // 2
    y, rec = run_net(net, prec, kind, 0, src, tab, None, n, B, H, W, 0, B * Ho * Wo * 64)
    assert rec == exp + (-1, -1, -1), "launch record %s, expected %s" % (dict(zip(ROOT_FIELDS, rec)), exp)
    assert src.unchanged() and (tab is None or tab.unchanged())
    y = y.view(B, Ho, Wo, 64)
    ops = Operands(folded, "f16", scaled(x))
    row_runs, col_runs, pts = march_strata(B, Ho, Wo, 4 * exp[5], seed=77)
    assert len(row_runs) == 13 and len(col_runs) == 6 and len(pts) >= 0.0099 * B * (Ho - 50) * (Wo - 22)
    worst, nbad, count = 0.0, 0, 0
    for r0, r1 in row_runs:
        b_, u_ = judge("f16", y[:, r0:r1], *ops.region(r0, r1, 0, Wo))
        nbad, worst, count = nbad + b_, max(worst, u_), count + B * (r1 - r0) * Wo * 64
    for c0, c1 in col_runs:
        b_, u_ = judge("f16", y[:, :, c0:c1], *ops.region(0, Ho, c0, c1))
        nbad, worst, count = nbad + b_, max(worst, u_), count + B * Ho * (c1 - c0) * 64
    pb, ph, pw = (torch.from_numpy(pts[:, i].copy()) for i in range(3))
    b_, u_ = judge("f16", y[pb, ph, pw], *ops.points(pb, ph, pw))
    nbad, worst, count = nbad + b_, max(worst, u_), count + len(pts) * 64
    print("%s: %d elements checked, worst |y - ref| / (tau(K) S) = %.3f" % (case_id(case), count, worst))
    _note(exp, worst)
    assert nbad == 0, "%d elements out of bounds (worst %.3f x tau(K) S)" % (nbad, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shape", POOL_CASES, ids=["%s-%dx%dx%d" % ((p,) + s) for p, s in POOL_CASES])
def test_pool1_is_the_same_call_s_conv1_maximum_bit_for_bit(synthetic_weights, prec, shape):
    """tap 1 == the 3 x 3 / 2 SAME maximum of tap 0 of the same inputs, bit for bit, in every precision (the taps convert
    float16 and the P format to float32 exactly), at odd and even H1, W1.  conv1's output is >= 0 after ReLU, so whether
    the pad value is -inf or 0 cannot be observed here; the window geometry is what this pins."""
    import torch
    B, H, W = shape
    net, _ = _net(synthetic_weights, False)
    dev = torch.device("cuda:0")
    case = (prec, 0, 0, 0, False, shape, "u8", None)
    src, tab, mask, n, x, mk = place_inputs(case, dev)
    H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
    t0, _ = run_net(net, prec, 0, 0, src, None, None, n, B, H, W, 0, B * H1 * W1 * 64)
    t1, rec = run_net(net, prec, 0, 0, src, None, None, n, B, H, W, 1, B * Hp * Wp * 64)
    assert rec[6:] == (POOL_OF[prec], -1, -1), dict(zip(ROOT_FIELDS, rec))
    assert src.unchanged()
    want = pool_ref(t0.view(B, H1, W1, 64))
    assert torch.equal(t1.view(B, Hp, Wp, 64), want), "%d elements differ" % int((t1.view(B, Hp, Wp, 64) != want).sum())


def _head_case(weights, prec, shape):
    import torch
    B, H, W = shape
    net, _ = _net(weights, False)
    dev = torch.device("cuda:0")
    case = (prec, 0, 0, 0, False, shape, "wide", None)
    src, tab, mask, n, x, mk = place_inputs(case, dev)
    h, w = H, W
    for _ in range(5):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x17, r17 = run_net(net, prec, 0, 0, src, None, None, n, B, H, W, 17, B * h * w * 2048)
    p, r18 = run_net(net, prec, 0, 0, src, None, None, n, B, H, W, 18, B * 2048)
    F, rF = run_net(net, prec, 0, 0, src, None, None, n, B, H, W, -1, B * 50)
    assert src.unchanged()
    root = launch_of(prec, 0, 0, 0, W % 4 == 0, shape) + (POOL_OF[prec],)
    assert r17 == root + (-1, -1) and r18 == root + (AVG_OF[prec], -1) and rF == root + (AVG_OF[prec], (B + 15) // 16), \
        (r17, r18, rF)
    dense = _dense_of(weights)
    p = p.view(B, 2048)
    pref, tol_p = head_ref(x17.view(B, h, w, 2048), dense)
    nbad, worst = excess(p, pref, tol_p)
    print("%s %s: HW = %d, pool5 worst %.3f of its bound" % (prec, shape, h * w, worst))
    assert nbad == 0, "pool5: %d out of bounds (worst %.3f)" % (nbad, worst)
    Fref, tol_F = dense_ref(p.double(), dense)
    nbad, worst = excess(F.view(B, 50), Fref, tol_F)
    print("%s %s: F_t worst %.3f of its composed bound" % (prec, shape, worst))
    assert nbad == 0, "F_t: %d out of bounds (worst %.3f)" % (nbad, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16", "f32s", "f32x3"])
@pytest.mark.parametrize("shape,HW", HEAD_HW, ids=["HW%d" % hw for _, hw in HEAD_HW])
def test_head_against_float64_around_the_pool_slices(synthetic_weights, prec, shape, HW):
    """pool5 from the same inputs' tap 17 within (tau(HW) + 2^-24) mean|x|, F_t from tap 18 within the bound composed layer
    by layer; HW around kPoolSplits = 8 (empty slices at HW = 1, 7, 9), every precision's average-pool kernel."""
    _head_case(synthetic_weights, prec, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("B", HEAD_B)
def test_head_dense_chunks_of_sixteen(synthetic_weights, B):
    _head_case(synthetic_weights, "f32", (B, 8, 8))
    if B == 33:
        _head_case(synthetic_weights, "f16", (B, 40, 40))
