"""The float16-mode conv GEMMs and block 1's fused kernels, all precisions, pinned to float64 element by element.

Every instantiation of conv_gemm_kernel on float16 tensors (plain weights and [hi | lo] SPLIT rows), of the three 256 x 128
kernels of conv_gemm_wide16.hip and of the fused conv2 + conv3 kernels is launched on purpose by a case of this file (or,
for the float32 tensors, of test_conv_gemm_f64.py), which names the launch it expects; dvsg_debug_last_conv_kernel (and, for
conv_gemm_kernel, dvsg_debug_last_conv_config) must report exactly that, and a CPU test checks that the two tables cover
every instantiation the built library holds.

A float16 output is held to an interval, not a tolerance: the stored value must be a correctly rounded value of something
within the accumulation error of the float64 result,

    E = tau(K) S,  lo = RN16(act(pre - E)),  hi = RN16(act(pre + E)),  lo <= y <= hi  (NaN fails),

with tau and C_ONE as in test_conv_gemm_f64.py, pre the float64 convolution of the operands exactly as the mode holds them
(float16 x and residual, w = hi + 2^-11 lo or hi, float32 bias) plus bias and residual, act ReLU or the identity (both
monotone, so the interval is exact), and S = conv(|x|, |hi| + 2^-11 |lo|) + |bias| + |res| (>= conv(|x|, |w|)).  The
kernel's rounding sites besides the float32 accumulation -- the fold hi + 2^-11 lo of the two accumulators, the bias add,
the residual add and the split-K / stream-K slab sums -- each cost at most 2^-24 of the running magnitude, inside the
C_ONE term of tau.  The lo accumulator's own accumulation error is 2^-11 of a sum of the same size, also inside S.
RN16 is NumPy's float64 -> float16 cast, correctly rounded in one step (torch's goes through float32 and rounds twice).

Every float16 case prints its worst |y - act(pre)| / (E + ulp16(y) / 2) and asserts a floor on the fraction of elements
that admit exactly one float16 value: the criterion must be sharp, not only pass.
"""
import ctypes
import math
import re

import numpy as np
import pytest

import test_conv_gemm_f64 as f64

tau = f64.tau
LO = 2.0 ** -11              # the lo rows' scale: w = hi + 2^-11 lo
MIB = 1 << 20
KERNEL_FIELDS = 6            # dvsg_debug_last_conv_kernel: family, four template arguments, weight source
SLAB_BASE = 2048 + 64 * MIB  # conv_gemm_op: tickets (align256(512 ints)) + the partial-tile slabs; the packed copies follow


# ---------------------------------------------------------------------------------------------------------------------
# the float16 rounding and the interval criterion

def rn16(v):
    """float64 -> nearest float16 (ties to even), correctly rounded in one step, returned as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)


def rtz16(v):
    """float64 -> float16 rounded toward zero (a wrong kernel's output rounding), as float64"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        r = v.astype(np.float16)
        away = np.abs(r.astype(np.float64)) > np.abs(v)
        r = np.where(away, np.nextafter(r, np.float16(0)), r)
    return r.astype(np.float64)


def ulp16(v):
    """spacing of float16 in the binade RN16(|v|) falls in (2^-24 below 2^-14, inf past the range), float64"""
    a = rn16(np.abs(np.asarray(v, dtype=np.float64)))
    _, e = np.frexp(a)
    u = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)
    return np.where(np.isinf(a), np.inf, np.where(a < 2.0 ** -14, 2.0 ** -24, u))


def interval16(pre, E, relu):
    a, b = pre - E, pre + E
    if relu:
        a, b = np.maximum(a, 0.0), np.maximum(b, 0.0)
    return rn16(a), rn16(b)


def check16(y, pre, E, relu):
    """(number of elements outside [lo, hi] (NaN counts), worst |y - act(pre)| / (E + ulp16(y)/2) over the finite
    elements, fraction of the non-clamped elements with lo == hi)"""
    lo, hi = interval16(pre, E, relu)
    bad = ~((lo <= y) & (y <= hi))
    act = np.maximum(pre, 0.0) if relu else pre
    fin = np.isfinite(y) & np.isfinite(act)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ratio = np.abs(y - act)[fin] / (E[fin] + ulp16(y[fin]) / 2)
    live = hi != 0
    single = float((lo == hi)[live].mean()) if live.any() else 1.0
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0, single


# ---------------------------------------------------------------------------------------------------------------------
# operands: two sets per case, plus the range edges
#   mixed: x in [-1, 3), zero-mean weights: S / |y| grows like sqrt(K), cancellation exercised, fewer single-valued outputs
#   pos:   x in [0, 1) (as after a ReLU), weights offset by 0.4 of their range: S / |y| = O(1), most outputs single-valued
#   tiny:  float16-subnormal activations (< 2^-19) and outputs in float16's subnormal range (< 2^-14)
#   large: outputs up to ~5e4;  overflow: most true outputs beyond 65520, which round to +inf
# Outside the mixed set the weights of the hi / lo pairs sit 0.1-0.45 of a float16 step beyond their hi piece, so every lo
# piece has the weight's sign: a kernel that drops or mis-scales the lo rows is then off by a fixed part of an output ulp
# at every element, instead of by a random sum of 2^-12-relative terms that falls inside tau(K) S from K ~ 4096 on.

def make16(shape, res_mode, opset, seed, device, split):
    """x, w64, wabs (|hi| + 2^-11 |lo|), wdev (the weights as the launch takes them), hi, lo, bias, res, res_stride"""
    import torch
    B, H, W, cin, cout, ks, stride = shape
    K = ks * ks * cin
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator(device=device).manual_seed(seed)

    def u(*s):
        return torch.rand(s, generator=g, device=device)

    ws = 2.0 / K ** 0.5
    if opset == "mixed":
        x, w, bscale = u(B, H, W, cin) * 4.0 - 1.0, (u(cout, K) - 0.5) * ws, 0.5
    elif opset == "tiny":
        x, w, bscale = u(B, H, W, cin) * 2.0 ** -19, (u(cout, K) - 0.1) * ws, 2.0 ** -19
    elif opset == "pos":
        x, w, bscale = u(B, H, W, cin), (u(cout, K) - 0.1) * ws, 0.5
    else:   # mean output 25.6 sqrt(K) big: 3e4 (large) or 8e4 (overflow)
        big = (3e4 if opset == "large" else 8e4) / (25.6 * K ** 0.5)
        x, w, bscale = u(B, H, W, cin) * 64.0, (u(cout, K) - 0.1) * ws * big, 500.0
    x = x.half()
    bias = (u(cout) - 0.5) * 2 * bscale
    res, rs = None, 1
    if res_mode:
        rs = 1 if res_mode == 1 else 2
        res = ((u(B, (ho - 1) * rs + 1, (wo - 1) * rs + 1, cout) - 0.5) * 2 * bscale).half()
    hi = w.half()
    lo = None
    if split:
        if opset != "mixed":
            a = hi.float().abs()
            step = torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -14))) - 10)
            w = torch.sign(hi.float()) * (a + (0.1 + 0.35 * u(cout, K)) * step)
            hi = w.half()
        lo = ((w - hi.float()) * 2048.0).half()
        wdev = torch.cat([hi.reshape(cout // 64, 64, K), lo.reshape(cout // 64, 64, K)], 1).reshape(2 * cout, K).contiguous()
        w64 = hi.double() + LO * lo.double()
        wabs = hi.double().abs() + LO * lo.double().abs()
    else:
        wdev, w64, wabs = hi.contiguous(), hi.double(), hi.double().abs()
    return x, w64, wabs, wdev, hi, lo, bias, res, rs


def reference16(x, w64, wabs, bias, res, ks, stride, rs):
    """float64 pre-activation and S"""
    pre = f64.conv64(x.double(), w64, ks, stride) + bias.double()
    S = f64.conv64(x.double().abs(), wabs, ks, stride) + bias.double().abs()
    if res is not None:
        r = res.double()[:, ::rs, ::rs]
        pre, S = pre + r, S + r.abs()
    return pre, S


# ---------------------------------------------------------------------------------------------------------------------
# the configuration matrix.  A shape is (B, H, W, Cin, Cout, ksize, stride).  mode "f16": plain float16 weights
# (dvsg_conv_gemm_f16), "f16s": hi / lo pairs (dvsg_conv_gemm_f16s).  `opts` are dvsg_debug_set_option values for the case
# (conv_gemm_kernel cases keep the 256 x 128 kernels out with a huge wide16_min_tiles, the wide16 cases force them with 1).
# `exp` is ("g", BN, WM, WN, MODE, ksplit, streamk_tail, mt_fast) for conv_gemm_kernel, or ("w", family, weight source).
# Scratch: "pk" = exactly what conv_gemm_op needs for the packed weight copies (base + 3 need), "pk-" = 256 bytes less.

GEMM = {"wide16_min_tiles": 1 << 30}
WIDE = {"wide16_min_tiles": 1}
NO_A = dict(WIDE, wide16_arows=0, wide16_hreuse=0)
DEFAULTS = {"conv_variant": 0, "wide16_min_tiles": 128, "wide16_arows": 1, "wide16_packed": 1, "wide16_hreuse": 1,
            "fused_hreuse": 1}
ALL6, NORES = f64.ALL6, f64.NORES

BASE = []   # (mode, shape, scratch, opts, exp, combos)
for ks in (1, 3):
    # plain float16 weights: conv_gemm_kernel's six configurations
    BASE += [("f16", (1, 3, 43, 64, 64, ks, 1), "none", GEMM, ("g", 64, 2, 2, 0, 1, 0, 0), ALL6),       # M = 129; K = 64 (1x1)
             ("f16", (1, 16, 8, 64, 128, ks, 1), "none", dict(GEMM, conv_variant=2), ("g", 64, 4, 2, 0, 1, 0, 0), ALL6),
             ("f16", (1, 511, 511, 64, 128, ks, 2), "none", GEMM, ("g", 128, 2, 2, 0, 1, 0, 0), ALL6),  # 512 wide tiles
             ("f16", (1, 514, 514, 64, 128, ks, 2), "none", GEMM, ("g", 128, 2, 4, 0, 1, 0, 0), ALL6),  # 517 wide tiles
             ("f16", (2, 17, 15, 2048, 128, 1, 2) if ks == 1 else (1, 20, 28, 256, 64, 3, 1), "17M", GEMM,
              ("g", 64, 2, 2, 1, 8, 0, 0), ALL6),
             ("f16", (1, 64, 128, 2048, 512, 1, 1) if ks == 1 else (1, 64, 128, 512, 512, 3, 1), "65M", GEMM,
              ("g", 128, 2, 4, 2, 1, 256, 0), NORES)]                                                     # 3x3: K = 4608
    # hi / lo pairs: always 128 stacked rows per tile
    BASE += [("f16s", (1, 3, 43, 64, 64, ks, 1), "none", GEMM, ("g", 128, 2, 2, 0, 1, 0, 0), ALL6),
             ("f16s", (1, 514, 514, 64, 64, ks, 2), "none", GEMM, ("g", 128, 2, 4, 0, 1, 0, 0), ALL6),
             ("f16s", (2, 17, 15, 2048, 128, 1, 2) if ks == 1 else (1, 20, 28, 256, 64, 3, 1), "17M", GEMM,
              ("g", 128, 2, 4, 1, 8, 0, 0), ALL6),
             ("f16s", (1, 64, 128, 2048, 256, 1, 1) if ks == 1 else (1, 64, 128, 512, 256, 3, 1), "65M", GEMM,
              ("g", 128, 2, 4, 2, 1, 256, 0), NORES)]
# the 256 x 128 kernels: 64-byte activation rows (family 1), 128-byte rows (2), a 3x3 kernel row from one staged run (3)
BASE += [
    ("f16", (1, 257, 1, 64, 128, 1, 1), "none", WIDE, ("w", 1, 0), ALL6),          # M = 257, one pixel wide, from [rows][K]
    ("f16s", (1, 257, 1, 64, 64, 1, 1), "none", WIDE, ("w", 1, 0), ALL6),
    ("f16", (1, 13, 20, 64, 128, 3, 1), "pk", NO_A, ("w", 1, 1), ALL6),              # packed, order 0
    ("f16s", (1, 31, 33, 64, 64, 3, 2), "pk", NO_A, ("w", 1, 1), ALL6),             # stride 2 from odd sizes
    ("f16", (1, 16, 20, 256, 128, 1, 1), "pk", WIDE, ("w", 2, 1), ALL6),
    ("f16s", (2, 5, 7, 512, 64, 1, 1), "pk", WIDE, ("w", 2, 1), ALL6),              # M = 70: below one tile
    ("f16", (1, 17, 17, 64, 128, 3, 2), "pk", WIDE, ("w", 2, 1), ALL6),
    ("f16s", (1, 12, 22, 128, 64, 3, 1), "pk", dict(WIDE, wide16_hreuse=0), ("w", 2, 1), ALL6),
    ("f16", (1, 14, 40, 64, 128, 3, 1), "pk", WIDE, ("w", 3, 1), ALL6),
    ("f16s", (2, 9, 30, 128, 64, 3, 1), "pk", WIDE, ("w", 3, 1), ALL6),
]
EXTRA = [
    # M = 32: 1x1 split-K 8 ways with K = 8192 (mt_fast: 128 rows x K x 2 bytes >= 2 MiB; 4096 outputs, enough for the
    # single-valued floor, which 128 outputs of M = 1 measured 0.09 against 0.10 could not hold), M = 1: 3x3 plain tiles
    ("f16s", (1, 4, 8, 8192, 128, 1, 1), "17M", GEMM, ("g", 128, 2, 4, 1, 8, 0, 1), [(1, 1)]),
    ("f16s", (1, 1, 1, 64, 64, 3, 1), "none", GEMM, ("g", 128, 2, 2, 0, 1, 0, 0), [(0, 1)]),
    ("f16", (1, 1, 1, 64, 128, 3, 1), "none", GEMM, ("g", 64, 2, 2, 0, 1, 0, 0), [(1, 1)]),
    ("f16", (1, 31, 15, 64, 64, 3, 2), "none", GEMM, ("g", 64, 2, 2, 0, 1, 0, 0), [(1, 2)]),
    ("f16", (1, 1, 1, 64, 128, 1, 1), "none", WIDE, ("w", 1, 0), [(1, 1)]),
    ("f16s", (1, 1, 1, 64, 64, 3, 1), "pk", WIDE, ("w", 3, 1), [(1, 1)]),
    # block 4's K = 4608 in the 256 x 128 geometry
    ("f16s", (1, 8, 40, 512, 256, 3, 1), "pk", WIDE, ("w", 3, 1), [(1, 1)]),
    # the packed copies: scratch exactly big enough, then 256 bytes short (the layer then runs from [rows][K])
    ("f16", (1, 16, 16, 64, 128, 1, 1), "pk", WIDE, ("w", 1, 1), [(0, 1)]),
    ("f16", (1, 16, 16, 64, 128, 1, 1), "pk-", WIDE, ("w", 1, 0), [(0, 1)]),
    ("f16s", (1, 12, 20, 64, 64, 3, 1), "pk", WIDE, ("w", 3, 1), [(1, 1)]),
    ("f16s", (1, 12, 20, 64, 64, 3, 1), "pk-", WIDE, ("w", 1, 0), [(1, 1)]),
    ("f16s", (1, 12, 20, 64, 64, 3, 1), "pk", dict(WIDE, wide16_packed=0, wide16_arows=0, wide16_hreuse=0), ("w", 1, 0),
     [(0, 0)]),
]

CASES = [(mode, shape, scratch, opts, exp, relu, res)
         for mode, shape, scratch, opts, exp, combos in BASE + EXTRA for relu, res in combos]


def case_id(c):
    mode, (B, H, W, cin, cout, ks, stride), scratch, opts, exp, relu, res = c
    o = "".join("-%s%d" % (k.replace("wide16_", "").replace("conv_", ""), v) for k, v in sorted(opts.items())
                if k != "wide16_min_tiles")
    return "%s-k%ds%d-%dx%dx%dx%d-%d-%s%s-%s-r%d-res%d" % (mode, ks, stride, B, H, W, cin, cout, scratch, o,
                                                         "g" if exp[0] == "g" else "w%d" % exp[1], relu, res)


def expected_records(c):
    """(dvsg_debug_last_conv_config or None, dvsg_debug_last_conv_kernel) the case must leave"""
    mode, (B, H, W, cin, cout, ks, stride), scratch, opts, exp, relu, res = c
    if exp[0] == "g":
        BN, WM, WN, MODE, ksplit, tail, mt_fast = exp[1:]
        return ((1, BN, WM, WN, ks, relu, res, MODE, int(mode == "f16s"), 0, ksplit, tail, mt_fast),
                (0, -1, -1, -1, -1, -1))
    fam, wsrc = exp[1:]
    split = int(mode == "f16s")
    args = (relu, res, split, -1) if fam == 3 else (ks, relu, res, split)
    return None, (fam,) + args + (wsrc,)


def instantiation(c):
    """the kernel a case runs as a coverage key: (family, template arguments ...); family 0 as (0, T, BN, ..., X3)"""
    cfg, ker = expected_records(c)
    if ker[0] == 0:
        return (0,) + tuple(cfg[:10])
    return tuple(v for v in ker[:5] if v != -1)


def scratch_bytes(kind, mode, shape):
    B, H, W, cin, cout, ks, stride = shape
    if kind in f64.SCRATCH:
        return f64.SCRATCH[kind]
    rows = 2 * cout if mode == "f16s" else cout
    need = -(-(rows * ks * ks * cin * 2) // 256) * 256
    return SLAB_BASE + 3 * need - (256 if kind == "pk-" else 0)


# ---------------------------------------------------------------------------------------------------------------------
# how sharp the criterion is: floors on the fraction of (non-clamped) elements that admit exactly one float16 value.
# Two admissible values happen in a fraction ~ 2 E / ulp16(y) ~ 2^-13 (sqrt(K) + 4) S / |y| of the elements.
#   pos, large, overflow, tiny: S / |y| ~ 1: 2 E / ulp16(y) <= 2^-13 (sqrt(8192) + 4) ~ 0.012, so >= 97 % at every K
#          here (float64 simulation of these operands: >= 98 %): floor 90 %
#   mixed: S / |y| ~ 1.1 sqrt(K) at the median and a heavy tail near y = 0.  SIM_MIXED holds the single-valued fractions
#          of a float64 simulation of these operands (5 x 6 pixels, both ReLU settings, the lower one); the floor is
#          0.8 x that, interpolated in log K
SIM_MIXED = ((64, 0.93), (256, 0.865), (512, 0.787), (576, 0.779), (1152, 0.689), (2048, 0.477), (2304, 0.524),
             (4608, 0.328), (8192, 0.121))


def single_floor(opset, K):
    if opset != "mixed":
        return 0.90
    ks, fs = zip(*SIM_MIXED)
    return 0.8 * float(np.interp(math.log(K), [math.log(k) for k in ks], fs))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: RN16 is correctly rounded in one step

def test_rn16_is_correctly_rounded_at_midpoints():
    """One float64 ulp either side of float16 midpoints rounds to the nearer neighbour -- in the normal range, the subnormal
    range and at the overflow threshold -- and exact midpoints go to even.  torch's double -> half (through float32) gets
    the first example wrong, which is why it is not used."""
    import torch
    cases = []
    for a in (1.0, 1.0 + 2 ** -10, 1.5, 3.0 * 2 ** -14, 2.0 ** -24, 5 * 2.0 ** -24, 1023 * 2.0 ** -24, 65504.0 - 32.0, -2.0):
        b = float(np.nextafter(np.float16(a), np.float16(np.inf)))
        mid = (a + b) / 2
        even = a if int(np.float16(a).view(np.uint16)) % 2 == 0 else b
        cases += [(np.nextafter(mid, -np.inf), a), (mid, even), (np.nextafter(mid, np.inf), b)]
    # 65520 is the midpoint between 65504 and the first value past float16's range: from it on, inf
    cases += [(np.nextafter(65520.0, -np.inf), 65504.0), (65520.0, np.inf), (1e6, np.inf), (-65520.0, -np.inf),
              (2.0 ** -26, 0.0), (np.nextafter(2.0 ** -25, 1.0), 2.0 ** -24), (2.0 ** -25, 0.0)]
    v = np.array([c[0] for c in cases])
    want = np.array([c[1] for c in cases])
    got = rn16(v)
    assert np.array_equal(got, want), [(a, b, c) for a, b, c in zip(v, got, want) if b != c]
    assert torch.tensor([1 + 2 ** -11 + 2 ** -40], dtype=torch.float64).half().item() == 1.0   # double rounding
    assert rn16(1 + 2 ** -11 + 2 ** -40) == 1 + 2 ** -10
    assert rtz16(np.array([1 + 2 ** -10 - 2 ** -40, -(1 + 2 ** -10 - 2 ** -40), 7e4])).tolist() == [1.0, -1.0, 65504.0]
    assert ulp16(1.0) == 2 ** -10 and ulp16(2.0 ** -20) == 2 ** -24 and ulp16(65504.0) == 32.0
    assert ulp16(np.nextafter(2.0, 0.0)) == 2 ** -9 and ulp16(1e6) == np.inf


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the criterion rejects wrong kernels at every (mode, K) of the matrix

def _small(shape):
    B, H, W, cin, cout, ks, stride = shape
    return (1, 5, 6, cin, min(cout, 128), ks, stride)


def _wrong_kernels(x, hi, lo, bias, res, ks, stride, rs, relu):
    """RN16 of simulated wrong kernels (float64): the lo rows dropped, the lo fold at 2^-10, one 32-k stage dropped (the
    middle one) at one pixel, one channel's bias dropped, every pixel's residual taken from its neighbour; and RTZ16 of
    the right result"""
    import torch
    xd = x.double()
    lo_d = lo.double() if lo is not None else torch.zeros_like(hi.double())
    w = hi.double() + LO * lo_d
    r = res.double()[:, ::rs, ::rs]

    def out(wf, b=bias.double(), rr=r):
        v = f64.conv64(xd, wf, ks, stride) + b + rr
        return rn16((v.clamp_min(0.0) if relu else v).numpy())

    pre = f64.conv64(xd, w, ks, stride) + bias.double() + r
    K = w.shape[1]
    st = 32 * ((K // 32) // 2)
    w_st = w.clone()
    w_st[:, st:st + 32] = 0.0
    one = f64.conv64(xd, w_st, ks, stride) + bias.double() + r
    drop_k = pre.clone()
    drop_k[0, 1, 1] = one[0, 1, 1]
    b2 = bias.double().clone()
    b2[int(bias.abs().argmax())] = 0.0
    rr = torch.roll(r, 1, dims=2)
    act = (lambda t: t.clamp_min(0.0)) if relu else (lambda t: t)   # noqa: E731
    bad = []
    if lo is not None:
        bad += [("lo rows dropped", out(hi.double())), ("lo fold at 2^-10", out(hi.double() + 2 * LO * lo_d))]
    bad += [("K stage dropped", rn16(act(drop_k).numpy())), ("bias dropped", out(w, b=b2)),
            ("neighbour's residual", out(w, rr=rr)), ("round toward zero", rtz16(act(pre).numpy()))]
    return bad


@pytest.mark.parametrize("opset", ["pos", "mixed"])
def test_criterion_rejects_wrong_kernels_at_every_mode_and_k(opset):
    """No GPU: on a CPU stand-in of every (mode, K, kernel size, stride) of the matrix the float64 result rounded with RN16
    passes, its single-valued fraction meets the floor the GPU cases assert, and each simulated wrong kernel fails.  The
    lo-row faults are asserted on the pos set, whose lo pieces carry their weight's sign (make16); in the mixed set their
    effect is a random sum below tau(K) S at large K, so there they are only exercised."""
    seen = set()
    for c in CASES:
        mode, shape = c[0], c[1]
        K = shape[5] ** 2 * shape[3]
        key = (mode, K, shape[5], shape[6])
        if key in seen:
            continue
        seen.add(key)
        s = _small(shape)
        x, w64, wabs, wdev, hi, lo, bias, res, rs = make16(s, 1, opset, 5, "cpu", mode == "f16s")
        pre, S = reference16(x, w64, wabs, bias, res, s[5], s[6], rs)
        pre, E = pre.numpy(), (tau(K) * S).numpy()
        for relu in (0, 1):
            good = rn16(np.maximum(pre, 0.0) if relu else pre)
            nbad, worst, single = check16(good, pre, E, relu)
            assert nbad == 0 and worst <= 1.0, (key, relu)
            assert single >= single_floor(opset, K), (key, relu, single, single_floor(opset, K))
            for name, bad in _wrong_kernels(x, hi, lo, bias, res, s[5], s[6], rs, relu):
                if opset == "mixed" and name.startswith("lo "):
                    continue
                assert check16(bad, pre, E, relu)[0] > 0, (key, relu, name)
    Ks = {k[1] for k in seen}
    assert {64, 4608, 8192} <= Ks


# ---------------------------------------------------------------------------------------------------------------------
# block 1's fused conv2 + conv3, every kernel and precision, through dvsg_debug_conv3x3_1x1.  A case is (prec, (B, H, W,
# Cin, Cout, stride), RES, fused_hreuse, family): RES 1 a full-size residual, 2 one sampled every other pixel, 3 the fused
# 1x1 shortcut of a 64-channel input.  The float32 modes are held to a composed tolerance (fused_tol), the float16 mode to
# the interval criterion with fused16_E.

PREC_CODE = {"f32": 0, "f16": 1, "f32s": 2, "f32x3": 3}
FUSED_CASES = [
    ("f32", (1, 9, 20, 64, 128, 1), 1, 1, 4), ("f32", (1, 13, 17, 64, 256, 2), 2, 1, 4),
    ("f32", (2, 10, 12, 64, 256, 1), 3, 1, 4), ("f32", (1, 1, 1, 64, 256, 1), 3, 1, 4),
    ("f32s", (1, 9, 20, 64, 128, 1), 1, 1, 4), ("f32s", (1, 13, 17, 128, 256, 2), 2, 1, 4),
    ("f32s", (2, 10, 12, 64, 256, 1), 3, 1, 4), ("f32s", (1, 1, 1, 64, 128, 1), 1, 1, 4),
    ("f32x3", (1, 9, 20, 64, 64, 1), 1, 1, 5), ("f32x3", (1, 13, 17, 128, 128, 2), 2, 1, 5),
    ("f32x3", (2, 10, 12, 64, 256, 1), 1, 1, 5), ("f32x3", (1, 1, 1, 64, 64, 1), 1, 1, 5),
    ("f16", (1, 9, 20, 64, 64, 1), 1, 1, 6),      # Cout 64: never the row-reuse kernel
    ("f16", (1, 9, 20, 64, 128, 1), 1, 0, 6),     # fused_hreuse off
    ("f16", (1, 13, 17, 64, 128, 2), 2, 1, 6), ("f16", (2, 10, 12, 64, 256, 1), 2, 1, 6),
    ("f16", (2, 10, 12, 64, 256, 1), 3, 0, 6), ("f16", (1, 10, 12, 128, 64, 1), 3, 1, 6),
    ("f16", (1, 1, 1, 64, 64, 1), 3, 1, 6),
    ("f16", (1, 9, 20, 64, 128, 1), 1, 1, 7), ("f16", (2, 10, 130, 64, 256, 1), 3, 1, 7),
    ("f16", (1, 1, 1, 64, 128, 1), 1, 1, 7), ("f16", (1, 1, 1, 64, 256, 1), 3, 1, 7),
]


def fused_id(c):
    prec, (B, h, w, cin, cout, stride), res, hreuse, fam = c
    return "%s-%dx%dx%dx%d-%d-s%d-res%d-h%d" % (prec, B, h, w, cin, cout, stride, res, hreuse)


def fused_record(c):
    prec, shape, res, hreuse, fam = c
    return (fam, res, int(prec == "f32s"), -1, -1, -1) if fam == 4 else (fam, res, -1, -1, -1, -1)


def fused_instantiation(c):
    return tuple(v for v in fused_record(c)[:3] if v != -1)


def fused_operands(shape, res_mode, opset, device):
    """float32 x, w2 [64][9 Cin], b2, w3 [Cout][64], b3, r (the residual tensor, or the shortcut's input [B,Ho,Wo,64]),
    wsc, bsc (RES 3), res_stride"""
    import torch
    B, h, w, cin, cout, stride = shape
    g = torch.Generator(device=device).manual_seed(23)

    def u(*s):
        return torch.rand(s, generator=g, device=device)

    off = 0.5 if opset == "mixed" else 0.1
    x = u(B, h, w, cin) - (0.3 if opset == "mixed" else 0.0)
    w2 = (u(64, 9 * cin) - off) * (2.0 / (9 * cin) ** 0.5)
    b2 = (u(64) - 0.5) * 0.5
    w3 = (u(cout, 64) - off) * 0.25
    b3 = u(cout) - 0.5
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    rs = 2 if res_mode == 2 else 1
    wsc = bsc = None
    if res_mode == 3:
        r = u(B, ho, wo, 64) - (0.3 if opset == "mixed" else 0.0)
        wsc, bsc = (u(cout, 64) - off) * 0.25, u(cout) - 0.5
    else:
        r = u(B, (ho - 1) * rs + 1, (wo - 1) * rs + 1, cout) - 0.5
    return x, w2, b2, w3, b3, r, wsc, bsc, rs


def _halves(w, lo_scale):
    """float16 hi = RN(w) and lo = RN((w - hi) / lo_scale) -- the P format and the f32s weights (lo_scale 1), the float16
    mode's weight pairs (lo_scale 2^-11) -- and the float64 value and magnitude they stand for"""
    hi = w.half()
    lo = ((w - hi.float()) / lo_scale).half()
    return hi, lo, hi.double() + lo_scale * lo.double(), hi.double().abs() + lo_scale * lo.double().abs()


def fused_held(prec, ops):
    """the operands as prec holds them: the launch's tensors (None where a CPU cannot make them) and the float64 values
    and magnitudes of the math"""
    import torch
    from coupe.dvsg_amd import _lib
    x, w2, b2, w3, b3, r, wsc, bsc, rs = ops
    cpu = x.device.type == "cpu"

    def tens(t):
        t = t.contiguous()
        if prec == "f16":
            return t.half(), t.half().double()
        if prec == "f32s":   # P format (cnn_device.h store4_p_pair): hi = RN(v), lo = RN(v - hi)
            return (None if cpu else f64._to_pieces(t)), _halves(t, 1.0)[2]
        return t, t.double()

    def wts(w):
        rows, K = w.shape
        if prec == "f16":   # [rows / 64][128][K]: 64 hi rows, then 64 lo rows
            hi, lo, v, a = _halves(w, LO)
            return torch.cat([hi.reshape(rows // 64, 64, K), lo.reshape(rows // 64, 64, K)], 1).contiguous(), v, a
        if prec == "f32s":  # [rows][K / 32][32 hi | 32 lo]
            hi, lo, v, a = _halves(w, 1.0)
            return torch.cat([hi.reshape(rows, K // 32, 32), lo.reshape(rows, K // 32, 32)], 2).contiguous(), v, a
        if prec == "f32x3" and not cpu:
            out = torch.empty((w.numel() * 6,), dtype=torch.uint8, device=w.device)
            _lib.call("dvsg_pack_weights_f32x3", w.data_ptr(), out.data_ptr(), rows, K, f64._stream())
            return out, w.double(), w.double().abs()
        return w.contiguous(), w.double(), w.double().abs()

    dev, val = {}, {}
    dev["x"], val["x"] = tens(x)
    dev["r"], val["r"] = tens(r)
    dev["w2"], val["w2"], val["w2a"] = wts(w2)
    dev["w3"], val["w3"], val["w3a"] = wts(w3)
    dev["b2"], dev["b3"] = b2, b3
    val["b2"], val["b3"] = b2.double(), b3.double()
    if wsc is not None:
        dev["wsc"], val["wsc"], val["wsca"] = wts(wsc)
        dev["bsc"], val["bsc"] = bsc, bsc.double()
    return dev, val


def fused_reference(val, stride, res_mode, rs):
    """float64: mid (= relu(pre2)), S2, pre3 (conv3's pre-activation) and Sr (the residual's or the shortcut's magnitude)"""
    pre2 = f64.conv64(val["x"], val["w2"], 3, stride) + val["b2"]
    S2 = f64.conv64(val["x"].abs(), val["w2a"], 3, stride) + val["b2"].abs()
    mid = pre2.clamp_min(0.0)
    if res_mode == 3:
        r = f64.conv64(val["r"], val["wsc"], 1, 1) + val["bsc"]
        Sr = f64.conv64(val["r"].abs(), val["wsca"], 1, 1) + val["bsc"].abs()
    else:
        r = val["r"][:, ::rs, ::rs]
        Sr = r.abs()
    return mid, S2, f64.conv64(mid, val["w3"], 1, 1) + val["b3"] + r, Sr


def fused_tol(prec, val, mid, S2, Sr, stride, res_mode):
    """float32 modes: bound(prec) of conv3 on S3 = conv(|mid| + B2, |w3|) + |b3| + Sr, over K = 64 -- or 128 when the
    shortcut's 64 products run in conv3's accumulators (RES 3: one chain, so tau(128) (S3 + S_sc), which is more than
    tau(64) S3 + tau(64) S_sc) -- plus conv2's bound B2 = bound(prec, 9 Cin, S2) carried through |w3|.  f32s: both GEMMs'
    dropped lo x lo products (S_drop, as in bound()); bound()'s output-rounding term of conv2 covers the intermediate,
    which that kernel keeps in LDS as pieces.  f32x3: bound()'s 2^-23 S of the dropped piece products, in both GEMMs."""
    K2 = val["w2"].shape[1]
    d14 = 2.0 ** -14
    S2_drop = f64.conv64(val["x"].abs() + d14, val["w2a"] + d14, 3, stride) if prec == "f32s" else None
    B2 = f64.bound(prec, K2, S2, S2_drop)
    S3 = f64.conv64(mid + B2, val["w3a"], 1, 1) + val["b3"].abs() + Sr
    S3_drop = None
    if prec == "f32s":
        S3_drop = f64.conv64(mid + B2 + d14, val["w3a"] + d14, 1, 1)
        if res_mode == 3:
            S3_drop = S3_drop + f64.conv64(val["r"].abs() + d14, val["wsca"] + d14, 1, 1)
    return f64.bound(prec, 128 if res_mode == 3 else 64, S3, S3_drop) + f64.conv64(B2, val["w3a"], 1, 1)


def _ulp16_t(t):
    import torch
    return torch.from_numpy(ulp16(t.cpu().numpy())).to(t.device)


def fused16_E(val, mid, S2, Sr, res_mode):
    """float16 mode: conv2's E2 = tau(9 Cin) S2; the tile goes to LDS as a float16 value (conv_fused.hip), so what conv3
    multiplies is within D = E2 + ulp16(|mid| + E2) / 2 of mid.  conv3 -- and the shortcut, in the same accumulators:
    K = 128 -- adds tau(K3) S3 with S3 = conv(|mid| + D, |w3|) + |b3| + Sr, and D is carried through |w3|.  Nothing else
    is rounded to float16 before the output: the residual and the shortcut's input are float16 operands, exact in float32,
    and the shortcut's result stays in the float32 accumulators."""
    E2 = tau(val["w2"].shape[1]) * S2
    D = E2 + 0.5 * _ulp16_t(mid + E2)
    S3 = f64.conv64(mid + D, val["w3a"], 1, 1) + val["b3"].abs() + Sr
    return tau(128 if res_mode == 3 else 64) * S3 + f64.conv64(D, val["w3a"], 1, 1)


# float16 fused: the intermediate's rounding makes D up to 2^-12 |mid|, carried through |w3| as a worst case, so
# 2 E / ulp16(y) ~ 2^-12 S3 / (2^-11.5 |y|) ~ 0.7 S3 / |y| and most outputs admit two float16 values: the interval is
# about one output ulp wide, still far below the 60 ulps the older tensor-wide norms allowed.  The lowest single-valued
# fractions over the FUSED_CASES with at least FUSED16_MIN_OUT outputs, measured on the MI355X (FUSED16_MEASURED; a CPU
# simulation of 5 x 6 pixels had estimated 0.088 / 0.118); the floors are 0.8 x those.  A one-pixel frame's 64-256
# outputs hold a handful of single-valued ones (measured 1 of 64): its cases print the fraction and leave the floor to
# the many-pixel cases of the same kernel.
FUSED16_MEASURED = {"pos": 0.068, "mixed": 0.086}
FUSED16_FLOOR = {k: 0.8 * v for k, v in FUSED16_MEASURED.items()}
FUSED16_MIN_OUT = 1024


def test_fused_bounds_flag_a_dropped_tile_a_wrong_shortcut_row_and_a_dropped_bias():
    """No GPU: for every precision and residual kind of FUSED_CASES, the fused reference passes its own bound (float32
    modes) or interval (float16, with the intermediate rounded to float16 as the kernel does), and fails when one pixel's
    intermediate row is dropped, when the shortcut uses its neighbour's weight row and when a conv3 bias is dropped."""
    import torch
    seen = set()
    for prec, (B, h, w, cin, cout, stride), res_mode, _, _ in FUSED_CASES:
        for opset in ("pos", "mixed"):
            key = (prec, cin, res_mode, opset)
            if key in seen:
                continue
            seen.add(key)
            stride = stride if res_mode != 3 else 1
            ops = fused_operands((1, 5, 6, cin, min(cout, 128), stride), res_mode, opset, "cpu")
            rs = ops[-1]
            _, val = fused_held(prec, ops)
            mid, S2, pre3, Sr = fused_reference(val, stride, res_mode, rs)
            mid_dev = torch.from_numpy(rn16(mid.numpy())) if prec == "f16" else mid

            def y_of(m, b3=val["b3"], wsc=val.get("wsc")):
                if res_mode == 3:
                    r = f64.conv64(val["r"], wsc, 1, 1) + val["bsc"]
                else:
                    r = val["r"][:, ::rs, ::rs]
                return (f64.conv64(m, val["w3"], 1, 1) + b3 + r).clamp_min(0.0)

            m2 = mid_dev.clone()
            m2[0, 1, 1] = 0.0
            b3 = val["b3"].clone()
            b3[int(val["b3"].abs().argmax())] = 0.0
            bads = [("intermediate row dropped", y_of(m2)), ("conv3 bias dropped", y_of(mid_dev, b3=b3))]
            if res_mode == 3:
                wsc = val["wsc"].clone()   # in the channel the ReLU clamps least
                n = int((pre3 > 0).reshape(-1, pre3.shape[-1]).sum(0).argmax())
                wsc[n] = val["wsc"][(n + 1) % wsc.shape[0]]
                bads.append(("shortcut weight row", y_of(mid_dev, wsc=wsc)))
            if prec == "f16":
                E = fused16_E(val, mid, S2, Sr, res_mode).numpy()
                assert check16(rn16(y_of(mid_dev).numpy()), pre3.numpy(), E, True)[0] == 0, key
                single = check16(rn16(pre3.clamp_min(0.0).numpy()), pre3.numpy(), E, True)[2]
                assert single >= FUSED16_FLOOR[opset], (key, single)
                for name, bad in bads:
                    assert check16(rn16(bad.numpy()), pre3.numpy(), E, True)[0] > 0, (key, name)
            else:
                tol = fused_tol(prec, val, mid, S2, Sr, stride, res_mode)
                ref = pre3.clamp_min(0.0)
                assert f64.excess(y_of(mid_dev), ref, tol)[0] == 0, key
                for name, bad in bads:
                    assert f64.excess(bad, ref, tol)[0] > 0, (key, name)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the two files' tables cover every conv kernel instantiation the library holds

_KERNEL = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+(conv[a-z0-9_]*?_kernel)I((?:DF16_|f|L[ib]\d+E)+)EEvN")
_ARG = re.compile(rb"DF16_|f|L[ib](\d+)E")
FAMILIES = ("conv_gemm_kernel", "conv_wide16_kernel", "conv_wide16a_kernel", "conv_wide16h_kernel", "conv3x3_1x1_kernel",
            "conv3x3_1x1_x3_kernel", "conv3x3_1x1_f16_kernel", "conv3x3_1x1_f16h_kernel")
# instantiations per family when this was written; conv_gemm_kernel as (0, T): float32 tensors, float16 tensors
MIN_COUNTS = {(0, 0): 168, (0, 1): 104, 1: 24, 2: 24, 3: 12, 4: 6, 5: 2, 6: 3, 7: 2}


def conv_kernel_instantiations():
    """coverage keys of every conv kernel in the built library: (family, template arguments ...), conv_gemm_kernel's T as
    0 (float) or 1 (_Float16, mangled DF16_)"""
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    found = set()
    for name, args in _KERNEL.findall(data):
        if name.decode() not in FAMILIES:   # conv1's and the other layers' kernels
            continue
        vals = tuple(1 if a.group(0) == b"DF16_" else 0 if a.group(0) == b"f" else int(a.group(1)) for a in _ARG.finditer(args))
        found.add((FAMILIES.index(name.decode()),) + vals)
    return found


def test_tables_cover_every_conv_kernel_instantiation():
    """All eight conv kernel families as the built library names them: an instantiation without a case in this file's
    tables or in test_conv_gemm_f64.py's fails here, and so does a build that has lost instantiations."""
    found = conv_kernel_instantiations()
    counts = {}
    for k in found:
        fam = (0, k[1]) if k[0] == 0 else k[0]
        counts[fam] = counts.get(fam, 0) + 1
    for fam, n in MIN_COUNTS.items():
        assert counts.get(fam, 0) >= n, (fam, counts.get(fam, 0), n)
    covered = {instantiation(c) for c in CASES} | {fused_instantiation(c) for c in FUSED_CASES}
    covered |= {(0,) + f64.instantiation(f64.expected_record(c)) for c in f64.CASES}
    missing = sorted(found - covered)
    assert not missing, "instantiations without a case: %s" % missing
    assert covered <= found, sorted(covered - found)


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def last_kernel():
    from coupe.dvsg_amd import _lib
    f = (ctypes.c_int * KERNEL_FIELDS)()
    _lib.call("dvsg_debug_last_conv_kernel", f, KERNEL_FIELDS)
    return tuple(f)


def _set_options(opts):
    from coupe.dvsg_amd import _lib
    for k, v in opts.items():
        _lib.call("dvsg_debug_set_option", k.encode(), v)


def run16(mode, shape, relu, res_mode, sbytes, opset, seed=11):
    """One dvsg_conv_gemm_f16 / _f16s launch twice between sentinels; returns y, pre and E as float64 NumPy arrays and the
    launch records, after checking the sentinels, the inputs' bytes and that the two launches agree bit for bit."""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    B, H, W, cin, cout, ks, stride = shape
    K = ks * ks * cin
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, w64, wabs, wdev, hi, lo, bias, res, rs = make16(shape, res_mode, opset, seed, dev, mode == "f16s")
    ins = {"x": f64.Guarded.of(x), "wt": f64.Guarded.of(wdev), "bias": f64.Guarded.of(bias)}
    if res is not None:
        ins["res"] = f64.Guarded.of(res)
    before = {k: g.body.clone() for k, g in ins.items()}
    fn = "dvsg_conv_gemm_f16s" if mode == "f16s" else "dvsg_conv_gemm_f16"
    ys, recs = [], []
    for _ in range(2):
        y = f64.Guarded(B * ho * wo * cout * 2, dev)
        sc = f64.Guarded(sbytes, dev) if sbytes else None
        _lib.call(fn, ins["x"].ptr(), ins["wt"].ptr(), ins["bias"].ptr(), ins["res"].ptr() if res is not None else 0,
                  y.ptr(), B, H, W, cin, cout, ks, stride, relu, rs, sc.ptr() if sc else 0, sbytes, f64._stream())
        recs.append((f64.last_config(), last_kernel()))
        torch.cuda.synchronize()
        assert y.intact(), "output sentinels overwritten"
        assert sc is None or sc.intact(), "scratch sentinels overwritten"
        ys.append(y)
    for k, g in ins.items():
        assert g.intact() and torch.equal(g.body, before[k]), "input %s changed" % k
    assert torch.equal(ys[0].body, ys[1].body), "two launches differ"
    assert recs[0] == recs[1]
    pre, S = reference16(x, w64, wabs, bias, res, ks, stride, rs)
    y = ys[0].view(torch.float16, (B, ho, wo, cout)).double()
    return y.cpu().numpy(), pre.cpu().numpy(), (tau(K) * S).cpu().numpy(), recs[0]


def _check_records(case, rec):
    want_cfg, want_ker = expected_records(case)
    cfg, ker = rec
    assert ker == want_ker, "launch record %s, expected %s" % (ker, want_ker)
    if want_cfg is None:
        assert cfg[0] == -1, cfg
    else:
        assert cfg == want_cfg, "conv config %s, expected %s" % (dict(zip(f64.FIELDS, cfg)), dict(zip(f64.FIELDS, want_cfg)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_f16_layer_configuration_against_float64(case):
    """One configuration, both operand sets: the launch records name exactly the expected kernel, every output element is
    a correctly rounded value within the accumulation error of the float64 result, the single-valued fraction meets its
    floor, nothing outside y and the stated scratch is written, the inputs keep their bytes, two launches agree."""
    mode, shape, scratch, opts, exp, relu, res = case
    K = shape[5] ** 2 * shape[3]
    try:
        _set_options(opts)
        for opset in ("mixed", "pos"):
            y, pre, E, rec = run16(mode, shape, relu, res, scratch_bytes(scratch, mode, shape), opset)
            _check_records(case, rec)
            nbad, worst, single = check16(y, pre, E, relu)
            print("%s %s: worst |y - ref| / (E + ulp/2) = %.3f; single-valued %.3f (floor %.3f)"
                  % (case_id(case), opset, worst, single, single_floor(opset, K)))
            assert nbad == 0, "%s: %d elements outside their interval (worst %.3g)" % (opset, nbad, worst)
            assert single >= single_floor(opset, K), (opset, single)
    finally:
        _set_options(DEFAULTS)


RANGE_CASES = [c for c in CASES if c[5:] == (1, 1) and (c[1], c[4]) in
               {((1, 3, 43, 64, 64, 1, 1), ("g", 128, 2, 2, 0, 1, 0, 0)), ((1, 14, 40, 64, 128, 3, 1), ("w", 3, 1)),
                ((1, 16, 20, 256, 128, 1, 1), ("w", 2, 1)), ((1, 514, 514, 64, 128, 3, 2), ("g", 128, 2, 4, 0, 1, 0, 0))}]


@pytest.mark.gpu
@pytest.mark.parametrize("opset", ["tiny", "large", "overflow"])
@pytest.mark.parametrize("case", RANGE_CASES, ids=[case_id(c) for c in RANGE_CASES])
def test_f16_operand_ranges(case, opset):
    """Float16-subnormal activations with subnormal outputs (the matrix cores keep subnormal inputs), outputs near 6e4,
    and true outputs past float16's range, which must come out as +inf (RN16), not saturated at 65504."""
    mode, shape, scratch, opts, exp, relu, res = case
    relu = 0 if opset == "overflow" else relu
    try:
        _set_options(opts)
        y, pre, E, rec = run16(mode, shape, relu, res, scratch_bytes(scratch, mode, shape), opset)
    finally:
        _set_options(DEFAULTS)
    nbad, worst, single = check16(y, pre, E, relu)
    lo, hi = interval16(pre, E, relu)
    fin = y[np.isfinite(y)]
    print("%s %s: max finite |y| %.4g, %.1f %% subnormal outputs, %d inf; worst %.3f; single-valued %.3f"
          % (case_id(case), opset, float(np.abs(fin).max()) if fin.size else 0.0,
             100.0 * float((np.abs(y) < 2.0 ** -14).mean()), int(np.isinf(y).sum()), worst, single))
    if opset == "tiny":
        assert float((np.abs(pre) < 2.0 ** -14).mean()) > 0.99
    elif opset == "large":
        assert 3e4 < float(np.abs(pre).max()) < 65504
    else:
        assert float(np.isinf(lo).mean()) > 0.5
    assert nbad == 0, "%s: %d elements outside their interval (worst %.3g)" % (opset, nbad, worst)
    assert single >= single_floor(opset, 64), single


@pytest.mark.gpu
@pytest.mark.parametrize("case", FUSED_CASES, ids=[fused_id(c) for c in FUSED_CASES])
def test_fused_kernel_against_float64(case):
    """One fused launch of one precision and residual kind, both operand sets, twice: the launch record names the kernel,
    every element meets its bound (float32 modes) or interval (float16), the sentinels around the output and every input
    are intact, the inputs keep their bytes and the two launches agree bit for bit."""
    import torch
    from coupe.dvsg_amd import _lib
    prec, shape, res_mode, hreuse, fam = case
    B, h, w, cin, cout, stride = shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    cuda = torch.device("cuda:0")
    try:
        _set_options({"fused_hreuse": hreuse})
        for opset in ("mixed", "pos"):
            ops = fused_operands(shape, res_mode, opset, cuda)
            rs = ops[-1]
            dev, val = fused_held(prec, ops)
            ins = {k: f64.Guarded.of(t) for k, t in dev.items()}
            before = {k: g.body.clone() for k, g in ins.items()}
            sc = res_mode == 3
            ys, recs = [], []
            for _ in range(2):
                y = f64.Guarded(B * ho * wo * cout * (2 if prec == "f16" else 4), cuda)
                _lib.call("dvsg_debug_conv3x3_1x1", PREC_CODE[prec], ins["x"].ptr(), ins["w2"].ptr(), ins["b2"].ptr(),
                          ins["w3"].ptr(), ins["b3"].ptr(), 0 if sc else ins["r"].ptr(), ins["r"].ptr() if sc else 0,
                          ins["wsc"].ptr() if sc else 0, ins["bsc"].ptr() if sc else 0, 64 if sc else 0, y.ptr(),
                          B, h, w, cin, cout, stride, rs, f64._stream())
                recs.append(last_kernel())
                torch.cuda.synchronize()
                assert y.intact(), "output sentinels overwritten"
                ys.append(y)
            for k, g in ins.items():
                assert g.intact() and torch.equal(g.body, before[k]), "input %s changed" % k
            assert torch.equal(ys[0].body, ys[1].body), "two launches differ"
            assert recs[0] == recs[1] == fused_record(case), (recs[0], fused_record(case))
            mid, S2, pre3, Sr = fused_reference(val, stride, res_mode, rs)
            if prec == "f16":
                yv = ys[0].view(torch.float16, (B, ho, wo, cout)).double().cpu().numpy()
                E = fused16_E(val, mid, S2, Sr, res_mode).cpu().numpy()
                nbad, worst, single = check16(yv, pre3.cpu().numpy(), E, True)
                print("%s %s: worst |y - ref| / (E + ulp/2) = %.3f; single-valued %.3f (floor %.2f)"
                      % (fused_id(case), opset, worst, single, FUSED16_FLOOR[opset]))
                assert nbad == 0, "%s: %d elements outside their interval (worst %.3g)" % (opset, nbad, worst)
                if yv.size >= FUSED16_MIN_OUT:
                    assert single >= FUSED16_FLOOR[opset], single
            else:
                yv = (f64._from_pieces(ys[0].body, (B, ho, wo, cout)) if prec == "f32s"
                      else ys[0].view(torch.float32, (B, ho, wo, cout)))
                nbad, worst = f64.excess(yv, pre3.clamp_min(0.0), fused_tol(prec, val, mid, S2, Sr, stride, res_mode))
                print("%s %s: worst %.3f of the bound" % (fused_id(case), opset, worst))
                assert nbad == 0, "%s: %d elements out of bounds (worst %.3g)" % (opset, nbad, worst)
    finally:
        _set_options(DEFAULTS)
