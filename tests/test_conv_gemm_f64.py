"""The float32-tensor conv GEMMs pinned to float64, element by element.

Every instantiation of conv_gemm_kernel on float32 tensors -- the exact path, "f32s" (float16 pieces) and "f32x3"
(bfloat16 pieces) -- is launched on purpose by a case of CASES, which names the configuration it expects; the launch
record (dvsg_debug_last_conv_config) must report exactly that, and a CPU test checks that the table covers every
instantiation the built library contains.  Each output element is held to its own float64 bound

    |y - ref| <= tau(K) S + (the mode's dropped cross products and output rounding) + K 2^-126,
    tau(K) = 2^-24 (C_SQRT sqrt(K) + C_ONE),

S = conv(|x|, |w|) + |b| + |r| being the element's own magnitude scale, and a CPU test shows that every bound used here
flags a dropped K stage, a dropped bias and a neighbour's residual.  Outputs, scratch, inputs and network workspaces sit
between NaN sentinels: nothing may be written outside them or change an input.
"""
import ctypes
import math
import re

import pytest

# tau(K) = 2^-24 (C_SQRT sqrt(K) + C_ONE)
C_SQRT, C_ONE = 1.0, 4.0
TINY = 2.0 ** -126          # per product: a subnormal product kept or flushed
GUARD = 64 << 10            # sentinel bytes on each side of every buffer
SENTINEL = 0xFF             # 0xFFFFFFFF / 0xFFFF: NaN as float32 and float16, so a stray read shows in the outputs
MIB = 1 << 20
SCRATCH = {"none": 0, "4M": 4 * MIB, "17M": 17 * MIB, "65M": 65 * MIB}
FIELDS = ("T", "BN", "WM", "WN", "KS", "RELU", "RES", "MODE", "SPLIT", "X3", "ksplit", "streamk_tail", "mt_fast")


def tau(K):
    return 2.0 ** -24 * (C_SQRT * math.sqrt(K) + C_ONE)


def bound(prec, K, S, S_drop=None):
    """Per-element bound on |y - ref| for a layer of depth K in precision `prec`, on the operands as the mode holds them.
    f32x3: the dropped a2 w3 + a3 w2 + a3 w3 are <= 2^-23 |a w| (|p2| <= 2^-8, |p3| <= 2^-16 of the operand: conv_gemm_tile.h
    X3).  f32s: the dropped a2 w2 with |p2| <= 2^-11 (|v| + 2^-14) (hi = f16(v) rounded to nearest, a subnormal hi below
    2^-14: cnn_device.h P format) -- S_drop = conv(|x| + 2^-14, |w| + 2^-14) -- and the output stored as hi + lo, lo
    rounded: 2^-22 |y| + 2^-25."""
    b = tau(K) * S + K * TINY
    if prec == "f32x3":
        b = b + 2.0 ** -23 * S
    elif prec == "f32s":
        b = b + 1.001 * 2.0 ** -22 * S_drop + 2.0 ** -22 * S + 2.0 ** -25
    return b


def conv64(x, w, k, stride):
    """NHWC float64 x [B,H,W,Cin], w [Cout][k*k*Cin] (kh, kw, c) -> [B,Ho,Wo,Cout], pad k // 2 (conv2d_same for 3x3)."""
    import torch
    cout = w.shape[0]
    w4 = w.reshape(cout, k, k, -1).permute(0, 3, 1, 2)
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w4, stride=stride, padding=k // 2).permute(0, 2, 3, 1)


def reference(x, w, bias, res, k, stride, res_stride, relu):
    """float64 ref and S for float64 operands; res is the full residual tensor (sampled every res_stride) or None."""
    ref = conv64(x, w, k, stride) + bias
    S = conv64(x.abs(), w.abs(), k, stride) + bias.abs()
    if res is not None:
        r = res[:, ::res_stride, ::res_stride]
        ref = ref + r
        S = S + r.abs()
    if relu:
        ref = ref.clamp_min(0.0)
    return ref, S


def excess(y, ref, tol):
    """max (|y - ref| - tol) (> 0: out of bounds; NaN counts as out) and the worst |y - ref| / tol."""
    import torch
    d = (y.double() - ref).abs()
    bad = ~(d <= tol)
    return int(bad.sum()), float((d / tol).max()) if not bool(torch.isnan(d).any()) else float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# The configuration matrix.  A shape is (B, H, W, Cin, Cout, ksize, stride); `exp` is (BN, WM, WN, MODE, ksplit,
# streamk_tail, mt_fast) -- the rest of the record (T, KS, RELU, RES, SPLIT, X3) follows from the case.  Every base row runs
# at relu 0 / 1 x residual modes 0 / 1 / 2 (mode 2: res_stride 2, a larger tensor sampled every other pixel), except the
# stream-K rows, which never carry a residual (launch_cfg) and run at relu 0 / 1.

SMALL_129 = (1, 3, 43, 32, 64, 1)       # M = 129: a full and a one-row M tile; Cin 32: one K stage per tap; one N tile
BIG_EXACT = (1, 511, 511, 32, 128, 2)   # stride 2, odd: 256 x 256 = 65536 pixels, exactly 512 128-wide tiles
BIG_OVER = (1, 514, 514, 32, 128, 2)    # stride 2, even: 257 x 257 -> 517 128-wide tiles
SPLITK_1 = (2, 17, 15, 1024, 128, 2)    # 1x1 stride 2, odd: 2 x 9 x 8 = 144 pixels, 4 tiles, K = 1024
SPLITK_3 = (1, 20, 28, 128, 64, 1)      # 3x3, K = 1152 (36 stages), 5 tiles
STREAMK_1 = (1, 64, 128, 1024, 512, 1)  # 8192 pixels: 256 wide tiles, one stream-K round, K = 1024
STREAMK_1L = (1, 64, 128, 4096, 512, 1)  # the same with K = 4096: the f32s / f32x3 stream-K threshold, mt_fast
STREAMK_3 = (1, 64, 128, 512, 512, 1)   # 3x3 512 -> 512, K = 4608: one stream-K round, mt_fast
SPLIT_FB = (1, 128, 128, 128, 64, 1)    # 3x3, 128 tiles: split-K 4 ways wants 16 MiB of slabs
ODD_96 = (1, 16, 8, 96, 64, 1)          # Cin 96 (a K stage straddles two 3x3 taps), M = 128: exactly one M tile


def _shape(base, ks):
    B, H, W, cin, cout, stride = base
    return (B, H, W, cin, cout, ks, stride)


BASE = []   # (prec, shape, scratch, variant, exp, combos)
ALL6 = [(r, m) for r in (0, 1) for m in (0, 1, 2)]
NORES = [(0, 0), (1, 0)]
for ks in (1, 3):
    # exact float32
    BASE += [("f32", _shape(SMALL_129, ks), "none", 0, (64, 2, 2, 0, 1, 0, 0), ALL6),
             ("f32", _shape(ODD_96, ks), "none", 2, (64, 4, 2, 0, 1, 0, 0), ALL6),
             ("f32", _shape(BIG_EXACT, ks), "17M", 0, (128, 2, 2, 0, 1, 0, 0), ALL6),
             ("f32", _shape(BIG_OVER, ks), "none", 0, (128, 2, 4, 0, 1, 0, 0), ALL6),
             ("f32", _shape(SPLITK_1 if ks == 1 else SPLITK_3, ks), "17M", 0, (64, 2, 2, 1, 8, 0, 0), ALL6),
             ("f32", _shape(STREAMK_1 if ks == 1 else STREAMK_3, ks), "65M", 0,
              (128, 2, 4, 2, 1, 256, 0 if ks == 1 else 1), NORES)]
    # f32s: the fat 4-wave tiles unless a variant asks for 8 waves
    BASE += [("f32s", _shape(SMALL_129, ks), "none", 0, (64, 2, 2, 0, 1, 0, 0), ALL6),
             ("f32s", _shape(ODD_96, ks), "none", 4, (64, 4, 2, 0, 1, 0, 0), ALL6),
             ("f32s", _shape(BIG_OVER, ks), "none", 0, (128, 2, 2, 0, 1, 0, 0), ALL6),
             ("f32s", _shape(BIG_EXACT, ks), "none", 2, (128, 2, 4, 0, 1, 0, 0), ALL6),
             ("f32s", _shape(SPLITK_1 if ks == 1 else SPLITK_3, ks), "17M", 0, (64, 2, 2, 1, 8, 0, 0), ALL6),
             ("f32s", _shape(STREAMK_1L if ks == 1 else STREAMK_3, ks), "65M", 0, (128, 2, 4, 2, 1, 256, 1), NORES)]
    # f32x3: 4 waves of 64-wide wave tiles
    BASE += [("f32x3", _shape(SMALL_129, ks), "none", 0, (64, 4, 1, 0, 1, 0, 0), ALL6),
             ("f32x3", _shape(BIG_OVER, ks), "none", 0, (128, 2, 2, 0, 1, 0, 0), ALL6),
             ("f32x3", _shape(SPLITK_1 if ks == 1 else SPLITK_3, ks), "17M", 0, (64, 4, 1, 1, 8, 0, 0), ALL6),
             ("f32x3", _shape(STREAMK_1L if ks == 1 else STREAMK_3, ks), "65M", 0, (128, 2, 2, 2, 1, 256, 1), NORES)]

# edges and the diagnostic variants, one combination each
EXTRA = [
    # scratch of 4 MiB: split-K does not fit and falls back to plain tiles; exactly 17 MiB: it runs
    ("f32", _shape(SPLIT_FB, 3), "4M", 0, (64, 2, 2, 0, 1, 0, 0), [(1, 1)]),
    ("f32", _shape(SPLIT_FB, 3), "17M", 0, (64, 2, 2, 1, 4, 0, 0), [(1, 1)]),
    ("f32x3", _shape(SPLIT_FB, 3), "4M", 0, (64, 4, 1, 0, 1, 0, 0), [(0, 2)]),
    # M = 1 (1x1 and 3x3), M = 128 at stride 2 from an odd frame
    ("f32", (1, 1, 1, 32, 64, 1, 1), "65M", 0, (64, 2, 2, 0, 1, 0, 0), [(1, 1)]),
    ("f32", (1, 1, 1, 96, 128, 3, 1), "none", 0, (64, 2, 2, 0, 1, 0, 0), [(0, 2)]),
    ("f32s", (1, 1, 1, 32, 64, 3, 1), "17M", 0, (64, 2, 2, 0, 1, 0, 0), [(1, 2)]),
    ("f32x3", (1, 1, 1, 64, 64, 1, 1), "none", 0, (64, 4, 1, 0, 1, 0, 0), [(0, 1)]),
    ("f32", (1, 31, 15, 32, 64, 3, 2), "none", 0, (64, 2, 2, 0, 1, 0, 0), [(1, 2)]),
    ("f32", (2, 16, 14, 96, 64, 1, 2), "none", 0, (64, 2, 2, 0, 1, 0, 0), [(0, 1)]),
    # split-K at M = 1: two slices of one tile
    ("f32", (1, 1, 1, 1024, 64, 1, 1), "17M", 0, (64, 2, 2, 1, 8, 0, 0), [(1, 1)]),
    # the A/B variants: 4 waves, 8 waves, no split-K, 64-wide tiles only, no stream-K tail
    ("f32", _shape(BIG_OVER, 1), "none", 1, (128, 2, 2, 0, 1, 0, 0), [(1, 0)]),
    ("f32", _shape(BIG_EXACT, 3), "none", 2, (128, 2, 4, 0, 1, 0, 0), [(0, 0)]),
    ("f32", _shape(SPLITK_3, 3), "17M", 3, (64, 4, 2, 0, 1, 0, 0), [(1, 1)]),
    ("f32", _shape(BIG_OVER, 3), "none", 4, (64, 4, 2, 0, 1, 0, 0), [(1, 1)]),
    ("f32", _shape(STREAMK_1, 1), "65M", 6, (64, 2, 2, 0, 1, 0, 0), [(1, 0)]),
    ("f32s", _shape(SPLITK_1, 1), "17M", 3, (64, 4, 2, 0, 1, 0, 0), [(0, 0)]),
    ("f32x3", _shape(STREAMK_3, 3), "65M", 6, (64, 4, 1, 0, 1, 0, 0), [(1, 0)]),
]

CASES = [(prec, shape, scratch, variant, exp, relu, res)
         for prec, shape, scratch, variant, exp, combos in BASE + EXTRA for relu, res in combos]


def case_id(c):
    prec, (B, H, W, cin, cout, ks, stride), scratch, variant, exp, relu, res = c
    return "%s-k%ds%d-%dx%dx%dx%d-%d-%s-v%d-r%d-res%d" % (prec, ks, stride, B, H, W, cin, cout, scratch, variant, relu, res)


def expected_record(c):
    prec, (B, H, W, cin, cout, ks, stride), scratch, variant, exp, relu, res = c
    BN, WM, WN, MODE, ksplit, tail, mt_fast = exp
    return (0, BN, WM, WN, ks, relu, res, MODE, int(prec == "f32s"), int(prec == "f32x3"), ksplit, tail, mt_fast)


def instantiation(rec):
    """(T, BN, WM, WN, KS, RELU, RES, MODE, SPLIT, X3) of a launch record"""
    return tuple(rec[:10])


# ---------------------------------------------------------------------------------------------------------------------
# operands (the same generator on the GPU and, for the sharpness test, on the CPU)

def make_operands(shape, res_mode, seed, device, ascale=1.0, wscale=1.0):
    import torch
    B, H, W, cin, cout, ks, stride = shape
    K = ks * ks * cin
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator(device=device).manual_seed(seed)
    x = (torch.rand((B, H, W, cin), generator=g, device=device) * 4.0 - 1.0) * ascale
    wt = (torch.rand((cout, K), generator=g, device=device) - 0.5) * (2.0 / K ** 0.5) * wscale
    bias = (torch.rand((cout,), generator=g, device=device) - 0.5) * ascale * wscale
    res, rs = None, 1
    if res_mode:
        rs = 1 if res_mode == 1 else 2
        res = (torch.rand((B, (ho - 1) * rs + 1, (wo - 1) * rs + 1, cout), generator=g, device=device) - 0.5) * ascale * wscale
    return x, wt, bias, res, rs


# ---------------------------------------------------------------------------------------------------------------------
# CPU: every bound used in this file is sharp

def _perturbations(x, w, bias, res, k, stride, rs, relu):
    """ref and three wrong answers: one K stage (32 consecutive k) out of one element, one channel's bias out, one pixel's
    residual taken from its neighbour."""
    import torch
    ref, S = reference(x, w, bias, res, k, stride, rs, relu)
    pre, _ = reference(x, w, bias, res, k, stride, rs, False)
    B, Ho, Wo, cout = ref.shape
    cin = x.shape[3]
    K = w.shape[1]
    # the stage's products for pixel (0, ho, wo), channel n: im2col row of that pixel
    xp = torch.nn.functional.pad(x, (0, 0, k // 2, k // 2, k // 2, k // 2))
    ho, wo = Ho // 2, Wo // 2
    patch = xp[0, ho * stride:ho * stride + k, wo * stride:wo * stride + k, :].reshape(-1)
    st = (K // 32) // 2
    prods = patch[st * 32:st * 32 + 32].unsqueeze(0) * w[:, st * 32:st * 32 + 32]
    stage = prods.sum(1)                                      # [cout]
    ok = (pre[0, ho, wo] > 0) & (pre[0, ho, wo] - stage > 0) if relu else torch.ones_like(stage, dtype=torch.bool)
    n = int(torch.nonzero(ok)[0])
    drop_k = ref.clone()
    v = pre[0, ho, wo, n] - stage[n]
    drop_k[0, ho, wo, n] = v.clamp_min(0.0) if relu else v
    drop_b = ref.clone()
    nb = int(bias.abs().argmax())
    v = pre[..., nb] - bias[nb]
    drop_b[..., nb] = v.clamp_min(0.0) if relu else v
    out = [("K stage", drop_k), ("bias", drop_b)]
    if res is not None:
        r = res[:, ::rs, ::rs]
        nbr = pre.clone()
        nbr[0, 0, 0] = pre[0, 0, 0] - r[0, 0, 0] + (r[0, 0, 1] if Wo > 1 else r[0, 1, 0])
        out.append(("residual", nbr.clamp_min(0.0) if relu else nbr))
    return ref, S, out


def _small_spatial(shape):
    """the CPU stand-in of a GPU case: same K, channels, stride and kernel, a few pixels"""
    B, H, W, cin, cout, ks, stride = shape
    return (1, 5, 6, cin, min(cout, 128), ks, stride)


def _bound_for(prec, K, x, w, bias, res, k, stride, rs, S):
    S_drop = None
    if prec == "f32s":
        S_drop = conv64(x.abs() + 2.0 ** -14, w.abs() + 2.0 ** -14, k, stride)
    return bound(prec, K, S, S_drop)


def test_bounds_flag_a_dropped_k_stage_a_dropped_bias_and_a_neighbours_residual():
    """No GPU: applied to the float64 ref itself after three perturbations, every bound this file uses flags each one --
    at every (precision, K) of the matrix, at the largest K (4608), for the fused kernel's composed bound and for the
    tiny-operand case at their own K."""
    import torch
    seen = set()
    for c in CASES:
        prec, shape = c[0], c[1]
        K = shape[5] ** 2 * shape[3]
        if (prec, K, shape[6]) in seen:
            continue
        seen.add((prec, K, shape[6]))
        s = _small_spatial(shape)
        x, w, bias, res, rs = (t.double() if isinstance(t, torch.Tensor) else t for t in make_operands(s, 1, 7, "cpu"))
        ref, S, perts = _perturbations(x, w, bias, res, s[5], s[6], rs, True)
        tol = _bound_for(prec, K, x, w, bias, res, s[5], s[6], rs, S)
        assert excess(ref, ref, tol)[0] == 0
        for name, bad in perts:
            assert excess(bad, ref, tol)[0] > 0, (prec, K, name)
    assert max(k for _, k, _ in seen) == 4608
    # the tiny-operand case
    x, w, bias, res, rs = (t.double() if isinstance(t, torch.Tensor) else t for t in _tiny_operands("cpu"))
    ref, S, perts = _perturbations(x, w, bias, res, 1, 1, rs, False)
    tol = bound("f32", 32, S)
    assert excess(ref, ref, tol)[0] == 0
    for name, bad in perts:
        assert excess(bad, ref, tol)[0] > 0, ("tiny", name)
    # the fused kernel's composed bound: each perturbation in conv3's stage, bias, residual, and in conv2's
    for B, h, w_, cin, cout, stride, res_stride in FUSED:
        ops = [t.double() if isinstance(t, torch.Tensor) else t for t in _fused_operands((1, 5, 6, cin, cout, stride, res_stride), "cpu")]
        x, w2, b2, w3, b3, res = ops
        mid, S2 = reference(x, w2, b2, None, 3, stride, 1, True)
        ref, S3, perts = _perturbations(mid, w3, b3, res, 1, 1, res_stride, True)
        tol = fused_bound(cin, S2, S3, w3)
        assert excess(ref, ref, tol)[0] == 0
        for name, bad in perts:
            assert excess(bad, ref, tol)[0] > 0, ("fused", cin, name)
        _, _, perts2 = _perturbations(x, w2, b2, None, 3, stride, 1, True)
        for name, bad_mid in perts2:
            bad = torch.relu(conv64(bad_mid, w3, 1, 1) + b3 + res[:, ::res_stride, ::res_stride])
            assert excess(bad, ref, tol)[0] > 0, ("fused conv2", cin, name)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the table covers every float32-tensor instantiation the library holds

_MANGLED = re.compile(rb"_ZN4dvsg12_GLOBAL__N_116conv_gemm_kernelIfLi(\d+)ELi(\d+)ELi(\d+)ELi(\d)ELb([01])ELi(\d)ELi(\d)"
                      rb"ELb([01])ELb([01])EEEvNS_\d+ConvGemmDevE")


def library_instantiations():
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    return {(0,) + tuple(int(v) for v in m) for m in _MANGLED.findall(data)}


def test_matrix_covers_every_float32_instantiation():
    """conv_gemm_kernel<float, BN, WM, WN, KS, RELU, RES, MODE, SPLIT, X3> as the built library names them (exact, f32s and
    f32x3): a new instantiation without a case in CASES fails here."""
    found = library_instantiations()
    assert len(found) >= 168, len(found)   # 64 exact + 64 f32s + 40 f32x3 when this was written
    covered = {instantiation(expected_record(c)) for c in CASES}
    missing = sorted(found - covered)
    assert not missing, "instantiations without a case: %s" % missing
    assert covered <= found, sorted(covered - found)


# ---------------------------------------------------------------------------------------------------------------------
# GPU helpers: buffers between sentinels

class Guarded(object):
    """`nbytes` usable bytes at a 256-byte aligned offset of a buffer with GUARD sentinel bytes on each side."""

    def __init__(self, nbytes, dev):
        import torch
        self.nbytes = nbytes
        self.flat = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        assert self.flat.data_ptr() % 256 == 0
        self.body = self.flat[GUARD:GUARD + nbytes]

    @classmethod
    def of(cls, t):
        """a guarded copy of tensor t (same dtype and shape)"""
        g = cls(t.numel() * t.element_size(), t.device)
        g.body.copy_(t.contiguous().view(-1).view(torch_uint8()))
        return g

    def ptr(self):
        return self.flat.data_ptr() + GUARD

    def view(self, dtype, shape):
        return self.body.view(dtype).view(shape)

    def intact(self):
        return bool((self.flat[:GUARD] == SENTINEL).all()) and bool((self.flat[GUARD + self.nbytes:] == SENTINEL).all())


def torch_uint8():
    import torch
    return torch.uint8


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def last_config():
    from coupe.dvsg_amd import _lib
    f = (ctypes.c_int * len(FIELDS))()
    _lib.call("dvsg_debug_last_conv_config", f, len(FIELDS))
    return tuple(f)


def _to_pieces(t):
    import torch
    from coupe.dvsg_amd import _lib
    out = torch.empty(t.numel() * 4, dtype=torch.uint8, device=t.device)
    _lib.call("dvsg_f32_to_pieces", t.data_ptr(), out.data_ptr(), t.numel(), _stream())
    return out


def _from_pieces(pcs, shape):
    import torch
    from coupe.dvsg_amd import _lib
    out = torch.empty(shape, dtype=torch.float32, device=pcs.device)
    _lib.call("dvsg_pieces_to_f32", pcs.data_ptr(), out.data_ptr(), out.numel(), _stream())
    return out


def run_layer(prec, shape, relu, res_mode, scratch_bytes, seed=11, ascale=1.0, wscale=1.0):
    """One dvsg_conv_gemm_<prec> launch twice, between sentinels; returns (y, ref, S, S_drop, record) after checking the
    sentinels, the inputs' bytes and that the two launches agree bit for bit."""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    B, H, W, cin, cout, ks, stride = shape
    K = ks * ks * cin
    ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, wt, bias, res, rs = make_operands(shape, res_mode, seed, dev, ascale, wscale)
    if prec == "f32s":   # the operands as the mode holds them: 22-bit pieces
        xs = _to_pieces(x)
        x = _from_pieces(xs, x.shape)
        hi = wt.half()
        lo = (wt - hi.float()).half()
        wdev = torch.cat([hi.reshape(cout, K // 32, 32), lo.reshape(cout, K // 32, 32)], 2).contiguous()
        w64 = hi.double() + lo.double()
        if res is not None:
            rp = _to_pieces(res)
            res = _from_pieces(rp, res.shape)
        ins = {"x": Guarded.of(xs), "wt": Guarded.of(wdev), "bias": Guarded.of(bias)}
        if res is not None:
            ins["res"] = Guarded.of(rp)
        fn = "dvsg_conv_gemm_f32s"
    else:
        w64 = wt.double()
        wdev = wt
        if prec == "f32x3":
            wdev = torch.empty((cout * K * 6,), dtype=torch.uint8, device=dev)
            _lib.call("dvsg_pack_weights_f32x3", wt.data_ptr(), wdev.data_ptr(), cout, K, _stream())
        ins = {"x": Guarded.of(x), "wt": Guarded.of(wdev), "bias": Guarded.of(bias)}
        if res is not None:
            ins["res"] = Guarded.of(res)
        fn = "dvsg_conv_gemm_" + prec
    before = {k: g.body.clone() for k, g in ins.items()}
    ybytes = B * ho * wo * cout * 4
    ys, recs = [], []
    for _ in range(2):
        y = Guarded(ybytes, dev)
        sc = Guarded(scratch_bytes, dev) if scratch_bytes else None
        _lib.call(fn, ins["x"].ptr(), ins["wt"].ptr(), ins["bias"].ptr(), ins["res"].ptr() if res is not None else 0,
                  y.ptr(), B, H, W, cin, cout, ks, stride, relu, rs, sc.ptr() if sc else 0, scratch_bytes, _stream())
        recs.append(last_config())
        torch.cuda.synchronize()
        assert y.intact(), "output sentinels overwritten"
        assert sc is None or sc.intact(), "scratch sentinels overwritten"
        ys.append(y)
    for k, g in ins.items():
        assert g.intact() and torch.equal(g.body, before[k]), "input %s changed" % k
    assert torch.equal(ys[0].body, ys[1].body), "two launches differ"
    assert recs[0] == recs[1]
    if prec == "f32s":
        y = _from_pieces(ys[0].body, (B, ho, wo, cout))
    else:
        y = ys[0].view(torch.float32, (B, ho, wo, cout))
    ref, S = reference(x.double(), w64, bias.double(), res.double() if res is not None else None, ks, stride, rs, relu)
    S_drop = conv64(x.double().abs() + 2.0 ** -14, w64.abs() + 2.0 ** -14, ks, stride) if prec == "f32s" else None
    return y, ref, S, S_drop, recs[0]


def _set_variant(v):
    from coupe.dvsg_amd import _lib
    _lib.call("dvsg_debug_set_option", b"conv_variant", v)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_layer_configuration_against_float64(case):
    """One configuration of the matrix: the launch record names exactly the expected kernel and work decomposition, every
    output element is within its float64 bound, nothing outside y and the stated scratch is written, the inputs keep their
    bytes, and a second launch gives the same bits."""
    prec, shape, scratch, variant, exp, relu, res = case
    K = shape[5] ** 2 * shape[3]
    try:
        _set_variant(variant)
        y, ref, S, S_drop, rec = run_layer(prec, shape, relu, res, SCRATCH[scratch])
    finally:
        _set_variant(0)
    assert rec == expected_record(case), "launch record %s, expected %s" % (dict(zip(FIELDS, rec)),
                                                                           dict(zip(FIELDS, expected_record(case))))
    nbad, worst = excess(y, ref, bound(prec, K, S, S_drop))
    err = (y.double() - ref).abs() / S.clamp_min(TINY)
    print("%s: worst |y - ref| / S = %.3g = %.2f x 2^-24 sqrt(K); %.3f of the bound"
          % (case_id(case), float(err.max()), float(err.max()) * 2 ** 24 / math.sqrt(K), worst))
    assert nbad == 0, "%d elements out of bounds (worst %.3g of the bound)" % (nbad, worst)


# ---------------------------------------------------------------------------------------------------------------------
# tiny operands: products at the float32 normal / subnormal boundary

def _tiny_operands(device):
    """1x1, K = 32: x, w uniform in [0, 4e-19), products below 1.6e-37 -- a quarter of them under 2^-126 = 1.2e-38 -- and
    sums of ~1.3e-36, several times the floor of 32 x 2^-126; bias and residual ~1e-36"""
    import torch
    g = torch.Generator(device=device).manual_seed(29)
    s = 4e-19
    x = torch.rand((1, 16, 16, 32), generator=g, device=device) * s
    w = torch.rand((64, 32), generator=g, device=device) * s
    bias = (torch.rand((64,), generator=g, device=device) - 0.5) * (16 * s * s)
    res = (torch.rand((1, 16, 16, 64), generator=g, device=device) - 0.5) * (16 * s * s)
    return x, w, bias, res, 1


@pytest.mark.gpu
def test_tiny_operands_subnormal_products():
    """x and w around 1e-19: many products below 2^-126.  Within tau(K) S + K 2^-126 whether the matrix cores keep
    subnormal products or flush them; the test prints which of the two the kernel's result is closer to."""
    import torch
    from coupe.dvsg_amd import _lib
    x, w, bias, res, rs = _tiny_operands(torch.device("cuda:0"))
    y = torch.full((1, 16, 16, 64), float("nan"), device="cuda")
    _lib.call("dvsg_conv_gemm_f32", x.data_ptr(), w.data_ptr(), bias.data_ptr(), res.data_ptr(), y.data_ptr(), 1, 16, 16, 32,
              64, 1, 1, 0, 1, 0, 0, _stream())
    torch.cuda.synchronize()
    ref, S = reference(x.double(), w.double(), bias.double(), res.double(), 1, 1, 1, False)
    prods = x.double().reshape(-1, 1, 32) * w.double().reshape(1, 64, 32)
    sub = prods.abs() < TINY
    flushed = torch.where(sub, torch.zeros_like(prods), prods).sum(2).reshape(ref.shape) + bias.double() + res.double()
    e_keep = float((y.double() - ref).abs().max())
    e_flush = float((y.double() - flushed).abs().max())
    print("tiny operands: %.1f %% of the products subnormal; max |y - exact| = %.3g, |y - flushed| = %.3g (2^-126 = %.3g): "
          "subnormal products %s" % (100.0 * float(sub.double().mean()), e_keep, e_flush, TINY,
                                     "kept" if e_keep < e_flush else "flushed"))
    nbad, worst = excess(y, ref, bound("f32", 32, S))
    assert nbad == 0, worst


# ---------------------------------------------------------------------------------------------------------------------
# block 1's fused conv2 + conv3

FUSED = [(2, 45, 80, 64, 256, 1, 1), (1, 37, 53, 64, 256, 2, 2), (3, 20, 31, 128, 128, 1, 1), (1, 90, 160, 64, 256, 2, 1),
         (1, 1, 1, 64, 128, 1, 1)]


def _fused_operands(shape, device):
    import torch
    B, h, w, cin, cout, stride, res_stride = shape
    g = torch.Generator(device=device).manual_seed(17)
    x = torch.rand((B, h, w, cin), generator=g, device=device) - 0.3
    w2 = (torch.rand((64, 9 * cin), generator=g, device=device) - 0.5) * (2.0 / (9 * cin) ** 0.5)
    b2 = torch.rand((64,), generator=g, device=device) - 0.5
    w3 = (torch.rand((cout, 64), generator=g, device=device) - 0.5) * 0.25
    b3 = torch.rand((cout,), generator=g, device=device) - 0.5
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    res = torch.rand((B, (ho - 1) * res_stride + 1, (wo - 1) * res_stride + 1, cout), generator=g, device=device) - 0.5
    return x, w2, b2, w3, b3, res


def fused_bound(cin, S2, S3, w3):
    """conv3's own bound on its S, plus the intermediate's bound carried through |w3|"""
    K2 = 9 * cin
    return bound("f32", 64, S3) + conv64(bound("f32", K2, S2), w3.abs(), 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,h,w,cin,cout,stride,res_stride", FUSED)
def test_fused_conv3x3_conv1x1_against_float64(B, h, w, cin, cout, stride, res_stride):
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    x, w2, b2, w3, b3, res = _fused_operands((B, h, w, cin, cout, stride, res_stride), dev)
    ins = {k: Guarded.of(t) for k, t in zip(("x", "w2", "b2", "w3", "b3", "res"), (x, w2, b2, w3, b3, res))}
    before = {k: g.body.clone() for k, g in ins.items()}
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ys = []
    for _ in range(2):
        y = Guarded(B * ho * wo * cout * 4, dev)
        _lib.call("dvsg_conv3x3_1x1_f32", ins["x"].ptr(), ins["w2"].ptr(), ins["b2"].ptr(), ins["w3"].ptr(), ins["b3"].ptr(),
                  ins["res"].ptr(), y.ptr(), B, h, w, cin, cout, stride, res_stride, _stream())
        torch.cuda.synchronize()
        assert y.intact()
        ys.append(y)
    assert torch.equal(ys[0].body, ys[1].body)
    for k, g in ins.items():
        assert g.intact() and torch.equal(g.body, before[k]), k
    mid, S2 = reference(x.double(), w2.double(), b2.double(), None, 3, stride, 1, True)
    ref, S3 = reference(mid, w3.double(), b3.double(), res.double(), 1, 1, res_stride, True)
    yv = ys[0].view(torch.float32, (B, ho, wo, cout))
    nbad, worst = excess(yv, ref, fused_bound(cin, S2, S3, w3.double()))
    err = (yv.double() - ref).abs() / S3
    print("fused %d->64->%d s%d B=%d %dx%d: worst |y - ref| / S3 = %.3g; %.3f of the bound"
          % (cin, cout, stride, B, h, w, float(err.max()), worst))
    assert nbad == 0, worst


# ---------------------------------------------------------------------------------------------------------------------
# the network entry points on a workspace of exactly the size the library asks for

NET_SHAPES = [(1, 1, 1), (1, 8, 8), (1, 20, 4), (3, 33, 47), (2, 30, 600), (19, 32, 32), (1, 720, 1280)]
PREC_CODE = {"f32": 0, "f16": 1, "f32s": 2, "f32x3": 3}
NET_ENTRIES = ([("dvsg_locnet_forward_" + p, p) for p in PREC_CODE] + [("dvsg_stabilize_" + p, p) for p in PREC_CODE] +
               [("dvsg_stabilize_ring_f32", "f32"), ("dvsg_stabilize_ring_u8", "f32"), ("dvsg_stabilize_masked_f32", "f32")])


@pytest.fixture(scope="module")
def locnet(synthetic_weights):
    import torch
    assert torch.cuda.is_available()
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


def _net_call(net, name, prec, ins, outs, B, H, W, ws_ptr, ws_bytes):
    from coupe.dvsg_amd import _lib
    h = net.handle
    if name.startswith("dvsg_locnet_forward_"):
        _lib.call(name, h, ins["x"].ptr(), B, H, W, outs["F"].ptr(), ws_ptr, ws_bytes, _stream())
        return
    o = (outs["out"].ptr(), outs["F"].ptr(), outs["xs"].ptr(), outs["ys"].ptr(), ws_ptr, ws_bytes, _stream())
    if name.startswith("dvsg_stabilize_ring_"):
        pool = ins["pool_u8" if name.endswith("u8") else "pool"]
        _lib.call(name, h, PREC_CODE[prec], pool.ptr(), 7 + B, ins["table"].ptr(), B, H, W, *o)
    elif name == "dvsg_stabilize_masked_f32":
        _lib.call(name, h, PREC_CODE[prec], ins["x"].ptr(), ins["u"].ptr(), ins["mask"].ptr(), B, H, W, *o)
    else:
        _lib.call(name, h, ins["x"].ptr(), ins["u"].ptr(), B, H, W, *o)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", NET_SHAPES)
def test_network_entry_points_stay_inside_the_workspace_they_ask_for(locnet, B, H, W):
    """Every dvsg_locnet_forward_* / dvsg_stabilize_* entry point (and the ring and masked forms) with a workspace of
    exactly dvsg_locnet_workspace_bytes(B, H, W) between sentinels -- not LocNet.workspace, which keeps the largest one it
    has seen: sentinels around the workspace, F_t, the frame and the grids intact, inputs unchanged, and the same bits as a
    call with a generous workspace."""
    import torch
    import inputs
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    need = ctypes.c_size_t()
    _lib.call("dvsg_locnet_workspace_bytes", locnet.handle, B, H, W, ctypes.byref(need))
    need = need.value
    assert need % 256 == 0
    x = torch.from_numpy(inputs.window_frames(5 + H, B, H, W)).to(dev)
    frames = torch.from_numpy(inputs.smooth_frames(7 + W, 7 + B, H, W)).to(dev)
    table = (torch.arange(7, dtype=torch.int32, device=dev).unsqueeze(0) + torch.arange(B, dtype=torch.int32, device=dev).unsqueeze(1)).contiguous()
    g = torch.Generator(device=dev).manual_seed(3)
    ins = {"x": Guarded.of(x), "u": Guarded.of(x[..., 18:].contiguous()), "pool": Guarded.of(frames),
           "pool_u8": Guarded.of((frames * 255.0).round().to(torch.uint8)), "table": Guarded.of(table),
           "mask": Guarded.of((torch.rand((B, H, W), generator=g, device=dev) > 0.2).float())}
    before = {k: gd.body.clone() for k, gd in ins.items()}
    big = torch.empty(need + (64 << 20), dtype=torch.uint8, device=dev)
    for name, prec in NET_ENTRIES:
        results = []
        for exact in (True, False):
            outs = {"F": Guarded(B * 50 * 4, dev), "out": Guarded(B * H * W * 3 * 4, dev), "xs": Guarded(B * H * W * 4, dev),
                    "ys": Guarded(B * H * W * 4, dev)}
            ws = Guarded(need, dev) if exact else None
            _net_call(locnet, name, prec, ins, outs, B, H, W, ws.ptr() if exact else big.data_ptr(),
                      need if exact else big.numel())
            torch.cuda.synchronize()
            assert ws is None or ws.intact(), "%s wrote past its %d-byte workspace" % (name, need)
            for k, gd in outs.items():
                assert gd.intact(), "%s: sentinels around %s overwritten" % (name, k)
            results.append(outs)
        for k, gd in ins.items():
            assert gd.intact() and torch.equal(gd.body, before[k]), "%s changed input %s" % (name, k)
        used = ("F",) if name.startswith("dvsg_locnet_forward_") else ("F", "out", "xs", "ys")
        for k in used:
            a, b = results[0][k].body.view(torch.float32), results[1][k].body.view(torch.float32)
            assert bool(torch.isfinite(a).all()), "%s: %s not finite" % (name, k)
            assert torch.equal(a, b), "%s: %s differs from the call with a generous workspace" % (name, k)
