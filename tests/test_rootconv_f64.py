"""rootconv_kernel -- conv1 for a window of S != 7 frames, cin = 3 S a kernel argument -- pinned to float64, element by element.

The method is test_root_head_f64.py's, restated with S in place of 7: every rootconv_kernel<TO, SRC> instantiation of the built
library is launched on purpose by a case of CASES, which names the launch record it expects (family 6, NW 4, TO, SRC); a CPU
test checks the table against the mangled names of the library.  tau, bound, excess, Guarded and TINY are
test_conv_gemm_f64.py's, the float16 interval check is test_conv_f16_f64.py's; the helpers that do not depend on the window
length (u8_to_f32, make_mask, Placed, last_root, positive_weights, conv_region) are test_root_head_f64.py's own.

Operands as the library holds them, NumPy float32 with one rounding per operation:

    scale = gamma / sqrt(var + 1e-5f),  w = w_tf[kh, kw, cs, n] * scale[n],  cs = (2 - c // S) * S + c % S   (make_conv1)
    a = fl(fl(x * 255) - mean_g), g = c // S;  masked: fl(fl(fl(x * m) * 255) - mean_g) on channels < 3 (S - 1);
    uint8: x = fl(v / 255.);  a table index outside [0, n_pool): x = 0;  on the pad ring a = 0 (not -mean).

Every precision multiplies these float32 operands exactly (v_mfma_f32_32x32x2_f32) and converts only the output, so there
is ONE reference per input.  K = 49 x 3 S, S_abs = conv(|a|, |w|) + |b| in float64, ref = relu(conv(a, w) + b):

    float output (f32, f32x3)   |y - ref| <= tau(K) S_abs + K 2^-126 + 2^-24 |mean scale|
    P format (f32s)             the same + 2^-22 S_abs + 2^-25                       (f64.bound "f32s": hi + lo, lo rounded)
    _Float16 output (f16)       y in [RN16(relu(pre - E)), RN16(relu(pre + E))], E the float bound
The 2^-24 |mean scale| is the host's shift = beta - mean * scale, which the compiler may contract (test_root_head_f64.py).

The positive set (uint8 frames >= 160, positive weights and bias: S_abs equals the value, every rounding acts on a partial
sum that grows to the value) is the sharp one.  Worst |y - ref| / (tau(K) S_abs) per window length, measured on one MI355X
(two accumulation chains per block, even and odd taps, 7 x kpad / 4 steps each):
    S                  1      2      5      8      16
    tau(K) x 2^24      16.1   21.1   31.1   38.3   52.5
    positive set       0.415  0.610  0.454  0.520  0.503      (float output; the P format 0.525 at S = 16)
    mixed-sign frames  <= 0.172 at every S and source (0.223 through the P format); float16 outputs inside their
                       rounding interval everywhere
The two-chain split therefore holds to S = 16 without a further one.  The file's GPU run takes 12 s.
"""
import re

import numpy as np
import pytest

import test_conv_gemm_f64 as f64
import test_conv_f16_f64 as f16t
import test_root_head_f64 as rh

tau, bound, excess, Guarded, TINY = f64.tau, f64.bound, f64.excess, f64.Guarded, f64.TINY
check16, rn16 = f16t.check16, f16t.rn16

F32 = np.float32
MEAN_G = rh.MEAN_G
PREFIX = rh.PREFIX
WINDOWS = (1, 2, 5, 8, 16)
TO_OF = {"f32": 0, "f32x3": 0, "f16": 1, "f32s": 2}


# ---------------------------------------------------------------------------------------------------------------------
# operands, NumPy float32 (test_root_head_f64.py's with S in place of 7)

def fold_conv1(weights, S):
    """make_conv1 / bn_fold: w [64, 3 S, 7, 7] (n, raw channel c, kh, kw) float32, bias [64] float32, bias slack [64] float64;
    G: the group size of the reversal (S; anything else is a planted defect)"""
    return _fold(weights, S, S)


def _fold(weights, S, G):
    def get(k):
        return np.asarray(weights[PREFIX + "resnet_v1_50/conv1/" + k + ":0"], dtype=F32)
    w = get("weights")                                       # [7, 7, 3 S, 64] HWIO, scaled-tensor channels
    assert w.shape == (7, 7, 3 * S, 64)
    gamma, beta, mu, var = (get("BatchNorm/" + k) for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    scale = (gamma / np.sqrt((var + F32(1e-5)).astype(F32)).astype(F32)).astype(F32)
    shift = (beta - (mu * scale).astype(F32)).astype(F32)
    cs = np.array([((2 - c // G) * G + c % G) % (3 * S) for c in range(3 * S)])
    wf = (w[:, :, cs, :] * scale[None, None, None, :]).astype(F32)
    slack = 2.0 ** -24 * np.abs(mu.astype(np.float64) * scale.astype(np.float64))
    return np.ascontiguousarray(wf.transpose(3, 2, 0, 1)), shift, slack


def reversal(S):
    return np.array([(2 - c // S) * S + c % S for c in range(3 * S)])


def gather_window(pool, table):
    """dvsg_window_gather_f32: pool [n, H, W, 3] float32, table [B, S] -> window [B, H, W, 3 S]; outside [0, n): zeros"""
    n = pool.shape[0]
    B, S = table.shape
    out = np.zeros((B,) + pool.shape[1:3] + (3 * S,), dtype=F32)
    for b in range(B):
        for s in range(S):
            i = int(table[b, s])
            if 0 <= i < n:
                out[b, :, :, 3 * s:3 * s + 3] = pool[i]
    return out


def scaled(x, mask=None, mask_all=False):
    """the staged activation a [B, H, W, 3 S] float32 (inside the image) of window x, mask plane [B, H, W] or None"""
    x = np.asarray(x, dtype=F32)
    C = x.shape[3]
    S = C // 3
    if mask is not None:
        x = x.copy()
        nm = C if mask_all else 3 * (S - 1)
        x[..., :nm] = (x[..., :nm] * mask[..., None].astype(F32)).astype(F32)
    mean = np.array([MEAN_G[c // S] for c in range(C)], dtype=F32)
    return ((x * F32(255.0)).astype(F32) - mean).astype(F32)


def pad3(a, ring=None):
    """[B, H, W, C] -> torch [B, C, H + 6, W + 6] float32; the ring is 0 (or, for the defect, `ring` per channel)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)
    p = torch.nn.functional.pad(t, (3, 3, 3, 3))
    if ring is not None:
        r = torch.from_numpy(np.asarray(ring, dtype=F32)).view(1, -1, 1, 1).expand_as(p).clone()
        r[:, :, 3:-3, 3:-3] = t
        p = r
    return p.contiguous()


class Operands(object):
    """conv1's float32 operands ready for a float64 evaluation: pre (before ReLU), S_abs and the float tolerance"""

    def __init__(self, folded, a, ring=None):
        import torch
        w, bias, slack = folded
        self.K = 49 * w.shape[1]
        self.w = torch.from_numpy(w.astype(np.float64))
        self.bias = torch.from_numpy(bias.astype(np.float64))
        self.slack = torch.from_numpy(slack)
        self.ap = pad3(a, ring)
        self.B, self.H, self.W = a.shape[:3]
        self.Ho, self.Wo = (self.H - 1) // 2 + 1, (self.W - 1) // 2 + 1

    def full(self):
        pre = rh.conv_region(self.ap, self.w, 0, self.Ho, 0, self.Wo) + self.bias
        S = rh.conv_region(self.ap.abs(), self.w.abs(), 0, self.Ho, 0, self.Wo) + self.bias.abs()
        return pre, S, tau(self.K) * S + self.K * TINY + self.slack


def tol_of(prec, S, tol):
    """the bound of the precision's OUTPUT format around the one float32-operand reference"""
    return tol + 2.0 ** -22 * S + 2.0 ** -25 if prec == "f32s" else tol


def judge(prec, K, y, pre, S, tol):
    """(number of elements out of bounds, worst |y - ref| / (tau(K) S)); f16: the interval criterion"""
    import torch
    ref = pre.clamp_min(0.0)
    unit = float(((y.double() - ref).abs() / (tau(K) * S)).max()) if not bool(torch.isnan(y).any()) else float("inf")
    if prec == "f16":
        return check16(y.double().numpy(), pre.numpy(), tol.expand_as(pre).numpy(), True)[0], unit
    return excess(y, ref, tol_of(prec, S, tol))[0], unit


# ---------------------------------------------------------------------------------------------------------------------
# the case table: (prec, S, kind, masked, off_grid, (B, H, W), inputs); kind 0 window / 1 float32 ring / 2 uint8 ring

SEAM_SHAPES = [(2, 12, 256), (2, 9, 253), (2, 13, 257), (2, 6, 514), (2, 20, 4), (2, 4, 37), (2, 1, 1)]
# Wo 128 127 129 257 2 19 1;  Ho 6 5 7 3 10 2 1;  W % 4 == 0 at 256 and 4
OUT_SHAPES = [(2, 7, 260), (2, 5, 258)]          # the other two output formats: two column tiles, aligned and not
POS_SHAPE = (2, 13, 257)
COMBOS = [(k, m) for m in (0, 1) for k in (0, 1, 2)]


def src_of(kind, aligned, masked):
    return 2 * kind + int(aligned) + 8 * int(masked)


def aligned_of(shape, off_grid):
    return shape[2] % 4 == 0 and not off_grid


def _cases():
    out = []
    n = 0
    for S in WINDOWS:                             # float output: every S meets every seam class, the sources cycle
        for shape in SEAM_SHAPES:
            kind, masked = COMBOS[n % 6]
            n += 1
            out.append(("f32", S, kind, masked, False, shape, "mixed"))
    n = 0
    for prec in ("f16", "f32s", "f32"):           # every SRC in every output format (f32: whatever the cycle above missed)
        for shape in OUT_SHAPES:
            for kind, masked in COMBOS:
                out.append((prec, WINDOWS[n % 5], kind, masked, False, shape, "mixed"))
                n += 1
    out.append(("f32", 8, 1, 0, True, (2, 12, 256), "mixed"))      # an aligned shape from a base off the 16-byte grid
    for S in WINDOWS:                             # the positive set: the bound is sharp
        out.append(("f32", S, 2, 0, False, POS_SHAPE, "pos"))
    out.append(("f16", 16, 2, 0, False, POS_SHAPE, "pos"))
    out.append(("f32s", 16, 0, 0, False, POS_SHAPE, "pos"))
    return out


def expected(case):
    prec, S, kind, masked, off_grid, shape, inputs = case
    return (6, 4, TO_OF[prec], src_of(kind, aligned_of(shape, off_grid), masked), -1, -1)


CASES = _cases()


def case_id(c):
    prec, S, kind, masked, off, (B, H, W), inputs = c
    return "%s-S%d-%s%s%s-%dx%dx%d-%s" % (prec, S, ("win", "ringf", "ringu")[kind], "-mask" if masked else "",
                                          "-off" if off else "", B, H, W, inputs)


# ---------------------------------------------------------------------------------------------------------------------
# CPU

_NAME = re.compile(rb"_ZN4dvsg12_GLOBAL__N_115rootconv_kernelI(f|DF16_|NS0_7PPiecesE)Li(\d+)EEEv")
_ANY = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+rootconv[a-z0-9_]*_kernelI[A-Za-z0-9_]*?EEEv")


def library_instantiations():
    """({(TO, SRC)} of rootconv_kernel, the number of distinct rootconv*_kernel instantiations whatever their arguments) from
    the mangled names in the built library"""
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    found = {({b"f": 0, b"DF16_": 1}.get(to, 2), int(src)) for to, src in _NAME.findall(data)}
    return found, len(set(_ANY.findall(data)))


def test_table_covers_every_rootconv_instantiation():
    """36 instantiations (3 output formats x 12 sources): one without a case, or a case naming one that does not exist,
    fails here; so does a rootconv kernel whose name this file's pattern does not parse."""
    found, named = library_instantiations()
    assert len(found) == 36 and named == 36, (len(found), named)
    covered = {(expected(c)[2], expected(c)[3]) for c in CASES}
    assert not sorted(found - covered), "rootconv_kernel instantiations without a case: %s" % sorted(found - covered)
    assert covered <= found, sorted(covered - found)
    for S in WINDOWS:                              # every window length meets every seam class at the float output
        mine = [c for c in CASES if c[0] == "f32" and c[1] == S]
        wos = {(c[5][2] - 1) // 2 + 1 for c in mine}
        hos = {(c[5][1] - 1) // 2 + 1 for c in mine}
        assert {127, 128, 129} <= wos and max(wos) >= 257, (S, sorted(wos))
        assert any(h % 2 for h in hos) and {1, 2, 3} <= {h % 4 for h in hos}, (S, sorted(hos))
        assert {(2, 20, 4), (2, 4, 37), (2, 1, 1)} <= {c[5] for c in mine}, S
        assert {True, False} == {c[5][2] % 4 == 0 for c in mine}
        assert any(c[6] == "pos" for c in mine), S


_WEIGHTS = {}


def weights_for(S, positive=False):
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if S not in _WEIGHTS:
        _WEIGHTS[S] = make_synthetic_weights(seed=0, c_in=3 * S)
    return rh.positive_weights(_WEIGHTS[S]) if positive else _WEIGHTS[S]


def test_operands_reproduce_the_oracle_at_five_frames():
    """the NumPy operands of this file against oracle.networks at S = 5 on a 9 x 11 window: scale_RGB bit for bit (after the
    group reversal that the weights fold), and conv1 + BatchNorm + ReLU of the oracle within the float32 bound"""
    import torch
    from oracle import networks as onet
    S = 5
    weights = weights_for(S)
    x = np.random.default_rng(5).uniform(0.0, 1.0, (2, 9, 11, 3 * S)).astype(F32)
    a = scaled(x)
    assert np.array_equal(onet.scale_RGB(x)[..., reversal(S)], a)
    scope = PREFIX + "resnet_v1_50/conv1"
    y = onet.conv2d_same_slim(onet.scale_RGB(x), onet._get(weights, scope + "/weights"), 2)
    y = np.maximum(onet.batch_norm_inference(y, weights, scope), 0.0)
    pre, Sabs, tol = Operands(fold_conv1(weights, S), a).full()
    # the oracle scales after the float32 GEMM (two more roundings of values <= S_abs) and adds beta - mean * scale in parts
    nbad, worst = excess(torch.from_numpy(y), pre.clamp_min(0.0), tol + 2.0 ** -22 * Sabs)
    assert nbad == 0, worst


@pytest.mark.parametrize("S", [5, 8])
def test_bounds_flag_the_planted_defects(S):
    """No GPU.  In every output format's bound: a float32 evaluation of the reference passes, and each planted defect -- a
    reversal with G = 7 instead of G = S, the mask on all 3 S channels, the pad ring at -mean, tap kw one pixel late -- is
    flagged."""
    import torch
    weights = weights_for(S)
    folded = fold_conv1(weights, S)
    B, H, W = 2, 9, 11
    x = rh.u8_to_f32(rh.make_pool("u8", B, H, W * S, 3).reshape(B, H, W, S, 3).reshape(B, H, W, 3 * S))
    mask = rh.make_mask(B, H, W, 4)
    meanC = np.array([MEAN_G[c // S] for c in range(3 * S)], dtype=F32)
    for masked in (False, True):
        a = scaled(x, mask if masked else None)
        ops = Operands(folded, a)
        ref = ops.full()
        y32 = (torch.nn.functional.conv2d(ops.ap, ops.w.float(), stride=2).permute(0, 2, 3, 1) + ops.bias.float()).clamp_min(0.0)
        defects = {
            "reversal with G = 7": Operands(_fold(weights, S, 7), a).full()[0],
            "pad ring -mean": Operands(folded, a, ring=-meanC).full()[0],
            "tap kw one pixel late": Operands(folded, np.concatenate([a[:, :, 1:], np.zeros_like(a[:, :, :1])], axis=2)).full()[0],
        }
        if masked:
            defects["mask on all channels"] = Operands(folded, scaled(x, mask, mask_all=True)).full()[0]
        for prec in ("f32", "f32s", "f16"):
            good = torch.from_numpy(rn16(y32.double().numpy())) if prec == "f16" else y32
            assert judge(prec, ops.K, good, *ref)[0] == 0, (prec, masked, "float32 evaluation rejected")
            for name, bad in defects.items():
                yb = bad.clamp_min(0.0)
                yb = torch.from_numpy(rn16(yb.numpy())) if prec == "f16" else yb
                assert judge(prec, ops.K, yb, *ref)[0] > 0, (S, prec, masked, name)


# ---------------------------------------------------------------------------------------------------------------------
# GPU

_NETS = {}


def net_for(S, positive=False):
    from coupe.dvsg_amd.networks import LocNet
    key = (S, positive)
    if key not in _NETS:
        w = weights_for(S, positive)
        _NETS[key] = (LocNet(w), fold_conv1(w, S))
    return _NETS[key]


def make_inputs(case):
    """(pool or window on the host as the kernel reads it, table or None, the float32 window x of the reference, mask)"""
    import inputs as tin
    prec, S, kind, masked, off_grid, (B, H, W), inputs = case
    seed = 1000 * H + W + S
    if inputs == "pos":
        pool = rh.make_pool("pos", B * S, H, W, seed)
    else:
        win = tin.window_frames(seed, B, H, W, S)                       # mixed sign after scaling, band-limited
        pool = np.ascontiguousarray(win.reshape(B, H, W, S, 3).transpose(0, 3, 1, 2, 4).reshape(B * S, H, W, 3))
        if kind == 2:
            pool = np.rint(pool * 255.0).astype(np.uint8)
    n = B * S
    table = np.arange(n, dtype=np.int32).reshape(B, S)[::-1].copy()     # not the identity order
    if kind != 0 and inputs != "pos":                                   # one index outside [0, n_pool) per window
        for b in range(B):
            if S > 1 or b == 0:
                table[b, (b + 1) % S] = -1 if b % 2 == 0 else n
    pf = rh.u8_to_f32(pool) if pool.dtype == np.uint8 else pool
    x = gather_window(pf, table)
    mask = rh.make_mask(B, H, W, seed + 1) if masked else None
    return (x if kind == 0 else pool), (table if kind else None), x, mask


WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_rootconv_against_float64(case):
    """tap 0 of one network call: the launch record names exactly the expected instantiation, every element is within its
    float64 bound (float16 output: inside the rounding interval), nothing outside the output and the workspace is written,
    the inputs keep their bytes."""
    import torch
    prec, S, kind, masked, off_grid, (B, H, W), inputs = case
    net, folded = net_for(S, inputs == "pos")
    dev = torch.device("cuda:0")
    src_h, table_h, x, mk = make_inputs(case)
    src = rh.Placed(src_h, dev, (1 if kind == 2 else 4) if off_grid else 0)
    tab = rh.Placed(table_h, dev) if kind else None
    mask = rh.Placed(mk, dev) if masked else None
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y, rec = rh.run_net(net, prec, kind, masked, src, tab, mask, B * S, B, H, W, 0, B * Ho * Wo * 64)
    assert rec[:6] == expected(case) and rec[6:] == (-1, -1, -1), "launch record %s, expected %s" % (rec, expected(case))
    for p in (src, tab, mask):
        assert p is None or p.unchanged(), "an input changed"
    pre, Sabs, tol = Operands(folded, scaled(x, mk)).full()
    if inputs == "pos":
        assert float((Sabs - pre).abs().max()) <= 1e-9 * float(Sabs.max()), "the positive set is not positive"
    nbad, unit = judge(prec, 49 * 3 * S, y.view(B, Ho, Wo, 64), pre, Sabs, tol)
    key = (S, inputs, prec)
    WORST[key] = max(WORST.get(key, 0.0), unit)
    print("%s: worst |y - ref| / (tau(K) S_abs) = %.3f (tau(K) = %.1f x 2^-24)" % (case_id(case), unit, tau(49 * 3 * S) * 2.0 ** 24))
    assert nbad == 0, "%d elements out of bounds (worst %.3f x tau(K) S_abs)" % (nbad, unit)


def _ring(S, B, H, W, seed):
    """a float32 pool of uint8-valued frames, its uint8 twin and a table with repeats"""
    import torch
    rng = np.random.default_rng(seed)
    n = B * S + 2
    pool8 = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    table = rng.integers(0, n, (B, S)).astype(np.int32)
    return torch.from_numpy(rh.u8_to_f32(pool8)).cuda(), torch.from_numpy(pool8).cuda(), torch.from_numpy(table).cuda()


def _gather(pool, table):
    import torch
    from coupe.dvsg_amd import _lib
    (B, S), (n, H, W, _) = table.shape, pool.shape
    out = torch.empty((B, H, W, 3 * S), dtype=torch.float32, device=pool.device)
    _lib.call("dvsg_window_gather_f32", pool.data_ptr(), n, H, W, table.data_ptr(), B, S, out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 8])
@pytest.mark.parametrize("H,W", [(33, 47), (64, 96)])
def test_sources_agree_bit_for_bit(S, H, W):
    """No tolerance: the float32 ring is the gathered window; the uint8 ring is the float32 ring of the converted frames; a
    mask of exact ones is no mask; the in-place ring writes the contiguous s_t_pred into its pool frames; f32x3's conv1 is
    f32's; and every full F_t comes out the same twice."""
    import torch
    B = 3
    net, _ = net_for(S)
    poolf, pool8, table = _ring(S, B, H, W, 17 * S + H)
    x = _gather(poolf, table)
    ones = torch.ones((B, H, W), device="cuda")
    for prec in ("f32", "f16", "f32s", "f32x3"):
        t0 = net.tap(x, 0, precision=prec)
        assert torch.equal(net.forward_ring(poolf, table, precision=prec, stage=0), t0), prec
        assert torch.equal(net.forward_ring(pool8, table, precision=prec, stage=0), t0), prec
        assert torch.equal(net.forward_masked(x, ones, precision=prec, stage=0), t0), prec
        assert torch.equal(net.forward_masked(poolf, ones, table=table, precision=prec, stage=0), t0), prec
        assert torch.equal(net.forward_masked(pool8, ones, table=table, precision=prec, stage=0), t0), prec
        F = net.forward(x, precision=prec)
        for again in (net.forward(x, precision=prec), net.forward_ring(poolf, table, precision=prec),
                      net.forward_ring(poolf, table, precision=prec), net.forward_ring(pool8, table, precision=prec),
                      net.forward_masked(pool8, ones, table=table, precision=prec)):
            assert torch.equal(again, F), prec
    assert torch.equal(net.tap(x, 0, precision="f32x3"), net.tap(x, 0, precision="f32"))
    # the whole step: contiguous s_t_pred against the in-place ring's pool frames
    out, F = torch.empty((B, H, W, 3), device="cuda"), torch.empty((B, 25, 2), device="cuda")
    net.stabilize_ring(poolf, table, out, F)
    n = poolf.shape[0]
    big = torch.cat([poolf, torch.zeros((B, H, W, 3), device="cuda")])
    slots = torch.arange(n, n + B, dtype=torch.int32, device="cuda")
    F2 = torch.empty_like(F)
    net.stabilize_ring_inplace(big, table, slots, F2)
    assert torch.equal(big[n:], out) and torch.equal(F2, F) and torch.equal(big[:n], poolf)
    want = torch.empty_like(out)
    net.stabilize(x, x[..., -3:].contiguous(), want, F2)
    assert torch.equal(want, out) and torch.equal(F2, F)
