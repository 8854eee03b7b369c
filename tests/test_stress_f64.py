"""The network's kernels pinned to float64, element by element, on the STRESS checkpoint (oracle/stress_weights.py).

Every other per-element float64 pin of the CNN (test_conv_gemm_f64.py, test_conv_f16_f64.py, test_root_head_f64.py,
test_rootconv_f64.py, test_units_f64.py, test_calibration_f64.py) runs on make_synthetic_weights(seed=0), whose folded
weights are a friendly O(0.03 .. 1).  The stress checkpoint has BatchNorm gamma from 0 to 2.5, variances over four decades,
dead channels and all-zero filters: of its 23.5 M folded conv weights some 84 000 nonzero ones lie below 2^-14 -- their
float16 `hi` piece is SUBNORMAL -- and 78 lie below 2^-24.  test_gpu_stress.py holds that checkpoint to F_t and pool5 end to
end, with bounds fitted to what the GPU gave.  This file holds the GPU to the derived bounds of the files above instead, on
those operands: no tolerance here is new, and none is a multiple of a GPU result.  Every number is f64.bound / tau / st /
check16 / judge / excess of the files it imports, a stated condition on the reference, or a printed measurement.

CPU (no GPU): the float64 reference restates the arbiter on this checkpoint (units, conv1, pool, head), the float32 replay
of every unit stays within the bounds in every mode, the reference meets the conditions that make the checkpoint a stress
(no float16 overflow interval, dead channels, elements on both sides of the f32s step at 2^-3, float16-subnormal and
sub-2^-25 weights), the defect "float16-subnormal weight pieces flushed to zero" is rejected at the four projection units
here and is INVISIBLE on the synthetic checkpoint (the statement of the gap this file closes), and the calibration rule
holds on stress layers whose means contain exact zeros.

GPU: units 2..17 in five modes at four shapes, the projection-heavy wiring options, conv1 / max pool / head, the whole
network against the chained bound, the float16 calibration on this checkpoint, and the denormal policy stated once on
stand-alone launches whose every weight piece is float16-subnormal.

The float16-subnormal policy, as found: see MEASURED.
"""
import numpy as np
import pytest

import calibration_ref as cr
import test_conv_gemm_f64 as f64
import test_conv_f16_f64 as f16t
import test_root_head_f64 as root
import test_units_f64 as tu

UNITS, F32 = tu.UNITS, np.float32
SHAPES = [(1, 70, 100), (2, 64, 96), (3, 33, 47), (1, 8, 8)]      # the tilings' edge classes of test_units_f64.SHAPES
BIG = SHAPES[:2]
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]
BIG_IDS = SHAPE_IDS[:2]
REPLAY_MODES = ("f32", "f32s", "f32x3", "f16")
PROJECTION = [U for U in UNITS if U.has_sc]                        # block1..4 unit_1
F16_MAX = 65504.0
NAMES = {"c1": "conv1", "c2": "conv2", "c3": "conv3", "sc": "shortcut"}

# Measured on one MI355X (GPU rows) and on the CPU (replay and mutant rows).  The file's 73 GPU cases run in 33 s, no case
# above 2 s; its 26 CPU cases in about 80 s, of which the four replay cases take 10 s each.  No ratio exceeds 1; no kernel defect
# was found.
MEASURED = """
GPU, worst |y - ref| / bound per unit over the four shapes and the wiring options (float16: |y - relu(pre)| / (E3 + ulp16(y) / 2))
    mode     block1 u1 u2 u3        block2 u1..u4               block3 u1..u6                          block4 u1..u3
    f32      0.077 0.083 0.083      0.162 0.065 0.065 0.064     0.130 0.050 0.048 0.050 0.050 0.048    0.021 0.037 0.037
    f32s     0.047 0.227 0.334      0.096 0.230 0.166 0.203     0.061 0.344 0.330 0.307 0.320 0.246    0.026 0.299 0.215
    f32x3    0.062 0.083 0.083      0.067 0.057 0.058 0.057     0.038 0.045 0.044 0.045 0.045 0.044    0.014 0.034 0.035
    f16      0.953 0.985 0.994      0.992 0.990 0.990 0.988     0.963 0.991 0.997 0.995 0.997 0.997    0.943 0.995 0.992
    f16cal   0.953 0.985 0.994      0.992 0.990 0.990 0.988     0.364 0.991 0.997 0.992 0.997 0.997    0.785 0.995 0.992
    f16cal known (PLAIN from the stress handle, 2 x 64 x 96)
             0.742 0.984 0.994      0.992 0.990 0.990 0.988     0.941 0.991 0.997 0.992 0.997 0.997    0.920 0.986 0.992
    The synthetic checkpoint reads 0.002 - 0.06 (f32), <= 0.004 (f32s) and 0.15 - 0.32 (f16) (test_units_f64.MEASURED).  Here a
    channel whose conv3 row is all zero is its shortcut plus a shift: E3 there is one addition's rounding, the float16
    interval admits one value and the f32s bound is the P format's own step, so the ratios sit at the storage rounding itself
    (f16 0.99, f32s 0.33 = the CPU replay's figures) and the test has no slack to hide a defect in.
    conv1, worst |y - ref| / bound over the four shapes, window / uint8 ring: f32 0.074 / 0.073, f32x3 0.046 / 0.048,
    f32s 0.060 / 0.049, f16 0.968 / 0.965 (the output's float16 rounding); tap 1 is tap 0's maximum bit for bit.
    pool5 0.18 - 0.49 of its bound, F_t 0.000 of its composed bound (test_root_head_f64._head_case, two shapes, four precisions).
    Whole network at 2 x 64 x 96, |F_t - arbiter| / max |F_t| (max |F_t| 47.8; the float32 oracle's own distance 1.7e-6):
        f32 1.3e-6   f32x3 6.0e-7   f32s 1.8e-6 (test_gpu_stress.py's fitted bound 6e-5)   f16 1.0e-3, calibrated 1.2e-3 (fitted 4e-2)
    The chained bound is vacuous here too (1e19 in f32 and f32x3, 4e47 in f32s, the 1e100 cap in float16).
    Calibration on 2 x 64 x 96: means, worst |mu - mean64| / bound: input 0.174, r1 0.0065, r2 0.0014; 52 layers, 23 445 504
    weights, 0 violations, 0 near-ties, worst |E| / running bound 1.000000.
    All-subnormal weight pieces, stand-alone 1x1 launches: f16 and f16s, conv_gemm_kernel and the 256 x 128 kernel, 0.998 (the
    output's float16 rounding); f32s 0.956; the float64 product on the positive channels is 1.24 K 2^-16, 1e3 - 1e4 bounds from 0.
CPU, float32 replay of the unmutated units, worst ratio over the 16 units, range over the four shapes:
    f32 0.06 - 0.17   f32s 0.33 - 0.34   f32x3 0.06 - 0.15   f16 0.995 - 0.997
    unit_ref(exact) against the arbiter: 1.5e-15 of a stage's maximum; conv1's operands 0.006 - 0.009 of their bound
CPU, "float16-subnormal weight pieces flushed to zero", worst ratio (elements out of bounds) at block1..4 unit_1:
    stress    f16   1 x 70 x 100   1.99 (6)      18.6 (39)     38.3 (154)    222 (123)
              f16   2 x 64 x 96    1.42 (10)     22.5 (73)     59.4 (228)    217 (134)
              f32s  1 x 70 x 100   30.8 (3576)   70.7 (2116)   466 (1201)    760 (606)
              f32s  2 x 64 x 96    31.4 (6070)   65.9 (3529)   415 (1702)    636 (587)
    synthetic f16   no element of any of the 16 units out of bounds, worst ratio 0.167 / 0.180 -- the unmutated replay's own
                    figure: invisible there.  (Nonzero folded weights below 2^-14 in the units' 52 layers: stress 77 448, 29 of
                    them below 2^-25; synthetic 42 490, the tail of a normal distribution beside rows of O(0.1).)
CPU, test_units_f64's quiet mutants at stage 5 of this checkpoint (1 x 70 x 100 / 2 x 64 x 96):
    conv3 bias dropped      f32 1.1e6 / 1.1e6    f32x3 9.7e5 / 9.7e5    f32s 305 / 301
    shortcut shift dropped  f32 1.7e4 / 1.2e4
The float16-subnormal policy, as found: subnormal pieces are operands like any other.  make_conv rounds on the host with
gradual underflow; the matrix cores multiply float16-subnormal inputs exactly (v_mfma_f32_32x32x16_f16 and the others take
them as they are); no translation unit is built with a flush-to-zero option, so the device's float32 -> float16 conversions
(P-format pieces, float16 stores) produce subnormals too.  Nothing is flushed and nothing had to be rescaled.  What a small
weight does lose is bits, and the operands' statement already carries that: below 2^-14 the pair rows hold w to 2^-36 and
the f32s rows, whose lo piece is not scaled, to 2^-25 absolute.
"""


@pytest.fixture(scope="module")
def stress():
    from oracle.stress_weights import make_stress_weights
    tu._threads()
    return make_stress_weights(seed=0)


def _sid(shape):
    return "%dx%dx%d" % shape


def arbiter_input(shape, seed=7):
    """the window tu.arbiter_taps feeds the arbiter at `shape`"""
    B, H, W = shape
    pool = root.u8_to_f32(root.make_pool("u8", B + 6, H, W, seed + 1000 * H + W))
    return root.gather_window(pool, root.make_table(B, B + 6, False))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference is meaningful on this checkpoint

@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_unit_reference_restates_the_arbiter_on_stress(stress, shape):
    """unit_ref(exact=True) on the arbiter's tap s - 1 reproduces tap s within 1e-12 of the stage's maximum, all 16 units
    (test_units_f64.test_unit_reference_is_the_arbiter_s_network's tolerance)"""
    taps, names = tu.arbiter_taps(stress, shape), tu._tap_names()
    worst = 0.0
    for i, U in enumerate(UNITS):
        x, want = taps[names[i]], taps[names[i + 1]]
        got = tu.unit_ref(stress, U, "f32", x, exact=True)[0].clamp_min(0.0)
        assert got.shape == want.shape, (U.name, got.shape, want.shape)
        err, top = float((got - want).abs().max()), float(want.abs().max())
        worst = max(worst, err / top)
        assert err <= 1e-12 * top, (U.name, err, top)
    print("stress %s: unit_ref(exact) against the arbiter, worst %.3g of a stage's maximum" % (_sid(shape), worst))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_root_and_head_references_restate_the_arbiter_on_stress(stress, shape):
    """conv1: Operands(fold_conv1(stress), "f32") against the arbiter's conv1 tap within tol + 2^-22 S, the tolerance
    test_root_head_f64.test_operands_reproduce_the_oracle states (the float32 fold and scaling against the float64 ones);
    the max pool of that tap bit for bit; pool5 and F_t from the arbiter's last tap, float64 against float64, within 1e-12
    of the largest element."""
    import torch
    from oracle.cnn_torch import TorchLocNet
    taps = tu.arbiter_taps(stress, shape)
    x = arbiter_input(shape)
    pre, S, tol = root.Operands(root.fold_conv1(stress), "f32", root.scaled(x)).full()
    nbad, worst = f64.excess(taps["conv1"], pre.clamp_min(0.0), tol + 2.0 ** -22 * S)
    print("stress %s: conv1 operands against the arbiter, worst %.3g of the bound" % (_sid(shape), worst))
    assert nbad == 0, (nbad, worst)
    assert torch.equal(root.pool_ref(taps["conv1"]), taps["pool1"])
    p, tol_p = root.head_ref(taps[UNITS[-1].name], None)
    assert float((p - taps["pool5"]).abs().max()) <= 1e-12 * float(taps["pool5"].abs().max())
    Fref, _ = root.dense_ref(taps["pool5"], root._dense_of(stress))
    F = torch.from_numpy(TorchLocNet(stress, dtype=torch.float64).forward(x).reshape(shape[0], 50))
    assert F.dtype == torch.float64
    assert float((Fref - F).abs().max()) <= 1e-12 * float(F.abs().max()), float((Fref - F).abs().max())


_REFS = {}


def unit_case(weights, shape, U, mode):
    """(x float32 in the mode's storage, pre, E3, the unmutated replay) of unit U from the arbiter's tap; computed once"""
    key = (id(weights), shape, U.stage, mode)
    if key not in _REFS:
        tu._threads()
        x = tu._mutant_input(weights, shape, U.stage, mode)
        pre, E3 = tu.unit_ref(weights, U, mode, x.double())
        _REFS[key] = (x, pre, E3, tu.replay(weights, U, mode, x), weights)
    return _REFS[key][:4]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_replay_is_within_bounds_on_stress(stress, shape):
    """the unmutated float32 replay leaves no element out of bounds in f32, f32s, f32x3 and f16, all 16 units"""
    for mode in REPLAY_MODES:
        worst_all = 0.0
        for U in UNITS:
            x, pre, E3, good = unit_case(stress, shape, U, mode)
            nbad, worst = tu.judge(mode, good, pre, E3)
            worst_all = max(worst_all, worst)
            assert nbad == 0, (U.name, mode, nbad, worst)
        print("stress %s %s: float32 replay, worst |y - ref| / bound over the 16 units %.3g" % (_sid(shape), mode, worst_all))


# Dead channels.  An identity unit's output channel relu(x + r) is identically 0 only where the unit before it left the
# channel 0 AND this unit's branch is never positive there, which this checkpoint (seed 0) has at every unit only at
# 1 x 8 x 8; at the three larger shapes block1/unit_3, block2/unit_2 and block2/unit_3 have none (counts printed), and no
# input seed changes a property of the checkpoint.  Asserted, therefore: at DEAD_EVERYWHERE every unit's output has a
# channel that is identically 0; at every shape each of the four PROJECTION units has one (shortcut and branch both dead: the
# units the flush mutant is judged at); and every unit, at every shape, has a conv3 row that is all zero -- a channel whose
# branch is its shift alone, so that E3 there is the rounding of one addition and the float16 interval admits one value.
DEAD_EVERYWHERE = (1, 8, 8)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_reference_meets_the_stress_conditions(stress, shape):
    """Conditions on the float64 arbiter alone, asserted: every tap stays below 65504 / 4 (no float16 overflow interval is
    entered, at any bound that is below three times the value); every unit's output has elements on both sides of 2^-3,
    where the P format's step changes; dead channels, see DEAD_EVERYWHERE."""
    taps = tu.arbiter_taps(stress, shape)
    for name in ["conv1"] + tu._tap_names():
        assert float(taps[name].abs().max()) < F16_MAX / 4, (name, float(taps[name].abs().max()))
    dead = {}
    for U in UNITS:
        y = taps[U.name]
        dead[U.name] = int((y.amax(dim=(0, 1, 2)) == 0).sum())
        pos = y[y > 0]
        assert bool((pos < 0.125).any()) and bool((pos > 0.125).any()), (U.name, float(pos.min()), float(pos.max()))
        w3 = tu.fold_conv(stress, U.scope + "conv3/")[0]
        assert bool((~w3.any(axis=1)).any()), (U.name, "no output channel whose residual branch is its shift alone")
        if U.has_sc or shape == DEAD_EVERYWHERE:
            assert dead[U.name] >= 1, (U.name, "no output channel that is identically 0")
    print("stress %s: largest activation %.4g; output channels identically 0 per unit: %s; %s"
          % (_sid(shape), max(float(taps[n].abs().max()) for n in tu._tap_names()), list(dead.values()),
             ", ".join("%s %.0f%% zero" % (U.name, 100 * float((taps[U.name] == 0).double().mean())) for U in PROJECTION)))


def folded_layers(weights):
    """{(unit index, kind): folded float32 [cout][K]} of the 52 convolutions"""
    out = {}
    for i, U in enumerate(UNITS):
        for kind in (("sc",) if U.has_sc else ()) + ("c1", "c2", "c3"):
            out[(i, kind)] = tu.fold_conv(weights, U.scope + NAMES[kind] + "/")[0]
    return out


def test_weights_meet_the_stress_conditions(stress, synthetic_weights):
    """every layer of each projection unit holds nonzero folded weights below 2^-14 (a subnormal float16 hi piece), some
    layer one below 2^-25 (q0 = 0 with the neighbour 2^-24: the calibration rule's smallest candidates).  The counts over the
    units' 52 layers are printed for both checkpoints: the synthetic one has such weights too (the tail of a normal
    distribution around 0), but beside rows of O(0.1) they move no output by a bound, which the flush mutant shows"""
    counts, tiny = {}, 0
    for (i, kind), w in folded_layers(stress).items():
        a = np.abs(w)
        counts[(i, kind)] = int(((a > 0) & (a < 2.0 ** -14)).sum())
        tiny += int(((a > 0) & (a < 2.0 ** -25)).sum())
    for U in PROJECTION:
        i = UNITS.index(U)
        for kind in ("sc", "c1", "c2", "c3"):
            assert counts[(i, kind)] > 0, (U.name, kind)
    assert tiny > 0
    syn = sum(int(((np.abs(w) > 0) & (np.abs(w) < 2.0 ** -14)).sum()) for w in folded_layers(synthetic_weights).values())
    print("nonzero folded weights below 2^-14: stress %d (below 2^-25: %d), synthetic %d" % (sum(counts.values()), tiny, syn))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the flush mutant, and the quiet mutants on this checkpoint
#
# Measured (CPU, worst |y - ref| / bound of the mutant; block1..4 unit_1): see MEASURED.

@pytest.mark.parametrize("mode", ["f16", "f32s"])
@pytest.mark.parametrize("shape", BIG, ids=BIG_IDS)
def test_flushed_subnormal_pieces_are_rejected_on_stress(stress, shape, mode):
    """float16-subnormal weight pieces read as 0: elements out of bounds at each of the four projection units, in the f16
    (pair rows) and the f32s comparison"""
    for U in PROJECTION:
        x, pre, E3, good = unit_case(stress, shape, U, mode)
        assert tu.judge(mode, good, pre, E3)[0] == 0, (U.name, mode)
        nbad, worst = tu.judge(mode, tu.replay(stress, U, mode, x, tu.FLUSH_SUBNORMAL), pre, E3)
        print("stress %s %s %s: flushed subnormal pieces, %d elements out, worst |y - ref| / bound %.3g"
              % (_sid(shape), mode, U.name, nbad, worst))
        assert nbad > 0 and worst > 1.0, (U.name, mode, nbad, worst)


@pytest.mark.parametrize("shape", BIG, ids=BIG_IDS)
def test_flushed_subnormal_pieces_are_invisible_on_the_synthetic_checkpoint(synthetic_weights, shape):
    """the statement of the gap: in the float16 mode the same defect leaves no element of any of the 16 units out of bounds
    on make_synthetic_weights(seed=0), the checkpoint of every other float64 pin"""
    worst_all = 0.0
    for U in UNITS:
        x, pre, E3, good = unit_case(synthetic_weights, shape, U, "f16")
        nbad, worst = tu.judge("f16", tu.replay(synthetic_weights, U, "f16", x, tu.FLUSH_SUBNORMAL), pre, E3)
        worst_all = max(worst_all, worst)
        assert nbad == 0, (U.name, nbad, worst)
    print("synthetic %s f16: flushed subnormal pieces, worst |y - ref| / bound over the 16 units %.3g" % (_sid(shape), worst_all))


@pytest.mark.parametrize("shape", BIG, ids=BIG_IDS)
def test_quiet_mutants_are_rejected_on_stress(stress, shape):
    """test_units_f64's "quiet"-class mutants, unchanged, at stage 5 of this checkpoint: the unmutated replay passes and
    every mutant that changes a bit of the output is rejected.  The floors 100 / 25 / 10 of that file were argued for the
    synthetic checkpoint and are not copied; the ratios are printed."""
    import torch
    tu._threads()
    bit = 0
    for defect, mode, stage, cls in tu.MUTANTS:
        if cls != "quiet":
            continue
        assert stage == 5
        U = UNITS[stage - 2]
        wts = tu.quiet_weights(stress, U)
        x = tu._mutant_input(stress, shape, stage, mode)
        pre, E3 = tu.unit_ref(wts, U, mode, x.double())
        good = tu.replay(wts, U, mode, x)
        assert tu.judge(mode, good, pre, E3)[0] == 0, (defect, mode)
        bad = tu.replay(wts, U, mode, x, defect)
        if torch.equal(bad, good):
            print("stress %s %-45s %-5s changes no bit" % (_sid(shape), defect, mode))
            continue
        bit += 1
        nbad, worst = tu.judge(mode, bad, pre, E3)
        print("stress %s %-45s %-5s %d elements out, worst |y - ref| / bound %.3g" % (_sid(shape), defect, mode, nbad, worst))
        assert nbad > 0 and worst > 1.0, (defect, mode, nbad, worst)
    assert bit > 0, "no quiet mutant changed a bit"


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the calibration rule on stress layers

def test_calibration_rule_on_stress_layers(stress):
    """calibration_ref.greedy on all 52 stress layers, with the float64 channel means of the arbiter's own tensors at
    2 x 64 x 96 (dead channels: mu == 0 exactly, where the rule must keep q0): check_rule finds 0 violations, near-ties
    within NEAR_TIE_CAP, running_bound <= 1 up to SUM_SLACK.  Asserted of the operands: some mean is exactly 0, some
    candidate q0 is float16-subnormal, and some is 0 with the neighbour +-2^-24 (|w| < 2^-25)."""
    from test_calibration_f64 import SUM_SLACK
    shape = (2, 64, 96)
    taps, names = tu.arbiter_taps(stress, shape), tu._tap_names()
    n_all = near_all = zeros = sub = below = 0
    worst_all = 0.0
    for i, U in enumerate(UNITS):
        inter = {}
        x = taps[names[i]]
        tu.unit_ref(stress, U, "f32", x, exact=True, inter=inter)
        means = {"c1": x, "sc": x, "c2": inter["a1"], "c3": inter["a2"]}
        for kind in (("sc",) if U.has_sc else ()) + ("c1", "c2", "c3"):
            w = tu.fold_conv(stress, U.scope + NAMES[kind] + "/")[0]
            t = means[kind]
            cin = t.shape[3]
            mu_k = cr.channel_means(t.reshape(-1, cin).mean(0).numpy(), w.shape[1], cin)
            q = cr.greedy(w, mu_k)
            bad, near = cr.check_rule(w, q, mu_k)
            assert bad == 0, (U.name, kind, bad)
            q0, other, exact = cr.candidates(w)
            assert np.array_equal(q[:, mu_k == 0].view(np.uint16), q0[:, mu_k == 0].view(np.uint16)), (U.name, kind, "mu == 0 must give q0")
            worst = cr.running_bound(w, q, mu_k)
            assert worst <= 1.0 + SUM_SLACK, (U.name, kind, worst)
            a0 = np.abs(q0.astype(np.float64))
            zeros += int((mu_k == 0).sum())
            sub += int(((a0 > 0) & (a0 < 2.0 ** -14) & ~exact).sum())
            below += int(((q0 == 0) & (w != 0) & (np.abs(other.astype(np.float64)) == 2.0 ** -24)).sum())
            n_all, near_all, worst_all = n_all + w.size, near_all + near, max(worst_all, worst)
    print("stress calibration rule: %d weights, 0 violations, %d near-ties, worst |E| / running bound %.6f; %d zero means, "
          "%d subnormal q0, %d q0 = 0 with neighbour 2^-24" % (n_all, near_all, worst_all, zeros, sub, below))
    assert near_all <= cr.NEAR_TIE_CAP * n_all, near_all
    assert zeros > 0 and sub > 0 and below > 0, (zeros, sub, below)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: units 2..17

UNIT_CASES = [(m, s) for m in tu.MODES for s in SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,shape", UNIT_CASES, ids=["%s-%s" % (m, _sid(s)) for m, s in UNIT_CASES])
def test_every_unit_against_float64_on_stress(stress, mode, shape):
    """taps 1..17 in one mode: every element of every unit's output within the bound composed from the previous tap;
    workspace and output sentinels intact (run_net), inputs unchanged; a repeated tap returns the same bits"""
    import torch
    run = tu.Run(stress, mode, shape)
    tu._check_units(stress, run, set(range(2, 18)), label=" [stress]")
    for stage in (5, 17):
        assert torch.equal(run.tap(stage).view(torch.int32), run.tap(stage).view(torch.int32)), "tap %d differs between two runs" % stage


# the projection-heavy settings: other kernels that read the same subnormal rows
WIRING = ([(m, {k: 0}) for m in ("f32", "f32s") for k in ("fuse_conv", "fuse_shortcut", "concat_sc")] +
          [(m, o) for m in ("f16", "f16cal") for o in ({"fuse_conv": 0}, {"fuse_shortcut": 0}, {"wide16_min_tiles": 1})] +
          [("f32x3", o) for o in ({"x3_fuse": 0}, {"x3_fuse": 2}, {"fuse_conv": 0}, {"concat_sc": 0})])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,opts", WIRING, ids=["%s-%s" % (m, tu._opt_id(o)) for m, o in WIRING])
def test_wiring_options_meet_the_same_reference_on_stress(stress, mode, opts):
    run = tu.Run(stress, mode, (2, 64, 96))
    try:
        tu._set_options(opts)
        tu._check_units(stress, run, set(range(2, 18)), opts, " [stress, %s]" % tu._opt_id(opts))
    finally:
        tu._set_options(opts, restore=True)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the root and the head

ROOT_CASES = [(p, s) for p in ("f32", "f16", "f32s", "f32x3") for s in SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,shape", ROOT_CASES, ids=["%s-%s" % (p, _sid(s)) for p, s in ROOT_CASES])
def test_conv1_and_pool_against_float64_on_stress(stress, prec, shape):
    """conv1 in the precision's default variant from a window tensor and from a uint8 ring, every element by
    test_root_head_f64's own judge against Operands(fold_conv1(stress)); tap 1 the 3 x 3 / 2 maximum of tap 0 bit for bit"""
    import torch
    B, H, W = shape
    net, folded = root._net(stress, False)
    dev = torch.device("cuda:0")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    for kind in (0, 2):
        case = (prec, 0, kind, 0, False, shape, "u8", None)
        src, tab, mask, n, x, mk = root.place_inputs(case, dev)
        y, _ = root.run_net(net, prec, kind, 0, src, tab, None, n, B, H, W, 0, B * Ho * Wo * 64)
        assert src.unchanged() and (tab is None or tab.unchanged()), "an input changed"
        pre, S, tol = root.Operands(folded, prec, root.scaled(x)).full()
        nbad, _ = root.judge(prec, y.view(B, Ho, Wo, 64), pre, S, tol)
        # (judge's own figure divides by tau(K) S, which is 0 in this checkpoint's dead channels: the ratio to the bound instead)
        if prec == "f16":
            worst = f16t.check16(y.view(B, Ho, Wo, 64).double().numpy(), pre.numpy(), tol.numpy(), True)[1]
        else:
            worst = f64.excess(y.view(B, Ho, Wo, 64), pre.clamp_min(0.0), tol)[1]
        print("stress conv1 %s %s %s: worst |y - ref| / bound = %.3f" % (prec, _sid(shape), ("window", "", "ring-u8")[kind], worst))
        assert nbad == 0, "%d elements out of bounds (worst %.3f of the bound)" % (nbad, worst)
        t1, _ = root.run_net(net, prec, kind, 0, src, tab, None, n, B, H, W, 1, B * Hp * Wp * 64)
        assert torch.equal(t1.view(B, Hp, Wp, 64), root.pool_ref(y.view(B, Ho, Wo, 64))), "pool1 is not tap 0's maximum"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16", "f32s", "f32x3"])
@pytest.mark.parametrize("shape", BIG, ids=BIG_IDS)
def test_head_against_float64_on_stress(stress, prec, shape):
    """pool5 from the same inputs' tap 17 and F_t from tap 18, test_root_head_f64._head_case on the stress handle"""
    root._head_case(stress, prec, shape)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the whole network

@pytest.mark.gpu
@pytest.mark.parametrize("mode", tu.MODES)
def test_whole_network_against_float64_on_stress(stress, mode):
    """The chained bound of test_units_f64.test_whole_network_against_float64 built on this checkpoint: F_t is held to it and
    the ratio printed.  That test's fixed 1e-5 / 5e-5 were set for the synthetic checkpoint and do not carry over.  f32 and
    f32x3 keep test_gpu_stress.py's yardstick: no further from the float64 arbiter than twice the float32 oracle's own
    distance, relative to max |F_t|.  f32s and the float16 modes: the composed bound alone; |F_t - arbiter| / max |F_t| is
    printed beside test_gpu_stress.py's fitted figure."""
    import torch
    import test_gpu_stress as gs
    from oracle.cnn_torch import TorchLocNet
    tu._threads()
    shape = (2, 64, 96)
    B, H, W = shape
    run = tu.Run(stress, mode, shape)
    F = run.forward()
    assert run.inputs_unchanged()
    x = root.gather_window(root.u8_to_f32(root.make_pool("u8", B + 6, H, W, 1000 * H + W)), root.make_table(B, B + 6, False))
    prec = tu._prec(mode)
    pre, S, tol = root.Operands(root.fold_conv1(stress), prec, root.scaled(x)).full()
    a = pre.clamp_min(0.0)
    E = tol + tu.st(a, tol, mode)
    a, E = root.pool_ref(a), root.pool_ref(E)
    for U in UNITS:
        pre, E3 = tu.unit_ref(stress, U, mode, a, E)
        a = pre.clamp_min(0.0)
        E = (E3 + tu.st(a, E3, mode)).clamp_max(1e100)
    p, tol_p = root.head_ref(a, None)
    Fref, tol_F = root.dense_ref(p, root._dense_of(stress), e0=tol_p + E.reshape(B, -1, 2048).mean(1))
    nbad, worst = f64.excess(F, Fref, tol_F)
    print("stress %s: F_t worst %.3g of its composed bound (max bound %.3g, max |F_t - ref| %.3g, max |F_t| %.3g)"
          % (mode, worst, float(tol_F.max()), float((F.double() - Fref).abs().max()), float(Fref.abs().max())))
    assert nbad == 0, (nbad, worst)
    rF = TorchLocNet(stress, dtype=torch.float64).forward(x).reshape(B, 50)
    o_rel = float(np.abs(TorchLocNet(stress).forward(x).reshape(B, 50) - rF).max() / np.abs(rF).max())
    rel = float(np.abs(F.numpy() - rF).max() / np.abs(rF).max())
    print("stress %s: |F_t - arbiter| / max |F_t| = %.3g; the float32 oracle's own %.3g; test_gpu_stress.py's fitted bound %s"
          % (mode, rel, o_rel, gs.BOUNDS[prec][0]))
    if prec in ("f32", "f32x3"):
        assert rel <= 2.0 * o_rel + 1e-6, (rel, o_rel)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the float16 calibration on this checkpoint (a handle of its own: test_units_f64._unit_net keys it by checkpoint,
# calibrated on inputs.window_frames(31, 2, 64, 96), test_calibration_f64.WINDOWS[0])

@pytest.mark.gpu
def test_calibration_means_against_float64_on_stress(stress):
    import test_calibration_f64 as tc
    assert tc.cal_of(stress, 0).net is tu._unit_net(stress, "f16cal")
    tc.test_means_against_float64(stress, 0)


@pytest.mark.gpu
def test_calibrated_weights_obey_the_rule_on_stress(stress):
    """0 violations over the 52 layers on the means they were chosen by, near-ties within NEAR_TIE_CAP, running_bound <= 1
    up to SUM_SLACK, and the calibration changed a weight"""
    import test_calibration_f64 as tc
    tc.test_weights_obey_the_rule_on_the_means_they_were_chosen_by(stress, 0)


@pytest.mark.gpu
def test_units_on_the_known_plain_weights_on_stress(stress):
    """row "f16cal known": PLAIN filled from the stress handle's read-back, no interval of the operand, at 2 x 64 x 96"""
    import test_calibration_f64 as tc
    tc.test_units_on_the_known_plain_weights(stress, {}, (2, 64, 96))
    assert not tu.PLAIN


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the denormal policy, stated once.  One 1x1 conv whose every weight lies in +-[2^-24, 2^-15): every float16 piece of it
# (hi, the 2^11-scaled lo of the pair rows, the unscaled lo of the f32s rows) is subnormal or 0, or the one normal value
# 2^-14 a scaled lo can round up to.  Activations 1.0 (the first 64 pixels) and uniform in [1, 2).  The first half of the
# output channels has positive weights: there the float64 product is K 2^-16 on average and a path that reads subnormal
# pieces as 0 returns 0.

DENORMAL_CASES = [("f16", (1, 3, 43, 64, 128, 1, 1), {}), ("f16", (1, 3, 43, 64, 128, 1, 1), f16t.WIDE),
                  ("f16s", (1, 3, 43, 64, 128, 1, 1), {}), ("f16s", (1, 3, 43, 64, 128, 1, 1), f16t.WIDE),
                  ("f32s", (1, 3, 43, 32, 64, 1, 1), {})]


def subnormal_operands(shape, seed):
    import torch
    B, H, W, cin, cout, ks, stride = shape
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** -24 + torch.rand((cout, cin), generator=g) * (2.0 ** -15 - 2.0 ** -24)
    sign = torch.where(torch.rand((cout, cin), generator=g) < 0.5, -1.0, 1.0)
    sign[:cout // 2] = 1.0
    w = (mag * sign).float()
    assert bool((w.abs() >= 2.0 ** -24).all()) and bool((w.abs() <= 2.0 ** -15).all())
    x = 1.0 + torch.rand((B * H * W, cin), generator=g)
    x[:64] = 1.0
    return x.view(B, H, W, cin).half().float(), w


@pytest.mark.gpu
@pytest.mark.parametrize("fn,shape,opts", DENORMAL_CASES,
                         ids=["%s-%s" % (f, tu._opt_id(o) or "default") for f, _, o in DENORMAL_CASES])
def test_float16_subnormal_weight_pieces_are_multiplied(fn, shape, opts):
    """dvsg_conv_gemm_f16 / _f16s / _f32s on all-subnormal weight pieces at the smallest 1x1 shape of test_conv_f16_f64.py /
    test_conv_gemm_f64.py: every output within check16 / f64.bound of the float64 product"""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    B, H, W, cin, cout, ks, stride = shape
    K = cin
    x, w = subnormal_operands(shape, 41)
    x, w = x.to(dev), w.to(dev)
    bias = torch.zeros(cout, device=dev)
    hi = w.half()
    assert bool((hi.float().abs() < 2.0 ** -14).all()) and bool((hi != 0).all()), "a hi piece is not subnormal"
    if fn == "f32s":
        xs = f64._to_pieces(x)
        assert torch.equal(f64._from_pieces(xs, x.shape), x)
        lo = (w - hi.float()).half()
        wdev = torch.cat([hi.reshape(cout, K // 32, 32), lo.reshape(cout, K // 32, 32)], 2).contiguous()
        w64, wabs, xdev, ybytes = hi.double() + lo.double(), hi.double().abs() + lo.double().abs(), xs, 4
    elif fn == "f16s":
        lo = ((w - hi.float()) * 2048.0).half()
        wdev = torch.cat([hi.reshape(cout // 64, 64, K), lo.reshape(cout // 64, 64, K)], 1).reshape(2 * cout, K).contiguous()
        w64, wabs = hi.double() + f16t.LO * lo.double(), hi.double().abs() + f16t.LO * lo.double().abs()
        xdev, ybytes = x.half(), 2
    else:
        lo = torch.zeros_like(hi)
        wdev, w64, wabs, xdev, ybytes = hi.contiguous(), hi.double(), hi.double().abs(), x.half(), 2
    assert bool((lo.float().abs() <= 2.0 ** -14).all())
    ins = {"x": f64.Guarded.of(xdev), "wt": f64.Guarded.of(wdev), "bias": f64.Guarded.of(bias)}
    before = {k: g.body.clone() for k, g in ins.items()}
    y = f64.Guarded(B * H * W * cout * ybytes, dev)
    try:
        f16t._set_options(opts)
        _lib.call("dvsg_conv_gemm_" + fn, ins["x"].ptr(), ins["wt"].ptr(), ins["bias"].ptr(), 0, y.ptr(), B, H, W, cin, cout,
                  ks, stride, 0, 1, 0, 0, f64._stream())
        rec = (f64.last_config(), f16t.last_kernel())
        torch.cuda.synchronize()
    finally:
        f16t._set_options(f16t.DEFAULTS)
    assert y.intact(), "output sentinels overwritten"
    for k, g in ins.items():
        assert g.intact() and torch.equal(g.body, before[k]), "input %s changed" % k
    pre, S = f16t.reference16(x, w64, wabs, bias, None, ks, stride, 1)
    half = cout // 2
    if fn == "f32s":
        got = f64._from_pieces(y.body, (B, H, W, cout))
        S_drop = f64.conv64(x.double().abs() + 2.0 ** -14, wabs + 2.0 ** -14, ks, stride)
        tol = f64.bound("f32s", K, S, S_drop)
        nbad, worst = f64.excess(got, pre, tol)
        margin = float((pre[..., :half].abs() / tol[..., :half]).min())
    else:
        got = y.view(torch.float16, (B, H, W, cout)).double()
        E = (f64.tau(K) * S).cpu().numpy()
        nbad, worst, _ = f16t.check16(got.cpu().numpy(), pre.cpu().numpy(), E, False)
        margin = float((pre[..., :half].abs().cpu().numpy() / (E[..., :half] + f16t.ulp16(pre[..., :half].cpu().numpy()))).min())
    print("subnormal weight pieces, dvsg_conv_gemm_%s %s (record %s): worst |y - ref| / bound %.3f; on the positive channels "
          "the product is at least %.3g bounds from 0, mean %.3g = %.2f K 2^-16"
          % (fn, tu._opt_id(opts) or "default", rec, worst, margin, float(pre[..., :half].mean()),
             float(pre[..., :half].mean()) / (K * 2.0 ** -16)))
    assert margin > 2.0, "a result of 0 would be inside the bound: the case cannot show a flush"
    assert nbad == 0, "%d elements out of bounds (worst %.3g)" % (nbad, worst)
