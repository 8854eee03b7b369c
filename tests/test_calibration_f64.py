"""dvsg_locnet_calibrate_f16 link by link: the channel means against float64, the re-rounded plain float16 weights against
the rule that chose them, what the rule is for, the handle's state, and the kernels on those weights at the plain float16
class's own bound.  The calibration is read back with dvsg_debug_calibration_means (the means and row counts redo() read,
kept in the handle) and dvsg_debug_plain_weights_f16 (a layer's plain copy wt16); the rule is calibration_ref.py's.

Windows (inputs.window_frames), with chunk = ceil(M / 512) rows per block of channel_sum_kernel and nblk = ceil(M / chunk):
    (2, 64, 96)     the units file's own calibration (seed 31, the same handle); M = 768 in block 1, chunk 2
    (1, 100, 140)   pooled map 25 x 35, M = 875, chunk 2, 438 blocks, the last one short
    (1, 8, 8)       M = 4, then 1 x 1 maps: nblk = M, one row per block
    (2, 160, 256)   M = 5120, chunk 10, 512 blocks: a float32 chain of nine additions inside a block

(a) Means.  The recording pass is the float32 network without fusion and without the `cat` launch, so slot 3 u is the mean
    of the float32 tap s - 1 at fuse_conv = 0, concat_sc = 0 (the same launches: the same bits), and slots 3 u + 1, 3 u + 2
    the means of r1 and r2, which no tap shows: test_units_f64.unit_ref gives a1, a2 in float64 and E1, E2 with
    |r1 - a1| <= E1, |r2 - a2| <= E2 (mode "f32").  Per slot and channel, with X = sum |x| (+ sum E) over the M rows:
        |mu - mean64| <= sum E / M + (gamma(chunk - 1) + (nblk + 64) 2^-53) X / M,   gamma(n) = n 2^-24 / (1 - n 2^-24)
    the carried bound, the float32 chain of chunk - 1 additions inside a block on that block's sum |x| ((chunk - 1) 2^-24 to
    first order; the blocks' sums add up to X), the nblk float64 additions of channel_sum_final, the division and the
    reference's own pairwise float64 sum (at most 62 levels).  Nothing fitted.  Row counts are exact: B h w, and B ho wo for
    slot + 2 of the three stride-2 units.  Channels past a slot's tensor hold 0 (the sums start at 0 and nothing is added);
    no layer reads them (k % cin < cin).  After mode 0, calibrate_f16(None) and mode 1 every mean is 1.0 and every count 0.
(b) The rule.  All 52 layers, block 1's included (re-rounded although block 1 keeps its pairs): calibration_ref.check_rule
    on the read-back weights with the read-back means finds 0 violations, near-ties within NEAR_TIE_CAP of the weights, and
    running_bound holds.  w is test_units_f64.fold_conv's float32 fold.  Mode 1 obeys the rule with mu = 1; mode 0 and
    calibrate_f16(None) give f16(w) bit for bit.
(c) What the rule is for.  With the INDEPENDENT float64 means of (a): every row of every 1x1 layer has
        |sum_k (q_k - w_k) mean64_k| <= max_k step_k |mean64_k| / 2 + sum_k |q_k - w_k| dmu_k,   dmu the bound of (a)
    -- on the calibration frames the bias of every output channel is within half a step.  The 3x3 layers see zero padding
    and, in three units, stride 2: border pixels miss taps and a strided conv reads a quarter of the pixels, so their true
    bias is not this sum over full-map means; they are held to (b) only.
(d) State.  Calibrating on A then on B leaves B's means and weights alone, bit for bit a fresh handle's; twice on A gives
    the same bits; the float32 weights and the hi / lo pairs are untouched (f32 and paired-f16 F_t keep their bits).
(e) The kernels multiply those weights.  test_units_f64.PLAIN filled from the read-back that (b) verified, _check_units in
    mode f16cal with no operand interval, all 16 units at (2, 64, 96) and (1, 70, 100): default options, and
    wide16_min_tiles = 1 with each of wide16_packed, wide16_arows, wide16_hreuse at 0 and at 1 (1 is the default: the three
    settings at 1 are one case), so that the three packed orders of the re-packed copy and the [rows][K] copy are all read.

Measured on one MI355X: MEASURED below.
"""
import ctypes

import numpy as np
import pytest

import calibration_ref as cr
import inputs as tin
import test_units_f64 as tu

UNITS, KINDS = tu.UNITS, tu.KINDS
NAMES = {"c1": "conv1", "c2": "conv2", "c3": "conv3", "sc": "shortcut"}
SLOT_OF = {"c1": 0, "sc": 0, "c2": 1, "c3": 2}
WINDOWS = [(31, (2, 64, 96)), (32, (1, 100, 140)), (33, (1, 8, 8)), (34, (2, 160, 256))]
WINDOW_IDS = ["%dx%dx%d" % s for _, s in WINDOWS]
UNFUSED = {"fuse_conv": 0, "concat_sc": 0}
SUM_SLACK = 2.0 ** -39          # float64 rounding of at most 4608 additions, and a near-tie taken the other way (MARGIN)

# Measured on one MI355X; the file's 24 GPU cases run in 26 s (no case above 6 s).  No ratio exceeds 1; no defect was found in
# calibrate_f16, calib_record or pack_plain.
MEASURED = """
(a) worst |mu - mean64| / bound by slot kind            input (3 u)   r1 (3 u + 1)   r2 (3 u + 2)
    2 x 64 x 96                                          0.28          0.0088         0.0018
    1 x 100 x 140                                        0.19          0.0093         0.0027
    1 x 8 x 8                                            0 (exact)     0.153          0.020
    2 x 160 x 256                                        0.097         0.0092         0.0019
    The input slots carry no E: their bound is the float32 chain alone (one addition at chunk 2, none at 1 x 8 x 8, where
    the float64 sum of at most four float32 values is exact), and the means sit at 0.1 - 0.3 of it.  r1 and r2 are held
    through E1, E2 of the float32 unit bound, which the units file reads at 0.005 - 0.06 itself.
(b) modes 0, 1, 2 (four windows, and mode 2 through the debug entry): 52 layers, 23 445 504 weights, 0 violations,
    0 near-ties; worst |E| / running bound 1.000000 (a row whose first inexact weight lies midway between its candidates).
(c) worst |bias| / (half a step + the means' bound) over the 36 1x1 layers: 0.970, 0.950, 0.995, 0.998 (windows as above).
(e) worst |y - ref| / bound per unit on the known plain weights, over both shapes and the five option settings:
    block1 0.118 0.123 0.152    block2 0.138 0.133 0.151 0.111    block3 0.159 0.128 0.153 0.129 0.135 0.105
    block4 0.145 0.156 0.127
    -- the plain float16 class reads what the paired class reads (0.15 - 0.32), where the interval of the operand read
    0.002 - 0.016.
"""


def layers():
    """(unit index, Unit, kind) of the 52 convolutions in calibrate_f16's order"""
    out = []
    for i, U in enumerate(UNITS):
        out += [(i, U, k) for k in (("sc",) if U.has_sc else ()) + ("c1", "c2", "c3")]
    return out


def folded(weights, U, kind):
    return tu.fold_conv(weights, U.scope + NAMES[kind] + "/")[0]


def read_means(net):
    from coupe.dvsg_amd import _lib
    means, rows = np.full((48, 2048), np.nan), np.full(48, np.nan)
    _lib.call("dvsg_debug_calibration_means", net.handle, means.ctypes.data, rows.ctypes.data)
    return means, rows


def read_plain(net, unit, kind):
    """(float16 [cout][K], cin) of dvsg_debug_plain_weights_f16, the buffer exactly as large as the dims-only call says"""
    from coupe.dvsg_amd import _lib
    dims = (ctypes.c_int * 3)()
    _lib.call("dvsg_debug_plain_weights_f16", net.handle, unit, KINDS[kind], None, 0, dims)
    q = np.zeros((dims[0], dims[1]), np.float16)
    _lib.call("dvsg_debug_plain_weights_f16", net.handle, unit, KINDS[kind], q.ctypes.data, q.nbytes, dims)
    return q, dims[2]


def read_all(net):
    return {(i, kind): read_plain(net, i, kind) for i, _, kind in layers()}


class Cal(object):
    """one handle calibrated on one window, and everything read back from it"""

    def __init__(self, weights, seed, shape):
        from coupe.dvsg_amd.networks import LocNet
        self.shape, self.x = shape, tin.window_frames(seed, *shape)
        if (seed, shape) == WINDOWS[0]:
            self.net = tu._unit_net(weights, "f16cal")           # the units file's own calibrated handle
        else:
            self.net = LocNet(weights)
            self.net.calibrate_f16(self.x)
        self.means, self.rows = read_means(self.net)
        self.q = read_all(self.net)
        self._ref = None

    def taps(self):
        """the float32 taps 1..16 of the calibration windows as the recording pass ran: no fusion, no `cat` launch"""
        import torch
        xd = torch.from_numpy(self.x).cuda()
        try:
            tu._set_options(UNFUSED)
            return [self.net.tap(xd, s, "f32").cpu() for s in range(1, 17)]
        finally:
            tu._set_options(UNFUSED, restore=True)

    def reference(self, weights):
        """(mean64 [48][2048], dmu [48][2048], rows [48]) of (a): float64 means from the GPU's own unfused float32 taps"""
        if self._ref is None:
            tu._threads()
            taps = self.taps()
            mean64, dmu, rows = np.zeros((48, 2048)), np.zeros((48, 2048)), np.zeros(48)
            for i, U in enumerate(UNITS):
                inter = {}
                x = taps[i].double()
                tu.unit_ref(weights, U, "f32", x, opts=UNFUSED, inter=inter)
                for j, (t, E) in enumerate(((x, None), (inter["a1"], inter["E1"]), (inter["a2"], inter["E2"]))):
                    C = t.shape[3]
                    v = t.reshape(-1, C).numpy()
                    M = v.shape[0]
                    e = np.zeros(C) if E is None else E.reshape(-1, C).numpy().sum(0)
                    X = np.abs(v).sum(0) + e
                    chunk = -(-M // 512)
                    nblk = -(-M // chunk)
                    u = (chunk - 1) * 2.0 ** -24
                    mean64[3 * i + j, :C] = v.sum(0) / M
                    dmu[3 * i + j, :C] = e / M + (u / (1 - u) + (nblk + 64) * 2.0 ** -53) * X / M
                    rows[3 * i + j] = M
            self._ref = (mean64, dmu, rows)
        return self._ref


_CALS = {}


def cal_of(weights, index):
    key = (id(weights), index)                    # (the checkpoint is kept in the entry, so its id stays its own)
    if key not in _CALS:
        _CALS[key] = (Cal(weights, *WINDOWS[index]), weights)
    return _CALS[key][0]


def widths():
    """channels of the three slots of every unit"""
    return [(U.cin, U.base, U.base) for U in UNITS]


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(WINDOWS)), ids=WINDOW_IDS)
def test_means_against_float64(synthetic_weights, index):
    """(a): every channel mean within its derived bound of the float64 mean, the row counts exact, unused channels 0"""
    cal = cal_of(synthetic_weights, index)
    B, H, W = cal.shape
    mean64, dmu, rows = cal.reference(synthetic_weights)
    maps = tu.maps(H, W)
    worst = np.zeros(48)
    for i, U in enumerate(UNITS):
        (h, w), (ho, wo) = maps[i], maps[i + 1]
        want = [B * h * w, B * h * w, B * ho * wo]
        for j, C in enumerate(widths()[i]):
            slot = 3 * i + j
            assert cal.rows[slot] == want[j] == rows[slot], (U.name, j, cal.rows[slot], want[j], rows[slot])
            assert bool((cal.means[slot, C:] == 0.0).all()), (U.name, j, "channels past the tensor are not 0")
            diff = np.abs(cal.means[slot, :C] - mean64[slot, :C])
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(dmu[slot, :C] > 0, diff / dmu[slot, :C], np.where(diff > 0, np.inf, 0.0))
            worst[slot] = r.max()
        print("%s %dx%dx%d: worst |mu - mean64| / bound, slots +0 +1 +2: %.3g %.3g %.3g"
              % ((U.name,) + cal.shape + tuple(worst[3 * i:3 * i + 3])))
    assert bool(np.isfinite(cal.means).all())
    print("%dx%dx%d: worst ratio by slot kind: input %.3g, r1 %.3g, r2 %.3g"
          % (cal.shape + (worst[0::3].max(), worst[1::3].max(), worst[2::3].max())))
    assert worst.max() <= 1.0, (int(worst.argmax()), worst.max())


def _check_all_layers(weights, q_of, means, label):
    """(b) over the 52 layers: violations, near-ties, worst running ratio"""
    bad_all, near_all, n_all, worst_all = 0, 0, 0, 0.0
    for i, U, kind in layers():
        w = folded(weights, U, kind)
        q, cin = q_of[(i, kind)]
        K = (9 if kind == "c2" else 1) * cin
        assert q.shape == w.shape == (w.shape[0], K) and cin == {"c1": U.cin, "sc": U.cin, "c2": U.base, "c3": U.base}[kind], (U.name, kind)
        mu_k = cr.channel_means(means[3 * i + SLOT_OF[kind]], K, cin)
        bad, near = cr.check_rule(w, q, mu_k)
        worst = cr.running_bound(w, q, mu_k)
        if bad:
            print("%s %s %s: %d violations of %d weights" % (label, U.name, kind, bad, w.size))
        bad_all, near_all, n_all, worst_all = bad_all + bad, near_all + near, n_all + w.size, max(worst_all, worst)
    print("%s: %d layers, %d weights, %d violations, %d near-ties, worst |E| / running bound %.6f"
          % (label, len(layers()), n_all, bad_all, near_all, worst_all))
    assert len(layers()) == 52
    assert bad_all == 0, bad_all
    assert near_all <= cr.NEAR_TIE_CAP * n_all, near_all
    assert worst_all <= 1.0 + SUM_SLACK, worst_all
    return worst_all


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(WINDOWS)), ids=WINDOW_IDS)
def test_weights_obey_the_rule_on_the_means_they_were_chosen_by(synthetic_weights, index):
    """(b), mode 2: the read-back weights of all 52 layers against the read-back means"""
    cal = cal_of(synthetic_weights, index)
    _check_all_layers(synthetic_weights, cal.q, cal.means, "mode 2 %dx%dx%d" % cal.shape)
    changed = sum(int((cal.q[(i, kind)][0] != cr.rtn(folded(synthetic_weights, U, kind))).sum()) for i, U, kind in layers())
    assert changed > 0, "the calibration changed no weight"


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(WINDOWS)), ids=WINDOW_IDS)
def test_bias_of_every_1x1_output_channel_is_within_half_a_step(synthetic_weights, index):
    """(c): with the independent float64 means and their bound, not the library's own"""
    cal = cal_of(synthetic_weights, index)
    mean64, dmu, _ = cal.reference(synthetic_weights)
    worst_all = 0.0
    for i, U, kind in layers():
        if kind == "c2":
            continue
        w = folded(synthetic_weights, U, kind)
        q, cin = cal.q[(i, kind)]
        slot = 3 * i + SLOT_OF[kind]
        mu, dm = mean64[slot, :cin], dmu[slot, :cin]
        q0, other, exact = cr.candidates(w)
        step = np.abs(other.astype(np.float64) - q0.astype(np.float64))
        dq = q.astype(np.float64) - w.astype(np.float64)
        bias = np.abs((dq * mu[None, :]).sum(1))
        allowed = (step * np.abs(mu)[None, :]).max(1) / 2 + (np.abs(dq) * dm[None, :]).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(allowed > 0, bias / allowed, np.where(bias > 0, np.inf, 0.0))
        worst_all = max(worst_all, float(r.max()))
        assert r.max() <= 1.0, (U.name, kind, int(r.argmax()), float(r.max()))
    print("%dx%dx%d: worst |bias| / (half a step + the means' bound) over the 36 1x1 layers: %.4f" % (cal.shape + (worst_all,)))


@pytest.mark.gpu
def test_modes_0_and_1_and_the_undo(synthetic_weights):
    """(b): mode 1 obeys the rule with mu = 1, mode 0 and calibrate_f16(None) hold f16(w) bit for bit; the means read back
    as the 1.0 the code uses and the row counts as 0.  The read-back rejects bad arguments with a status."""
    import torch
    from coupe.dvsg_amd import DvsgError, _lib
    from coupe.dvsg_amd.networks import LocNet
    net = LocNet(synthetic_weights)
    ones = np.ones((48, 2048))

    def state():
        means, rows = read_means(net)
        return means, rows, read_all(net)

    def rtn_everywhere(q_of):
        return all(np.array_equal(q_of[(i, k)][0].view(np.uint16), cr.rtn(folded(synthetic_weights, U, k)).view(np.uint16))
                   for i, U, k in layers())

    means, rows, q_of = state()                                            # a new handle
    assert np.array_equal(means, ones) and not rows.any() and rtn_everywhere(q_of)
    x = torch.from_numpy(tin.window_frames(35, 1, 8, 8)).cuda()
    ws, nbytes = net.workspace(1, 8, 8)

    def debug_calibrate(mode):
        _lib.call("dvsg_debug_calibrate_f16_weights", net.handle, x.data_ptr(), 1, 8, 8, mode, ws.data_ptr(), nbytes,
                  torch.cuda.current_stream().cuda_stream)

    debug_calibrate(1)
    means, rows, q_of = state()
    assert np.array_equal(means, ones) and not rows.any()
    _check_all_layers(synthetic_weights, q_of, ones, "mode 1")
    assert not rtn_everywhere(q_of)
    debug_calibrate(2)
    means, rows, q_of = state()
    assert rows.all() and not np.array_equal(means, ones)
    _check_all_layers(synthetic_weights, q_of, means, "mode 2 through the debug entry")
    debug_calibrate(0)
    means, rows, q_of = state()
    assert np.array_equal(means, ones) and not rows.any() and rtn_everywhere(q_of)
    net.calibrate_f16(tin.window_frames(35, 1, 8, 8))
    assert not rtn_everywhere(read_all(net))
    net.calibrate_f16(None)
    means, rows, q_of = state()
    assert np.array_equal(means, ones) and not rows.any() and rtn_everywhere(q_of)
    dims = (ctypes.c_int * 3)()
    for args in ((None, 0, 0, None, 0, dims), (net.handle, 16, 0, None, 0, dims), (net.handle, -1, 0, None, 0, dims),
                 (net.handle, 0, 4, None, 0, dims), (net.handle, 1, 3, None, 0, dims), (net.handle, 0, 0, None, 0, None)):
        with pytest.raises(DvsgError, match="dvsg_debug_plain_weights_f16"):
            _lib.call("dvsg_debug_plain_weights_f16", *args)
    small = np.zeros(8, np.float16)
    with pytest.raises(DvsgError, match="dvsg_debug_plain_weights_f16"):
        _lib.call("dvsg_debug_plain_weights_f16", net.handle, 0, 0, small.ctypes.data, small.nbytes, dims)
    assert not small.any()
    with pytest.raises(DvsgError, match="dvsg_debug_calibration_means"):
        _lib.call("dvsg_debug_calibration_means", net.handle, None, None)


@pytest.mark.gpu
def test_a_second_calibration_replaces_the_first(synthetic_weights):
    """(d)"""
    import torch
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    fresh_b = cal_of(synthetic_weights, 1)                                  # a handle calibrated on B alone
    a, b = tin.window_frames(36, 2, 64, 96), fresh_b.x
    probe = torch.from_numpy(tin.window_frames(37, 1, 64, 96)).cuda()
    net = LocNet(synthetic_weights)
    before = [net.forward(probe, precision=p).clone() for p in ("f32", "f16")]     # (uncalibrated: pairs everywhere)

    def same(q1, q2):
        return all(np.array_equal(q1[k][0].view(np.uint16), q2[k][0].view(np.uint16)) for k in q1)

    net.calibrate_f16(a)
    means_a, rows_a = read_means(net)
    q_a = read_all(net)
    net.calibrate_f16(a)
    means_a2, rows_a2 = read_means(net)
    assert np.array_equal(means_a, means_a2) and np.array_equal(rows_a, rows_a2) and same(q_a, read_all(net))
    assert torch.equal(net.forward(probe, precision="f32"), before[0]), "a calibration changed the float32 path"
    net.calibrate_f16(b)
    means_b, rows_b = read_means(net)
    q_b = read_all(net)
    assert np.array_equal(means_b, fresh_b.means) and np.array_equal(rows_b, fresh_b.rows), "the first calibration shows through"
    assert same(q_b, fresh_b.q), "weights of the second calibration differ from a fresh handle's"
    assert not np.array_equal(means_b, means_a) and not same(q_b, q_a)
    # the float32 weights and the hi / lo pairs: re-rounded through the debug entry the pair policy stays "everywhere", and
    # both paths give the bits they gave before any calibration
    net.calibrate_f16(None)
    xb = torch.from_numpy(b).cuda()
    ws, nbytes = net.workspace(*fresh_b.shape)
    _lib.call("dvsg_debug_calibrate_f16_weights", net.handle, xb.data_ptr(), fresh_b.shape[0], fresh_b.shape[1], fresh_b.shape[2],
              2, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert same(read_all(net), fresh_b.q)
    after = [net.forward(probe, precision=p) for p in ("f32", "f16")]
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])


# (e)
PLAIN_OPTS = [{}, {"wide16_min_tiles": 1}, {"wide16_min_tiles": 1, "wide16_packed": 0}, {"wide16_min_tiles": 1, "wide16_arows": 0},
              {"wide16_min_tiles": 1, "wide16_hreuse": 0}]
PLAIN_CASES = [(o, s) for o in PLAIN_OPTS for s in tu.WIRING_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("opts,shape", PLAIN_CASES, ids=["%s-%dx%dx%d" % ((tu._opt_id(o) or "default",) + s) for o, s in PLAIN_CASES])
def test_units_on_the_known_plain_weights(synthetic_weights, opts, shape):
    """(e): the calibrated net's 16 units against float64 on the plain copies read back from the handle -- no interval of
    the operand, the plain float16 class's own bound"""
    cal = cal_of(synthetic_weights, 0)
    run = tu.Run(synthetic_weights, "f16cal", shape)
    assert run.net is cal.net
    try:
        for i, U, kind in layers():
            tu.PLAIN[(id(synthetic_weights), U.scope + NAMES[kind] + "/")] = cal.q[(i, kind)][0]
        tu._set_options(opts)
        tu._check_units(synthetic_weights, run, set(range(2, 18)), opts, " [known plain weights, %s]" % (tu._opt_id(opts) or "default"))
    finally:
        tu.PLAIN.clear()
        tu._set_options(opts, restore=True)
