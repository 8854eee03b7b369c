"""No GPU: the NumPy restatement of calibrate_f16's re-rounding rule (calibration_ref.py) obeys its own checker and the
half-step bound on layers of the network's shapes, and the checker rejects the defects the calibration could have and still
pass an end-to-end F_t tolerance: round-to-nearest weights, means of the wrong index or slot, an error sum carried into the
next output row, a weight two float16 steps away, the neighbour on the wrong side of negative weights."""
import numpy as np
import pytest

import calibration_ref as cr

F32 = np.float32
# (cout, K, cin): block 1's conv1 of a later unit, block 2's conv2, block 4's conv2, block 4's conv3
LAYERS = [(256, 64, 64), (128, 1152, 128), (512, 4608, 512), (2048, 512, 512)]
SUM_SLACK = 2.0 ** -39          # float64 rounding of at most 4608 additions, and a near-tie taken the other way (MARGIN)

_CASES = {}


def layer(cout, K, cin, seed=0):
    """(w float32 [cout][K], mu [cin]): weights across six decades, both signs, some float16 values already (+0 and -0
    among them), one weight whose upper float16 neighbour is infinite; non-negative means across three decades, some 0"""
    key = (cout, K, cin, seed)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * seed + cout + K)
        w = (rng.standard_normal((cout, K)) * 10.0 ** rng.uniform(-6.0, 0.0, (cout, K))).astype(F32)
        ex = rng.uniform(size=w.shape) < 0.02
        w[ex] = w[ex].astype(np.float16).astype(F32)
        w[0, 3], w[1, 5], w[2, 7] = F32(0.0), F32(-0.0), F32(65510.0)        # f16(65510) = 65504, whose upper neighbour is inf
        w[3, 0] = F32(-2.0 ** -26)                                          # f16 gives -0; its candidates are -0 and -2^-24
        mu = np.abs(rng.standard_normal(cin)) * 10.0 ** rng.uniform(-3.0, 0.0, cin)
        mu[rng.uniform(size=cin) < 0.1] = 0.0                               # dead channels after the ReLU
        _CASES[key] = (w, mu)
    return _CASES[key]


def final_sum(w, q, mu_k):
    return cr.error_sums(w, q, mu_k)[:, -1]


@pytest.mark.parametrize("cout,K,cin", LAYERS, ids=["%dx%d" % s[:2] for s in LAYERS])
def test_greedy_obeys_its_checker_and_the_half_step_bound(cout, K, cin):
    w, mu = layer(cout, K, cin)
    mu_k = cr.channel_means(mu, K, cin)
    q = cr.greedy(w, mu_k)
    bad, near = cr.check_rule(w, q, mu_k)
    worst = cr.running_bound(w, q, mu_k)
    print("%d x %d: %d violations, %d near-ties, worst |E| / bound %.6f" % (cout, K, bad, near, worst))
    assert bad == 0 and near <= cr.NEAR_TIE_CAP * w.size
    assert worst <= 1.0 + SUM_SLACK
    q0, other, exact = cr.candidates(w)
    assert np.array_equal(q[exact].view(np.uint16), q0[exact].view(np.uint16)) and bool(exact.sum() > 0.015 * w.size)
    assert np.signbit(q[1, 5]) and q[1, 5] == 0 and not np.signbit(q[0, 3])
    assert q[2, 7] == np.float16(65504.0) and np.isinf(other[2, 7])
    assert other[3, 0].view(np.uint16) == 0x8001 and q0[3, 0].view(np.uint16) == 0x8000
    assert bool((q != q0).any()) and bool((q[w < 0] != q0[w < 0]).any())
    assert bool(np.isfinite(q.astype(F32)).all())
    # mu == 0 channels keep round to nearest
    dead = mu_k == 0
    assert dead.any() and np.array_equal(q[:, dead].view(np.uint16), q0[:, dead].view(np.uint16))
    # the candidates bracket w one float16 step apart
    lo, hi = np.minimum(q0, other).astype(np.float64), np.maximum(q0, other).astype(np.float64)
    assert bool(((lo <= w) & (w <= hi))[~exact].all())


def _greedy_carry(w, mu_k):
    """the rule with E carried from the end of row n into row n + 1 (the defect), weight by weight"""
    q0, other, exact = cr.candidates(w)
    q = q0.copy()
    w64, q064, o64 = w.astype(np.float64), q0.astype(np.float64), other.astype(np.float64)
    E = 0.0
    for n in range(w.shape[0]):
        for k in range(w.shape[1]):
            if exact[n, k]:
                continue
            e0, e1 = E + (q064[n, k] - w64[n, k]) * mu_k[k], E + (o64[n, k] - w64[n, k]) * mu_k[k]
            if abs(e1) < abs(e0) and np.isfinite(o64[n, k]):
                q[n, k], E = other[n, k], e1
            else:
                E = e0
    return q


def _two_steps(q):
    return np.nextafter(np.nextafter(q, np.float16(np.inf)), np.float16(np.inf))


def test_checker_rejects_each_defect():
    w, mu = layer(128, 1152, 128)
    K, cin = 1152, 128
    mu_k = cr.channel_means(mu, K, cin)
    good = cr.greedy(w, mu_k)
    assert cr.check_rule(w, good, mu_k)[0] == 0
    q0, other, exact = cr.candidates(w)
    seen = {}
    seen["round to nearest"] = cr.check_rule(w, cr.rtn(w), mu_k)[0]
    seen["means indexed k // 9"] = cr.check_rule(w, cr.greedy(w, mu[np.arange(K) // 9]), mu_k)[0]
    moved = good.copy()
    moved[17, 301] = _two_steps(good[17, 301])
    assert not exact[17, 301]
    seen["one weight two steps away"] = cr.check_rule(w, moved, mu_k)[0]
    first = np.flatnonzero(np.array([cr.check_rule(w[17:18, :k], moved[17:18, :k], mu_k[:k])[0] for k in (301, 302)]))
    assert list(first) == [1]              # the moved weight itself; the later ones of its row are judged against a shifted E
    # neighbour() without its sign handling: "up" adds one to the bit pattern, which moves a negative float16 DOWN
    with np.errstate(over="ignore"):
        wrong = np.nextafter(q0, np.where(q0.astype(F32) < w, np.float16(-np.inf), np.float16(np.inf)).astype(np.float16))
    wrong = np.where(exact | (w > 0), other, wrong)
    assert bool((wrong != other)[w < 0].any())
    seen["wrong side for negative weights"] = cr.check_rule(w, cr.greedy_from(w, q0, wrong, exact, mu_k)[0], mu_k)[0]
    mu_b = layer(128, 1152, 128, seed=1)[1]                            # another slot's means
    seen["two slots' means swapped"] = cr.check_rule(w, cr.greedy(w, cr.channel_means(mu_b, K, cin)), mu_k)[0]
    ws, mus = layer(256, 64, 64)
    mus_k = cr.channel_means(mus, 64, 64)
    assert np.array_equal(_greedy_carry(ws[:1], mus_k), cr.greedy(ws[:1], mus_k))        # the scalar loop is the rule for one row
    seen["E carried into the next row"] = cr.check_rule(ws, _greedy_carry(ws, mus_k), mus_k)[0]
    for name, bad in seen.items():
        print("%-34s %d violations" % (name, bad))
        assert bad > 0, name
    # and a moved exact weight, an infinite weight, the other candidate on a dead channel
    for n, k, v, rest in ((0, 3, np.float16(-0.0), 0), (2, 7, np.float16(np.inf), K)):     # (the sum loses 65504's -6 mu)
        m = good.copy()
        m[n, k] = v
        assert 1 <= cr.check_rule(w, m, mu_k)[0] <= 1 + rest, (n, k)
    dead = np.flatnonzero((mu_k == 0))[0]
    n = int(np.flatnonzero(~exact[:, dead])[0])
    m = good.copy()
    m[n, dead] = other[n, dead]
    assert cr.check_rule(w, m, mu_k)[0] == 1


@pytest.mark.parametrize("cout,K,cin", [LAYERS[0], LAYERS[3]], ids=["256x64", "2048x512"])
def test_greedy_removes_the_bias_of_1x1_layers(cout, K, cin):
    """what the rule is for: the rms over output rows of sum_k (q_k - w_k) mu_k against round to nearest's.  A simulation on
    random layers gives 0.02 - 0.27; asserted is only that it is below 1."""
    w, mu = layer(cout, K, cin)
    mu_k = cr.channel_means(mu, K, cin)
    w = w.copy()
    w[2, 7] = F32(1.0)                     # (the one-candidate weight carries a bias of 6 mu no rule can remove)
    e = final_sum(w, cr.greedy(w, mu_k), mu_k)
    e0 = final_sum(w, cr.rtn(w), mu_k)
    ratio = float(np.sqrt((e * e).mean()) / np.sqrt((e0 * e0).mean()))
    print("%d x %d: rms bias after the rule / round to nearest = %.4f" % (cout, K, ratio))
    assert ratio < 1.0


def test_read_back_rejects_null_pointers_with_a_status():
    """no device work: dvsg_debug_calibration_means and dvsg_debug_plain_weights_f16 without a handle"""
    import ctypes
    from coupe.dvsg_amd import _lib
    lib = _lib.load()
    buf = np.zeros(48)
    assert lib.dvsg_debug_calibration_means(None, buf.ctypes.data, buf.ctypes.data) == -1
    assert b"dvsg_debug_calibration_means" in lib.dvsg_last_error_string()
    dims = (ctypes.c_int * 3)()
    assert lib.dvsg_debug_plain_weights_f16(None, 0, 0, None, 0, dims) == -1
    assert b"dvsg_debug_plain_weights_f16" in lib.dvsg_last_error_string()
