"""The float16 calibration's re-rounding rule, restated in NumPy float64 from the comment above calibrate_f16 (locnet.hip).
Imports nothing from the product.

A layer's folded float32 weights w [cout][K] (k = (kh, kw, c)) get one float16 each.  q0 = f16(w) is round to nearest;
`other` is q0's float16 neighbour on the other side of w, so the two candidates bracket w and lie one float16 step apart.
Along k, per output row n, a float64 sum E of (q - w) mu_k is kept, mu_k the mean activation of weight k's input channel
(mu[k % cin]: the channel's mean for each of a 3x3 layer's nine taps).  The rule:

    take `other`  iff  |E + (other - w) mu_k| < |E + (q0 - w) mu_k|  and `other` is finite;   else q0
    E becomes the chosen candidate's sum;  a weight that is a float16 already is kept and leaves E as it was;
    E starts at 0 for every output row.

check_rule judges a set of float16 weights by that rule along ITS OWN choices: E before k is the sum over the earlier k of
the given q, so a wrong weight is a violation where it stands, shifts E for the rest of its own row only, and every other
row is judged as before.  The library's E is the same sequence of float64 additions (numpy's cumsum along an axis is
sequential), except that a host compiler may contract E + d * mu into one FMA: where the two candidates' |e| differ by less
than `margin` relative, either is accepted and counted as a near-tie.

running_bound: |E_k| <= max_{j <= k} step_j |mu_j| / 2, step the distance of the two candidates.  The candidates' sums lie
step |mu| apart with E between them ((q0 - w) and (other - w) have opposite signs): either 0 lies between them and the nearer
is within half their distance, or both lie on E's side of 0 and the nearer is closer to 0 than E was.  Where `other` is
infinite the rule has one candidate and the argument none: the step is taken as infinite there, and the row's bound with it.
"""
import numpy as np

MARGIN = 2.0 ** -40
NEAR_TIE_CAP = 1e-6          # near-ties outside mu == 0 per weight, over a whole net (a simulation of random layers gives 0)


def candidates(w):
    """(q0, other, exact): float16 [cout][K] twice and the mask of weights that are float16 values already (other = q0)"""
    w = np.asarray(w, dtype=np.float32)
    q0 = w.astype(np.float16)
    q0f = q0.astype(np.float32)
    exact = q0f == w
    toward = np.where(q0f < w, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)
    with np.errstate(over="ignore"):
        other = np.nextafter(q0, toward)
    return q0, np.where(exact, q0, other), exact


def channel_means(mu, K, cin):
    """mu_k [K] of a layer from its slot's channel means: mu[k % cin]"""
    return np.asarray(mu, dtype=np.float64)[np.arange(K) % cin]


def greedy_from(w, q0, other, exact, mu_k):
    """the rule on given candidates, sequential along k (all rows at once): (q float16 [cout][K], E float64 [cout] at the end)"""
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    d0 = (q0.astype(np.float64) - w64) * mu_k[None, :]
    with np.errstate(invalid="ignore"):
        d1 = (other.astype(np.float64) - w64) * mu_k[None, :]
    finite = np.isfinite(other.astype(np.float32))
    q = q0.copy()
    E = np.zeros(w64.shape[0])
    for k in range(w64.shape[1]):
        e0, e1 = E + d0[:, k], E + d1[:, k]
        with np.errstate(invalid="ignore"):
            take = (np.abs(e1) < np.abs(e0)) & finite[:, k] & ~exact[:, k]
        q[take, k] = other[take, k]
        E = np.where(exact[:, k], E, np.where(take, e1, e0))
    return q, E


def greedy(w, mu_k):
    """the re-rounded float16 weights of a layer w [cout][K] float32 for the means mu_k [K]"""
    q0, other, exact = candidates(w)
    return greedy_from(w, q0, other, exact, np.asarray(mu_k, dtype=np.float64))[0]


def error_sums(w, q, mu_k):
    """float64 [cout][K]: E after k, the cumulative sum of (q - w) mu along k"""
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.cumsum((np.asarray(q).astype(np.float64) - w64) * np.asarray(mu_k, dtype=np.float64)[None, :], axis=1)


def check_rule(w, q, mu_k, margin=MARGIN):
    """(violations, near-ties) of float16 weights q against the rule, along q's own choices.  A violation: a weight that is
    not bit for bit one of its two candidates (an exact weight: not itself, the sign of a zero included), an infinite one, the
    candidate with the larger |E + d|, or `other` where mu_k == 0 or the two |e| are equal.  Within `margin` relative of a
    tie either candidate passes and a near-tie is counted."""
    w = np.asarray(w, dtype=np.float32)
    q = np.asarray(q)
    assert q.dtype == np.float16 and q.shape == w.shape
    mu_k = np.asarray(mu_k, dtype=np.float64)
    q0, other, exact = candidates(w)
    w64 = w.astype(np.float64)
    bits, bits0, bits1 = q.view(np.uint16), q0.view(np.uint16), other.view(np.uint16)
    is0, is1 = bits == bits0, (bits == bits1) & ~exact
    d = (q.astype(np.float64) - w64) * mu_k[None, :]
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(d), d, 0.0)
    E = np.cumsum(d, axis=1) - d                          # E before k
    e0 = E + (q0.astype(np.float64) - w64) * mu_k[None, :]
    with np.errstate(invalid="ignore"):
        e1 = E + (other.astype(np.float64) - w64) * mu_k[None, :]
    finite1 = np.isfinite(other.astype(np.float32))
    a0 = np.abs(e0)
    a1 = np.where(finite1, np.abs(e1), np.inf)            # an infinite neighbour is never the smaller
    no_choice = exact | (mu_k[None, :] == 0.0) | (a0 == a1) | ~finite1
    near = ~no_choice & (np.abs(a0 - a1) < margin * np.maximum(a0, a1))
    want1 = ~no_choice & (a1 < a0)
    bad = ~(is0 | is1)                                    # neither candidate (or an exact weight moved)
    bad |= is1 & ~finite1
    bad |= ~bad & ~near & (is1 != want1)
    return int(bad.sum()), int(near.sum())


def running_bound(w, q, mu_k):
    """worst |E_k| / (max_{j <= k} step_j |mu_j| / 2) over a layer (0 where the bound is 0 and so is E; inf if E is not);
    a holding layer gives <= 1 up to the float64 rounding of the sums"""
    w = np.asarray(w, dtype=np.float32)
    mu_k = np.asarray(mu_k, dtype=np.float64)
    q0, other, exact = candidates(w)
    with np.errstate(invalid="ignore"):
        step = np.abs(other.astype(np.float64) - q0.astype(np.float64))        # 0 for an exact weight, inf past the range
        half = np.where(exact, 0.0, step * np.abs(mu_k)[None, :] / 2)
    half = np.where(np.isnan(half), np.inf, half)                              # inf x (mu == 0): no candidate to take
    cap = np.maximum.accumulate(half, axis=1)
    E = np.abs(error_sums(w, q, mu_k))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(cap > 0, E / cap, np.where(E > 0, np.inf, 0.0))
    return float(ratio.max())


def rtn(w):
    """round to nearest: what a new handle, mode 0 and calibrate_f16(None) hold"""
    return np.asarray(w, dtype=np.float32).astype(np.float16)
