"""NumPy restatement of dvsg_shake_motion_u8 (include/dvsg_amd.h, "SHAKE MOTION") on top of tests/shake_ref.py, of the host
figures of coupe.dvsg_amd.shake (motion_figures, motion_summary, compare_motion), and the NumPy-only planes that show the rule
measures what it claims.  Nothing is imported from the product.  The rule is integer arithmetic, so the bar against the kernel
is bit equality; the figures are exact rationals until one division (and one square root), so they are equal bit for bit too.

Steps 1 - 5 are shake_ref's.  Then, per pair:
6. Block (a, c) of the ny x nx grid has X = 2c - (nx - 1), Y = 2a - (ny - 1): units of 8 reduced pixels, zero at the centre.
7. A block is an inlier iff it is valid, the pair is ok, |vx - gx| <= gate and |vy - gy| <= gate (gate >= 0, sixteenths).
8. Over the inliers: n_in, Sx = sum X, Sy = sum Y, Su = sum vx, Sv = sum vy, Sxx = sum (X^2 + Y^2), Sxu = sum (X vx + Y vy),
   Sxv = sum (X vy - Y vx), Suu = sum (vx^2 + vy^2).
9. The row is int64 [gx, gy, n_valid, ok, n_in, Sx, Sy, Su, Sv, Sxx, Sxu, Sxv, Suu]; from n_in on it is 0 when the pair is not ok.

Figures, with N = n_in: Pn = N Sxu - Sx Su - Sy Sv, Rn = N Sxv - Sx Sv + Sy Su, Qn = N Sxx - Sx^2 - Sy^2, Vn = N Suu - Su^2 - Sv^2.
Fit iff ok, N >= max(min_blocks, 3) and Qn > 0.  zoom = Pn / (128 Qn), roll = Rn / (128 Qn),
rss = max((Vn Qn - Pn^2 - Rn^2) / (N Qn), 0), wobble = (f / 16) sqrt(rss / N).  The model behind them is
(vx, vy) = (tx, ty) + 128 (zoom X - roll Y, roll X + zoom Y), least squares over the inliers."""
import math
from fractions import Fraction

import numpy as np

import shake_ref

COLUMNS = ("gx", "gy", "n_valid", "ok", "n_in", "Sx", "Sy", "Su", "Sv", "Sxx", "Sxu", "Sxv", "Suu")


def motion_row(blocks, ny, nx, min_blocks, gate):
    """int64 [13] of one pair from its block rows [ny * nx, 3], in Python integers"""
    assert len(blocks) == ny * nx and gate >= 0
    gx, gy, n_valid, ok = (int(v) for v in shake_ref.global_vector(np.asarray(blocks), min_blocks))
    sums = dict.fromkeys(COLUMNS[4:], 0)
    for a in range(ny):
        for c in range(nx):
            vx, vy, valid = (int(v) for v in blocks[a * nx + c])
            if not (valid and ok and abs(vx - gx) <= gate and abs(vy - gy) <= gate):
                continue
            X, Y = 2 * c - (nx - 1), 2 * a - (ny - 1)
            sums["n_in"] += 1
            sums["Sx"] += X
            sums["Sy"] += Y
            sums["Su"] += vx
            sums["Sv"] += vy
            sums["Sxx"] += X * X + Y * Y
            sums["Sxu"] += X * vx + Y * vy
            sums["Sxv"] += X * vy - Y * vx
            sums["Suu"] += vx * vx + vy * vy
    return np.array([gx, gy, n_valid, ok] + [sums[k] for k in COLUMNS[4:]], dtype=np.int64)


def motion_rows(blocks, ny, nx, min_blocks, gate):
    """int64 [n - 1, 13] from block rows [n - 1, n_blk, 3]"""
    return np.stack([motion_row(b, ny, nx, min_blocks, gate) for b in blocks])


def measure(planes, factor, radius, margin_y, margin_x, texture, min_blocks, gate):
    """The whole call on uint8 [n, H, W]: (rows int64 [n - 1, 13], blocks int32 [n - 1, n_blk, 3])"""
    vectors, blocks = shake_ref.measure(planes, factor, radius, margin_y, margin_x, texture, min_blocks)
    ny, nx = shake_ref.block_counts(planes.shape[1] // factor, planes.shape[2] // factor, margin_y, margin_x)
    rows = motion_rows(blocks, ny, nx, min_blocks, gate)
    assert rows[:, :4].tolist() == vectors.tolist()
    return rows, blocks


def fit(row, min_blocks):
    """(N, Pn, Rn, Qn, rss) of a fit pair, exact; None of a pair that is not fit"""
    gx, gy, n_valid, ok, N, Sx, Sy, Su, Sv, Sxx, Sxu, Sxv, Suu = (int(v) for v in row)
    if not ok or N < max(min_blocks, 3):
        return None
    Qn = N * Sxx - Sx ** 2 - Sy ** 2
    if Qn <= 0:
        return None
    Pn = N * Sxu - Sx * Su - Sy * Sv
    Rn = N * Sxv - Sx * Sv + Sy * Su
    Vn = N * Suu - Su ** 2 - Sv ** 2
    rss = Fraction(Vn * Qn - Pn ** 2 - Rn ** 2, N * Qn)
    return N, Pn, Rn, Qn, (rss if rss > 0 else Fraction(0))


def figures(row, factor=1, min_blocks=8):
    """coupe.dvsg_amd.shake.motion_figures"""
    x = fit(row, min_blocks)
    if x is None:
        return dict(fit=False, zoom=None, roll=None, wobble=None)
    N, Pn, Rn, Qn, rss = x
    return dict(fit=True, zoom=float(Fraction(Pn, 128 * Qn)), roll=float(Fraction(Rn, 128 * Qn)),
                wobble=factor / 16 * math.sqrt(float(rss / N)))


def _rms(values):
    return math.sqrt(math.fsum(v * v for v in values) / len(values)) if values else None


def summary(rows, factor, min_blocks=8):
    """coupe.dvsg_amd.shake.motion_summary from rows [n - 1, 13]: per pair one exact division each, over pairs math.fsum"""
    figs = [figures(r, factor, min_blocks) for r in rows]
    fits = [fit(r, min_blocks) for r in rows]
    roll = [g["roll"] for g in figs if g["fit"]]
    d_roll, d_zoom = [], []
    for p, q in zip(figs[:-1], figs[1:]):
        if p["fit"] and q["fit"]:
            d_roll.append(q["roll"] - p["roll"])
            d_zoom.append(q["zoom"] - p["zoom"])
    have = [x for x in fits if x is not None]
    wobble = None
    if have:
        wobble = factor / 16 * math.sqrt(math.fsum(float(x[4]) for x in have) / sum(x[0] for x in have))
    deg = lambda v: None if v is None else math.degrees(v)
    zoom_jitter = _rms(d_zoom)
    return dict(frames=len(figs) + 1, pairs=len(figs), unfit=len(figs) - len(have), roll_rms_deg=deg(_rms(roll)),
                roll_jitter_deg=deg(_rms(d_roll)), zoom_jitter_pct=None if zoom_jitter is None else 100 * zoom_jitter,
                wobble_rms=wobble)


def compare(rows_a, rows_b, factor, min_blocks=8):
    """coupe.dvsg_amd.shake.compare_motion"""
    sa, sb = summary(rows_a, factor, min_blocks), summary(rows_b, factor, min_blocks)

    def ratio(key):
        return sb[key] / sa[key] if sa[key] and sb[key] is not None else None
    return dict(a=sa, b=sb, roll_jitter_ratio=ratio("roll_jitter_deg"), wobble_ratio=ratio("wobble_rms"))


# ---- a brute-force fit to hold the sums against -------------------------------------------------------------------

def least_squares(points):
    """The similarity (tx, ty, p, r) that minimises sum |(vx, vy) - (tx + p X - r Y, ty + r X + p Y)|^2 over
    points [(X, Y, vx, vy), ...], and that minimum, all as Fractions: the 4 x 4 normal equations by Gauss-Jordan elimination.
    None when they are singular."""
    rows = []
    for X, Y, vx, vy in points:
        rows.append(([1, 0, X, -Y], vx))
        rows.append(([0, 1, Y, X], vy))
    A = [[Fraction(sum(r[i] * r[j] for r, _ in rows)) for j in range(4)] + [Fraction(sum(r[i] * b for r, b in rows))]
         for i in range(4)]
    for i in range(4):
        pivot = next((k for k in range(i, 4) if A[k][i] != 0), None)
        if pivot is None:
            return None
        A[i], A[pivot] = A[pivot], A[i]
        A[i] = [v / A[i][i] for v in A[i]]
        for k in range(4):
            if k != i:
                A[k] = [v - A[k][i] * w for v, w in zip(A[k], A[i])]
    sol = [A[i][4] for i in range(4)]
    rss = sum((sum(c * s for c, s in zip(r, sol)) - b) ** 2 for r, b in rows)
    return sol, rss


# ---- test planes, NumPy only --------------------------------------------------------------------------------------

def sample(tex, sy, sx):
    """uint8: `tex` at the float64 coordinates (sy, sx), bilinear, rounded half up; every coordinate must lie inside"""
    iy, ix = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    assert iy.min() >= 0 and ix.min() >= 0 and iy.max() + 1 < tex.shape[0] and ix.max() + 1 < tex.shape[1]
    ay, ax = sy - iy, sx - ix
    t = tex.astype(np.float64)
    out = ((1 - ay) * ((1 - ax) * t[iy, ix] + ax * t[iy, ix + 1]) + ay * ((1 - ax) * t[iy + 1, ix] + ax * t[iy + 1, ix + 1]))
    return np.floor(out + 0.5).astype(np.uint8)


def similarity_coords(H, W, angle=0.0, scale=1.0, t=(0.0, 0.0)):
    """(sy, sx) float64 [H, W]: centre + scale Rot(angle) (p - centre) + t, relative to the plane's own origin; t = (ty, tx).
    Rot turns (x, y) into (x cos - y sin, x sin + y cos), so the block vectors show roll = scale sin(angle) and
    zoom = scale cos(angle) - 1."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = (H - 1) / 2, (W - 1) / 2
    dy, dx = y - cy, x - cx
    c, s = scale * math.cos(angle), scale * math.sin(angle)
    return cy + s * dx + c * dy + t[0], cx + c * dx - s * dy + t[1]


def similarity_plane(tex, H, W, pad, angle=0.0, scale=1.0, t=(0.0, 0.0)):
    """The H x W window of `tex` at (pad, pad) seen through the warp: against shake_ref.shifted(tex, 0, 0, H, W, pad) as the
    previous frame, its content came from where the warp says."""
    sy, sx = similarity_coords(H, W, angle, scale, t)
    return sample(tex, sy + pad, sx + pad)


def bend_coords(H, W, amp, shift_x=0.3):
    """(sy, sx): shifted by shift_x in x and bent by amp sin(2 pi x / W) in y -- motion no similarity explains"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return y + amp * np.sin(2 * math.pi * x / W), x + shift_x


def bend_plane(tex, H, W, pad, amp, patch=None):
    """The bent window; patch = (y0, x0, h, w, dy, dx): the content of that rectangle came from (dy, dx) further on, an
    object that moves on its own."""
    sy, sx = bend_coords(H, W, amp)
    if patch is not None:
        y0, x0, h, w, dy, dx = patch
        sy[y0:y0 + h, x0:x0 + w] += dy
        sx[y0:y0 + h, x0:x0 + w] += dx
    return sample(tex, sy + pad, sx + pad)
