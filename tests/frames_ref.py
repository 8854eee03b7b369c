"""NumPy references of the frame-format kernels of coupe/dvsg_amd/csrc/frames.hip, written from that file's header comment
and from include/dvsg_amd.h -- not from oracle/frames.py, which the CPU tests compare them with.  No product import.

Layout everywhere: frames [n,H,W,3], channel last; `flip` exchanges channels 0 and 2 (BGR <-> RGB)."""
import numpy as np

F32 = np.float32
U24, U25, U53 = 2.0 ** -24, 2.0 ** -25, 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------------
# conversions

def u8_to_f32(u, flip):
    """eval.py:79-80: float32(float64(u) / 255.), channels exchanged under flip"""
    u = np.asarray(u, dtype=np.uint8)
    if flip:
        u = u[..., ::-1]
    return (u.astype(np.float64) / 255.).astype(F32)


def to_u8(x):
    """np.uint8(x * 255.) of eval.py:112 with the kernel's documented saturation (common.h: to_u8): the product is float64
    and is truncated toward zero; a product >= 255 (and +inf) gives 255; a product <= 0, NaN and -inf give 0.  np.uint8
    itself WRAPS for the same inputs (np.uint8(1.5 * 255.) is 126 on this platform, and the cast of NaN is undefined), so
    this is not np.uint8 outside [0, 1]."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(x, dtype=np.float64) * 255.
        out = np.zeros(d.shape, dtype=np.uint8)
        mid = (d > 0.) & (d < 255.)
        out[mid] = np.trunc(d[mid]).astype(np.uint8)
        out[d >= 255.] = 255
    return out


def place_rows(dst, rows, dst_W, x0):
    """the side-by-side layout: a copy of the bytes `dst` (n H rows of dst_W pixels) with rows [n,H,W,3] in the columns
    [x0, x0 + W) of every row and every other byte as it was"""
    rows = np.asarray(rows, dtype=np.uint8)
    n, H, W, _ = rows.shape
    assert x0 >= 0 and dst_W >= x0 + W
    out = np.array(dst, dtype=np.uint8).reshape(n * H, dst_W, 3)
    out[:, x0:x0 + W] = rows.reshape(n * H, W, 3)
    return out.reshape(n, H, dst_W, 3)


def slot_ok(slots, n_pool):
    slots = np.asarray(slots)
    return (slots >= 0) & (slots < n_pool)


def egress_slots(pool, slots):
    """frames [n,...] read from pool frames `slots`: a slot outside [0, n_pool) reads as a frame of zeros"""
    pool, slots = np.asarray(pool), np.asarray(slots)
    ok = slot_ok(slots, pool.shape[0])
    out = pool[np.where(ok, slots, 0)].copy()
    out[~ok] = 0
    return out


def ingest_slots(pool, frames, slots):
    """a copy of `pool` with frame i written to pool frame slots[i]; a slot outside [0, n_pool) writes nothing at all
    (distinct slots: two frames into one slot race)"""
    out = np.array(pool)
    ok = slot_ok(slots, out.shape[0])
    good = np.asarray(slots)[ok]
    assert len(set(good.tolist())) == good.size
    out[good] = np.asarray(frames)[ok]
    return out


def ingest_u8_half(dst, rows, slots, n_pool, dst_W, x0):
    """place_rows for the uint8 half of an ingest: the rows of a frame whose slot lies outside the pool stay as they were"""
    rows = np.asarray(rows, dtype=np.uint8)
    n, H, W, _ = rows.shape
    before = np.array(dst, dtype=np.uint8).reshape(n, H, dst_W, 3)
    out = place_rows(before, rows, dst_W, x0)
    out[~slot_ok(slots, n_pool)] = before[~slot_ok(slots, n_pool)]
    return out


def window_gather(pool, idx):
    """eval.py:103-104: patches[b,y,x,3s+c] = pool[idx[b,s],y,x,c]; an index outside the pool reads as zeros"""
    pool, idx = np.asarray(pool), np.asarray(idx)
    B, S = idx.shape
    fr = egress_slots(pool, idx.reshape(-1)).reshape((B, S) + pool.shape[1:])         # [B,S,h,w,3]
    return np.ascontiguousarray(np.moveaxis(fr, 1, 3)).reshape(B, pool.shape[1], pool.shape[2], 3 * S)


# ---------------------------------------------------------------------------------------------------------------------
# resize

RESIZE_DEFECTS = ("weight_f64", "scale_f32", "lower_clamp_keeps_weight", "columns_first", "u8_half_channel")


def resize_coords(n_dst, n_src):
    """float64 (d + .5) * (n_src / n_dst) - .5"""
    return (np.arange(n_dst, dtype=np.float64) + .5) * (np.float64(n_src) / np.float64(n_dst)) - .5


def resize_taps(n_dst, n_src, defect=None):
    """(s0, s1, w1) of the kernel's resize_tap: the coordinate is the float32 of the float64 expression, the weight of
    tap s1 its float32 fractional part (exact for a coordinate >= 0: a float32 minus its floor needs no more bits), and on
    either clamp the weight is 0"""
    if defect == "scale_f32":
        f = ((np.arange(n_dst, dtype=np.float64) + .5) * np.float64(F32(n_src) / F32(n_dst)) - .5).astype(F32)
    else:
        f = resize_coords(n_dst, n_src).astype(F32)
    s = np.floor(f).astype(np.int64)
    w = (f - s.astype(F32)).astype(F32)
    lo = s < 0
    s[lo] = 0
    if defect != "lower_clamp_keeps_weight":
        w[lo] = 0
    hi = s >= n_src - 1
    s[hi] = n_src - 1
    w[hi] = 0
    return s, np.minimum(s + 1, n_src - 1), w


def _frames64(u8, flip):
    u = np.asarray(u8, dtype=np.uint8)
    u = u[None] if u.ndim == 3 else u
    p = u.astype(np.float64) / 255.
    return p[..., ::-1] if flip else p


def resize_variant(u8, dh, dw, flip, defect=None):
    """resize_exact, or a simulated wrong kernel (RESIZE_DEFECTS)"""
    p = _frames64(u8, flip)
    x0, x1, wx = resize_taps(dw, p.shape[2], defect)
    y0, y1, wy = resize_taps(dh, p.shape[1], defect)
    one = np.float64(1) if defect == "weight_f64" else F32(1)
    a1, a0 = wx.astype(np.float64)[None, None, :, None], (one - wx).astype(np.float64)[None, None, :, None]
    b1, b0 = wy.astype(np.float64)[None, :, None, None], (one - wy).astype(np.float64)[None, :, None, None]
    if defect == "columns_first":
        cols = p[:, y0] * b0 + p[:, y1] * b1
        return cols[:, :, x0] * a0 + cols[:, :, x1] * a1
    rows = p[:, :, x0] * a0 + p[:, :, x1] * a1               # two products and one sum, float64, nothing fused
    return rows[:, y0] * b0 + rows[:, y1] * b1


def resize_exact(u8, dh, dw, flip):
    """the kernel's definition of cv2.resize(u8 / 255., (dw, dh)), rounding for rounding -> float64 [n,dh,dw,3]"""
    return resize_variant(u8, dh, dw, flip)


def resize_u8_half(v, flip, defect=None):
    """the uint8 half of a resize: to_u8 of the float64 value, back in the SOURCE's channel order"""
    b = to_u8(v)
    return b[..., ::-1] if flip and defect != "u8_half_channel" else b


def _geometric_taps(n_dst, n_src):
    x = resize_coords(n_dst, n_src)
    s = np.floor(x).astype(np.int64)
    w = x - s
    lo = s < 0
    s[lo], w[lo] = 0, 0.
    hi = s >= n_src - 1
    s[hi], w[hi] = n_src - 1, 0.
    return s, np.minimum(s + 1, n_src - 1), w, x


def resize_geometric(u8, dh, dw, flip):
    """the same map with float64 coordinates and weights throughout: clamped bilinear interpolation at half-pixel centres"""
    p = _frames64(u8, flip)
    x0, x1, wx, _ = _geometric_taps(dw, p.shape[2])
    y0, y1, wy, _ = _geometric_taps(dh, p.shape[1])
    wx, wy = wx[None, None, :, None], wy[None, :, None, None]
    rows = p[:, :, x0] * (1. - wx) + p[:, :, x1] * wx
    return rows[:, y0] * (1. - wy) + rows[:, y1] * wy


def _axis_reach(n_dst, n_src):
    """per destination index: (first tap, last tap) over the exact and the geometric cell, and how far the sample point
    may move"""
    s0, s1, _ = resize_taps(n_dst, n_src)
    g0, g1, _, x = _geometric_taps(n_dst, n_src)
    return np.minimum(s0, g0), np.maximum(s1, g1), U24 * np.abs(x) + 8. * U53 * (np.abs(x) + 1.)


def resize_bound(u8, dh, dw, flip, float64_only=False):
    """Per value [n,dh,dw,3]: how far resize_exact may lie from resize_geometric (and from any float64 evaluation of the same
    clamped bilinear map, such as torch's).  Derived, not fitted:

    I(X, Y), the clamped bilinear interpolant, is continuous and piecewise linear in X at fixed Y and in Y at fixed X; its
    slope in X is a convex combination (over the two rows of Y's cell) of adjacent-pixel differences p[r,c+1] - p[r,c] of
    the cells that X passes through, and 0 beyond a clamp.  resize_exact evaluates I at (X~, Y~), X~ = float32(X):
        |X~ - X| <= 2^-24 |X|, and the float64 expression itself carries three roundings: 8 x 2^-53 (|X| + 1) covers it
        (on this side and on the other evaluation's side).
    Going from (X, Y) to (X~, Y) to (X~, Y~) moves the value by at most dX L_x + dY L_y, with L_x (L_y) the largest
    adjacent-pixel difference along x (y) inside the rectangle of taps of both cells -- the exact one and the geometric one,
    which differ where the rounding carries a coordinate across an integer; there hi - lo is 2 taps, never more.
    The fractional weight w of the float32 coordinate is exact, but 1 - w is rounded to float32: |e| <= 2^-25, so a pass
    computes p0 (1 - w + e) + p1 w = the interpolant + e p0: 2^-25 |p| per axis, |p| <= the largest tap (the second pass
    sees the first's result, itself at most (1 + 2^-25) times the largest tap).
    The seven float64 operations of a value (division by 255, four products... two sums per pass) add a few 2^-53 of the
    largest tap on either side: 16 x 2^-53 |p|.
        bound = dX L_x + dY L_y + 2 x 2^-25 (1 + 2^-24) |p|max + 16 x 2^-53 |p|max
    float64_only: the part of it that two float64 evaluations of the map may differ by (no 2^-24, no 2^-25 term)."""
    p = _frames64(u8, flip)
    sh, sw = p.shape[1], p.shape[2]
    clo, chi, dX = _axis_reach(dw, sw)
    rlo, rhi, dY = _axis_reach(dh, sh)
    assert (chi - clo).max() <= 2 and (rhi - rlo).max() <= 2
    Dx, Dy = np.zeros_like(p), np.zeros_like(p)
    Dx[:, :, :-1] = np.abs(np.diff(p, axis=2))               # Dx[r, c] = |p[r, c + 1] - p[r, c]|, 0 in the last column
    Dy[:, :-1] = np.abs(np.diff(p, axis=1))
    taps_r = [np.minimum(rlo + k, rhi) for k in range(3)]
    taps_c = [np.minimum(clo + k, chi) for k in range(3)]
    cells_r = [np.minimum(rlo + k, np.maximum(rhi - 1, rlo)) for k in range(2)]    # rlo == rhi only at sh - 1: Dy is 0 there
    cells_c = [np.minimum(clo + k, np.maximum(chi - 1, clo)) for k in range(2)]

    def most(a, rs, cs):
        return np.max([a[:, r][:, :, c] for r in rs for c in cs], axis=0)
    Lx, Ly, pmax = most(Dx, taps_r, cells_c), most(Dy, cells_r, taps_c), most(p, taps_r, taps_c)
    if float64_only:
        x, y = np.abs(resize_coords(dw, sw)), np.abs(resize_coords(dh, sh))
        return (8. * U53 * (x + 1.))[None, None, :, None] * Lx + (8. * U53 * (y + 1.))[None, :, None, None] * Ly + 16. * U53 * pmax
    return (dX[None, None, :, None] * Lx + dY[None, :, None, None] * Ly
            + 2. * U25 * (1. + U24) * pmax + 16. * U53 * pmax)


# ---------------------------------------------------------------------------------------------------------------------
# the comparisons of tests/test_frames_f64.py (the CPU tests hand simulated wrong kernels to the same functions)

def count_differing(got, want):
    """number of elements whose BITS differ (same dtype and shape required; NaN == NaN, +0 != -0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    raw = np.dtype("u%d" % got.dtype.itemsize)
    return int((got.view(raw) != want.view(raw)).sum())


def check_resize(got32, exact64, bound, independent64):
    """float32 output of a resize against float32(resize_exact) and against an independent float64 value ->
    (indices of the elements off resize_exact's bits, how many of those are more than 1 float32 ulp off,
     worst |got - independent| / (bound + 2^-24 |independent|))"""
    got = np.ascontiguousarray(got32)
    assert got.dtype == F32 and got.shape == exact64.shape == bound.shape == independent64.shape
    want = exact64.astype(F32)
    off = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    far = 0
    for i in off:
        g, w = got[tuple(i)], want[tuple(i)]
        far += not (g == np.nextafter(w, F32(np.inf)) or g == np.nextafter(w, F32(-np.inf)))
    d = np.abs(got.astype(np.float64) - independent64)
    E = bound + U24 * np.abs(independent64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d <= E, np.where(E > 0, d / E, 0.), np.inf)
    return off, int(far), float(q.max())


def resize_passes(off, far, ratio, size):
    """the verdict of test_frames_f64.py on check_resize's figures: nothing beyond 1 ulp, at most 1e-6 of the elements off
    resize_exact's bits (none at all below a million elements), and the independent bound held"""
    return far == 0 and len(off) <= 1e-6 * size and ratio <= 1.
