"""NumPy restatement of the shake measurement dvsg_shake_measure_u8 (include/dvsg_amd.h, "SHAKE") and of
coupe.dvsg_amd.shake.summary, and the NumPy-only test planes.  Nothing is imported from the product.  All of the rule is
integer arithmetic, so the bar against the kernels is bit equality.

1. Reduce.  With f = factor >= 1, h = H / f and w = W / f (integer division, trailing rows and columns dropped):
   r[i][j] = (sum of the f x f bytes + f*f/2) / (f*f), in uint8.  For f = 1 this is the plane itself.
2. Blocks.  Blocks are 16 x 16 on the reduced plane.  ny = (h - 2*margin_y) / 16, nx = (w - 2*margin_x) / 16, n_blk = ny*nx.
   Block (a, c) has its top-left at (margin_y + 16a, margin_x + 16c).  1 <= radius <= 16, both margins >= radius,
   1 <= n_blk <= 2048.
3. Match.  For a block of frame t at (y0, x0) and every (dy, dx) in [-R, R]^2:
   S(dy,dx) = sum over the 256 pixels |cur[y0+i][x0+j] - prev[y0+i+dy][x0+j+dx]|, at most 65280.  The best candidate is the
   minimum under the order (S, dy*dy + dx*dx, dy, dx): equal SADs resolve to the shortest vector, then the smallest dy, then
   the smallest dx.  So cur[y][x] looks like prev[y+dy][x+dx]: the vector says where the content came from.
4. Validity and the sixteenth-pel step.  A block is invalid when its best candidate lies on the search boundary (|dy| == R
   or |dx| == R).  Otherwise, with S0 the best SAD, Sxm / Sxp its left / right neighbours and Sym / Syp its upper / lower
   ones: cx = Sxm - 2*S0 + Sxp, and cy likewise, both >= 0.  The block is valid iff cx >= max(texture, 1) and
   cy >= max(texture, 1).  vx = 16*dx + floor((16*(Sxm - Sxp) + cx) / (2*cx)), and vy likewise: a floor with a possibly
   negative numerator; the fraction lies in [-8, 8].  Invalid blocks report (0, 0, 0); valid ones report (vx, vy, 1).
5. Global vector of a pair.  n_valid counts the valid blocks, ok = n_valid >= min_blocks (min_blocks >= 1).  gx is the lower
   median of vx over the valid blocks, the element of rank (n_valid - 1) / 2 in sorted order; gy the same for vy,
   independently.  The row is [gx, gy, n_valid, ok], with gx = gy = 0 when not ok.  Sixteenths of a reduced pixel per frame."""
import math

import numpy as np

BLOCK = 16


def reduce(plane, factor):
    """uint8 [H, W] -> uint8 [H / f, W / f]"""
    plane = np.asarray(plane)
    assert plane.dtype == np.uint8 and plane.ndim == 2 and factor >= 1
    f = int(factor)
    h, w = plane.shape[0] // f, plane.shape[1] // f
    s = plane[:h * f, :w * f].astype(np.int64).reshape(h, f, w, f).sum(axis=(1, 3))
    return ((s + f * f // 2) // (f * f)).astype(np.uint8)


def block_counts(h, w, margin_y, margin_x):
    return max(h - 2 * margin_y, 0) // BLOCK, max(w - 2 * margin_x, 0) // BLOCK


def sad_table(cur, prev, radius, margin_y, margin_x):
    """int64 [2R + 1, 2R + 1, ny, nx]: S(dy, dx) of every block, indexed [dy + R, dx + R]"""
    R = int(radius)
    ny, nx = block_counts(cur.shape[0], cur.shape[1], margin_y, margin_x)
    assert cur.shape == prev.shape and cur.dtype == prev.dtype == np.uint8
    assert 1 <= R <= 16 and margin_y >= R and margin_x >= R and 1 <= ny * nx <= 2048
    c = cur[margin_y:margin_y + BLOCK * ny, margin_x:margin_x + BLOCK * nx].astype(np.int64)
    S = np.empty((2 * R + 1, 2 * R + 1, ny, nx), dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            p = prev[margin_y + dy:margin_y + dy + BLOCK * ny, margin_x + dx:margin_x + dx + BLOCK * nx].astype(np.int64)
            S[dy + R, dx + R] = np.abs(c - p).reshape(ny, BLOCK, nx, BLOCK).sum(axis=(1, 3))
    return S


def subpel(s_minus, s0, s_plus, d):
    """(curvature, 16 d + floor((16 (S- - S+) + c) / (2 c))) of one axis; the second is None for c == 0"""
    c = int(s_minus) - 2 * int(s0) + int(s_plus)
    if c <= 0:
        return c, None
    return c, 16 * d + (16 * (int(s_minus) - int(s_plus)) + c) // (2 * c)    # Python's // floors


def block_row(S, radius, texture):
    """(vx, vy, valid) of one block from its table S [2R + 1, 2R + 1]"""
    R = int(radius)
    best = None
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            key = (int(S[dy + R, dx + R]), dy * dy + dx * dx, dy, dx)
            if best is None or key < best:
                best = key
    s0, _, dy, dx = best
    if abs(dy) == R or abs(dx) == R:
        return 0, 0, 0
    cx, vx = subpel(S[dy + R, dx + R - 1], s0, S[dy + R, dx + R + 1], dx)
    cy, vy = subpel(S[dy + R - 1, dx + R], s0, S[dy + R + 1, dx + R], dy)
    need = max(int(texture), 1)
    if cx < need or cy < need:
        return 0, 0, 0
    return vx, vy, 1


def match(cur, prev, radius, margin_y, margin_x, texture):
    """int32 [n_blk, 3]: (vx, vy, valid) of every block of the reduced plane `cur` against `prev`"""
    S = sad_table(cur, prev, radius, margin_y, margin_x)
    ny, nx = S.shape[2:]
    return np.array([block_row(S[:, :, a, c], radius, texture) for a in range(ny) for c in range(nx)], dtype=np.int32)


def lower_median(values):
    values = sorted(int(v) for v in values)
    return values[(len(values) - 1) // 2]


def global_vector(blocks, min_blocks):
    """int32 [4]: [gx, gy, n_valid, ok]"""
    assert min_blocks >= 1
    valid = blocks[blocks[:, 2] == 1]
    n_valid = len(valid)
    if n_valid < min_blocks:
        return np.array([0, 0, n_valid, 0], dtype=np.int32)
    return np.array([lower_median(valid[:, 0]), lower_median(valid[:, 1]), n_valid, 1], dtype=np.int32)


def measure(planes, factor, radius, margin_y, margin_x, texture, min_blocks):
    """The whole call on uint8 [n, H, W]: (vectors int32 [n - 1, 4], blocks int32 [n - 1, n_blk, 3])"""
    red = [reduce(p, factor) for p in planes]
    blocks = np.stack([match(red[t], red[t - 1], radius, margin_y, margin_x, texture) for t in range(1, len(red))])
    vectors = np.stack([global_vector(b, min_blocks) for b in blocks])
    return vectors, blocks


def default_geometry(H, W, factor=None, radius=12, margin=0.125):
    """(factor, margin_y, margin_x) of coupe.dvsg_amd.shake.measure's defaults"""
    f = max(1, -(-W // 512)) if factor is None else int(factor)
    h, w = H // f, W // f
    return f, max(radius, math.ceil(margin * h)), max(radius, math.ceil(margin * w))


def summary(vectors, factor, width):
    """coupe.dvsg_amd.shake.summary from rows [n - 1, 4]: exact integer sums, then one division and one square root each."""
    rows = [[int(v) for v in r] for r in np.asarray(vectors)]
    ok = [r for r in rows if r[3]]
    speed_sum = sum(r[0] * r[0] + r[1] * r[1] for r in ok)
    jitter_sum = jitter_n = 0
    for a, b in zip(rows[:-1], rows[1:]):
        if a[3] and b[3]:
            jitter_sum += (b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2
            jitter_n += 1
    speed = factor / 16 * math.sqrt(speed_sum / len(ok)) if ok else None
    jitter = factor / 16 * math.sqrt(jitter_sum / jitter_n) if jitter_n else None
    return dict(frames=len(rows) + 1, pairs=len(rows), lost=len(rows) - len(ok), speed_rms=speed, jitter_rms=jitter,
                speed_pct=None if speed is None else 100 * speed / width,
                jitter_pct=None if jitter is None else 100 * jitter / width)


# ---- test planes, NumPy only --------------------------------------------------------------------------------------

def box_blur(x, width):
    """One pass of a width x width box mean over float64 [H, W], wrapping at the edges (the size stays)."""
    r = width // 2
    for axis in (0, 1):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r + 1, r)
        c = np.cumsum(np.pad(x, pad, mode="wrap"), axis=axis)
        n = x.shape[axis]
        hi = np.take(c, np.arange(width, width + n), axis=axis)
        lo = np.take(c, np.arange(0, n), axis=axis)
        x = (hi - lo) / width
    return x


def texture(seed, H, W, box=5):
    """uint8 [H, W]: three passes of a `box`-wide box blur over seeded noise, stretched to [0, 255].  box=17 for planes that
    are then reduced."""
    x = np.random.RandomState(seed).randint(0, 256, size=(H, W)).astype(np.float64)
    for _ in range(3):
        x = box_blur(x, box)
    x = (x - x.min()) / (x.max() - x.min())
    return np.floor(x * 255.0 + 0.5).astype(np.uint8)


def shifted(big, oy, ox, H, W, pad):
    """The H x W window of `big` at (pad + oy, pad + ox): against the window at (pad, pad) as the previous frame its content
    came from (dy, dx) = (oy, ox)."""
    assert 0 <= pad + oy and pad + oy + H <= big.shape[0] and 0 <= pad + ox and pad + ox + W <= big.shape[1]
    return np.ascontiguousarray(big[pad + oy:pad + oy + H, pad + ox:pad + ox + W])


def shifted_subpel(big, oy, ox, H, W, pad):
    """The same for a fractional (oy, ox) >= the integer part: the bilinear blend of the four integer windows, rounded."""
    iy, ix = math.floor(oy), math.floor(ox)
    ay, ax = oy - iy, ox - ix
    out = np.zeros((H, W), dtype=np.float64)
    for sy, wy in ((0, 1 - ay), (1, ay)):
        for sx, wx in ((0, 1 - ax), (1, ax)):
            if wy * wx:
                out += wy * wx * shifted(big, iy + sy, ix + sx, H, W, pad).astype(np.float64)
    return np.floor(out + 0.5).astype(np.uint8)


def stripes(H, W, period=8):
    """Vertical stripes: every row the same, so no block has an edge in y."""
    row = np.where((np.arange(W) // (period // 2)) % 2 == 0, 40, 200).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row, (H, W)))


def checkerboard(H, W, cell=2):
    """A checkerboard of `cell`-pixel squares: its period is 2 cell in both directions."""
    y, x = np.mgrid[0:H, 0:W]
    return np.where(((y // cell) + (x // cell)) % 2 == 0, 30, 220).astype(np.uint8)
