"""The 10-bit sample and word rules of the P010 render (include/dvsg_amd.h, "P010 frames") in NumPy, on the coordinate,
validity, weight and border-move functions of tests/bicubic_ref.py and tests/border_ref.py: every float32 operation below is
one NumPy float32 operation in the header's order.  x_s, y_s are INPUTS, as there.  `render_bilinear` and `render_bicubic`
give the value of every sample of a plane under a border mode; dtype=np.float64 evaluates the same formulas in float64 from
the same float32 x_s, y_s (replicate and mirror), for tests/test_p010_cpu.py.

A plane is [ph, pw, C] uint16 WORDS (the sample in the high 10 bits): luma (C = 1) or chroma (C = 2, centred on 512).
`P010Batch` is a seeded batch of surfaces with a byte pitch, a UV plane that need not follow the Y plane, and bytes between
the frames."""
import numpy as np

import bicubic_ref as R
import border_ref as B

f32 = np.float32


def samples(words, chroma, dtype=f32):
    """s = word >> 6; (float)s / 1023.0f, chroma (float)((int)s - 512) / 1023.0f"""
    s = np.asarray(words).astype(np.int32) >> 6
    return ((s - 512) if chroma else s).astype(dtype) / dtype(1023)


def to_word(v, chroma):
    """clamp(floor((double)v * 1023.0 + 0.5), 0, 1023) << 6, chroma + 512.5; NaN gives 0 -- both filters"""
    d = np.asarray(v, f32).astype(np.float64) * 1023.0 + (512.5 if chroma else 0.5)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(d), 0.0, np.clip(np.floor(d), 0.0, 1023.0))
    return (d.astype(np.uint16) << 6).astype(np.uint16)


def _cubic_at(s, x, y, dtype=f32):
    """steps 3-5 of the bicubic paragraph at (x, y) inside the plane of samples s of `dtype`"""
    ph, pw = s.shape[:2]
    x0f, y0f = np.floor(x), np.floor(y)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    weights = R.weights_f32 if dtype is f32 else R.weights_f64
    wx, wy = weights(x - x0f)[..., None], weights(y - y0f)[..., None]
    cols = [np.clip(x0 - 1 + k, 0, pw - 1) for k in range(4)]
    rows = [np.clip(y0 - 1 + r, 0, ph - 1) for r in range(4)]
    h = []
    for r in range(4):
        p = [s[rows[r], cols[k]] for k in range(4)]
        h.append(((wx[0] * p[0] + wx[1] * p[1]) + wx[2] * p[2]) + wx[3] * p[3])
    v = ((wy[0] * h[0] + wy[1] * h[1]) + wy[2] * h[2]) + wy[3] * h[3]
    assert v.dtype == dtype
    return v


def render_bicubic(plane, x_s, y_s, border, chroma, dtype=f32):
    """(v [oh, ow, C], written bool [oh, ow]) of the bicubic render of a plane of words under `border`.  dtype=np.float64
    (replicate and mirror only) evaluates the same formulas in float64 (w3 from its own polynomial) from the same float32
    x_s, y_s."""
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    s = samples(plane, chroma, dtype)
    ok = R.valid(ph, pw, x_s, y_s)
    if border in ("black", "keep"):
        assert dtype is f32
        x, y = R.coords(ph, pw, x_s, y_s)
        v = _cubic_at(s, np.where(ok, x, f32(0)), np.where(ok, y, f32(0)))
        return np.where(ok[..., None], v, f32(0)), (ok if border == "keep" else np.ones_like(ok))
    x, y = B.coords(ph, pw, x_s, y_s, dtype)
    nan = np.isnan(x) | np.isnan(y)
    xc = B.move(np.where(nan, dtype(0), x), pw, border, dtype)
    yc = B.move(np.where(nan, dtype(0), y), ph, border, dtype)
    return np.where(nan[..., None], dtype(0), _cubic_at(s, xc, yc, dtype)), np.ones_like(ok)


def _sampler_a(s, x_s, y_s):
    """plane_a_load and sampler A's blend on the float32 image s, its coordinate, clip and weight expressions in their order;
    0.0f where the sample is invalid"""
    ph, pw = s.shape[:2]
    x, y = R.coords(ph, pw, x_s, y_s)
    ok = R.valid(ph, pw, x_s, y_s)
    x, y = np.where(ok, x, f32(0)), np.where(ok, y, f32(0))
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, pw - 1), np.clip(x1, 0, pw - 1)
    y0, y1 = np.clip(y0, 0, ph - 1), np.clip(y1, 0, ph - 1)
    x0f, x1f, y0f, y1f = (a.astype(f32) for a in (x0, x1, y0, y1))
    wa, wb = ((x1f - x) * (y1f - y))[..., None], ((x1f - x) * (y - y0f))[..., None]
    wc, wd = ((x - x0f) * (y1f - y))[..., None], ((x - x0f) * (y - y0f))[..., None]
    v = ((wa * s[y0, x0] + wb * s[y1, x0]) + wc * s[y0, x1]) + wd * s[y1, x1]
    assert v.dtype == f32
    return np.where(ok[..., None], v, f32(0)), ok


def render_bilinear(plane, x_s, y_s, border, chroma, dtype=f32):
    """(v [oh, ow, C], written bool [oh, ow]) of the bilinear render of a plane of words under `border`: sampler A on the
    float image (black, keep), or border_ref's taps and weights at the moved coordinate (replicate, mirror; a NaN coordinate
    loads from (0, 0) and blends to 0).  dtype=np.float64 (replicate and mirror only) evaluates the same formulas in float64
    from the same float32 x_s, y_s."""
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    if border in ("black", "keep"):
        assert dtype is f32
        v, ok = _sampler_a(samples(plane, chroma), x_s, y_s)
        return v, (ok if border == "keep" else np.ones_like(ok))
    x, y = B.coords(ph, pw, x_s, y_s, dtype)
    nan = np.isnan(x) | np.isnan(y)
    xc = B.move(np.where(nan, dtype(0), x), pw, border, dtype)
    yc = B.move(np.where(nan, dtype(0), y), ph, border, dtype)
    v = B.bilinear_taps(samples(plane, chroma, dtype), xc, yc, dtype)
    return np.where(nan[..., None], dtype(0), v), np.ones(nan.shape, dtype=bool)


class P010Batch(object):
    """n P010 frames of H x W samples in one uint8 buffer [n, rows, pitch]: Y words in rows [0, H), UV words in rows
    [uv_row, uv_row + H / 2), `tail` rows behind them (frame_stride larger than the frame), `pitch` bytes per row (even,
    >= 2 W).  fill None: seeded samples in [0, 1023] with 0 and 1023 in both planes, `low` or-ed into every word's low 6
    bits, seeded bytes everywhere else; a byte value: every byte that."""

    def __init__(self, seed, n, H, W, pitch=None, uv_row=None, tail=0, low=0, fill=None):
        self.n, self.H, self.W = n, H, W
        self.pitch = 2 * W if pitch is None else pitch
        self.uv_row = H if uv_row is None else uv_row
        assert H % 2 == 0 and W % 2 == 0 and self.pitch >= 2 * W and self.pitch % 2 == 0 and self.uv_row >= H
        self.rows = self.uv_row + H // 2 + tail
        if fill is not None:
            self.buf = np.full((n, self.rows, self.pitch), fill, dtype=np.uint8)
            return
        rng = np.random.default_rng(seed)
        self.buf = rng.integers(0, 256, (n, self.rows, self.pitch), dtype=np.uint8)
        for lo, hi in ((0, H), (self.uv_row, self.uv_row + H // 2)):
            s = rng.integers(0, 1024, (n, hi - lo, W), dtype=np.uint16)
            s[:, 0, 0], s[:, 0, 1], s[:, -1, -2], s[:, -1, -1] = 0, 1023, 1023, 0
            self.buf[:, lo:hi, :2 * W] = ((s << 6) | np.uint16(low)).astype("<u2").view(np.uint8)

    @property
    def frame_stride(self):
        return self.rows * self.pitch

    @property
    def uv_offset(self):
        return self.uv_row * self.pitch

    def words(self, buf=None):
        """(luma [n, H, W, 1], chroma [n, H / 2, W / 2, 2]) uint16 copies of the two planes of `buf`"""
        buf = self.buf if buf is None else buf
        H, W, n = self.H, self.W, self.n
        y = np.ascontiguousarray(buf[:, :H, :2 * W]).view("<u2")
        uv = np.ascontiguousarray(buf[:, self.uv_row:self.uv_row + H // 2, :2 * W]).view("<u2")
        return y.reshape(n, H, W, 1), uv.reshape(n, H // 2, W // 2, 2)

    def outside(self, buf=None):
        """The bytes of `buf` that belong to neither plane: beyond 2 W of a row, between the planes, behind the frame."""
        buf = self.buf if buf is None else buf
        m = np.ones(buf.shape[1:], dtype=bool)
        m[:self.H, :2 * self.W] = False
        m[self.uv_row:self.uv_row + self.H // 2, :2 * self.W] = False
        return buf[:, m]
