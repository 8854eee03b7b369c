"""The border modes of the source-size renders (include/dvsg_amd.h, "Border modes") restated in NumPy on the helpers of
tests/bicubic_ref.py: every float32 operation below is one NumPy float32 operation, in the header's order, so the device's
bytes and float32 bits are these.  x_s, y_s (the TPS map's normalised source coordinates of every output sample) are INPUTS,
as in bicubic_ref.

A plane is [ph, pw, C] uint8: the RGB image (C = 3), NV12 luma (C = 1) or NV12 chroma (C = 2, samples centred on 128).
`render(plane, x_s, y_s, border, bicubic, chroma)` gives (v float32 [oh, ow, C], written bool [oh, ow]): the value of
every sample and whether the render stores it ("keep" leaves an invalid sample to the caller's bytes).  dtype=np.float64
evaluates the same formulas in float64 from the same float32 x_s, y_s, for the rule's own properties."""
import numpy as np

import bicubic_ref as R

f32 = np.float32
BORDERS = {"black": 0, "replicate": 1, "mirror": 2, "keep": 3}


def coords(ph, pw, x_s, y_s, dtype=f32):
    """steps 1: sampler A's x, y"""
    if dtype is f32:
        return R.coords(ph, pw, x_s, y_s)
    return (np.asarray(x_s, dtype) + 1.0) * pw / 2.0, (np.asarray(y_s, dtype) + 1.0) * ph / 2.0


def move(x, n, border, dtype=f32):
    """xc of a coordinate x (no NaN) on an axis of n samples: one reflection (mirror), then the clamp into [0, n - 1]"""
    x = np.asarray(x, dtype)
    m = dtype(n - 1)
    if border == "mirror":
        x = np.where(x < dtype(0), -x, np.where(x > m, (m + m) - x, x))
    return np.minimum(np.maximum(x, dtype(0)), m).astype(dtype)


def bilinear_taps(s, xc, yc, dtype=f32):
    """the bilinear filter at (xc, yc) inside the image s [ph, pw, C] of samples of `dtype`: taps x0 and min(x0 + 1, pw - 1),
    the upper weight from the unclipped index, sampler A's blend"""
    ph, pw = s.shape[:2]
    assert s.dtype == dtype
    x0f, y0f = np.floor(xc), np.floor(yc)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, pw - 1), np.minimum(y0 + 1, ph - 1)
    one = dtype(1)
    wx0, wx1, wy0, wy1 = (x0f + one) - xc, xc - x0f, (y0f + one) - yc, yc - y0f
    wa, wb, wc, wd = ((wx0 * wy0)[..., None], (wx0 * wy1)[..., None], (wx1 * wy0)[..., None], (wx1 * wy1)[..., None])
    v = ((wa * s[y0, x0] + wb * s[y1, x0]) + wc * s[y0, x1]) + wd * s[y1, x1]
    assert v.dtype == dtype
    return v


def bilinear_at(plane, xc, yc, chroma=False, dtype=f32):
    """bilinear_taps on the samples of a plane of bytes"""
    return bilinear_taps(R.samples(np.asarray(plane), chroma, dtype), xc, yc, dtype)


def bicubic_at(plane, xc, yc, chroma=False, dtype=f32):
    """steps 3-5 of the bicubic paragraph at (xc, yc) inside the plane"""
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    x0f, y0f = np.floor(xc), np.floor(yc)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    weights = R.weights_f32 if dtype is f32 else R.weights_f64
    wx, wy = weights(xc - x0f)[..., None], weights(yc - y0f)[..., None]
    cols = [np.clip(x0 - 1 + k, 0, pw - 1) for k in range(4)]
    rows = [np.clip(y0 - 1 + r, 0, ph - 1) for r in range(4)]
    s = R.samples(plane, chroma, dtype)
    h = []
    for r in range(4):
        p = [s[rows[r], cols[k]] for k in range(4)]
        h.append(((wx[0] * p[0] + wx[1] * p[1]) + wx[2] * p[2]) + wx[3] * p[3])
    v = ((wy[0] * h[0] + wy[1] * h[1]) + wy[2] * h[2]) + wy[3] * h[3]
    assert v.dtype == dtype
    return v


def black(plane, x_s, y_s, bicubic, chroma=False):
    """DVSG_BORDER_BLACK in float32: sampler A (bilinear), or the bicubic paragraph"""
    return R.render_f32(plane, x_s, y_s, chroma) if bicubic else R.bilinear_f32(plane, x_s, y_s, chroma)


def render(plane, x_s, y_s, border, bicubic, chroma=False, dtype=f32):
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    ok = R.valid(ph, pw, x_s, y_s)
    if border in ("black", "keep"):
        assert dtype is f32
        return black(plane, x_s, y_s, bicubic, chroma), (ok if border == "keep" else np.ones_like(ok))
    x, y = coords(ph, pw, x_s, y_s, dtype)
    nan = np.isnan(x) | np.isnan(y)
    xc = move(np.where(nan, dtype(0), x), pw, border, dtype)
    yc = move(np.where(nan, dtype(0), y), ph, border, dtype)
    v = (bicubic_at if bicubic else bilinear_at)(plane, xc, yc, chroma, dtype)
    return np.where(nan[..., None], dtype(0), v), np.ones_like(ok)


def to_u8(v, bicubic, chroma=False):
    """the byte of a float32 value: the bicubic render rounds to nearest, the bilinear one truncates (np.uint8(v * 255.) in
    float64, saturating, NaN -> 0) except for chroma, which it re-centres and rounds: floor(v * 255. + 128.5)"""
    if bicubic or chroma:
        return R.to_u8(v, chroma)
    d = np.asarray(v, f32).astype(np.float64) * 255.0
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(d), 0.0, np.clip(d, 0.0, 255.0))
    return np.floor(d).astype(np.uint8)
