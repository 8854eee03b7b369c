"""The bicubic filter of the source-size renders (include/dvsg_amd.h, "Views and the render filter") restated in NumPy,
operation for operation: every float32 operation below is one NumPy float32 operation, in the header's order, so the
device's bytes and float32 bits are these.  x_s, y_s (the TPS map's normalised source coordinates of every output sample)
are INPUTS: on the GPU tests they come from the grid-only form of dvsg_tps_warp_zoom_f32.

A plane is [ph, pw, C] uint8: the RGB image (C = 3), NV12 luma (C = 1) or NV12 chroma (C = 2, samples centred on 128).

`render_f64` evaluates the same formula in float64 (weights, samples and sums), for error figures; `bilinear_f32` is sampler
A on the same plane, for the sharpness comparison."""
import numpy as np

f32 = np.float32
A = -0.75


def coords(ph, pw, x_s, y_s):
    """rule 1: float32 x, y"""
    x_s, y_s = np.asarray(x_s, f32), np.asarray(y_s, f32)
    x = ((x_s + f32(1)) * f32(pw)) / f32(2)
    y = ((y_s + f32(1)) * f32(ph)) / f32(2)
    return x, y


def valid(ph, pw, x_s, y_s):
    """rule 2: sample_a_valid -- 0 <= x < pw - 1, 0 <= y < ph - 1, not NaN (a NaN fails every comparison)"""
    x, y = coords(ph, pw, x_s, y_s)
    with np.errstate(invalid="ignore"):
        return (x >= f32(0)) & (x < f32(pw - 1)) & (y >= f32(0)) & (y < f32(ph - 1))


def weights_f32(t):
    """rule 3, float32: [4, ...] for the taps floor - 1 .. floor + 2"""
    t = np.asarray(t, f32)
    u = t + f32(1)
    w0 = ((f32(A) * u - f32(5 * A)) * u + f32(8 * A)) * u - f32(4 * A)
    w1 = ((f32(1.25) * t - f32(2.25)) * t) * t + f32(1)
    v = f32(1) - t
    w2 = ((f32(1.25) * v - f32(2.25)) * v) * v + f32(1)
    w3 = ((f32(1) - w0) - w1) - w2
    return np.stack([w0, w1, w2, w3])


def weights_f64(t):
    """the same polynomials in float64 (w3 from its own polynomial, not from the other three)"""
    t = np.asarray(t, np.float64)
    u, v, w = t + 1.0, 1.0 - t, 2.0 - t
    return np.stack([((A * u - 5 * A) * u + 8 * A) * u - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                     ((A + 2) * v - (A + 3)) * v * v + 1, ((A * w - 5 * A) * w + 8 * A) * w - 4 * A])


def samples(plane, chroma, dtype=f32):
    """rule 4: (float)b / 255.0f, chroma (float)((int)b - 128) / 255.0f"""
    p = np.asarray(plane)
    v = (p.astype(np.int32) - 128) if chroma else p.astype(np.int32)
    return v.astype(dtype) / dtype(255)


def _taps(ph, pw, x, y, ok):
    x0 = np.where(ok, np.floor(np.where(ok, x, 0)), 0).astype(np.int64)
    y0 = np.where(ok, np.floor(np.where(ok, y, 0)), 0).astype(np.int64)
    cols = [np.clip(x0 - 1 + k, 0, pw - 1) for k in range(4)]
    rows = [np.clip(y0 - 1 + r, 0, ph - 1) for r in range(4)]
    return x0, y0, cols, rows


def render_f32(plane, x_s, y_s, chroma=False):
    """rules 1-5: float32 [oh, ow, C] (x_s, y_s are [oh, ow]); an invalid sample is exactly 0.0f"""
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    x, y = coords(ph, pw, x_s, y_s)
    ok = valid(ph, pw, x_s, y_s)
    x0, y0, cols, rows = _taps(ph, pw, x, y, ok)
    with np.errstate(invalid="ignore", over="ignore"):
        wx = weights_f32(np.where(ok, x - x0.astype(f32), f32(0)))[..., None]
        wy = weights_f32(np.where(ok, y - y0.astype(f32), f32(0)))[..., None]
    s = samples(plane, chroma)
    h = []
    for r in range(4):
        p = [s[rows[r], cols[k]] for k in range(4)]
        h.append(((wx[0] * p[0] + wx[1] * p[1]) + wx[2] * p[2]) + wx[3] * p[3])
    v = ((wy[0] * h[0] + wy[1] * h[1]) + wy[2] * h[2]) + wy[3] * h[3]
    assert v.dtype == f32
    return np.where(ok[..., None], v, f32(0))


def render_f64(plane, x_s, y_s, chroma=False):
    """the same formula evaluated in float64 from the same float32 x_s, y_s (coordinates included)"""
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    ok = valid(ph, pw, x_s, y_s)
    x = (np.asarray(x_s, np.float64) + 1.0) * pw / 2.0
    y = (np.asarray(y_s, np.float64) + 1.0) * ph / 2.0
    x0, y0, cols, rows = _taps(ph, pw, x, y, ok)
    wx = weights_f64(np.where(ok, x - x0, 0.0))[..., None]
    wy = weights_f64(np.where(ok, y - y0, 0.0))[..., None]
    s = samples(plane, chroma, np.float64)
    v = 0.0
    for r in range(4):
        v = v + wy[r] * sum(wx[k] * s[rows[r], cols[k]] for k in range(4))
    return np.where(ok[..., None], v, 0.0)


def to_u8(v, chroma=False):
    """rule 6: clamp(floor((double)v * 255.0 + 0.5), 0, 255), chroma + 128.5; NaN gives 0"""
    d = np.asarray(v, f32).astype(np.float64) * 255.0 + (128.5 if chroma else 0.5)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(d), 0.0, np.clip(np.floor(d), 0.0, 255.0))
    return d.astype(np.uint8)


def bilinear_f32(plane, x_s, y_s, chroma=False):
    """sampler A (ThinPlateSpline.py:30-90) on the plane, float32 operation for operation: what the bilinear render blends"""
    plane = np.asarray(plane)
    ph, pw = plane.shape[:2]
    x, y = coords(ph, pw, x_s, y_s)
    with np.errstate(invalid="ignore"):
        x0 = np.clip(np.floor(np.nan_to_num(x)), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
        y0 = np.clip(np.floor(np.nan_to_num(y)), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, pw - 1), np.clip(y0 + 1, 0, ph - 1)
    x0, y0 = np.clip(x0, 0, pw - 1), np.clip(y0, 0, ph - 1)
    x0f, x1f, y0f, y1f = (a.astype(f32) for a in (x0, x1, y0, y1))
    wa, wb = ((x1f - x) * (y1f - y))[..., None], ((x1f - x) * (y - y0f))[..., None]
    wc, wd = ((x - x0f) * (y1f - y))[..., None], ((x - x0f) * (y - y0f))[..., None]
    s = samples(plane, chroma)
    return ((wa * s[y0, x0] + wb * s[y1, x0]) + wc * s[y0, x1]) + wd * s[y1, x1]
