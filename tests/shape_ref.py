"""NumPy restatement of the warp-shaping rule (include/dvsg_amd.h, "Warp shaping"): F_t [n,25,2] float32 -> F' [n,25,2]
float32.  Everything is float64 scalar arithmetic in explicit loops -- every product, sum and division a separate NumPy
scalar operation, hence rounded on its own; every sum sequential over i = 0..24 from 0.0 -- with strength and rigidity taken
as float32 and widened, and ONE rounding to float32 at the end."""
import numpy as np

MODELS = {"affine": 0, "similarity": 1, "translation": 2}
f64 = np.float64

V_SRC = np.array([[x, y] for y in (-1.0, -0.5, 0.0, 0.5, 1.0) for x in (-1.0, -0.5, 0.0, 0.5, 1.0)], dtype=np.float32)


def fit(d, model):
    """L [25,2] float64: the least-squares fit of `model` to the displacements d [25,2] float64 of one frame"""
    px = [f64(v) for v in V_SRC[:, 0]]
    py = [f64(v) for v in V_SRC[:, 1]]
    dx = [f64(v) for v in d[:, 0]]
    dy = [f64(v) for v in d[:, 1]]
    sx, sy = f64(0.0), f64(0.0)
    for i in range(25):
        sx = sx + dx[i]
        sy = sy + dy[i]
    mx, my = sx / f64(25.0), sy / f64(25.0)
    L = np.empty((25, 2), f64)
    if model == "translation":
        for i in range(25):
            L[i, 0], L[i, 1] = mx, my
    elif model == "similarity":
        sa, sb = f64(0.0), f64(0.0)
        for i in range(25):
            sa = sa + (px[i] * dx[i] + py[i] * dy[i])
            sb = sb + (px[i] * dy[i] - py[i] * dx[i])
        a, b = sa / f64(25.0), sb / f64(25.0)
        for i in range(25):
            L[i, 0] = (mx + a * px[i]) - b * py[i]
            L[i, 1] = (my + b * px[i]) + a * py[i]
    elif model == "affine":
        sxx, sxy, syx, syy = f64(0.0), f64(0.0), f64(0.0), f64(0.0)
        for i in range(25):
            sxx = sxx + px[i] * dx[i]
            sxy = sxy + py[i] * dx[i]
            syx = syx + px[i] * dy[i]
            syy = syy + py[i] * dy[i]
        axx, axy, ayx, ayy = sxx / f64(12.5), sxy / f64(12.5), syx / f64(12.5), syy / f64(12.5)
        for i in range(25):
            L[i, 0] = (mx + axx * px[i]) + axy * py[i]
            L[i, 1] = (my + ayx * px[i]) + ayy * py[i]
    else:
        raise ValueError("model %r" % (model,))
    return L


def shape(F, model="affine", strength=1.0, rigidity=0.0):
    """F' of the rule for F [n,25,2] (or [25,2]) float32"""
    F = np.asarray(F)
    assert F.dtype == np.float32 and F.shape[-2:] == (25, 2)
    s = f64(np.float32(strength))
    k = f64(1.0) - f64(np.float32(rigidity))
    flat = F.reshape(-1, 25, 2)
    out = np.empty(flat.shape, f64)
    with np.errstate(invalid="ignore"):
        for b in range(flat.shape[0]):
            d = flat[b].astype(f64)
            L = fit(d, model)
            for i in range(25):
                for c in range(2):
                    out[b, i, c] = s * (L[i, c] + k * (d[i, c] - L[i, c]))
    return out.astype(np.float32).reshape(F.shape)
