"""The crop's NumPy reference (tests/crop_ref.py) against the oracle, without a GPU: known answers of the scan, the validity
predicate against sampler A itself, `crop_zoom`, the promise the margin makes, and three simulated wrong kernels.

The promise of the margin, as a condition (stated, not measured).  `free` says that every pixel of the PLAIN output grid
whose normalised Chebyshev distance from the centre is below `free` is valid.  A pixel of the grid zoomed by
z <= free - margin lies at a distance <= z, inside a cell of the plain grid whose four corners are at most one pixel further
out on each axis, i.e. (the margin is one pixel of the SHORTER axis, the larger of the two in normalised units) at a distance
< free: all four are valid.  The valid set 0 <= x < W - 1, 0 <= y < H - 1 is convex in source coordinates, so the zoomed
pixel is valid too PROVIDED the map deviates from its bilinear interpolation over that one cell by less than the corners'
distance to the border of the valid set.  A thin-plate spline of 25 control points with |F_t| <= 0.1 bends by ~1e-4 px
over a cell at these sizes; a map that folds or tears inside one cell breaks the promise.  The test below draws F_t in that
range and requires 0 invalid pixels on the zoomed grid, evaluated in float64."""
import numpy as np
import pytest

import crop_ref
import inputs as tin

F32 = np.float32
SIZES = ((36, 64), (45, 80), (288, 512))


def oracle_map(F, oh, ow):
    """float32 T of the float64 solve on V_src + F, and the float32 oracle's x_s, y_s [B, oh * ow]"""
    from oracle import thin_plate_spline as otps
    B = F.shape[0]
    coord = tin.v_src(B)
    rhs = (coord + F).astype(F32)
    T = otps.solve_system(coord.astype(np.float64), rhs.astype(np.float64), dtype=np.float64).astype(F32)
    xs, ys = otps.source_coords(T, coord, oh, ow)
    return coord, T, xs, ys


@pytest.mark.parametrize("H,W", [(36, 64), (45, 80)])
def test_zero_motion_loses_the_last_row_and_column(H, W):
    _, _, xs, ys = oracle_map(np.zeros((1, 25, 2), dtype=F32), H, W)
    n, kmin = crop_ref.scan(xs, ys, H, W, H, W)
    D = (H - 1) * (W - 1)
    assert n[0] == H + W - 1 and kmin[0] == D
    assert crop_ref.free(kmin, H, W)[0] == 1.0


def _inside_planes(B, H, W, oh, ow):
    """x_s, y_s that put every sample at the centre of the source: all valid"""
    return np.zeros((B, oh, ow), dtype=F32), np.zeros((B, oh, ow), dtype=F32)


@pytest.mark.parametrize("oh,ow,i,j", [(5, 9, 0, 0), (5, 9, 2, 4), (8, 6, 7, 1), (37, 64, 36, 20), (2, 2, 1, 0)])
def test_one_invalid_pixel_gives_its_key_and_none_gives_int32_max(oh, ow, i, j):
    H, W = 11, 13
    xs, ys = _inside_planes(2, H, W, oh, ow)
    n, kmin = crop_ref.scan(xs, ys, H, W, oh, ow)
    assert (n == 0).all() and (kmin == crop_ref.INT32_MAX).all()
    assert (crop_ref.free(kmin, oh, ow) == 1.0).all()
    xs[1, i, j] = 2.0                                         # x = 1.5 W: beyond the frame
    n, kmin = crop_ref.scan(xs, ys, H, W, oh, ow)
    want = max(abs(2 * j - (ow - 1)) * (oh - 1), abs(2 * i - (oh - 1)) * (ow - 1))
    assert n.tolist() == [0, 1] and kmin.tolist() == [crop_ref.INT32_MAX, want]
    xs[1, i, j] = np.nan
    ys[0, 0, 0] = np.nan
    n, kmin = crop_ref.scan(xs, ys, H, W, oh, ow)
    assert n.tolist() == [1, 1] and kmin[1] == want and kmin[0] == (oh - 1) * (ow - 1)


def test_one_row_or_one_column_of_source_has_no_valid_sample():
    xs = np.linspace(-1.5, 1.5, 40).astype(F32)
    assert not crop_ref.valid(xs, np.zeros_like(xs), 5, 1).any()
    assert not crop_ref.valid(np.zeros_like(xs), xs, 1, 5).any()


def predicate_samples(H, W, n, seed):
    """normalised x_s, y_s [1, 6 n]: anywhere near the frame, squeezed into the pixel cells [-1, 0) and [W-1, W) (rows
    alike), on integer pixel coordinates, and far outside"""
    rng = np.random.default_rng(seed)
    to_x = lambda px: (2.0 * px / W - 1.0)
    to_y = lambda py: (2.0 * py / H - 1.0)
    px = np.concatenate([rng.uniform(-2, W + 2, n), rng.uniform(-1, 0, n), rng.uniform(W - 1, W, n),
                         rng.integers(-2, W + 3, n).astype(np.float64), rng.uniform(0, W - 1, n), rng.uniform(-300, 300 + W, n)])
    py = np.concatenate([rng.uniform(-2, H + 2, n), rng.uniform(0, H - 1, n), rng.uniform(0, H - 1, n),
                         rng.integers(-2, H + 3, n).astype(np.float64), rng.uniform(H - 1, H, n), rng.uniform(-300, 300 + H, n)])
    flip = rng.random(px.size) < 0.3                         # the squeezed cells on the other axis too
    px2 = np.where(flip, rng.uniform(0, W - 1, px.size), px)
    py2 = np.where(flip, np.concatenate([rng.uniform(-1, 0, 3 * n), rng.uniform(H - 1, H, 3 * n)]), py)
    return to_x(px2).astype(F32)[None], to_y(py2).astype(F32)[None]


@pytest.mark.parametrize("H,W", [(36, 64), (7, 5), (2, 2), (288, 512)])
def test_predicate_is_sampler_a_on_an_image_of_ones(H, W):
    """valid <=> the oracle's interpolate_a of an all-ones image gives 1; invalid <=> it gives 0.  The four weights are
    separately rounded float32 products added in a fixed order, so "1" and "0" are held to the rounding of that sum,
    7 u sum |w| (the blend bound of tests/test_tps_f64.py), not to bit equality: the weights of a sample 300 px outside
    the frame are ~300 and cancel to ~1e-5, never to a value near 1."""
    from oracle import thin_plate_spline as otps
    xs, ys = predicate_samples(H, W, 2000, seed=H * W)
    v = otps.interpolate_a(np.ones((1, H, W, 1), dtype=F32), xs, ys)[0, :, 0].astype(np.float64)
    ok = crop_ref.valid(xs, ys, H, W)[0]
    x, y = crop_ref.pixel_coords(xs, ys, H, W)
    ax = np.maximum(np.maximum(-x[0], x[0] - (W - 1)), 0.0).astype(np.float64)   # distance to the frame's index range
    ay = np.maximum(np.maximum(-y[0], y[0] - (H - 1)), 0.0).astype(np.float64)
    wsum = (2.0 * ax + 1.0) * (2.0 * ay + 1.0)              # >= (|x1 - x| + |x - x0|)(|y1 - y| + |y - y0|) = sum |w|
    tol = 7.0 * 2.0 ** -24 * wsum
    assert ok.sum() >= 50 and (~ok).sum() >= 50
    assert (np.abs(v[ok] - 1.0) <= tol[ok]).all()
    assert (np.abs(v[~ok]) <= tol[~ok]).all() and tol.max() < 0.5
    exact = (v[ok] == 1.0).mean(), (v[~ok] == 0.0).mean()
    print("valid samples exactly 1: %.4f, invalid samples exactly 0: %.4f" % exact)
    # the cells the clip decides: [-1, 0) and [W-1, W) are invalid, [0, W-1) is valid
    assert not crop_ref.valid(F32(2.0 * -0.5 / W - 1.0), F32(0.0), H, W)
    assert not crop_ref.valid(F32(2.0 * (W - 0.5) / W - 1.0), F32(0.0), H, W)
    assert crop_ref.valid(F32(-1.0), F32(-1.0), H, W) == (H > 1 and W > 1)       # pixel (0, 0) exactly


def test_crop_zoom_margin_clamps_and_rounding():
    from coupe.dvsg_amd.clip import crop_zoom
    for fn in (crop_zoom, crop_ref.crop_zoom):
        assert fn([1.0, 0.9, 0.95], out_hw=(36, 64)) == F32(0.9 - 2.0 / 35)        # one pixel of the shorter axis
        assert fn([1.0, 0.9], out_hw=(64, 36)) == F32(0.9 - 2.0 / 35)
        assert fn([0.9], margin=0.0) == F32(0.9) and fn([0.9], margin=0.0).dtype == np.float32
        assert float(fn([0.9], margin=0.0)) != 0.9                                  # rounded to float32, once
        assert fn([0.55], margin=0.1) == F32(0.5) and fn([0.2], margin=0.0, crop_min=0.25) == F32(0.25)
        assert fn([1.0], margin=0.0) == F32(1.0) and fn([1.0], margin=0.0, crop_min=1.0) == F32(1.0)
        assert fn([1.0, 1.0], margin=-0.0) <= F32(1.0)
    for bad in (dict(free_=[]), dict(free_=[np.nan]), dict(free_=[0.5], margin=-1.0), dict(free_=[0.5], crop_min=0.0),
                dict(free_=[0.5], crop_min=1.5), dict(free_=[0.5])):
        kw = dict(bad)
        with pytest.raises(ValueError):
            crop_zoom(kw.pop("free_"), **kw)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("a", [0.0, 0.02, 0.05, 0.1])
def test_zoom_from_the_margin_leaves_no_border(H, W, a):
    """5 draws of F_t uniform in [-a, a]: scan of the float32 oracle's map on the plain grid, z = crop_zoom(free), then the
    float64 map on the grid zoomed by z shows no invalid pixel (the condition is in the docstring of this file)"""
    B = 5
    F = np.random.default_rng(int(a * 1000) + H).uniform(-a, a, (B, 25, 2)).astype(F32)
    coord, T, xs, ys = oracle_map(F, H, W)
    _, kmin = crop_ref.scan(xs, ys, H, W, H, W)
    fr = crop_ref.free(kmin, H, W)
    for b in range(B):                                        # each draw is a clip of its own
        z = crop_ref.crop_zoom(fr[b:b + 1], out_hw=(H, W))
        assert z > 0.5, "the draw hit crop_min: it says nothing about the margin"
        x64, y64 = crop_ref.map_f64(T[b:b + 1], coord[b:b + 1], H, W, z)
        n, _ = crop_ref.scan(x64.astype(F32), y64.astype(F32), H, W, H, W)
        assert n[0] == 0, (a, b, float(z), int(n[0]))


def test_float64_map_at_zoom_one_is_the_oracle_s():
    from oracle import thin_plate_spline as otps
    F = tin.control_vectors(3, 2)
    coord = tin.v_src(2)
    rhs = (coord + F).astype(F32)
    T64 = otps.solve_system(coord.astype(np.float64), rhs.astype(np.float64), dtype=np.float64)
    xo, yo = otps.source_coords_f64(coord, rhs, 9, 14)
    xm, ym = crop_ref.map_f64(T64, coord, 9, 14, 1.0)
    assert np.abs(xm.reshape(2, -1) - xo).max() < 1e-12 and np.abs(ym.reshape(2, -1) - yo).max() < 1e-12


@pytest.mark.parametrize("oh,ow", [(5, 9), (37, 64), (6, 259)])
def test_reference_rejects_three_wrong_kernels(oh, ow):
    """rows behind out_h in the last 4-row group counted; the clip at x < W in place of x < W - 1; the key without its
    aspect factors -- on a near-identity map plus one sample per frame squeezed into [W-1, W)"""
    H, W = oh, ow
    F = tin.control_vectors(oh, 2, scale=0.02)
    coord, T, xs, ys = oracle_map(F, oh, ow)
    xs = xs.reshape(2, oh, ow).copy()
    xs[:, 1, 1] = F32(2.0 * (W - 0.5) / W - 1.0)          # off the centre: the key of the centre is 0 with or without factors
    good = crop_ref.scan(xs, ys, H, W, oh, ow)
    pad = (-oh) % 4
    xp, yp = crop_ref.map_f64(T, coord, oh, ow, 1.0, rows=np.arange(oh, oh + pad))
    for mut in crop_ref.MUTANTS:
        got = crop_ref.scan(xs, ys, H, W, oh, ow, mut, xp.astype(F32), yp.astype(F32))
        differs = not (np.array_equal(got[0], good[0]) and np.array_equal(got[1], good[1]))
        assert differs, mut
