"""No-GPU checks of the online crop: the ratchet's NumPy restatement (tests/ratchet_ref.py) against `crop_zoom`, the draws
of the GPU border-free test against the oracle, and the new entry points and OnlineStabilizer's crop options rejecting bad
arguments before any device work."""
import numpy as np
import pytest

import crop_ref
import inputs as tin
import ratchet_ref

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# a pure ratchet ends at crop_zoom of the whole stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("planes", [1, 2])
def test_pure_ratchet_ends_at_crop_zoom_of_all_frames(seed, planes):
    """recover = 0, start 1.0: after the last frame the state is crop_zoom(all frees, margin, crop_min) bit for bit -- min
    and max commute and the float32 rounding is monotone -- for the product's crop_zoom and the reference's alike; the
    zoom sequence never increases."""
    from coupe.dvsg_amd.clip import crop_zoom
    rng = np.random.default_rng(seed)
    H, W = (36, 64) if seed % 2 else (72, 128)
    (lh, lw), (ch, cw) = ratchet_ref.plane_grids(H, W)
    Da, Db = (lh - 1) * (lw - 1), (ch - 1) * (cw - 1)
    N = 200
    lo = 0.3 if seed >= 6 else 0.7                           # the last two sequences dip below crop_min + margin
    ka = (rng.uniform(lo, 1.2, N) * Da).astype(np.int64)     # values above D too
    kb = (rng.uniform(lo, 1.2, N) * Db).astype(np.int64)
    ka[rng.integers(0, N, 5)] = crop_ref.INT32_MAX
    margin, crop_min = (ratchet_ref.nv12_margin(H, W), 0.5) if seed % 3 else (0.0, 0.6)
    state = np.array([0.25, 1.0, 0.25], dtype=F32)
    zooms, frees = [], []
    for k in range(N):
        z, f, w = ratchet_ref.ratchet(state, [1], ka[k:k + 1], Da, kb[k:k + 1] if planes == 2 else None, Db, margin, crop_min, 0.0)
        assert w[0] and z[0] == state[1] and z.dtype == np.float32
        zooms.append(z[0])
        frees.append(f[0])
    want_free = crop_ref.free(ka, lh, lw) if planes == 1 else ratchet_ref.free_of_keys(ka, kb, H, W)
    assert np.array_equal(np.array(frees), want_free)
    assert (np.diff(np.array(zooms, dtype=np.float64)) <= 0).all()
    for fn in (crop_zoom, crop_ref.crop_zoom):
        want = fn(want_free, margin=margin, crop_min=crop_min)
        assert want.dtype == np.float32 and state[1].tobytes() == want.tobytes(), (state[1], want)
    assert state[0] == F32(0.25) and state[2] == F32(0.25)
    if seed >= 6:
        assert state[1] == F32(crop_min), "crop_min was meant to bind"


def test_ratchet_recover_start_and_skipped_slots():
    st = np.array([0.8, 1.0], dtype=F32)
    D = 100
    z, f, w = ratchet_ref.ratchet(st, [0, 5, 1], [50, 60, 100], D, margin=0.1, crop_min=0.5, recover=0.0)
    assert w.tolist() == [True, False, True] and np.isnan(z[1]) and np.isnan(f[1])
    assert z[0] == F32(0.5) and z[2] == F32(1.0 - 0.1) and f.tolist()[::2] == [0.5, 1.0]
    # recover > 0: the zoom climbs back by at most `recover` per frame, never above the frame's own target
    st = np.array([0.6], dtype=F32)
    seq = [ratchet_ref.ratchet(st, [0], [D], D, margin=0.0, crop_min=0.5, recover=0.125)[0][0] for _ in range(5)]
    assert seq == [F32(float(F32(0.6)) + 0.125), F32(float(F32(float(F32(0.6)) + 0.125)) + 0.125),
                   F32(float(F32(float(F32(float(F32(0.6)) + 0.125)) + 0.125)) + 0.125), F32(1.0), F32(1.0)]
    # a start below the first target holds (crop_start)
    st = np.array([0.8], dtype=F32)
    assert ratchet_ref.ratchet(st, [0], [D], D, margin=0.0)[0][0] == F32(0.8)


# ---------------------------------------------------------------------------------------------------------------------
# the draws of the GPU border-free test: the reference itself leaves no border on either grid
# ---------------------------------------------------------------------------------------------------------------------
def test_there_are_at_least_twenty_draws_within_the_smooth_map_bound():
    assert len(ratchet_ref.BORDER_FREE_DRAWS) >= 20 and len(set(ratchet_ref.BORDER_FREE_DRAWS)) == len(ratchet_ref.BORDER_FREE_DRAWS)
    assert {d[:2] for d in ratchet_ref.BORDER_FREE_DRAWS} == {(36, 64), (72, 128)}
    for H, W, seed, a in ratchet_ref.BORDER_FREE_DRAWS:
        assert a <= 0.1 and np.abs(ratchet_ref.draw_F(seed, a)).max() <= 0.1


@pytest.mark.parametrize("H,W,seed,a", ratchet_ref.BORDER_FREE_DRAWS)
def test_reference_leaves_no_border_in_either_plane(H, W, seed, a):
    """float32 oracle scan of both planes -> free = the smaller -> crop_zoom with the chroma margin -> the float64 map on
    both zoomed grids: 0 invalid pixels, and the zoom is not crop_min's (the draw would say nothing about the margin)."""
    from oracle import thin_plate_spline as otps
    F = ratchet_ref.draw_F(seed, a)
    coord = tin.v_src(1)
    rhs = (coord + F).astype(F32)
    T = otps.solve_system(coord.astype(np.float64), rhs.astype(np.float64), dtype=np.float64).astype(F32)
    kmin = []
    for gh, gw in ratchet_ref.plane_grids(H, W):
        xs, ys = otps.source_coords(T, coord, gh, gw)
        kmin.append(crop_ref.scan(xs, ys, gh, gw, gh, gw)[1])
    free = ratchet_ref.free_of_keys(kmin[0], kmin[1], H, W)
    z = crop_ref.crop_zoom(free, margin=ratchet_ref.nv12_margin(H, W))
    assert 0.5 < z < 1.0
    for gh, gw in ratchet_ref.plane_grids(H, W):
        x64, y64 = crop_ref.map_f64(T, coord, gh, gw, z)
        n, _ = crop_ref.scan(x64.astype(F32), y64.astype(F32), gh, gw, gh, gw)
        assert n[0] == 0, (gh, gw, float(z), int(n[0]))


def test_chroma_leaves_the_source_before_luma():
    """x_s valid up to 1 - 4/W on the chroma grid, 1 - 2/W on the luma grid: a sample between the two is a chroma border only"""
    H, W = 36, 64
    xs = F32(1.0 - 3.0 / W)
    assert crop_ref.valid(xs, F32(0.0), H, W) and not crop_ref.valid(xs, F32(0.0), H // 2, W // 2)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: status -1 and a telling message, no device work (pointers are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.dvsg_last_error_string()


def test_zoomed_render_rejects_bad_arguments(lib):
    f = lib.dvsg_tps_render_zoom_nv12
    #        net F  y  uv pitch stride n  H  W  zoom T  oy ouv opitch ostride stream
    assert f(None, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL net" in _err(lib)
    assert b"dvsg_tps_render_zoom_nv12" in _err(lib)
    assert f(8, None, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, None, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL source" in _err(lib)
    assert f(8, 8, 8, None, 8, 96, 1, 8, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL source" in _err(lib)
    assert b"dvsg_tps_render_zoom_nv12" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, None, 8, 8, 8, 96, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, None, 8, 8, 96, None) == -1 and b"NULL output" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, None, 8, 96, None) == -1 and b"NULL output" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 6, 5, 8, 8, 8, 8, 8, 96, None) == -1 and b"even" in _err(lib) and b"W=5" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 5, 6, 8, 8, 8, 8, 8, 96, None) == -1 and b"even" in _err(lib) and b"H=5" in _err(lib)
    assert f(8, 8, 8, 8, 7, 96, 1, 8, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"source pitch=7 < W=8" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 7, 96, None) == -1 and b"output pitch=7 < W=8" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 65536, 8, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"n=65536" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 2, 8, 8, 8, 8, 8, 8, 8, 8, None) == -1 and b"output frame_stride" in _err(lib)


def test_ratchet_rejects_bad_arguments(lib):
    f = lib.dvsg_crop_ratchet_f32
    #        ka D_a kb D_b slots n state n_state margin crop_min recover zoom free stream
    ok = [8, 100, None, 0, 8, 1, 8, 4, 0.0, 0.5, 0.0, 8, 8, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    for pos in (0, 4, 6, 11, 12):
        assert call(**{"p%d" % pos: None}) == -1 and b"NULL" in _err(lib), pos
    assert call(p9=0.0) == -1 and b"crop_min=0" in _err(lib)
    assert call(p9=1.5) == -1 and b"crop_min" in _err(lib)
    assert call(p9=float("nan")) == -1 and b"crop_min" in _err(lib)
    assert call(p8=-0.01) == -1 and b"margin=-0.01" in _err(lib)
    assert call(p8=float("nan")) == -1 and b"margin" in _err(lib)
    assert call(p10=-1.0) == -1 and b"recover" in _err(lib)
    assert call(p1=0) == -1 and b"D_a=0" in _err(lib)
    assert call(p2=8, p3=0) == -1 and b"D_b=0" in _err(lib)
    assert call(p5=0) == -1 and b"n=0" in _err(lib)
    assert call(p7=0) == -1 and b"n_state=0" in _err(lib)


def test_coefficients_rejects_bad_arguments(lib):
    f = lib.dvsg_tps_coefficients_f32
    assert f(None, 8, 1, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, None, 1, 8, None) == -1 and f(8, 8, 1, None, None) == -1
    assert f(8, 8, 0, 8, None) == -1 and b"n=0" in _err(lib)


def test_online_crop_options_raise_before_the_device():
    """A StabNet without weights needs no device: the crop checks come first, with stabilize_clip's wording."""
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = StabNet(32, 48)
    for bad in ("AUTO", 0, 1.5, True, -0.5, float("nan"), [0.9]):
        with pytest.raises(ValueError, match="crop must be None, 'auto' or a zoom in") as e:
            OnlineStabilizer(model, crop=bad)
        with pytest.raises(ValueError) as c:
            stabilize_clip(model, None, np.zeros((1, 32, 48, 3), np.uint8), crop=bad)
        assert str(e.value) == str(c.value)
        with pytest.raises(ValueError, match="crop must be"):
            OnlineStabilizer(model, frame_format="nv12", crop=bad)
    for kw in (dict(crop_margin=-0.1), dict(crop_min=0.0), dict(crop_min=1.5), dict(crop_start=0.0), dict(crop_start=1.1),
               dict(crop_recover=-1.0), dict(crop_recover=float("nan"))):
        with pytest.raises(ValueError, match="crop_"):
            OnlineStabilizer(model, crop="auto", **kw)
