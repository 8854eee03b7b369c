"""No-GPU checks of the NV12 frame format: the integer table and its known answers, the byte round trips of the render's
two planes, and the three entry points and OnlineStabilizer's options rejecting bad arguments before any device work."""
import numpy as np
import pytest

import nv12_ref


def test_table_is_the_rounded_decimals():
    for m in (nv12_ref.BT601, nv12_ref.BT709):
        assert nv12_ref.COEF[m] == tuple(int(round(c * 2 ** 20)) for c in nv12_ref.DECIMALS[m])
    assert nv12_ref.COEF[nv12_ref.BT601] == (1220542, 1673527, -852492, -409993, 2116026)
    assert nv12_ref.COEF[nv12_ref.BT709] == (1220945, 1879825, -558796, -223608, 2215014)


@pytest.mark.parametrize("m", [nv12_ref.BT601, nv12_ref.BT709])
def test_known_answers_and_saturation(m):
    assert nv12_ref.yuv_to_rgb(16, 128, 128, m).tolist() == [0, 0, 0]
    assert nv12_ref.yuv_to_rgb(235, 128, 128, m).tolist() == [255, 255, 255]
    # both ends: below black / above white on a neutral pixel, and the chroma extremes on a mid grey
    assert nv12_ref.yuv_to_rgb(0, 128, 128, m).tolist() == [0, 0, 0]
    assert nv12_ref.yuv_to_rgb(255, 128, 128, m).tolist() == [255, 255, 255]
    assert nv12_ref.yuv_to_rgb(128, 128, 255, m)[0] == 255 and nv12_ref.yuv_to_rgb(128, 128, 0, m)[0] == 0
    assert nv12_ref.yuv_to_rgb(128, 255, 128, m)[2] == 255 and nv12_ref.yuv_to_rgb(128, 0, 128, m)[2] == 0
    assert nv12_ref.yuv_to_rgb(16, 255, 255, m)[1] == 0 and nv12_ref.yuv_to_rgb(235, 0, 0, m)[1] == 255
    # grey stays grey and monotone
    g = nv12_ref.yuv_to_rgb(np.arange(256), 128, 128, m)
    assert (g[:, 0] == g[:, 1]).all() and (g[:, 1] == g[:, 2]).all() and (np.diff(g[:, 0].astype(int)) >= 0).all()


@pytest.mark.parametrize("m", [nv12_ref.BT601, nv12_ref.BT709])
def test_sums_fit_int32(m):
    """The largest intermediate magnitude over all (Y, U, V) is below 2^31 (and below 2^30, as the header says): every sum
    is monotone in each of Y, U, V, so the extremes sit at the corners of the cube."""
    cy, cvr, cvg, cug, cub = nv12_ref.COEF[m]
    corners = np.array([(y, u, v) for y in (0, 255) for u in (0, 255) for v in (0, 255)])
    big = max(int(np.abs(s).max()) for s in nv12_ref.sums(corners[:, 0], corners[:, 1], corners[:, 2], m))
    terms = max(239 * cy, 128 * abs(cvr), 128 * abs(cub), 128 * (abs(cvg) + abs(cug)))
    assert big < 2 ** 30 < 2 ** 31 and terms < 2 ** 30
    # the int32 restatement agrees with the int64 sums on a seeded sample and on the corners
    rng = np.random.default_rng(1)
    Y, U, V = (np.concatenate([rng.integers(0, 256, 1 << 16), corners[:, k]]) for k in range(3))
    want = np.clip(np.stack([s >> 20 for s in nv12_ref.sums(Y, U, V, m)], -1), 0, 255).astype(np.uint8)
    assert np.array_equal(nv12_ref.yuv_to_rgb(Y, U, V, m), want)


def test_plane_round_trips_are_exact():
    """Luma: uint8(float(Y / 255.) * 255.) == Y; chroma: floor(float((c - 128) / 255.) * 255. + 128.5) == c, for all 256
    bytes.  And the float32 image the render samples -- one correctly rounded float32 division of the exact integer -- is
    the float64 quotient rounded once, for every byte of either plane."""
    b = np.arange(256)
    yf = (b.astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal((yf.astype(np.float64) * 255.0).astype(np.uint8), b)
    cf = ((b.astype(np.float64) - 128.0) / 255.0).astype(np.float32)
    assert np.array_equal(np.clip(np.floor(cf.astype(np.float64) * 255.0 + 128.5), 0, 255).astype(np.int64), b)
    assert np.array_equal(b.astype(np.float32) / np.float32(255.0), yf)
    assert np.array_equal((b - 128).astype(np.float32) / np.float32(255.0), cf)


def test_ref_replicates_chroma_and_flips():
    b = nv12_ref.Batch(3, 2, 4, 6, pitch=8, uv_row=6)
    y, uv = b.planes()
    rgb = nv12_ref.nv12_to_rgb(y, uv, nv12_ref.BT709)
    assert rgb.shape == (2, 4, 6, 3) and b.frame_stride == 8 * 8 and b.uv_offset == 48
    for (f, i, j) in [(0, 0, 0), (1, 3, 5), (0, 2, 3), (1, 1, 4)]:
        want = nv12_ref.yuv_to_rgb(y[f, i, j], uv[f, i // 2, 2 * (j // 2)], uv[f, i // 2, 2 * (j // 2) + 1], nv12_ref.BT709)
        assert np.array_equal(rgb[f, i, j], want)
    assert np.array_equal(nv12_ref.nv12_to_rgb(y, uv, nv12_ref.BT709, 1), rgb[..., ::-1])


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: status -1 and a telling message, no device work (pointers are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.dvsg_last_error_string()


def test_convert_rejects_bad_arguments(lib):
    f = lib.dvsg_frames_nv12_to_rgb_u8
    #        y  uv pitch stride n  H  W  m flip dst stream
    assert f(None, 8, 8, 96, 1, 8, 8, 0, 0, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, None, 8, 96, 1, 8, 8, 0, 0, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 0, 0, None, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 96, 1, 7, 8, 0, 0, 8, None) == -1 and b"even" in _err(lib) and b"H=7" in _err(lib)
    assert f(8, 8, 10, 96, 1, 8, 9, 0, 0, 8, None) == -1 and b"even" in _err(lib) and b"W=9" in _err(lib)
    assert f(8, 8, 8, 96, 1, 2, 8, 0, 0, 8, None) == -1 and b"4x4" in _err(lib)
    assert f(8, 8, 7, 96, 1, 8, 8, 0, 0, 8, None) == -1 and b"pitch=7 < W=8" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 2, 0, 8, None) == -1 and b"matrix=2" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, -1, 0, 8, None) == -1 and b"matrix=-1" in _err(lib)
    assert f(8, 8, 8, 96, 65536, 8, 8, 0, 0, 8, None) == -1 and b"n=65536" in _err(lib)
    assert f(8, 8, 8, 96, 0, 8, 8, 0, 0, 8, None) == -1 and b"n=0" in _err(lib)
    assert f(8, 8, 8, 63, 2, 8, 8, 0, 0, 8, None) == -1 and b"frame_stride" in _err(lib)


def test_ingest_rejects_bad_arguments(lib):
    f = lib.dvsg_frames_ingest_nv12
    #        y  uv pitch stride n sH sW  m pool n_pool slots dH dW stream
    assert f(None, 8, 8, 96, 1, 8, 8, 0, 8, 4, 8, 8, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, None, 8, 96, 1, 8, 8, 0, 8, 4, 8, 8, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 0, None, 4, 8, 8, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 0, 8, 4, None, 8, 8, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 96, 1, 9, 8, 0, 8, 4, 8, 8, 8, None) == -1 and b"even" in _err(lib)
    assert f(8, 8, 12, 96, 1, 8, 11, 0, 8, 4, 8, 8, 8, None) == -1 and b"even" in _err(lib)
    assert f(8, 8, 6, 96, 1, 8, 8, 0, 8, 4, 8, 8, 8, None) == -1 and b"pitch=6 < W=8" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 5, 8, 4, 8, 8, 8, None) == -1 and b"matrix=5" in _err(lib)
    assert f(8, 8, 8, 96, 65536, 8, 8, 0, 8, 4, 8, 8, 8, None) == -1 and b"n=65536" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 0, 8, 0, 8, 8, 8, None) == -1 and b"n_pool=0" in _err(lib)
    assert f(8, 8, 8, 96, 1, 8, 8, 0, 8, 4, 8, 0, 8, None) == -1 and b"bad shape" in _err(lib)


def test_render_rejects_bad_arguments(lib):
    f = lib.dvsg_tps_render_nv12
    #        net F  y  uv pitch stride n  H  W  T  oy ouv opitch ostride stream
    assert f(None, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL net" in _err(lib)
    assert f(8, None, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, None, 8, 8, 96, 1, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL source" in _err(lib)
    assert f(8, 8, 8, None, 8, 96, 1, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"NULL source" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, None, 8, 8, 8, 96, None) == -1 and b"NULL" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, None, 8, 8, 96, None) == -1 and b"NULL output" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, None, 8, 96, None) == -1 and b"NULL output" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 6, 5, 8, 8, 8, 8, 96, None) == -1 and b"even" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 5, 6, 8, 8, 8, 8, 96, None) == -1 and b"even" in _err(lib)
    assert f(8, 8, 8, 8, 7, 96, 1, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"source pitch=7 < W=8" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 1, 8, 8, 8, 8, 8, 7, 96, None) == -1 and b"output pitch=7 < W=8" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 65536, 8, 8, 8, 8, 8, 8, 96, None) == -1 and b"n=65536" in _err(lib)
    assert f(8, 8, 8, 8, 8, 96, 2, 8, 8, 8, 8, 8, 8, 8, None) == -1 and b"output frame_stride" in _err(lib)


def test_online_options_raise_before_the_device():
    """A StabNet without weights needs no device; the NV12 option checks come before anything else."""
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    model = StabNet(32, 48)
    for kw, name in [(dict(side_by_side=True), "side_by_side"), (dict(as_uint8=True), "as_uint8"),
                     (dict(channel_order="bgr"), "channel_order")]:
        with pytest.raises(ValueError, match=name):
            OnlineStabilizer(model, frame_format="nv12", **kw)
    with pytest.raises(ValueError, match="frame_format"):
        OnlineStabilizer(model, frame_format="i420")
    with pytest.raises(ValueError, match="yuv_matrix"):
        OnlineStabilizer(model, frame_format="nv12", yuv_matrix="bt2020")
    assert stabilize_clips(model, [], frame_format="nv12") == []
