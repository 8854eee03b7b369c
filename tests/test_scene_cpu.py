"""No-GPU checks of the scene-cut step: the NumPy restatement (tests/scene_ref.py) against a float64 evaluation and known
answers, the two test scenes' conditions, the state machine, and the new entry points and OnlineStabilizer's options
rejecting bad arguments before any device work."""
import ctypes

import numpy as np
import pytest

import scene_ref

F32 = np.float32
SKIP = (0, 16, 24, 28, 30, 31, 32)
SPAN = 32


# ---------------------------------------------------------------------------------------------------------------------
# the histogram
# ---------------------------------------------------------------------------------------------------------------------
def test_histogram_equals_float64_on_dyadic_inputs():
    """Inputs j / 256 are exact in float32.  The float32 luma differs from the float64 one by the roundings of 0.299f, 0.587f,
    0.114f and of seven operations on values <= 256: below 7 * 256 * 2^-24 = 1.1e-4 in t = 255 Y + 0.5.  The draw keeps every
    float64 t further than 1e-3 from a bin edge (a multiple of 4), so both evaluations must put every pixel in the same bin."""
    rng = np.random.default_rng(7)
    frame = (rng.integers(0, 257, (32, 48, 3)) / 256.0).astype(F32)
    f = frame.astype(np.float64)
    t = (0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]) * 255.0 + 0.5
    assert np.abs(t - 4.0 * np.round(t / 4.0)).min() > 1e-3, "the draw has a pixel on a bin edge: take another seed"
    got = scene_ref.histogram(frame)
    assert got.dtype == np.int32 and got.shape == (64,) and got.sum() == 32 * 48
    assert np.array_equal(got, scene_ref.histogram_f64(frame))
    assert (got > 0).sum() > 30


def test_histogram_known_answers():
    n = 5 * 7
    h = scene_ref.histogram(np.zeros((5, 7, 3), F32))
    assert h[0] == n and h.sum() == n
    h = scene_ref.histogram(np.ones((5, 7, 3), F32))
    assert h[63] == n and h.sum() == n
    h = scene_ref.histogram(np.full((5, 7, 3), np.nan, F32))
    assert h[0] == n and h.sum() == n
    one_nan = np.ones((5, 7, 3), F32)
    one_nan[2, 3, 1] = np.nan                                    # one NaN channel poisons its pixel's luma only
    h = scene_ref.histogram(one_nan)
    assert h[0] == 1 and h[63] == n - 1
    for v, b in ((7.5, 63), (np.inf, 63), (-0.25, 0), (-np.inf, 0), (1e30, 63), (-1e30, 0)):
        h = scene_ref.histogram(np.full((5, 7, 3), v, F32))
        assert h[b] == n and h.sum() == n, v
    # q = 3 and q = 4 straddle the first bin edge: Y 255 + 0.5 = 3.5 + ... and 4.5 + ...
    assert scene_ref.quantise(np.array([3.2 / 255, 3.6 / 255, 254.4 / 255, 254.6 / 255], F32)).tolist() == [3, 4, 254, 255]


def test_the_scenes_are_separated_by_the_threshold():
    """The conditions the GPU tests rest on, stated in the issue: S = 2 H W exactly across the cut (score 1.0) and every
    within-scene score below 0.6, so threshold 0.75 separates them."""
    A, B = scene_ref.scene_a(), scene_ref.scene_b()
    assert A.shape == B.shape == (12, 32, 48, 3) and A.dtype == B.dtype == np.float32
    n_pix = 32 * 48
    assert scene_ref.distance(scene_ref.histogram(B[0]), scene_ref.histogram(A[-1])) == 2 * n_pix
    sa, sb = scene_ref.scores(A), scene_ref.scores(B)
    assert sa.max() < 0.6 and sb.max() < 0.6, (sa.max(), sb.max())
    assert scene_ref.scores(np.concatenate([A, B]))[11] == 1.0
    assert scene_ref.threshold_count(0.75, 32, 48) == 2304
    assert scene_ref.threshold_count(1.0, 32, 48) == 2 * n_pix and scene_ref.threshold_count(1e-9, 32, 48) == 1
    from coupe.dvsg_amd.online import scene_threshold_count
    for thr in (0.75, 1.0, 1e-9, 0.3333):
        assert scene_threshold_count(thr, 32, 48) == scene_ref.threshold_count(thr, 32, 48)


# ---------------------------------------------------------------------------------------------------------------------
# the state machine
# ---------------------------------------------------------------------------------------------------------------------
def _pool(n_rings=2, H=4, W=4):
    return np.zeros((n_rings * (SPAN + 2), H, W, 3), F32)


def _push(pool, state, value, ring=0, thr=32, min_len=1, zoom=None, crop_start=1.0):
    pool[ring * (SPAN + 2) + SPAN + 1] = value
    t, o, c = scene_ref.scene_step(pool, [ring], SKIP, state, thr, min_len, zoom, crop_start)
    return t[0], int(o[0]), int(c[0])


def test_state_machine_counts_cuts_and_restarts_the_window():
    from coupe.dvsg_amd.online import stream_window_row
    pool, state = _pool(), np.zeros((2, 68), np.int32)
    zoom = np.array([0.7, 0.6], F32)
    seq = [0.0, 0.0, 0.0, 1.0, 1.0, 0.0]         # cuts at frames 3 and 5
    want_k = [0, 1, 2, 0, 1, 0]
    for i, v in enumerate(seq):
        t, o, c = _push(pool, state, v, zoom=zoom, crop_start=0.9)
        row, out = stream_window_row(want_k[i], 0, SKIP)
        assert np.array_equal(t, row) and o == out and c == (1 if i in (3, 5) else 0), i
        assert state[0, 0] == want_k[i] + 1 and state[0, 3] == 0
        assert state[0, 2] == (32 if i in (3, 5) else 0)
        assert zoom[0] == (F32(0.7) if i < 3 else F32(0.9))
    assert state[0, 1] == 2 and state[0, 4] == 16 and state[0, 4:].sum() == 16
    assert not state[1].any() and zoom[1] == F32(0.6)
    # step 0 reads the input slot only; step k >= 1 reads history slots of frames 0 .. k - 1 of the new run
    for k in range(1, 80):
        row, out = stream_window_row(k, 34, SKIP)
        hist = row[:-1] - 34
        live = {j % 33 for j in range(max(0, k - 33), k)}
        assert set(hist.tolist()) <= live and row[-1] == 34 + 33 and out - 34 == k % 33


def test_first_frame_never_cuts_and_min_len_suppresses():
    pool, state = _pool(), np.zeros((2, 68), np.int32)
    state[0, 4:] = 7                               # a stale histogram in a ring at k == 0 is not compared against
    assert _push(pool, state, 1.0, thr=1)[2] == 0 and state[0, 2] == 0 and state[0, 0] == 1
    # min_len = 3: cuts at k = 1, 2 are suppressed (S is still recorded), k = 3 cuts
    vals = [0.0, 1.0, 0.0]
    for k, v in enumerate(vals, start=1):
        want = 1 if k == 3 else 0
        assert _push(pool, state, v, thr=1, min_len=3)[2] == want, k
        assert state[0, 2] == 32
    assert state[0, 0] == 1 and state[0, 1] == 1
    # min_len = 0 behaves as 1
    st2 = np.zeros((2, 68), np.int32)
    assert _push(pool, st2, 0.0, min_len=0)[2] == 0
    assert _push(pool, st2, 1.0, min_len=0)[2] == 1


def test_full_threshold_needs_disjoint_histograms():
    pool, state = _pool(), np.zeros((2, 68), np.int32)
    half = np.zeros((4, 4, 3), F32)
    half[:2] = 1.0
    assert _push(pool, state, 0.0)[2] == 0
    assert _push(pool, state, half)[2] == 0 and state[0, 2] == 16     # S = H W: half the pixels moved
    assert _push(pool, state, half)[2] == 0 and state[0, 2] == 0
    full = np.full((4, 4, 3), 0.5, F32)
    assert _push(pool, state, full)[2] == 1 and state[0, 2] == 32     # S = 2 H W
    assert _push(pool, state, 0.0, thr=31)[2] == 1


def test_skipped_ring_touches_nothing():
    pool, state = _pool(), np.zeros((2, 68), np.int32)
    pool[SPAN + 1] = 1.0
    before = state.copy()
    zoom = np.array([0.5, 0.5], F32)
    t, o, c = scene_ref.scene_step(pool, [2, -1, 0], SKIP, state, 1, 1, zoom, 1.0)
    assert (t[:2] == -1).all() and o[:2].tolist() == [-1, -1] and c.tolist() == [0, 0, 0]
    assert np.array_equal(state[1], before[1]) and state[0, 0] == 1 and state[0, 4 + 63] == 16
    # a ring whose input slot lies outside the pool is skipped too
    t, o, c = scene_ref.scene_step(pool[:SPAN + 2 + 5], [1], SKIP, state, 1, 1)
    assert (t == -1).all() and o[0] == -1 and not state[1].any()


# ---------------------------------------------------------------------------------------------------------------------
# bad arguments: a status and a message, before any device work
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.dvsg_last_error_string()


def test_scene_step_rejects_bad_arguments(lib):
    f = lib.dvsg_scene_step_f32
    skip = (ctypes.c_int32 * 7)(*SKIP)
    #     pool n_pool H  W  rings B skip S state n_state thr min_len zoom start table out cut ws  bytes stream
    ok = [16, 34, 4, 4, 16, 1, skip, 7, 16, 1, 16, 1, None, 1.0, 16, 16, 16, 16, 256, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    for pos in (0, 4, 6, 8, 14, 15, 16, 17):
        assert call(**{"p%d" % pos: None}) == -1 and b"NULL" in _err(lib), pos
    assert call(p5=0) == -1 and b"B=0" in _err(lib)
    assert call(p5=-3) == -1 and b"B=-3" in _err(lib)
    assert call(p7=0) == -1 and b"S=0" in _err(lib)
    assert call(p7=17) == -1 and b"S=17" in _err(lib)
    assert call(p2=32768, p3=32768) == -1 and b"2 H W" in _err(lib)
    assert call(p2=0) == -1 and b"positive" in _err(lib)
    assert call(p10=0) == -1 and b"thr_count=0" in _err(lib)
    assert call(p10=33) == -1 and b"thr_count=33" in _err(lib)
    assert call(p10=-1) == -1 and b"thr_count=-1" in _err(lib)
    assert call(p11=-1) == -1 and b"min_len=-1" in _err(lib)
    assert call(p1=0) == -1 and b"n_pool=0" in _err(lib)
    assert call(p9=0) == -1 and b"n_state=0" in _err(lib)
    bad = (ctypes.c_int32 * 7)(0, 16, 16, 28, 30, 31, 32)
    assert call(p6=bad) == -1 and b"skip[2]=16" in _err(lib)
    assert call(p18=255) != 0 and b"256 needed" in _err(lib)
    assert call(p17=24) != 0 and b"aligned" in _err(lib)


def test_scene_workspace_bytes_rejects_bad_arguments(lib):
    f = lib.dvsg_scene_workspace_bytes
    n = ctypes.c_size_t(12345)
    assert f(3, None) == -1 and b"NULL" in _err(lib)
    assert f(0, ctypes.byref(n)) == -1 and b"B=0" in _err(lib)
    assert f(65536, ctypes.byref(n)) == -1 and b"B=65536" in _err(lib)
    assert n.value == 12345
    assert f(3, ctypes.byref(n)) == 0 and n.value == 3 * 64 * 4


@pytest.mark.parametrize("bad", [0, -0.1, 1.5, float("nan"), True, "auto", [0.5]])
def test_online_stabilizer_rejects_bad_scene_cut(bad):
    """Raised before the model's weights are looked at and before the device is touched: StabNet(32, 48) has neither."""
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    with pytest.raises(ValueError, match=r"scene_cut must be None or a threshold in \(0, 1\]"):
        OnlineStabilizer(StabNet(32, 48), scene_cut=bad)


@pytest.mark.parametrize("bad", [-1, 1.5, True, None])
def test_online_stabilizer_rejects_bad_scene_min_len(bad):
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    with pytest.raises(ValueError, match="scene_min_len must be an integer >= 0"):
        OnlineStabilizer(StabNet(32, 48), scene_cut=0.5, scene_min_len=bad)
