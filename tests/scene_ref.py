"""NumPy restatement of the scene-cut step dvsg_scene_step_f32 (include/dvsg_amd.h, "ONLINE streams, SCENE CUTS"), and the
two test scenes.  The luma is float32 with every operation rounded on its own -- NumPy's float32 array arithmetic does not
fuse, the kernel is compiled with -ffp-contract=off -- and everything after the one quantisation is integer, so the bar against
the kernel is bit equality.  No oracle imports, no product kernels: only `online.stream_window_row`, which is host NumPy."""
import numpy as np

import inputs

F32 = np.float32
BINS = 64
STATE_INTS = 68   # k, cuts, S, 0, the previous histogram [64]


def luma_f32(rgb):
    """Y = fl(fl(fl(0.299f r) + fl(0.587f g)) + fl(0.114f b)) of float32 [..., 3]"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.float32
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    with np.errstate(all="ignore"):
        y = (F32(0.299) * r + F32(0.587) * g) + F32(0.114) * b
    assert y.dtype == np.float32
    return y


def quantise(y):
    """q = clamp((int)floorf(fl(Y 255f) + 0.5f), 0, 255) as int64; NaN -> 0"""
    with np.errstate(all="ignore"):
        t = np.floor(np.asarray(y, dtype=F32) * F32(255.0) + F32(0.5))
    assert t.dtype == np.float32
    t = np.where(np.isnan(t), F32(0.0), t)
    return np.clip(t, F32(0.0), F32(255.0)).astype(np.int64)


def histogram(frame):
    """64 bins of int32 counts over the pixels of a float32 frame [..., 3]: bin = q >> 2"""
    q = quantise(luma_f32(frame)).reshape(-1)
    return np.bincount(q >> 2, minlength=BINS).astype(np.int32)


def histogram_f64(frame):
    """The same histogram from a plain float64 evaluation: for inputs on which no float32 operation rounds across a bin edge
    (tests/test_scene_cpu.py uses exact dyadic ones) it equals `histogram`."""
    f = np.asarray(frame, dtype=np.float64)
    y = 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]
    t = np.floor(y * 255.0 + 0.5)
    t = np.where(np.isnan(t), 0.0, t)
    q = np.clip(t, 0.0, 255.0).astype(np.int64).reshape(-1)
    return np.bincount(q >> 2, minlength=BINS).astype(np.int32)


def distance(cur, prev):
    """S = sum_b |cur[b] - prev[b]|"""
    return int(np.abs(cur.astype(np.int64) - prev.astype(np.int64)).sum())


def threshold_count(threshold, H, W):
    """ceil(threshold 2 H W) in float64"""
    return int(np.ceil(np.float64(threshold) * np.float64(2 * H * W)))


def scene_step(pool, rings, skip, state, thr_count, min_len, zoom_state=None, crop_start=1.0):
    """One call for the B rows of a step.  pool float32 [n_pool,H,W,3] (read only); state int32 [n_state,68] and zoom_state
    float32 [n_state] (or None) are updated IN PLACE.  Returns (table int32 [B,S], out_slots int32 [B], cut int32 [B])."""
    from coupe.dvsg_amd.online import stream_window_row
    assert state.dtype == np.int32 and state.shape[1] == STATE_INTS
    skip = [int(s) for s in skip]
    S, span = len(skip), skip[-1]
    B, n_pool, n_state = len(rings), pool.shape[0], state.shape[0]
    table = np.full((B, S), -1, dtype=np.int32)
    out_slots = np.full(B, -1, dtype=np.int32)
    cut = np.zeros(B, dtype=np.int32)
    for b in range(B):
        r = int(rings[b])
        if not 0 <= r < n_state:
            continue
        base = r * (span + 2)
        if base + span + 1 >= n_pool:
            continue
        cur = histogram(pool[base + span + 1])
        k = int(state[r, 0])
        S_b = 0 if k == 0 else distance(cur, state[r, 4:])
        if k >= max(1, int(min_len)) and S_b >= int(thr_count):
            cut[b] = 1
            k = 0
            state[r, 1] += 1
            if zoom_state is not None:
                zoom_state[r] = F32(crop_start)
        table[b], out_slots[b] = stream_window_row(k, base, skip)
        state[r, 0], state[r, 2], state[r, 3] = k + 1, S_b, 0
        state[r, 4:] = cur
    return table, out_slots, cut


# ---- the test scenes: disjoint luma ranges, because smooth_frames draws independent frames (within-scene scores at
# 32 x 48 reach ~0.44).  Scene A's luma lies in [0.05, 0.45], scene B's in [0.55, 0.95]: no bin is shared, S = 2 H W.
H, W = 32, 48
THRESHOLD = 0.75


def scene_a(n=12, h=H, w=W):
    return (F32(0.05) + F32(0.4) * inputs.smooth_frames(4001, n, h, w)).astype(F32)


def scene_b(n=12, h=H, w=W):
    return (F32(0.55) + F32(0.4) * inputs.smooth_frames(4002, n, h, w)).astype(F32)


def scores(frames):
    """score = S / (2 H W) between consecutive frames of a float32 clip [N,H,W,3] -> float64 [N - 1]"""
    hs = [histogram(f) for f in frames]
    n_pix = frames.shape[1] * frames.shape[2]
    return np.array([distance(hs[i + 1], hs[i]) / (2.0 * n_pix) for i in range(len(hs) - 1)])
