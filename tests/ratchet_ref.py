"""NumPy restatement of the per-stream zoom controller dvsg_crop_ratchet_f32 (include/dvsg_amd.h, "CROP"), and the fixed
draws of the border-free test.  Python floats are IEEE float64 and every operation below is rounded on its own, as the
kernel's are (-ffp-contract=off); np.float32(x) of a float64 rounds once, to nearest.  tests/crop_ref.py holds the scan,
`free` and `crop_zoom` this builds on and is left as it is."""
import numpy as np

import crop_ref

F32 = np.float32


def ratchet(state, slots, key_a, D_a, key_b=None, D_b=0, margin=0.0, crop_min=0.5, recover=0.0):
    """One call for the n frames of a step.  state: float32 [n_state], updated IN PLACE.  Returns (zoom float32 [n],
    free float64 [n], written bool [n]); a frame whose slot is outside [0, n_state) is skipped: written False, nothing of
    it set (zoom and free hold NaN there)."""
    assert state.dtype == np.float32
    n = len(slots)
    zoom, free, written = np.full(n, np.nan, dtype=F32), np.full(n, np.nan, dtype=np.float64), np.zeros(n, dtype=bool)
    for i in range(n):
        sl = int(slots[i])
        if not 0 <= sl < state.size:
            continue
        f = float(min(int(key_a[i]), int(D_a))) / float(D_a)
        if key_b is not None:
            fb = float(min(int(key_b[i]), int(D_b))) / float(D_b)
            f = fb if fb < f else f
        target = f - float(margin)
        target = target if target > float(crop_min) else float(crop_min)
        target = target if target < 1.0 else 1.0
        held = float(state[sl]) + float(recover)
        z = F32(target if target < held else held)
        state[sl] = zoom[i] = z
        free[i], written[i] = f, True
    return zoom, free, written


def nv12_margin(H, W):
    """the default margin of an NV12 stream: one pixel of the chroma grid's shorter axis"""
    return 2.0 / (min(H // 2, W // 2) - 1)


# The border-free test (tests/test_gpu_online_crop.py) renders these draws, F_t uniform in [-a, a] from
# default_rng(seed), (1, 25, 2), at luma H x W.  |F_t| <= 0.1 is DESIGN section 5.00000's smooth-map caveat: the margin
# promises a border-free zoomed grid only for a map that bends by much less than a pixel over one cell.  The seeds were
# chosen on the CPU so that the reference itself -- the float32 oracle's scan of both planes, crop_zoom with the NV12
# margin, then the float64 map on both zoomed grids -- leaves 0 invalid pixels in luma and in chroma
# (tests/test_online_crop_cpu.py repeats that for every draw); none is left out at run time.
BORDER_FREE_DRAWS = [(H, W, seed, a) for H, W in ((36, 64), (72, 128)) for seed, a in
                     ((1, 0.1), (2, 0.1), (3, 0.1), (4, 0.1), (5, 0.1), (6, 0.1), (7, 0.05), (8, 0.05), (9, 0.05), (10, 0.02),
                      (11, 0.1), (12, 0.1))]


def draw_F(seed, a):
    return np.random.default_rng(seed).uniform(-a, a, (1, 25, 2)).astype(F32)


def plane_grids(H, W):
    """the two grids of an NV12 frame: luma, chroma; each is scanned with the source and the output of its own size"""
    return (H, W), (H // 2, W // 2)


def free_of_keys(kmin_luma, kmin_chroma, H, W):
    (lh, lw), (ch, cw) = plane_grids(H, W)
    return np.minimum(crop_ref.free(kmin_luma, lh, lw), crop_ref.free(kmin_chroma, ch, cw))
