"""CPU side of tests/test_frames_f64.py: the NumPy references of tests/frames_ref.py against the oracle and against torch's
float64 bilinear interpolation, the facts about the uint8 conversion that choose the edge inputs, the case tables, eleven
simulated wrong kernels handed to the comparisons the GPU tests use, and the coverage table against the built library."""
import os
import re

import numpy as np
import pytest

import frames_ref as fr
import test_frames_f64 as t

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES_SRC = os.path.join(os.path.dirname(HERE), "coupe", "dvsg_amd", "csrc", "frames.hip")
CPU_ONLY_PAIR = ((1080, 1920), (288, 512))            # too slow for nothing on the GPU; the references meet it here


# ---------------------------------------------------------------------------------------------------------------------
# the case tables

def test_tables_meet_every_residue_and_the_asked_sizes():
    assert {3 * W % 4 for W in t.TO_U8_W} == {0, 1, 2, 3} and set(t.TO_U8_H) == {1, 3} and set(t.TO_U8_N) == {1, 2}
    for W, H, n in t.TO_U8_SHAPES:                      # every shape, the single row included, meets all four residues
        res = set()
        for dst_W, x0 in t.to_u8_layouts(W):
            assert dst_W >= x0 + W
            res |= t.row_residues(n * H, dst_W, x0)
        assert res == {0, 1, 2, 3}, (W, H, n)
    assert {t.row_residues(4, 2 * dw + 1, x0) == {0, 1, 2, 3} for _, (_, dw) in t.RESIZE_PAIRS for x0 in (0, 1, dw, dw + 1)} == {True}
    assert {(B * h * w * 3 * S) % 4 for S, B, h, w in t.GATHER_CASES if B > 1} == {0, 1, 2, 3}
    assert {(h * w * 3 * S) % 4 for S, B, h, w in t.GATHER_CASES} == {1, 2, 3}           # every seam between windows straddles a group
    for S, B, h, w in t.GATHER_CASES:
        idx = t.gather_indices(S, B, S + B + w)
        ok = fr.slot_ok(idx, t.N_POOL)
        assert ok.any() and (not ok.all() or (S, B) == (1, 1))
        if S > 1:
            assert not ok[:-1, -1].any() and not ok[1:, 0].any()
    assert {1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025} == set(t.U8F32_NPIX) and set(t.U8F32_OFFSETS) == {0, 1, 2, 3}
    for table in (t.SLOTS_EGRESS, t.SLOTS_INGEST):
        flat = [s for v in table.values() for s in v]
        assert {-1, t.N_POOL, t.N_POOL + 3} <= set(flat) and any(len(v) == 1 for v in table.values())
    assert any(len(set(v)) < len(v) for v in t.SLOTS_EGRESS.values())
    asked = [((1, 1), (3, 4)), ((1, 9), (5, 4)), ((7, 1), (3, 6)), ((2, 2), (9, 13)), ((3, 5), (3, 5)), ((17, 23), (32, 48)),
             ((48, 64), (32, 48)), ((45, 70), (32, 48)), ((64, 96), (32, 48)), ((20, 30), (40, 60)), ((67, 101), (37, 53)),
             ((300, 9), (8, 259))]
    assert t.RESIZE_PAIRS[:12] == asked and t.SAME_SIZE in asked
    # item 6: just above the cap of grid_for, and not by much
    cap = t.STRIDE_CAP
    n, H, W = t.BIG_U8F32
    assert cap < (n * H * W + 3) // 4 < 1.01 * cap
    B, S, h, w = t.BIG_GATHER
    assert cap < (B * h * w * 3 * S + 3) // 4 < 1.31 * cap
    n, sh, sw, dh, dw = t.BIG_RESIZE
    assert cap < n * dh * dw < 1.04 * cap
    assert "inline int grid_for(size_t items, int cap = 1 << 16)" in open(FRAMES_SRC).read()


# ---------------------------------------------------------------------------------------------------------------------
# the resize references

ALL_PAIRS = t.RESIZE_PAIRS + [CPU_ONLY_PAIR]
ALL_IDS = t.RESIZE_IDS + ["1080x1920-288x512"]


def _case(pair, kind, flip):
    if pair == CPU_ONLY_PAIR:
        (sh, sw), (dh, dw) = pair
        u = t.make_image(kind, 1, sh, sw, 11)
        return u, fr.resize_exact(u, dh, dw, flip), fr.resize_bound(u, dh, dw, flip), t.torch_bilinear(u, dh, dw, flip)
    return t.resize_case(pair, kind, flip)


@pytest.mark.parametrize("pair", ALL_PAIRS, ids=ALL_IDS)
def test_resize_exact_is_the_oracle_bit_for_bit(pair):
    from oracle import frames as oframes
    (sh, sw), (dh, dw) = pair
    for kind in t.IMAGE_KINDS:
        for flip in ((1,) if pair == CPU_ONLY_PAIR else (0, 1)):
            u, exact = _case(pair, kind, flip)[:2]
            want = np.stack([oframes.resize_linear(t.flipped(f, flip) / 255., dw, dh) for f in u])
            assert fr.count_differing(exact, want) == 0, (kind, flip)


@pytest.mark.parametrize("pair", ALL_PAIRS, ids=ALL_IDS)
def test_resize_geometric_is_torch_and_resize_exact_within_the_bound(pair):
    """the two float64 evaluations of the clamped bilinear map agree to the float64 part of the bound (the coordinate's own
    roundings times the adjacent difference, a few 2^-53 of the taps), and resize_exact lies within resize_bound of torch
    at every value"""
    (sh, sw), (dh, dw) = pair
    for kind in t.IMAGE_KINDS:
        worst64 = worst = 0.0
        for flip in ((1,) if pair == CPU_ONLY_PAIR else (0, 1)):
            u, exact, bound, indep = _case(pair, kind, flip)
            geo = fr.resize_geometric(u, dh, dw, flip)
            slack = fr.resize_bound(u, dh, dw, flip, float64_only=True)
            for a, E, what in ((geo, slack, "geometric"), (exact, bound, "exact")):
                d = np.abs(a - indep)
                assert (d <= E).all(), (kind, flip, what, float(d.max()), np.argwhere(~(d <= E))[:3].tolist())
            with np.errstate(divide="ignore", invalid="ignore"):
                worst64 = max(worst64, float(np.where(slack > 0, np.abs(geo - indep) / slack, 0.).max()))
                worst = max(worst, float(np.where(bound > 0, np.abs(exact - indep) / bound, 0.).max()))
        print("%s %s: |geometric - torch| / float64 slack %.3f, |exact - torch| / bound %.3f" % (ALL_IDS[ALL_PAIRS.index(pair)],
                                                                                                 kind, worst64, worst))


COMMON = sorted({3840, 2560, 1920, 1440, 1280, 960, 854, 640, 512, 2160, 1080, 810, 720, 540, 480, 360, 288})


def _coords32(n_dst, n_src, opencv):
    """float32 coordinates for destination sizes n_dst [D] x source sizes n_src [S] -> [D, S, max(n_dst)] (unused: NaN)"""
    n_dst, n_src = np.asarray(n_dst, dtype=np.float64)[:, None, None], np.asarray(n_src, dtype=np.float64)[None, :, None]
    scale = 1. / (n_dst / n_src) if opencv else n_src / n_dst
    d = np.arange(int(n_dst.max()), dtype=np.float64)[None, None, :]
    return np.where(d < n_dst, ((d + .5) * scale - .5), np.nan).astype(F32)


def test_two_spellings_of_the_scale_give_the_same_taps():
    """OpenCV computes the scale as 1. / (dw / sw), the kernel and the oracle as sw / dw.  The taps and the weight are
    functions of the float32 coordinate alone, so identical coordinates are identical taps.  Counted when this was
    written: 0 differing pairs of 159 201 with both sizes in 1..399, 0 of 289 of the usual video sizes."""
    small = np.arange(1, 400)
    differing = pairs = 0
    for chunk in np.array_split(small, 8):
        a, b = _coords32(chunk, small, False), _coords32(chunk, small, True)
        differing += int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())
        pairs += a.shape[0] * a.shape[1]
    assert pairs == 159201 and differing == 0, differing
    common = 0
    for nd in COMMON:
        a, b = _coords32([nd], COMMON, False), _coords32([nd], COMMON, True)
        common += int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())
    assert len(COMMON) ** 2 == 289 and common == 0, common
    print("scale spellings: 0 of %d small and 0 of %d common pairs differ" % (pairs, len(COMMON) ** 2))


# ---------------------------------------------------------------------------------------------------------------------
# to_u8

def test_to_u8_saturates_where_numpy_wraps():
    x = np.array([0., -0., 1., 1.5, -0.25, np.nan, np.inf, -np.inf, 256 / 255., 5e-324, 1e300, -1e300, 0.999999, 0.5, 1e-9])
    assert fr.to_u8(x).tolist() == [0, 0, 255, 255, 0, 0, 255, 0, 255, 0, 255, 0, 254, 127, 0]
    assert fr.to_u8(F32(np.nextafter(F32(1), F32(0)))) == 254 and fr.to_u8(np.nextafter(F32(1), F32(2))) == 255
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(fr.to_u8(fr.u8_to_f32(u, 0)), u)                  # eval.py:80 then :112 gives the byte back
    before = np.arange(2 * 3 * 5 * 3, dtype=np.uint8)
    rows = np.full((2, 3, 2, 3), 200, dtype=np.uint8)
    placed = fr.place_rows(before, rows, 5, 2)
    assert (placed[:, :, 2:4] == 200).all() and np.array_equal(placed[:, :, :2], before.reshape(2, 3, 5, 3)[:, :, :2])
    assert np.array_equal(placed[:, :, 4:], before.reshape(2, 3, 5, 3)[:, :, 4:])


def test_to_u8_edges_tell_truncation_from_rounding_and_float32_from_float64():
    k = np.arange(1, 256)
    at32 = (k / 255.).astype(F32)
    below32 = np.nextafter(at32, F32(-np.inf))
    assert np.array_equal(fr.to_u8(at32), k) and np.array_equal(fr.to_u8(below32), k - 1)
    assert np.array_equal(np.rint(below32.astype(np.float64) * 255.), k)    # a rounding conversion gives k for all 255
    at64 = k / 255.
    below64 = np.nextafter(at64, -np.inf)
    assert np.array_equal(fr.to_u8(below64), k - 1)
    assert np.array_equal(fr.to_u8(below64.astype(F32)), k)                 # a conversion that first rounds to float32 gives k
    assert (fr.to_u8(at64) >= k - 1).all()                                  # (k / 255.) * 255. may land just below k in float64
    e32, e64 = t.edge_values(np.float32), t.edge_values(np.float64)
    assert e32.dtype == F32 and e64.dtype == np.float64 and set(at32.tolist()) <= set(e32.tolist())
    assert set(below64.tolist()) <= set(e64.tolist()) and np.isnan(e32).any() and np.isinf(e64).sum() == 2


def test_no_float32_separates_a_float32_product_from_the_float64_product():
    """The kernel multiplies in float64.  Would a float32 product x * 255.f, rounded to float32 and truncated, ever give
    another byte for a float32 x in [0, 1]?  Only if the rounding lifts the product onto an integer k from below.  Near
    x = k / 255, consecutive floats x are 255 ulp(x) apart in the product, while just below k the float32 grid is 128 or
    256 ulp(x) wide (k = 255 x lies 7 or 8 binades above x), so half a grid step reaches at most 128 ulp(x) down from k:
    at most one float x per k has its exact product that close -- the float just below k / 255 (the next one down is
    another 255 ulp(x) away).  Checking that one (and its lower neighbour, for good measure) settles every x: its
    product lies at least half an ulp of k below k for all 255 k.  Found: 0 of 255.  Nobody needs to look for such inputs."""
    k = np.arange(1, 256)
    x = np.nextafter((k / 255.).astype(F32), F32(-np.inf))
    separating = 0
    for cand in (x, np.nextafter(x, F32(-np.inf))):
        p32 = (cand * F32(255)).astype(F32)
        separating += int((np.trunc(p32) != np.trunc(cand.astype(np.float64) * 255.)).sum())
        gap = k - cand.astype(np.float64) * 255.                            # exact: 24 x 8 bits fit a double
        assert (gap >= 0.5 * np.spacing(np.nextafter(k.astype(F32), F32(0))).astype(np.float64)).all()
    assert separating == 0


# ---------------------------------------------------------------------------------------------------------------------
# simulated wrong kernels, one defect each, against the comparisons of test_frames_f64.py

def sim_to_u8(x, flip, before, dst_W, x0, defect=None):
    """frames_to_u8_kernel group by group: four values of a row per thread, one packed store where the group is whole and
    its first byte on the 4-byte grid, bytes otherwise"""
    n, H, W, _ = x.shape
    rows, rv = n * H, 3 * W
    b = fr.to_u8(x).reshape(rows, rv)
    if defect == "to_u8_rounds":
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.nan_to_num(np.asarray(x, dtype=np.float64) * 255., nan=0., posinf=255., neginf=0.)
        b = np.rint(np.clip(d, 0., 255.)).astype(np.uint8).reshape(rows, rv)
    out = np.array(before, dtype=np.uint8).reshape(-1)
    for row in range(rows):
        d0 = row * 3 * dst_W + 3 * x0
        for v0 in range(0, rv, 4):
            whole = v0 + 4 <= rv
            if defect == "tail_group_dropped" and not whole:
                continue
            o = []
            for i in range(min(4, rv - v0)):
                v = v0 + i
                if flip and defect == "flip_per_group":
                    sv = min(v0 + (2, 1, 0, 3)[i], rv - 1)
                elif flip:
                    sv = 3 * (v // 3) + 2 - v % 3
                else:
                    sv = v
                o.append(b[row, sv])
            if defect == "packed_store_reversed" and whole and (d0 + v0) % 4 == 0:
                o = o[::-1]
            out[d0 + v0:d0 + v0 + len(o)] = o
    return out.reshape(n, H, dst_W, 3)


def sim_gather(pool, idx, defect=None):
    """window_gather_kernel: four consecutive floats per thread; the defect takes the index row of the group's first
    float for all four"""
    n_pool, h, w, _ = pool.shape
    B, S = idx.shape
    C = 3 * S
    pw = h * w * C
    e = np.arange(B * pw)
    b, rem = e // pw, e % pw
    pix, c = rem // C, rem % C
    row = (e // 4 * 4) // pw if defect == "straddling_group_one_index_row" else b
    f = idx[row, c // 3]
    ok = fr.slot_ok(f, n_pool)
    v = np.where(ok, pool[np.where(ok, f, 0), pix // w, pix % w, c % 3], F32(0))
    return v.astype(F32).reshape(B, h, w, C)


TO_U8_DEFECTS = ("to_u8_rounds", "tail_group_dropped", "packed_store_reversed", "flip_per_group")
# The shapes at which a defect cannot change a value, reasoned and then asserted:
#   tail_group_dropped       3 W % 4 == 0: there is no tail group (W = 4, 64)
#   packed_store_reversed    W = 1: three values, no whole group
#   flip_per_group           W = 1: the group IS the pixel
#   to_u8_rounds             none
TO_U8_NEUTRAL = {"to_u8_rounds": set(), "tail_group_dropped": {4, 64}, "packed_store_reversed": {1}, "flip_per_group": {1}}


@pytest.mark.parametrize("defect", TO_U8_DEFECTS)
def test_simulated_to_u8_defects_are_rejected(defect):
    neutral = set()
    for W, H, n in t.TO_U8_SHAPES:
        changed = 0
        for flip in (0, 1):
            for dst_W, x0 in t.to_u8_layouts(W):
                x = t.to_u8_values(np.float32, n, H, W, W * 100 + H * 10 + n + x0)
                before = t.byte_pattern(n * H * dst_W * 3)
                want = fr.place_rows(before, fr.to_u8(t.flipped(x, flip)), dst_W, x0)
                assert fr.count_differing(sim_to_u8(x, flip, before, dst_W, x0), want) == 0      # the simulation itself is right
                changed += fr.count_differing(sim_to_u8(x, flip, before, dst_W, x0, defect), want) > 0
        if not changed:
            neutral.add((W, H, n))
    assert {s[0] for s in neutral} == TO_U8_NEUTRAL[defect] and len(neutral) == 4 * len(TO_U8_NEUTRAL[defect]), sorted(neutral)
    assert len(t.TO_U8_SHAPES) - len(neutral) >= len(t.TO_U8_SHAPES) / 2
    print("%s: value-neutral at %s" % (defect, sorted(neutral)))


def test_simulated_gather_defect_is_rejected():
    """neutral exactly where there is no seam: B = 1"""
    neutral = []
    for S, B, h, w in t.GATHER_CASES:
        pool = np.random.default_rng(S * 100 + B * 10 + h).uniform(0.1, 1., (t.N_POOL, h, w, 3)).astype(F32)
        idx = t.gather_indices(S, B, S + B + w)
        want = fr.window_gather(pool, idx)
        assert fr.count_differing(sim_gather(pool, idx), want) == 0
        if fr.count_differing(sim_gather(pool, idx, "straddling_group_one_index_row"), want) == 0:
            neutral.append((S, B, h, w))
    assert neutral == [c for c in t.GATHER_CASES if c[1] == 1], neutral
    assert len(t.GATHER_CASES) - len(neutral) >= len(t.GATHER_CASES) / 2


def test_simulated_exchange_of_zero_fill_and_skip_is_rejected():
    """egress that skips a frame whose slot is outside the pool (instead of writing zeros) and ingest that zero-fills the
    uint8 half of such a frame (instead of writing nothing; the pool frame does not exist).  The "shapes" are the slot
    variants; neutral exactly where every slot is inside the pool."""
    H, W, dst_W, x0 = 3, 5, 12, 6
    pool = t.to_u8_values(np.float32, t.N_POOL, H, W, 3)
    neutral = []
    for name, slots in t.SLOTS_EGRESS.items():
        before = t.byte_pattern(len(slots) * H * dst_W * 3)
        rows = fr.to_u8(fr.egress_slots(pool, slots))
        want = fr.place_rows(before, rows, dst_W, x0)
        wrong = fr.ingest_u8_half(before, rows, slots, t.N_POOL, dst_W, x0)
        if fr.count_differing(wrong, want) == 0:
            neutral.append(name)
    assert neutral == ["permuted", "duplicated", "one"] and len(neutral) <= len(t.SLOTS_EGRESS) / 2
    neutral = []
    (sh, sw), (dh, dw) = pair = t.RESIZE_PAIRS[3]
    u, exact = t.resize_case(pair, "noise", 1)[:2]
    for name, slots in t.SLOTS_INGEST.items():
        n = len(slots)
        before = t.byte_pattern(n * dh * (2 * dw + 1) * 3)
        rows = fr.resize_u8_half(exact[:n], 1)
        want = fr.ingest_u8_half(before, rows, slots, t.N_POOL, 2 * dw + 1, 1)
        zeroed = np.where(fr.slot_ok(slots, t.N_POOL)[:, None, None, None], rows, 0)
        wrong = fr.place_rows(before, zeroed, 2 * dw + 1, 1)
        if fr.count_differing(wrong, want) == 0:
            neutral.append(name)
    assert neutral == ["permuted", "one"] and len(neutral) <= len(t.SLOTS_INGEST) / 2


# The size pairs at which a resize defect changes no bit of the float32 output and no byte of the uint8 half, at any of the
# three images and either flip.  What decides it, and then the list as computed (asserted, so a change of the tables shows):
#   weight_f64                float32(1 - w) is EXACT wherever the coordinate is >= 0.5: w is then a multiple of 2^-23 (the
#                             ulp of a float32 >= 0.5, or of its fractional part above 1), and 1 - w in [0, 1] needs multiples
#                             of 2^-24 at the most.  It rounds only for a coordinate in (0, 0.5) that is no short dyadic
#                             fraction: a scale below 2 / 3 on some axis, or a first centre at .1667 (scale 4 / 3).  So the
#                             float32 weight of OpenCV is visible in the first cell of an axis only.
#   scale_f32                 neutral where the quotient of the sizes is a float32 on both axes (or the axis has one source
#                             pixel and every tap is clamped)
#   lower_clamp_keeps_weight  neutral where no coordinate is negative: both axes reduce, or have one source pixel (the
#                             upper clamp zeroes the weight again)
#   columns_first             the order of the passes shows only through the last float64 bit: the float32 output never
#                             changed, the uint8 half does on the "flat" image, where the taps are equal and the
#                             truncation turns k - 2^-45 into k - 1; neutral where an axis has weights 0 and 1 only, and
#                             (by the few values involved) at three small pairs
#   u8_half_channel           none: every image has pixels whose channels 0 and 2 differ
_ONE_TAP = ["1x1-3x4", "1x9-5x4", "7x1-3x6", "3x5-3x5"]
RESIZE_NEUTRAL = {
    "weight_f64": _ONE_TAP + ["17x23-32x48", "64x96-32x48", "20x30-40x60", "67x101-37x53"],
    "scale_f32": ["1x1-3x4", "1x9-5x4", "3x5-3x5", "64x96-32x48", "20x30-40x60"],
    "lower_clamp_keeps_weight": _ONE_TAP + ["48x64-32x48", "45x70-32x48", "64x96-32x48", "67x101-37x53"],
    "columns_first": ["1x1-3x4", "1x9-5x4", "7x1-3x6", "2x2-9x13", "3x5-3x5", "300x9-8x259", "5x4-9x3"],
    "u8_half_channel": [],
}


@pytest.mark.parametrize("defect", fr.RESIZE_DEFECTS)
def test_simulated_resize_defects_are_rejected(defect):
    neutral, by_bound = [], 0
    for pair, pid in zip(t.RESIZE_PAIRS, t.RESIZE_IDS):
        (sh, sw), (dh, dw) = pair
        changed = 0
        for kind in t.IMAGE_KINDS:
            for flip in (0, 1):
                u, exact, bound, indep = t.resize_case(pair, kind, flip)
                wrong = fr.resize_variant(u, dh, dw, flip, defect)
                before = t.byte_pattern(u.shape[0] * dh * (2 * dw + 1) * 3)
                want8 = fr.place_rows(before, fr.resize_u8_half(exact, flip), 2 * dw + 1, 1)
                wrong8 = fr.place_rows(before, fr.resize_u8_half(wrong, flip, defect), 2 * dw + 1, 1)
                differs = fr.count_differing(wrong.astype(F32), exact.astype(F32)) + fr.count_differing(wrong8, want8)
                off, far, ratio = fr.check_resize(wrong.astype(F32), exact, bound, indep)
                rejected = not fr.resize_passes(off, far, ratio, wrong.size) or fr.count_differing(wrong8, want8) > 0
                assert rejected == (differs > 0), (pid, kind, flip, differs, len(off), far, ratio)
                changed += differs > 0
                by_bound += ratio > 1.
        if not changed:
            neutral.append(pid)
    print("%s: value-neutral at %s; the bound against torch alone rejects %d of %d (pair, image, flip)" % (
        defect, neutral, by_bound, 6 * len(t.RESIZE_PAIRS)))
    assert len(t.RESIZE_PAIRS) - len(neutral) >= len(t.RESIZE_PAIRS) / 2, neutral
    assert neutral == RESIZE_NEUTRAL[defect], neutral


# ---------------------------------------------------------------------------------------------------------------------
# coverage

def test_table_covers_every_kernel_of_frames_hip_in_the_library():
    """every __global__ of frames.hip, every instantiation of it in the built library: 5 when this was written; a new one
    without a case fails here"""
    from coupe.dvsg_amd import _lib
    names = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(FRAMES_SRC).read())
    assert sorted(names) == ["frames_to_u8_kernel", "frames_u8_to_f32_kernel", "resize_u8_kernel", "window_gather_kernel"]
    pat = re.compile(rb"_ZN4dvsg12_GLOBAL__N_1\d+(" + "|".join(names).encode() + rb")(?:I([a-z])E)?E")
    found = {(n.decode(),) + ((a.decode(),) if a else ()) for n, a in pat.findall(open(_lib.LIB_PATH, "rb").read())}
    assert len(found) >= 5 and found == set(t.COVERED), (sorted(found - set(t.COVERED)), sorted(set(t.COVERED) - found))
    tests = {n for n in dir(t) if n.startswith("test_")}
    for cases in t.COVERED.values():
        assert cases and all(c.split(" ")[0] in tests for c in cases), cases
