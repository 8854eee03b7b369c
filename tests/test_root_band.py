"""root_band_kernel -- float32 conv1 for big launches: row pairs in bands, one workgroup per CU -- against the one-row
conv1_kernel<4, float, SRC>, bit for bit.

The band kernel feeds the same operands, in the same order, through the same instruction into the same two chains per
output element as the one-row kernel (conv1_f32.hip), so its output must EQUAL that kernel's: no tolerance, the tensors
are compared as int32.  The one-row kernel is held to float64 element by element in test_root_head_f64.py, and equality
carries that bound over.  conv1_variant 6 forces the band kernel at any size (bands of at most 3 pairs), 7 the one-row
kernel; 0 is the library's own choice, restated here as `root_bands`.
"""
import re

import numpy as np
import pytest

import test_root_head_f64 as rh
import test_units_f64 as units

ROOT_FIELDS = rh.ROOT_FIELDS


def root_bands(B, Ho, wtiles):
    """launch_conv1's rule restated: (bands per column tile and image, pairs in the longest band), (0, 0): not selected"""
    pairs, cols = (Ho + 1) // 2, B * wtiles
    best, best_fill = 0, 0.0
    for rounds in range(3, 7):
        bands = min(256 * rounds // cols, pairs // 4)
        if bands < 1 or cols * bands < 3 * 256:
            continue
        fill = (cols * bands) / (256.0 * rounds)
        if fill > best_fill:
            best, best_fill = bands, fill
    return (best, -(-pairs // best)) if best else (0, 0)


def launch_of(variant, kind, masked, aligned, shape):
    """the float32 launch record restated for conv1_variant 0, 6, 7: (family, NW, TO, SRC, bands, pairs per band)"""
    B, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    SRC = rh.src_of(kind, aligned, masked)
    bands, ppb = root_bands(B, Ho, (Wo + 127) // 128)
    if variant == 6:
        ppb = 3
        bands = ((Ho + 1) // 2 + 2) // 3
    if not masked and variant != 7 and (variant == 6 or bands > 0):
        return (7, 8, 0, SRC, bands, ppb)
    return (0, 4, 0, SRC, -1, -1)


# (shape, base moved off the 16-byte grid): what each exercises is in the comment
BAND_SHAPES = [((2, 12, 256), False),    # Wo 128 exactly
               ((2, 9, 253), False),     # Wo 127, unaligned
               ((2, 13, 257), False),    # Wo 129; Ho 7: odd, the last pair single
               ((2, 6, 514), False),     # Wo 257: three column tiles, the last of one pixel
               ((2, 52, 20), False),     # Ho 26: 13 pairs -> bands of 3, the last band with one pair
               ((1, 54, 255), False),    # Ho 27: 14 pairs, the last pair single, a ragged last band
               ((2, 1, 4), False),       # Ho 1: every other input row is padding
               ((2, 1, 1), False),       # one-pixel rows
               ((2, 2, 3), False),
               ((2, 12, 256), True)]     # the unaligned instantiation at W % 4 == 0


def _band_cases():
    out = []
    for i, (shape, off) in enumerate(BAND_SHAPES):
        for j in range(2):                          # two sources per shape: all six SRC values run
            kind = (2 * i + j) % 3
            inputs = "wide" if (kind != 2 and (i + j) % 3 == 0) else "u8"
            out.append((shape, off, kind, inputs))
    return out


BAND_CASES = _band_cases()
BIG = (16, 720, 1280)


def _id(c):
    (B, H, W), off, kind, inputs = c
    return "%s%s-%dx%dx%d-%s" % (("win", "ringf", "ringu")[kind], "-off" if off else "", B, H, W, inputs)


# ---------------------------------------------------------------------------------------------------------------------
# CPU

def test_the_rule_never_selects_the_band_kernel_at_a_pinned_shape():
    """test_root_head_f64.py and test_units_f64.py pin the float32 record (0, 4, 0, SRC, -1, -1) at conv1_variant 0 for
    every shape they run: the rule must leave all of them to the one-row kernel, and take B = 16 at 1280 x 720 in 16
    bands (80 column tiles x 16 = 1280 workgroups, five rounds of 256 CUs)."""
    pinned = list(rh.A_SHAPES) + list(rh.U_SHAPES) + [rh.OFF_GRID] + [s for _, s in rh.POOL_CASES] + list(units.SHAPES)
    assert len(pinned) > 30
    for shape in pinned:
        for kind in (0, 1, 2):
            exp = launch_of(0, kind, 0, shape[2] % 4 == 0, shape)
            assert exp[0] == 0 and exp[4:] == (-1, -1), (shape, exp)
            assert exp == rh.launch_of("f32", 0, kind, 0, shape[2] % 4 == 0, shape), shape
    assert root_bands(16, 360, 5) == (16, 12)
    assert launch_of(0, 2, 0, True, BIG) == (7, 8, 0, 5, 16, 12)
    assert launch_of(0, 2, 1, True, BIG)[0] == 0 and launch_of(7, 2, 0, True, BIG)[0] == 0
    # the rule's own terms: at least three rounds of workgroups, at least four pairs per band, never past six rounds
    for B, Ho, wt in ((16, 360, 5), (64, 1080, 15), (8, 360, 5), (32, 180, 3), (256, 16, 1), (3, 2000, 1)):
        bands, ppb = root_bands(B, Ho, wt)
        if bands:
            assert 768 <= B * wt * bands <= 6 * 256 and (Ho + 1) // 2 // bands >= 4 and ppb * bands >= (Ho + 1) // 2
    assert root_bands(1, 360, 5) == (0, 0)


def test_band_cases_run_every_source():
    srcs = {rh.src_of(kind, rh.aligned_of(shape, off), 0) for shape, off, kind, _ in BAND_CASES}
    assert srcs == set(range(6)), sorted(srcs)
    multi = [s for s, _ in BAND_SHAPES if launch_of(6, 0, 0, False, s)[4] > 1]
    assert (2, 52, 20) in multi and (1, 54, 255) in multi


def test_the_library_holds_six_band_kernels_under_their_own_name():
    """six instantiations (window, float32 ring, uint8 ring; aligned or not), and the conv1 kernel set that
    test_root_head_f64.py tabulates is what it was: 62 instantiations, each with a case there."""
    from coupe.dvsg_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    mine = set(int(v) for v in re.findall(rb"_ZN4dvsg12_GLOBAL__N_116root_band_kernelILi(\d+)EEEv", data))
    assert mine == set(range(6)), sorted(mine)
    conv, pool = rh.library_instantiations()
    assert len(conv) == 62 and len(pool) == 4, (len(conv), len(pool))
    assert conv == {rh.instantiation(c[7]) for c in rh.CASES + rh.MARCH_CASES}
    assert sum(1 for c in conv if c[0] == "conv1_kernel") == 14


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _run(net, variant, kind, masked, src, tab, mask, n, shape, stage, out_floats):
    rh._set_variant(variant)
    try:
        return rh.run_net(net, "f32", kind, masked, src, tab, mask, n, shape[0], shape[1], shape[2], stage, out_floats)
    finally:
        rh._set_variant(0)


def _equal_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAND_CASES, ids=[_id(c) for c in BAND_CASES])
def test_band_kernel_equals_the_one_row_kernel_bit_for_bit(synthetic_weights, case):
    """tap 0 at conv1_variant 6 and 7: equal as int32, the records name the two kernels, nothing outside the output and
    the workspace is written, the inputs keep their bytes."""
    import torch
    shape, off, kind, inputs = case
    B, H, W = shape
    net, _ = rh._net(synthetic_weights, False)
    dev = torch.device("cuda:0")
    src, tab, mask, n, x, mk = rh.place_inputs(("f32", 6, kind, 0, off, shape, inputs, None), dev)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    aligned = rh.aligned_of(shape, off)
    y6, rec6 = _run(net, 6, kind, 0, src, tab, None, n, shape, 0, B * Ho * Wo * 64)
    y7, rec7 = _run(net, 7, kind, 0, src, tab, None, n, shape, 0, B * Ho * Wo * 64)
    assert rec6 == launch_of(6, kind, 0, aligned, shape) + (-1, -1, -1), dict(zip(ROOT_FIELDS, rec6))
    assert rec7 == launch_of(7, kind, 0, aligned, shape) + (-1, -1, -1), dict(zip(ROOT_FIELDS, rec7))
    assert rec6[0] == 7 and rec7[:3] == (0, 4, 0)
    assert src.unchanged() and (tab is None or tab.unchanged()), "an input changed"
    assert float(y7.abs().max()) > 0.0
    differ = int((y6.view(torch.int32) != y7.view(torch.int32)).sum())
    if differ:
        d = (y6.view(B, Ho, Wo, 64) != y7.view(B, Ho, Wo, 64)).nonzero()
        print("differ at (b, ho, wo, n): first %s last %s" % (d[0].tolist(), d[-1].tolist()))
    assert differ == 0, "%d of %d elements differ" % (differ, y6.numel())


@pytest.mark.gpu
def test_a_masked_source_takes_the_one_row_kernel(synthetic_weights):
    import torch
    shape = (2, 13, 257)
    B, H, W = shape
    net, _ = rh._net(synthetic_weights, False)
    src, tab, mask, n, x, mk = rh.place_inputs(("f32", 6, 0, 1, False, shape, "u8", None), torch.device("cuda:0"))
    y, rec = _run(net, 6, 0, 1, src, None, mask, n, shape, 0, B * 7 * 129 * 64)
    assert rec == (0, 4, 0, rh.src_of(0, False, 1), -1, -1, -1, -1, -1), dict(zip(ROOT_FIELDS, rec))
    assert rec[:6] == launch_of(6, 0, 1, False, shape)


@pytest.mark.gpu
def test_the_library_s_own_choice_at_sixteen_720p_windows(synthetic_weights):
    """B = 16 at 1280 x 720, conv1_variant 0: family 7 in 16 bands; tap 0 and F_t of the whole network equal the one-row
    kernel's bit for bit.  (A uint8 frame ring: 22 frames instead of a 1.2 GB window tensor.)"""
    import torch
    B, H, W = BIG
    net, _ = rh._net(synthetic_weights, False)
    dev = torch.device("cuda:0")
    n = B + 6
    src = rh.Placed(rh.make_pool("u8", n, H, W, 720), dev)
    tab = rh.Placed(rh.make_table(B, n, oob=True), dev)
    floats = B * (H // 2) * (W // 2) * 64
    y0, rec0 = _run(net, 0, 2, 0, src, tab, None, n, BIG, 0, floats)
    assert rec0 == (7, 8, 0, 5, 16, 12, -1, -1, -1), dict(zip(ROOT_FIELDS, rec0))
    assert rec0[:6] == launch_of(0, 2, 0, True, BIG)
    y7, rec7 = _run(net, 7, 2, 0, src, tab, None, n, BIG, 0, floats)
    assert rec7[:6] == (0, 4, 0, 5, -1, -1), dict(zip(ROOT_FIELDS, rec7))
    assert float(y7.abs().max()) > 0.0 and _equal_bits(y0, y7), "tap 0 differs"
    del y0, y7
    F0, rec0 = _run(net, 0, 2, 0, src, tab, None, n, BIG, -1, B * 50)
    F7, rec7 = _run(net, 7, 2, 0, src, tab, None, n, BIG, -1, B * 50)
    assert rec0[0] == 7 and rec0[4] == 16 and rec7[0] == 0
    assert bool(torch.isfinite(F7).all()) and _equal_bits(F0, F7), "F_t differs"
    assert src.unchanged() and tab.unchanged()


@pytest.mark.gpu
def test_sixty_bands_down_one_long_frame(synthetic_weights):
    """a (1, 720, 4) window at conv1_variant 6: 180 pairs in 60 bands of one column tile"""
    import torch
    shape = (1, 720, 4)
    net, _ = rh._net(synthetic_weights, False)
    src, tab, mask, n, x, mk = rh.place_inputs(("f32", 6, 0, 0, False, shape, "u8", None), torch.device("cuda:0"))
    y6, rec6 = _run(net, 6, 0, 0, src, None, None, n, shape, 0, 360 * 2 * 64)
    y7, rec7 = _run(net, 7, 0, 0, src, None, None, n, shape, 0, 360 * 2 * 64)
    assert rec6 == (7, 8, 0, 1, 60, 3, -1, -1, -1), dict(zip(ROOT_FIELDS, rec6))
    assert rec7[:6] == (0, 4, 0, 1, -1, -1)
    assert src.unchanged() and float(y7.abs().max()) > 0.0 and _equal_bits(y6, y7)
