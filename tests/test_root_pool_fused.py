"""The float32 root max pool in the band kernel's epilogue -- root_band_pool_kernel + root_pool_seams_kernel -- against the
tree's own two-kernel path (root_band_kernel, then maxpool_kernel<float>), bit for bit.

The two-kernel path is held to float64 element by element (test_root_head_f64.py: conv1_kernel and the pool;
test_root_band.py: the band kernel equals conv1_kernel), and a max only selects one of its inputs, so equality as int32
carries those bounds over: no tolerance here.  `root_pool` 2 fuses wherever the band kernel runs and `conv1_variant` 6 runs
it at any size in bands of at most 3 pairs, which puts tile seams, band seams and their corners into frames of a few rows;
`root_pool` 1 is the reference.  The launch record names the kernels: conv1 family 7 both ways, max pool kernel 4 (the
seam kernel behind the pooling band kernel) or 0 (maxpool_kernel<float>).

The CPU test restates the partition -- what a workgroup owns, what it leaves as a partial, which conv values it stores
for its neighbours, and the seam kernel's flat index -- in NumPy and checks it against a plain 3x3 / stride 2 max pool.
"""
import numpy as np
import pytest

import test_root_head_f64 as rh

ROOT_FIELDS = rh.ROOT_FIELDS
FIRST = (2, 32, 516)     # conv 16 x 258, pooled 8 x 129: column tiles of 128, 128 and 2 px; 8 pairs in bands of 3, 3, 2
CORNER = (2, 32, 260)    # conv 16 x 130, pooled 8 x 65: the last tile one pooled column wide
SINGLE = (2, 28, 260)    # conv 14 x 130: 7 pairs in bands of 3, 3, 1
BIG = (16, 720, 1280)


# ---------------------------------------------------------------------------------------------------------------------
# the partition, in NumPy

def band_start(i, ppb, nbig):
    """first pair of band i (root_band_kernel: p0)"""
    return i * ppb - (i - nbig if i > nbig else 0)


def plain_pool(conv):
    """3x3 / stride 2 max pool of [Ho, Wo, C], Ho and Wo even: TF 'SAME' pads nothing on the top and the left"""
    Ho, Wo, C = conv.shape
    out = np.full((Ho // 2, Wo // 2, C), -np.inf, conv.dtype)
    for r in range(Ho // 2):
        for c in range(Wo // 2):
            out[r, c] = conv[2 * r:min(2 * r + 3, Ho), 2 * c:min(2 * c + 3, Wo)].max(axis=(0, 1))
    return out


def band_kernel_model(conv, bands, ppb, nbig, tile):
    """what the pooling band kernel leaves behind: (pooled tensor with partial maxima at the seams, conv tensor holding only
    the stored taps -- NaN where nothing was written)"""
    Ho, Wo, C = conv.shape
    pairs, Wp = Ho // 2, Wo // 2
    pooled = np.full((pairs, Wp, C), np.nan, conv.dtype)
    taps = np.full_like(conv, np.nan)
    for band in range(bands):
        p0 = band_start(band, ppb, nbig)
        p1 = min(p0 + (ppb if band < nbig else ppb - 1), pairs)
        for wo0 in range(0, Wo, tile):
            nv = min(tile, Wo - wo0)
            carry = None
            for p in range(p0, p1):
                up, lo = conv[2 * p, wo0:wo0 + nv], conv[2 * p + 1, wo0:wo0 + nv]
                hu = np.stack([up[2 * lc:min(2 * lc + 3, nv)].max(axis=0) for lc in range(nv // 2)])
                hl = np.stack([lo[2 * lc:min(2 * lc + 3, nv)].max(axis=0) for lc in range(nv // 2)])
                if p > p0:
                    pooled[p - 1, wo0 // 2:wo0 // 2 + nv // 2] = np.maximum(carry, hu)
                carry = np.maximum(hu, hl)
                if p + 1 == p1:
                    pooled[p, wo0 // 2:wo0 // 2 + nv // 2] = carry
                if wo0 > 0:
                    taps[2 * p:2 * p + 2, wo0] = conv[2 * p:2 * p + 2, wo0]
                if p == p0 and p0 > 0:
                    taps[2 * p, wo0:wo0 + nv] = up
    return pooled, taps


def seam_kernel_model(pooled, taps, bands, ppb, nbig, tile, groups=16):
    """root_pool_seams_kernel, thread by thread: flat index e -> (pooled row, column, channel group) -> the taps it adds.
    Returns how many elements it finished."""
    Ho, Wo, C = taps.shape
    Hp, Wp, half = Ho // 2, Wo // 2, tile // 2
    ncs = -(-Wo // tile) - 1
    n_col = Hp * ncs * groups
    total = n_col + (bands - 1) * Wp * groups
    done = 0
    for e in range(total):
        c4 = e % groups
        if e < n_col:
            t = e // groups
            c = half * (t % ncs) + half - 1
            r = (t // ncs) % Hp
            p, full = r + 1, nbig * ppb
            i = p // ppb if p < full else nbig + (p - full) // max(ppb - 1, 1)
            col_seam, row_seam = True, p < Hp and i < bands and band_start(i, ppb, nbig) == p
        else:
            t = (e - n_col) // groups
            c = t % Wp
            r = band_start((t // Wp) % (bands - 1) + 1, ppb, nbig) - 1
            if r < 0 or r + 1 >= Hp:
                continue
            if c % half == half - 1 and 2 * c + 2 < Wo:
                continue
            col_seam, row_seam = False, True
        ch = slice(4 * c4, 4 * c4 + 4)
        m = pooled[r, c, ch]
        if col_seam:
            for i in range(3):
                if 2 * r + i < Ho:
                    m = np.maximum(m, taps[2 * r + i, 2 * c + 2, ch])
        if row_seam:
            for j in range(3):
                if 2 * c + j < Wo and not (col_seam and j == 2):
                    m = np.maximum(m, taps[2 * r + 2, 2 * c + j, ch])
        assert not np.isnan(m).any(), "read a conv value nobody stored, at pooled (%d, %d)" % (r, c)
        pooled[r, c, ch] = m
        done += 1
    return done


def variant6_split(Ho):
    bands = ((Ho + 1) // 2 + 2) // 3
    return bands, 3, bands


def test_partition_and_seam_merge_equal_a_plain_max_pool():
    """tiles of 128 at the widths the GPU cases run, then random band and tile splits at small sizes: partial maxima + the
    seam kernel's taps == the plain pool, every seam element is finished exactly once, and no tap is read that the band
    kernel did not store"""
    rng = np.random.default_rng(26)
    splits = [(16, 258, 128) + variant6_split(16), (16, 130, 128) + variant6_split(16), (14, 130, 128) + variant6_split(14),
              (8, 384, 128, 1, 4, 1), (24, 256, 128, 3, 4, 3), (2, 2, 128, 1, 1, 1)]
    for _ in range(40):
        ppb = int(rng.integers(2, 6))
        nbig, nsmall = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        pairs = nbig * ppb + nsmall * (ppb - 1)
        tile = 2 * int(rng.integers(1, 6))
        Wo = 2 * int(rng.integers(1, 14))
        splits.append((2 * pairs, Wo, tile, nbig + nsmall, ppb, nbig))
    for Ho, Wo, tile, bands, ppb, nbig in splits:
        assert band_start(bands, ppb, nbig) >= Ho // 2 > band_start(bands - 1, ppb, nbig), "not a split of the pairs"
        conv = np.maximum(rng.standard_normal((Ho, Wo, 64)).astype(np.float32), 0)      # post-ReLU: zeros among the values
        pooled, taps = band_kernel_model(conv, bands, ppb, nbig, tile)
        assert not np.isnan(pooled).any(), "a pooled element nobody wrote"
        ref = plain_pool(conv)
        partial = (pooled != ref).any(axis=2)
        seam = np.zeros_like(partial)
        seam[:, [c for c in range(Wo // 2) if c % (tile // 2) == tile // 2 - 1 and 2 * c + 2 < Wo]] = True
        seam[[band_start(i, ppb, nbig) - 1 for i in range(1, bands)], :] = True
        assert not (partial & ~seam).any(), "an element off the seams is not whole"
        done = seam_kernel_model(pooled, taps, bands, ppb, nbig, tile)
        assert done == 16 * int(seam.sum()), (done, int(seam.sum()))
        assert np.array_equal(pooled, ref), (Ho, Wo, tile, bands, ppb, nbig)
        # the stored conv values are a small part of the tensor: column 0 of the tiles but the first, the bands' first rows
        stored = ~np.isnan(taps[..., 0])
        expect = np.zeros_like(stored)
        expect[:, tile::tile] = True
        expect[[2 * band_start(i, ppb, nbig) for i in range(1, bands)], :] = True
        assert np.array_equal(stored, expect)


def test_the_gpu_shapes_hold_what_their_comments_say():
    for (B, H, W), pairs, last_band, tiles in ((FIRST, 8, 2, (128, 128, 2)), (CORNER, 8, 2, (128, 2)), (SINGLE, 7, 1, (128, 2))):
        Ho, Wo = H // 2, W // 2
        bands, ppb, nbig = variant6_split(Ho)
        assert Ho % 2 == 0 and Wo % 2 == 0 and Ho // 2 == pairs and bands == 3
        assert pairs - band_start(bands - 1, ppb, nbig) == last_band
        assert tuple(min(128, Wo - w) for w in range(0, Wo, 128)) == tiles


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _set(name, v):
    from coupe.dvsg_amd import _lib
    _lib.call("dvsg_debug_set_option", name, v)


def _run(net, variant, root_pool, kind, src, tab, n, shape, stage, out_floats):
    _set(b"conv1_variant", variant)
    _set(b"root_pool", root_pool)
    try:
        return rh.run_net(net, "f32", kind, 0, src, tab, None, n, shape[0], shape[1], shape[2], stage, out_floats)
    finally:
        _set(b"conv1_variant", 0)
        _set(b"root_pool", 0)


def _pooled_dims(shape):
    B, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return B, (Ho + 1) // 2, (Wo + 1) // 2


def _both(net, kind, src, tab, n, shape, variant=6, fused_pool=2):
    """stage-1 taps of the fused and the two-kernel path, with their launch records"""
    B, Hp, Wp = _pooled_dims(shape)
    yf, recf = _run(net, variant, fused_pool, kind, src, tab, n, shape, 1, B * Hp * Wp * 64)
    yr, recr = _run(net, variant, 1, kind, src, tab, n, shape, 1, B * Hp * Wp * 64)
    assert recr[0] == 7 and recr[6] == 0, dict(zip(ROOT_FIELDS, recr))
    assert recf[:6] == recr[:6], (recf, recr)
    return yf.view(B, Hp, Wp, 64), recf, yr.view(B, Hp, Wp, 64)


def _assert_equal_bits(yf, yr):
    import torch
    differ = yf.view(torch.int32) != yr.view(torch.int32)
    if bool(differ.any()):
        d = differ.nonzero()
        print("differ at (b, r, c, n): first %s last %s" % (d[0].tolist(), d[-1].tolist()))
    assert int(differ.sum()) == 0, "%d of %d elements differ" % (int(differ.sum()), yf.numel())
    assert float(yr.abs().max()) > 0.0


SRC_CASES = [(kind, off) for kind in (0, 1, 2) for off in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,off", SRC_CASES, ids=["%s%s" % (("win", "ringf", "ringu")[k], "-off" if o else "") for k, o in SRC_CASES])
def test_fused_pool_equals_the_two_kernels_for_every_source(synthetic_weights, kind, off):
    """column seams, a ragged last tile and three bands, through all six SRC instantiations"""
    import torch
    net, _ = rh._net(synthetic_weights, False)
    case = ("f32", 6, kind, 0, off, FIRST, "wide" if kind == 1 else "u8", None)
    src, tab, mask, n, x, mk = rh.place_inputs(case, torch.device("cuda:0"))
    yf, recf, yr = _both(net, kind, src, tab, n, FIRST)
    assert recf[3] == rh.src_of(kind, rh.aligned_of(FIRST, off), 0) and recf[4:6] == (3, 3)
    assert recf[6] == 4, "the fused kernels did not run: %s" % dict(zip(ROOT_FIELDS, recf))
    assert src.unchanged() and (tab is None or tab.unchanged()), "an input changed"
    _assert_equal_bits(yf, yr)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [CORNER, SINGLE], ids=["corner", "single-pair-band"])
def test_a_one_column_last_tile_a_corner_and_a_band_of_one_pair(synthetic_weights, shape):
    import torch
    net, _ = rh._net(synthetic_weights, False)
    src, tab, mask, n, x, mk = rh.place_inputs(("f32", 6, 0, 0, False, shape, "u8", None), torch.device("cuda:0"))
    yf, recf, yr = _both(net, 0, src, None, n, shape)
    assert recf[6] == 4 and recf[4:6] == (3, 3), dict(zip(ROOT_FIELDS, recf))
    # pooled (2, 63) and (5, 63): the last row of a band and the last column of a tile at once
    for r in (2, 5):
        assert torch.equal(yf[:, r, 63].view(torch.int32), yr[:, r, 63].view(torch.int32)), "corner (%d, 63)" % r
    assert torch.equal(yf[:, :, 64].view(torch.int32), yr[:, :, 64].view(torch.int32)), "the one-column tile"
    _assert_equal_bits(yf, yr)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 30, 516), (2, 32, 514)], ids=["H1-odd", "W1-odd"])
def test_an_odd_conv_size_keeps_the_two_kernels(synthetic_weights, shape):
    import torch
    net, _ = rh._net(synthetic_weights, False)
    src, tab, mask, n, x, mk = rh.place_inputs(("f32", 6, 0, 0, False, shape, "u8", None), torch.device("cuda:0"))
    yf, recf, yr = _both(net, 0, src, None, n, shape)
    assert recf[0] == 7 and recf[6] == 0, "root_pool 2 fused at an odd size: %s" % dict(zip(ROOT_FIELDS, recf))
    _assert_equal_bits(yf, yr)


@pytest.mark.gpu
def test_a_tap_of_conv1_keeps_the_two_kernels(synthetic_weights):
    """stage 0 reads conv1's whole output: root_pool 2 must not fuse, and the tap is the band kernel's"""
    import torch
    net, _ = rh._net(synthetic_weights, False)
    src, tab, mask, n, x, mk = rh.place_inputs(("f32", 6, 0, 0, False, FIRST, "u8", None), torch.device("cuda:0"))
    y2, rec2 = _run(net, 6, 2, 0, src, None, n, FIRST, 0, 2 * 16 * 258 * 64)
    y1, rec1 = _run(net, 6, 1, 0, src, None, n, FIRST, 0, 2 * 16 * 258 * 64)
    assert rec2 == rec1 and rec2[0] == 7 and rec2[6] == -1, dict(zip(ROOT_FIELDS, rec2))
    assert torch.equal(y2.view(torch.int32), y1.view(torch.int32)) and float(y1.abs().max()) > 0.0


@pytest.mark.gpu
def test_a_nan_pixel_and_an_inf_pixel(synthetic_weights):
    """NaN positions and every other value equal the two-kernel path's (the payload of a NaN is not compared)"""
    import torch
    net, _ = rh._net(synthetic_weights, False)
    B, H, W = FIRST
    dev = torch.device("cuda:0")
    n = B + 6
    pool = rh.make_pool("wide", n, H, W, 26)
    x = rh.gather_window(pool, rh.make_table(B, n, oob=False))
    x[0, 11, 255, :] = np.nan          # feeds conv columns on both sides of the first column seam
    x[1, 22, 300, 4] = np.inf
    src = rh.Placed(x, dev)
    yf, recf, yr = _both(net, 0, src, None, n, FIRST)
    assert recf[6] == 4, dict(zip(ROOT_FIELDS, recf))
    nan_f, nan_r = torch.isnan(yf), torch.isnan(yr)
    assert torch.equal(nan_f, nan_r), "NaN positions differ"
    assert torch.equal(yf[~nan_f].view(torch.int32), yr[~nan_r].view(torch.int32))
    assert bool(torch.isinf(yr).any()) or bool(nan_r.any()) or float(yr.abs().max()) > 0.0
    assert src.unchanged()


@pytest.mark.gpu
def test_sixteen_720p_windows_with_default_options(synthetic_weights):
    """B = 16 at 1280 x 720, nothing forced: the fused kernels run (16 bands of 12 and 11 pairs, 5 column tiles); the stage-1
    tap and F_t equal root_pool 1's bit for bit.  (A uint8 frame ring: 22 frames instead of a 1.2 GB window tensor.)"""
    import torch
    B, H, W = BIG
    net, _ = rh._net(synthetic_weights, False)
    dev = torch.device("cuda:0")
    n = B + 6
    src = rh.Placed(rh.make_pool("u8", n, H, W, 726), dev)
    tab = rh.Placed(rh.make_table(B, n, oob=True), dev)
    yf, recf, yr = _both(net, 2, src, tab, n, BIG, variant=0, fused_pool=0)
    assert recf == (7, 8, 0, 5, 16, 12, 4, -1, -1), dict(zip(ROOT_FIELDS, recf))
    _assert_equal_bits(yf, yr)
    del yf, yr
    Ff, recf = _run(net, 0, 0, 2, src, tab, n, BIG, -1, B * 50)
    Fr, recr = _run(net, 0, 1, 2, src, tab, n, BIG, -1, B * 50)
    assert recf[:7] == (7, 8, 0, 5, 16, 12, 4) and recr[:7] == (7, 8, 0, 5, 16, 12, 0), (recf, recr)
    assert bool(torch.isfinite(Fr).all()) and torch.equal(Ff.view(torch.int32), Fr.view(torch.int32)), "F_t differs"
    assert src.unchanged() and tab.unchanged()
