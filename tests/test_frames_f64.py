"""The frame-format kernels of frames.hip pinned to exact and float64 references (tests/frames_ref.py), every element.

Every pixel that enters or leaves the product passes one of them: dvsg_frames_u8_to_f32, _f32_to_u8, _f64_to_u8,
_resize_u8_f32, _ingest_u8, _f32_to_u8_slots and dvsg_window_gather_f32.  All but the resize are byte and index work and
are held BIT FOR BIT; so is the resize against frames_ref.resize_exact, which performs the kernel's roundings one by one,
and its float32 output is held besides to torch's float64 bilinear interpolation (half-pixel centres, computed on the CPU:
an implementation that shares no text with the kernel or the oracle) within frames_ref.resize_bound + 2^-24 |v|, a bound
derived in that function's docstring and fitted to nothing.

Every output lies between guard bytes (Guarded of test_conv_gemm_f64.py) and is filled with a byte pattern first: every
byte outside the addressed rows and columns must come back unchanged.

1.  frames_u8_to_f32_kernel: all 256 byte values in every channel, npix in U8F32_NPIX, the source 0-3 bytes off the 4-byte
    grid (dst must be 16-byte aligned, so the source is the only alignment there is), both flips; the same through
    dvsg_frames_ingest_u8 at source size == model size, into the slots of SLOTS_INGEST.
2.  frames_to_u8_kernel<float | double>: W in TO_U8_W (3 W % 4 = 0, 1, 2, 3), H in (1, 3), n in (1, 2), the layouts of
    to_u8_layouts (the first byte of a row at all four residues mod 4), both flips, uniform values with the edge set
    (edge_values: k / 255 and the float just below it for every k, +-0, subnormals, 1 and its neighbours, 256 / 255,
    +-inf, NaN) in the first and last value of every row and either side of a group boundary; the whole edge set in one
    row; dvsg_frames_f32_to_u8_slots on SLOTS_EGRESS.
3.  window_gather_kernel: S x B x (h, w) of the tables below, -1 and n_pool in the last slot of window b and the first
    of window b + 1.
4.  resize_u8_kernel through dvsg_frames_resize_u8_f32 and dvsg_frames_ingest_u8: RESIZE_PAIRS x IMAGE_KINDS, both
    flips, without the uint8 half and with it at x0 in (0, 1, dst_W, dst_W + 1), n in (1, 3).  Four pairs and one kind
    of image were added to the issue's tables: the pairs that enlarge (a weight left on the lower clamp shows only where
    a coordinate is negative, which of the twelve asked pairs four have), and the "flat" image of constant 3 x 3
    blocks (on constant taps the two passes give p (a0 + a1) rounded one way or another, and the truncation of the uint8
    half turns that last float64 bit into a byte: the one place where the order of the passes shows).
    The 1-ulp route (an element off float32(resize_exact) by one float32 ulp, for at most 1e-6 of the elements) was
    taken by NO element of any case on the MI355X: every float32 value equals float32(resize_exact) bit for bit.
5.  One OnlineStabilizer step with every frame kind at once (two resized uint8 sizes, same-size uint8, float32, float64).
6.  The second pass of the grid-stride loops: one case per kernel just above 65 536 x 256 groups, reference computed on
    the device.
7.  COVERED: every __global__ of frames.hip found in the built library, with the cases that launch it
    (tests/test_frames_ref_cpu.py compares it with the mangled names).

Measured on one MI355X: 242 cases in 4.0 s; everything bit-exact; worst ratio of a resize to torch's
float64 0.84 (67 x 101 -> 37 x 53, stripes).  No kernel defect was found."""
import functools

import numpy as np
import pytest

import frames_ref as fr
import test_conv_gemm_f64 as f64

pytestmark = pytest.mark.gpu
Guarded = f64.Guarded
F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------
# tables (plain data: the CPU tests read them too)

N_POOL = 5
SLOTS_EGRESS = {"permuted": [3, 0, 4], "outside": [-1, 2, N_POOL], "outside, duplicated": [N_POOL + 3, 1, 1],
                "duplicated": [2, 2, 0], "one": [4], "one outside": [N_POOL + 3]}
SLOTS_INGEST = {"permuted": [3, 0, 4], "outside": [-1, 2, N_POOL], "far outside": [N_POOL + 3, 1, 0], "one": [4],
                "one outside": [-1], "one at n_pool": [N_POOL]}

U8F32_NPIX = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025)
U8F32_OFFSETS = (0, 1, 2, 3)

TO_U8_W, TO_U8_H, TO_U8_N = (1, 2, 3, 4, 5, 13, 64, 65), (1, 3), (1, 2)
TO_U8_SHAPES = [(W, H, n) for W in TO_U8_W for H in TO_U8_H for n in TO_U8_N]

GATHER_S, GATHER_B = (1, 2, 3, 5, 7), (1, 2, 3)
GATHER_HW = ((1, 1), (1, 3), (3, 5), (5, 5), (9, 11))
GATHER_CASES = [(S, B, h, w) for S in GATHER_S for B in GATHER_B for h, w in GATHER_HW]

RESIZE_PAIRS = [((1, 1), (3, 4)), ((1, 9), (5, 4)), ((7, 1), (3, 6)), ((2, 2), (9, 13)), ((3, 5), (3, 5)),
                ((17, 23), (32, 48)), ((48, 64), (32, 48)), ((45, 70), (32, 48)), ((64, 96), (32, 48)), ((20, 30), (40, 60)),
                ((67, 101), (37, 53)), ((300, 9), (8, 259)),
                ((3, 2), (4, 7)), ((5, 4), (9, 3)), ((9, 16), (32, 48)), ((13, 19), (32, 48))]      # added: they enlarge
SAME_SIZE = ((3, 5), (3, 5))
IMAGE_KINDS = ("noise", "stripes", "flat")
RESIZE_N = 3
RESIZE_IDS = ["%dx%d-%dx%d" % (s + d) for s, d in RESIZE_PAIRS]

# item 6: the smallest asked sizes with more than 65 536 x 256 groups
STRIDE_CAP = 65536 * 256
BIG_U8F32 = (3, 4320, 5200)
BIG_GATHER = (2, 7, 1080, 1920)
BIG_RESIZE = (3, 300, 300, 2400, 2400)

COVERED = {
    ("frames_u8_to_f32_kernel",): ["test_u8_to_f32_every_byte_every_alignment", "test_ingest_same_size_into_slots",
                                   "test_every_frame_kind_in_one_step", "test_second_pass_u8_to_f32"],
    ("frames_to_u8_kernel", "f"): ["test_to_u8_float_double_and_slots (float, slots)", "test_to_u8_whole_edge_set",
                                   "test_every_frame_kind_in_one_step", "test_second_pass_f32_to_u8"],
    ("frames_to_u8_kernel", "d"): ["test_to_u8_float_double_and_slots (double)", "test_to_u8_whole_edge_set",
                                   "test_every_frame_kind_in_one_step"],
    ("window_gather_kernel",): ["test_window_gather", "test_second_pass_window_gather"],
    ("resize_u8_kernel",): ["test_resize_exact_and_against_torch", "test_every_frame_kind_in_one_step",
                            "test_second_pass_resize"],
}


def to_u8_layouts(W):
    """(dst_W, dst_x0): tight, three offsets into a wider row, and the right half of a side-by-side row of odd width"""
    return [(W, 0), (W + 2, 1), (W + 2, 2), (W + 4, 3), (2 * W + 1, W + 1)]


def row_residues(rows, dst_W, x0):
    """first byte of every row relative to the 4-byte grid (the destination itself is 256-byte aligned)"""
    return {(r * 3 * dst_W + 3 * x0) % 4 for r in range(rows)}


def byte_pattern(nbytes):
    """never 0 and never 255 (what a zero-fill or a saturation writes), period 251"""
    return (np.arange(nbytes, dtype=np.int64) % 251 + 2).astype(np.uint8)


def edge_values(dtype):
    """k / 255 and the value of `dtype` just below it for every k in 1..255, and the specials"""
    dt = np.dtype(dtype).type
    at = (np.arange(1, 256) / 255.).astype(dt)
    below = np.nextafter(at, dt(-np.inf))
    tiny = np.finfo(dt)
    special = np.array([0., -0., tiny.smallest_subnormal, -tiny.smallest_subnormal, tiny.tiny / 2, tiny.tiny, 1.,
                        np.nextafter(dt(1), dt(np.inf)), np.nextafter(dt(1), dt(-np.inf)), dt(256 / 255.), np.inf, -np.inf,
                        np.nan, 1.5, -0.25, tiny.max, -tiny.max, 0.5], dtype=dt)
    return np.concatenate([special, at, below])


def to_u8_values(dtype, n, H, W, seed):
    """uniform [n,H,W,3] with edge values in the first and last value of every row and either side of each of the first
    group boundaries (values 3 | 4 and 7 | 8), a different run of the edge set in every row"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0., 1., (n * H, 3 * W)).astype(dtype)
    edges = edge_values(dtype)
    at = [p for p in sorted({0, 3 * W - 1, 3, 4, 7, 8}) if p < 3 * W]
    k = seed
    for r in range(n * H):
        for p in at:
            x[r, p] = edges[k % edges.size]
            k += 265                                  # half the edge set and one: k / 255 and the value below it alternate
    return x.reshape(n, H, W, 3)


def flipped(x, flip):
    return x[..., ::-1] if flip else x


def make_image(kind, n, sh, sw, seed):
    """noise: white; stripes: columns alternate 0 and 255 (the largest adjacent difference: the bound is widest and the
    weights matter most); flat: constant 3 x 3 blocks (see the module docstring)"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    if kind == "stripes":
        u = np.zeros((n, sh, sw, 3), dtype=np.uint8)
        u[:, :, 1::2] = 255
        return u
    blocks = rng.integers(0, 256, (n, -(-sh // 3), -(-sw // 3), 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 3, axis=1), 3, axis=2)[:, :sh, :sw])


def torch_bilinear(u8, dh, dw, flip):
    """torch's float64 bilinear interpolation with half-pixel centres, on the CPU: the independent arbiter"""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(flipped(np.asarray(u8), flip))).to(torch.float64) / 255.
    out = torch.nn.functional.interpolate(p.permute(0, 3, 1, 2), size=(dh, dw), mode="bilinear", align_corners=False)
    return out.permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def resize_case(pair, kind, flip):
    """(image [RESIZE_N,sh,sw,3], resize_exact, resize_bound, torch) of a case, computed once and never written to"""
    (sh, sw), (dh, dw) = pair
    u = make_image(kind, RESIZE_N, sh, sw, sh * 1009 + sw * 31 + dh)
    out = (u, fr.resize_exact(u, dh, dw, flip), fr.resize_bound(u, dh, dw, flip), torch_bilinear(u, dh, dw, flip))
    for a in out:
        a.setflags(write=False)
    return out


def gather_indices(S, B, seed):
    """random, then -1 / n_pool in the last slot of window b and the first of window b + 1 (alternating which is which), so
    that the group of four floats across the seam mixes a frame of zeros with a real one.  With S == 1 those two slots are
    the whole window: there every other window reads outside the pool instead."""
    idx = np.random.default_rng(seed).integers(0, N_POOL, (B, S)).astype(np.int32)
    if S == 1:
        idx[(B + 1) % 2::2, 0] = [-1, N_POOL][:len(idx[(B + 1) % 2::2])] if B > 1 else idx[0, 0]
        return idx
    idx[B - 1, S - 1] = N_POOL + 3
    for b in range(B - 1):
        idx[b, S - 1], idx[b + 1, 0] = (-1, N_POOL) if b % 2 == 0 else (N_POOL, -1)
    if B == 1 and S > 2:
        idx[0, 0] = -1
    return idx


# ---------------------------------------------------------------------------------------------------------------------
# plumbing

def _call(name, *args):
    from coupe.dvsg_amd import _lib
    _lib.call(name, *args)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(before):
    """a guarded device buffer holding the bytes of `before`"""
    import torch
    b = np.ascontiguousarray(before)
    g = Guarded(b.nbytes, torch.device("cuda"))
    g.body.copy_(torch.from_numpy(b.reshape(-1).view(np.uint8)))
    return g


def _back(g, dtype, shape):
    import torch
    torch.cuda.synchronize()
    assert g.intact(), "guard bytes overwritten"
    return g.body.cpu().numpy().view(dtype).reshape(shape)


def _slots(s):
    return _dev(np.asarray(s, dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. uint8 -> float32

def u8_source(npix, frames=1):
    """pixel p, channel c = 7 p + 85 c (+ 3 per frame) mod 256: 256 consecutive pixels hold every byte value in every channel"""
    p, c, f = np.arange(npix)[None, :, None], np.arange(3)[None, None, :], np.arange(frames)[:, None, None]
    return ((7 * p + 85 * c + 3 * f) % 256).astype(np.uint8)


def _at_offset(u, offset):
    """the bytes of u on the device, `offset` bytes past a 256-byte aligned address"""
    import torch
    buf = torch.zeros(offset + u.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[offset:offset + u.size].copy_(torch.from_numpy(u.reshape(-1)))
    return buf, buf.data_ptr() + offset


@pytest.mark.parametrize("offset", U8F32_OFFSETS)
@pytest.mark.parametrize("npix", U8F32_NPIX)
def test_u8_to_f32_every_byte_every_alignment(npix, offset):
    u = u8_source(npix)[0]
    if npix >= 256:
        assert all(set(u[:, c].tolist()) == set(range(256)) for c in range(3))
    keep, src = _at_offset(u, offset)
    for flip in (0, 1):
        g = _guarded(np.full(npix * 3, -7.0, dtype=F32))
        _call("dvsg_frames_u8_to_f32", src, npix, flip, g.ptr(), 0)
        got = _back(g, F32, (npix, 3))
        assert fr.count_differing(got, fr.u8_to_f32(u, flip)) == 0, (npix, offset, flip)


@pytest.mark.parametrize("offset", U8F32_OFFSETS)
@pytest.mark.parametrize("npix", U8F32_NPIX)
def test_ingest_same_size_into_slots(npix, offset):
    """source size == model size routes dvsg_frames_ingest_u8 to the conversion kernel, frame i into slots[i]; with
    3 npix % 4 != 0 the frames of one call start at different residues"""
    from coupe.dvsg_amd import DvsgError
    pool0 = np.full((N_POOL, 1, npix, 3), -7.0, dtype=F32)
    for v, (name, slots) in enumerate(SLOTS_INGEST.items()):
        flip, n = v % 2, len(slots)
        u = u8_source(npix, n)
        keep, src = _at_offset(u, offset)
        g, d_slots = _guarded(pool0), _slots(slots)
        _call("dvsg_frames_ingest_u8", src, n, 1, npix, flip, g.ptr(), N_POOL, d_slots.data_ptr(), 1, npix, 0, 0, 0, 0)
        got = _back(g, F32, pool0.shape)
        want = fr.ingest_slots(pool0, fr.u8_to_f32(u, flip).reshape(n, 1, npix, 3), slots)
        assert fr.count_differing(got, want) == 0, (npix, offset, name)
    with pytest.raises(DvsgError, match="no size change"):
        _call("dvsg_frames_ingest_u8", src, 1, 1, npix, 0, g.ptr(), N_POOL, d_slots.data_ptr(), 1, npix, g.ptr(), npix, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. float32 / float64 -> uint8

def _to_u8_run(entry, x, flip, dst_W, x0, slots=None):
    """launch one egress of frames x [n,H,W,3] (or of pool x through `slots`) into a patterned, guarded destination ->
    (bytes that came back, bytes the reference expects)"""
    H, W = x.shape[1], x.shape[2]
    n = x.shape[0] if slots is None else len(slots)
    before = byte_pattern(n * H * dst_W * 3)
    g = _guarded(before)
    d_x = _dev(x)
    if slots is None:
        _call(entry, d_x.data_ptr(), n, H, W, flip, g.ptr(), dst_W, x0, 0)
        frames = x
    else:
        d_slots = _slots(slots)
        _call(entry, d_x.data_ptr(), x.shape[0], d_slots.data_ptr(), n, H, W, flip, g.ptr(), dst_W, x0, 0)
        frames = fr.egress_slots(x, slots)
    want = fr.place_rows(before, fr.to_u8(flipped(frames, flip)), dst_W, x0)
    return _back(g, np.uint8, want.shape), want


@pytest.mark.parametrize("W,H,n", TO_U8_SHAPES)
def test_to_u8_float_double_and_slots(W, H, n):
    for flip in (0, 1):
        for dst_W, x0 in to_u8_layouts(W):
            seed = W * 100 + H * 10 + n + x0
            for entry, dtype in (("dvsg_frames_f32_to_u8", np.float32), ("dvsg_frames_f64_to_u8", np.float64)):
                got, want = _to_u8_run(entry, to_u8_values(dtype, n, H, W, seed), flip, dst_W, x0)
                assert fr.count_differing(got, want) == 0, (entry, flip, dst_W, x0)
    pool = to_u8_values(np.float32, N_POOL, H, W, W + H)
    for v, (name, slots) in enumerate(SLOTS_EGRESS.items()):
        dst_W, x0 = to_u8_layouts(W)[v % 5]
        got, want = _to_u8_run("dvsg_frames_f32_to_u8_slots", pool, v % 2, dst_W, x0, slots)
        assert fr.count_differing(got, want) == 0, (name, dst_W, x0)


@pytest.mark.parametrize("flip", [0, 1])
def test_to_u8_whole_edge_set(flip):
    """every edge value of both formats in one row each (padded to whole pixels with 0.5), at two residues"""
    from coupe.dvsg_amd import DvsgError
    for entry, dtype in (("dvsg_frames_f32_to_u8", np.float32), ("dvsg_frames_f64_to_u8", np.float64)):
        e = edge_values(dtype)
        x = np.concatenate([e, np.full(-e.size % 3, 0.5, dtype=dtype)]).reshape(1, 1, -1, 3)
        for dst_W, x0 in ((x.shape[2], 0), (x.shape[2] + 3, 3)):
            got, want = _to_u8_run(entry, x, flip, dst_W, x0)
            assert fr.count_differing(got, want) == 0, (entry, dst_W, x0)
    with pytest.raises(DvsgError, match="do not fit"):
        _to_u8_run("dvsg_frames_f64_to_u8", x, flip, x.shape[2], 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. window gather

@pytest.mark.parametrize("S,B,h,w", GATHER_CASES)
def test_window_gather(S, B, h, w):
    pool = np.random.default_rng(S * 100 + B * 10 + h).uniform(0.1, 1., (N_POOL, h, w, 3)).astype(F32)
    idx = gather_indices(S, B, S + B + w)
    g = _guarded(np.full(B * h * w * 3 * S, -7.0, dtype=F32))
    d_pool, d_idx = _dev(pool), _dev(idx)
    _call("dvsg_window_gather_f32", d_pool.data_ptr(), N_POOL, h, w, d_idx.data_ptr(), B, S, g.ptr(), 0)
    got = _back(g, F32, (B, h, w, 3 * S))
    assert fr.count_differing(got, fr.window_gather(pool, idx)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. resize

def u8_layouts(dw):
    """(u8_W, u8_x0) of the uint8 half, None: without it.  The row is 2 dw + 1 pixels wide (odd: the rows start at
    different residues), which x0 = dw + 1 fills to the last byte"""
    return [None] + [(2 * dw + 1, x0) for x0 in (0, 1, dw, dw + 1)]


@pytest.mark.parametrize("kind", IMAGE_KINDS)
@pytest.mark.parametrize("pair", RESIZE_PAIRS, ids=RESIZE_IDS)
def test_resize_exact_and_against_torch(pair, kind):
    from coupe.dvsg_amd import DvsgError
    (sh, sw), (dh, dw) = pair
    worst, launches, routed = 0.0, 0, 0
    ingest_variants = list(SLOTS_INGEST.items())
    for flip in (0, 1):
        u, exact, bound, indep = resize_case(pair, kind, flip)
        d_u = _dev(u.copy())
        for n in (1, RESIZE_N):
            for layout in u8_layouts(dw):
                u8_W, x0 = layout or (0, 0)
                before8 = byte_pattern(n * dh * u8_W * 3) if layout else None
                want8 = fr.place_rows(before8, fr.resize_u8_half(exact[:n], flip), u8_W, x0) if layout else None
                # the resize entry
                g, g8 = _guarded(np.full((n, dh, dw, 3), -7.0, dtype=F32)), _guarded(before8) if layout else None
                _call("dvsg_frames_resize_u8_f32", d_u.data_ptr(), n, sh, sw, flip, g.ptr(), dh, dw,
                      g8.ptr() if layout else 0, u8_W, x0, 0)
                got = _back(g, F32, (n, dh, dw, 3))
                off, far, ratio = fr.check_resize(got, exact[:n], bound[:n], indep[:n])
                assert fr.resize_passes(off, far, ratio, got.size), (
                    "flip %d n %d layout %s: %d elements off float32(resize_exact) (first %s), %d beyond 1 ulp, worst "
                    "ratio to torch's float64 %.3f" % (flip, n, layout, len(off), off[:1].tolist(), far, ratio))
                worst, launches, routed = max(worst, ratio), launches + 1, routed + len(off)
                if layout:
                    assert fr.count_differing(_back(g8, np.uint8, want8.shape), want8) == 0, (flip, n, layout)
                # the ingest entry: same frames into pool slots
                name, slots = ingest_variants[launches % len(ingest_variants)]
                slots = slots[:n] if len(slots) >= n else [2, -1, 0][:n]
                pool0 = np.full((N_POOL, dh, dw, 3), -7.0, dtype=F32)
                g, g8, d_slots = _guarded(pool0), _guarded(before8) if layout else None, _slots(slots)
                args = (d_u.data_ptr(), n, sh, sw, flip, g.ptr(), N_POOL, d_slots.data_ptr(), dh, dw,
                        g8.ptr() if layout else 0, u8_W, x0, 0)
                if pair == SAME_SIZE and layout:
                    with pytest.raises(DvsgError, match="no size change"):
                        _call("dvsg_frames_ingest_u8", *args)
                    continue
                _call("dvsg_frames_ingest_u8", *args)
                want = fr.ingest_slots(pool0, exact[:n].astype(F32), slots)
                assert fr.count_differing(_back(g, F32, pool0.shape), want) == 0, (flip, n, layout, name, slots)
                if layout:
                    want8 = fr.ingest_u8_half(before8, fr.resize_u8_half(exact[:n], flip), slots, N_POOL, u8_W, x0)
                    assert fr.count_differing(_back(g8, np.uint8, want8.shape), want8) == 0, (flip, n, layout, name, slots)
    assert routed == 0          # fewer than a million elements per launch: the 1-ulp route is closed here
    print("resize %s %s: %d launches of each entry, worst ratio to torch float64 %.3f" % (RESIZE_IDS[RESIZE_PAIRS.index(pair)],
                                                                                          kind, launches, worst))


# ---------------------------------------------------------------------------------------------------------------------
# 5. every frame kind in one step

def test_every_frame_kind_in_one_step(synthetic_weights):
    """Five streams, one frame kind each, three steps; the dictionary is not in the order the step sorts the kinds into.
    Per stream: the input slot and the left half of `side` are, bit for bit, what the direct kernel call for its kind
    writes; the right half is its `out`.  Nothing is asserted about the stabilised values (tests/test_gpu_online.py)."""
    import torch
    import inputs
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    H, W, flip = 32, 48, 1
    model = StabNet(H, W).load_weights(synthetic_weights)
    model.get_evaluation_model(7)
    on = OnlineStabilizer(model, max_streams=5, side_by_side=True, as_uint8=True, channel_order="bgr")
    sids = {k: on.open() for k in ("u8 45x70", "u8 40x60", "u8 same", "f32", "f64")}
    order = ["f64", "u8 same", "u8 45x70", "f32", "u8 40x60"]
    steps = 3
    clips = {"u8 45x70": (inputs.smooth_frames(7101, steps, 45, 70) * 255).astype(np.uint8),
             "u8 40x60": (inputs.smooth_frames(7102, steps, 40, 60) * 255).astype(np.uint8),
             "u8 same": (inputs.smooth_frames(7103, steps, H, W) * 255).astype(np.uint8),
             "f32": inputs.smooth_frames(7104, steps, H, W).astype(np.float32),
             "f64": inputs.smooth_frames(7105, steps, H, W).astype(np.float64) * (1 - 2.0 ** -30)}
    assert clips["f64"].dtype == np.float64 and not np.array_equal(clips["f64"], clips["f64"].astype(F32))

    def direct(kind, frame):
        """(input slot [H,W,3] float32, left half [H,W,3] uint8) by the direct call for the kind"""
        d = _dev(frame[None])
        slot = torch.full((1, H, W, 3), -7.0, device="cuda")
        side = torch.zeros((1, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
        if kind in ("u8 45x70", "u8 40x60"):
            _call("dvsg_frames_resize_u8_f32", d.data_ptr(), 1, frame.shape[0], frame.shape[1], flip, slot.data_ptr(), H, W,
                  side.data_ptr(), 2 * W, 0, 0)
        elif kind == "u8 same":
            _call("dvsg_frames_u8_to_f32", d.data_ptr(), H * W, flip, slot.data_ptr(), 0)
            _call("dvsg_frames_f32_to_u8", slot.data_ptr(), 1, H, W, flip, side.data_ptr(), 2 * W, 0, 0)
        elif kind == "f32":
            slot.copy_(d)
            _call("dvsg_frames_f32_to_u8", slot.data_ptr(), 1, H, W, flip, side.data_ptr(), 2 * W, 0, 0)
        else:
            slot.copy_(d)                                                  # one rounding to float32 (the feed cast)
            _call("dvsg_frames_f64_to_u8", d.data_ptr(), 1, H, W, flip, side.data_ptr(), 2 * W, 0, 0)
        torch.cuda.synchronize()
        return slot[0].cpu().numpy(), side[0, :, :W].cpu().numpy()

    for k in range(steps):
        res = on.step({sids[name]: clips[name][k] for name in order})
        assert list(res) == [sids[name] for name in order]
        pool = on.pool.cpu().numpy()
        for name in order:
            out, side = res[sids[name]]
            ring = on._streams[sids[name]][0]
            want_slot, want_left = direct(name, clips[name][k])
            got_slot = pool[ring * on.frames_per_stream + on.span + 1]
            assert fr.count_differing(got_slot, want_slot) == 0, (k, name)
            assert out.dtype == np.uint8 and out.shape == (H, W, 3) and side.shape == (H, 2 * W, 3)
            assert fr.count_differing(side[:, :W], want_left) == 0, (k, name)
            assert np.array_equal(side[:, W:], out), (k, name)
            assert want_left.any()
    lefts = [direct(name, clips[name][0])[1] for name in order]
    assert all(not np.array_equal(lefts[0], x) for x in lefts[1:])         # five different frames: a swap would show


# ---------------------------------------------------------------------------------------------------------------------
# 6. the second pass of the grid-stride loops (reference computed and compared on the device)

def _t255():
    """255 as a device tensor: torch divides by a Python scalar on the device by multiplying with its reciprocal, which
    is not the correctly rounded quotient the kernels and eval.py:80 compute; tensor / tensor is"""
    import torch
    return torch.tensor(255., dtype=torch.float64, device="cuda")


def test_second_pass_u8_to_f32():
    import torch
    n, H, W = BIG_U8F32
    npix = n * H * W
    assert (npix + 3) // 4 > STRIDE_CAP
    src = torch.randint(0, 256, (npix, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    dst = torch.full((npix, 3), -7.0, device="cuda")
    _call("dvsg_frames_u8_to_f32", src.data_ptr(), npix, 1, dst.data_ptr(), 0)
    want = (src.flip(1).to(torch.float64) / _t255()).to(torch.float32)
    assert torch.equal(dst, want)


def test_second_pass_f32_to_u8():
    import torch
    n, H, W = BIG_U8F32
    assert n * H * ((3 * W + 3) // 4) > STRIDE_CAP
    x = torch.rand((n, H, W, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(2)) * 1.2 - 0.1
    dst = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    _call("dvsg_frames_f32_to_u8", x.data_ptr(), n, H, W, 1, dst.data_ptr(), W, 0, 0)
    want = (x.flip(3).to(torch.float64) * 255.).clamp_(0., 255.).trunc_().to(torch.uint8)
    assert torch.equal(dst, want)


def test_second_pass_window_gather():
    import torch
    B, S, h, w = BIG_GATHER
    assert (B * h * w * 3 * S + 3) // 4 > STRIDE_CAP
    pool = torch.rand((N_POOL, h, w, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3)) + 0.1
    idx = gather_indices(S, B, 5)
    got, d_idx = torch.full((B, h, w, 3 * S), -7.0, device="cuda"), _dev(idx)
    _call("dvsg_window_gather_f32", pool.data_ptr(), N_POOL, h, w, d_idx.data_ptr(), B, S, got.data_ptr(), 0)
    padded = torch.cat([pool, torch.zeros_like(pool[:1])])
    safe = torch.from_numpy(np.where(fr.slot_ok(idx, N_POOL), idx, N_POOL).astype(np.int64)).cuda()
    want = padded[safe].permute(0, 2, 3, 1, 4).reshape(B, h, w, 3 * S)
    assert torch.equal(got, want)


def test_second_pass_resize():
    """resize_exact in torch float64 on the device: eager products and sums, one kernel each, so nothing is fused"""
    import torch
    n, sh, sw, dh, dw = BIG_RESIZE
    assert n * dh * dw > STRIDE_CAP
    flip = 1
    src = torch.randint(0, 256, (n, sh, sw, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    got = torch.full((n, dh, dw, 3), -7.0, device="cuda")
    got8 = torch.full((n, dh, dw, 3), 7, dtype=torch.uint8, device="cuda")
    _call("dvsg_frames_resize_u8_f32", src.data_ptr(), n, sh, sw, flip, got.data_ptr(), dh, dw, got8.data_ptr(), dw, 0, 0)
    p = src.flip(3).to(torch.float64) / _t255()
    x0, x1, wx = fr.resize_taps(dw, sw)
    y0, y1, wy = fr.resize_taps(dh, sh)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a1, a0 = dev(wx.astype(np.float64)).view(1, 1, dw, 1), dev((F32(1) - wx).astype(np.float64)).view(1, 1, dw, 1)
    b1, b0 = dev(wy.astype(np.float64)).view(1, dh, 1, 1), dev((F32(1) - wy).astype(np.float64)).view(1, dh, 1, 1)
    rows = p[:, :, dev(x0)] * a0 + p[:, :, dev(x1)] * a1
    want = rows[:, dev(y0)] * b0 + rows[:, dev(y1)] * b1
    del rows
    assert torch.equal(got, want.to(torch.float32))
    assert torch.equal(got8, (want * 255.).clamp_(0., 255.).trunc_().to(torch.uint8).flip(3))
