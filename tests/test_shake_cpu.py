"""No-GPU checks of the shake measurement: the conditions under which the NumPy restatement (tests/shake_ref.py) is a
meaningful reference for tests/test_gpu_shake.py -- shifted textures come back, flat, striped and out-of-range content drops
out, the tie-break, the floor and the median behave as written -- and the host side of coupe.dvsg_amd.shake: summary, compare,
luma_of, the chunking, the two entry points' refusals (every one before any device work) and the command line's.

Observed on the reference's own inputs, not a bound: the five sub-pixel shifts of test_subpel_shifts_are_close come back within
0.125 reduced pixels of the truth."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import shake_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def big_1080():
    """A 17-wide-box texture with room for shifts of up to 48 source pixels around a 1080 x 1920 window."""
    if "big" not in _CACHE:
        _CACHE["big"] = shake_ref.texture(11, 1080 + 96, 1920 + 96, box=17)
    return _CACHE["big"]


def measure_1080(oy, ox):
    big = big_1080()
    planes = np.stack([shake_ref.shifted(big, 0, 0, 1080, 1920, 48), shake_ref.shifted(big, oy, ox, 1080, 1920, 48)])
    assert shake_ref.default_geometry(1080, 1920) == (4, 34, 60)
    return shake_ref.measure(planes, 4, 12, 34, 60, 256, 8)


@pytest.mark.parametrize("oy,ox", [(8, -12), (2, 2), (40, 0)])
def test_integer_shifts_within_the_radius_come_back_exactly(oy, ox):
    vectors, blocks = measure_1080(oy, ox)
    assert blocks.shape == (1, 264, 3) and (blocks[0, :, 2] == 1).all()
    gx, gy, n_valid, ok = (int(v) for v in vectors[0])
    assert (n_valid, ok) == (264, 1)
    assert (gy * 4, gx * 4) == (16 * oy, 16 * ox)       # sixteenths of a reduced pixel x factor = sixteenths of a source pixel


def small_pair(cur, prev, radius=4, margin=4, texture=256, min_blocks=1):
    return shake_ref.measure(np.stack([prev, cur]), 1, radius, margin, margin, texture, min_blocks)


def test_a_flat_plane_gives_no_valid_block():
    flat = np.full((56, 72), 117, dtype=np.uint8)
    vectors, blocks = small_pair(flat, flat)
    assert blocks.shape == (1, 12, 3) and not blocks.any()
    assert vectors.tolist() == [[0, 0, 0, 0]]


def test_vertical_stripes_give_no_valid_block():
    s = shake_ref.stripes(56, 80)
    vectors, blocks = small_pair(s[:, :72], s[:, 1:73])
    assert not blocks.any() and vectors.tolist() == [[0, 0, 0, 0]]


def test_a_checkerboard_shifted_by_its_period_resolves_to_zero():
    """Every shift by a multiple of the period has SAD 0: the shortest vector wins."""
    c = shake_ref.checkerboard(60, 80, cell=2)
    vectors, blocks = small_pair(c[4:, 4:76], c[:56, :72], radius=6, margin=6)
    assert blocks.shape[1] == 6 and (blocks == [0, 0, 1]).all()
    assert vectors.tolist() == [[0, 0, 6, 1]]


def test_a_shift_equal_to_the_radius_gives_no_valid_block():
    big = shake_ref.texture(3, 72, 96)
    prev = shake_ref.shifted(big, 0, 0, 56, 72, 8)
    for oy, ox in ((4, 0), (0, -4), (-4, 4)):
        vectors, blocks = small_pair(shake_ref.shifted(big, oy, ox, 56, 72, 8), prev)
        assert not blocks.any() and vectors.tolist() == [[0, 0, 0, 0]], (oy, ox)
    vectors, blocks = small_pair(shake_ref.shifted(big, 3, -3, 56, 72, 8), prev)      # one inside: all come back
    assert (blocks[0, :, 2] == 1).all() and vectors.tolist() == [[-48, 48, 12, 1]]


def test_subpel_shifts_are_close():
    """An observation on the reference's own inputs (the module docstring records it); asserted only as far as the rule
    guarantees: the parabola moves the integer minimum by at most half a pixel."""
    big = shake_ref.texture(12, 300 + 40, 500 + 40)
    prev = shake_ref.shifted(big, 0, 0, 300, 500, 20)
    worst = 0.0
    for oy, ox in ((0.25, 0.5), (1.5, -2.75), (3.3, 0.1), (-0.6, 2.2), (0.0, 0.9)):
        planes = np.stack([prev, shake_ref.shifted_subpel(big, oy, ox, 300, 500, 20)])
        vectors, blocks = shake_ref.measure(planes, 1, 12, 38, 63, 256, 8)
        assert vectors[0, 3] == 1 and vectors[0, 2] == blocks.shape[1] == 322
        worst = max(worst, abs(vectors[0, 0] / 16 - ox), abs(vectors[0, 1] / 16 - oy))
    print("largest deviation of the five sub-pixel shifts: %.4f reduced pixels" % worst)
    assert worst <= 0.5


def test_the_floor_takes_negative_numerators_down():
    # c = 10: numerator 16 (S- - S+) + 10 over 20
    assert shake_ref.subpel(5, 0, 5, 2) == (10, 32)             # 10 / 20 -> 0
    assert shake_ref.subpel(4, 0, 6, 2) == (10, 32 - 2)         # -22 / 20 = -1.1 -> -2
    assert shake_ref.subpel(6, 0, 4, 2) == (10, 32 + 2)         # 42 / 20 = 2.1 -> 2
    assert shake_ref.subpel(0, 0, 10, -1) == (10, -16 - 8)      # -150 / 20 = -7.5 -> -8
    assert shake_ref.subpel(10, 0, 0, -1) == (10, -16 + 8)      # 170 / 20 = 8.5 -> 8
    assert shake_ref.subpel(3, 3, 3, 0) == (0, None)
    # a table whose minimum has a lopsided neighbourhood: block_row applies the same floor
    S = np.full((5, 5), 1000, dtype=np.int64)
    S[2, 2], S[2, 1], S[2, 3], S[1, 2], S[3, 2] = 0, 4, 6, 300, 100
    assert shake_ref.block_row(S, 2, 1) == (-2, 4, 1)           # x: -22 / 20 -> -2;  y: (3200 + 400) / 800 = 4.5 -> 4
    assert shake_ref.block_row(S, 2, 11) == (0, 0, 0)           # cx = 10 below the texture threshold


def test_the_median_is_the_lower_one_and_per_axis():
    rows = np.array([[5, -3, 1], [99, 99, 0], [-7, 8, 1], [2, 8, 1], [40, -9, 1]], dtype=np.int32)
    # valid vx: -7 2 5 40 -> rank 1 = 2;  valid vy: -9 -3 8 8 -> rank 1 = -3
    assert shake_ref.global_vector(rows, 4).tolist() == [2, -3, 4, 1]
    assert shake_ref.global_vector(rows, 5).tolist() == [0, 0, 4, 0]
    assert shake_ref.global_vector(rows[:3], 1).tolist() == [-7, -3, 2, 1]
    assert shake_ref.global_vector(rows[1:2], 1).tolist() == [0, 0, 0, 0]


def test_reduce_rounds_half_up_and_drops_the_ragged_edge():
    p = np.array([[0, 1, 9], [1, 0, 9], [9, 9, 9]], dtype=np.uint8)
    assert shake_ref.reduce(p, 2).tolist() == [[1]]             # (2 + 2) / 4
    assert shake_ref.reduce(p, 3).tolist() == [[5]]             # (47 + 4) / 9
    assert shake_ref.reduce(p, 1) is not p and (shake_ref.reduce(p, 1) == p).all()


# ---- coupe.dvsg_amd.shake on the host -----------------------------------------------------------------------------

VECTORS = np.array([[16, 0, 9, 1], [-16, 32, 9, 1], [0, 0, 3, 0], [48, 0, 9, 1], [48, -16, 9, 1]], dtype=np.int64)


def test_summary_on_hand_made_vectors():
    from coupe.dvsg_amd import shake
    s = shake.summary(shake.Track(VECTORS, 4, (1080, 1920), None))
    # ok rows: 256, 1280, 2304, 2560 -> 6400 / 4;  differences of rows 0-1 (1024 + 1024) and 3-4 (256): 2304 / 2
    speed, jitter = 4 / 16 * math.sqrt(6400 / 4), 4 / 16 * math.sqrt(2304 / 2)
    assert s == dict(frames=6, pairs=5, lost=1, speed_rms=speed, jitter_rms=jitter, speed_pct=100 * speed / 1920,
                     jitter_pct=100 * jitter / 1920)
    assert speed == 10.0
    assert s == shake_ref.summary(VECTORS, 4, 1920)
    lost = shake.summary(shake.Track(np.array([[0, 0, 1, 0]], dtype=np.int64), 1, (64, 96), None))
    assert lost == dict(frames=2, pairs=1, lost=1, speed_rms=None, jitter_rms=None, speed_pct=None, jitter_pct=None)
    assert lost == shake_ref.summary([[0, 0, 1, 0]], 1, 96)


def test_compare_adds_the_jitter_ratio():
    from coupe.dvsg_amd import shake
    a = shake.Track(VECTORS, 4, (1080, 1920), None)
    b = shake.Track(np.array([[16, 0, 9, 1], [16, 16, 9, 1], [16, 32, 9, 1]], dtype=np.int64), 4, (1080, 1920), None)
    c = shake.compare(a, b)
    assert c["a"] == shake.summary(a) and c["b"] == shake.summary(b)
    assert c["b"]["jitter_rms"] == 4.0 and c["jitter_ratio"] == 4.0 / c["a"]["jitter_rms"]
    assert shake.compare(b, shake.Track(VECTORS[:1], 4, (1080, 1920), None))["jitter_ratio"] is None


def test_geometry_defaults():
    from coupe.dvsg_amd import shake
    assert shake.geometry(1080, 1920) == (4, 34, 60)
    assert shake.geometry(2160, 3840) == (8, 34, 60)
    assert shake.geometry(270, 480) == (1, 34, 60)
    assert shake.geometry(64, 96) == (1, 12, 12)
    assert shake.geometry(203, 125, factor=3, radius=5) == (3, 9, 6)
    for args in ((1080, 1920), (64, 96), (720, 1281), (2160, 3840)):
        assert shake.geometry(*args) == shake_ref.default_geometry(*args)


def test_chunks_overlap_by_one_frame_and_cover_every_pair_once():
    from coupe.dvsg_amd import shake
    assert shake.chunk_ranges(9, 64) == [(0, 9)]
    assert shake.chunk_ranges(9, 9) == [(0, 9)]
    assert shake.chunk_ranges(9, 3) == [(0, 3), (2, 5), (4, 7), (6, 9)]
    assert shake.chunk_ranges(9, 2) == [(i, i + 2) for i in range(8)]
    assert shake.chunk_ranges(10, 4) == [(0, 4), (3, 7), (6, 10)]
    assert shake.chunk_ranges(8, 4) == [(0, 4), (3, 7), (6, 8)]
    assert shake.chunk_ranges(2, 64) == [(0, 2)]
    for n in range(2, 20):
        for chunk in range(2, 8):
            pairs = [t for a, b in shake.chunk_ranges(n, chunk) for t in range(a + 1, b)]
            assert pairs == list(range(1, n)), (n, chunk)
    with pytest.raises(ValueError, match="chunk"):
        shake.chunk_ranges(9, 1)


def test_luma_of_each_layout():
    import torch
    from coupe.dvsg_amd import shake
    rng = np.random.RandomState(5)
    n, H, W = 2, 8, 12
    nv12 = rng.randint(0, 256, size=(n, 3 * H // 2, W)).astype(np.uint8)
    nv16 = rng.randint(0, 256, size=(n, 2 * H, W)).astype(np.uint8)
    for frames, fmt in ((nv12, "nv12"), (nv16, "nv16")):
        t = torch.from_numpy(frames)
        y = shake.luma_of(t, fmt)
        assert y.shape == (n, H, W) and y.data_ptr() == t.data_ptr() and y.stride() == (frames.shape[1] * W, W, 1)   # no copy
        assert np.array_equal(y.numpy(), frames[:, :H])
        assert np.array_equal(shake.luma_of(frames, fmt).numpy(), frames[:, :H])
    for rows, fmt in ((3 * H // 2, "p010"), (2 * H, "p210")):
        words = (rng.randint(0, 1024, size=(n, rows, W)) << 6).astype(np.uint16)
        as_bytes = words.view(np.uint8)
        assert as_bytes.shape == (n, rows, 2 * W)
        want = (words[:, :H] >> 8).astype(np.uint8)
        assert np.array_equal(shake.luma_of(as_bytes, fmt).numpy(), want)
        assert np.array_equal(shake.luma_of(words.view(np.int16), fmt).numpy(), want)      # 16-bit words of any torch dtype
    rgb = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    rgb[0, 0, 0], rgb[0, 0, 1] = 255, 0
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    got = shake.luma_of(rgb, "rgb")
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), (77 * r + 150 * g + 29 * b + 128) >> 8)
    assert got[0, 0, 0] == 255 and got[0, 0, 1] == 0
    with pytest.raises(ValueError, match="frame_format"):
        shake.luma_of(nv12, "yuyv")
    with pytest.raises(ValueError, match="3 H / 2"):
        shake.luma_of(nv12[:, :11], "nv12")


# ---- the C entry points, before any device work -------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def test_the_two_names_are_bound_and_exported(lib):
    from coupe.dvsg_amd import _lib
    for name in ("dvsg_shake_workspace_bytes", "dvsg_shake_measure_u8"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["dvsg_shake_workspace_bytes"]) == 8 and len(_lib.SIGNATURES["dvsg_shake_measure_u8"]) == 16
    header = open(os.path.join(ROOT, "include", "dvsg_amd.h")).read()
    start, end = header.index("int dvsg_shake_workspace_bytes("), header.index(" * NV12 frames")
    block = " ".join(header[header.index(" * SHAKE"):start].replace("\n *", " ").split())
    assert "synchronous" in block and "legacy default stream" in block and "stream" not in header[start:end]


GOOD = dict(n=2, H=1080, W=1920, factor=4, radius=12, margin_y=34, margin_x=60)
# (changed arguments, the words the message must hold): the geometry, shared by both entry points
GEOMETRY_REFUSALS = [
    (dict(n=1), ["n=1", "[2, 4096]"]), (dict(n=4097), ["n=4097"]),
    (dict(H=0), ["0x1920"]), (dict(W=16385), ["1080x16385"]),
    (dict(factor=0), ["factor=0"]), (dict(factor=17), ["factor=17"]),
    (dict(radius=0), ["radius=0"]), (dict(radius=17, margin_y=40), ["radius=17"]),
    (dict(margin_y=11), ["margin_y=11", "radius=12"]), (dict(margin_x=11), ["margin_x=11", "radius=12"]),
    (dict(margin_y=128), ["no 16 x 16 block", "270x480"]),
    (dict(factor=1), ["7056 blocks", "factor=1"]),
]


def workspace_bytes(lib, **kw):
    a = dict(GOOD, **kw)
    out = ctypes.c_size_t(12345)
    rc = lib.dvsg_shake_workspace_bytes(a["n"], a["H"], a["W"], a["factor"], a["radius"], a["margin_y"], a["margin_x"],
                                        ctypes.byref(out))
    return rc, out.value, lib.dvsg_last_error_string().decode()


def measure_call(lib, luma=4096, pitch=None, frame_stride=None, texture=256, min_blocks=8, vectors=None, blocks=None,
                 workspace=4096, workspace_bytes=1 << 40, **kw):
    """dvsg_shake_measure_u8 with made-up device addresses: every refusal comes before they would be used."""
    a = dict(GOOD, **kw)
    pitch = a["W"] if pitch is None else pitch
    frame_stride = a["H"] * pitch if frame_stride is None else frame_stride
    vectors = np.full((max(a["n"] - 1, 1), 4), -7, dtype=np.int32) if vectors is None else vectors
    vp = vectors.ctypes.data if isinstance(vectors, np.ndarray) else vectors
    rc = lib.dvsg_shake_measure_u8(luma, pitch, frame_stride, a["n"], a["H"], a["W"], a["factor"], a["radius"], a["margin_y"],
                                   a["margin_x"], texture, min_blocks, vp, blocks, workspace, workspace_bytes)
    if isinstance(vectors, np.ndarray):
        assert (vectors == -7).all(), "a refused call wrote to vectors_host"
    return rc, lib.dvsg_last_error_string().decode()


def test_workspace_bytes_and_its_refusals(lib):
    rc, got, _ = workspace_bytes(lib)
    # two reduced planes of 270 x 480 (a multiple of 16), 264 block rows of 3 int32, one vector row
    assert rc == 0 and got == 2 * 270 * 480 + 264 * 12 + 16
    rc, got, _ = workspace_bytes(lib, n=5, H=125, W=203, factor=3, radius=5, margin_y=5, margin_x=6)
    # 41 x 67 planes at a stride of 2752, ny = 1, nx = 3: 4 x 3 block rows = 144 bytes, 4 vector rows
    assert rc == 0 and got == 5 * 2752 + 144 + 64
    for change, words in GEOMETRY_REFUSALS:
        rc, got, text = workspace_bytes(lib, **change)
        assert rc == -1 and got == 12345, change
        assert "dvsg_shake_workspace_bytes" in text and all(w in text for w in words), (change, text)
    a = GOOD
    assert lib.dvsg_shake_workspace_bytes(a["n"], a["H"], a["W"], a["factor"], a["radius"], a["margin_y"], a["margin_x"], None) == -1
    assert "NULL bytes" in lib.dvsg_last_error_string().decode()


def test_measure_refuses_every_bad_argument_before_any_device_work(lib):
    for change, words in GEOMETRY_REFUSALS:
        rc, text = measure_call(lib, **change)
        assert rc == -1, change
        assert "dvsg_shake_measure_u8" in text and all(w in text for w in words), (change, text)
    for kw, status, words in [
            (dict(luma=None), -1, ["NULL pointer"]),
            (dict(vectors=0), -1, ["NULL pointer"]),
            (dict(pitch=1919), -1, ["pitch=1919", "W=1920"]),
            (dict(pitch=2048, frame_stride=1079 * 2048 + 1919), -1, ["frame_stride=2211711", "2211712"]),
            (dict(texture=-1), -1, ["texture=-1"]),
            (dict(min_blocks=0), -1, ["min_blocks=0"]),
            (dict(workspace=None), -1, ["NULL workspace"]),
            (dict(workspace=4104), -3, ["16-byte aligned"]),
            (dict(workspace_bytes=2 * 270 * 480 + 264 * 12 + 16 - 1), -3, ["262383 bytes", "262384 needed", "dvsg_shake_workspace_bytes"]),
            (dict(workspace_bytes=0), -3, ["0 bytes"])]:
        rc, text = measure_call(lib, **kw)
        assert rc == status, (kw, rc, text)
        assert "dvsg_shake_measure_u8" in text and all(w in text for w in words), (kw, text)


# ---- the command line ---------------------------------------------------------------------------------------------

def run_cli(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.shake"] + list(argv), capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=120)


def test_help_runs():
    out = run_cli("--help")
    assert out.returncode == 0, out.stderr[-2000:]
    for word in ("--radius", "--factor", "--margin", "--texture", "--min-blocks", "--json", "--format", "--size"):
        assert word in out.stdout, word


def y4m_file(path, W, H, n=2):
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip C420jpeg\n" % (W, H))
        for _ in range(n):
            f.write(b"FRAME\n" + bytes(W * H * 3 // 2))
    return str(path)


def test_two_files_of_different_sizes_are_refused_cleanly(tmp_path, capsys):
    """Decided from the two headers: status 1 and one line, no device, no traceback."""
    from coupe.dvsg_amd import shake
    a, b = y4m_file(tmp_path / "a.y4m", 96, 64), y4m_file(tmp_path / "b.y4m", 64, 64)
    assert shake.main([a, b]) == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "differ in size" in err and "96x64" in err and "64x64" in err
    assert shake.main([a, a, a]) == 1 and "one clip or two" in capsys.readouterr().err
    assert shake.main([str(tmp_path / "missing.y4m")]) == 1 and "missing.y4m" in capsys.readouterr().err
    assert shake.main([a, "--format", "nv12"]) == 1 and "--size" in capsys.readouterr().err
