"""No-GPU checks of the shake motion measurement (include/dvsg_amd.h "SHAKE MOTION"): that the NumPy restatement
tests/shake_motion_ref.py is a meaningful reference for tests/test_gpu_shake_motion.py -- its sums are those of a brute-force
least-squares similarity in exact rationals, every edge of the rule behaves as written, and on warped textures the roll, the
zoom and the wobble that were applied come back -- and the host side of coupe.dvsg_amd.shake: motion_figures, motion_summary
and compare_motion equal the reference's exactly, dvsg_shake_motion_u8 refuses its bad arguments before any device work, and
the command line refuses --gate without --motion.

The rule's `Qn > 0` only ever bites together with `N >= 3`: Qn = N sum |p - mean p|^2 is zero only when all inliers are one
block.  A single row (Y = 0 only) or a single column of three or more blocks has Qn > 0 and IS fit -- points on a line still
fix a similarity -- and the cases below assert that, with the roll and the zoom of such a row coming back exactly.

Observed on the recipe's planes (270 x 480 of shake_ref.texture(7, 350, 560), f = 1, R = 12, margins (34, 60), 264 blocks, all
valid), roll / zoom / wobble in reduced pixels:
  identity 0 / 0 / 0.004;  angle 0.005: 0.00499 / 0 / 0.156;  angle 0.01, t = (1.5, -2.25): 0.01004 / 0 / 0.150;
  scale 1.01: -0.00005 / 0.01014 / 0.151;  angle -0.008, scale 0.995, t = (3, 1): -0.00792 / -0.00500 / 0.145;
  bend amp 0: 0.068, amp 1: 0.438;  an 80 x 100 patch at (100, 200) moving by (6, -6): gate 64 n_in 234, 0.069; gate 400 n_in
  264, 2.69."""
import ctypes
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import shake_motion_ref as ref
import shake_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def random_blocks(seed, ny, nx, invalid=0.2, spread=40):
    """int32 [ny * nx, 3]: vectors around a common motion with a roll and a zoom in them, some blocks invalid"""
    rng = np.random.RandomState(seed)
    rows = []
    for a in range(ny):
        for c in range(nx):
            X, Y = 2 * c - (nx - 1), 2 * a - (ny - 1)
            vx = 37 + 3 * X - 2 * Y + rng.randint(-spread, spread + 1)
            vy = -21 + 2 * X + 3 * Y + rng.randint(-spread, spread + 1)
            rows.append((vx, vy, 1) if rng.rand() >= invalid else (0, 0, 0))
    return np.array(rows, dtype=np.int32)


def inliers(blocks, ny, nx, row, gate):
    """[(X, Y, vx, vy), ...] of the blocks the rule lets into the fit, written out once more, from the row's own median"""
    gx, gy = int(row[0]), int(row[1])
    out = []
    for i, (vx, vy, valid) in enumerate(blocks.tolist()):
        if valid and row[3] and abs(vx - gx) <= gate and abs(vy - gy) <= gate:
            out.append((2 * (i % nx) - (nx - 1), 2 * (i // nx) - (ny - 1), vx, vy))
    return out


@pytest.mark.parametrize("seed,ny,nx,gate", [(1, 5, 7, 1000), (2, 5, 7, 30), (3, 2, 3, 25), (4, 12, 22, 20), (5, 1, 6, 1000),
                                             (6, 6, 1, 1000)])
def test_the_sums_are_those_of_a_least_squares_similarity(seed, ny, nx, gate):
    blocks = random_blocks(seed, ny, nx)
    row = ref.motion_row(blocks, ny, nx, 1, gate)
    points = inliers(blocks, ny, nx, row, gate)
    assert int(row[4]) == len(points) >= 3
    if gate < 1000:
        assert len(points) < int(row[2]), "the gate drops nothing: the case does not test it"
    (tx, ty, p, r), rss = ref.least_squares(points)
    N, Pn, Rn, Qn, got_rss = ref.fit(row, 1)
    assert Fraction(Pn, Qn) == p and Fraction(Rn, Qn) == r and got_rss == rss
    fig = ref.figures(row, 1, 1)
    assert fig == dict(fit=True, zoom=float(p / 128), roll=float(r / 128), wobble=1 / 16 * math.sqrt(float(rss / N)))
    # the translation is not part of the row's figures, but the sums hold it: mean v = t + p mean X -+ r mean Y
    assert Fraction(int(row[7]), N) == tx + p * Fraction(int(row[5]), N) - r * Fraction(int(row[6]), N)
    assert Fraction(int(row[8]), N) == ty + r * Fraction(int(row[5]), N) + p * Fraction(int(row[6]), N)


def exact_blocks(ny, nx, p, r, tx=5, ty=-9):
    """Every block valid, on the similarity (tx, ty) + (p X - r Y, r X + p Y) exactly"""
    return np.array([(tx + p * (2 * c - (nx - 1)) - r * (2 * a - (ny - 1)), ty + r * (2 * c - (nx - 1)) + p * (2 * a - (ny - 1)), 1)
                     for a in range(ny) for c in range(nx)], dtype=np.int32)


def test_an_exact_similarity_comes_back_with_no_wobble():
    row = ref.motion_row(exact_blocks(4, 5, 3, -2), 4, 5, 8, 1000)
    # the lower medians (rank 9 of 20): 3 X + 2 Y has ... -2 0 | 0 2 ... around its middle, -2 X + 3 Y has ... -1 -1 | 1 1 ...
    assert row[:5].tolist() == [5 + 0, -9 - 1, 20, 1, 20]
    assert row[5:7].tolist() == [0, 0]                           # Sx = Sy = 0: the grid is centred
    assert ref.figures(row, 2, 8) == dict(fit=True, zoom=3 / 128, roll=-2 / 128, wobble=0.0)


def test_a_block_at_the_gate_is_in_and_one_beyond_it_is_out():
    blocks = np.array([(0, 0, 1)] * 9, dtype=np.int32)
    blocks[5], blocks[6], blocks[7], blocks[8] = (10, 0, 1), (11, 0, 1), (0, -10, 1), (0, -11, 1)
    row = ref.motion_row(blocks, 3, 3, 1, 10)
    assert row[:5].tolist() == [0, 0, 9, 1, 7]
    # X of the grid's columns is -2 0 2, Y of its rows -2 0 2.  Out: blocks 6 at (X, Y) = (-2, 2) and 8 at (2, 2).  Of the
    # rest only 5 at (2, 0) with (10, 0) and 7 at (0, 2) with (0, -10) move: Sxu = 2 * 10 + 2 * -10, Sxv = 0.
    assert row[5:].tolist() == [0 + 2 - 2, 0 - 2 - 2, 10, -10, 48 - 8 - 8, 0, 0, 200]
    assert ref.motion_row(blocks, 3, 3, 1, 11)[4] == 9 and ref.motion_row(blocks, 3, 3, 1, 9)[4] == 5
    assert ref.motion_row(blocks, 3, 3, 1, 0)[4] == 5              # gate 0: only the blocks on the median itself


def test_too_few_inliers_and_a_single_block_are_unfit():
    unfit = dict(fit=False, zoom=None, roll=None, wobble=None)
    one = ref.motion_row(np.array([(7, -3, 1)], dtype=np.int32), 1, 1, 1, 64)
    assert one.tolist() == [7, -3, 1, 1, 1, 0, 0, 7, -3, 0, 0, 0, 58]    # X = Y = 0: every product with them is 0
    assert ref.fit(one, 1) is None and ref.figures(one, 1, 1) == unfit       # N = 1, and Qn = 0
    two = ref.motion_row(np.array([(7, -3, 1), (0, 0, 0), (9, -3, 1)], dtype=np.int32), 1, 3, 1, 64)
    assert two[4] == 2 and ref.figures(two, 1, 1) == unfit                   # N = 2 < 3 whatever min_blocks
    # N below min_blocks although the pair is ok: 9 valid, the gate keeps 7
    blocks = np.array([(0, 0, 1)] * 9, dtype=np.int32)
    blocks[6], blocks[8] = (99, 0, 1), (0, 99, 1)
    row = ref.motion_row(blocks, 3, 3, 8, 10)
    assert row[2:5].tolist() == [9, 1, 7] and ref.figures(row, 1, 8) == unfit and ref.figures(row, 1, 7)["fit"]


def test_one_row_and_one_column_of_blocks_are_fit():
    """Y = 0 only, or all inliers in one column: Qn > 0 for three blocks or more, and the similarity is the one applied."""
    row = ref.motion_row(exact_blocks(1, 5, 4, 1), 1, 5, 3, 1000)
    assert row[6] == 0 and ref.fit(row, 3)[3] > 0
    assert ref.figures(row, 1, 3) == dict(fit=True, zoom=4 / 128, roll=1 / 128, wobble=0.0)
    column = exact_blocks(5, 3, -2, 3)
    column[[i for i in range(15) if i % 3 != 1]] = (0, 0, 0)             # only the middle column is valid
    row = ref.motion_row(column, 5, 3, 3, 1000)
    assert row[4] == 5 and row[5] == 0 and ref.figures(row, 1, 3) == dict(fit=True, zoom=-2 / 128, roll=3 / 128, wobble=0.0)


def test_a_pair_that_is_not_ok_has_a_zero_tail():
    blocks = random_blocks(8, 3, 4, invalid=0.0)
    row = ref.motion_row(blocks, 3, 4, 13, 1000)
    assert row.tolist() == [0, 0, 12, 0] + [0] * 9 and not ref.figures(row, 1, 1)["fit"]
    assert ref.motion_row(blocks, 3, 4, 12, 1000)[3:5].tolist() == [1, 12]
    none = ref.motion_row(np.zeros((12, 3), dtype=np.int32), 3, 4, 1, 1000)
    assert none.tolist() == [0] * 13


def hand_rows():
    """Seven pairs on a 4 x 5 grid: fit, fit, not ok, fit, too few inliers, fit, fit"""
    if "rows" not in _CACHE:
        rows = []
        for k, (p, r) in enumerate([(3, -2), (1, 1), (0, 0), (-2, 4), (0, 0), (2, 2), (5, -1)]):
            blocks = exact_blocks(4, 5, p, r, tx=k, ty=-k)
            blocks[:, :2] += np.random.RandomState(k).randint(-3, 4, size=(20, 2)).astype(np.int32)
            if k == 2:
                blocks[3:] = (0, 0, 0)                       # 3 valid blocks of the 8 it needs
            if k == 4:
                blocks[:, 0] += 100 * np.arange(20, dtype=np.int32)   # ok, but no two blocks agree: hardly an inlier
            rows.append(ref.motion_row(blocks, 4, 5, 8, 24))
        _CACHE["rows"] = np.stack(rows)
    return _CACHE["rows"]


def test_the_summary_leaves_unfit_pairs_out():
    rows = hand_rows()
    figs = [ref.figures(r, 2, 8) for r in rows]
    assert [f["fit"] for f in figs] == [True, True, False, True, False, True, True]
    assert rows[2, 3] == 0 and rows[4, 3] == 1 and rows[4, 4] < 8
    s = ref.summary(rows, 2, 8)
    assert (s["frames"], s["pairs"], s["unfit"]) == (8, 7, 2)
    fit = [f for f in figs if f["fit"]]
    assert s["roll_rms_deg"] == math.degrees(math.sqrt(math.fsum(f["roll"] ** 2 for f in fit) / 5))
    # consecutive and both fit: pairs (0, 1) and (5, 6) only
    d = [figs[1]["roll"] - figs[0]["roll"], figs[6]["roll"] - figs[5]["roll"]]
    assert s["roll_jitter_deg"] == math.degrees(math.sqrt(math.fsum(v * v for v in d) / 2))
    z = [figs[1]["zoom"] - figs[0]["zoom"], figs[6]["zoom"] - figs[5]["zoom"]]
    assert s["zoom_jitter_pct"] == 100 * math.sqrt(math.fsum(v * v for v in z) / 2)
    have = [ref.fit(r, 8) for r in rows if ref.fit(r, 8) is not None]
    assert s["wobble_rms"] == 2 / 16 * math.sqrt(math.fsum(float(x[4]) for x in have) / sum(x[0] for x in have)) > 0
    empty = ref.summary(rows[2:3], 2, 8)
    assert empty == dict(frames=2, pairs=1, unfit=1, roll_rms_deg=None, roll_jitter_deg=None, zoom_jitter_pct=None, wobble_rms=None)
    alone = ref.summary(rows[:1], 2, 8)
    assert alone["roll_jitter_deg"] is None and alone["zoom_jitter_pct"] is None and alone["roll_rms_deg"] is not None


# ---- coupe.dvsg_amd.shake on the host -----------------------------------------------------------------------------

def test_the_host_figures_equal_the_references():
    from coupe.dvsg_amd import shake
    rows = hand_rows()
    extra = np.stack([ref.motion_row(random_blocks(s, 12, 22), 12, 22, 8, 64) for s in range(20, 26)])
    for which, grid in ((rows, (4, 5)), (extra, (12, 22))):
        for f, min_blocks in ((1, 8), (4, 8), (3, 1), (2, 300)):
            track = shake.MotionTrack(which, f, (1080, 1920), grid, None)
            for r in which:
                assert shake.motion_figures(r, f, min_blocks) == ref.figures(r, f, min_blocks)
            assert shake.motion_summary(track, min_blocks) == ref.summary(which, f, min_blocks)
    assert any(ref.figures(r, 1, 8)["fit"] for r in extra)
    assert shake.motion_figures(rows[0]) == ref.figures(rows[0], 1, 8)       # the defaults: reduced pixels, 8 blocks
    a, b = shake.MotionTrack(rows, 2, (540, 960), (4, 5), None), shake.MotionTrack(rows[::-1].copy(), 2, (540, 960), (4, 5), None)
    got = shake.compare_motion(a, b)
    assert got == ref.compare(rows, rows[::-1], 2, 8)
    assert got["roll_jitter_ratio"] == got["b"]["roll_jitter_deg"] / got["a"]["roll_jitter_deg"]
    assert got["wobble_ratio"] == got["b"]["wobble_rms"] / got["a"]["wobble_rms"]
    lost = shake.MotionTrack(rows[2:3], 2, (540, 960), (4, 5), None)
    none = shake.compare_motion(a, lost)
    assert none["roll_jitter_ratio"] is None and none["wobble_ratio"] is None and none == ref.compare(rows, rows[2:3], 2, 8)
    assert shake.compare_motion(lost, a)["wobble_ratio"] is None
    # a's wobble is 0: no ratio
    still = np.stack([ref.motion_row(exact_blocks(4, 5, p, 0), 4, 5, 8, 1000) for p in (1, 2, 3)])
    zero = shake.compare_motion(shake.MotionTrack(still, 2, (540, 960), (4, 5), None), a)
    assert zero["a"]["wobble_rms"] == 0.0 and zero["wobble_ratio"] is None and zero == ref.compare(still, rows, 2, 8)


# ---- the C entry points, before any device work -------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


GOOD = dict(n=2, H=1080, W=1920, factor=4, radius=12, margin_y=34, margin_x=60)
NEED = 2 * 270 * 480 + 264 * 12 + 13 * 8       # two reduced planes (a multiple of 16), 264 block rows, one row of 13 int64


def test_the_two_names_are_bound_exported_and_documented(lib):
    from coupe.dvsg_amd import _lib
    for name in ("dvsg_shake_motion_workspace_bytes", "dvsg_shake_motion_u8"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["dvsg_shake_motion_workspace_bytes"]) == 8 and len(_lib.SIGNATURES["dvsg_shake_motion_u8"]) == 17
    assert lib.dvsg_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "dvsg_amd.h")).read()
    start = header.index("int dvsg_shake_motion_workspace_bytes(")
    block = " ".join(header[header.index(" * SHAKE MOTION"):start].replace("\n *", " ").split())
    for words in ("synchronous and takes no stream", "every argument is checked before any HIP call", "waits for the device",
                  "three kernels on the legacy default stream", "copies the results to the host", "allocates and frees nothing"):
        assert words in block, words
    declaration = header[start:header.index(";", header.index("int dvsg_shake_motion_u8("))]
    assert "stream" not in declaration and "int gate, int64_t *motion_host" in declaration


def motion_workspace_bytes(lib, **kw):
    a = dict(GOOD, **kw)
    out = ctypes.c_size_t(12345)
    rc = lib.dvsg_shake_motion_workspace_bytes(a["n"], a["H"], a["W"], a["factor"], a["radius"], a["margin_y"], a["margin_x"],
                                               ctypes.byref(out))
    return rc, out.value, lib.dvsg_last_error_string().decode()


def motion_call(lib, luma=4096, pitch=None, frame_stride=None, texture=256, min_blocks=8, gate=64, motion=None, workspace=4096,
                workspace_bytes=1 << 40, **kw):
    """dvsg_shake_motion_u8 with made-up device addresses: every refusal comes before they would be used."""
    a = dict(GOOD, **kw)
    pitch = a["W"] if pitch is None else pitch
    frame_stride = a["H"] * pitch if frame_stride is None else frame_stride
    motion = np.full((max(a["n"] - 1, 1), 13), -7, dtype=np.int64) if motion is None else motion
    mp = motion.ctypes.data if isinstance(motion, np.ndarray) else motion
    rc = lib.dvsg_shake_motion_u8(luma, pitch, frame_stride, a["n"], a["H"], a["W"], a["factor"], a["radius"], a["margin_y"],
                                  a["margin_x"], texture, min_blocks, gate, mp, None, workspace, workspace_bytes)
    if isinstance(motion, np.ndarray):
        assert (motion == -7).all(), "a refused call wrote to motion_host"
    return rc, lib.dvsg_last_error_string().decode()


def test_the_size_query(lib):
    rc, got, _ = motion_workspace_bytes(lib)
    assert rc == 0 and got == NEED
    rc, got, _ = motion_workspace_bytes(lib, n=5, H=125, W=203, factor=3, radius=5, margin_y=5, margin_x=6)
    assert rc == 0 and got == 5 * 2752 + 144 + 4 * 13 * 8            # tests/test_shake_cpu.py's figures, rows of 13 int64
    rc, got, text = motion_workspace_bytes(lib, factor=1)
    assert rc == -1 and got == 12345 and "dvsg_shake_motion_workspace_bytes" in text and "7056 blocks" in text
    a = GOOD
    assert lib.dvsg_shake_motion_workspace_bytes(a["n"], a["H"], a["W"], a["factor"], a["radius"], a["margin_y"], a["margin_x"],
                                                 None) == -1
    assert "NULL bytes" in lib.dvsg_last_error_string().decode()


def test_motion_refuses_every_bad_argument_before_any_device_work(lib):
    for kw, status, words in [
            (dict(gate=-1), -1, ["gate=-1"]),
            (dict(gate=(1 << 20) + 1), -1, ["gate=1048577", "1048576"]),
            (dict(motion=0), -1, ["NULL motion_host"]),
            (dict(luma=None), -1, ["NULL luma"]),
            (dict(n=1), -1, ["n=1"]),
            (dict(margin_x=11), -1, ["margin_x=11", "radius=12"]),
            (dict(pitch=1919), -1, ["pitch=1919", "W=1920"]),
            (dict(pitch=2048, frame_stride=1079 * 2048 + 1919), -1, ["frame_stride=2211711", "2211712"]),
            (dict(texture=-1), -1, ["texture=-1"]),
            (dict(min_blocks=0), -1, ["min_blocks=0"]),
            (dict(workspace=None), -1, ["NULL workspace"]),
            (dict(workspace=4104), -3, ["workspace", "16-byte aligned"]),
            (dict(workspace_bytes=NEED - 1), -3, ["workspace", "%d bytes" % (NEED - 1), "%d needed" % NEED,
                                                  "dvsg_shake_motion_workspace_bytes"]),
            # what dvsg_shake_workspace_bytes reports is short by the wider rows
            (dict(workspace_bytes=2 * 270 * 480 + 264 * 12 + 16), -3, ["dvsg_shake_motion_workspace_bytes"])]:
        rc, text = motion_call(lib, **kw)
        assert rc == status, (kw, rc, text)
        assert "dvsg_shake_motion_u8" in text and all(w in text for w in words), (kw, text)
    assert motion_call(lib, gate=0, workspace_bytes=0)[0] == -3 and motion_call(lib, gate=1 << 20, workspace_bytes=0)[0] == -3


# ---- the command line ---------------------------------------------------------------------------------------------

def run_cli(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.shake"] + list(argv), capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=120)


def test_help_names_the_two_options():
    out = run_cli("--help")
    assert out.returncode == 0, out.stderr[-2000:]
    text = " ".join(out.stdout.split())
    for word in ("--motion", "--gate N", "roll", "zoom", "wobble", "sixteenths"):
        assert word in text, word


def test_gate_without_motion_is_a_usage_error(tmp_path, capsys):
    from coupe.dvsg_amd import shake
    path = tmp_path / "a.y4m"
    path.write_bytes(b"YUV4MPEG2 W96 H64 F25:1 Ip C420jpeg\n" + (b"FRAME\n" + bytes(96 * 64 * 3 // 2)) * 2)
    assert shake.main([str(path), "--gate", "32"]) == 1
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "--gate" in err and "--motion" in err
    assert shake.main([str(tmp_path / "missing.y4m"), "--gate", "32"]) == 1           # before any file is opened
    assert "--motion" in capsys.readouterr().err


# ---- the recipe: the rule measures what it claims -----------------------------------------------------------------

H, W, PAD = 270, 480, 40
WARPS = [dict(), dict(angle=0.005), dict(angle=0.01, t=(1.5, -2.25)), dict(scale=1.01), dict(angle=-0.008, scale=0.995, t=(3, 1))]
PATCH = (100, 200, 80, 100, 6, -6)


def recipe(cur_of, gate=64):
    """(row, figures in reduced pixels) of `cur` against the unwarped plane: f = 1, R = 12, margins (34, 60), 12 x 22 blocks"""
    if "tex" not in _CACHE:
        _CACHE["tex"] = shake_ref.texture(7, 350, 560)
        _CACHE["prev"] = shake_ref.shifted(_CACHE["tex"], 0, 0, H, W, PAD)
        assert shake_ref.default_geometry(H, W) == (1, 34, 60)
    rows, blocks = ref.measure(np.stack([_CACHE["prev"], cur_of(_CACHE["tex"])]), 1, 12, 34, 60, 256, 8, gate)
    assert blocks.shape == (1, 264, 3)
    return rows[0], ref.figures(rows[0], 1, 8)


def bent(amp, patch=None, gate=64):
    key = ("bent", amp, patch, gate)
    if key not in _CACHE:
        _CACHE[key] = recipe(lambda tex: ref.bend_plane(tex, H, W, PAD, amp, patch), gate)
    return _CACHE[key]


@pytest.mark.parametrize("warp", WARPS, ids=lambda w: "-".join("%s=%s" % kv for kv in w.items()) or "identity")
def test_roll_and_zoom_come_back(warp):
    row, fig = recipe(lambda tex: ref.similarity_plane(tex, H, W, PAD, **warp))
    angle, scale = warp.get("angle", 0.0), warp.get("scale", 1.0)
    print(warp, row.tolist(), fig)
    assert row[2] == row[4] == 264 and fig["fit"]
    assert abs(fig["roll"] - scale * math.sin(angle)) <= 3e-4
    assert abs(fig["zoom"] - (scale * math.cos(angle) - 1)) <= 3e-4
    if not warp:
        assert fig["wobble"] <= 0.01


def test_a_bend_is_wobble():
    flat, bend = bent(0)[1], bent(1)[1]
    print(flat, bend)
    assert flat["fit"] and bend["fit"] and bend["wobble"] >= 3 * flat["wobble"] > 0


def test_the_gate_keeps_a_moving_patch_out_of_the_fit():
    free = bent(0)[1]
    row, fig = bent(0, PATCH)
    wide_row, wide = bent(0, PATCH, gate=400)
    print(row.tolist(), fig, wide_row.tolist(), wide)
    assert row[4] < row[2] == 264 and abs(fig["wobble"] - free["wobble"]) <= 0.01
    assert wide_row[4] == 264 and wide["wobble"] > 1
