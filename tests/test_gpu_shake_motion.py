"""GPU: dvsg_shake_motion_u8 and coupe.dvsg_amd.shake.measure_motion against the NumPy restatement
tests/shake_motion_ref.py, bit for bit: all 13 columns of every pair and, where requested, every block -- the rule is integer
arithmetic, so there is no tolerance.  tests/test_shake_motion_cpu.py checks that the reference is meaningful; here every case
asserts on the reference what makes it a case (a gate that cuts, 2048 blocks, a pair with no valid block), so no comparison is
of zeros against zeros by accident.

Shapes: one block at R = 1 (X = Y = 0, every product 0); a 2 x 3 grid (the centring of an even and of an odd count); a 5 x 7
grid over three frames of a rolled and zoomed texture, with a gate that keeps everything and with one taken from the
reference's own block rows so that a block lies exactly on it and another beyond; 32 x 64 = 2048 blocks, the rank count and
the sums at their largest; a factor that divides neither side; rows at a pitch of W + 5 from an odd address with poison
between; three pairs whose middle one has no valid block.

On the 2048-block case: with every block an inlier Sxx = sum (X^2 + Y^2) is 3,493,888 there, and it cannot pass 2^31 at any
size the call accepts: a side is at most 16384, so a grid is at most 1023 blocks wide, |X| <= 1022, and one row of 1023 blocks
has Sxx = 356,866,048; with |v| <= 248 sixteenths, |Sxu| <= 129,769,472 and Suu <= 251,920,384.  The sums of a row therefore
fit 32 bits and the row is int64 for headroom and for the products the host makes of them (N Sxx passes 2^31 here, which the
case asserts).  The case asserts the reference's Sxx as computed, not a bound it cannot reach.

On the pair with no valid block: a flat plane would void both pairs it belongs to, so the middle pair is a jump by the
radius instead (every minimum on the search boundary); two flat planes are a case of their own."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shake_motion_ref as ref
import shake_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xAB
ALL = 1 << 20          # the largest gate: every valid block of an ok pair is an inlier
_CACHE = {}


def call(planes, f, R, my, mx, texture, min_blocks, gate, layout=(0, 0, 0), workspace=None):
    """dvsg_shake_motion_u8 on the planes laid out at pitch W + layout[0], frame stride H pitch + layout[1], from a base
    layout[2] bytes into the buffer, poison everywhere else.  Returns (rows int64 [n - 1, 13], blocks int32 [n - 1, n_blk, 3]);
    both arrays start as -7."""
    import torch
    from coupe.dvsg_amd import _lib
    lib = _lib.load()
    n, H, W = planes.shape
    pitch = W + layout[0]
    frame_stride = H * pitch + layout[1]
    host = np.full(layout[2] + n * frame_stride + 64, POISON, dtype=np.uint8)
    for t in range(n):
        rows = np.lib.stride_tricks.as_strided(host[layout[2] + t * frame_stride:], shape=(H, W), strides=(pitch, 1))
        rows[...] = planes[t]
    dev = torch.from_numpy(host).cuda()
    need = ctypes.c_size_t()
    _lib.call("dvsg_shake_motion_workspace_bytes", n, H, W, f, R, my, mx, ctypes.byref(need))
    if workspace is None:
        workspace = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert workspace.numel() >= need.value
    ny, nx = shake_ref.block_counts(H // f, W // f, my, mx)
    motion = np.full((n - 1, 13), -7, dtype=np.int64)
    blocks = np.full((n - 1, ny * nx, 3), -7, dtype=np.int32)
    rc = lib.dvsg_shake_motion_u8(dev.data_ptr() + layout[2], pitch, frame_stride, n, H, W, f, R, my, mx, texture, min_blocks, gate,
                                  motion.ctypes.data, blocks.ctypes.data, workspace.data_ptr(), workspace.numel())
    assert rc == 0, lib.dvsg_last_error_string().decode()
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host), "the call wrote to its input"
    return motion, blocks


def same(got, want):
    got_rows, got_blocks = got
    want_rows, want_blocks = want
    assert got_blocks.shape == want_blocks.shape and got_blocks.dtype == want_blocks.dtype == np.int32
    bad = np.argwhere((got_blocks != want_blocks).any(axis=2))
    assert len(bad) == 0, "%d block(s) differ, first (pair, block) %s: got %s, want %s" % (
        len(bad), bad[0].tolist(), got_blocks[tuple(bad[0])].tolist(), want_blocks[tuple(bad[0])].tolist())
    assert got_rows.dtype == want_rows.dtype == np.int64 and got_rows.shape == want_rows.shape
    for t, (g, w) in enumerate(zip(got_rows.tolist(), want_rows.tolist())):
        assert g == w, "pair %d: %s" % (t, ", ".join("%s got %d want %d" % (c, a, b) for c, a, b in zip(ref.COLUMNS, g, w) if a != b))


def check(planes, f, R, my, mx, texture, min_blocks, gate, layout=(0, 0, 0)):
    want = ref.measure(planes, f, R, my, mx, texture, min_blocks, gate)
    print("gate %d: %d block(s), rows %s" % (gate, want[1].shape[1], want[0].tolist()))
    same(call(planes, f, R, my, mx, texture, min_blocks, gate, layout), want)
    return want


def warped_clip(seed, H, W, warps, pad=8, box=5):
    """Frame 0 is the texture's window; frame k sees it through warps[k - 1] (shake_motion_ref.similarity_plane)"""
    tex = shake_ref.texture(seed, H + 2 * pad, W + 2 * pad, box=box)
    return np.stack([shake_ref.shifted(tex, 0, 0, H, W, pad)] + [ref.similarity_plane(tex, H, W, pad, **w) for w in warps])


def test_one_block():
    """ny = nx = 1 at R = 1: X = Y = 0, so Sx, Sy, Sxx, Sxu and Sxv are 0 whatever the vector"""
    planes = warped_clip(41, 18, 18, [dict(t=(0.25, 0.375))])
    rows, _ = check(planes, 1, 1, 1, 1, 16, 1, 64)
    assert rows[0, 2:5].tolist() == [1, 1, 1] and rows[0, :2].any()
    assert rows[0, 5:7].tolist() == [0, 0] and rows[0, 9:12].tolist() == [0, 0, 0] and rows[0, 12] > 0


def test_a_2_x_3_grid():
    """The centring of an even count (Y = -1, 1) and of an odd one (X = -2, 0, 2)"""
    planes = warped_clip(42, 40, 56, [dict(angle=0.02, scale=1.02, t=(1.25, -0.5))])
    rows, blocks = check(planes, 1, 4, 4, 4, 16, 1, ALL)
    assert blocks.shape[1] == 6 and rows[0, 2:5].tolist() == [6, 1, 6]
    assert rows[0, 5:7].tolist() == [0, 0] and rows[0, 9] == 4 * 4 + 6 * 1
    assert len(set(map(tuple, blocks[0, :, :2].tolist()))) > 1, "the vectors do not differ per block"


def clip_5x7():
    if "5x7" not in _CACHE:
        planes = warped_clip(43, 96, 128, [dict(angle=0.01, scale=1.01), dict(angle=-0.01, scale=1.01, t=(0.5, 1.0))])
        _, blocks = shake_ref.measure(planes, 1, 4, 4, 4, 64, 8)
        _CACHE["5x7"] = planes, blocks
    return _CACHE["5x7"]


def test_a_5_x_7_grid_with_a_gate_that_keeps_every_block():
    planes, blocks = clip_5x7()
    assert blocks.shape == (2, 35, 3)
    rows, _ = check(planes, 1, 4, 4, 4, 64, 8, ALL)
    assert (rows[:, 3] == 1).all() and (rows[:, 4] == rows[:, 2]).all() and (rows[:, 2] >= 30).all()
    for b in blocks:
        assert len(set(map(tuple, b[b[:, 2] == 1, :2].tolist()))) >= 10, "the vectors hardly differ per block"
    fig = ref.figures(rows[0], 1, 8)
    assert fig["fit"] and abs(fig["roll"] - 0.0101) < 2e-3 and abs(fig["zoom"] - 0.01) < 2e-3      # the case is what it says


def test_a_5_x_7_grid_with_a_block_exactly_on_the_gate():
    planes, blocks = clip_5x7()
    first = blocks[0][blocks[0][:, 2] == 1]
    gx, gy = shake_ref.lower_median(first[:, 0]), shake_ref.lower_median(first[:, 1])
    distance = np.maximum(np.abs(first[:, 0] - gx), np.abs(first[:, 1] - gy))
    values = sorted(set(distance.tolist()))
    gate = values[len(values) // 2]
    assert (distance == gate).any() and (distance > gate).any() and gate > 0
    rows, _ = check(planes, 1, 4, 4, 4, 64, 8, gate)
    assert 0 < rows[0, 4] < rows[0, 2] and rows[0, 4] == (distance <= gate).sum()
    assert ref.motion_row(blocks[0], 5, 7, 8, gate + 1)[4] >= rows[0, 4] > ref.motion_row(blocks[0], 5, 7, 8, gate - 1)[4]
    assert (rows[:, 3] == 1).all() and (rows[:, 4] > 0).all()


def test_2048_blocks():
    """32 x 64 blocks at R = 1: a sub-pixel shift and a slight roll, so every vector is a sixteenth-pel step of its own.  The
    module docstring has why Sxx is asserted as computed."""
    planes = warped_clip(44, 514, 1026, [dict(angle=0.0004, t=(0.2, -0.15))], pad=4)
    rows, blocks = check(planes, 1, 1, 1, 1, 16, 8, ALL)
    assert blocks.shape == (1, 2048, 3)
    n_valid, ok, n_in = rows[0, 2:5].tolist()
    assert ok == 1 and n_in == n_valid >= 1800
    assert len(set(map(tuple, blocks[0, :, :2].tolist()))) >= 20
    if n_in == 2048:
        assert rows[0, 9] == 3493888 and rows[0, 5] == rows[0, 6] == 0
    assert 3000000 < rows[0, 9] <= 3493888 < 1 << 31 and n_in * int(rows[0, 9]) > 1 << 31
    gated = check(planes, 1, 1, 1, 1, 16, 8, 2)[0]
    assert 0 < gated[0, 4] < n_valid


def test_a_factor_that_divides_neither_side():
    planes = warped_clip(45, 125, 203, [dict(angle=0.01, t=(3.0, -1.5)), dict(scale=1.02)], pad=12, box=17)
    rows, blocks = check(planes, 3, 5, 5, 6, 16, 1, ALL)
    assert blocks.shape == (2, 3, 3) and (rows[:, 2] >= 2).all() and rows[:, 9].all()


def test_a_pitch_of_w_plus_5_from_an_odd_address_with_poison_between():
    planes = warped_clip(46, 41, 67, [dict(angle=0.02, t=(-0.75, 1.5))])
    rows, blocks = check(planes, 1, 3, 3, 5, 16, 2, ALL, layout=(5, 37, 3))
    assert blocks.shape == (1, 6, 3) and rows[0, 3] == 1 and rows[0, 4] >= 4


def test_three_pairs_of_which_the_middle_one_has_no_valid_block():
    H, W, R, pad = 56, 88, 4, 8
    tex = shake_ref.texture(47, H + 2 * pad, W + 2 * pad)
    at = lambda oy, ox: shake_ref.shifted_subpel(tex, oy, ox, H, W, pad)
    planes = np.stack([at(0, 0), at(1, -0.5), at(1, -0.5 + R), at(1.75, R)])
    rows, blocks = check(planes, 1, R, 4, 4, 64, 4, ALL)
    assert rows[1].tolist() == [0] * 13 and not blocks[1].any()
    assert rows[0, 3] == rows[2, 3] == 1 and rows[0, 4] > 0 and rows[2, 4] > 0
    s = ref.summary(rows, 1, 4)
    assert s["unfit"] == 1 and s["roll_jitter_deg"] is None and s["roll_rms_deg"] is not None


def test_two_flat_planes():
    rows, blocks = check(np.full((2, 40, 56), 117, dtype=np.uint8), 1, 4, 4, 4, 16, 1, ALL)
    assert not rows.any() and not blocks.any()


def test_two_calls_on_one_workspace_keep_no_state():
    import torch
    planes, _ = clip_5x7()
    other = warped_clip(48, 96, 128, [dict(scale=0.99, t=(-1.0, 0.25))])
    small = warped_clip(42, 40, 56, [dict(angle=0.02, scale=1.02, t=(1.25, -0.5))])
    need = ctypes.c_size_t()
    from coupe.dvsg_amd import _lib
    _lib.call("dvsg_shake_motion_workspace_bytes", 3, 96, 128, 1, 4, 4, 4, ctypes.byref(need))
    ws = torch.full((need.value,), POISON, dtype=torch.uint8, device="cuda")
    args = (1, 4, 4, 4, 64, 8)
    want_a, want_b = ref.measure(planes, *args, 12), ref.measure(other, *args, ALL)
    assert want_a[0].tolist() != want_b[0].tolist()[:1] * 2
    same(call(planes, *args, 12, workspace=ws), want_a)
    same(call(other, *args, ALL, workspace=ws), want_b)                   # fewer pairs, another gate: nothing of A is left
    same(call(small, 1, 4, 4, 4, 16, 1, ALL, workspace=ws), ref.measure(small, 1, 4, 4, 4, 16, 1, ALL))   # another geometry
    same(call(planes, *args, 12, workspace=ws), want_a)


def test_columns_0_to_3_and_the_blocks_equal_the_existing_call():
    import torch
    from coupe.dvsg_amd import _lib
    planes, _ = clip_5x7()
    rows, blocks = call(planes, 1, 4, 4, 4, 64, 8, 12)
    n, H, W = planes.shape
    need = ctypes.c_size_t()
    _lib.call("dvsg_shake_workspace_bytes", n, H, W, 1, 4, 4, 4, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    dev = torch.from_numpy(planes).cuda()
    vectors = np.full((n - 1, 4), -7, dtype=np.int32)
    old_blocks = np.full((n - 1, 35, 3), -7, dtype=np.int32)
    _lib.call("dvsg_shake_measure_u8", dev.data_ptr(), W, H * W, n, H, W, 1, 4, 4, 4, 64, 8, vectors.ctypes.data,
              old_blocks.ctypes.data, ws.data_ptr(), need.value)
    assert rows[:, :4].tolist() == vectors.tolist() and vectors[:, 3].all() and vectors[:, :2].any()
    assert np.array_equal(blocks, old_blocks)


# ---- coupe.dvsg_amd.shake.measure_motion --------------------------------------------------------------------------

def clip_small():
    """6 frames of 56 x 88: a texture that wanders by integer and sub-pixel steps, with a slight roll on the way"""
    if "clip" not in _CACHE:
        warps = [dict(t=(1, -2)), dict(angle=0.01, t=(1.5, -1.25)), dict(t=(0, 0.5)), dict(scale=1.02, t=(-2, 2)), dict(t=(-2.25, 3))]
        _CACHE["clip"] = warped_clip(31, 56, 88, warps)
        assert shake_ref.default_geometry(56, 88, radius=4) == (1, 7, 11)
        _CACHE["clip_ref"] = ref.measure(_CACHE["clip"], 1, 4, 7, 11, 256, 2, 5)
    return _CACHE["clip"], _CACHE["clip_ref"]


def test_measure_motion_on_a_host_array_a_device_tensor_and_a_view():
    import torch
    from coupe.dvsg_amd import shake
    clip, (want_rows, want_blocks) = clip_small()
    assert want_rows[:, 3].all() and (want_rows[:, 4] < want_rows[:, 2]).any() and (want_rows[:, 4] >= 3).all()
    kw = dict(radius=4, min_blocks=2, gate=5, blocks=True)
    for luma in (clip, torch.from_numpy(clip).cuda()):
        track = shake.measure_motion(luma, **kw)
        assert track.factor == 1 and track.size == (56, 88) and track.grid == (2, 4)
        assert track.rows.dtype == track.blocks.dtype == np.int64 and track.rows.shape == (5, 13)
        assert track.rows.tolist() == want_rows.tolist() and track.blocks.tolist() == want_blocks.tolist()
    assert shake.measure_motion(clip, radius=4, min_blocks=2, gate=5).blocks is None
    old = shake.measure(clip, radius=4, min_blocks=2, blocks=True)
    assert track.rows[:, :4].tolist() == old.vectors.tolist() and track.blocks.tolist() == old.blocks.tolist()
    default = shake.measure_motion(clip, radius=4, min_blocks=2)             # gate 64
    assert default.rows.tolist() == ref.measure(clip, 1, 4, 7, 11, 256, 2, 64)[0].tolist()
    # the Y rows of an NV12 batch where they lie, and a (tensor, pitch, frame_stride) view of the same surfaces
    nv12 = torch.full((6, 84, 88), POISON, dtype=torch.uint8)
    nv12[:, :56] = torch.from_numpy(clip)
    nv12 = nv12.cuda()
    assert shake.measure_motion(shake.luma_of(nv12, "nv12"), **kw).rows.tolist() == want_rows.tolist()
    view = (torch.as_strided(nv12, (6, 56, 88), (84 * 88, 88, 1)), 88, 84 * 88)
    assert shake.measure_motion(view, **kw).rows.tolist() == want_rows.tolist()
    assert shake.motion_summary(track, 2) == ref.summary(want_rows, 1, 2)
    with pytest.raises(shake._lib.DvsgError, match="gate=-1"):
        shake.measure_motion(clip, radius=4, min_blocks=2, gate=-1)


@pytest.mark.parametrize("chunk", [2, 3])
def test_chunking_changes_no_row(chunk):
    from coupe.dvsg_amd import shake
    clip, (want_rows, want_blocks) = clip_small()
    track = shake.measure_motion(clip, radius=4, min_blocks=2, gate=5, blocks=True, chunk=chunk)
    assert track.rows.tolist() == want_rows.tolist() and track.blocks.tolist() == want_blocks.tolist()


# ---- end to end: the 9-frame clip of tests/test_gpu_shake.py's end-to-end test, restated ---------------------------

OPTIONS = ["--radius", "4", "--texture", "16", "--min-blocks", "1"]


def stabilised():
    """(input NV12 [9, 96, 96], output NV12): 9 synthetic frames of 64 x 96 through the seeded synthetic 9-channel checkpoint
    at model size 38 x 54 with skip_length (0, 2, 3), stabilize_clips(frame_format="nv12"), float32"""
    import nv12_ref
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import stabilize_clips
    from coupe.dvsg_amd.weights import make_synthetic_weights
    from coupe.dvsg_amd.y4m import default_yuv_matrix
    if "stabilised" not in _CACHE:
        skip = (0, 2, 3)
        before = nv12_ref.smooth_batch(700, 9, 64, 96).buf
        net = StabNet(38, 54).load_weights(make_synthetic_weights(seed=0, c_in=3 * len(skip)))
        net.get_evaluation_model(len(skip))
        net.precision = "f32"
        after = stabilize_clips(net, [before], frame_format="nv12", skip_length=skip, yuv_matrix=default_yuv_matrix(64))[0]
        _CACHE["stabilised"] = before, np.asarray(after)
    return _CACHE["stabilised"]


def reference_rows(nv12, gate):
    f, my, mx = shake_ref.default_geometry(64, 96, radius=4)
    assert (f, my, mx) == (1, 8, 12)
    return ref.measure(np.ascontiguousarray(nv12[:, :64]), f, 4, my, mx, 16, 1, gate)[0]


def write_y4m(tmp_path, clips):
    import torch
    from coupe.dvsg_amd import y4m
    paths = []
    for name, clip in clips:
        i420 = y4m.nv12_to_i420(torch.from_numpy(clip)).numpy()
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            w = y4m.Y4MWriter(f, 96, 64, (25, 1))
            for frame in i420:
                w.write(frame)
            w.flush()
    return paths


def run_cli(*argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.shake"] + list(argv), capture_output=True, text=True, env=env,
                          cwd=ROOT, timeout=300)


def test_the_command_line_with_motion(tmp_path):
    """--motion --json equals the reference's summaries -- equality, not the ratio: an untrained network steadies nothing --
    and everything the command printed without --motion is still there, unchanged."""
    before, after = stabilised()
    assert before.shape == after.shape == (9, 96, 96)
    paths = write_y4m(tmp_path, (("before.y4m", before), ("after.y4m", after)))
    rows = [reference_rows(before, 64), reference_rows(after, 64)]
    want = ref.compare(rows[0], rows[1], 1, 1)
    print("before %s\nafter  %s" % (want["a"], want["b"]))
    assert want["a"]["pairs"] == 8 and want["a"]["unfit"] < 8 and want["a"]["wobble_rms"] is not None
    out = run_cli("--motion", "--json", *(OPTIONS + paths))
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert got["motion_a"] == want["a"] and got["motion_b"] == want["b"]
    assert got["roll_jitter_ratio"] == want["roll_jitter_ratio"] and got["wobble_ratio"] == want["wobble_ratio"]
    old = [shake_ref.summary(r[:, :4], 1, 96) for r in rows]
    ja, jb = old[0]["jitter_rms"], old[1]["jitter_rms"]
    assert got["a"] == old[0] and got["b"] == old[1] and got["files"] == paths and got["factor"] == 1
    assert got["jitter_ratio"] == (jb / ja if ja and jb is not None else None)
    assert sorted(got) == sorted(["a", "b", "jitter_ratio", "files", "factor", "motion_a", "motion_b", "roll_jitter_ratio",
                                  "wobble_ratio"])


def motion_line(path, s):
    fmt = lambda v, unit: "n/a" if v is None else "%.4f %s" % (v, unit)
    return "%s: roll %s, roll jitter %s, zoom jitter %s, wobble %s, %d unfit" % (
        path, fmt(s["roll_rms_deg"], "deg/frame"), fmt(s["roll_jitter_deg"], "deg/frame"), fmt(s["zoom_jitter_pct"], "%/frame"),
        fmt(s["wobble_rms"], "px"), s["unfit"])


def test_the_text_output_with_and_without_motion(tmp_path, capsys):
    """In this process (the front end's `main`): with --motion one more line per clip and two more ratios, with another gate
    other figures, and without it the lines it printed before."""
    from coupe.dvsg_amd import shake
    before, after = stabilised()
    paths = write_y4m(tmp_path, (("before.y4m", before), ("after.y4m", after)))
    want = ref.compare(reference_rows(before, 64), reference_rows(after, 64), 1, 1)
    assert shake.main(OPTIONS + paths) == 0
    plain = capsys.readouterr().out.splitlines()
    assert len(plain) == 3 and plain[0].startswith(paths[0] + ": 9 frames 96x64, 8 pairs") and plain[2].startswith("jitter ratio B / A:")
    assert shake.main(["--motion"] + OPTIONS + paths) == 0
    lines = capsys.readouterr().out.splitlines()
    ratio = lambda v: "n/a" if v is None else "%.3f" % v
    assert lines == [plain[0], motion_line(paths[0], want["a"]), plain[1], motion_line(paths[1], want["b"]), plain[2],
                     "roll jitter ratio B / A: " + ratio(want["roll_jitter_ratio"]), "wobble ratio B / A: " + ratio(want["wobble_ratio"])]
    narrow = ref.summary(reference_rows(before, 24), 1, 1)
    assert narrow != want["a"] and narrow["unfit"] < 8, "a gate of 24 changes nothing: the option is not tested"
    assert shake.main(["--motion", "--gate", "24"] + OPTIONS + paths[:1]) == 0
    assert capsys.readouterr().out.splitlines() == [plain[0], motion_line(paths[0], narrow)]
    assert shake.main(["--json"] + OPTIONS + paths[:1]) == 0
    assert sorted(json.loads(capsys.readouterr().out)) == ["a", "factor", "files"]
