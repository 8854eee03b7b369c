"""GPU: dvsg_shake_measure_u8 and coupe.dvsg_amd.shake against the NumPy restatement tests/shake_ref.py, bit for bit: every
row of vectors_host and every block of blocks_host, nothing left out -- the rule is integer arithmetic, so there is no
tolerance.  tests/test_shake_cpu.py checks that the reference is meaningful (shifts come back, flat and striped content
drops out); here every textured case asserts on the reference that some block is valid, and the flat and striped cases
that none is, so no comparison is of zeros against zeros by accident.

Shapes (reduced size, radius, margins, factor): one block with the smallest window; one block with the largest; rows at a pitch
of W + 5 from an odd address with a frame stride beyond the frame and poison between; a factor that divides neither side
with a 5-frame clip; the default geometry of 1080p."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shake_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xAB
# name -> H, W, factor, radius, margin_y, margin_x, min_blocks, layout (pitch - W, frame_stride - H pitch, offset of the base)
SHAPES = {
    "one_block_r1": (18, 18, 1, 1, 1, 1, 1, (0, 0, 0)),
    "one_block_r16": (48, 50, 1, 16, 16, 16, 1, (0, 0, 0)),
    "pitched_41x67": (41, 67, 1, 3, 3, 5, 2, (5, 37, 3)),
    "factor3_125x203": (125, 203, 3, 5, 5, 6, 1, (0, 0, 0)),
    "default_1080p": (1080, 1920, 4, 12, 34, 60, 8, (0, 0, 0)),
}
KINDS = ("shift_int", "shift_sub", "noise", "flat", "stripes", "checker", "boundary", "extremes")
TEXTURED = ("shift_int", "shift_sub", "checker")
_CACHE = {}


def big_texture(shape):
    """The shape's texture with room for shifts of up to (radius + 1) factor source pixels on every side."""
    H, W, f, R = SHAPES[shape][:4]
    pad = (R + 1) * f
    if ("big", shape) not in _CACHE:
        _CACHE["big", shape] = shake_ref.texture(100 + len(shape), H + 2 * pad, W + 2 * pad, box=5 if f == 1 else 17)
    return _CACHE["big", shape], pad


def planes_of(shape, kind):
    """uint8 [n, H, W]; frame 0 is the previous plane of frame 1"""
    H, W, f, R = SHAPES[shape][:4]
    big, pad = big_texture(shape)
    at = lambda oy, ox: shake_ref.shifted(big, oy, ox, H, W, pad)
    inside = min(R - 1, 2)                         # an integer shift inside the radius, in reduced pixels (0 for R = 1)
    if kind == "shift_int":
        return np.stack([at(0, 0), at(inside * f, -min(R - 1, 3) * f)])
    if kind == "shift_sub":
        return np.stack([at(0, 0), shake_ref.shifted_subpel(big, (inside - 0.75) * f if inside else 0.25 * f, 0.375 * f, H, W, pad)])
    if kind == "clip5":                            # integer and sub-pixel shifts in turn, each against the frame before it
        offs = [(0, 0), (f, -2 * f), (1.5 * f, -2.25 * f), (-f, 0), (-0.5 * f, 3.125 * f)]
        return np.stack([shake_ref.shifted_subpel(big, oy, ox, H, W, pad) for oy, ox in offs])
    if kind == "noise":
        rng = np.random.RandomState(7)
        return rng.randint(0, 256, size=(2, H, W)).astype(np.uint8)
    if kind == "flat":
        return np.full((2, H, W), 117, dtype=np.uint8)
    if kind == "stripes":
        s = shake_ref.stripes(H, W + f, period=8 * f)
        return np.stack([s[:, f:], s[:, :W]])
    if kind == "checker":                          # 2-pixel squares on the reduced plane, shifted by their period
        c = shake_ref.checkerboard(H + 4 * f, W + 4 * f, cell=2 * f)
        return np.stack([c[:H, :W], c[4 * f:, 4 * f:]]) if R >= 4 else np.stack([c[:H, :W], c[:H, :W]])
    if kind == "boundary":                         # the minimum on the search boundary: a shift by the radius
        return np.stack([at(0, 0), at(0, R * f)])
    if kind == "extremes":                         # every SAD is 65280
        return np.stack([np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)])
    raise KeyError(kind)


def call(planes, f, R, my, mx, texture, min_blocks, layout=(0, 0, 0), workspace_short=0):
    """dvsg_shake_measure_u8 on the planes laid out at the given pitch, frame stride and base offset, poison everywhere else.
    Returns (status, vectors int32 [n - 1, 4], blocks int32 [n - 1, n_blk, 3]); both arrays start as -7."""
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
    _lib.call("dvsg_shake_workspace_bytes", n, H, W, f, R, my, mx, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    ny, nx = shake_ref.block_counts(H // f, W // f, my, mx)
    vectors = np.full((n - 1, 4), -7, dtype=np.int32)
    blocks = np.full((n - 1, ny * nx, 3), -7, dtype=np.int32)
    rc = lib.dvsg_shake_measure_u8(dev.data_ptr() + layout[2], pitch, frame_stride, n, H, W, f, R, my, mx, texture, min_blocks,
                                   vectors.ctypes.data, blocks.ctypes.data, ws.data_ptr(), need.value - workspace_short)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host), "the call wrote to its input"
    return rc, vectors, blocks


def check(shape, kind, texture=256):
    H, W, f, R, my, mx, min_blocks, layout = SHAPES[shape]
    planes = planes_of(shape, kind)
    want_v, want_b = shake_ref.measure(planes, f, R, my, mx, texture, min_blocks)
    valid = want_b[:, :, 2].sum(axis=1)
    print("%s %s: %d block(s), valid per pair %s, vectors %s" % (shape, kind, want_b.shape[1], valid.tolist(), want_v.tolist()))
    if kind in TEXTURED or kind == "clip5":
        assert (valid >= 1).all(), "the reference finds no valid block in a textured case"
    if kind in ("flat", "stripes", "boundary", "extremes"):
        assert not valid.any() and not want_b.any() and not want_v.any()
    rc, got_v, got_b = call(planes, f, R, my, mx, texture, min_blocks, layout)
    assert rc == 0
    assert got_b.shape == want_b.shape and got_b.dtype == want_b.dtype == np.int32
    bad = np.argwhere((got_b != want_b).any(axis=2))
    assert len(bad) == 0, "%d block(s) differ, first (pair, block) %s: got %s, want %s" % (
        len(bad), bad[0].tolist(), got_b[tuple(bad[0])].tolist(), want_b[tuple(bad[0])].tolist())
    assert got_v.tolist() == want_v.tolist()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_row_and_block_equals_the_reference(shape, kind):
    check(shape, kind)


def test_a_five_frame_clip_with_a_factor_that_divides_neither_side():
    check("factor3_125x203", "clip5")


@pytest.mark.parametrize("texture", [0, 1, 4000])
def test_the_texture_threshold(texture):
    """0 and 1 are the same threshold (max(texture, 1)); 4000 drops four of the six noise blocks and keeps two."""
    check("pitched_41x67", "noise", texture=texture)
    check("pitched_41x67", "checker", texture=texture)


def clip_small():
    """6 frames of 56 x 88: a texture that wanders by integer and sub-pixel steps"""
    if "clip" not in _CACHE:
        big = shake_ref.texture(31, 56 + 16, 88 + 16)
        offs = [(0, 0), (1, -2), (1.5, -1.25), (0, 0.5), (-2, 2), (-2.25, 3)]
        _CACHE["clip"] = np.stack([shake_ref.shifted_subpel(big, oy, ox, 56, 88, 8) for oy, ox in offs])
        _CACHE["clip_ref"] = shake_ref.measure(_CACHE["clip"], 1, 4, 7, 11, 256, 2)
    return _CACHE["clip"], _CACHE["clip_ref"]


def test_measure_on_a_host_array_and_on_a_device_tensor():
    import torch
    from coupe.dvsg_amd import shake
    clip, (want_v, want_b) = clip_small()
    assert shake_ref.default_geometry(56, 88, radius=4) == (1, 7, 11) and want_v[:, 3].all()
    kw = dict(radius=4, min_blocks=2, blocks=True)
    host = shake.measure(clip, **kw)
    dev = shake.measure(torch.from_numpy(clip).cuda(), **kw)
    for track in (host, dev):
        assert track.factor == 1 and track.size == (56, 88)
        assert track.vectors.dtype == track.blocks.dtype == np.int64
        assert track.vectors.tolist() == want_v.tolist() and track.blocks.tolist() == want_b.tolist()
    assert shake.measure(clip, radius=4, min_blocks=2).blocks is None
    # the Y rows of an NV12 batch where they lie, and a (tensor, pitch, frame_stride) view of the same surfaces
    nv12 = torch.full((6, 84, 88), POISON, dtype=torch.uint8)
    nv12[:, :56] = torch.from_numpy(clip)
    nv12 = nv12.cuda()
    y = shake.luma_of(nv12, "nv12")
    assert y.data_ptr() == nv12.data_ptr() and not y.is_contiguous()
    assert shake.measure(y, **kw).blocks.tolist() == want_b.tolist()
    view = (torch.as_strided(nv12, (6, 56, 88), (84 * 88, 88, 1)), 88, 84 * 88)
    assert shake.measure(view, **kw).vectors.tolist() == want_v.tolist()
    with pytest.raises(ValueError, match="frame_stride"):
        shake.measure((view[0], 88, 84 * 88 + 1000), **kw)      # the last plane would end outside the tensor


@pytest.mark.parametrize("chunk", [2, 3])
def test_chunking_changes_no_row(chunk):
    from coupe.dvsg_amd import shake
    clip, (want_v, want_b) = clip_small()
    track = shake.measure(clip, radius=4, min_blocks=2, blocks=True, chunk=chunk)
    assert track.vectors.tolist() == want_v.tolist() and track.blocks.tolist() == want_b.tolist()


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    from coupe.dvsg_amd import _lib
    clip, _ = clip_small()
    rc, vectors, blocks = call(clip, 1, 4, 7, 11, 256, 2, workspace_short=1)
    assert rc == -3 and "dvsg_shake_workspace_bytes" in _lib.load().dvsg_last_error_string().decode()
    assert (vectors == -7).all() and (blocks == -7).all()
    rc, vectors, blocks = call(clip, 1, 4, 7, 11, 256, 2)
    assert rc == 0 and (vectors != -7).any() and (blocks != -7).all()


# ---- end to end: the 9-frame clip and model of tests/test_gpu_pipe.py, stabilised as NV12 -------------------------

MEASURE_KW = dict(radius=4, texture=16, min_blocks=1)


def stabilised():
    """(input NV12 [9, 96, 96], output NV12) of stabilize_clips(frame_format="nv12") on test_gpu_pipe's clip and model"""
    import test_gpu_pipe as pipe
    return pipe.clips()["single"], pipe.reference("single")[0]


def reference_summary(nv12):
    f, my, mx = shake_ref.default_geometry(64, 96, radius=MEASURE_KW["radius"])
    vectors, _ = shake_ref.measure(np.ascontiguousarray(nv12[:, :64]), f, MEASURE_KW["radius"], my, mx, MEASURE_KW["texture"],
                                   MEASURE_KW["min_blocks"])
    return shake_ref.summary(vectors, f, 96)


def test_summary_of_a_stabilised_clip_equals_the_reference():
    import torch
    from coupe.dvsg_amd import shake
    before, after = stabilised()
    assert before.shape == after.shape == (9, 96, 96)
    tracks = [shake.measure(shake.luma_of(torch.from_numpy(c).cuda(), "nv12"), **MEASURE_KW) for c in (before, after)]
    want = [reference_summary(before), reference_summary(after)]
    print("before %s\nafter  %s" % tuple(want))
    assert [shake.summary(t) for t in tracks] == want
    assert want[0]["pairs"] == 8 and want[0]["lost"] < 8      # the input's motion is measured, not lost
    result = shake.compare(*tracks)
    ja, jb = want[0]["jitter_rms"], want[1]["jitter_rms"]
    assert result["a"] == want[0] and result["b"] == want[1]
    assert result["jitter_ratio"] == (jb / ja if ja and jb is not None else None)


def test_the_command_line_prints_the_same_numbers(tmp_path):
    import torch
    from coupe.dvsg_amd import y4m
    before, after = stabilised()
    paths = []
    for name, clip in (("before.y4m", before), ("after.y4m", after)):
        i420 = y4m.nv12_to_i420(torch.from_numpy(clip)).numpy()
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            w = y4m.Y4MWriter(f, 96, 64, (25, 1))
            for frame in i420:
                w.write(frame)
            w.flush()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    options = ["--radius", "4", "--texture", "16", "--min-blocks", "1"]
    out = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.shake", "--json"] + options + paths, capture_output=True,
                         text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    want = [reference_summary(before), reference_summary(after)]
    assert got["a"] == want[0] and got["b"] == want[1] and got["files"] == paths and got["factor"] == 1
    ja, jb = want[0]["jitter_rms"], want[1]["jitter_rms"]
    assert got["jitter_ratio"] == (jb / ja if ja and jb is not None else None)
    text = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.shake"] + options + paths, capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=300)
    assert text.returncode == 0, text.stderr[-2000:]
    lines = text.stdout.splitlines()
    assert len(lines) == 3 and lines[0].startswith(paths[0] + ": 9 frames 96x64, 8 pairs") and lines[2].startswith("jitter ratio B / A:")
