"""GPU: pipe.stabilize_pipes and the front end against `stabilize_clips(frame_format="nv12")` on the NV12 form of the same
frames, byte for byte -- nothing in the pipeline is arithmetic, so there are no tolerances.  Model 38 x 54 (test_gpu_nv12.py's),
sources 64 x 96 and 20 x 32, a 9-channel synthetic checkpoint with skip_length (0, 2, 3): the ring of 5 frames wraps at the
fourth frame, so a 9-frame clip runs in the steady state."""
import io
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import nv12_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = (38, 54)
SKIP = (0, 2, 3)
BIG, SMALL = (64, 96), (20, 32)      # (H0, W0)
JOIN = 60.0
HEADER = "YUV4MPEG2 W96 H64 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED"

_CACHE = {}


def model():
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if "model" not in _CACHE:
        m = StabNet(*MODEL).load_weights(make_synthetic_weights(seed=0, c_in=3 * len(SKIP)))
        m.get_evaluation_model(len(SKIP))
        m.precision = "f32"
        _CACHE["model"] = m
    return _CACHE["model"]


def with_cut(nv12, at):
    """The dark scene 0.05 + 0.4 x before frame `at` and the bright scene 0.55 + 0.4 x from it on, x the clip's own luma in
    [0, 1] (examples/stabilize_stream.py's construction)."""
    H0 = 2 * nv12.shape[1] // 3
    out = nv12.copy()
    x = (nv12[:, :H0].astype(np.float64) - 16) / 219
    for k in range(len(nv12)):
        out[k, :H0] = (16 + ((0.05 if k < at else 0.55) + 0.4 * x[k]) * 219).astype(np.uint8)
    return out


def clips():
    """NV12 clips [N, 3 H0 / 2, W0] and their I420 form: 0 is the single clip, 0 (with a cut at frame 5), 1, 2 the three."""
    import torch
    from coupe.dvsg_amd import y4m
    if "clips" not in _CACHE:
        nv12 = [nv12_ref.smooth_batch(700, 9, *BIG).buf, nv12_ref.smooth_batch(701, 5, *SMALL).buf,
                nv12_ref.smooth_batch(702, 6, *BIG).buf]
        three = [with_cut(nv12[0], 5), nv12[1], nv12[2]]
        i420 = lambda c: y4m.nv12_to_i420(torch.from_numpy(c)).numpy()
        _CACHE["clips"] = dict(single=nv12[0], single_i420=i420(nv12[0]), three=three, three_i420=[i420(c) for c in three])
    return _CACHE["clips"]


THREE_KW = dict(crop="auto", scene_cut=0.75)


def reference(which):
    """stabilize_clips on the NV12 clips, once: the matrix is the one `yuv_matrix="auto"` resolves to for 64 rows."""
    from coupe.dvsg_amd.online import stabilize_clips
    from coupe.dvsg_amd.y4m import default_yuv_matrix
    if which not in _CACHE:
        matrix = default_yuv_matrix(BIG[0])
        assert matrix == "bt601"
        if which == "single":
            _CACHE[which] = stabilize_clips(model(), [clips()["single"]], frame_format="nv12", skip_length=SKIP, yuv_matrix=matrix)
        else:
            _CACHE[which] = stabilize_clips(model(), clips()["three"], frame_format="nv12", batch=2, skip_length=SKIP,
                                            yuv_matrix=matrix, **THREE_KW)
    return _CACHE[which]


def y4m_bytes(i420, header=None):
    H0, W0 = 2 * i420.shape[1] // 3, i420.shape[2]
    header = header or "YUV4MPEG2 W%d H%d F25:1 Ip C420jpeg" % (W0, H0)
    return header.encode() + b"\n" + b"".join(b"FRAME\n" + f.tobytes() for f in i420)


def run(sources, sinks, **kw):
    """stabilize_pipes on a thread with a bounded join: a deadlock fails the test instead of sitting out the suite's limit."""
    from coupe.dvsg_amd.pipe import stabilize_pipes
    box = {}

    def target():
        try:
            import torch
            torch.cuda.set_device(0)
            box["stats"] = stabilize_pipes(model(), sources, sinks, skip_length=SKIP, **kw)
        except BaseException as e:
            box["error"] = e
    model()                              # built on the test's own thread
    t = threading.Thread(target=target, name="test-caller")
    t.start()
    t.join(JOIN)
    assert not t.is_alive(), "stabilize_pipes did not return within %g s" % JOIN
    if "error" in box:
        raise box["error"]
    assert [t.name for t in threading.enumerate() if t.name.startswith("stabilize_pipes")] == []
    return box["stats"]


def nv12_frames_of_y4m(data):
    """The frames of a Y4M stream as NV12 [N, 3 H0 / 2, W0] (converted on the host), and its reader."""
    import torch
    from coupe.dvsg_amd import y4m
    r = y4m.Y4MReader(io.BytesIO(data))
    frames = list(r)
    return y4m.i420_to_nv12(torch.from_numpy(np.stack(frames))).numpy() if frames else np.empty((0,) + r.frame_shape, np.uint8), r


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s against %s" % (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), "%s: %d bytes differ, first in frame %d" % (
        what, int((got != want).sum()), int(np.argwhere((got != want).reshape(len(got), -1).any(axis=1))[0, 0]))


def run_three(depth):
    from coupe.dvsg_amd import y4m
    outs = [io.BytesIO() for _ in range(3)]
    sources = [y4m.Y4MReader(io.BytesIO(y4m_bytes(c))) for c in clips()["three_i420"]]
    sinks = [y4m.Y4MWriter(o, s.width, s.height, s.fps) for o, s in zip(outs, sources)]
    stats = run(sources, sinks, batch=2, depth=depth, **THREE_KW)
    return [o.getvalue() for o in outs], stats


@pytest.mark.gpu
def test_one_y4m_source_is_stabilize_clips():
    from coupe.dvsg_amd import y4m
    out = io.BytesIO()
    src = y4m.Y4MReader(io.BytesIO(y4m_bytes(clips()["single_i420"])))
    stats = run([src], [y4m.Y4MWriter(out, src.width, src.height, src.fps)])
    got, r = nv12_frames_of_y4m(out.getvalue())
    assert (r.width, r.height) == (96, 64)
    want = reference("single")[0]
    same(got, want, "the one source")
    assert stats[0]["frames"] == 9 and 1 <= stats[0]["high_water"] <= 3 and stats[0]["zoom"] is None and stats[0]["cuts"] is None
    assert not np.array_equal(want, clips()["single"]), "the reference must have moved the frames"


@pytest.mark.gpu
def test_three_sources_two_rings_crop_and_a_cut():
    """Ring hand-over (source 2 takes source 1's ring after five steps), two sizes in one step, the zoom ratchet and a detected
    cut, through the pipeline: every sink is stabilize_clips' result for its clip."""
    data, stats = _CACHE.get("three@3") or _CACHE.setdefault("three@3", run_three(3))
    want = reference("three")
    for i in range(3):
        got, _ = nv12_frames_of_y4m(data[i])
        same(got, want[i], "source %d" % i)
    assert [s["frames"] for s in stats] == [9, 5, 6]
    assert [s["cuts"] for s in stats] == [1, 0, 0], stats
    assert all(0.5 <= s["zoom"] <= 1.0 for s in stats), stats


@pytest.mark.gpu
def test_depth_1_and_depth_3_give_the_same_bytes():
    deep, _ = _CACHE.get("three@3") or _CACHE.setdefault("three@3", run_three(3))
    serial, stats = run_three(1)
    assert serial == deep
    assert all(s["high_water"] == 1 for s in stats)


@pytest.mark.gpu
def test_raw_nv12_in_and_out(monkeypatch):
    """The raw NV12 path gives the Y4M path's frames, and never calls the repack."""
    from coupe.dvsg_amd import pipe, y4m

    def no_repack(*a, **k):
        raise AssertionError("the raw NV12 path must not repack")
    monkeypatch.setattr(pipe.y4m, "i420_to_nv12", no_repack)
    monkeypatch.setattr(pipe.y4m, "nv12_to_i420", no_repack)
    out = io.BytesIO()
    clip = clips()["single"]
    src = y4m.RawNV12Reader(io.BytesIO(clip.tobytes()), BIG[1], BIG[0])
    stats = run([src], [y4m.RawNV12Writer(out, BIG[1], BIG[0])])
    monkeypatch.undo()
    got = np.frombuffer(out.getvalue(), np.uint8).reshape(clip.shape)
    same(got, reference("single")[0], "raw NV12")
    assert stats[0]["frames"] == 9


@pytest.mark.gpu
def test_the_front_end_on_files(tmp_path):
    """python -m coupe.dvsg_amd.pipe, one fresh child process: exit 0, the output parses, carries the input's tags, and holds
    the frames of the one-source case."""
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(y4m_bytes(clips()["single_i420"], HEADER))
    want = reference("single")[0]
    out = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--synthetic-weights", "--model-size", "54x38",
                          "--skip-length", "0,2,3", "--input", str(src), "--output", str(dst), "--stats"],
                         cwd=ROOT, capture_output=True, timeout=120)
    err = out.stderr.decode()
    assert out.returncode == 0, err[-3000:]
    assert out.stdout == b"" and "synthetic" in err and "9 frames" in err, err
    data = dst.read_bytes()
    head = data[:data.index(b"\n")].decode().split(" ")
    assert head[0] == "YUV4MPEG2" and set(HEADER.split(" ")[1:]) <= set(head[1:]), head
    got, r = nv12_frames_of_y4m(data)
    assert r.tags == ("XYSCSS=420MPEG2", "XCOLORRANGE=LIMITED") and r.colorspace == "420mpeg2"
    assert tuple(r.fps) == (30000, 1001) and tuple(r.aspect) == (1, 1)
    same(got, want, "the front end")
