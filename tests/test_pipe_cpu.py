"""CPU: the mechanics of pipe.stabilize_pipes with the stabiliser replaced by a stand-in that returns its input (the
private `_step_fn`): order, schedule, back-pressure, failure without hangs or stray threads; and the front end's argument
errors.  What the real step computes is tests/test_gpu_pipe.py's."""
import io
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from coupe.dvsg_amd import y4m
from coupe.dvsg_amd.pipe import stabilize_pipes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN = 30.0


def frames_of(seed, n, W, H):
    return np.random.default_rng(seed).integers(0, 256, (n, 3 * H // 2, W), dtype=np.uint8)


def y4m_bytes(frames, W, H):
    return b"YUV4MPEG2 W%d H%d F25:1 Ip C420jpeg\n" % (W, H) + b"".join(b"FRAME\n" + f.tobytes() for f in frames)


def y4m_pair(frames, W, H):
    out = io.BytesIO()
    return y4m.Y4MReader(io.BytesIO(y4m_bytes(frames, W, H))), y4m.Y4MWriter(out, W, H, (25, 1)), out


def payloads(out, W, H):
    return [f.tobytes() for f in y4m.Y4MReader(io.BytesIO(out.getvalue()))]


def identity(frames):
    return dict(frames)


def call(*args, **kw):
    """stabilize_pipes on a thread of its own with a bounded join: (result, exception).  A deadlock fails the test."""
    box = {}

    def target():
        try:
            box["result"] = stabilize_pipes(*args, **kw)
        except BaseException as e:
            box["error"] = e
    t = threading.Thread(target=target, name="test-caller")
    t.start()
    t.join(JOIN)
    assert not t.is_alive(), "stabilize_pipes did not return within %g s" % JOIN
    return box.get("result"), box.get("error")


def loop_threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("stabilize_pipes")]


def test_order_and_schedule_for_three_sources_of_different_length():
    """Lengths 9, 5 and 1 with batch=2: every sink gets its own source's frames in order, and the steps' batches are those of
    stabilize_clips' schedule -- 0 and 1 together for five steps, then 2 takes 1's place for one step, then 0 alone."""
    sizes = [(16, 12), (8, 4), (16, 12)]
    clips = [frames_of(10 + i, n, W, H) for i, (n, (W, H)) in enumerate(zip((9, 5, 1), sizes))]
    ends = [y4m_pair(c, W, H) for c, (W, H) in zip(clips, sizes)]
    steps = []

    def step(frames):
        steps.append([tuple(t.shape) for t in frames.values()])
        assert all(t.dtype.is_floating_point is False and t.dim() == 2 for t in frames.values())
        return dict(frames)
    stats, err = call(None, [e[0] for e in ends], [e[1] for e in ends], batch=2, depth=3, _step_fn=step)
    assert err is None
    big, small = (18, 16), (6, 8)
    assert steps == [[big, small]] * 5 + [[big, big]] + [[big]] * 3
    for (W, H), clip, (_, _, out), st in zip(sizes, clips, ends, stats):
        assert payloads(out, W, H) == [f.tobytes() for f in clip]
        assert st["frames"] == len(clip) and 1 <= st["high_water"] <= 3
    assert loop_threads() == []


def test_the_step_sees_nv12_and_every_layout_pair_round_trips():
    """A Y4M source reaches the step as NV12 (the index formula of test_y4m_cpu.py, here through y4m itself on the host);
    Y4M -> raw NV12, raw NV12 -> Y4M and raw -> raw sinks receive the matching bytes."""
    import torch
    W, H = 12, 8
    i420 = frames_of(20, 4, W, H)
    nv12 = y4m.i420_to_nv12(torch.from_numpy(i420)).numpy()
    seen = []

    def step(frames):
        seen.extend(t.cpu().numpy().copy() for t in frames.values())
        return dict(frames)
    outs = [io.BytesIO() for _ in range(3)]
    sources = [y4m.Y4MReader(io.BytesIO(y4m_bytes(i420, W, H))), y4m.RawNV12Reader(io.BytesIO(nv12.tobytes()), W, H),
               y4m.RawNV12Reader(io.BytesIO(nv12.tobytes()), W, H)]
    sinks = [y4m.RawNV12Writer(outs[0], W, H), y4m.Y4MWriter(outs[1], W, H, 25), y4m.RawNV12Writer(outs[2], W, H)]
    stats, err = call(None, sources, sinks, batch=1, depth=2, _step_fn=step)
    assert err is None and [s["frames"] for s in stats] == [4, 4, 4]
    assert len(seen) == 12 and all(np.array_equal(s, nv12[k % 4]) for k, s in enumerate(seen))
    assert outs[0].getvalue() == nv12.tobytes() and outs[2].getvalue() == nv12.tobytes()
    assert payloads(outs[1], W, H) == [f.tobytes() for f in i420]


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_a_slow_sink_stalls_its_reader(depth):
    """Back-pressure: with a sink that sleeps per frame, the frames between readinto and write never exceed depth -- counted
    here at the source and the sink, and by the loop's own high-water mark."""
    W, H, n = 8, 4, 10
    clip = frames_of(30, n, W, H)
    src, snk, out = y4m_pair(clip, W, H)
    lock = threading.Lock()
    count = dict(read=0, written=0, worst=0)

    class Source(object):
        width, height, frame_shape, layout = W, H, src.frame_shape, "i420"

        def readinto(self, buf):
            ok = src.readinto(buf)
            with lock:
                count["read"] += bool(ok)
                count["worst"] = max(count["worst"], count["read"] - count["written"])
            return ok

    class Sink(object):
        layout = "i420"

        def write(self, frame):
            time.sleep(0.01)
            snk.write(frame)
            with lock:
                count["written"] += 1
    stats, err = call(None, [Source()], [Sink()], depth=depth, _step_fn=identity)
    assert err is None and stats[0]["frames"] == n
    assert count["worst"] <= depth and stats[0]["high_water"] == depth, (count, stats)
    assert payloads(out, W, H) == [f.tobytes() for f in clip]


def test_depth_must_be_positive_and_ends_must_pair_up():
    src, snk, _ = y4m_pair(frames_of(31, 1, 8, 4), 8, 4)
    with pytest.raises(ValueError, match="depth"):
        stabilize_pipes(None, [src], [snk], depth=0, _step_fn=identity)
    with pytest.raises(ValueError, match="one sink per source"):
        stabilize_pipes(None, [src], [], _step_fn=identity)
    with pytest.raises(ValueError, match="16 x 12"):
        stabilize_pipes(None, [src], [y4m.Y4MWriter(io.BytesIO(), 16, 12, 25)], _step_fn=identity)
    assert stabilize_pipes(None, [], [], _step_fn=identity) == []
    assert loop_threads() == []


def test_a_source_without_frames():
    """An empty stream between two others: it gets its header and no frames, and holds nobody up."""
    W, H = 8, 4
    clips = [frames_of(40, 3, W, H), frames_of(41, 0, W, H), frames_of(42, 2, W, H)]
    ends = [y4m_pair(c, W, H) for c in clips]
    stats, err = call(None, [e[0] for e in ends], [e[1] for e in ends], batch=1, depth=2, _step_fn=identity)
    assert err is None and [s["frames"] for s in stats] == [3, 0, 2]
    for clip, (_, _, out) in zip(clips, ends):
        assert payloads(out, W, H) == [f.tobytes() for f in clip]


class Boom(Exception):
    pass


@pytest.mark.parametrize("depth", [1, 3])
def test_a_reader_that_raises_ends_the_call(depth):
    W, H = 8, 4
    clips = [frames_of(50, 9, W, H), frames_of(51, 9, W, H)]
    ends = [y4m_pair(c, W, H) for c in clips]
    inner = ends[1][0]

    class Source(object):
        width, height, frame_shape, layout = W, H, inner.frame_shape, "i420"

        def readinto(self, buf):
            if inner.frames_read == 4:
                raise Boom("frame 4")
            return inner.readinto(buf)
    stats, err = call(None, [ends[0][0], Source()], [e[1] for e in ends], depth=depth, _step_fn=identity)
    assert stats is None and isinstance(err, Boom)
    assert loop_threads() == []
    # what was stabilised before the failure has reached the sinks: the four steps both sources took part in
    for clip, (_, _, out) in zip(clips, ends):
        assert payloads(out, W, H) == [f.tobytes() for f in clip[:4]]


@pytest.mark.parametrize("depth", [1, 3])
def test_a_writer_that_raises_ends_the_call(depth):
    W, H = 8, 4
    clips = [frames_of(60, 40, W, H), frames_of(61, 40, W, H)]
    ends = [y4m_pair(c, W, H) for c in clips]

    class Sink(object):
        layout, written = "i420", 0

        def write(self, frame):
            if self.written == 2:
                raise BrokenPipeError(32, "Broken pipe")
            self.written += 1
    stats, err = call(None, [e[0] for e in ends], [ends[0][1], Sink()], depth=depth, _step_fn=identity)
    assert stats is None and isinstance(err, BrokenPipeError)
    assert loop_threads() == []
    got = payloads(ends[0][2], W, H)                       # the other sink holds a prefix of its own stream, in order
    assert got == [f.tobytes() for f in clips[0][:len(got)]]


def test_a_step_that_raises_ends_the_call():
    W, H = 8, 4
    src, snk, out = y4m_pair(frames_of(70, 9, W, H), W, H)
    calls = []

    def step(frames):
        calls.append(1)
        if len(calls) == 3:
            raise Boom("step 2")
        return dict(frames)
    stats, err = call(None, [src], [snk], depth=3, _step_fn=step)
    assert isinstance(err, Boom) and loop_threads() == []
    assert len(payloads(out, W, H)) == 2


@pytest.mark.parametrize("depth", [1, 3])
def test_a_truncated_source_flushes_its_complete_frames_first(depth):
    W, H = 8, 4
    clip = frames_of(80, 6, W, H)
    out = io.BytesIO()
    src = y4m.Y4MReader(io.BytesIO(y4m_bytes(clip, W, H)[:-5]))
    stats, err = call(None, [src], [y4m.Y4MWriter(out, W, H, 25)], depth=depth, _step_fn=identity)
    assert isinstance(err, y4m.Y4MError) and "frame 5" in str(err) and "43 of 48" in str(err)
    assert payloads(out, W, H) == [f.tobytes() for f in clip[:5]]
    assert loop_threads() == []


# ---- the front end: argument errors, checked before any device or stream is touched

def front_end(*args, stdin=b""):
    return subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe"] + list(args), input=stdin, cwd=ROOT,
                          capture_output=True, timeout=120)


@pytest.mark.parametrize("args,word", [
    (["--format", "nv12", "--synthetic-weights"], "--size"),
    (["--synthetic-weights", "--input", "a.y4m", "--input", "b.y4m", "--output", "c.y4m"], "one output per input"),
    (["--input", "a.y4m", "--output", "c.y4m"], "--ckpt"),
    (["--synthetic-weights", "--depth", "0"], "--depth"),
    (["--synthetic-weights", "--model-size", "512"], "--model-size"),
])
def test_argument_errors_are_one_line_and_status_1(args, word):
    out = front_end(*args)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err)
    assert out.stdout == b"" and len(err.strip().splitlines()) == 1 and "Traceback" not in err, err
    assert word in err, err


def test_a_malformed_stream_is_one_line_and_status_1(tmp_path):
    """No device is needed to refuse a stream: its header is read before the weights are loaded."""
    bad = tmp_path / "bad.y4m"
    bad.write_bytes(b"YUV4MPEG2 W64 H96 F25:1 C444\n")
    out = front_end("--synthetic-weights", "--input", str(bad), "--output", str(tmp_path / "out.y4m"))
    err = out.stderr.decode()
    assert out.returncode == 1 and len(err.strip().splitlines()) == 1 and "C444" in err and "Traceback" not in err, err
    out = front_end("--synthetic-weights", "--output", str(tmp_path / "out.y4m"), stdin=b"not video\n")
    err = out.stderr.decode()
    assert out.returncode == 1 and len(err.strip().splitlines()) == 1 and "YUV4MPEG2" in err, err
    assert not (tmp_path / "out.y4m").exists()
