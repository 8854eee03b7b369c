"""CPU: the unbounded model of the online stabiliser (tests/online_model.py) is itself held to something.

* its schedules still contain every case they were written for (`coverage`), so shortening one later cannot lose a case;
* its history rule against a literal transcription of eval.py:93-124's list loop, with integer labels for frames and a
  fake stabilise function whose "result" is the tuple of the window's labels;
* its scene state machine against `scene_ref.scene_step` (the restatement the kernel is pinned to) on random histograms;
* the planted cuts of the float content really are cuts, and nothing else is."""
import numpy as np
import pytest

import online_model as om
import scene_ref

SCHEDULES = ["rgb", "source_res", "nv12", "model_size", "p010"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the schedules keep their cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCHEDULES)
def test_schedule_covers_its_cases(name):
    sched = om.make_schedule(name)
    assert om.make_schedule(name) == sched and om.make_schedule(name).streams == sched.streams, "deterministic"
    f = om.coverage(sched)
    assert 80 <= len(sched) <= 100 and 6 <= len(f["streams"]) <= 8 and f["max_open"] == sched.max_streams == 3
    assert f["longest"] >= 70, "a stream whose ring wraps twice"
    assert f["reuse_after_long"], "a ring reused after a stream of >= 70 frames"
    assert f["reuse_after_one_frame"], "a ring reused after a 1-frame stream"
    assert f["close_and_open_before_one_step"], "close() and open() of one ring before the same step"
    assert f["left_out"] == f["streams"], "every stream is left out of a step in which another is fed"
    assert f["opened_not_fed"], "a stream opened in a step in which it is not fed"
    assert f["empty_step"], "a step that feeds nothing"
    assert {1, 3} <= f["batch_sizes"], "steps with B = 1 and with B = 3"
    assert min(f["reset_k"]) < 33 < max(f["reset_k"]), "reset() before and after the ring is full: %s" % f["reset_k"]
    seeds = [s["seed"] for s in sched.streams.values()]
    assert len(set(seeds)) == len(seeds), "every stream has its own content"
    if name == "rgb":
        assert f["max_groups"] >= 3 and f["max_sizes"] >= 2, "three frame kinds and two source sizes in one step"
        assert set(s["kind"] for s in sched.streams.values()) == {"u8a", "u8b", "u8s", "f32", "f64"}
        assert not sched.scene
    else:
        assert sched.scene
        assert f["cut_alone"], "a cut in one stream while another in the same step does not cut"
        assert f["two_cuts"], "two streams cutting in one step"
        assert f["suppressed"] >= 1, "a planted cut that scene_min_len = 3 suppresses: the window mixes scenes"
        assert max(f["cut_k"]) > 34, "a cut after the ring is full: %s" % f["cut_k"]
        assert f["planted_after_reset"] >= 1, "a scene change on the frame right after reset(): step 0 either way, no cut"
        if name != "model_size":
            assert f["max_sizes"] >= 2, "two source sizes in one step"
    # the feed order of some step is not its batch order: the model and the product both have to sort
    if name in ("rgb", "model_size"):
        rank = {"u8a": 1, "u8b": 0, "u8s": 2, "f32": 3, "f64": 4}
        assert any([rank[sched.streams[n]["kind"]] for w, n in ev if w == "feed"] !=
                   sorted(rank[sched.streams[n]["kind"]] for w, n in ev if w == "feed") for ev in sched)
    if name == "p010":
        want = {"host_u16", "host_u8", "dev_u8"} | ({"dev_u16"} if om._has_torch_uint16() else set())
        assert f["forms"] == want, "words and bytes, from the host and on the device: %s" % f["forms"]
        assert set(s["kind"] for s in sched.streams.values()) == {"pa", "pb"} and om.SIZES["pa"] != om.SIZES["pb"]
        assert f["size_returns"], "one of the two sizes is fed alone after a step that fed both, and both are fed again later"
        assert f["shared_launch"], "a run of two streams of one size"
        # tests/test_gpu_online_model.py runs this schedule under border="keep": a reset() and a planted cut on such a stream
        assert f["reset_k"] and f["cuts"]
    if name == "rgb":
        # the unstable half of a float64 frame between two rows rendered from the float32 slot (feed order 1, 3, 2)
        assert any([sched.streams[n]["kind"] for w, n in ev if w == "feed"] == ["u8s", "f64", "f32"] for ev in sched)


def test_stream_content_is_its_own():
    sched = om.make_schedule("rgb")
    for n, spec in sched.streams.items():
        fr = om.stream_frames(spec)
        assert fr.shape[0] == spec["n"]
        if spec["kind"] == "f64":
            assert fr.dtype == np.float64 and fr.min() > 0.0 and fr.max() < 1.0
            f32 = fr.astype(np.float32)
            a, b = (fr * 255.0).astype(np.uint8), (f32.astype(np.float64) * 255.0).astype(np.uint8)
            assert (a != b).mean() > 0.2, "float64 content whose bytes tell a float32 detour"
    nv = om.make_schedule("nv12")
    fr = om.stream_frames(nv.streams["a"])
    assert fr.dtype == np.uint8 and fr.shape[1:] == (60, 48)


def test_p010_content_uses_all_sixteen_bits():
    """10-bit codes whose two bits below the high byte vary, seeded non-zero low 6 bits in every word, chroma around 512,
    and scenes whose high bytes (what the network and the cut statistic see) share no luma value; the uint8 form is the
    same words' bytes."""
    sched = om.make_schedule("p010")
    for n, spec in sched.streams.items():
        fr = om.stream_frames(spec)
        H, W = om.SIZES[spec["kind"]]
        u16 = spec["form"].endswith("u16")
        assert fr.dtype == (np.uint16 if u16 else np.uint8) and fr.shape == (spec["n"], 3 * H // 2, W if u16 else 2 * W), n
        words = fr if u16 else fr.view("<u2")
        assert np.array_equal(om.stream_frames(dict(spec, form="host_u16")), words)
        assert ((words & 0x3F) != 0).all()
        code = words >> 6
        assert len(np.unique(code[:, :H] & 3)) == 4 and len(np.unique(code[:, H:] & 3)) == 4
        y, uv = code[:, :H].astype(int), code[:, H:].astype(int)
        assert 64 <= y.min() and y.max() <= 940 and 480 <= uv.min() and uv.max() <= 544 and uv.min() < 512 < uv.max()
        sc = np.asarray(spec["scenes"])
        hi = words[:, :H] >> 8
        if (sc == 0).any() and (sc == 1).any():
            assert hi[sc == 0].max() < hi[sc == 1].min()
    nv = om.stream_frames(om.make_schedule("nv12").streams["a"])
    pa = om.stream_frames(sched.streams["a"])
    assert np.abs((pa[:, :40] >> 8).astype(int) - nv[:, :40]).max() <= 1, "the high byte is the NV12 schedule's luma"


def test_planted_cuts_are_the_only_cuts_of_the_float_content():
    """score >= 0.75 exactly where the scene changes (model-size float32 content, which the statistic reads as it is)."""
    sched = om.make_schedule("model_size")
    for n, spec in sched.streams.items():
        fr = om.stream_frames(spec).astype(np.float32)
        if fr.shape[0] < 2:
            continue
        sc = np.asarray(spec["scenes"])
        assert np.array_equal(scene_ref.scores(fr) >= om.THRESHOLD, sc[1:] != sc[:-1]), n


# ---------------------------------------------------------------------------------------------------------------------
# 2. the history rule against eval.py's list loop
# ---------------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def _fake_stabilise(window):
    """The "result" of a window: the tuple of its labels, named by a short label of its own (a tuple of tuples of tuples
    would grow sevenfold per step).  Equal windows get equal labels, different windows different ones."""
    return _RESULTS.setdefault(tuple(window), "s%d" % len(_RESULTS))


def _eval_py_loop(frames, skip=om.SKIP):
    """eval.py:93-124 on a list."""
    total = list(frames)
    span = skip[-1] - skip[0]
    for _ in range(span):
        total.insert(0, total[0])
    idx, outs = list(skip), []
    for frame_idx in range(span, len(total)):
        s_t_pred = _fake_stabilise(total[i] for i in idx)
        outs.append(s_t_pred)
        total[idx[-1]] = s_t_pred
        if frame_idx == span:
            for i in range(span):
                total[i] = s_t_pred
        idx = [i + 1 for i in idx]
    return outs


@pytest.mark.parametrize("runs", [[100], [1, 1, 2, 33, 34, 29], [32, 35, 33], [5, 70, 25]])
def test_history_is_eval_py(runs):
    """100 frames; reset() after each run, so the runs' first frames are first frames after a reset."""
    h = om.History()
    label, got, want = 0, [], []
    for n in runs:
        frames = list(range(label, label + n))
        label += n
        want += _eval_py_loop(frames)
        for f in frames:
            r = _fake_stabilise(h.window(f))
            got.append(r)
            h.write_back(r)
        assert h.k == n and len(h.total) <= 33, "entries nothing can read are dropped"
        h.restart()
    assert label == 100 and got == want
    assert got[0] == _fake_stabilise((0,) * 7), "step 0: 32 copies of the unstable frame and that frame"
    assert len(set(got)) == 100, "every step has a window of its own"


def test_history_other_skip():
    skip = (0, 3, 5)
    h = om.History(skip)
    got = []
    for f in range(12):
        r = _fake_stabilise(h.window(f))
        got.append(r)
        h.write_back(r)
    assert got == _eval_py_loop(list(range(12)), skip)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the scene state machine against scene_ref.scene_step
# ---------------------------------------------------------------------------------------------------------------------
def _frame_with_bins(bins, H, W):
    """a grey float32 frame whose pixel p falls into luma bin bins[p]"""
    v = ((4.0 * np.asarray(bins, dtype=np.float64) + 1.5) / 255.0).astype(np.float32).reshape(H, W, 1)
    return np.repeat(v, 3, axis=2)


@pytest.mark.parametrize("min_len", [0, 1, 3])
def test_scene_state_is_scene_step(min_len):
    rng = np.random.default_rng(77 + min_len)
    H, W, span = 6, 8, om.SKIP[-1]
    thr = scene_ref.threshold_count(0.5, H, W)
    state = np.zeros((2, scene_ref.STATE_INTS), dtype=np.int32)
    pool = np.zeros((2 * (span + 2), H, W, 3), dtype=np.float32)
    mine = [om.SceneState(thr, min_len) for _ in range(2)]
    cuts_seen = 0
    for step in range(120):
        rows = [0, 1] if step % 5 else [1]          # ring 0 is left out of every fifth step
        hists = {}
        for r in rows:
            if step in (40, 41) and r == 1:         # the caller's reset, twice in a row
                state[r] = 0
                mine[r].restart()
            side = int(rng.random() < 0.3)          # which half of the bins most pixels fall into
            far = rng.random(H * W) < (0.9 if side else 0.1)
            bins = np.where(far, rng.integers(32, 64, H * W), rng.integers(0, 32, H * W))
            frame = _frame_with_bins(bins, H, W)
            pool[r * (span + 2) + span + 1] = frame
            hists[r] = scene_ref.histogram(frame)
            assert np.array_equal(hists[r], np.bincount(bins, minlength=64)), "the frame has the histogram it was built for"
        _, _, cut = scene_ref.scene_step(pool, np.array(rows, dtype=np.int32), om.SKIP, state, thr, min_len)
        for b, r in enumerate(rows):
            assert mine[r].step(hists[r]) == bool(cut[b]), "step %d ring %d" % (step, r)
            assert (mine[r].k, mine[r].cuts, mine[r].S) == tuple(int(v) for v in state[r, :3]), "step %d ring %d" % (step, r)
        cuts_seen += int(cut.sum())
    assert cuts_seen >= 10
