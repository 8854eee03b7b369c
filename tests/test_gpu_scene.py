"""GPU: scene cuts of live streams (dvsg_scene_step_f32, OnlineStabilizer(scene_cut=...); include/dvsg_amd.h "ONLINE streams,
SCENE CUTS").

The statistic is integer after one quantisation and the step only chooses which ring slots a stream reads and writes, so every
bar here is BIT equality: the kernel against its NumPy restatement (tests/scene_ref.py), and a stream with a detected cut
against close() + open() + push() done by hand.  Runs that are compared share their batch composition step by step (the CNN's
float32 association depends on the batch, tests/test_gpu_online.py)."""
import ctypes

import numpy as np
import pytest

import inputs
import scene_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
SKIP = (0, 16, 24, 28, 30, 31, 32)
THR = scene_ref.THRESHOLD


def _model(weights, H, W, precision="f32"):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights)
    model.get_evaluation_model(7)
    model.precision = precision
    return model


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel is its NumPy restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _frame(rng, H, W, lo, kind):
    """A float32 frame with luma around [lo, lo + 0.3]; kind poisons it."""
    f = (lo + 0.3 * rng.random((H, W, 3))).astype(F32)
    if kind == "nan":
        f[:] = np.nan
    elif kind == "wild":   # out-of-range values, infinities and a few NaN channels among ordinary pixels
        flat = f.reshape(-1, 3)
        idx = rng.permutation(flat.shape[0])[:max(4, flat.shape[0] // 7)]
        vals = np.array([-3.0, 7.5, np.inf, -np.inf, np.nan, 1.0, 0.0, -0.0], dtype=F32)
        flat[idx, rng.integers(0, 3, idx.size)] = vals[rng.integers(0, vals.size, idx.size)]
    return f


@pytest.mark.parametrize("with_zoom", [True, False])
@pytest.mark.parametrize("H,W,B,skip", [(20, 4, 1, SKIP), (37, 53, 3, SKIP), (32, 48, 2, SKIP), (64, 96, 5, SKIP),
                                        (288, 512, 2, (0, 3, 5))])
def test_scene_step_is_its_numpy_restatement(H, W, B, skip, with_zoom):
    """Three consecutive calls that carry state.  B valid rings in permuted order, one ring outside [0, n_state) and one whose
    input slot lies outside the pool; one ring starts in mid-run (k = 5); frames with NaN, infinities and out-of-range values.
    table, out_slots, cut, the whole state tensor and the zoom state equal the restatement's; the guard rows behind every
    output keep their poison and the pool is unchanged.  20 x 4: fewer pixels than one workgroup; 37 x 53: an odd pixel
    count, so odd frames start off the 16-byte grid (head and tail paths); 288 x 512: 36 workgroups per frame."""
    import torch
    from coupe.dvsg_amd import _lib
    rng = np.random.default_rng(H * 131 + W * 7 + B)
    S, span = len(skip), skip[-1]
    per = span + 2
    n_rings, n_state = B + 1, B + 3                 # the pool holds one ring more than the step uses; the state two more
    n_pool = n_rings * per + 1                      # + 1: ring B + 1's input slot is still outside
    pool = np.full((n_pool, H, W, 3), 0.25, dtype=F32)
    valid = rng.permutation(n_rings)[:B]
    rings = np.concatenate([valid, [n_state + 5, B + 1]]).astype(np.int32)
    rows = rings.size
    # without the zoom state the calls also run with min_len = 2, which holds back the cuts of a ring's second frame
    thr, min_len, crop_start = scene_ref.threshold_count(0.5, H, W), 1 if with_zoom else 2, 0.875
    state = np.zeros((n_state, 68), dtype=np.int32)
    state[valid[0], :4] = (5, 2, 17, 0)             # a ring in mid-run: its first row here is the window of step 5
    state[valid[0], 4:] = rng.multinomial(H * W, np.ones(64) / 64.0)
    for r in range(n_state):
        if r not in valid:
            state[r] = 12345 + r                    # rows no call may touch
    zoom = (0.5 + 0.01 * np.arange(n_state)).astype(F32)
    d_state = torch.from_numpy(state).cuda()
    d_zoom = torch.from_numpy(zoom).cuda()
    d_rings = torch.from_numpy(rings).cuda()
    c_skip = (ctypes.c_int32 * S)(*skip)
    need = ctypes.c_size_t()
    _lib.call("dvsg_scene_workspace_bytes", rows, ctypes.byref(need))
    assert need.value == rows * 64 * 4
    # per call and valid ring: (luma offset, poison).  Offsets 0.0 / 0.65 give disjoint histograms, so a change is a cut.
    plan = [[(0.0, None)] * B, [((0.65, "wild") if i % 2 == 0 else (0.0, None)) for i in range(B)],
            [((0.65, None) if i % 2 == 0 else (0.0, "nan" if i == 1 else "wild")) for i in range(B)]]
    cuts_seen = 0
    for call, frames in enumerate(plan):
        for i, (lo, kind) in enumerate(frames):
            pool[valid[i] * per + span + 1] = _frame(rng, H, W, lo, kind)
        d_pool = torch.from_numpy(pool).cuda()
        before = d_pool.clone()
        table = torch.full((rows + 1, S), -77, dtype=torch.int32, device="cuda")
        out_slots = torch.full((rows + 1,), -77, dtype=torch.int32, device="cuda")
        cut = torch.full((rows + 1,), -77, dtype=torch.int32, device="cuda")
        ws = torch.full((need.value // 4 + 64,), -77, dtype=torch.int32, device="cuda")
        _lib.call("dvsg_scene_step_f32", d_pool.data_ptr(), n_pool, H, W, d_rings.data_ptr(), rows, c_skip, S,
                  d_state.data_ptr(), n_state, thr, min_len, d_zoom.data_ptr() if with_zoom else None, crop_start,
                  table.data_ptr(), out_slots.data_ptr(), cut.data_ptr(), ws.data_ptr(), need.value, _stream())
        torch.cuda.synchronize()
        w_table, w_out, w_cut = scene_ref.scene_step(pool, rings, skip, state, thr, min_len, zoom if with_zoom else None,
                                                     crop_start)
        what = "call %d" % call
        assert np.array_equal(table[:rows].cpu().numpy(), w_table), what
        assert np.array_equal(out_slots[:rows].cpu().numpy(), w_out), what
        assert np.array_equal(cut[:rows].cpu().numpy(), w_cut), what
        assert np.array_equal(d_state.cpu().numpy(), state), what
        assert d_zoom.cpu().numpy().tobytes() == zoom.tobytes(), what
        assert bool((table[rows] == -77).all()) and int(out_slots[rows]) == -77 and int(cut[rows]) == -77, what
        assert bool((ws[need.value // 4:] == -77).all()), "%s: the workspace was written past its size" % what
        hist = ws[:need.value // 4].view(rows, 64).cpu().numpy()
        for b in range(B):
            assert np.array_equal(hist[b], state[rings[b], 4:]) and hist[b].sum() == H * W, what
        assert not hist[B:].any(), "%s: a skipped row has no histogram" % what
        assert torch.equal(d_pool.view(torch.int32), before.view(torch.int32)), "%s: the pool is only read" % what
        assert (w_table[B:] == -1).all() and (w_out[B:] == -1).all() and not w_cut[B:].any()
        cuts_seen += int(w_cut.sum())
    assert cuts_seen >= (1 if B == 1 or not with_zoom else 2), "the plan was meant to cut"
    for r in range(n_state):
        if r not in valid:
            assert (state[r] == 12345 + r).all()


# ---------------------------------------------------------------------------------------------------------------------
# the clips of the stream tests: the two scenes as float frames, as uint8 at 45 x 70 and as NV12 at 36 x 64
# ---------------------------------------------------------------------------------------------------------------------
def _levels(seed, n, H, W, lo, C=3):
    return (F32(lo) + F32(0.4) * inputs.smooth_frames(seed, n, H, W, C=C)).astype(F32)


def _clips(kind, n=12):
    """(A, B, OnlineStabilizer options): scene A's luma in [0.05, 0.45], scene B's in [0.55, 0.95] in every format (a resize is
    a convex combination and the grey NV12 frames convert to R = G = B)."""
    if kind == "float":
        return scene_ref.scene_a(n), scene_ref.scene_b(n), {}
    if kind == "u8_source_res":
        A, B = (np.round(_levels(s, n, 45, 70, lo) * 255).astype(np.uint8) for s, lo in ((4001, 0.05), (4002, 0.55)))
        return A, B, dict(source_res=True)
    assert kind == "nv12"
    out = []
    for s, lo in ((4001, 0.05), (4002, 0.55)):
        y = np.round(16 + 219 * _levels(s, n, 36, 64, lo, C=1)[..., 0]).astype(np.uint8)
        out.append(np.concatenate([y, np.full((n, 18, 64), 128, np.uint8)], axis=1))
    return out[0], out[1], dict(frame_format="nv12")


def _push_all(on, sid, frames):
    return [on.push(sid, f) for f in frames]


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s, frame %d" % (what, k)
        assert g.tobytes() == w.tobytes(), "%s, frame %d: %d values differ" % (what, k, int((g != w).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# 2. one stream with one cut
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x3"])
@pytest.mark.parametrize("kind", ["float", "u8_source_res", "nv12"])
def test_cut_restarts_the_stream(synthetic_weights, precision, kind):
    """Scene A (12 frames) then scene B (12 frames) through one stream with scene_cut=0.75: the A outputs are those of a
    stream without the option, the B outputs those of a fresh stream fed B alone, and the state reports the one cut.
    Without the restart the B outputs differ (the stream without the option, fed on, shows it)."""
    from coupe.dvsg_amd.online import OnlineStabilizer
    A, B, kw = _clips(kind)
    model = _model(synthetic_weights, 32, 48, precision)
    on = OnlineStabilizer(model, scene_cut=THR, **kw)
    off = OnlineStabilizer(model, **kw)
    fresh = OnlineStabilizer(model, **kw)
    s_on, s_off, s_fresh = on.open(), off.open(), fresh.open()
    assert on.scene_state(s_on) == dict(frames_since_cut=0, cuts=0, score=0.0)
    got = _push_all(on, s_on, np.concatenate([A, B]))
    st = on.scene_state(s_on)
    print("scene_state after A + B (%s, %s): %s" % (kind, precision, st))
    want_a = _push_all(off, s_off, A)
    want_b = _push_all(fresh, s_fresh, B)
    _same(got[:12], want_a, "scene A against scene_cut=None")
    _same(got[12:], want_b, "scene B against a fresh stream")
    assert st["cuts"] == 1 and st["frames_since_cut"] == 12 and 0.0 <= st["score"] < THR
    assert on._streams[s_on][1] == 24, "the host counts frames pushed"
    carried = _push_all(off, s_off, B[:2])
    assert any(c.tobytes() != w.tobytes() for c, w in zip(carried, want_b)), \
        "without a restart, B's first frames are warped by the old history"
    with pytest.raises(ValueError, match="without scene_cut"):
        off.scene_state(s_off)


# ---------------------------------------------------------------------------------------------------------------------
# 3. two streams: the cut of one is close() + open() by hand, the other is left alone
# ---------------------------------------------------------------------------------------------------------------------
def test_cut_is_close_and_open_at_two_streams(synthetic_weights):
    from coupe.dvsg_amd.online import OnlineStabilizer
    A, B = scene_ref.scene_a(), scene_ref.scene_b()
    C = _levels(4003, 24, 32, 48, 0.05)
    assert scene_ref.scores(C).max() < THR
    model = _model(synthetic_weights, 32, 48)
    on = OnlineStabilizer(model, max_streams=2, scene_cut=THR)
    hand = OnlineStabilizer(model, max_streams=2)
    s0, s1 = on.open(), on.open()
    h0, h1 = hand.open(), hand.open()
    AB = np.concatenate([A, B])
    for k in range(24):
        if k == 12:
            hand.close(h0)
            h0 = hand.open()
            assert hand._streams[h0][0] == 0, "the reopened stream takes the same ring"
        got = on.step({s0: AB[k], s1: C[k]})
        want = hand.step({h0: AB[k], h1: C[k]})
        _same([got[s0], got[s1]], [want[h0], want[h1]], "step %d" % k)
    assert on.scene_state(s0)["cuts"] == 1 and on.scene_state(s0)["frames_since_cut"] == 12
    assert on.scene_state(s1)["cuts"] == 0 and on.scene_state(s1)["frames_since_cut"] == 24


# ---------------------------------------------------------------------------------------------------------------------
# 4. crop="auto": the zoom restarts with the history
# ---------------------------------------------------------------------------------------------------------------------
def test_cut_restarts_the_crop_zoom(synthetic_weights):
    """crop_margin=0.25 puts free - margin below crop_start, so scene A ratchets the zoom down.  On the cut frame the zoom is
    the one a fresh stream has after its first frame, bit for bit, and the cropped outputs of scene B are the fresh stream's."""
    from coupe.dvsg_amd.online import OnlineStabilizer
    A, B = scene_ref.scene_a(), scene_ref.scene_b()
    model = _model(synthetic_weights, 32, 48)
    kw = dict(crop="auto", crop_margin=0.25)
    on = OnlineStabilizer(model, scene_cut=THR, **kw)
    fresh = OnlineStabilizer(model, **kw)
    s_on, s_fresh = on.open(), fresh.open()
    zooms = []
    for f in A:
        on.push(s_on, f)
        zooms.append(on.crop_state(s_on)["zoom"])
    print("zoom over scene A: %s" % [round(float(z), 4) for z in zooms])
    assert zooms[-1] < F32(1.0), "scene A was meant to lower the zoom"
    # the synthetic network bends every frame alike, so B alone would reach A's zoom again and hide a missing restart:
    # leave the ring where a harder shaken scene A would have left it (crop_min), below anything B reaches on its own
    on._crop_zoom[on._streams[s_on][0]] = on.crop_min
    assert on.crop_state(s_on)["zoom"] == F32(0.5)
    for k, f in enumerate(B):
        got, want = on.push(s_on, f), fresh.push(s_fresh, f)
        z, zf = on.crop_state(s_on), fresh.crop_state(s_fresh)
        assert z["zoom"].tobytes() == zf["zoom"].tobytes() and z["free"] == zf["free"], "frame %d of B: %s, %s" % (k, z, zf)
        _same([got], [want], "cropped frame %d of B" % k)
    assert on.scene_state(s_on)["cuts"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. no cut, no change
# ---------------------------------------------------------------------------------------------------------------------
def test_stream_without_a_cut_is_unchanged(synthetic_weights):
    """40 frames of one scene (the ring of 34 wraps): every output is that of scene_cut=None."""
    from coupe.dvsg_amd.online import OnlineStabilizer
    C = _levels(4003, 40, 32, 48, 0.05)
    assert scene_ref.scores(C).max() < THR
    model = _model(synthetic_weights, 32, 48)
    on, off = OnlineStabilizer(model, scene_cut=THR), OnlineStabilizer(model)
    s_on, s_off = on.open(), off.open()
    _same(_push_all(on, s_on, C), _push_all(off, s_off, C), "scene_cut=0.75 against None")
    st = on.scene_state(s_on)
    assert st["cuts"] == 0 and st["frames_since_cut"] == 40
    assert st["score"] == scene_ref.scores(C)[-1]


# ---------------------------------------------------------------------------------------------------------------------
# 6. reset(sid): the caller's own cut
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_cut", [None, THR])
def test_reset_is_a_fresh_stream(synthetic_weights, scene_cut):
    """Within one scene nothing is detected, so only reset() restarts the stream: the frames pushed after it equal a fresh
    stream's.  crop="auto" goes back to crop_start with it."""
    from coupe.dvsg_amd.online import OnlineStabilizer
    A = scene_ref.scene_a()
    model = _model(synthetic_weights, 32, 48)
    kw = dict(crop="auto", crop_margin=0.25)
    on = OnlineStabilizer(model, scene_cut=scene_cut, **kw)
    fresh = OnlineStabilizer(model, **kw)
    s_on, s_fresh = on.open(), fresh.open()
    _push_all(on, s_on, A[:5])
    assert on.crop_state(s_on)["zoom"] < F32(1.0)
    on.reset(s_on)
    assert on.crop_state(s_on) == dict(zoom=F32(1.0), free=None)
    if scene_cut is not None:
        assert on.scene_state(s_on) == dict(frames_since_cut=0, cuts=0, score=0.0)
    _same(_push_all(on, s_on, A[5:10]), _push_all(fresh, s_fresh, A[5:10]), "after reset()")
    assert on.crop_state(s_on)["zoom"].tobytes() == fresh.crop_state(s_fresh)["zoom"].tobytes()
    if scene_cut is not None:
        st = on.scene_state(s_on)
        assert st["cuts"] == 0 and st["frames_since_cut"] == 5
    with pytest.raises(ValueError, match="never opened"):
        on.reset(99)


# ---------------------------------------------------------------------------------------------------------------------
# 7. stabilize_clips passes the option through
# ---------------------------------------------------------------------------------------------------------------------
def test_stabilize_clips_passes_scene_cut_through(synthetic_weights):
    """[A + B, A]: the per-stream runs are driven by hand in the same lockstep (two streams for 12 steps, then clip 0 alone on
    its own ring, restarted by close() + open()), because batching changes the CNN's float32 association."""
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    A, B = scene_ref.scene_a(), scene_ref.scene_b()
    model = _model(synthetic_weights, 32, 48)
    got = stabilize_clips(model, [np.concatenate([A, B]), A], scene_cut=THR)
    assert got[0].shape == (24, 32, 48, 3) and got[1].shape == (12, 32, 48, 3)
    hand = OnlineStabilizer(model, max_streams=2)
    h0, h1 = hand.open(), hand.open()
    want0, want1 = [], []
    for k in range(12):
        r = hand.step({h0: A[k], h1: A[k]})
        want0.append(r[h0])
        want1.append(r[h1])
    hand.close(h0)
    hand.close(h1)
    h0 = hand.open()
    want0 += _push_all(hand, h0, B)
    _same(list(got[0]), want0, "clip A + B")
    _same(list(got[1]), want1, "clip A")
