"""GPU: checkpoints of another window length (conv1 [7,7,3S,64], S != 7) through every layer above the root-conv kernel:
LocNet against the oracle in every precision, stabilize_clip and OnlineStabilizer with a 5-entry skip_length, float16
calibration, graph capture, and the host-side rejections.  The tolerances are the ones the S = 7 tests use at these shapes
(test_gpu_cnn.py, test_gpu_f32x3.py, test_gpu_f32s.py, test_gpu_f16.py), unchanged."""
import numpy as np
import pytest

import inputs

SKIP5 = (0, 16, 24, 28, 32)
F_TOL = {"f32": 1e-5, "f32s": 1e-5, "f32x3": 1e-5, "f16": 5e-5}
# pixels outside the counted border-discontinuity pixels: (tolerance, delta of the border mask): test_gpu_cnn.py's
# test_stabnet_evaluation_model for the float32 family, test_gpu_f16.py's test_f16_stabilize_and_determinism for float16
PIX_TOL = {"f32": (3e-3, 3e-2), "f32s": (3e-3, 3e-2), "f32x3": (3e-3, 3e-2), "f16": (6e-3, 0.2)}
# the cap on the counted pixels is the one those tests put on the delta = 3e-2 mask; the float16 test's wider delta = 0.2
# mask carries none there (2.0 % / 2.1 % of the pixels of these two windows, printed below)
BORDER_CAP = 0.01
SEED = {5: 231, 8: 232}

_WEIGHTS = {}
_ORACLE = {}


def weights_for(S):
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if S not in _WEIGHTS:
        _WEIGHTS[S] = make_synthetic_weights(seed=0, c_in=3 * S)
    return _WEIGHTS[S]


def oracle_for(S):
    """the oracle's evaluation graph on the S-frame windows of this file, computed once: (x, s_t_pred, F_t, x_s, y_s)"""
    from oracle import model as omodel
    if S not in _ORACLE:
        B, H, W = 2, 64, 96
        x = inputs.window_frames(SEED[S], B, H, W, S)
        ref = omodel.StabNet(H, W).run(weights_for(S), x, x[..., -3:], fetch=("s_t_pred", "F_t", "x_offset_t", "y_offset_t"))
        _ORACLE[S] = (x,) + tuple(ref)
    return _ORACLE[S]


def _model(S, H, W, precision="f32"):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights_for(S))
    model.get_evaluation_model(S)
    model.precision = precision
    return model


@pytest.mark.parametrize("S", [5, 8])
def test_the_chosen_seeds_stay_under_the_border_cap(S):
    """No GPU, the oracle alone: the border-discontinuity pixels the end-to-end test leaves out are under the cap."""
    from oracle import thin_plate_spline as otps
    x, r_pred, r_F, r_x, r_y = oracle_for(S)
    B, H, W = x.shape[:3]
    assert otps.border_discontinuity_mask(r_x, r_y, H, W, delta=3e-2).mean() < BORDER_CAP, S


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f32s", "f32x3", "f16"])
@pytest.mark.parametrize("S", [5, 8])
def test_evaluation_graph_against_the_oracle(S, precision):
    from coupe.dvsg_amd.model import Session
    from oracle import thin_plate_spline as otps
    x, r_pred, r_F, r_x, r_y = oracle_for(S)
    B, H, W = x.shape[:3]
    model = _model(S, H, W, precision)
    assert model.locnet.in_channels == 3 * S
    ins, outs = model.get_evaluation_model(S)
    pred, F, xs, ys = Session().run([outs["s_t_pred"], outs["F_t"], outs["x_offset_t"], outs["y_offset_t"]],
                                    {ins["patches_t"]: x, ins["u_t"]: x[..., -3:]})
    ferr = np.abs(F - r_F).max()
    tol, delta = PIX_TOL[precision]
    border = otps.border_discontinuity_mask(r_x, r_y, H, W, delta=delta).reshape(B, H, W)
    perr = np.abs(pred - r_pred).max(axis=3)[~border].max()
    print("S = %d %s: F_t error %.3g, pixel error %.3g, border pixels %.4f" % (S, precision, ferr, perr, border.mean()))
    assert ferr <= F_TOL[precision], ferr
    assert (delta != 3e-2 or border.mean() < BORDER_CAP) and perr < tol, perr


@pytest.mark.gpu
def test_clip_loop_through_the_ring_is_the_window_loop():
    """stabilize_clip with a 5-entry skip_length against the oracle's recurrence (window_index_table) fed window by window
    through LocNet.stabilize on the gathered window: bit for bit, as test_gpu_ring.py asserts for S = 7."""
    import torch
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.clip import stabilize_clip, window_index_table
    from coupe.dvsg_amd.model import Session
    N, H, W, S = 40, 32, 48, 5
    frames = inputs.smooth_frames(3001, N, H, W)
    model = _model(S, H, W)
    got = stabilize_clip(model, Session(), frames, skip_length=SKIP5)
    table_h = window_index_table(N, SKIP5)
    assert table_h.shape == (N, S)
    table = torch.from_numpy(table_h).cuda()
    pool = torch.empty((2 * N, H, W, 3), device="cuda")
    pool[:N] = torch.from_numpy(frames).cuda()
    F = torch.empty((1, 25, 2), device="cuda")
    x = torch.empty((1, H, W, 3 * S), device="cuda")
    for k in range(N):
        _lib.call("dvsg_window_gather_f32", pool.data_ptr(), 2 * N, H, W, table[k:k + 1].data_ptr(), 1, S, x.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        model.locnet.stabilize(x, pool[k:k + 1], pool[N + k:N + k + 1], F)
    assert np.array_equal(got, pool[N:].cpu().numpy())


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s, frame %d" % (what, k)
        assert g.tobytes() == w.tobytes(), "%s, frame %d: %d values differ" % (what, k, int((g != w).sum()))


@pytest.mark.gpu
def test_two_online_streams_are_two_clips():
    """Two streams of different length in one OnlineStabilizer(skip_length=5 entries), pushed in turn: each is stabilize_clip
    of its own frames, bit for bit (the ring of 34 frames wraps for the longer one)."""
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import Session
    from coupe.dvsg_amd.online import OnlineStabilizer
    H, W = 32, 48
    model = _model(5, H, W)
    clips = [inputs.smooth_frames(3002, 40, H, W), inputs.smooth_frames(3003, 9, H, W)]
    on = OnlineStabilizer(model, max_streams=2, skip_length=SKIP5)
    sids = [on.open(), on.open()]
    got = [[], []]
    for k in range(40):
        for i in range(2):
            if k < len(clips[i]):
                got[i].append(on.push(sids[i], clips[i][k]))
    for i in range(2):
        want = stabilize_clip(model, Session(), clips[i], skip_length=SKIP5)
        _same(got[i], list(want), "stream %d" % i)


@pytest.mark.gpu
def test_a_planted_cut_restarts_a_five_frame_stream():
    """scene_cut with S = 5: scene A then scene B through one stream -- A's outputs are those of a stream without the
    option, B's those of a fresh stream (dvsg_scene_step_f32 writes the [B,S] table rows)."""
    import scene_ref
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(5, 32, 48)
    A, B = scene_ref.scene_a(12), scene_ref.scene_b(12)
    on = OnlineStabilizer(model, skip_length=SKIP5, scene_cut=scene_ref.THRESHOLD)
    off, fresh = OnlineStabilizer(model, skip_length=SKIP5), OnlineStabilizer(model, skip_length=SKIP5)
    s_on, s_off, s_fresh = on.open(), off.open(), fresh.open()
    got = [on.push(s_on, f) for f in np.concatenate([A, B])]
    _same(got[:12], [off.push(s_off, f) for f in A], "scene A against scene_cut=None")
    want_b = [fresh.push(s_fresh, f) for f in B]
    _same(got[12:], want_b, "scene B against a fresh stream")
    st = on.scene_state(s_on)
    assert st["cuts"] == 1 and st["frames_since_cut"] == 12
    carried = [off.push(s_off, f) for f in B[:2]]
    assert any(c.tobytes() != w.tobytes() for c, w in zip(carried, want_b)), "without a restart the old history warps B"


@pytest.mark.gpu
def test_nv12_streams_with_five_frames():
    """frame_format="nv12" at one small even size, S = 5: two streams of different length pushed in turn are
    stabilize_clips' per-clip results, bit for bit."""
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    model = _model(5, 32, 48)
    H0, W0 = 36, 64
    clips = []
    for seed, n in ((4001, 20), (4002, 7)):
        y = np.round(16 + 219 * inputs.smooth_frames(seed, n, H0, W0, C=1)[..., 0]).astype(np.uint8)
        clips.append(np.concatenate([y, np.full((n, H0 // 2, W0), 128, np.uint8)], axis=1))
    on = OnlineStabilizer(model, max_streams=2, skip_length=SKIP5, frame_format="nv12")
    sids = [on.open(), on.open()]
    got = [[], []]
    for k in range(20):
        for i in range(2):
            if k < len(clips[i]):
                got[i].append(on.push(sids[i], clips[i][k]))
    assert got[0][0].shape == (3 * H0 // 2, W0) and got[0][0].dtype == np.uint8
    for i in range(2):
        want = stabilize_clips(model, [clips[i]], skip_length=SKIP5, frame_format="nv12")[0]
        _same(got[i], list(want), "NV12 stream %d" % i)


@pytest.mark.gpu
def test_calibrated_float16_at_five_frames():
    """calibrate_f16 (whose float32 pass starts with the root-conv kernel) followed by a float16 forward stays inside the
    float16 tolerance against the oracle"""
    import torch
    from coupe.dvsg_amd.networks import LocNet
    x, r_pred, r_F, r_x, r_y = oracle_for(5)
    net = LocNet(weights_for(5))
    xd = torch.from_numpy(x).cuda()
    before = net.forward(xd, precision="f16").cpu().numpy()
    net.calibrate_f16(xd)
    after = net.forward(xd, precision="f16").cpu().numpy()
    print("float16 F_t error at S = 5: pairs %.3g, calibrated %.3g" % (np.abs(before - r_F).max(), np.abs(after - r_F).max()))
    assert np.abs(before - r_F).max() < F_TOL["f16"] and np.abs(after - r_F).max() < F_TOL["f16"]
    assert np.abs(net.forward(xd, precision="f32").cpu().numpy() - r_F).max() <= F_TOL["f32"]


@pytest.mark.gpu
def test_a_five_frame_ring_step_replays_from_a_captured_graph():
    """LocNet.stabilize_ring at S = 5 (dynamic LDS, its limit raised when the handle was made) captured once and replayed
    twice on fresh pool values: bit for bit the eager call."""
    import torch
    from coupe.dvsg_amd.networks import LocNet
    B, H, W, n, S = 2, 64, 96, 12, 5
    net = LocNet(weights_for(S))
    pools = [torch.from_numpy(inputs.smooth_frames(281 + i, n, H, W)).cuda() for i in range(3)]
    table = torch.from_numpy(np.random.default_rng(9).integers(0, n, (B, S)).astype(np.int32)).cuda()
    pool = pools[0].clone()
    out, F = torch.empty((B, H, W, 3), device="cuda"), torch.empty((B, 25, 2), device="cuda")
    net.stabilize_ring(pool, table, out, F)            # warm-up: the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.stabilize_ring(pool, table, out, F)
    for fresh in pools[1:]:
        pool.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        got_out, got_F = out.clone(), F.clone()
        want_out, want_F = torch.empty_like(out), torch.empty_like(F)
        net.stabilize_ring(fresh, table, want_out, want_F)
        torch.cuda.synchronize()
        assert torch.equal(got_out, want_out) and torch.equal(got_F, want_F)


@pytest.mark.gpu
def test_window_width_is_still_checked_on_the_host(synthetic_weights):
    """A 15-channel model rejects a 7-entry skip_length and a [B,7] table; a 21-channel model still rejects a 5-entry one."""
    import torch
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import Session, StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    H, W = 32, 48
    frames = inputs.smooth_frames(252, 2, H, W)
    m5 = _model(5, H, W)
    with pytest.raises(ValueError, match="conv1"):
        stabilize_clip(m5, Session(), frames)                       # the default 7-entry skip_length
    with pytest.raises(ValueError, match="conv1"):
        OnlineStabilizer(m5)
    pool = torch.zeros((8, H, W, 3), device="cuda")
    out, F = torch.empty((1, H, W, 3), device="cuda"), torch.empty((1, 25, 2), device="cuda")
    with pytest.raises(ValueError, match=r"\[B,5\]"):
        m5.locnet.stabilize_ring(pool, torch.zeros((1, 7), dtype=torch.int32, device="cuda"), out, F)
    with pytest.raises(ValueError, match="15"):
        m5.locnet.forward_masked(torch.zeros((1, H, W, 21), device="cuda"), torch.ones((1, H, W), device="cuda"))
    m7 = StabNet(H, W).load_weights(synthetic_weights)
    m7.get_evaluation_model(7)
    with pytest.raises(ValueError, match="conv1"):
        stabilize_clip(m7, Session(), frames, skip_length=SKIP5)
    with pytest.raises(ValueError, match=r"\[B,7\]"):
        m7.locnet.stabilize_ring(pool, torch.zeros((1, 5), dtype=torch.int32, device="cuda"), out, F)
