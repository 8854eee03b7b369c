"""GPU: online streams over bounded frame rings (coupe.dvsg_amd.online, include/dvsg_amd.h "ONLINE streams").

The new entry points only move where frames are read from or written to, so against the calls they restate the bar
is BIT equality: dvsg_stabilize_ring_inplace_f32 against dvsg_stabilize_ring_f32, dvsg_frames_ingest_u8 against
dvsg_frames_u8_to_f32 / dvsg_frames_resize_u8_f32, dvsg_frames_f32_to_u8_slots against dvsg_frames_f32_to_u8, and one
online stream against stabilize_clip.  Streams batched together differ from one clip alone by float32 re-association in
the CNN only (split-K / stream-K cuts depend on the launch's tile count), which the recurrence carries forward: they are
held to the golden clip loop's bounds (tests/test_gpu_golden.py::test_eval_clip_loop)."""
import os

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def net(synthetic_weights):
    import torch
    assert torch.cuda.is_available()
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


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
# 1. the kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16", "f32s", "f32x3"])
@pytest.mark.parametrize("H,W", [(64, 96), (37, 53), (20, 4)])
def test_inplace_ring_is_the_contiguous_ring(net, precision, H, W):
    """Results written into permuted pool slots equal dvsg_stabilize_ring_f32's contiguous s_t_pred, F_t, x_s, y_s;
    every other pool frame is left alone."""
    import torch
    B, n = 3, 12
    rng = np.random.default_rng(H * 1000 + W)
    pool = torch.from_numpy(np.concatenate([inputs.smooth_frames(500 + H + i, 4, H, W) for i in range(3)])).cuda()
    slots = np.array([n - 1, n - 3, n - 2], dtype=np.int32)            # permuted, none of them in the table
    table = torch.from_numpy(rng.integers(0, n - 3, (B, 7)).astype(np.int32)).cuda()

    def outs():
        return (torch.empty((B, 25, 2), device="cuda"), torch.empty((B * H * W,), device="cuda"),
                torch.empty((B * H * W,), device="cuda"))
    want_out = torch.empty((B, H, W, 3), device="cuda")
    wF, wx, wy = outs()
    net.stabilize_ring(pool, table, want_out, wF, wx, wy, precision=precision)
    got_pool = pool.clone()
    gF, gx, gy = outs()
    net.stabilize_ring_inplace(got_pool, table, torch.from_numpy(slots).cuda(), gF, gx, gy, precision=precision)
    torch.cuda.synchronize()
    for b in range(B):
        assert torch.equal(got_pool[int(slots[b])], want_out[b]), "sample %d: max diff %g" % (
            b, float((got_pool[int(slots[b])] - want_out[b]).abs().max()))
    assert torch.equal(got_pool[:n - 3], pool[:n - 3])
    for g, w_, name in ((gF, wF, "F_t"), (gx, wx, "x_s"), (gy, wy, "y_s")):
        assert torch.equal(g, w_), "%s: max diff %g" % (name, float((g - w_).abs().max()))


def test_inplace_ring_out_of_range_slot_writes_nothing(net):
    import torch
    B, H, W, n = 3, 40, 64, 10
    pool = torch.from_numpy(np.concatenate([inputs.smooth_frames(600 + i, 5, H, W) for i in range(2)])).cuda()
    table = torch.from_numpy(np.random.default_rng(6).integers(0, n - 1, (B, 7)).astype(np.int32)).cuda()
    want_out, wF = torch.empty((B, H, W, 3), device="cuda"), torch.empty((B, 25, 2), device="cuda")
    net.stabilize_ring(pool, table, want_out, wF)
    got_pool, gF = pool.clone(), torch.empty((B, 25, 2), device="cuda")
    net.stabilize_ring_inplace(got_pool, table, torch.tensor([n, n - 1, -1], dtype=torch.int32, device="cuda"), gF)
    torch.cuda.synchronize()
    assert torch.equal(got_pool[:n - 1], pool[:n - 1])
    assert torch.equal(got_pool[n - 1], want_out[1])
    assert torch.equal(gF, wF)


def _ingest(src, pool, slots, H, W, flip, u8=None, u8_W=0, u8_x0=0):
    from coupe.dvsg_amd import _lib
    n, sh, sw = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    _lib.call("dvsg_frames_ingest_u8", src.data_ptr(), n, sh, sw, flip, pool.data_ptr(), int(pool.shape[0]),
              slots.data_ptr(), H, W, u8.data_ptr() if u8 is not None else 0, u8_W, u8_x0, _stream())


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("H,W", [(32, 48), (37, 53), (1, 1)])
def test_ingest_same_size_is_u8_to_f32(flip, H, W):
    import torch
    from coupe.dvsg_amd import _lib
    n = 3
    src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H)).cuda()
    want = torch.empty((n, H, W, 3), device="cuda")
    _lib.call("dvsg_frames_u8_to_f32", src.data_ptr(), n * H * W, flip, want.data_ptr(), _stream())
    pool = torch.full((7, H, W, 3), -7.0, device="cuda")
    slots = torch.tensor([5, 0, 3], dtype=torch.int32, device="cuda")
    _ingest(src, pool, slots, H, W, flip)
    torch.cuda.synchronize()
    for i, s in enumerate([5, 0, 3]):
        assert torch.equal(pool[s], want[i])
    assert bool((pool[[1, 2, 4, 6]] == -7.0).all())


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("with_u8", [False, True])
def test_ingest_resized_is_resize_u8_f32(flip, with_u8):
    import torch
    from coupe.dvsg_amd import _lib
    n, sh, sw, H, W = 3, 45, 70, 32, 48
    src = torch.randint(0, 256, (n, sh, sw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).cuda()
    want = torch.empty((n, H, W, 3), device="cuda")
    want8 = torch.zeros((n, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    _lib.call("dvsg_frames_resize_u8_f32", src.data_ptr(), n, sh, sw, flip, want.data_ptr(), H, W,
              want8.data_ptr() if with_u8 else 0, 2 * W, 0, _stream())
    pool = torch.full((6, H, W, 3), -7.0, device="cuda")
    got8 = torch.zeros((n, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    slots = [4, 1, 2]
    _ingest(src, pool, torch.tensor(slots, dtype=torch.int32, device="cuda"), H, W, flip,
            got8 if with_u8 else None, 2 * W, 0)
    torch.cuda.synchronize()
    for i, s in enumerate(slots):
        assert torch.equal(pool[s], want[i])
    assert bool((pool[[0, 3, 5]] == -7.0).all())
    assert torch.equal(got8, want8)
    if with_u8:
        assert int(got8[:, :, :W].max()) > 0


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("H,W", [(32, 48), (37, 53)])
def test_f32_to_u8_slots_is_f32_to_u8(flip, H, W):
    import torch
    from coupe.dvsg_amd import _lib
    pool = torch.rand((5, H, W, 3), generator=torch.Generator().manual_seed(W)).cuda()
    slots = [3, 0, 4]
    want = torch.zeros((3, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    _lib.call("dvsg_frames_f32_to_u8", pool[slots].contiguous().data_ptr(), 3, H, W, flip, want.data_ptr(), 2 * W, W,
              _stream())
    got = torch.zeros_like(want)
    _lib.call("dvsg_frames_f32_to_u8_slots", pool.data_ptr(), 5, torch.tensor(slots, dtype=torch.int32, device="cuda").data_ptr(),
              3, H, W, flip, got.data_ptr(), 2 * W, W, _stream())
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 2. one stream is stabilize_clip, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32x3"])
@pytest.mark.parametrize("case", ["float40", "float80", "u8_bgr_side80", "device40"])
def test_one_stream_is_stabilize_clip(synthetic_weights, precision, case):
    import torch
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import Session
    from coupe.dvsg_amd.online import OnlineStabilizer
    H, W = 32, 48
    model = _model(synthetic_weights, H, W, precision)
    kw = {}
    if case in ("float40", "device40"):
        frames = inputs.smooth_frames(3001, 40, H, W)        # the golden clip
    elif case == "float80":
        frames = inputs.smooth_frames(3002, 80, H, W)        # the ring wraps twice
    else:
        frames = (inputs.smooth_frames(3003, 80, 45, 70) * 255).astype(np.uint8)
        kw = dict(channel_order="bgr", side_by_side=True, as_uint8=True)
    if case == "device40":
        frames = torch.from_numpy(frames).cuda()
    want = stabilize_clip(model, Session(), frames, **kw)
    on = OnlineStabilizer(model, **kw)
    sid = on.open()
    got = [on.push(sid, frames[k]) for k in range(frames.shape[0])]
    if case == "device40":
        assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
        assert torch.equal(torch.stack(got), want)
    elif kw:
        assert np.array_equal(np.stack([g[0] for g in got]), want[0])
        assert np.array_equal(np.stack([g[1] for g in got]), want[1])
        assert want[0].dtype == np.uint8 and want[1].shape == (80, H, 2 * W, 3)
    else:
        assert np.array_equal(np.stack(got), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. many streams against the golden clip loop
# ---------------------------------------------------------------------------------------------------------------------
def _golden():
    with np.load(os.path.join(GOLD, "clip.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    N, H, W = 40, 32, 48
    mask = np.unpackbits(g["border_mask_bits"])[:N * H * W].astype(bool).reshape(N, H, W)
    return g["stabilised"], mask


def _meets_golden_bounds(out, ref, mask, what):
    n = out.shape[0]
    err = np.abs(out - ref[:n]).reshape(n, -1)
    med, bad = np.median(err, axis=1), (err > 1e-3).mean(axis=1)
    assert med.max() < 3e-6, "%s: median error per step %s" % (what, med)
    assert bad.max() <= 1e-3, "%s: fraction of values off by > 1e-3, per step: %s" % (what, bad)
    inner = np.abs(out - ref[:n]).max(axis=3)[~mask[:n]]
    assert inner.max() < 1e-4, "%s: max error away from the border jumps %.3g" % (what, inner.max())


def test_many_streams_against_golden(synthetic_weights):
    """Stream a runs the 40-frame golden clip; b opens at step 5 with its first 17 frames; c has one frame and closes,
    and d takes c's ring at the next step with the first 10 frames.  Each meets the golden bounds on its prefix."""
    from coupe.dvsg_amd.online import OnlineStabilizer, stabilize_clips
    H, W = 32, 48
    frames = inputs.smooth_frames(3001, 40, H, W)
    ref, mask = _golden()
    model = _model(synthetic_weights, H, W)
    on = OnlineStabilizer(model, max_streams=3)
    a, c = on.open(), on.open()
    plan = {a: frames, c: frames[:1]}
    got = {a: [], c: []}
    pos = {a: 0, c: 0}
    d = b = None
    for step in range(40):
        if step == 1:
            on.close(c)
            d = on.open()
            plan[d], got[d], pos[d] = frames[:10], [], 0
        if step == 5:
            b = on.open()
            plan[b], got[b], pos[b] = frames[:17], [], 0
        feed = {sid: plan[sid][pos[sid]] for sid in on.open_streams if pos[sid] < len(plan[sid])}
        for sid, out in on.step(feed).items():
            got[sid].append(out)
            pos[sid] += 1
    for sid, n in ((a, 40), (b, 17), (c, 1), (d, 10)):
        assert len(got[sid]) == n
        _meets_golden_bounds(np.stack(got[sid]), ref, mask, "stream %d" % sid)
    outs = stabilize_clips(model, [frames, frames[:17], frames[:1], frames[:10]], batch=3)
    for o, n in zip(outs, (40, 17, 1, 10)):
        assert o.shape == (n, H, W, 3)
        _meets_golden_bounds(o, ref, mask, "stabilize_clips clip of %d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bounded memory, 5. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_memory_is_bounded(synthetic_weights):
    import torch
    from coupe.dvsg_amd.online import OnlineStabilizer
    H, W = 32, 48
    model = _model(synthetic_weights, H, W)
    on = OnlineStabilizer(model, max_streams=2)
    assert tuple(on.pool.shape) == (2 * 34, H, W, 3)
    s0, s1 = on.open(), on.open()
    frames = (inputs.smooth_frames(3004, 8, 45, 70) * 255).astype(np.uint8)
    on.step({s0: frames[0], s1: frames[1]})
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    seen = []
    for k in range(1, 201):
        on.step({s0: frames[k % 8], s1: frames[(k + 3) % 8]})
        if k in (40, 200):
            torch.cuda.synchronize()
            seen.append(torch.cuda.memory_allocated())
    assert seen == [base, base]
    assert tuple(on.pool.shape) == (2 * 34, H, W, 3)


def test_errors_are_python_errors(synthetic_weights):
    import torch
    from coupe.dvsg_amd.online import OnlineStabilizer
    H, W = 32, 48
    model = _model(synthetic_weights, H, W)
    on = OnlineStabilizer(model, max_streams=2)
    frame = inputs.smooth_frames(3005, 1, H, W)[0]
    s0 = on.open()
    on.push(s0, frame)
    on.close(s0)
    with pytest.raises(ValueError, match="closed"):
        on.push(s0, frame)
    s1, s2 = on.open(), on.open()
    with pytest.raises(RuntimeError, match="all 2 streams"):
        on.open()
    with pytest.raises(ValueError, match="float frames must already be"):
        on.push(s1, inputs.smooth_frames(3005, 1, H + 1, W)[0])
    with pytest.raises(ValueError, match="never opened"):
        on.step({s1: frame, 99: frame})
    with pytest.raises(TypeError):
        on.push(s2, frame.astype(np.int32))
    # a refused step changed nothing: s1 is still at step 0 and gives stabilize_clip's first frame
    from coupe.dvsg_amd.clip import stabilize_clip
    assert np.array_equal(on.push(s1, frame), stabilize_clip(model, None, frame[None])[0])
    torch.cuda.synchronize()
