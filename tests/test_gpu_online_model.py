"""GPU: `OnlineStabilizer` against the unbounded-history model (tests/online_model.py), bit for bit at every step.

Each case drives the product and the model through one schedule of about 90 steps and 7 streams on 3 rings
(`online_model.make_schedule`; tests/test_online_model_cpu.py asserts what each schedule contains): rings that wrap twice,
rings reused after a long and after a 1-frame stream, streams left out of steps, empty steps, reset() before and after the
ring is full, mixed frame kinds and source sizes in one step, and -- in the scene schedules -- planted cuts alone, in two
streams at once, suppressed by scene_min_len, after the ring is full and on the frame after a reset().  Every returned
output must be `array_equal` (uint8, float32 and NV12 bytes, both halves of a side_by_side pair); after the last step
`crop_state` and `scene_state` of every open stream must match, and the cuts the model saw must be the planted ones.

`test_p010_all_options` drives the "p010" schedule (10-bit surfaces of two sizes, fed as host and device words and bytes; a size
that disappears for a step and comes back) in two forms, `test_stabilize_clips_p010` holds stabilize_clips(frame_format="p010"),
the expected value of tests/test_gpu_p010.py::test_pipes_ten_bit, to the model.

The model runs ONE `LocNet.stabilize` call per step at the product's B and batch order, so no tolerance is needed; the
premise (a ring call at B is gather + stabilise at B; the n = 1 renders are the batched ones) is pinned by
tests/test_gpu_ring.py and tests/test_gpu_online.py and was not measured for these schedules before this file ran.
`test_batch_rows_permute` pins what the model relies on beyond that: a row's result does not depend on its position.

Measured on one MI355X in one run (the yardstick tests/test_gpu_online.py::test_one_stream_is_stabilize_clip[f32-float80]
took 1.02 s there): test_rgb_model_size plain-f32 1.62 s (it also computes the schedule's content), plain-f16 0.97 s,
side_u8_bgr 1.04 s; test_source_res_all_options keep_f32 1.47 s, mirror_side_u8 1.08 s; test_nv12_all_options 1.20 s;
test_model_size_crop_and_cuts 1.18 s; test_stabilize_clips 1.06 s; test_batch_rows_permute 0.85 - 0.92 s per precision."""
import numpy as np
import pytest

import inputs
import online_model as om

pytestmark = pytest.mark.gpu
H, W = om.MODEL_H, om.MODEL_W


def _model(weights, precision="f32"):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights)
    model.get_evaluation_model(7)
    model.precision = precision
    return model


_CONTENT = {}


def _content(sched):
    """The streams' frames, computed once per schedule: NumPy for the streams fed from the host, device tensors otherwise."""
    import torch
    if sched.name not in _CONTENT:
        _CONTENT[sched.name] = {n: om.stream_frames(spec) for n, spec in sched.streams.items()}
    return {n: (fr if sched.streams[n]["host"] else torch.from_numpy(fr).cuda()) for n, fr in _CONTENT[sched.name].items()}


def _parts(o):
    import torch
    names = ("out", "side") if isinstance(o, tuple) else ("out",)
    vals = o if isinstance(o, tuple) else (o,)
    return [(n, v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for n, v in zip(names, vals)]


def _same_outputs(got, want, where):
    assert list(got) == list(want), "%s: the outputs' stream ids %s, the model's %s" % (where, list(got), list(want))
    for sid in want:
        assert isinstance(got[sid], tuple) == isinstance(want[sid], tuple), "%s, stream %d" % (where, sid)
        for (name, g), (_, w_) in zip(_parts(got[sid]), _parts(want[sid])):
            what = "%s, stream %d (%s), output %r" % (where, sid, where_k.get(sid, "?"), name)
            assert g.dtype == w_.dtype and g.shape == w_.shape, "%s: %s %s against %s %s" % (what, g.dtype, g.shape, w_.dtype,
                                                                                              w_.shape)
            assert np.array_equal(g, w_), "%s: %d of %d values differ" % (what, int((g != w_).sum()), g.size)


where_k = {}   # sid -> "name, k = ..." of the step being compared, for the failure message


def _run(sched, on, ref):
    import torch
    frames = _content(sched)
    sid, pos = {}, {n: 0 for n in sched.streams}
    for t, events in enumerate(sched):
        feed = {}
        for what, n in events:
            if what == "open":
                sid[n] = on.open()
                assert ref.open() == sid[n]
            elif what == "close":
                on.close(sid[n])
                ref.close(sid[n])
            elif what == "reset":
                on.reset(sid[n])
                ref.reset(sid[n])
            else:
                feed[sid[n]] = frames[n][pos[n]]
                pos[n] += 1
                where_k[sid[n]] = "%s, k = %d" % (n, ref.k_of(sid[n]))
        got, want = on.step(feed), ref.step(feed)
        for s, f in feed.items():
            first = got[s][0] if isinstance(got[s], tuple) else got[s]
            assert isinstance(first, torch.Tensor) == isinstance(f, torch.Tensor), \
                "step %d: NumPy in, NumPy out; device in, device out" % t
        _same_outputs(got, want, "%s step %d" % (sched.name, t))
    assert on.open_streams == ref.open_streams and len(ref.open_streams) == 3
    for s in ref.open_streams:
        if ref.crop is not None:
            g, w_ = on.crop_state(s), ref.crop_state(s)
            assert g["zoom"].dtype == np.float32 and g["zoom"].tobytes() == w_["zoom"].tobytes() and g["free"] == w_["free"], \
                "crop_state of stream %d: %s, the model's %s" % (s, g, w_)
        if ref.scene_thr is not None:
            assert on.scene_state(s) == ref.scene_state(s), "scene_state of stream %d" % s
    if ref.scene_thr is not None:
        planted = [(t, sid[n]) for t, n in om.coverage(sched)["cuts"]]
        assert sorted(ref.cut_log) == sorted(planted), "the model cut at %s, planted were %s" % (ref.cut_log, planted)
    for s in list(on.open_streams):
        on.close(s)
    assert not on._keep, "a closed stream keeps no surface"


def _both(weights, kw, precision="f32"):
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = _model(weights, precision)
    return OnlineStabilizer(model, max_streams=om.MAX_STREAMS, **kw), om.UnboundedStreams(model, max_streams=om.MAX_STREAMS, **kw)


SCENE = dict(scene_cut=om.THRESHOLD, scene_min_len=om.MIN_LEN)


@pytest.mark.parametrize("form", ["plain-f32", "plain-f16", "side_u8_bgr"])
def test_rgb_model_size(synthetic_weights, form):
    """Resized uint8 of two sizes, same-size uint8, float32 and float64 frames; the host counts the steps (no scene_cut)."""
    kw = dict(as_uint8=False) if form.startswith("plain") else dict(side_by_side=True, as_uint8=True, channel_order="bgr")
    _run(om.make_schedule("rgb"), *_both(synthetic_weights, kw, "f16" if form == "plain-f16" else "f32"))


@pytest.mark.parametrize("form", ["keep_f32", "mirror_side_u8"])
def test_source_res_all_options(synthetic_weights, form):
    kw = dict(source_res=True, crop="auto", render_filter="bicubic", strength=0.8, rigidity=0.5, shape_model="similarity", **SCENE)
    kw.update(dict(border="keep") if form == "keep_f32" else dict(border="mirror", as_uint8=True, side_by_side=True))
    _run(om.make_schedule("source_res"), *_both(synthetic_weights, kw))


def test_nv12_all_options(synthetic_weights):
    """NV12 of two sizes, bilinear; stream a arrives as host arrays, the others as device tensors."""
    _run(om.make_schedule("nv12"), *_both(synthetic_weights, dict(frame_format="nv12", crop="auto", border="keep", **SCENE)))


@pytest.mark.parametrize("form", ["keep_bilinear", "mirror_bicubic_shaped"])
def test_p010_all_options(synthetic_weights, form):
    """P010 of two sizes; the streams arrive as host uint16, host uint8, device uint16 (where torch has it) and device uint8
    and leave in the form they came in.  One of the two sizes is fed alone for a step and comes back (the per-size high-byte
    buffers are dropped and made again); two streams of one size share a launch; keep_bilinear is the render form
    tests/test_gpu_p010.py::test_bilinear_borders_are_the_reference pins."""
    kw = dict(frame_format="p010", crop="auto", **SCENE)
    kw.update(dict(border="keep") if form == "keep_bilinear" else
              dict(render_filter="bicubic", border="mirror", strength=0.8, rigidity=0.5, shape_model="similarity"))
    _run(om.make_schedule("p010"), *_both(synthetic_weights, kw))


def test_model_size_crop_and_cuts(synthetic_weights):
    _run(om.make_schedule("model_size"), *_both(synthetic_weights, dict(crop="auto", crop_recover=0.01, **SCENE)))


def test_stabilize_clips(synthetic_weights):
    """Five clips of 1, 9, 40, 75 and 20 frames through two rings, against the model fed clip by clip in the same lockstep."""
    from coupe.dvsg_amd.online import stabilize_clips
    model = _model(synthetic_weights)
    clips = [inputs.smooth_frames(5300 + i, n, H, W) for i, n in enumerate((1, 9, 40, 75, 20))]
    got = stabilize_clips(model, clips, batch=2)
    want = om.run_clips(om.UnboundedStreams(model, max_streams=2), clips, 2)
    for c, (g, w_) in enumerate(zip(got, want)):
        assert g.shape == (len(w_), H, W, 3)
        for k in range(len(w_)):
            assert np.array_equal(g[k], w_[k]), "clip %d, frame %d: %d values differ" % (c, k, int((g[k] != w_[k]).sum()))


def test_stabilize_clips_p010(synthetic_weights):
    """Three P010 clips of 1, 9 and 40 frames (two sizes) through two rings, one given as uint16 words and two as uint8
    bytes, against the model fed clip by clip in the same lockstep: frame by frame, dtype by dtype."""
    from coupe.dvsg_amd.online import stabilize_clips
    model = _model(synthetic_weights)
    specs = [dict(kind=k, seed=5500 + i, n=n, scenes=[0] * n, form=f)
             for i, (k, n, f) in enumerate((("pa", 1, "host_u8"), ("pb", 9, "host_u16"), ("pa", 40, "host_u8")))]
    clips = [om.stream_frames(s) for s in specs]
    assert [c.dtype for c in clips] == [np.uint8, np.uint16, np.uint8]
    kw = dict(frame_format="p010", crop="auto", border="keep")
    got = stabilize_clips(model, clips, batch=2, **kw)
    want = om.run_clips(om.UnboundedStreams(model, max_streams=2, **kw), clips, 2)
    for c, (g, w_) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == clips[c].dtype and g.shape == clips[c].shape, "clip %d" % c
        assert not np.array_equal(g, clips[c])
        for k in range(len(w_)):
            assert w_[k].dtype == g.dtype and np.array_equal(g[k], w_[k]), "clip %d, frame %d: %d values differ" % (
                c, k, int((g[k] != w_[k]).sum()))


@pytest.mark.parametrize("precision", ["f32", "f16", "f32s", "f32x3"])
def test_batch_rows_permute(synthetic_weights, precision):
    """Three different windows at 32 x 48, then the same windows with the rows permuted: the permuted outputs, bit for bit."""
    import torch
    from coupe.dvsg_amd.networks import LocNet
    net = LocNet(synthetic_weights)
    x = torch.from_numpy(inputs.window_frames(5401, 3, H, W)).cuda()
    perm = [2, 0, 1]

    def run(x):
        u = x[..., 18:].contiguous()
        out, F = torch.empty((3, H, W, 3), device="cuda"), torch.empty((3, 25, 2), device="cuda")
        net.stabilize(x, u, out, F, precision=precision)
        torch.cuda.synchronize()
        return out, F
    out, F = run(x)
    pout, pF = run(x[perm].contiguous())
    assert torch.equal(pF, F[perm]), "F_t: max diff %g" % float((pF - F[perm]).abs().max())
    assert torch.equal(pout, out[perm]), "s_t_pred: max diff %g" % float((pout - out[perm]).abs().max())
