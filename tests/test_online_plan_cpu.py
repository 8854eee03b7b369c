"""No-GPU checks of `coupe.dvsg_amd.online.plan_step`: what a step of OnlineStabilizer decides before its first launch --
the batch order, the runs of one ingest and one render launch each, every refusal with its type and text, and the word
form of P010 frames -- on CPU tensors and NumPy arrays.  The expected messages are written out here, not taken from the
module, so that a reworded refusal fails."""
import re

import numpy as np
import pytest
import torch

from coupe.dvsg_amd.online import Row, plan_step

H, W = 32, 48


def _streams(sids):
    """sid -> [ring, count] as OnlineStabilizer keeps it, and the look-up plan_step is given"""
    table = {sid: [ring, 10 * ring + 3] for ring, sid in enumerate(sids)}
    return table, table.__getitem__


def _u8(h, w):
    return np.zeros((h, w, 3), dtype=np.uint8)


def _mixed_feed():
    """Two resized uint8 sizes, same-size uint8, float32 and float64 in an order that is not the batch order; two streams
    each of (45, 70) and of float32, so that equal keys have a feed order to keep; NumPy and tensors mixed."""
    return {
        "f64": np.zeros((H, W, 3), dtype=np.float64),
        "f32_a": torch.zeros((H, W, 3), dtype=torch.float32),
        "big_a": _u8(45, 70),
        "same": torch.zeros((H, W, 3), dtype=torch.uint8),
        "small": _u8(40, 64),
        "f32_b": np.zeros((H, W, 3), dtype=np.float32),
        "big_b": torch.zeros((45, 70, 3), dtype=torch.uint8),
    }


def test_batch_order_rgb():
    feed = _mixed_feed()
    table, stream_of = _streams(list(feed))
    rows, runs = plan_step(feed, stream_of, H, W)
    assert [r.sid for r in rows] == ["small", "big_a", "big_b", "same", "f32_a", "f32_b", "f64"]
    assert [r.key for r in rows] == [(0, 40, 64), (0, 45, 70), (0, 45, 70), (1,), (2,), (2,), (3,)]
    assert runs == [(0, 1), (1, 3), (3, 4), (4, 6), (6, 7)]
    for r in rows:
        assert isinstance(r, Row) and isinstance(r.t, torch.Tensor)
        assert [r.ring, r.k] == table[r.sid] and r.words is False
        assert r.host == isinstance(feed[r.sid], np.ndarray)
        assert tuple(r.t.shape) == tuple(feed[r.sid].shape)
    assert rows[0].t.dtype == torch.uint8 and rows[4].t.dtype == torch.float32 and rows[6].t.dtype == torch.float64


def test_equal_keys_keep_feed_order():
    for order in (["p", "q", "r"], ["r", "q", "p"], ["q", "r", "p"]):
        feed = {sid: _u8(45, 70) for sid in order}
        rows, runs = plan_step(feed, _streams(order)[1], H, W, source_res=True)
        assert [r.sid for r in rows] == order and runs == [(0, 3)]


def _check_partition(rows, runs):
    assert runs[0][0] == 0 and runs[-1][1] == len(rows)
    for (i, j), nxt in zip(runs, runs[1:] + [None]):
        assert i < j and len(set(r.key for r in rows[i:j])) == 1
        if nxt is not None:
            assert nxt[0] == j and rows[j].key != rows[i].key     # maximal
    assert [r.key for r in rows] == sorted(r.key for r in rows)


def test_runs_partition_the_batch():
    feed = _mixed_feed()
    rows, runs = plan_step(feed, _streams(list(feed))[1], H, W)
    _check_partition(rows, runs)
    one = {"a": _u8(H, W)}
    assert plan_step(one, _streams(["a"])[1], H, W)[1] == [(0, 1)]
    # surfaces of two sizes, interleaved: NV12 [3 H0 / 2, W0], P010 uint8 [3 H0 / 2, 2 W0]
    for fmt, bps in (("nv12", 1), ("p010", 2)):
        sizes = {"a": (40, 48), "b": (36, 64), "c": (40, 48), "d": (36, 64), "e": (36, 64)}
        feed = {sid: np.zeros((3 * h0 // 2, bps * w0), dtype=np.uint8) for sid, (h0, w0) in sizes.items()}
        rows, runs = plan_step(feed, _streams(list(feed))[1], H, W, frame_format=fmt, source_res=True)
        _check_partition(rows, runs)
        assert [r.sid for r in rows] == ["b", "d", "e", "a", "c"] and runs == [(0, 3), (3, 5)]
        assert [r.key for r in rows] == [(36, 64)] * 3 + [(40, 48)] * 2


REFUSALS = [
    ("rank", {}, np.zeros((H, W), dtype=np.uint8), ValueError, "stream 'bad': a frame must be [h,w,3], got (32, 48)"),
    ("channels", {}, np.zeros((H, W, 4), dtype=np.uint8), ValueError, "stream 'bad': a frame must be [h,w,3], got (32, 48, 4)"),
    ("float_source_res", dict(source_res=True), np.zeros((H, W, 3), dtype=np.float32), ValueError,
     "stream 'bad': source_res renders the uint8 source frame; a float frame has no source beyond the model's size"),
    ("float_other_size", {}, np.zeros((45, 70, 3), dtype=np.float32), ValueError,
     "stream 'bad': float frames must already be [32,48,3] (StabNet(h, w) fixes the STN out_size), got (45, 70, 3)"),
    ("int32", {}, np.zeros((H, W, 3), dtype=np.int32), TypeError,
     "stream 'bad': frames must be uint8 or floating point, got torch.int32"),
    ("crop_grid", dict(source_res=True, crop=True), _u8(1, 70), ValueError,
     "a crop needs an output grid of at least 2 x 2, got 1 x 70"),
    # H0 = 41: 3 H0 / 2 rounds down to 61 rows
    ("nv12_odd_h0", dict(frame_format="nv12", source_res=True), np.zeros((61, 48), dtype=np.uint8), ValueError,
     "stream 'bad': an NV12 frame [3*H0/2, W0] needs even H0, W0 >= 4 (odd sizes have no chroma layout), got (61, 48)"),
    ("nv12_rank", dict(frame_format="nv12", source_res=True), _u8(60, 48), ValueError,
     "stream 'bad': an NV12 frame must be [3*H0/2, W0], got (60, 48, 3)"),
    ("nv12_int32", dict(frame_format="nv12", source_res=True), np.zeros((60, 48), dtype=np.int32), TypeError,
     "stream 'bad': NV12 frames must be uint8, got torch.int32"),
    ("nv12_float", dict(frame_format="nv12", source_res=True), np.zeros((60, 48), dtype=np.float32), ValueError,
     "stream 'bad': frame_format='nv12' takes uint8 surfaces, not float frames (torch.float32)"),
    ("p010_odd_bytes", dict(frame_format="p010", source_res=True), np.zeros((60, 97), dtype=np.uint8), ValueError,
     "stream 'bad': a P010 uint8 frame [3*H0/2, 2*W0] needs even H0, W0 >= 4 (odd sizes have no chroma layout), got (60, 97)"),
    ("p010_int32", dict(frame_format="p010", source_res=True), np.zeros((60, 96), dtype=np.int32), TypeError,
     "stream 'bad': P010 frames must be uint8 or uint16, got torch.int32"),
    ("p010_rank", dict(frame_format="p010", source_res=True), np.zeros((2, 60, 96), dtype=np.uint8), ValueError,
     "stream 'bad': a P010 frame must be [3*H0/2, 2*W0], got (2, 60, 96)"),
]


@pytest.mark.parametrize("name,options,frame,exc,message", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "tensor"])
def test_refusals(name, options, frame, exc, message, as_tensor):
    frame = torch.from_numpy(frame) if as_tensor else frame
    with pytest.raises(exc, match="^" + re.escape(message) + "$"):
        plan_step({"bad": frame}, _streams(["bad"])[1], H, W, **options)


def test_a_closed_stream_is_refused_by_the_look_up():
    def stream_of(sid):
        raise ValueError("stream %d is closed" % sid)
    with pytest.raises(ValueError, match="^stream 4 is closed$"):
        plan_step({4: _u8(H, W)}, stream_of, H, W)


@pytest.mark.parametrize("options,good,bad", [
    ({}, _u8(45, 70), np.zeros((H, W, 3), dtype=np.int32)),
    (dict(frame_format="nv12", source_res=True), np.zeros((60, 48), dtype=np.uint8), np.zeros((61, 48), dtype=np.uint8)),
    (dict(frame_format="p010", source_res=True), np.zeros((60, 48), dtype=np.uint16), np.zeros((60, 97), dtype=np.uint8)),
], ids=["rgb", "nv12", "p010"])
def test_a_refused_feed_has_no_effect(options, good, bad):
    feed = {"first": good, "middle": torch.from_numpy(good.view(np.uint8).copy()), "last": bad}
    table, stream_of = _streams(list(feed))
    before_table = {sid: list(st) for sid, st in table.items()}
    before_feed = {sid: (id(fr), fr.dtype, tuple(fr.shape)) for sid, fr in feed.items()}
    result = None
    with pytest.raises((ValueError, TypeError)):
        result = plan_step(feed, stream_of, H, W, **options)
    assert result is None
    assert table == before_table and list(feed) == ["first", "middle", "last"]
    assert {sid: (id(fr), fr.dtype, tuple(fr.shape)) for sid, fr in feed.items()} == before_feed
    assert not good.any() and not bad.any() and good.flags.writeable


def test_p010_word_flag():
    h0, w0 = 40, 48
    words = (np.arange(3 * h0 // 2 * w0, dtype=np.uint32) * 64 % 65536).astype(np.uint16).reshape(3 * h0 // 2, w0)
    as_bytes = words.view(np.uint8)
    feed = {"w": words, "b": as_bytes, "t": torch.from_numpy(as_bytes.copy())}
    rows, runs = plan_step(feed, _streams(list(feed))[1], H, W, frame_format="p010", source_res=True)
    assert [r.sid for r in rows] == ["w", "b", "t"] and runs == [(0, 3)]
    assert [r.words for r in rows] == [True, False, False] and [r.host for r in rows] == [True, True, False]
    for r in rows:
        assert r.key == (h0, w0) and r.t.dtype == torch.uint8 and tuple(r.t.shape) == (3 * h0 // 2, 2 * w0)
        assert np.array_equal(r.t.numpy(), as_bytes)              # the words' bytes, low byte first
    assert words.dtype == np.uint16 and words.shape == (3 * h0 // 2, w0)
    u16 = getattr(torch, "uint16", None)
    if u16 is not None:                                           # the same words as a tensor, where this torch has them
        (r,), _ = plan_step({"w": torch.from_numpy(as_bytes.copy()).view(u16)}, _streams(["w"])[1], H, W,
                            frame_format="p010", source_res=True)
        assert r.words is True and r.host is False and r.t.dtype == torch.uint8 and np.array_equal(r.t.numpy(), as_bytes)
    # an NV12 stream has no word form: uint16 is refused, not reinterpreted
    with pytest.raises(TypeError, match="NV12 frames must be uint8, got"):
        plan_step({"w": torch.zeros((60, 48), dtype=torch.int16)}, _streams(["w"])[1], H, W, frame_format="nv12", source_res=True)
