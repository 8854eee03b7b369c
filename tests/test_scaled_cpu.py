"""No-GPU checks of the render at a delivery size (include/dvsg_amd.h, "Output size"): the factors, the Python option
checks, the pipe's arguments and Y4M `A` tag, the two host-side entry points' argument checks, and -- on the NumPy
restatement tests/scaled_ref.py alone -- the property the feature exists for: the area filter does not alias where the
point-sampled render does."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_ref as B   # noqa: E402
import scaled_ref as S   # noqa: E402

f32 = np.float32


# ---- 1. the factors
@pytest.mark.parametrize("src, out, want", [((24, 40), (12, 20), (2, 2)), ((26, 44), (12, 20), (3, 3)),
                                            ((24, 40), (24, 10), (1, 4)), ((24, 40), (36, 60), (1, 1))])
def test_scaled_factors(src, out, want):
    from coupe.dvsg_amd.networks import scaled_factors
    assert scaled_factors(src, out) == want
    assert S.factors(src, out) == want


def test_scaled_factors_refuse_more_than_four():
    from coupe.dvsg_amd.networks import scaled_factors
    with pytest.raises(ValueError, match="4x"):
        scaled_factors((24, 40), (4, 8))
    with pytest.raises(ValueError, match="positive"):
        scaled_factors((24, 40), (0, 8))


# ---- 2. the option checks
def test_check_out_size_refusals():
    from coupe.dvsg_amd.networks import check_out_size
    assert check_out_size(None) is None and check_out_size(None, False) is None
    assert check_out_size((12, 20)) == (12, 20) and check_out_size([np.int64(7), 9]) == (7, 9)
    for bad in ((12,), (12, 20, 3), 12, "12x20", (12.0, 20), (0, 20), (12, -1), (True, 20)):
        with pytest.raises(ValueError, match="out_size"):
            check_out_size(bad)
    with pytest.raises(ValueError, match="source_res"):
        check_out_size((12, 20), source_size_render=False)
    for odd in ((13, 20), (12, 21), (2, 20)):
        with pytest.raises(ValueError, match="even"):
            check_out_size(odd, True, surface=True)
    assert check_out_size((13, 21), True, surface=False) == (13, 21)


def test_online_options_raise_before_the_device():
    """A StabNet without weights needs no device: the out_size conflicts are named before anything else happens."""
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = StabNet(32, 48)
    for kw, name in [(dict(), "source_res"), (dict(source_res=True, border="keep"), "keep"),
                     (dict(source_res=True, side_by_side=True), "side_by_side"),
                     (dict(frame_format="nv12", border="keep"), "keep")]:
        with pytest.raises(ValueError, match=name):
            OnlineStabilizer(model, out_size=(12, 20), **kw)
    for fmt in ("nv12", "p010"):
        with pytest.raises(ValueError, match="even"):
            OnlineStabilizer(model, frame_format=fmt, out_size=(13, 20))


def test_plan_step_refuses_a_frame_minified_more_than_four_times():
    import torch
    from coupe.dvsg_amd.online import plan_step
    stream_of = lambda sid: (0, 0)   # noqa: E731
    ok = torch.zeros((24, 40, 3), dtype=torch.uint8)
    rows, runs = plan_step({0: ok}, stream_of, 8, 8, "rgb", True, False, (12, 20))
    assert len(rows) == 1 and runs == [(0, 1)]
    with pytest.raises(ValueError, match="stream 0.*4x"):
        plan_step({0: ok}, stream_of, 8, 8, "rgb", True, False, (4, 20))
    nv12 = torch.zeros((36, 40), dtype=torch.uint8)
    with pytest.raises(ValueError, match="4x"):
        plan_step({0: nv12}, stream_of, 8, 8, "nv12", True, False, (12, 8))
    assert plan_step({0: nv12}, stream_of, 8, 8, "nv12", True, False, (12, 10))[1] == [(0, 1)]


# ---- 3. the pipe's arguments
def test_pipe_arguments():
    from coupe.dvsg_amd import pipe
    args = pipe._arguments(["--synthetic-weights", "--out-size", "640x360"])
    assert args.out_size == (360, 640)
    assert pipe._arguments(["--synthetic-weights"]).out_size is None
    with pytest.raises(pipe._UsageError, match="WxH"):
        pipe._arguments(["--synthetic-weights", "--out-size", "640"])
    with pytest.raises(pipe._UsageError, match="keep"):
        pipe._arguments(["--synthetic-weights", "--out-size", "640x360", "--border", "keep"])
    with pytest.raises(pipe._UsageError, match="even"):
        pipe._arguments(["--synthetic-weights", "--out-size", "641x360"])


# ---- 4. the A tag of the pipe's Y4M header
def test_y4m_header_carries_the_size_and_the_aspect_rule():
    import io
    from coupe.dvsg_amd import pipe, y4m
    assert pipe.output_aspect((1, 1), (1080, 1920), (360, 640)) == (1, 1)      # 640 * 1080 == 360 * 1920
    assert pipe.output_aspect((4, 3), (24, 40), (12, 20)) == (4, 3)
    assert pipe.output_aspect((1, 1), (1080, 1920), (360, 600)) == (0, 0)
    assert pipe.output_aspect(None, (24, 40), (12, 20)) is None
    assert pipe.output_aspect(None, (24, 40), (12, 22)) == (0, 0)
    for out, tag in (((12, 20), b"A1:1"), ((12, 22), b"A0:0")):
        f = io.BytesIO()
        w = y4m.Y4MWriter(f, out[1], out[0], (25, 1), aspect=pipe.output_aspect((1, 1), (24, 40), out))
        w.write(np.zeros((3 * out[0] // 2, out[1]), np.uint8))
        head = f.getvalue().split(b"\n")[0].split(b" ")
        assert head[0] == b"YUV4MPEG2" and b"W%d" % out[1] in head and b"H%d" % out[0] in head and tag in head


def test_stabilize_pipes_checks_the_sinks_against_out_size():
    """_check_ends alone: a sink that states a size states out_size's"""
    from coupe.dvsg_amd import pipe

    class End(object):
        layout = "nv12"

        def __init__(self, w, h):
            self.width, self.height, self.frame_shape = w, h, (3 * h // 2, w)
    assert pipe._check_ends([End(40, 24)], [End(20, 12)], (12, 20)) == 8
    with pytest.raises(ValueError, match="out_size"):
        pipe._check_ends([End(40, 24)], [End(40, 24)], (12, 20))
    with pytest.raises(ValueError, match="size of the input"):
        pipe._check_ends([End(40, 24)], [End(20, 12)])


# ---- the two host-side entry points: no device work, pointers never dereferenced
def test_view_create_scaled_rejects_bad_arguments_without_a_handle():
    from coupe.dvsg_amd import _lib
    lib = _lib.load()
    v = ctypes.c_void_p()
    assert lib.dvsg_locnet_view_create_scaled(None, 12, 20, ctypes.byref(v)) == -1
    assert b"NULL net" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create_scaled(8, 12, 20, None) == -1 and b"NULL view" in lib.dvsg_last_error_string()
    for oh, ow, word in ((0, 7, b"out_H=0"), (7, 0, b"out_W=0"), (-1, 4, b"out_H=-1"), (4, -2, b"out_W=-2")):
        assert lib.dvsg_locnet_view_create_scaled(8, oh, ow, ctypes.byref(v)) == -1
        assert word in lib.dvsg_last_error_string() and not v.value
    h, w = ctypes.c_int(5), ctypes.c_int(5)
    assert lib.dvsg_locnet_render_size(None, ctypes.byref(h), ctypes.byref(w)) == 0 and (h.value, w.value) == (0, 0)
    assert lib.dvsg_locnet_render_size(None, None, None) == 0


# ---- 5. the property: a 1-pixel checkerboard under the identity map
def _identity(gh, gw):
    """x_s, y_s of the identity map on a grid: tf.linspace(-1, 1, n) per axis"""
    return (np.broadcast_to(np.linspace(-1.0, 1.0, gw, dtype=f32)[None, :], (gh, gw)).copy(),
            np.broadcast_to(np.linspace(-1.0, 1.0, gh, dtype=f32)[:, None], (gh, gw)).copy())


@pytest.mark.parametrize("src, out", [((32, 48), (16, 24)), ((48, 96), (16, 32)), ((64, 64), (16, 16)), ((26, 44), (12, 20))])
def test_area_filter_does_not_alias_where_point_sampling_does(src, out):
    (H, W), (oh, ow) = src, out
    board = (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 255).astype(np.uint8)[..., None]
    sy, sx = S.factors(src, out)
    xs, ys = _identity(sy * oh, sx * ow)
    area_f32, area = S.render(board, xs, ys, sy, sx, "black", False)
    assert area_f32.dtype == f32 and area.shape == (oh, ow, 1) and area.dtype == np.uint8
    inner = area[1:-1, 1:-1]
    print("area interior %d..%d" % (inner.min(), inner.max()))
    assert inner.min() >= 112 and inner.max() <= 144
    xs1, ys1 = _identity(oh, ow)
    point = B.to_u8(B.render(board, xs1, ys1, "black", False)[0], False)[1:-1, 1:-1]
    print("point-sampled interior %d..%d" % (point.min(), point.max()))
    assert point.min() <= 40 and point.max() >= 200


def test_average_is_row_major_float32():
    """the order of the sum is visible in float32: three values whose sum depends on it"""
    v = np.array([[1.0, 2.0 ** -24], [2.0 ** -24, 2.0 ** -23]], f32)[..., None]
    got = S.average(v, 2, 2)[0, 0, 0]
    acc = f32(1.0)
    for t in (f32(2.0 ** -24), f32(2.0 ** -24), f32(2.0 ** -23)):
        acc = f32(acc + t)
    assert got == f32(acc / f32(4)) and got != f32((np.float64(1.0) + 2.0 ** -22) / 4)
