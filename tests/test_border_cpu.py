"""No-GPU checks of the border modes of the source-size renders (include/dvsg_amd.h, "Border modes"): the two entry
points' declarations, bindings and argument checks (decided before the handle is read), the Python options, the front
end's flag, and the properties of the rule itself on its NumPy restatement tests/border_ref.py, in float64 and float32."""
import ctypes
import os
import re

import numpy as np
import pytest

import bicubic_ref as R
import border_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvsg_amd.h")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def test_border_calls_are_declared_exported_and_bound(lib):
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import RENDER_BORDERS, RENDER_FILTERS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+dvsg_locnet_view_create_border\(const dvsg_locnet_t \*net, int render_filter, int render_border, "
                     r"dvsg_locnet_t \*\*view\);", text)
    assert re.search(r"int\s+dvsg_locnet_render_border\(const dvsg_locnet_t \*net\);", text)
    for name, value in (("BLACK", 0), ("REPLICATE", 1), ("MIRROR", 2), ("KEEP", 3)):
        assert re.search(r"#define\s+DVSG_BORDER_%s\s+%d\b" % (name, value), text), name
    for name in ("dvsg_locnet_view_create_border", "dvsg_locnet_render_border"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert "stream" not in re.search(r"int\s+%s\(([^)]*)\)" % name, text).group(1)
    assert RENDER_BORDERS == {"black": 0, "replicate": 1, "mirror": 2, "keep": 3}
    assert RENDER_BORDERS == BR.BORDERS
    assert RENDER_FILTERS == {"bilinear": 0, "bicubic": 1}
    assert lib.dvsg_abi_version() == 1


def test_view_create_border_rejects_bad_arguments_before_the_handle_is_read(lib):
    view = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)      # never dereferenced: every call below is refused first
    assert lib.dvsg_locnet_view_create_border(None, 1, 1, ctypes.byref(view)) == -1
    assert b"dvsg_locnet_view_create_border: NULL net" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create_border(fake, 2, 1, ctypes.byref(view)) == -1
    assert b"render_filter=2" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create_border(fake, 1, 4, ctypes.byref(view)) == -1
    assert b"render_border=4" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create_border(fake, 0, -1, ctypes.byref(view)) == -1
    assert b"render_border=-1" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create_border(fake, 1, 1, None) == -1
    assert b"NULL view" in lib.dvsg_last_error_string()
    assert not view.value
    assert lib.dvsg_locnet_render_border(None) == 0
    # the old constructor keeps its own name in its messages
    assert lib.dvsg_locnet_view_create(fake, 2, ctypes.byref(view)) == -1
    assert b"dvsg_locnet_view_create: render_filter=2" in lib.dvsg_last_error_string()
    assert lib.dvsg_abi_version() == 1


def test_python_options_raise_value_errors_without_a_device():
    from coupe.dvsg_amd.clip import render_source_into, stabilize_clip
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.networks import check_border
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = StabNet(32, 48)
    frames = np.zeros((2, 32, 48, 3), np.uint8)
    for border in ("replicate", "mirror", "keep"):
        # no source-size render: RGB at the model's size, float frames
        with pytest.raises(ValueError, match="source_res"):
            OnlineStabilizer(model, border=border)
        with pytest.raises(ValueError, match="source_res"):
            OnlineStabilizer(model, border=border, crop="auto", as_uint8=True)
        with pytest.raises(ValueError, match="source_res"):
            stabilize_clip(model, None, frames, border=border)
        with pytest.raises(ValueError, match="source_res"):
            check_border(border, False)
        assert check_border(border, True) == border
    assert check_border("black", False) == "black"
    for bad in ("clamp", "", None, 1, b"mirror"):
        with pytest.raises(ValueError, match="border"):
            OnlineStabilizer(model, source_res=True, border=bad)
        with pytest.raises(ValueError, match="border"):
            stabilize_clip(model, None, frames, source_res=True, border=bad)
    with pytest.raises(ValueError, match="border"):
        OnlineStabilizer(model, frame_format="nv12", border="wrap")
    # "keep": no side_by_side layout, and stabilize_clip's batched renders do not run one frame at a time
    with pytest.raises(ValueError, match="side_by_side"):
        OnlineStabilizer(model, source_res=True, side_by_side=True, border="keep")
    with pytest.raises(ValueError, match="border"):
        stabilize_clip(model, None, frames, source_res=True, border="keep")
    with pytest.raises(ValueError, match="border"):
        render_source_into(model, None, None, None, 0, None, side=object(), border="keep")


def test_pipe_command_line_takes_the_flag():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "--border" in out.stdout
    for name in ("black", "replicate", "mirror", "keep"):
        assert name in out.stdout
    bad = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--border", "wrap"], cwd=ROOT, capture_output=True,
                         text=True)
    assert bad.returncode != 0 and "--border" in bad.stderr


# ---------------------------------------------------------------------------------------------------------------------
# the rule's own properties.  x_s, y_s are built so that sampler A's x, y take chosen values: x_s = 2 x / pw - 1.
# ---------------------------------------------------------------------------------------------------------------------
PH, PW = 9, 13


def _plane(C=3, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (PH, PW, C), dtype=np.uint8)


def _norm(x, n):
    return (2.0 * np.asarray(x, np.float64) / n - 1.0).astype(f32)


def _line(axis, at, other):
    """x_s, y_s [1, n] of samples at `at` along `axis` (0: x, 1: y), the other coordinate fixed at `other`"""
    at = np.asarray(at, np.float64)[None]
    o = np.full_like(at, other)
    return (_norm(at, PW), _norm(o, PH)) if axis == 0 else (_norm(o, PW), _norm(at, PH))


@pytest.mark.parametrize("dtype", [np.float64, f32])
@pytest.mark.parametrize("bicubic", [False, True])
@pytest.mark.parametrize("border", ["replicate", "mirror"])
def test_continuous_across_the_valid_invalid_boundary_on_all_four_sides(border, bicubic, dtype):
    """Just inside and just outside each of the four edges of the valid set (x = 0, x = pw - 1, y = 0, y = ph - 1) the sample
    differs by no more than the step times the filter's largest slope (the kernels' derivatives are below 2 per pixel and
    samples lie in [0, 1]), plus the coordinate's own float32 rounding.  The black border jumps by the sample itself."""
    plane = _plane()
    eps = 1e-3
    for axis, n in ((0, PW), (1, PH)):
        for edge in (0.0, float(n - 1)):
            at = np.array([edge - eps, edge + eps])
            for other in (2.3, 5.0):
                x_s, y_s = _line(axis, at, other)
                ok = R.valid(PH, PW, x_s, y_s)[0]
                assert ok[0] != ok[1], "one sample on each side of the boundary"
                v, _ = BR.render(plane, x_s, y_s, border, bicubic, dtype=dtype)
                jump = np.abs(v[0, 0].astype(np.float64) - v[0, 1].astype(np.float64)).max()
                assert jump <= 4 * 2 * eps + 1e-5, (axis, edge, other, jump)
    x_s, y_s = _line(0, np.array([-eps, eps]), 2.3)
    b = BR.black(plane, x_s, y_s, bicubic)
    assert np.abs(b[0, 0] - b[0, 1]).max() > 0.01


@pytest.mark.parametrize("dtype", [np.float64, f32])
@pytest.mark.parametrize("bicubic", [False, True])
def test_mirror_reflects_about_the_edge(bicubic, dtype):
    """MIRROR at x = -k is the sample at x = +k (and at x = m + k the sample at m - k), for y as well: exactly, where k and
    the coordinates are exact in float32"""
    plane = _plane(C=2, seed=8)
    k = np.array([0.5, 1.25, 3.0])
    for axis, n in ((0, PW), (1, PH)):
        m = n - 1.0
        for outside, inside in ((-k, k), (m + k, m - k)):
            a, _ = BR.render(plane, *_line(axis, outside, 4.5), "mirror", bicubic, True, dtype=dtype)
            b, _ = BR.render(plane, *_line(axis, inside, 4.5), "mirror", bicubic, True, dtype=dtype)
            # _norm rounds x_s once; sampler A's x comes back within an ulp of the intended value on both sides
            assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= 1e-5, (axis, outside)
    # one reflection only: beyond it the coordinate clamps to the far edge
    far, _ = BR.render(plane, *_line(0, np.array([-40.0]), 4.5), "mirror", bicubic, True, dtype=dtype)
    edge, _ = BR.render(plane, *_line(0, np.array([PW - 1.0]), 4.5), "replicate", bicubic, True, dtype=dtype)
    assert np.array_equal(far, edge)
    assert np.array_equal(BR.move(f32([-2.5, 14.5, 3.0]), PW, "mirror"), f32([2.5, 9.5, 3.0]))
    assert np.array_equal(BR.move(f32([-2.5, 14.5, 3.0]), PW, "replicate"), f32([0.0, 12.0, 3.0]))


@pytest.mark.parametrize("dtype", [np.float64, f32])
@pytest.mark.parametrize("bicubic", [False, True])
@pytest.mark.parametrize("border", ["replicate", "mirror"])
def test_a_flat_plane_stays_flat(border, bicubic, dtype):
    """Every sample of a constant plane, valid or not, is the constant up to the rounding of weights that sum to 1 (a few
    ulp); the bicubic render's bytes, which round to nearest, are the constant itself.  (The bilinear render truncates, so a
    blend one ulp short of b / 255 gives b - 1 inside the frame as well: the border mode adds nothing to that.)"""
    rng = np.random.default_rng(5)
    x_s = rng.uniform(-1.6, 1.6, (40, 50)).astype(f32)
    y_s = rng.uniform(-1.6, 1.6, (40, 50)).astype(f32)
    ok = R.valid(PH, PW, x_s, y_s)
    assert ok.any() and (~ok).any()
    for byte in (1, 77, 200, 255):
        for chroma, C in ((False, 3), (True, 2)):
            plane = np.full((PH, PW, C), byte, np.uint8)
            v, written = BR.render(plane, x_s, y_s, border, bicubic, chroma, dtype=dtype)
            s = (byte - 128 if chroma else byte) / 255.0
            assert written.all()
            assert np.abs(v.astype(np.float64) - s).max() <= (16 * np.finfo(dtype).eps)
            if bicubic and dtype is f32:
                assert (BR.to_u8(v, True, chroma) == byte).all()


def test_valid_samples_are_the_black_renders_and_planes_of_one_row_fill_from_it():
    rng = np.random.default_rng(6)
    plane = _plane()
    x_s = rng.uniform(-1.5, 1.5, (30, 40)).astype(f32)
    y_s = rng.uniform(-1.5, 1.5, (30, 40)).astype(f32)
    x_s[0, :3] = np.nan
    ok = R.valid(PH, PW, x_s, y_s)
    for bicubic in (False, True):
        b = BR.black(plane, x_s, y_s, bicubic)
        for border in ("replicate", "mirror"):
            v, _ = BR.render(plane, x_s, y_s, border, bicubic)
            assert np.array_equal(v[ok].view(np.uint32), b[ok].view(np.uint32))
            assert (v[0, :3] == 0).all(), "a NaN coordinate gives the black value"
        k, written = BR.render(plane, x_s, y_s, "keep", bicubic)
        assert np.array_equal(written, ok) and np.array_equal(k.view(np.uint32), b.view(np.uint32))
        # ph == 1: no sample is valid; every sample is filled from the single row
        row = _plane()[:1]
        v, _ = BR.render(row, x_s, y_s, "replicate", bicubic)
        flat = np.repeat(row, 3, axis=0)
        w, _ = BR.render(flat, x_s, np.zeros_like(y_s), "replicate", bicubic)
        assert not R.valid(1, PW, x_s, y_s).any()
        assert np.abs(v - w)[~np.isnan(x_s)].max() <= 1e-6
