"""No-GPU checks of the bicubic render filter: the NumPy restatement (tests/bicubic_ref.py) against its own float64
evaluation, the byte rules, the argument checks of dvsg_locnet_view_create (decided before any device work), and the
Python options' ValueErrors.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import bicubic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvsg_amd.h")


@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def the_filter_exists():
    """bicubic_ref.py is the specification of a library feature: on a tree without it no test of this file has a subject."""
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import RENDER_FILTERS
    assert "dvsg_locnet_view_create" in _lib.SIGNATURES and "bicubic" in RENDER_FILTERS


def test_weights_at_zero_are_exact():
    """t = 0 is the identity: a frame rendered with F_t = 0 on integer coordinates takes the centre tap alone."""
    w = R.weights_f32(np.float32(0))
    assert w.dtype == np.float32 and w.tolist() == [0.0, 1.0, 0.0, 0.0]
    assert R.weights_f64(0.0).tolist() == [0.0, 1.0, 0.0, 0.0]


def test_float32_weights_against_float64():
    """10^5 t drawn from default_rng(20).random (float32, [0, 1)).  Worst |w_f32 - w_f64| seen: 1.2094e-06 (20.3 x 2^-24),
    in w0 and w3 -- their polynomial in u = t + 1 sums terms of size up to 6 to a result below 0.15 --; w1 and w2 stay
    within 1.53e-07.  w3 = ((1 - w0) - w1) - w2 is three float32 subtractions of partial results below 1.2, each rounded by
    at most 2^-24: the four float32 weights, summed exactly, are within 3 x 2^-24 of 1 (for every t drawn they ARE 1)."""
    t = np.random.default_rng(20).random(100000).astype(np.float32)
    w32, w64 = R.weights_f32(t), R.weights_f64(t)
    assert w32.dtype == np.float32
    err = np.abs(w32.astype(np.float64) - w64).max(axis=1)
    print("worst float32 weight error per tap:", err)
    assert err.max() <= 1.2095e-06
    assert max(err[1], err[2]) <= 1.53e-07
    assert np.abs(w64.sum(axis=0) - 1.0).max() <= 8 * 2.0 ** -52     # four float64 polynomials of magnitude <= 1
    assert np.abs(w32.astype(np.float64).sum(axis=0) - 1.0).max() <= 3 * 2.0 ** -24


def test_byte_rules_for_all_256_values():
    b = np.arange(256)
    luma, chroma = R.samples(b, False), R.samples(b, True)
    assert luma.dtype == np.float32 and chroma.dtype == np.float32
    # rule 4 is the bilinear path's sample: the float64 quotient rounded once
    assert np.array_equal(luma, (b.astype(np.float64) / 255.0).astype(np.float32))
    assert np.array_equal(chroma, ((b.astype(np.float64) - 128.0) / 255.0).astype(np.float32))
    # rule 6 takes every sample back to its byte, and saturates
    assert np.array_equal(R.to_u8(luma), b) and np.array_equal(R.to_u8(chroma, chroma=True), b)
    assert R.to_u8(np.float32([-0.2, -1e-3, 1.0019, 1.3, np.nan, np.inf, -np.inf])).tolist() == [0, 0, 255, 255, 0, 255, 0]
    assert R.to_u8(np.float32([-0.7, 0.7, np.nan]), chroma=True).tolist() == [0, 255, 0]
    # round to nearest, halves up (exact float32 inputs): 0.5 * 255 + 0.5 = 128.0, 0.25 -> 64.25, 0.75 -> 191.75
    assert R.to_u8(np.float32([0.5, 0.25, 0.75])).tolist() == [128, 64, 191]
    # an invalid sample is 0.0f: byte 0, chroma 128
    assert R.to_u8(np.float32(0)) == 0 and R.to_u8(np.float32(0), chroma=True) == 128


@pytest.mark.parametrize("chroma", [False, True])
def test_flat_planes_stay_flat_for_every_byte(chroma):
    """Why the bytes round to nearest: on a flat plane of byte k the blend is k / 255 only up to rounding, and truncation
    would return k - 1 at some phases.  Every byte, 64 random phases, every valid sample: exactly k."""
    rng = np.random.default_rng(3)
    ph, pw = 6, 7
    x_s = rng.uniform(-1.0, 0.7, (8, 8)).astype(np.float32)
    y_s = rng.uniform(-1.0, 0.6, (8, 8)).astype(np.float32)
    ok = R.valid(ph, pw, x_s, y_s)
    assert ok.sum() > 40
    for k in range(256):
        plane = np.full((ph, pw, 1), k, np.uint8)
        out = R.to_u8(R.render_f32(plane, x_s, y_s, chroma), chroma)[..., 0]
        assert np.all(out[ok] == k), k
        assert np.all(out[~ok] == (128 if chroma else 0))


def test_reference_float32_against_its_float64_evaluation():
    """The float32 restatement against the same formula in float64 on a random plane: the blend of 16 samples in [0, 1] with
    weights of magnitude <= 1 accumulates a few float32 roundings plus the weights' own error (above), so 1e-5 is
    generous by an order of magnitude and still far below half a byte step (2e-3)."""
    rng = np.random.default_rng(5)
    plane = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    x_s = rng.uniform(-1.1, 1.0, (16, 16)).astype(np.float32)
    y_s = rng.uniform(-1.1, 1.0, (16, 16)).astype(np.float32)
    a, b = R.render_f32(plane, x_s, y_s), R.render_f64(plane, x_s, y_s)
    ok = R.valid(9, 11, x_s, y_s)
    assert ok.any() and (~ok).any()
    assert np.all(a[~ok] == 0.0)
    # (the float64 side forms x in float64: where the float32 x rounded up onto an integer the two floors differ, and the
    # interpolant, continuous there, still agrees)
    assert np.abs(a.astype(np.float64) - b)[ok].max() < 1e-5


def test_edge_taps_replicate():
    """x0 = 0 and x0 = pw - 2 (and the same in y): the taps outside the plane are its edge samples."""
    plane = np.arange(5 * 6, dtype=np.uint8).reshape(5, 6, 1) * 8
    pad = np.pad(plane, ((1, 2), (1, 2), (0, 0)), mode="edge")
    ph, pw = 5, 6
    # sample centres shifted by (0.25, 0.5) in every cell of the valid range
    xx, yy = np.meshgrid(np.arange(pw - 1) + 0.25, np.arange(ph - 1) + 0.5)
    x_s = (2 * xx / pw - 1).astype(np.float32)
    y_s = (2 * yy / ph - 1).astype(np.float32)
    got = R.render_f64(plane, x_s, y_s)[..., 0]
    wx, wy = R.weights_f64(0.25), R.weights_f64(0.5)
    for i in range(ph - 1):
        for j in range(pw - 1):
            want = sum(wy[r] * wx[k] * pad[i + r, j + k, 0] / 255.0 for r in range(4) for k in range(4))
            assert abs(got[i, j] - want) < 1e-6, (i, j)


def sharpness_case():
    """The GPU test's input: a 24 x 96 luma plane with 0.5 + 0.4 sin(2 pi x / 6) in every row, and the map of a pure
    translation by 2.5 source pixels (all 25 control points displaced by 5 / 96 in x).  Returns plane, x_s, y_s (the
    analytic map: x_s = x_t + d) and the shifted signal at every output sample."""
    H, W = 24, 96
    sig = lambda x: 0.5 + 0.4 * np.sin(2 * np.pi * x / 6)
    plane = np.tile(np.floor(sig(np.arange(W)) * 255 + 0.5).astype(np.uint8)[None, :, None], (H, 1, 1))
    d = np.float32(2.5 * 2 / W)
    x_t = np.float32(-1) + np.float32(2) / np.float32(W - 1) * np.arange(W, dtype=np.float32)
    y_t = np.float32(-1) + np.float32(2) / np.float32(H - 1) * np.arange(H, dtype=np.float32)
    x_s, y_s = np.tile((x_t + d)[None], (H, 1)), np.tile(y_t[:, None], (1, W))
    return plane, x_s, y_s, sig, d


def test_bicubic_is_sharper_than_bilinear_on_the_references():
    """The inequality the GPU sharpness test asserts, on the two NumPy references alone (analytic map): mean absolute error
    against the analytically shifted signal over the valid samples 0.0066 (bicubic) against 0.0229 (bilinear); the
    fitted amplitude is 1.015 x (bicubic, a 1.5 % overshoot at this half-pixel phase) against 0.915 x (bilinear: 8.5 % lost)."""
    plane, x_s, y_s, sig, _ = sharpness_case()
    ok = R.valid(24, 96, x_s, y_s)
    x, _ = R.coords(24, 96, x_s, y_s)
    truth = sig(x.astype(np.float64))
    bc, bl = R.render_f32(plane, x_s, y_s)[..., 0], R.bilinear_f32(plane, x_s, y_s)[..., 0]
    e_bc, e_bl = np.abs(bc - truth)[ok].mean(), np.abs(bl - truth)[ok].mean()
    print("mean |error|: bicubic %.5f bilinear %.5f" % (e_bc, e_bl))
    assert ok.sum() > 2000
    assert e_bc < e_bl


def test_view_create_rejects_bad_arguments_before_any_device_work(lib):
    view = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)
    assert lib.dvsg_locnet_view_create(None, 1, ctypes.byref(view)) == -1
    assert b"net" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create(fake, 2, ctypes.byref(view)) == -1
    assert b"render_filter=2" in lib.dvsg_last_error_string()
    assert lib.dvsg_locnet_view_create(fake, -1, ctypes.byref(view)) == -1
    assert lib.dvsg_locnet_view_create(fake, 1, None) == -1
    assert b"view" in lib.dvsg_last_error_string()
    assert not view.value
    assert lib.dvsg_locnet_render_filter(None) == 0
    assert lib.dvsg_abi_version() == 1


def test_view_calls_are_declared_and_bound(lib):
    from coupe.dvsg_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+dvsg_locnet_view_create\(const dvsg_locnet_t \*net, int render_filter, dvsg_locnet_t \*\*view\);", text)
    assert re.search(r"int\s+dvsg_locnet_render_filter\(const dvsg_locnet_t \*net\);", text)
    assert re.search(r"#define\s+DVSG_RENDER_BILINEAR\s+0\b", text) and re.search(r"#define\s+DVSG_RENDER_BICUBIC\s+1\b", text)
    for name in ("dvsg_locnet_view_create", "dvsg_locnet_render_filter"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert "stream" not in re.search(r"int\s+%s\(([^)]*)\)" % name, text).group(1)
    from coupe.dvsg_amd.networks import RENDER_FILTERS
    assert RENDER_FILTERS == {"bilinear": 0, "bicubic": 1}


def test_python_options_raise_value_errors_without_a_device():
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = StabNet(32, 48)
    frames = np.zeros((2, 32, 48, 3), np.uint8)
    # bicubic where no source-size render happens: RGB at the model's size
    with pytest.raises(ValueError, match="source_res"):
        OnlineStabilizer(model, render_filter="bicubic")
    with pytest.raises(ValueError, match="source_res"):
        OnlineStabilizer(model, render_filter="bicubic", crop="auto", as_uint8=True)
    with pytest.raises(ValueError, match="source_res"):
        stabilize_clip(model, None, frames, render_filter="bicubic")
    # any other value names the option
    for bad in ("lanczos", "", None, 1, b"bicubic"):
        with pytest.raises(ValueError, match="render_filter"):
            OnlineStabilizer(model, source_res=True, render_filter=bad)
        with pytest.raises(ValueError, match="render_filter"):
            stabilize_clip(model, None, frames, source_res=True, render_filter=bad)
    with pytest.raises(ValueError, match="render_filter"):
        OnlineStabilizer(model, frame_format="nv12", render_filter="nearest")


def test_pipe_command_line_takes_the_flag():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "--render-filter" in out.stdout and "bicubic" in out.stdout
    bad = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--render-filter", "lanczos"], cwd=ROOT,
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "--render-filter" in bad.stderr
