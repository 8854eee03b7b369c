"""No-GPU checks of warp shaping (include/dvsg_amd.h, "Warp shaping"): the properties of the rule on its NumPy restatement
tests/shape_ref.py, the two entry points' declarations, bindings and argument checks (decided before the handle is read), the
Python options and the front end's flags."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import shape_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvsg_amd.h")
f32 = np.float32
P = S.V_SRC.astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def random_F(seed, n=4):
    return np.random.default_rng(seed).uniform(-0.05, 0.05, (n, 25, 2)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# the rule's own properties
# ---------------------------------------------------------------------------------------------------------------------
def test_the_grid_is_the_models_and_has_the_moments_the_rule_divides_by():
    from coupe.dvsg_amd.model import V_SRC
    assert np.array_equal(S.V_SRC, V_SRC) and S.V_SRC.dtype == f32
    assert P.sum(axis=0).tolist() == [0.0, 0.0] and (P[:, 0] * P[:, 1]).sum() == 0.0
    assert (P[:, 0] ** 2).sum() == 12.5 and (P[:, 1] ** 2).sum() == 12.5 and (P ** 2).sum() == 25.0


def test_full_rigidity_returns_a_field_of_its_own_model_unchanged():
    """Coefficients that are small multiples of 2^-6 on a grid of multiples of 2^-1: every product and every partial sum is a
    multiple of 2^-7 below 2^6, exact in float32 and float64, so the fit is exact and (s, rho) = (1, 1) gives F back bit for bit."""
    q = 2.0 ** -6
    t = np.array([3 * q, -5 * q])
    A = np.array([[2 * q, -3 * q], [1 * q, 4 * q]])               # affine
    a, b = 3 * q, -2 * q
    R = np.array([[a, -b], [b, a]])                               # similarity: L_x = a px - b py, L_y = b px + a py
    fields = {"affine": t + P @ A.T, "similarity": t + P @ R.T, "translation": np.broadcast_to(t, (25, 2))}
    for model, F in fields.items():
        F = np.ascontiguousarray(F, f32)[None]
        assert np.array_equal(F.astype(np.float64)[0], fields[model]), "the field itself is exact in float32"
        assert np.array_equal(bits(S.shape(F, model, 1.0, 1.0)), bits(F)), model
    # a more general model holds the narrower ones: affine returns the similarity and the constant field too
    for name in ("similarity", "translation"):
        F = np.ascontiguousarray(fields[name], f32)[None]
        assert np.array_equal(bits(S.shape(F, "affine", 1.0, 1.0)), bits(F)), name
    # and a narrower one does not return the wider field
    F = np.ascontiguousarray(fields["affine"], f32)[None]
    assert not np.array_equal(S.shape(F, "similarity", 1.0, 1.0), F)
    assert not np.array_equal(S.shape(F, "translation", 1.0, 1.0), F)


@pytest.mark.parametrize("model", sorted(S.MODELS))
def test_strength_zero_gives_zeros(model):
    for rho in (0.0, 0.4, 1.0):
        assert (S.shape(random_F(1), model, 0.0, rho) == 0).all()


def test_the_affine_residual_is_orthogonal_to_one_px_and_py():
    """For w in (1, px, py) the sum of w_i (d_i - L_i) is zero in exact arithmetic.  In float64 (u = 2^-53, S = the sum of
    |d_i| of the component): the parameter that w belongs to carries at most 25 u S of its sequential sum and division into the
    functional (25 dmx, or 12.5 da with |p| <= 1); forming L_i (four roundings of terms no larger than |L_i|) and d_i - L_i (one)
    adds at most 5 u (|L_i| + |r_i|) <= 15 u |d|-sized terms per point; the other two parameters enter through sums of p that are
    exactly zero.  40 u S in all, asserted as 64 u S.  The test's own sums are exact (math.fsum; w r is exact for w in 0, 0.5, 1)."""
    u = 2.0 ** -53
    F = random_F(2, 6)
    for b in range(len(F)):
        d = F[b].astype(np.float64)
        r = d - S.fit(d, "affine")
        for c in range(2):
            tol = 64 * u * math.fsum(np.abs(d[:, c]))
            for w in (np.ones(25), P[:, 0], P[:, 1]):
                assert abs(math.fsum(w * r[:, c])) <= tol, (b, c)
    # and the fit is not the field: the residual itself is of the size of d
    assert np.abs(r).max() > 1e-3


def test_half_strength_without_rigidity_is_half_the_field():
    """rho = 0: F' = (float)(0.5 (L + (d - L))).  L + (d - L) is d up to a few float64 roundings, 0.5 F is exact in float32, so F'
    is 0.5 F or its float32 neighbour."""
    F = random_F(3)
    for model in S.MODELS:
        got = S.shape(F, model, 0.5, 0.0)
        half = f32(0.5) * F
        assert (np.abs(got.astype(np.float64) - half.astype(np.float64)) <= np.spacing(np.abs(half)).astype(np.float64)).all()
        assert (got == half).mean() > 0.9
    # the unshaped pair leaves F to the same rounding
    got = S.shape(F, "affine", 1.0, 0.0)
    assert (np.abs(got.astype(np.float64) - F.astype(np.float64)) <= np.spacing(np.abs(F)).astype(np.float64)).all()


@pytest.mark.parametrize("model", sorted(S.MODELS))
def test_a_nan_spoils_its_own_frame_only(model):
    F = random_F(4, 3)
    bad = F.copy()
    bad[1, 7, 0] = np.nan
    got = S.shape(bad, model, 0.5, 0.5)
    want = S.shape(F, model, 0.5, 0.5)
    assert np.isnan(got[1, :, 0]).all(), "x of every point of the frame: the NaN enters the mean"
    assert np.array_equal(bits(got[[0, 2]]), bits(want[[0, 2]]))
    if model == "similarity":        # a and b sum products of both components; the other models fit y on its own
        assert np.isnan(got[1]).all()
    else:
        assert np.array_equal(bits(got[1, :, 1]), bits(want[1, :, 1]))


def test_strength_and_rigidity_are_taken_as_float32():
    F = random_F(5, 1)
    assert np.array_equal(bits(S.shape(F, "affine", 0.1, 0.3)), bits(S.shape(F, "affine", f32(0.1), f32(0.3))))
    assert np.array_equal(bits(S.shape(F, "affine", 0.1, 0.3)), bits(S.shape(F, "affine", float(f32(0.1)), float(f32(0.3)))))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI, without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def test_shape_calls_are_declared_exported_and_bound(lib):
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import SHAPE_MODELS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+dvsg_locnet_view_create_shaped\(const dvsg_locnet_t \*net, int render_filter, int render_border,\s+"
                     r"int shape_model,\s+float strength, float rigidity, dvsg_locnet_t \*\*view\);", text)
    assert re.search(r"int\s+dvsg_locnet_render_shape\(const dvsg_locnet_t \*net, int \*shape_model, float \*strength, "
                     r"float \*rigidity\);", text)
    for name, value in (("AFFINE", 0), ("SIMILARITY", 1), ("TRANSLATION", 2)):
        assert re.search(r"#define\s+DVSG_SHAPE_%s\s+%d\b" % (name, value), text), name
    for name in ("dvsg_locnet_view_create_shaped", "dvsg_locnet_render_shape"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert "stream" not in re.search(r"int\s+%s\(([^)]*)\)" % name, text).group(1)
    assert SHAPE_MODELS == {"affine": 0, "similarity": 1, "translation": 2} == S.MODELS
    assert lib.dvsg_abi_version() == 1


def report(lib, handle):
    m, s, r = ctypes.c_int(-7), ctypes.c_float(-7.0), ctypes.c_float(-7.0)
    assert lib.dvsg_locnet_render_shape(handle, ctypes.byref(m), ctypes.byref(s), ctypes.byref(r)) == 0
    return m.value, s.value, r.value


def test_view_create_shaped_rejects_bad_arguments_before_the_handle_is_read(lib):
    view = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)      # never dereferenced: every call below is refused first
    fn = lib.dvsg_locnet_view_create_shaped
    err = lib.dvsg_last_error_string
    assert fn(None, 0, 0, 0, 0.5, 0.5, ctypes.byref(view)) == -1
    assert b"dvsg_locnet_view_create_shaped: NULL net" in err()
    assert fn(fake, 0, 0, 0, 0.5, 0.5, None) == -1
    assert b"dvsg_locnet_view_create_shaped: NULL view" in err()
    assert fn(fake, 2, 0, 0, 0.5, 0.5, ctypes.byref(view)) == -1
    assert b"dvsg_locnet_view_create_shaped: render_filter=2" in err()
    assert fn(fake, 1, 4, 0, 0.5, 0.5, ctypes.byref(view)) == -1
    assert b"render_border=4" in err()
    for bad in (3, -1):
        assert fn(fake, 1, 3, bad, 0.5, 0.5, ctypes.byref(view)) == -1
        assert b"shape_model=%d" % bad in err()
    for bad, text in ((-0.25, b"strength=-0.25"), (1.5, b"strength=1.5"), (float("nan"), b"strength=nan"),
                      (float("inf"), b"strength=inf")):
        assert fn(fake, 0, 0, 1, bad, 0.5, ctypes.byref(view)) == -1
        assert text in err().lower(), err()
    for bad, text in ((-0.25, b"rigidity=-0.25"), (1.5, b"rigidity=1.5"), (float("nan"), b"rigidity=nan")):
        assert fn(fake, 0, 0, 2, 0.5, bad, ctypes.byref(view)) == -1
        assert text in err().lower(), err()
    assert fn(fake, 0, 0, 0, float(np.nextafter(f32(1), f32(2))), 0.0, ctypes.byref(view)) == -1
    assert not view.value
    assert report(lib, None) == (0, 1.0, 0.0)
    assert lib.dvsg_locnet_render_shape(None, None, None, None) == 0
    # the older constructors keep their own names in their messages
    assert lib.dvsg_locnet_view_create_border(fake, 1, 4, ctypes.byref(view)) == -1
    assert b"dvsg_locnet_view_create_border: render_border=4" in err()
    assert lib.dvsg_abi_version() == 1


def test_render_shape_reports_each_view_on_a_stand_in_parent(lib):
    """The view constructors are host-side: of the handle they are given they read whether it is itself a view and count one
    more view on it, nothing else.  A zeroed block stands in for a network's handle (not a view, no views), so the views, their
    reports and the rule "a view of a view is a view of the parent, nothing inherited" are checked without a device."""
    block = ctypes.create_string_buffer(1 << 20)
    parent = ctypes.c_void_p(ctypes.addressof(block))
    made = []

    def make(name, handle, *args):
        v = ctypes.c_void_p()
        assert getattr(lib, name)(handle, *args, ctypes.byref(v)) == 0, lib.dvsg_last_error_string()
        made.append(v)
        return v
    try:
        assert report(lib, make("dvsg_locnet_view_create", parent, 1)) == (0, 1.0, 0.0)
        assert report(lib, make("dvsg_locnet_view_create_border", parent, 1, 2)) == (0, 1.0, 0.0)
        shaped = make("dvsg_locnet_view_create_shaped", parent, 1, 2, 1, 0.25, 0.75)
        assert report(lib, shaped) == (1, 0.25, 0.75)
        assert (lib.dvsg_locnet_render_filter(shaped), lib.dvsg_locnet_render_border(shaped)) == (1, 2)
        edge = make("dvsg_locnet_view_create_shaped", parent, 0, 0, 2, 0.0, 1.0)
        assert report(lib, edge) == (2, 0.0, 1.0)
        assert (lib.dvsg_locnet_render_filter(edge), lib.dvsg_locnet_render_border(edge)) == (0, 0)
        tenth = make("dvsg_locnet_view_create_shaped", parent, 0, 0, 0, 0.1, 0.0)
        assert report(lib, tenth) == (0, float(f32(0.1)), 0.0)
        # unshaped whatever its model: the report still says what the view was made with
        assert report(lib, make("dvsg_locnet_view_create_shaped", parent, 0, 3, 2, 1.0, 0.0)) == (2, 1.0, 0.0)
        # a view of a view: nothing inherited, through any constructor
        assert report(lib, make("dvsg_locnet_view_create_border", shaped, 0, 1)) == (0, 1.0, 0.0)
        assert report(lib, make("dvsg_locnet_view_create", shaped, 0)) == (0, 1.0, 0.0)
        nested = make("dvsg_locnet_view_create_shaped", shaped, 0, 0, 2, 0.5, 0.5)
        assert report(lib, nested) == (2, 0.5, 0.5)
        # NULL outputs are skipped
        s = ctypes.c_float()
        assert lib.dvsg_locnet_render_shape(shaped, None, ctypes.byref(s), None) == 0 and s.value == 0.25
        # nested views count on the parent: every one of them can be destroyed in any order
        assert lib.dvsg_locnet_destroy(shaped) == 0
        made.remove(shaped)
        assert report(lib, nested) == (2, 0.5, 0.5)
    finally:
        for v in made:
            assert lib.dvsg_locnet_destroy(v) == 0
    assert block.raw == bytes(len(block)), "the views are gone: the stand-in counts none"


# ---------------------------------------------------------------------------------------------------------------------
# Python
# ---------------------------------------------------------------------------------------------------------------------
def test_check_shape():
    from coupe.dvsg_amd.networks import check_shape
    assert check_shape() == (1.0, 0.0, "affine")
    assert check_shape(0.1, 1, "similarity") == (float(f32(0.1)), 1.0, "similarity")
    assert check_shape(1.0, 0.0, "translation", False) == (1.0, 0.0, "translation")
    for bad in (-0.1, 1.01, float("nan"), "0.5", None, True, [0.5]):
        with pytest.raises(ValueError, match="strength"):
            check_shape(strength=bad)
        with pytest.raises(ValueError, match="rigidity"):
            check_shape(rigidity=bad)
    for bad in ("rigid", "", None, 0, b"affine"):
        with pytest.raises(ValueError, match="shape_model"):
            check_shape(shape_model=bad)
    for kw in (dict(strength=0.5), dict(rigidity=1.0), dict(strength=0.0, rigidity=0.5, shape_model="translation")):
        with pytest.raises(ValueError, match="source_res"):
            check_shape(source_size_render=False, **kw)
        assert check_shape(**kw)[2] == kw.get("shape_model", "affine")


def test_python_options_raise_value_errors_without_a_device():
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = StabNet(32, 48)
    frames = np.zeros((2, 32, 48, 3), np.uint8)
    for kw in (dict(strength=0.5), dict(rigidity=0.5), dict(strength=0.5, rigidity=1.0, shape_model="similarity")):
        # no source-size render: RGB at the model's size, float frames
        with pytest.raises(ValueError, match="source_res"):
            OnlineStabilizer(model, **kw)
        with pytest.raises(ValueError, match="source_res"):
            OnlineStabilizer(model, crop="auto", as_uint8=True, **kw)
        with pytest.raises(ValueError, match="source_res"):
            stabilize_clip(model, None, frames, **kw)
    for bad in (-1.0, 2.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="strength"):
            OnlineStabilizer(model, source_res=True, strength=bad)
        with pytest.raises(ValueError, match="rigidity"):
            OnlineStabilizer(model, frame_format="nv12", rigidity=bad)
        with pytest.raises(ValueError, match="strength"):
            stabilize_clip(model, None, frames, source_res=True, strength=bad)
    with pytest.raises(ValueError, match="shape_model"):
        OnlineStabilizer(model, source_res=True, shape_model="rigid")
    with pytest.raises(ValueError, match="shape_model"):
        stabilize_clip(model, None, frames, source_res=True, shape_model="rigid")


def test_pipe_command_line_takes_the_flags():
    out = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0
    for name in ("--strength", "--rigidity", "--shape-model", "affine", "similarity", "translation"):
        assert name in out.stdout, name
    bad = subprocess.run([sys.executable, "-m", "coupe.dvsg_amd.pipe", "--shape-model", "rigid"], cwd=ROOT, capture_output=True,
                         text=True)
    assert bad.returncode != 0 and "--shape-model" in bad.stderr
