"""The views of a network handle as values: what the six constructors hand on and what they reset (include/dvsg_amd.h,
"Render filter" to "Chroma sampling"; coupe/dvsg_amd/csrc/views.cpp makes every view in one place).

A view carries six properties: filter, border, shape (model, strength, rigidity), surface format, chroma format and output
size.  dvsg_locnet_view_create / _border / _shaped set the first three from their arguments and give the other three their
defaults, whatever handle they are applied to; _surface / _scaled / _chroma replace one property and inherit the other five.
The tests walk every order of the inheriting constructors from each value constructor and read all six getters after each
step, so a property dropped or defaulted anywhere along a chain shows at the step that lost it.  No test renders a frame but
the last, one 4x4 NV12 frame, whose point is the argument check in front of the render."""
import ctypes
import itertools

import pytest

pytestmark = pytest.mark.gpu

BILINEAR, BICUBIC = 0, 1
BLACK, REPLICATE, MIRROR = 0, 1, 2
AFFINE, SIMILARITY = 0, 1
NV12, P010 = 0, 1
C420, C422 = 0, 1
DEFAULTS = dict(filter=BILINEAR, border=BLACK, shape=(AFFINE, 1.0, 0.0), surface=NV12, chroma=C420, size=(0, 0))

# the value constructors with non-default arguments (0.5 and 0.25 are float32 values): name, arguments, what they set
VALUE = (
    ("dvsg_locnet_view_create", (BICUBIC,), dict(filter=BICUBIC)),
    ("dvsg_locnet_view_create_border", (BICUBIC, MIRROR), dict(filter=BICUBIC, border=MIRROR)),
    ("dvsg_locnet_view_create_shaped", (BICUBIC, REPLICATE, SIMILARITY, ctypes.c_float(0.5), ctypes.c_float(0.25)),
     dict(filter=BICUBIC, border=REPLICATE, shape=(SIMILARITY, 0.5, 0.25))),
)
# the inheriting constructors: property, name, non-default arguments, their value, default arguments
INHERIT = (
    ("surface", "dvsg_locnet_view_create_surface", (P010,), P010, (NV12,)),
    ("size", "dvsg_locnet_view_create_scaled", (36, 64), (36, 64), (0, 0)),
    ("chroma", "dvsg_locnet_view_create_chroma", (C422,), C422, (C420,)),
)
DESTROY_REFUSED = b"dvsg_locnet_destroy: the handle still has %d view(s); destroy them first"


def _lib():
    from coupe.dvsg_amd import _lib
    return _lib


def _locnet(weights):
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(weights)


@pytest.fixture(scope="module")
def net(synthetic_weights):
    return _locnet(synthetic_weights)


def props(handle):
    """all six getters of a handle"""
    lib = _lib().load()
    model, strength, rigidity = ctypes.c_int(-1), ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.dvsg_locnet_render_shape(handle, ctypes.byref(model), ctypes.byref(strength), ctypes.byref(rigidity)) == 0
    h, w = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.dvsg_locnet_render_size(handle, ctypes.byref(h), ctypes.byref(w)) == 0
    return dict(filter=lib.dvsg_locnet_render_filter(handle), border=lib.dvsg_locnet_render_border(handle),
                shape=(model.value, strength.value, rigidity.value), surface=lib.dvsg_locnet_render_surface(handle),
                chroma=lib.dvsg_locnet_render_chroma(handle), size=(h.value, w.value))


class Views(object):
    """makes views and destroys what is left of them, newest first"""

    def __init__(self):
        self.made = []

    def make(self, name, handle, *args):
        v = ctypes.c_void_p()
        _lib().call(name, handle, *(args + (ctypes.byref(v),)))
        assert v.value, name
        self.made.append(v)
        return v

    def destroy(self, v):
        self.made.remove(v)
        assert _lib().load().dvsg_locnet_destroy(v) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for v in reversed(self.made):
            _lib().load().dvsg_locnet_destroy(v)
        self.made = []


def dressed(views, handle, start=VALUE[2]):
    """a view with no property at its default, and its properties"""
    name, args, sets = start
    v, want = views.make(name, handle, *args), dict(DEFAULTS, **sets)
    for prop, ctor, ctor_args, value, _ in INHERIT:
        v, want = views.make(ctor, v, *ctor_args), dict(want, **{prop: value})
    return v, want


def test_getter_defaults(net):
    assert props(None) == DEFAULTS and props(net.handle) == DEFAULTS
    assert _lib().load().dvsg_locnet_in_channels(None) == 0


@pytest.mark.parametrize("start", VALUE, ids=[v[0] for v in VALUE])
def test_inheritance_chains(net, start):
    lib = _lib().load()
    name, args, sets = start
    with Views() as views:
        for order in itertools.permutations(INHERIT):
            v, want = views.make(name, net.handle, *args), dict(DEFAULTS, **sets)
            assert props(v) == want, name
            for prop, ctor, ctor_args, value, _ in order:
                v, want = views.make(ctor, v, *ctor_args), dict(want, **{prop: value})
                assert props(v) == want, (name, [o[0] for o in order], prop)
                assert lib.dvsg_locnet_in_channels(v) == net.in_channels
            # one of them again, with its default value: that property alone goes back
            for prop, ctor, _, _, default_args in order:
                back = views.make(ctor, v, *default_args)
                assert props(back) == dict(want, **{prop: DEFAULTS[prop]}), (name, [o[0] for o in order], prop)
                assert lib.dvsg_locnet_in_channels(back) == net.in_channels


def test_value_constructors_reset(net):
    """on a fully dressed view: the arguments' filter, border and shape, the defaults of surface, chroma and size"""
    with Views() as views:
        full, want = dressed(views, net.handle)
        assert props(full) == want and all(want[k] != DEFAULTS[k] for k in DEFAULTS)
        for name, args, sets in VALUE + (("dvsg_locnet_view_create", (BILINEAR,), {}),):
            assert props(views.make(name, full, *args)) == dict(DEFAULTS, **sets), name
        assert props(full) == want


def test_parent_and_lifetime(synthetic_weights):
    """every view is the parent's: it is not destroyed while any lives, whatever the order they go in"""
    lib = _lib().load()
    parent = _locnet(synthetic_weights)   # (a handle of this test's own: it ends destroyed)
    with Views() as views:
        full, _ = dressed(views, parent.handle)
        full2, _ = dressed(views, full, VALUE[1])                  # views of a view
        made = list(views.made)
        assert len(made) == 8 and all(lib.dvsg_locnet_in_channels(v) == parent.in_channels for v in made)
        # the first made first, then inwards from both ends: no order of parents and children matters
        for v in [made[i] for i in (0, 7, 1, 6, 3, 4, 2, 5)]:
            assert lib.dvsg_locnet_destroy(parent.handle) == -1
            assert lib.dvsg_last_error_string() == DESTROY_REFUSED % len(views.made)
            views.destroy(v)
    assert lib.dvsg_locnet_destroy(parent.handle) == 0
    parent.handle = None


def test_scaled_table_forgets_a_destroyed_view(net):
    """The renders learn a scaled view's size from the table of scaled views, by the pointer's value.  A destroyed scaled view
    leaves no entry: an unscaled view that the allocator puts at its address has size (0, 0) for the getter and for
    dvsg_tps_render_nv12, whose argument check accepts output planes of the source's size, 4x4, there."""
    import torch
    lib = _lib().load()
    with Views() as views:
        scaled = views.make("dvsg_locnet_view_create_scaled", net.handle, 36, 64)
        address = scaled.value
        assert props(scaled)["size"] == (36, 64)
        views.destroy(scaled)
        reused = None
        for _ in range(256):
            v = views.make("dvsg_locnet_view_create", net.handle, BILINEAR)
            if v.value == address:
                reused = v
                break
        if reused is None:   # (the allocator's business; the rest of this test has nothing to stand on then)
            print("test_scaled_table_forgets_a_destroyed_view: no view landed on the destroyed view's address in 256 "
                  "allocations; the stale-entry check did not run")
            return
        assert props(reused) == DEFAULTS
        F = torch.zeros((1, 25, 2), device="cuda")
        T = torch.empty((1, 2, 28), device="cuda")
        y, uv = torch.zeros((4, 4), dtype=torch.uint8, device="cuda"), torch.zeros((2, 4), dtype=torch.uint8, device="cuda")
        out_y, out_uv = torch.empty_like(y), torch.empty_like(uv)
        rc = lib.dvsg_tps_render_nv12(reused, F.data_ptr(), y.data_ptr(), uv.data_ptr(), 4, 24, 1, 4, 4, T.data_ptr(),
                                      out_y.data_ptr(), out_uv.data_ptr(), 4, 24, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.dvsg_last_error_string()
        torch.cuda.synchronize()
