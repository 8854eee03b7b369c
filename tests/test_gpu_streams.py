"""GPU: every entry point of include/dvsg_amd.h that takes a `stream` is held to the header's stream contract
("Conventions": asynchronous and stream-ordered; none allocates, frees or synchronises; calls on distinct streams are
re-entrant as long as their output / workspace buffers are distinct).  Values are pinned elsewhere; here every comparison is
BIT equality of a call against the same call run alone or eagerly, and no number in this file is fitted.

0. `CASES` maps every such entry point to one or more builders; `EXEMPT` names the ones the header itself documents as
   synchronous (tests/test_abi_cpu.py checks on the CPU that the two cover the header).  A builder allocates everything up
   front and returns a `Case`: input, output and state tensors and `issue(stream)`, which makes exactly ONE ABI call through
   `_lib.call` and allocates nothing.  The four source-size renders are registered once on the plain handle and once per row
   of `VIEWS` (label -> LocNet.view arguments), on the plain and on the _zoom_ entry point: every kernel family behind a
   view property (bicubic, the three border modes, shaping, P010 words, a delivery size, 4:2:2 chroma rows) is launched,
   and dvsg_tps_coefficients_f32 and dvsg_tps_coverage_net_f32 are given the shaped view.  `VIEW_CONSTRUCTORS` names, for
   every view constructor of the header, the rows built through it (tests/test_abi_cpu.py holds it to the header and to
   the rows' arguments on the CPU).  No row of the table is refused by render_scaled_check.  View handles are made in the
   builder with LocNet.view (`cubic` by dvsg_locnet_view_create itself, which LocNet.view never calls).  What makes such a case able to fail is asserted on its eager references before any replay is compared
   (`ViewCheck`): the outputs of the three seeds differ pairwise; the output differs from that of the same call through
   the plain handle on the same inputs while T is the plain handle's bit for bit (on a shaped view T differs); and a
   `keep` output, poisoned beforehand, has bytes inside each plane that still are the poison and bytes that are not.
1. Capture and replay: `issue` is captured on one non-blocking stream into a HIP graph (default capture error mode: an
   allocation, a free, a synchronisation or a launch on another stream inside the call fails the capture) and replayed three
   times on fresh input values, restored state and poisoned outputs; each replay equals the eager call on those values.  The
   scene step carries its state through the three replays as three consecutive steps.
2. Re-entrancy at the ABI: pairs of cases on two non-blocking streams of ONE handle, each with its own workspace of exactly
   dvsg_locnet_workspace_bytes between sentinels, released together by one event; once more from two Python threads, each of
   which also makes an invalid call and reads its own dvsg_last_error_string().  Four of the pairs are views of one parent:
   two delivery sizes on a shared F_t, a P010 beside an NV16 view, one scaled view twice, and the plain handle beside a
   scaled view on one source buffer.
2a. The table of scaled views (g_scaled_views, views.cpp: the library's one process-global host table on a hot path, read
   by every NV12 render before it touches the handle): two threads render through scaled views while a third makes and
   destroys 64 scaled views of the same parent; the renders equal their runs alone, the sizes of the views used and of the
   plain handle are unchanged, the parent's views are those from before, and each thread's refused call names the size of
   its own view.
3. The Python facade: LocNet.workspace is per stream; forward / stabilize / tap of one LocNet under two torch streams, and two
   OnlineStabilizers that share a model, equal the serial runs -- with default options, and as an NV12 stream (bicubic,
   mirrored border, crop="auto", a scene cut at its third step, asserted) beside a P210 stream at half strength and size.
4. Calibration is synchronous: a float16 forward queued on a non-blocking stream in front of dvsg_locnet_calibrate_f16(NULL)
   or dvsg_debug_calibrate_f16_weights(mode 0 / 1) on that stream still runs on the weights it was issued against.

The bounded delay of 2-4 is ordinary work, a chain of torch.matmul sized once per module with events (about 20 ms).  A run is
CONCLUSIVE when the event recorded right behind the delay has not completed at the moment the host returns from issuing the
calls under test; an inconclusive run doubles the chain, at most four times, and then FAILS.  A condition, not a tolerance.
Measured on one MI355X: 198 cases in 34.6 s, next to 21.7 s for the 156 cases of the module before the views, on the same
machine in the same run (26.7 s for the 198 on another machine); every delayed case conclusive behind one chain; the slowest
cases are the three calibration ones (2-3 s: each re-rounds 25 M weights on the host several times), the two facade pairs of
OnlineStabilizers take about 1 s each and every view case well under 0.2 s.  `keep` is visible at the default scale of
vectors(): the poisoned `keep` outputs hold 69 to 1722 untouched samples of 17649 (RGB, float32) and 70 to 1436 untouched
bytes per plane (NV12), the small counts under the zoom.

Found with this module (the paragraph is in the header's "Conventions" block).  Against the library and facade from before
the fixes: the captured dvsg_scene_step_f32 differed from its second replay on (a memset node zeroed the histograms and did
not take effect again; it is a kernel now); LocNet.workspace handed one buffer to every stream, and forward, stabilize and two
OnlineStabilizers on a shared model returned wrong values under two streams (tap at stage 9 happened to pass); modes 0 / 1 of
dvsg_debug_calibrate_f16_weights rewrote the weights under a queued float16 forward, while the undo form of
dvsg_locnet_calibrate_f16, which has the same defect in the code, happened to pass: the 20 ms delay ran out before redo()
reached the layers that forward reads.  Sections 1 (every other case) and 2 passed before and after.  The parity taps'
hipMemcpyAsync (device to device, locnet.hip) is captured as a memcpy node and replays correctly: every
dvsg_locnet_forward_tap_* case below passes, so it needs no kernel of its own.
With the views (sections 0 to 3 extended): every capture case, the four pairs of views and the thread test on the table of
scaled views passed against the library as it was; the dispatch and the table needed no change.  The facade pair on the
newer formats did not: before, the run was inconclusive behind every delay up to 16 chains of 20 ms, because the first
step of an "nv16" / "p210" OnlineStabilizer built the index of the even chroma rows on the host and copied it to the device,
and that copy waits for the caller's stream ("device tensors in still means nothing synchronised", online.py); after, with
the index made on the device, it is conclusive behind one chain and equals the serial run, bit for bit."""
import ctypes
import gc
import threading

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

POISON = 0xA5
NET_SHAPES = [(2, 64, 96), (3, 33, 47)]     # split-K launches of blocks 3-4 run at batch 1-3 (test_units_f64.py); ragged
PRECISIONS = ("f32", "f16", "f32s", "f32x3")
PREC_CODE = {"f32": 0, "f16": 1, "f32s": 2, "f32x3": 3}      # DVSG_PRECISION_*
TAP_STAGES = (0, 5, 17, 18)
SRC = (37, 53)                              # tests/test_gpu_source_res.py's odd frame
NV = (38, 54)                               # tests/test_gpu_nv12.py's MODEL
LOSS = (3, 33, 65)                          # tests/test_gpu_losses.py
SCENE = (37, 53, 3)                         # tests/test_gpu_scene.py
SURF = (68, 102)                            # the NV12 / P010 / 4:2:2 source of the surface renders

# label -> the LocNet.view arguments of a view the four source-size renders are given.  Every row is registered on the plain
# and on the _zoom_ entry point; what it launches is read off tps_render_impl (warp_kernels.hip) and tps_render_nv12_impl
# (nv12.hip).  The scaled sizes give factors 2 x 2 and 3 x 3 (37 / 13 and 53 / 18 do not divide), are even and >= 4 for the
# surfaces, and no scaled row asks for `keep` (render_scaled_check): no row is refused.
_SHAPE = dict(strength=0.25, rigidity=0.75, shape_model="similarity")
VIEWS = {
    # RGB and surface rows
    "cubic": dict(render_filter="bicubic"),                                   # tps_ / nv12_render_cubic_kernel
    # RGB rows
    "replicate": dict(border="replicate"),                                    # tps_render_border_kernel
    "cubic-mirror": dict(render_filter="bicubic", border="mirror"),           # tps_render_border_kernel, cubic
    "keep": dict(border="keep"),                                              # tps_render_border_kernel, keep
    "shaped": dict(**_SHAPE),                                                 # tps_shape_apply_kernel forms T
    "scaled-2x2": dict(out_size=(19, 27)),                                    # tps_render_scaled_kernel
    "scaled-3x3-cubic-mirror": dict(render_filter="bicubic", border="mirror", out_size=(13, 18)),
    # surface rows
    "mirror": dict(border="mirror"),                                          # nv12_render_border_kernel
    "cubic-keep": dict(render_filter="bicubic", border="keep"),               # nv12_render_border_kernel, cubic, keep
    "p010": dict(surface="p010"),                                             # p010_render_kernel
    "p010-cubic-replicate": dict(render_filter="bicubic", border="replicate", surface="p010"),
    "scaled-3x3": dict(out_size=(24, 36)),                                    # nv12_render_scaled_kernel on bytes
    "p010-scaled-2x2-cubic-mirror": dict(render_filter="bicubic", border="mirror", surface="p010", out_size=(34, 52)),
    "nv16": dict(chroma="422"),                                               # the NV12 kernels, chroma rows = H
    "p210-cubic-mirror-shaped": dict(render_filter="bicubic", border="mirror", surface="p010", chroma="422", **_SHAPE),
    "p210-scaled-2x2": dict(surface="p010", out_size=(34, 52), chroma="422"),  # nv12_render_scaled_kernel, words, 4:2:2
}
RGB_VIEWS = ("cubic", "replicate", "cubic-mirror", "keep", "shaped", "scaled-2x2", "scaled-3x3-cubic-mirror")
SURFACE_VIEWS = ("cubic", "mirror", "cubic-keep", "p010", "p010-cubic-replicate", "scaled-3x3", "p010-scaled-2x2-cubic-mirror",
                 "nv16", "p210-cubic-mirror-shaped", "p210-scaled-2x2")
# Every view constructor of the header -> the labels built through it (tests/test_abi_cpu.py: each declared constructor is
# here, none is empty, every label exists, and the entries are what `constructors_of` derives from the arguments).
# LocNet.view never calls dvsg_locnet_view_create (it is dvsg_locnet_view_create_border with a black border), so the views
# listed for it are made by that constructor itself (`_view`) and destroyed with the module's context.
VIEW_CONSTRUCTORS = {
    "dvsg_locnet_view_create": ("cubic",),
    "dvsg_locnet_view_create_border": ("replicate", "cubic-mirror", "keep", "scaled-3x3-cubic-mirror", "mirror", "cubic-keep",
                                       "p010-cubic-replicate", "p010-scaled-2x2-cubic-mirror"),
    "dvsg_locnet_view_create_shaped": ("shaped", "p210-cubic-mirror-shaped"),
    "dvsg_locnet_view_create_surface": ("p010", "p010-cubic-replicate", "p010-scaled-2x2-cubic-mirror",
                                        "p210-cubic-mirror-shaped", "p210-scaled-2x2"),
    "dvsg_locnet_view_create_scaled": ("scaled-2x2", "scaled-3x3-cubic-mirror", "scaled-3x3", "p010-scaled-2x2-cubic-mirror",
                                       "p210-scaled-2x2"),
    "dvsg_locnet_view_create_chroma": ("nv16", "p210-cubic-mirror-shaped", "p210-scaled-2x2"),
}


def _shaped(label):
    kw = VIEWS.get(label, {})
    return kw.get("strength", 1.0) != 1.0 or kw.get("rigidity", 0.0) != 0.0


def constructors_of(label):
    """The constructors the view of `label` is built through: LocNet.view's chain (coupe/dvsg_amd/networks.py), innermost
    first, with dvsg_locnet_view_create in the place of _border for the labels `_view` makes with it."""
    kw, chain = VIEWS[label], []
    if _shaped(label):
        chain.append("dvsg_locnet_view_create_shaped")
    elif label in VIEW_CONSTRUCTORS["dvsg_locnet_view_create"]:
        assert kw.get("border", "black") == "black", "dvsg_locnet_view_create takes a filter only"
        chain.append("dvsg_locnet_view_create")
    elif kw.get("render_filter", "bilinear") != "bilinear" or kw.get("border", "black") != "black":
        chain.append("dvsg_locnet_view_create_border")
    if kw.get("surface", "nv12") != "nv12":
        chain.append("dvsg_locnet_view_create_surface")
    if kw.get("out_size") is not None:
        chain.append("dvsg_locnet_view_create_scaled")
    if kw.get("chroma", "420") != "420":
        chain.append("dvsg_locnet_view_create_chroma")
    return chain


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _rng(seed, salt):
    return np.random.default_rng(1000003 * seed + salt)


def uni(shape, lo=0.0, hi=1.0, salt=0, dtype=np.float32):
    return lambda seed: _t(_rng(seed, salt).uniform(lo, hi, shape).astype(dtype))


def ints(shape, lo, hi, salt=0, dtype=np.int32):
    return lambda seed: _t(_rng(seed, salt).integers(lo, hi, shape).astype(dtype))


def fixed(a):
    a = np.ascontiguousarray(a)
    return lambda seed: _t(a)


def vectors(n, salt=0, scale=0.05):
    return lambda seed: _t(inputs.control_vectors(977 * seed + salt, n, scale=scale))


def _poison(t):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.view(_torch().uint8).fill_(POISON)


def _bits(t):
    return t.contiguous().view(-1).view(_torch().uint8)


def _guarded(nbytes):
    import test_conv_gemm_f64 as f64
    return f64.Guarded(nbytes, _torch().device("cuda:0"))


class Case(object):
    """Everything one ABI call touches, allocated before the first `issue`."""

    def __init__(self):
        self.inputs, self.outputs, self.state, self.also, self.guards, self.keep = [], [], [], [], [], []
        self.issue = None
        self.carry = False          # the scene step: state runs on through the three replays
        self.view = None            # a case on a view handle: its `ViewCheck`

    def inp(self, gen):
        t = gen(0).clone()
        self.inputs.append((t, gen))
        return t

    def out(self, shape, dtype=None):
        torch = _torch()
        t = torch.empty(shape, dtype=dtype or torch.float32, device="cuda")
        self.outputs.append(t)
        return t

    def st(self, value):
        t = value.clone()
        self.state.append((t, value.clone()))
        return t

    def work(self, nbytes):
        """scratch of exactly nbytes between sentinels -> (pointer, nbytes)"""
        g = _guarded(nbytes)
        self.guards.append(g)
        return g.ptr(), nbytes

    def fill(self, seed):
        for t, gen in self.inputs:
            t.copy_(gen(seed))

    def restore(self):
        for t, v in self.state:
            t.copy_(v)

    def poison(self):
        for t in self.outputs:
            _poison(t)

    def snapshot(self):
        return [t.clone() for t in self.outputs + [t for t, _ in self.state] + self.also]

    def same(self, want, what):
        got = self.outputs + [t for t, _ in self.state] + self.also
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert _torch().equal(_bits(g), _bits(w)), "%s: checked tensor %d of %d differs" % (what, i, len(got))
        for g in self.guards:
            assert g.intact(), "%s: a workspace was written outside its bytes" % what


class ViewCheck(object):
    """What makes a case on a view handle able to fail, asserted on its eager references before any replay is compared.
    plain_issue(stream): the same ABI call through the plain handle on the same inputs, into plain_outputs (the first is T),
    allocated by the builder.  pairs(w): [(tensor of the snapshot w, the same region of a plain output)], or None for the
    entry points that write nothing but T and counts.  fresh: the outputs that must differ between any two seeds (default:
    all).  kept(w): the planes of a `keep` output, [(what, tensor)]."""

    def __init__(self, label, plain_issue, plain_outputs, pairs=None, fresh=None, kept=None):
        self.label, self.plain_issue, self.plain_outputs = label, plain_issue, plain_outputs
        self.pairs, self.fresh, self.kept = pairs, fresh, kept

    def check(self, c, want, s, side, what):
        """want: the eager snapshots of seeds 1, 2, 3; the inputs still hold seed 3's values."""
        torch = _torch()
        fresh = range(len(c.outputs)) if self.fresh is None else self.fresh
        for a, b in ((0, 1), (0, 2), (1, 2)):
            for i in fresh:
                assert not torch.equal(_bits(want[a][i]), _bits(want[b][i])), \
                    "%s: output %d is the same for seeds %d and %d: a replay on stale values would pass" % (what, i, a + 1, b + 1)
        for t in self.plain_outputs:
            _poison(t)
        torch.cuda.synchronize()
        self.plain_issue(s)
        side.synchronize()
        same_T = torch.equal(_bits(want[2][0]), _bits(self.plain_outputs[0]))
        if _shaped(self.label):
            assert not same_T, "%s: T of the shaped view is the plain handle's" % what
        else:
            assert same_T, "%s: T differs from the plain handle's on an unshaped view" % what
        if self.pairs is not None:
            assert any(not torch.equal(_bits(v), _bits(p)) for v, p in self.pairs(want[2])), \
                "%s: the view renders what the plain handle renders: the property was not exercised" % what
        if self.kept is not None:
            for w in want:
                for name, plane in self.kept(w):
                    left = int(plane.isnan().sum()) if plane.dtype.is_floating_point else int((plane == POISON).sum())
                    print("STREAMS %s: %s keeps %d of %d" % (what, name, left, plane.numel()))
                    assert 0 < left < plane.numel(), "%s: %s keeps %d of %d: `keep` is not visible" % (what, name, left, plane.numel())


class Ctx(object):
    """What the builders share: the handle, the ABI, a scratch for the stand-alone convs."""

    def __init__(self, weights):
        from coupe.dvsg_amd import _lib
        from coupe.dvsg_amd.networks import LocNet
        torch = _torch()
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        self.net = LocNet(weights)
        self.h = self.net.handle
        self.lib = _lib
        self._scratch = None
        self._own = {}              # label -> a view made by dvsg_locnet_view_create itself (LocNet.view never calls it)

    def call(self, name, *args):
        self.lib.call(name, *args)

    def view(self, label):
        """The handle of VIEWS[label], made on first use and kept; "": the plain handle."""
        if not label:
            return self.h
        from coupe.dvsg_amd.networks import RENDER_FILTERS
        kw = VIEWS[label]
        if label not in VIEW_CONSTRUCTORS["dvsg_locnet_view_create"]:
            return self.net.view(**kw)
        v = self._own.get(label)
        if v is None:
            assert set(kw) == {"render_filter"}, "dvsg_locnet_view_create takes a filter only"
            v = self._own[label] = ctypes.c_void_p()
            self.call("dvsg_locnet_view_create", self.h, RENDER_FILTERS[kw["render_filter"]], ctypes.byref(v))
        return v

    def render_size(self, handle):
        oh, ow = ctypes.c_int(-1), ctypes.c_int(-1)
        self.call("dvsg_locnet_render_size", handle, ctypes.byref(oh), ctypes.byref(ow))
        return oh.value, ow.value

    def n_views(self):
        """The live views of the parent, from the refusal of dvsg_locnet_destroy(parent) (the header: "destroying a parent
        that still has views is DVSG_ERR_INVALID_ARG and destroys nothing"); only asked while LocNet holds a view."""
        import re
        assert self.net._views, "the parent has no view: dvsg_locnet_destroy would destroy it"
        lib = self.lib.load()
        assert lib.dvsg_locnet_destroy(self.h) == -1
        return int(re.search(r"still has (\d+) view", lib.dvsg_last_error_string().decode()).group(1))

    def close(self):
        for v in self._own.values():
            self.call("dvsg_locnet_destroy", v)
        self._own = {}

    def ws_bytes(self, B, H, W):
        need = ctypes.c_size_t()
        self.call("dvsg_locnet_workspace_bytes", self.h, B, H, W, ctypes.byref(need))
        return need.value

    def scratch(self):
        if self._scratch is None:
            self._scratch = _torch().empty(66 << 20, dtype=_torch().uint8, device="cuda")
        return self._scratch

    def cur(self):
        return _torch().cuda.current_stream().cuda_stream


CASES = {}


def case(name, label=""):
    def deco(fn):
        fn.label = label
        CASES.setdefault(name, []).append(fn)
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------------------------
# the network entries
# ---------------------------------------------------------------------------------------------------------------------
def _tap_cap(B, H, W):
    """floats that hold any stage of a frame no smaller than 33 x 47: conv1's map or block 1's output, or pool5"""
    h1, w1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h2, w2 = (h1 + 1) // 2, (w1 + 1) // 2
    return B * max(h1 * w1 * 64, h2 * w2 * 256, 2048)


def _ring(c, B, H, W, u8, salt):
    """a frame pool of 8 + B frames and a table [B,7] into its first 8 -> (pool, n_pool, table)"""
    n = 8 + B
    pool = c.inp(ints((n, H, W, 3), 0, 256, salt, np.uint8) if u8 else uni((n, H, W, 3), salt=salt))
    table = c.inp(ints((B, 7), 0, 8, salt + 1))
    return pool, n, table


def _mask(c, B, H, W, salt):
    return c.inp(uni((B, H, W), 0.0, 1.0, salt))


def net_case(kind, prec, B, H, W, stage=-1, src=0):
    def build(ctx):
        c = Case()
        ws, nb = c.work(ctx.ws_bytes(B, H, W))
        code, h = PREC_CODE[prec], ctx.h
        n = B * H * W
        if kind in ("forward", "tap", "stabilize", "masked"):
            x = c.inp(uni((B, H, W, 21), salt=1))
        if kind in ("stabilize", "masked"):
            u = c.inp(uni((B, H, W, 3), salt=2))
        if kind in ("stabilize", "masked", "ring_f32", "ring_u8", "ring_masked_f32", "ring_masked_u8"):
            s_out, F, xs, ys = c.out((B, H, W, 3)), c.out((B, 25, 2)), c.out((n,)), c.out((n,))
        if kind == "forward":
            F = c.out((B, 25, 2))
            c.issue = lambda s: ctx.call("dvsg_locnet_forward_" + prec, h, x.data_ptr(), B, H, W, F.data_ptr(), ws, nb, s)
        elif kind == "tap":
            act = c.out((_tap_cap(B, H, W),))
            dims = (ctypes.c_int * 3)()
            c.keep.append(dims)
            c.issue = lambda s: ctx.call("dvsg_locnet_forward_tap_" + prec, h, x.data_ptr(), B, H, W, stage, act.data_ptr(),
                                         act.numel() * 4, dims, ws, nb, s)
        elif kind == "stabilize":
            c.issue = lambda s: ctx.call("dvsg_stabilize_" + prec, h, x.data_ptr(), u.data_ptr(), B, H, W, s_out.data_ptr(),
                                         F.data_ptr(), xs.data_ptr(), ys.data_ptr(), ws, nb, s)
        elif kind == "masked":
            m = _mask(c, B, H, W, 3)
            c.issue = lambda s: ctx.call("dvsg_stabilize_masked_f32", h, code, x.data_ptr(), u.data_ptr(), m.data_ptr(), B, H,
                                         W, s_out.data_ptr(), F.data_ptr(), xs.data_ptr(), ys.data_ptr(), ws, nb, s)
        elif kind in ("ring_f32", "ring_u8"):
            pool, n_pool, table = _ring(c, B, H, W, kind == "ring_u8", 4)
            c.issue = lambda s: ctx.call("dvsg_stabilize_" + kind, h, code, pool.data_ptr(), n_pool, table.data_ptr(), B, H, W,
                                         s_out.data_ptr(), F.data_ptr(), xs.data_ptr(), ys.data_ptr(), ws, nb, s)
        elif kind in ("ring_masked_f32", "ring_masked_u8"):
            pool, n_pool, table = _ring(c, B, H, W, kind == "ring_masked_u8", 6)
            m = _mask(c, B, H, W, 8)
            c.issue = lambda s: ctx.call("dvsg_stabilize_" + kind, h, code, pool.data_ptr(), n_pool, table.data_ptr(),
                                         m.data_ptr(), B, H, W, s_out.data_ptr(), F.data_ptr(), xs.data_ptr(), ys.data_ptr(),
                                         ws, nb, s)
        elif kind == "inplace":
            # the contract: the out slots are distinct and no table entry names one -- the table reads frames 0..7 only
            pool, n_pool, table = _ring(c, B, H, W, False, 9)
            slots = c.inp(fixed(np.arange(8, 8 + B, dtype=np.int32)))
            F, xs, ys = c.out((B, 25, 2)), c.out((n,)), c.out((n,))
            c.also.append(pool)
            c.issue = lambda s: ctx.call("dvsg_stabilize_ring_inplace_f32", h, code, pool.data_ptr(), n_pool, table.data_ptr(),
                                         slots.data_ptr(), B, H, W, F.data_ptr(), xs.data_ptr(), ys.data_ptr(), ws, nb, s)
        elif kind in ("forward_ring", "forward_masked"):
            dims = (ctypes.c_int * 3)()
            c.keep.append(dims)
            if src == 0:
                x = c.inp(uni((B, H, W, 21), salt=1))
                n_pool, table = 0, None
            else:
                x, n_pool, table = _ring(c, B, H, W, src == 2, 11)
            out = c.out((B * 50 if stage < 0 else _tap_cap(B, H, W),))
            tp = table.data_ptr() if table is not None else None
            if kind == "forward_ring":
                c.issue = lambda s: ctx.call("dvsg_locnet_forward_ring", h, code, x.data_ptr(), int(src == 2), n_pool, tp, B, H,
                                             W, stage, out.data_ptr(), out.numel() * 4, dims, ws, nb, s)
            else:
                m = _mask(c, B, H, W, 13)
                c.issue = lambda s: ctx.call("dvsg_locnet_forward_masked", h, code, x.data_ptr(), src, n_pool, tp,
                                             m.data_ptr(), B, H, W, stage, out.data_ptr(), out.numel() * 4, dims, ws, nb, s)
        else:
            raise AssertionError(kind)
        return c
    return build


def _register_network():
    main, ragged = NET_SHAPES
    for shape in NET_SHAPES:
        sid = "%dx%dx%d" % shape
        # the ragged shape: every precision of forward, stabilize and the last tap; the other forms in float32
        precs_all = PRECISIONS
        precs = PRECISIONS if shape == main else ("f32",)
        for p in precs_all:
            case("dvsg_locnet_forward_" + p, sid)(net_case("forward", p, *shape))
            case("dvsg_stabilize_" + p, sid)(net_case("stabilize", p, *shape))
            for st in (TAP_STAGES if shape == main else TAP_STAGES[-1:]):
                case("dvsg_locnet_forward_tap_" + p, "%s-stage%d" % (sid, st))(net_case("tap", p, *shape, stage=st))
        for p in precs:
            tag = "%s-%s" % (p, sid)
            case("dvsg_stabilize_ring_f32", tag)(net_case("ring_f32", p, *shape))
            case("dvsg_stabilize_ring_u8", tag)(net_case("ring_u8", p, *shape))
            case("dvsg_stabilize_ring_inplace_f32", tag)(net_case("inplace", p, *shape))
            case("dvsg_stabilize_masked_f32", tag)(net_case("masked", p, *shape))
            case("dvsg_stabilize_ring_masked_f32", tag)(net_case("ring_masked_f32", p, *shape))
            case("dvsg_stabilize_ring_masked_u8", tag)(net_case("ring_masked_u8", p, *shape))
            case("dvsg_locnet_forward_ring", tag + "-f32pool-F")(net_case("forward_ring", p, *shape, stage=-1, src=1))
            case("dvsg_locnet_forward_ring", tag + "-u8pool-stage1")(net_case("forward_ring", p, *shape, stage=1, src=2))
            case("dvsg_locnet_forward_masked", tag + "-window-F")(net_case("forward_masked", p, *shape, stage=-1, src=0))
            case("dvsg_locnet_forward_masked", tag + "-f32pool-stage0")(net_case("forward_masked", p, *shape, stage=0, src=1))
            case("dvsg_locnet_forward_masked", tag + "-u8pool-stage1")(net_case("forward_masked", p, *shape, stage=1, src=2))


_register_network()


# ---------------------------------------------------------------------------------------------------------------------
# TPS, flow and spatial transformers
# ---------------------------------------------------------------------------------------------------------------------
def _crop_case(i):
    import test_gpu_crop as crop
    return crop.CASES[i]


def _coord_T(c, cs, salt=0):
    """coord [B,P,2] and a solved near-identity T [B,2,P+3] of a tests/test_gpu_crop.py case, T fresh per seed"""
    import test_gpu_crop as crop
    coord = c.inp(fixed(crop.case_T("near", cs)[0]))
    T = c.inp(lambda seed: _t(crop.case_T("near", cs, seed=seed + salt)[1]))
    return coord, T


@case("dvsg_tps_solve_f32")
def _solve(ctx):
    import test_tps_f64 as tps
    c, B, P = Case(), 3, 25
    coord = c.inp(lambda seed: _t(tps.control_points(P, B, True, seed=seed)))
    rhs = c.inp(vectors(B, 1))
    T = c.out((B, 2, P + 3))
    c.issue = lambda s: ctx.call("dvsg_tps_solve_f32", coord.data_ptr(), rhs.data_ptr(), 1, B, P, T.data_ptr(), s)
    return c


@case("dvsg_tps_solve_checked_f32")
def _solve_checked(ctx):
    import test_tps_f64 as tps
    c, B, P = Case(), 3, 25

    def coords(seed):   # sample 1 repeats a control point: its system is singular and counted
        a = tps.control_points(P, B, True, seed=seed)
        a[1, 3] = a[1, 2]
        return _t(a)
    coord = c.inp(coords)
    rhs = c.inp(vectors(B, 1))
    T = c.out((B, 2, P + 3))
    n_sing = c.st(_torch().full((1,), 5, dtype=_torch().int32, device="cuda"))    # ADDED to: 5 -> 6
    c.issue = lambda s: ctx.call("dvsg_tps_solve_checked_f32", coord.data_ptr(), rhs.data_ptr(), 1, B, P, T.data_ptr(),
                                 n_sing.data_ptr(), s)
    return c


def _warp_builder(zoomed, i):
    def build(ctx):
        import test_gpu_crop as crop
        c = Case()
        cs = _crop_case(i)
        oh, ow, sh, sw, B, P = cs
        coord, T = _coord_T(c, cs)
        U = c.inp(uni((B, sh, sw, 3), -1.0, 1.0, 5))
        out, xs, ys = c.out((B, oh, ow, 3)), c.out((B * oh * ow,)), c.out((B * oh * ow,))
        if zoomed:
            z = c.inp(fixed(crop.ZOOMS[:B]))
            c.issue = lambda s: ctx.call("dvsg_tps_warp_zoom_f32", U.data_ptr(), coord.data_ptr(), T.data_ptr(), z.data_ptr(),
                                         B, sh, sw, 3, P, oh, ow, out.data_ptr(), xs.data_ptr(), ys.data_ptr(), s)
        else:
            c.issue = lambda s: ctx.call("dvsg_tps_warp_f32", U.data_ptr(), coord.data_ptr(), T.data_ptr(), B, sh, sw, 3, P, oh,
                                         ow, out.data_ptr(), xs.data_ptr(), ys.data_ptr(), s)
        return c
    return build


for _i in (1, 2):
    case("dvsg_tps_warp_f32", "crop%d" % _i)(_warp_builder(False, _i))
    case("dvsg_tps_warp_zoom_f32", "crop%d" % _i)(_warp_builder(True, _i))


def _coverage_builder(i):
    def build(ctx):
        import test_gpu_crop as crop
        c = Case()
        cs = _crop_case(i)
        oh, ow, sh, sw, B, P = cs
        coord, T = _coord_T(c, cs)
        z = c.inp(fixed(crop.ZOOMS[:B]))
        nb, km = c.out((B,), _torch().int32), c.out((B,), _torch().int32)
        ws, wb = c.work(crop.cover_bytes(B, oh, ow))
        c.issue = lambda s: ctx.call("dvsg_tps_coverage_f32", coord.data_ptr(), T.data_ptr(), z.data_ptr(), B, P, sh, sw, oh, ow,
                                     nb.data_ptr(), km.data_ptr(), ws, wb, s)
        return c
    return build


for _i in (1, 2):
    case("dvsg_tps_coverage_f32", "crop%d" % _i)(_coverage_builder(_i))


def _coverage_net_builder(label=""):
    def build(ctx, n=3):
        import test_gpu_crop as crop
        torch = _torch()
        c = Case()
        oh, ow, sh, sw = 8, crop.KT + 3, 9, 300        # the grid and source of crop.CASES[2]
        F = c.inp(vectors(n, 3, scale=0.08))
        z = c.inp(fixed(crop.ZOOMS[:n]))

        def call(handle, T, nb, km, ws, wb):
            return lambda s: ctx.call("dvsg_tps_coverage_net_f32", handle, F.data_ptr(), z.data_ptr(), n, sh, sw, oh, ow,
                                      T.data_ptr(), nb.data_ptr(), km.data_ptr(), ws, wb, s)
        T = c.out((n, 2, 28))
        nb, km = c.out((n,), torch.int32), c.out((n,), torch.int32)
        c.issue = call(ctx.view(label), T, nb, km, *c.work(crop.cover_bytes(n, oh, ow)))
        if label:   # the counts of a coarse grid need not move with the seed or the shape: T is what is held to both
            plain = [torch.empty_like(t) for t in (T, nb, km)]
            c.view = ViewCheck(label, call(ctx.h, *(plain + list(c.work(crop.cover_bytes(n, oh, ow))))), plain, fresh=(0,))
        return c
    return build


_coverage_net = _coverage_net_builder()
case("dvsg_tps_coverage_net_f32")(_coverage_net)
case("dvsg_tps_coverage_net_f32", "shaped")(_coverage_net_builder("shaped"))


def _coefficients_builder(label=""):
    def build(ctx):
        c, n = Case(), 3
        F = c.inp(vectors(n, 4))
        T, h = c.out((n, 2, 28)), ctx.view(label)
        c.issue = lambda s: ctx.call("dvsg_tps_coefficients_f32", h, F.data_ptr(), n, T.data_ptr(), s)
        if label:
            pT = _torch().empty_like(T)
            c.view = ViewCheck(label, lambda s: ctx.call("dvsg_tps_coefficients_f32", ctx.h, F.data_ptr(), n, pT.data_ptr(), s),
                               [pT])
        return c
    return build


case("dvsg_tps_coefficients_f32")(_coefficients_builder())
case("dvsg_tps_coefficients_f32", "shaped")(_coefficients_builder("shaped"))


@case("dvsg_crop_ratchet_f32")
def _ratchet(ctx):
    torch = _torch()
    c, n, n_state, Da, Db = Case(), 3, 5, 36 * 52, 17 * 25
    ka = c.inp(ints((n,), 0, 2 * Da, 1))
    kb = c.inp(ints((n,), 0, 2 * Db, 2))
    slots = c.inp(fixed(np.array([4, 9, 1], dtype=np.int32)))       # 9: outside [0, n_state), that frame is skipped
    state = c.st(_t(np.array([1.0, 0.75, 0.5, 0.25, 0.9], dtype=np.float32)))
    zoom, free = c.out((n,)), c.out((n,), torch.float64)
    c.issue = lambda s: ctx.call("dvsg_crop_ratchet_f32", ka.data_ptr(), Da, kb.data_ptr(), Db, slots.data_ptr(), n,
                                 state.data_ptr(), n_state, 0.02, 0.5, 0.01, zoom.data_ptr(), free.data_ptr(), s)
    return c


@case("dvsg_flow_warp_f32")
def _flow(ctx):
    c = Case()
    B, H, W = LOSS
    im = c.inp(uni((B, H, W, 3), salt=1))
    flow = c.inp(uni((B, H, W, 2), -6.0, 6.0, 2))
    out = c.out((B, H, W, 3))
    c.issue = lambda s: ctx.call("dvsg_flow_warp_f32", im.data_ptr(), flow.data_ptr(), B, H, W, 3, out.data_ptr(), s)
    return c


@case("dvsg_stn_sample_f32")
def _stn_sample(ctx):
    c = Case()
    B, H, W, oh, ow = 3, 33, 65, 20, 31
    im = c.inp(uni((B, H, W, 3), salt=1))
    xs = c.inp(uni((B * oh * ow,), -1.1, 1.1, 2))
    ys = c.inp(uni((B * oh * ow,), -1.1, 1.1, 3))
    out = c.out((B, oh, ow, 3))
    c.issue = lambda s: ctx.call("dvsg_stn_sample_f32", im.data_ptr(), xs.data_ptr(), ys.data_ptr(), B, H, W, 3, oh, ow,
                                 out.data_ptr(), s)
    return c


def _grid_builder(name):
    def build(ctx):
        c = Case()
        B, H, W, oh, ow = 3, 33, 65, 20, 31
        im = c.inp(uni((B, H, W, 3), salt=1))
        out, xs, ys = c.out((B, oh, ow, 3)), c.out((B * oh * ow,)), c.out((B * oh * ow,))
        if name == "dvsg_grid_affine_f32":
            ident = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)
            th = c.inp(lambda seed: _t((ident + _rng(seed, 7).uniform(-0.1, 0.1, (B, 6))).astype(np.float32)))
        else:
            th = c.inp(lambda seed: _t(inputs.mask_homographies(seed + 70, B)))
        c.issue = lambda s: ctx.call(name, th.data_ptr(), im.data_ptr(), B, H, W, 3, oh, ow, out.data_ptr(), xs.data_ptr(),
                                     ys.data_ptr(), s)
        return c
    return build


case("dvsg_grid_affine_f32")(_grid_builder("dvsg_grid_affine_f32"))
case("dvsg_grid_projective_f32")(_grid_builder("dvsg_grid_projective_f32"))


@case("dvsg_grid_elastic_f32")
def _elastic(ctx):
    c = Case()
    B, H, W, oh, ow, g = 3, 33, 65, 20, 31, 4
    n = g * g
    src = np.empty((2, n), np.float32)
    linv = np.empty((n, n + 3), np.float32)
    ctx.call("dvsg_elastic_constants_f32", g, src.ctypes.data, linv.ctypes.data)
    d_src, d_linv = c.inp(fixed(src)), c.inp(fixed(linv))
    th = c.inp(lambda seed: _t((src[None] + _rng(seed, 9).uniform(-0.05, 0.05, (B, 2, n))).astype(np.float32)))
    im = c.inp(uni((B, H, W, 3), salt=1))
    out, xs, ys = c.out((B, oh, ow, 3)), c.out((B * oh * ow,)), c.out((B * oh * ow,))
    c.issue = lambda s: ctx.call("dvsg_grid_elastic_f32", th.data_ptr(), d_linv.data_ptr(), d_src.data_ptr(), n, im.data_ptr(),
                                 B, H, W, 3, oh, ow, out.data_ptr(), xs.data_ptr(), ys.data_ptr(), s)
    return c


@case("dvsg_scale_rgb_f32")
def _scale_rgb(ctx):
    c = Case()
    B, H, W, C = 2, 37, 53, 6
    x = c.inp(uni((B, H, W, C), salt=1))
    out = c.out((B, H, W, C))
    c.issue = lambda s: ctx.call("dvsg_scale_rgb_f32", x.data_ptr(), B, H, W, C, out.data_ptr(), s)
    return c


@case("dvsg_random_mask_plane_f32")
def _mask_plane(ctx):
    c = Case()
    B, H, W = 3, 33, 47
    th = c.inp(lambda seed: _t(inputs.mask_homographies(seed + 30, B)))
    m = c.out((B, H, W))
    c.issue = lambda s: ctx.call("dvsg_random_mask_plane_f32", th.data_ptr(), B, H, W, m.data_ptr(), s)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone convolutions: a 3x3 launch of 2 x 6 x 10 pixels, few enough tiles that K is split over workgroups, so the
# tickets in `scratch` are zeroed and used by every call
# ---------------------------------------------------------------------------------------------------------------------
CONV = dict(B=2, h=6, w=10, cin=128, cout=128, k=3, stride=1)


def _conv_w(seed=5):
    cin, cout, k = CONV["cin"], CONV["cout"], CONV["k"]
    K = k * k * cin
    rng = np.random.default_rng(seed)
    return ((rng.uniform(-0.5, 0.5, (cout, K))) * (2.0 / K ** 0.5)).astype(np.float32), \
        rng.uniform(-0.5, 0.5, (cout,)).astype(np.float32)


def _pieces_of_weights(w):
    """[Cout][K/32][32 hi | 32 lo] float16, hi = f16(w), lo = f16(w - hi) (dvsg_conv_gemm_f32s)"""
    torch = _torch()
    w = _t(w)
    hi = w.half()
    lo = (w - hi.float()).half()
    co, K = w.shape
    return torch.cat([hi.view(co, K // 32, 32), lo.view(co, K // 32, 32)], dim=2).contiguous()


def _split_of_weights(w):
    """[Cout/64][128][K] float16: 64 rows of hi = f16(w), then 64 rows of lo = f16((w - hi) * 2048) (dvsg_conv_gemm_f16s)"""
    torch = _torch()
    w = _t(w)
    hi = w.half()
    lo = ((w - hi.float()) * 2048.0).half()
    co, K = w.shape
    return torch.cat([hi.view(co // 64, 64, K), lo.view(co // 64, 64, K)], dim=1).contiguous()


def _conv_builder(name):
    def build(ctx):
        torch = _torch()
        c = Case()
        B, h, w, cin, cout, k, stride = (CONV[n] for n in ("B", "h", "w", "cin", "cout", "k", "stride"))
        wt, bias = _conv_w()
        scr = ctx.scratch()
        half = name in ("dvsg_conv_gemm_f16", "dvsg_conv_gemm_f16s")

        def act(shape, salt):   # an activation tensor in the entry's own format, fresh per seed
            g = uni(shape, -0.3, 0.7, salt)
            if half:
                return lambda seed: g(seed).half()
            if name == "dvsg_conv_gemm_f32s":
                def pieces(seed):
                    x = g(seed)
                    y = torch.empty_like(x)
                    ctx.call("dvsg_f32_to_pieces", x.data_ptr(), y.data_ptr(), x.numel(), ctx.cur())
                    return y
                return pieces
            return g
        x = c.inp(act((B, h, w, cin), 1))
        res = c.inp(act((B, h, w, cout), 2))
        y = c.out((B, h, w, cout), torch.float16 if half else torch.float32)
        b = c.inp(fixed(bias))
        if name == "dvsg_conv_gemm_f32":
            wd = c.inp(fixed(wt))
        elif name == "dvsg_conv_gemm_f16":
            wd = _t(wt).half()
        elif name == "dvsg_conv_gemm_f32s":
            wd = _pieces_of_weights(wt)
        elif name == "dvsg_conv_gemm_f16s":
            wd = _split_of_weights(wt)
        else:
            wd = torch.empty(6 * wt.size, dtype=torch.uint8, device="cuda")
            w32 = _t(wt)
            ctx.call("dvsg_pack_weights_f32x3", w32.data_ptr(), wd.data_ptr(), cout, wt.shape[1], ctx.cur())
            torch.cuda.synchronize()
        c.keep.append(wd)
        c.issue = lambda s: ctx.call(name, x.data_ptr(), wd.data_ptr(), b.data_ptr(), res.data_ptr(), y.data_ptr(), B, h, w, cin,
                                     cout, k, stride, 1, 1, scr.data_ptr(), scr.numel(), s)
        return c
    return build


for _n in ("dvsg_conv_gemm_f32", "dvsg_conv_gemm_f32s", "dvsg_conv_gemm_f32x3", "dvsg_conv_gemm_f16", "dvsg_conv_gemm_f16s"):
    case(_n)(_conv_builder(_n))


def _fused_builder(name):
    """block 1's conv2 + conv3 at tests/test_gpu_cnn.py's stride-2 case with the subsampled residual"""
    def build(ctx):
        torch = _torch()
        c = Case()
        B, h, w, cin, cout, stride, rs = 1, 37, 53, 64, 256, 2, 2
        rng = np.random.default_rng(17)
        w2 = (rng.uniform(-0.5, 0.5, (64, 9 * cin)) * (2.0 / (9 * cin) ** 0.5)).astype(np.float32)
        w3 = (rng.uniform(-0.5, 0.5, (cout, 64)) * 0.25).astype(np.float32)
        b2, b3 = c.inp(fixed(rng.uniform(-0.5, 0.5, 64).astype(np.float32))), \
            c.inp(fixed(rng.uniform(-0.5, 0.5, cout).astype(np.float32)))
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        x = c.inp(uni((B, h, w, cin), -0.3, 0.7, 1))
        res = c.inp(uni((B, (ho - 1) * rs + 1, (wo - 1) * rs + 1, cout), -0.5, 0.5, 2))
        y = c.out((B, ho, wo, cout))
        d2, d3 = _t(w2), _t(w3)
        if name == "dvsg_conv3x3_1x1_f32x3":
            p2 = torch.empty(6 * w2.size, dtype=torch.uint8, device="cuda")
            p3 = torch.empty(6 * w3.size, dtype=torch.uint8, device="cuda")
            ctx.call("dvsg_pack_weights_f32x3", d2.data_ptr(), p2.data_ptr(), 64, w2.shape[1], ctx.cur())
            ctx.call("dvsg_pack_weights_f32x3", d3.data_ptr(), p3.data_ptr(), cout, 64, ctx.cur())
            torch.cuda.synchronize()
            d2, d3 = p2, p3
        c.keep += [d2, d3]
        if name == "dvsg_debug_conv3x3_1x1":
            c.issue = lambda s: ctx.call(name, 0, x.data_ptr(), d2.data_ptr(), b2.data_ptr(), d3.data_ptr(), b3.data_ptr(),
                                         res.data_ptr(), None, None, None, 0, y.data_ptr(), B, h, w, cin, cout, stride, rs, s)
        else:
            c.issue = lambda s: ctx.call(name, x.data_ptr(), d2.data_ptr(), b2.data_ptr(), d3.data_ptr(), b3.data_ptr(),
                                         res.data_ptr(), y.data_ptr(), B, h, w, cin, cout, stride, rs, s)
        return c
    return build


for _n in ("dvsg_conv3x3_1x1_f32", "dvsg_conv3x3_1x1_f32x3", "dvsg_debug_conv3x3_1x1"):
    case(_n)(_fused_builder(_n))


@case("dvsg_pack_weights_f32x3")
def _pack(ctx):
    c, cout, K = Case(), 64, 288
    w = c.inp(uni((cout, K), -1.0, 1.0, 1))
    out = c.out((6 * cout * K,), _torch().uint8)
    c.issue = lambda s: ctx.call("dvsg_pack_weights_f32x3", w.data_ptr(), out.data_ptr(), cout, K, s)
    return c


def _pieces_builder(name):
    def build(ctx):
        c, n = Case(), 32 * 331
        if name == "dvsg_f32_to_pieces":
            x = c.inp(uni((n,), -2.0, 2.0, 1))
        else:   # 2 n float16 pieces: per 128-byte group 32 hi halves, then 32 lo halves
            x = c.inp(lambda seed: uni((2 * n,), -2.0, 2.0, 1)(seed).half())
        y = c.out((n,))
        c.issue = lambda s: ctx.call(name, x.data_ptr(), y.data_ptr(), n, s)
        return c
    return build


case("dvsg_f32_to_pieces")(_pieces_builder("dvsg_f32_to_pieces"))
case("dvsg_pieces_to_f32")(_pieces_builder("dvsg_pieces_to_f32"))


# ---------------------------------------------------------------------------------------------------------------------
# frame formats, rings, renders
# ---------------------------------------------------------------------------------------------------------------------
def _u8_frames(n, H, W, salt):
    return ints((n, H, W, 3), 0, 256, salt, np.uint8)


@case("dvsg_frames_u8_to_f32")
def _u8_to_f32(ctx):
    c = Case()
    n_pix = 2 * SRC[0] * SRC[1]
    src = c.inp(ints((n_pix * 3,), 0, 256, 1, np.uint8))
    dst = c.out((n_pix * 3,))
    c.issue = lambda s: ctx.call("dvsg_frames_u8_to_f32", src.data_ptr(), n_pix, 1, dst.data_ptr(), s)
    return c


@case("dvsg_frames_resize_u8_f32")
def _resize(ctx):
    c, n = Case(), 2
    (h, w), (H0, W0) = SRC, (68, 102)
    src = c.inp(_u8_frames(n, H0, W0, 1))
    dst = c.out((n, h, w, 3))
    u8 = c.out((n, h, 2 * w, 3), _torch().uint8)
    c.issue = lambda s: ctx.call("dvsg_frames_resize_u8_f32", src.data_ptr(), n, H0, W0, 1, dst.data_ptr(), h, w, u8.data_ptr(),
                                 2 * w, w, s)
    return c


@case("dvsg_window_gather_f32")
def _gather(ctx):
    c, n_pool, B = Case(), 9, 3
    h, w = SRC
    pool = c.inp(uni((n_pool, h, w, 3), salt=1))
    idx = c.inp(ints((B * 7,), -1, n_pool + 1, 2))       # -1 and n_pool read as frames of zeros
    out = c.out((B, h, w, 21))
    c.issue = lambda s: ctx.call("dvsg_window_gather_f32", pool.data_ptr(), n_pool, h, w, idx.data_ptr(), B, 7, out.data_ptr(), s)
    return c


def _ingest_builder(resized):
    def build(ctx):
        c, n, n_pool = Case(), 3, 5
        h, w = SRC
        H0, W0 = (68, 102) if resized else SRC
        src = c.inp(_u8_frames(n, H0, W0, 1))
        slots = c.inp(fixed(np.array([4, 0, n_pool + 3], dtype=np.int32)))     # the last: out of range, skipped
        pool = c.out((n_pool, h, w, 3))
        u8 = c.out((n, h, 2 * w, 3), _torch().uint8) if resized else None
        up = u8.data_ptr() if resized else None
        c.issue = lambda s: ctx.call("dvsg_frames_ingest_u8", src.data_ptr(), n, H0, W0, 1, pool.data_ptr(), n_pool,
                                     slots.data_ptr(), h, w, up, 2 * w if resized else 0, 0, s)
        return c
    return build


case("dvsg_frames_ingest_u8", "same-size")(_ingest_builder(False))
case("dvsg_frames_ingest_u8", "resized")(_ingest_builder(True))


@case("dvsg_frames_f32_to_u8_slots")
def _to_u8_slots(ctx):
    c, n, n_pool = Case(), 3, 5
    h, w = SRC
    pool = c.inp(uni((n_pool, h, w, 3), -0.1, 1.1, 1))
    slots = c.inp(fixed(np.array([4, -2, 1], dtype=np.int32)))
    dst = c.out((n, h, 2 * w, 3), _torch().uint8)
    c.issue = lambda s: ctx.call("dvsg_frames_f32_to_u8_slots", pool.data_ptr(), n_pool, slots.data_ptr(), n, h, w, 1,
                                 dst.data_ptr(), 2 * w, w, s)
    return c


def _to_u8_builder(name, dtype):
    def build(ctx):
        c, n = Case(), 2
        h, w = SRC
        src = c.inp(uni((n, h, w, 3), -0.1, 1.1, 1, dtype))
        dst = c.out((n, h, 2 * w, 3), _torch().uint8)
        c.issue = lambda s: ctx.call(name, src.data_ptr(), n, h, w, 0, dst.data_ptr(), 2 * w, w, s)
        return c
    return build


case("dvsg_frames_f32_to_u8")(_to_u8_builder("dvsg_frames_f32_to_u8", np.float32))
case("dvsg_frames_f64_to_u8")(_to_u8_builder("dvsg_frames_f64_to_u8", np.float64))


def _render_u8_builder(zoomed, F=None, label=""):
    """The RGB render of SRC frames through the view of `label` ("": the plain handle): out_f32 [n, oh, ow, 3] and out_u8 in
    the right half of rows of 2 ow pixels, (oh, ow) the view's size or the source's."""
    def build(ctx):
        import test_gpu_crop as crop
        torch = _torch()
        c, n = Case(), 3
        H0, W0 = SRC
        oh, ow = VIEWS.get(label, {}).get("out_size") or SRC
        Fd = F if F is not None else c.inp(vectors(n, 5))
        src = c.inp(_u8_frames(n, H0, W0, 1))
        z = c.inp(fixed(crop.ZOOMS[:n])) if zoomed else None

        def outs(h, w, alloc):
            return alloc((n, 2, 28), torch.float32), alloc((n, h, w, 3), torch.float32), alloc((n, h, 2 * w, 3), torch.uint8)

        def call(handle, T, o32, o8):
            w = o32.shape[2]
            if zoomed:
                return lambda s: ctx.call("dvsg_tps_render_zoom_u8", handle, Fd.data_ptr(), src.data_ptr(), n, H0, W0, 1,
                                          z.data_ptr(), T.data_ptr(), o32.data_ptr(), o8.data_ptr(), 2 * w, w, s)
            return lambda s: ctx.call("dvsg_tps_render_u8", handle, Fd.data_ptr(), src.data_ptr(), n, H0, W0, 1, T.data_ptr(),
                                      o32.data_ptr(), o8.data_ptr(), 2 * w, w, s)
        c.issue = call(ctx.view(label), *outs(oh, ow, c.out))
        if label:
            assert ctx.render_size(ctx.view(label)) == (VIEWS[label].get("out_size") or (0, 0))
            # the plain handle writes source-size frames: a scaled view is compared with their top left (oh, ow) pixels
            plain = outs(H0, W0, lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda"))
            c.view = ViewCheck(
                label, call(ctx.h, *plain), plain,
                pairs=lambda w: [(w[1], plain[1][:, :oh, :ow]), (w[2][:, :, ow:], plain[2][:, :oh, W0:W0 + ow])],
                kept=(lambda w: [("out_f32", w[1]), ("out_u8", w[2][:, :, ow:])]) if VIEWS[label].get("border") == "keep" else None)
        return c
    return build


case("dvsg_tps_render_u8")(_render_u8_builder(False))
case("dvsg_tps_render_zoom_u8")(_render_u8_builder(True))
for _l in RGB_VIEWS:
    case("dvsg_tps_render_u8", _l)(_render_u8_builder(False, label=_l))
    case("dvsg_tps_render_zoom_u8", _l)(_render_u8_builder(True, label=_l))


def _nv12_in(c, n, H, W, pitch, uv_row, salt):
    import nv12_ref
    b = nv12_ref.Batch(0, n, H, W, pitch, uv_row)
    buf = c.inp(lambda seed: _t(nv12_ref.Batch(31 * seed + salt, n, H, W, pitch, uv_row).buf))
    return b, buf


@case("dvsg_frames_nv12_to_rgb_u8")
def _nv12_convert(ctx):
    c, n = Case(), 2
    H, W = NV
    b, buf = _nv12_in(c, n, H, W, 64, 40, 1)
    dst = c.out((n, H, W, 3), _torch().uint8)
    c.issue = lambda s: ctx.call("dvsg_frames_nv12_to_rgb_u8", buf.data_ptr(), buf.data_ptr() + b.uv_offset, b.pitch,
                                 b.frame_stride, n, H, W, 1, 1, dst.data_ptr(), s)
    return c


def _nv12_ingest_builder(resized):
    def build(ctx):
        c, n, n_pool = Case(), 3, 5
        h, w = NV
        H0, W0, pitch, uv_row = (68, 102, 128, 72) if resized else (h, w, 64, 40)     # tests/test_gpu_nv12.py's layouts
        b, buf = _nv12_in(c, n, H0, W0, pitch, uv_row, 2)
        slots = c.inp(fixed(np.array([4, n_pool + 3, 2], dtype=np.int32)))
        pool = c.out((n_pool, h, w, 3))
        c.issue = lambda s: ctx.call("dvsg_frames_ingest_nv12", buf.data_ptr(), buf.data_ptr() + b.uv_offset, b.pitch,
                                     b.frame_stride, n, H0, W0, 0, pool.data_ptr(), n_pool, slots.data_ptr(), h, w, s)
        return c
    return build


case("dvsg_frames_ingest_nv12", "same-size")(_nv12_ingest_builder(False))
case("dvsg_frames_ingest_nv12", "resized")(_nv12_ingest_builder(True))


def _surface(label, seed, n, H, W, pitch, uv_row, fill=None):
    """A batch of the frames the view of `label` reads and writes: nv12_ref.Batch, p010_ref.P010Batch or, for a 4:2:2 view,
    yuv422_ref.Batch422 of bytes or words."""
    kw = VIEWS.get(label, {})
    words = kw.get("surface", "nv12") == "p010"
    if kw.get("chroma", "420") == "422":
        import yuv422_ref
        return yuv422_ref.Batch422(seed, n, H, W, words, pitch, uv_row, fill=fill)
    if words:
        import p010_ref
        return p010_ref.P010Batch(seed, n, H, W, pitch, uv_row, fill=fill)
    import nv12_ref
    return nv12_ref.Batch(seed, n, H, W, pitch, uv_row, fill=fill)


def _surface_source(label, seed, n=3):
    """SURF frames for the view of `label`: packed bytes as the plain cases read them, words with a row gap and a plane gap"""
    H, W = SURF
    words = VIEWS.get(label, {}).get("surface", "nv12") == "p010"
    return _surface(label, seed, n, H, W, 2 * W + 4 if words else W, H + 2 if words else H)


def _shared_surface(label="", n=3):
    """one source buffer for two calls of a pair: not an input of either, so neither refills it -> (batch, device bytes)"""
    b = _surface_source(label, 77, n)
    return b, _t(b.buf)


def _render_nv12_builder(zoomed, F=None, label="", src=None):
    """The surface render of SURF frames through the view of `label` ("": the plain handle).  The label gives the sample
    (bytes, or P010 words), the chroma rows (H / 2, or H for 4:2:2) and the size of the frames written; the output has 26
    bytes behind every row and 4 rows between the planes, poisoned like the planes themselves."""
    def build(ctx):
        import test_gpu_crop as crop
        torch = _torch()
        c, n = Case(), 3
        H, W = SURF
        kw = VIEWS.get(label, {})
        oh, ow = kw.get("out_size") or SURF
        bps = 2 if kw.get("surface", "nv12") == "p010" else 1
        if src is None:
            b = _surface_source(label, 0)
            buf = c.inp(lambda seed: _t(_surface_source(label, 31 * seed + 3).buf))
        else:
            b, buf = src
        Fd = F if F is not None else c.inp(vectors(n, 6))
        z = c.inp(fixed(crop.ZOOMS[:n])) if zoomed else None

        def call(handle, T, out, ob):
            if zoomed:
                return lambda s: ctx.call("dvsg_tps_render_zoom_nv12", handle, Fd.data_ptr(), buf.data_ptr(),
                                          buf.data_ptr() + b.uv_offset, b.pitch, b.frame_stride, n, H, W, z.data_ptr(),
                                          T.data_ptr(), out.data_ptr(), out.data_ptr() + ob.uv_offset, ob.pitch, ob.frame_stride, s)
            return lambda s: ctx.call("dvsg_tps_render_nv12", handle, Fd.data_ptr(), buf.data_ptr(),
                                      buf.data_ptr() + b.uv_offset, b.pitch, b.frame_stride, n, H, W, T.data_ptr(),
                                      out.data_ptr(), out.data_ptr() + ob.uv_offset, ob.pitch, ob.frame_stride, s)
        ob = _surface(label, 0, n, oh, ow, bps * ow + 26, oh + 4, fill=POISON)
        T = c.out((n, 2, 28))
        out = c.out(ob.buf.shape, torch.uint8)
        c.issue = call(ctx.view(label), T, out, ob)
        if label:
            import nv12_ref
            assert ctx.render_size(ctx.view(label)) == (kw.get("out_size") or (0, 0))
            # The plain handle on the same bytes: it reads them as NV12 (fewer bytes of every row, fewer chroma rows) and writes
            # an NV12 frame of SURF.  At the source's size that fits the view's own output layout, so the two outputs are
            # compared whole; of a scaled view the first ow bytes of the oh luma rows are compared with those of a source-size
            # NV12 output.
            scaled = (oh, ow) != SURF
            pb = nv12_ref.Batch(0, n, H, W, W + 26, H + 4, fill=POISON) if scaled else ob
            pT, p_out = torch.empty_like(T), torch.empty(pb.buf.shape, dtype=torch.uint8, device="cuda")
            c.view = ViewCheck(
                label, call(ctx.h, pT, p_out, pb), [pT, p_out],
                pairs=(lambda w: [(w[1][:, :oh, :ow], p_out[:, :oh, :ow])]) if scaled else (lambda w: [(w[1], p_out)]),
                kept=(lambda w: [("luma", w[1][:, :oh, :bps * ow]), ("chroma", w[1][:, ob.uv_row:, :bps * ow])])
                if kw.get("border") == "keep" else None)
        return c
    return build


case("dvsg_tps_render_nv12")(_render_nv12_builder(False))
case("dvsg_tps_render_zoom_nv12")(_render_nv12_builder(True))
for _l in SURFACE_VIEWS:
    case("dvsg_tps_render_nv12", _l)(_render_nv12_builder(False, label=_l))
    case("dvsg_tps_render_zoom_nv12", _l)(_render_nv12_builder(True, label=_l))


@case("dvsg_scene_step_f32")
def _scene(ctx):
    """tests/test_gpu_scene.py's (37, 53, 3) case: three consecutive steps that carry `state` and the zoom state; the input
    slots change between the steps from one luma band to a disjoint one and back, so the steps cut."""
    import scene_ref
    import test_gpu_scene as scene
    torch = _torch()
    c = Case()
    c.carry = True
    H, W, B = SCENE
    skip = scene.SKIP
    S, span = len(skip), skip[-1]
    per = span + 2
    n_state = B + 2
    n_pool = (B + 1) * per
    rings_h = np.array([2, 0, 1, n_state + 5], dtype=np.int32)        # the last: outside [0, n_state), a row of -1
    rows = rings_h.size

    def pool_of(seed):
        rng = _rng(seed, 3)
        pool = np.full((n_pool, H, W, 3), 0.25, dtype=np.float32)
        for i in range(B):   # seeds alternate the luma band of every other ring
            lo = 0.65 if (seed + i) % 2 else 0.0
            pool[rings_h[i] * per + span + 1] = scene._frame(rng, H, W, lo, "wild" if i == 1 else None)
        return _t(pool)
    pool = c.inp(pool_of)
    rings = c.inp(fixed(rings_h))
    state0 = np.zeros((n_state, 68), dtype=np.int32)
    state0[2, :4] = (5, 2, 17, 0)                                     # ring 2 starts in mid-run
    state0[2, 4:] = np.random.default_rng(1).multinomial(H * W, np.ones(64) / 64.0)
    state0[3:] = 12345                                                # rows no call may touch
    state = c.st(_t(state0))
    zoom = c.st(_t((0.5 + 0.01 * np.arange(n_state)).astype(np.float32)))
    table = c.out((rows, S), torch.int32)
    out_slots, cut = c.out((rows,), torch.int32), c.out((rows,), torch.int32)
    need = ctypes.c_size_t()
    ctx.call("dvsg_scene_workspace_bytes", rows, ctypes.byref(need))
    ws, wb = c.work(need.value)
    c_skip = (ctypes.c_int32 * S)(*skip)
    c.keep.append(c_skip)
    thr = scene_ref.threshold_count(0.5, H, W)
    c.issue = lambda s: ctx.call("dvsg_scene_step_f32", pool.data_ptr(), n_pool, H, W, rings.data_ptr(), rows, c_skip, S,
                                 state.data_ptr(), n_state, thr, 1, zoom.data_ptr(), 0.875, table.data_ptr(),
                                 out_slots.data_ptr(), cut.data_ptr(), ws, wb, s)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------
def _loss_ws(ctx, c):
    B, H, W = LOSS
    need = ctypes.c_size_t()
    ctx.call("dvsg_loss_workspace_bytes", B, H, W, ctypes.byref(need))
    return c.work(need.value)


@case("dvsg_loss_image_f32")
def _loss_image(ctx):
    torch = _torch()
    c = Case()
    B, H, W = LOSS
    coord, T = _coord_T(c, (H, W, H, W, B, 25))
    U, gt = c.inp(uni((B, H, W, 3), salt=1)), c.inp(uni((B, H, W, 3), salt=2))
    pred, mask, ps, mean = c.out((B, H, W, 3)), c.out((B, H, W)), c.out((B,)), c.out((1,))
    sums = c.out((B, 2), torch.float64)
    ws, wb = _loss_ws(ctx, c)
    c.issue = lambda s: ctx.call("dvsg_loss_image_f32", U.data_ptr(), coord.data_ptr(), T.data_ptr(), gt.data_ptr(), B, H, W, 25,
                                 pred.data_ptr(), mask.data_ptr(), ps.data_ptr(), mean.data_ptr(), sums.data_ptr(), ws, wb, s)
    return c


@case("dvsg_loss_temporal_f32")
def _loss_temporal(ctx):
    torch = _torch()
    c = Case()
    B, H, W = LOSS
    pred, gt = c.inp(uni((B, H, W, 3), salt=1)), c.inp(uni((B, H, W, 3), salt=2))
    mp, mg = c.inp(uni((B, H, W), salt=3)), c.inp(uni((B, H, W), salt=4))
    flow = c.inp(uni((B, H, W, 2), -6.0, 6.0, 5))
    ps, mean, sums = c.out((B,)), c.out((1,)), c.out((B, 2), torch.float64)
    ws, wb = _loss_ws(ctx, c)
    c.issue = lambda s: ctx.call("dvsg_loss_temporal_f32", pred.data_ptr(), mp.data_ptr(), flow.data_ptr(), gt.data_ptr(),
                                 mg.data_ptr(), B, H, W, ps.data_ptr(), mean.data_ptr(), sums.data_ptr(), ws, wb, s)
    return c


@case("dvsg_loss_masked_mse_f32")
def _loss_mse(ctx):
    torch = _torch()
    c = Case()
    B, H, W = LOSS
    pred, gt = c.inp(uni((B, H, W, 3), salt=1)), c.inp(uni((B, H, W, 3), salt=2))
    m = c.inp(uni((B, H, W), salt=3))
    ps, mean, sums = c.out((B,)), c.out((1,)), c.out((B, 2), torch.float64)
    ws, wb = _loss_ws(ctx, c)
    c.issue = lambda s: ctx.call("dvsg_loss_masked_mse_f32", pred.data_ptr(), gt.data_ptr(), m.data_ptr(), B, H, W, 3, 1,
                                 ps.data_ptr(), mean.data_ptr(), sums.data_ptr(), ws, wb, s)
    return c


@case("dvsg_loss_grid_f32")
def _loss_grid(ctx):
    c, B = Case(), LOSS[0]
    V = c.inp(fixed(inputs.v_src(B)))
    F = c.inp(vectors(B, 7))
    ident, im, dist, dm = c.out((B,)), c.out((1,)), c.out((B,)), c.out((1,))
    c.issue = lambda s: ctx.call("dvsg_loss_grid_f32", V.data_ptr(), F.data_ptr(), B, 5, ident.data_ptr(), im.data_ptr(),
                                 dist.data_ptr(), dm.data_ptr(), s)
    return c


@case("dvsg_loss_surf_f32")
def _loss_surf(ctx):
    import test_gpu_losses as losses
    torch = _torch()
    c, N = Case(), 50
    B, H, W = LOSS
    coord, T = _coord_T(c, (H, W, H, W, B, 25))
    surf = c.inp(lambda seed: _t(losses.make_surf(31 + seed, B, N, H, W)))
    dims = c.inp(fixed(np.array([0.0, 14.0, 21.0], dtype=np.float32)))     # a zero divisor goes through div_no_nan
    coords, ps, mean, sums = c.out((B, N, 2)), c.out((B,)), c.out((1,)), c.out((B,), torch.float64)
    c.issue = lambda s: ctx.call("dvsg_loss_surf_f32", surf.data_ptr(), dims.data_ptr(), coord.data_ptr(), T.data_ptr(), B, N, H,
                                 W, 25, coords.data_ptr(), ps.data_ptr(), mean.data_ptr(), sums.data_ptr(), s)
    return c


# The only entries outside the contract: the header itself calls them synchronous.  The reason is the header's own phrase.
EXEMPT = {
    "dvsg_locnet_calibrate_f16": "Deterministic (fixed-order sums); synchronous; mutates the handle",
    "dvsg_debug_calibrate_f16_weights": "The A/B form of dvsg_locnet_calibrate_f16 (tools/f16_ef_sweep.py)",
}

ALL = [(name, i) for name in sorted(CASES) for i in range(len(CASES[name]))]
ALL_IDS = ["%s%s" % (name, "-" + CASES[name][i].label if CASES[name][i].label else "") for name, i in ALL]


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(synthetic_weights):
    import time
    t0 = time.time()
    c = Ctx(synthetic_weights)
    yield c
    c.close()
    print("\nSTREAMS module total: %.1f s" % (time.time() - t0))


class Delay(object):
    """The bounded delay: `count` matmuls of 4096 x 4096 float32, sized once by timing a chain with events so that one chain
    takes about 20 ms.  enqueue(stream, scale) queues scale chains and returns the event recorded right behind them."""

    TARGET_MS = 20.0

    def __init__(self):
        torch = _torch()
        self.a = torch.rand((4096, 4096), device="cuda")
        self.b = torch.rand((4096, 4096), device="cuda")
        self.c = torch.empty((4096, 4096), device="cuda")
        self.stream = torch.cuda.Stream()
        with torch.cuda.stream(self.stream):
            torch.matmul(self.a, self.b, out=self.c)            # the BLAS library's own first-call work
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(8):
                torch.matmul(self.a, self.b, out=self.c)
            e1.record()
        e1.synchronize()
        per = e0.elapsed_time(e1) / 8.0
        self.count = max(1, int(np.ceil(self.TARGET_MS / max(per, 1e-3))))
        print("\nSTREAMS delay: %.3f ms per matmul, %d per chain" % (per, self.count))

    def enqueue(self, stream, scale):
        torch = _torch()
        with torch.cuda.stream(stream):
            for _ in range(self.count * scale):
                torch.matmul(self.a, self.b, out=self.c)
            ev = torch.cuda.Event()
            ev.record()
        return ev


@pytest.fixture(scope="module")
def delay(ctx):
    return Delay()


def behind_delay(delay, run, what):
    """run(scale) queues the delay and the calls under test and returns the delay's event as queried when the host came back
    from issuing them, after synchronising.  Conclusive: that query was False.  Doubles the delay at most four times."""
    torch = _torch()
    scale = 1
    for _ in range(5):
        done_at_return = run(scale)
        torch.cuda.synchronize()
        if not done_at_return:
            print("STREAMS %s: conclusive behind %d chain(s) of %.0f ms" % (what, scale, delay.TARGET_MS))
            return scale
        scale *= 2
    raise AssertionError("%s: inconclusive: the delay had finished before the calls were issued, up to %d chains of %.0f ms"
                         % (what, scale // 2, delay.TARGET_MS))


# ---------------------------------------------------------------------------------------------------------------------
# 1. capture and replay
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,i", ALL, ids=ALL_IDS)
def test_replays_from_a_captured_graph(ctx, name, i):
    torch = _torch()
    c = CASES[name][i](ctx)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()          # torch's pool streams are non-blocking
    s = side.cuda_stream
    c.fill(0)
    c.restore()
    torch.cuda.synchronize()
    c.issue(s)                          # warm up
    side.synchronize()
    # the eager reference: the same call on the values of seeds 1..3
    want = []
    c.restore()
    for seed in (1, 2, 3):
        c.fill(seed)
        if not c.carry:
            c.restore()
        c.poison()
        torch.cuda.synchronize()
        c.issue(s)
        side.synchronize()
        want.append(c.snapshot())
    if c.carry:
        assert any(int(w[2][:3].sum()) > 0 for w in want), "the scene plan was meant to cut"
    if c.view is not None:
        c.view.check(c, want, s, side, ALL_IDS[ALL.index((name, i))])
    c.fill(0)
    c.restore()
    torch.cuda.synchronize()
    # a dead network held by a reference cycle frees device memory when the collector finds it (tests/test_gpu_cnn.py)
    gc.collect()
    gc.disable()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.issue(s)
    finally:
        gc.enable()
    torch.cuda.synchronize()
    c.restore()
    for k, seed in enumerate((1, 2, 3)):
        c.fill(seed)
        if not c.carry:
            c.restore()
        c.poison()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.same(want[k], "%s, replay %d" % (name, k + 1))


# ---------------------------------------------------------------------------------------------------------------------
# 2. re-entrancy at the ABI
# ---------------------------------------------------------------------------------------------------------------------
def _shared_F(n=3):
    return _t(inputs.control_vectors(55, n))


PAIRS = {
    "f32-f32": lambda: (net_case("forward", "f32", 2, 64, 96), net_case("forward", "f32", 2, 64, 96), (1, 2)),
    "f32-f16-ragged": lambda: (net_case("forward", "f32", 2, 64, 96), net_case("forward", "f16", 3, 33, 47), (1, 2)),
    "f32s-f32x3": lambda: (net_case("stabilize", "f32s", 2, 64, 96), net_case("stabilize", "f32x3", 2, 64, 96), (1, 2)),
    "ring_u8-masked": lambda: (net_case("ring_u8", "f32", 2, 64, 96), net_case("masked", "f32", 2, 64, 96), (1, 2)),
    "render_u8-render_nv12": lambda: (lambda F: (_render_u8_builder(False, F), _render_nv12_builder(False, F), (1, 2)))(_shared_F()),
    "stabilize-coverage_net": lambda: (net_case("stabilize", "f32", 2, 64, 96), _coverage_net, (1, 2)),
    # views of ONE parent: a shared F_t at two delivery sizes; two surface views; one view twice; and the plain handle beside
    # a scaled view on one source buffer, where the size each call writes comes from a table looked up by the handle's address
    "views-scaled_u8-scaled_nv12": lambda: (lambda F: (_render_u8_builder(False, F, "scaled-2x2"),
                                                       _render_nv12_builder(False, F, "scaled-3x3"), (1, 2)))(_shared_F()),
    "views-p010-nv16": lambda: (_render_nv12_builder(False, label="p010"), _render_nv12_builder(False, label="nv16"), (1, 2)),
    "views-one-view-twice": lambda: (_render_nv12_builder(False, label="p010-scaled-2x2-cubic-mirror"),
                                     _render_nv12_builder(False, label="p010-scaled-2x2-cubic-mirror"), (1, 2)),
    "views-plain-scaled-one-source": lambda: (lambda src: (_render_nv12_builder(False, src=src),
                                                           _render_nv12_builder(False, label="scaled-3x3", src=src),
                                                           (1, 2)))(_shared_surface()),
}


def _alone(c, seed, s, stream):
    torch = _torch()
    c.fill(seed)
    c.restore()
    c.poison()
    torch.cuda.synchronize()
    c.issue(s)
    stream.synchronize()
    return c.snapshot()


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_two_streams_of_one_handle(ctx, delay, pair):
    torch = _torch()
    ba, bb, (seed_a, seed_b) = PAIRS[pair]()
    a, b = ba(ctx), bb(ctx)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    want_a, want_b = _alone(a, seed_a, s1.cuda_stream, s1), _alone(b, seed_b, s2.cuda_stream, s2)

    def run(scale):
        for c in (a, b):
            c.restore()
            c.poison()
        torch.cuda.synchronize()
        ev = delay.enqueue(delay.stream, scale)
        s1.wait_event(ev)
        s2.wait_event(ev)
        a.issue(s1.cuda_stream)
        b.issue(s2.cuda_stream)
        return ev.query()
    behind_delay(delay, run, pair)
    a.same(want_a, pair + ": first call")
    b.same(want_b, pair + ": second call")


def test_two_threads_of_one_handle(ctx, delay):
    """The first pair again, the two calls issued from two Python threads (ctypes releases the GIL: the host side of the
    library runs concurrently), each followed by an invalid call of its own -- they return before any launch -- whose
    message only that thread may see."""
    torch = _torch()
    a, b = net_case("forward", "f32", 2, 64, 96)(ctx), net_case("forward", "f32", 2, 64, 96)(ctx)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    want_a, want_b = _alone(a, 1, s1.cuda_stream, s1), _alone(b, 2, s2.cuda_stream, s2)
    lib = ctx.lib.load()
    x, F = a.inputs[0][0], a.outputs[0]
    ws = a.guards[0]
    bad = {"A": lambda: lib.dvsg_locnet_forward_f32(ctx.h, x.data_ptr(), 0, 64, 96, F.data_ptr(), ws.ptr(), ws.nbytes, 0),
           "B": lambda: lib.dvsg_locnet_forward_f32(ctx.h, x.data_ptr(), 2, 64, 96, F.data_ptr(), ws.ptr(), 1024, 0)}
    seen = {}

    def run(scale):
        for c in (a, b):
            c.poison()
        torch.cuda.synchronize()
        ev = delay.enqueue(delay.stream, scale)
        s1.wait_event(ev)
        s2.wait_event(ev)
        gate = threading.Barrier(2)
        errors = []

        def worker(tag, c, s):
            try:
                gate.wait(timeout=60)
                c.issue(s)
                done = ev.query()
                rc = bad[tag]()
                gate.wait(timeout=60)               # both failures are made before either message is read
                seen[tag] = (rc, lib.dvsg_last_error_string().decode(), done)
            except Exception as e:                  # noqa: a worker's failure is the test's
                errors.append(e)
                gate.abort()
        ts = [threading.Thread(target=worker, args=("A", a, s1.cuda_stream)),
              threading.Thread(target=worker, args=("B", b, s2.cuda_stream))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        return seen["A"][2] or seen["B"][2]
    behind_delay(delay, run, "two threads")
    a.same(want_a, "thread A")
    b.same(want_b, "thread B")
    assert seen["A"][0] == -1 and "bad shape" in seen["A"][1] and "B=0" in seen["A"][1], seen["A"]
    assert seen["B"][0] < 0 and "workspace" in seen["B"][1] and "bad shape" not in seen["B"][1], seen["B"]


def test_two_threads_of_views(ctx, delay):
    """Two renders through scaled views from two Python threads while a third makes and destroys 64 scaled views of the same
    parent: the NV12 renders look the size of their handle up, by its address, in a process-global table that the view
    constructors and dvsg_locnet_destroy write (the invariant above g_scaled_mutex, views.cpp).  A bounded loop of valid
    calls.  Each worker then makes a call that is refused before any launch and reads its own message: the output pitch is
    too short for the VIEW's row -- 34 bytes for the 36 of the byte view, the 102 bytes of a source row of bytes for the
    2 x 52 of the word view -- so the message also shows that the size came from the right table entry."""
    torch = _torch()
    labels = {"A": "scaled-3x3", "B": "p210-scaled-2x2"}
    a, b = (_render_nv12_builder(False, label=labels[t])(ctx) for t in "AB")
    plain = _render_nv12_builder(False)(ctx)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    want_a, want_b = _alone(a, 1, s1.cuda_stream, s1), _alone(b, 2, s2.cuda_stream, s2)
    want_plain = _alone(plain, 3, s1.cuda_stream, s1)
    views = {t: ctx.view(labels[t]) for t in "AB"}
    sizes = {t: ctx.render_size(views[t]) for t in "AB"}
    assert sizes == {t: VIEWS[labels[t]]["out_size"] for t in "AB"} and ctx.render_size(ctx.h) == (0, 0)
    n_views = ctx.n_views()
    lib = ctx.lib.load()
    H, W = SURF

    def refused(c, tag, pitch):
        (buf, _), (F, _), T, out = c.inputs[0], c.inputs[1], c.outputs[0], c.outputs[1]
        src = _surface_source(labels[tag], 0)
        return lambda: lib.dvsg_tps_render_nv12(views[tag], F.data_ptr(), buf.data_ptr(), buf.data_ptr() + src.uv_offset,
                                                src.pitch, src.frame_stride, 3, H, W, T.data_ptr(), out.data_ptr(),
                                                out.data_ptr() + 64, pitch, 1 << 20, 0)
    bad = {"A": refused(a, "A", 34), "B": refused(b, "B", W)}
    seen, churn = {}, []

    def run(scale):
        for c in (a, b):
            c.poison()
        del churn[:]
        torch.cuda.synchronize()
        ev = delay.enqueue(delay.stream, scale)
        s1.wait_event(ev)
        s2.wait_event(ev)
        start, both = threading.Barrier(3), threading.Barrier(2)
        errors = []

        def worker(tag, c, s):
            try:
                start.wait(timeout=60)
                c.issue(s)
                done = ev.query()
                rc = bad[tag]()
                both.wait(timeout=60)               # both failures are made before either message is read
                seen[tag] = (rc, lib.dvsg_last_error_string().decode(), done)
            except Exception as e:                  # noqa: a worker's failure is the test's
                errors.append(e)
                start.abort()
                both.abort()

        def churner():
            try:
                start.wait(timeout=60)
                for k in range(64):
                    v = ctypes.c_void_p()
                    rc = lib.dvsg_locnet_view_create_scaled(ctx.h, 8 + k, 12 + k, ctypes.byref(v))
                    churn.append((rc, lib.dvsg_locnet_destroy(v) if rc == 0 else None))
            except Exception as e:                  # noqa
                errors.append(e)
                start.abort()
        ts = [threading.Thread(target=worker, args=("A", a, s1.cuda_stream)),
              threading.Thread(target=worker, args=("B", b, s2.cuda_stream)), threading.Thread(target=churner)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        return seen["A"][2] or seen["B"][2]
    behind_delay(delay, run, "two threads of views")
    assert churn == [(0, 0)] * 64, churn
    a.same(want_a, "thread A")
    b.same(want_b, "thread B")
    assert {t: ctx.render_size(views[t]) for t in "AB"} == sizes and ctx.render_size(ctx.h) == (0, 0)
    assert ctx.n_views() == n_views, "the parent's views are not those from before the test"
    _alone(plain, 3, s1.cuda_stream, s1)            # a source-size frame into an output of exactly that size, as before
    plain.same(want_plain, "the plain handle after the views came and went")
    assert seen["A"][0] == -1 and "output pitch=34 < W=36" in seen["A"][1], seen["A"]
    assert seen["B"][0] == -1 and "output pitch=102 < 2 W = 104" in seen["B"][1], seen["B"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python facade
# ---------------------------------------------------------------------------------------------------------------------
def test_facade_workspace_is_per_stream(ctx):
    torch = _torch()
    net = ctx.net
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        w1, n1 = net.workspace(2, 64, 96)
    with torch.cuda.stream(s2):
        w2, n2 = net.workspace(2, 64, 96)
    with torch.cuda.stream(s1):
        w1b, n1b = net.workspace(2, 64, 96)
    assert n1 == n2 == n1b == ctx.ws_bytes(2, 64, 96) and w1.numel() >= n1 and w2.numel() >= n2
    a0, a1, b0, b1 = w1.data_ptr(), w1.data_ptr() + w1.numel(), w2.data_ptr(), w2.data_ptr() + w2.numel()
    assert a1 <= b0 or b1 <= a0, "two streams share workspace bytes"
    assert w1b.data_ptr() == w1.data_ptr() and w1b.numel() == w1.numel(), "the same stream must get the same buffer back"


def _facade_calls():
    def forward(net, x, u):
        return [net.forward(x)]

    def stabilize(net, x, u):
        torch = _torch()
        out, F = torch.empty_like(u), torch.empty((x.shape[0], 25, 2), device="cuda")
        net.stabilize(x, u, out, F)
        return [out, F]

    def tap(net, x, u):
        return [net.tap(x, 9)]
    return {"forward": forward, "stabilize": stabilize, "tap": tap}


@pytest.mark.parametrize("what", ["forward", "stabilize", "tap"])
def test_facade_two_streams_one_locnet(ctx, delay, what):
    """8 x 64 x 96 on one stream and 2 x 64 x 96 on another, released together: the serial results, bit for bit."""
    torch = _torch()
    fn = _facade_calls()[what]
    net = ctx.net
    xs = [uni((B, 64, 96, 21), salt=40 + B)(1) for B in (8, 2)]
    us = [x[..., 18:].contiguous() for x in xs]
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    want = []
    for x, u, s in zip(xs, us, ss):
        with torch.cuda.stream(s):
            want.append([t.clone() for t in fn(net, x, u)])
        s.synchronize()
    got = []

    def run(scale):
        del got[:]
        ev = delay.enqueue(delay.stream, scale)
        for x, u, s in zip(xs, us, ss):
            s.wait_event(ev)
            with torch.cuda.stream(s):
                got.append(fn(net, x, u))
        return ev.query()
    behind_delay(delay, run, what)
    for k in (0, 1):
        for g, w in zip(got[k], want[k]):
            assert torch.equal(_bits(g), _bits(w)), "%s on stream %d differs from its serial run" % (what, k)


def _online_pair(which, H, W):
    """(options of the two stabilisers, their frames [2][steps]).  "defaults": float frames at the model's size, three steps.
    "views": four steps through the newer stream formats -- an NV12 stream (tests/test_gpu_scene.py's clips: two frames of
    scene A, then two of scene B) rendered bicubic with a mirrored border, cropped and cut on the device, beside a P210
    stream of SURF frames rendered at half strength and at half size."""
    if which == "defaults":
        return [dict(max_streams=1)] * 2, \
            [[_t(inputs.smooth_frames(60 + 10 * k + j, 1, H, W)[0]) for j in range(3)] for k in (0, 1)]
    import test_gpu_scene as scene
    import yuv422_ref
    A, B, kw = scene._clips("nv12", 2)
    assert kw == dict(frame_format="nv12")
    p210 = yuv422_ref.Batch422(91, 4, SURF[0], SURF[1], words=True).buf        # packed: [4, 2 H, 2 W] bytes
    return [dict(frame_format="nv12", crop="auto", scene_cut=scene.THR, render_filter="bicubic", border="mirror"),
            dict(frame_format="p210", out_size=(34, 52), strength=0.5)], \
        [[_t(f) for f in np.concatenate([A, B])], [_t(f) for f in p210]]


@pytest.mark.parametrize("which", ["defaults", "views"])
def test_facade_two_online_stabilizers_share_a_model(ctx, delay, synthetic_weights, which):
    """Two OnlineStabilizers on one model, three or four steps each under its own stream, against the same streams stepped
    one after the other."""
    import test_gpu_scene as scene
    from coupe.dvsg_amd.online import OnlineStabilizer
    torch = _torch()
    H, W = 64, 96
    model = scene._model(synthetic_weights, H, W)
    options, frames = _online_pair(which, H, W)
    steps = len(frames[0])
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()

    def opened():
        ons = [OnlineStabilizer(model, **kw) for kw in options]
        return ons, [on.open() for on in ons]
    ons, sids = opened()
    torch.cuda.synchronize()
    want = [[], []]
    for j in range(steps):
        for k in (0, 1):
            with torch.cuda.stream(ss[k]):
                want[k].append(ons[k].push(sids[k], frames[k][j]).clone())
            ss[k].synchronize()
    torch.cuda.synchronize()
    if which == "views":
        st = ons[0].scene_state(sids[0])
        assert st["cuts"] == 1 and st["frames_since_cut"] == 2, "scene B was meant to cut at the third step: %s" % (st,)
        assert tuple(want[1][0].shape) == (2 * 34, 2 * 52) and tuple(want[0][0].shape) == tuple(frames[0][0].shape)
    got = [[], []]
    state = {}

    def fresh():
        state["ons"], state["sids"] = opened()
        for k in (0, 1):
            del got[k][:]
        torch.cuda.synchronize()

    def run(scale):
        fresh()
        late = False
        for j in range(steps):
            ev = delay.enqueue(delay.stream, scale)
            for k in (0, 1):
                ss[k].wait_event(ev)
                with torch.cuda.stream(ss[k]):
                    got[k].append(state["ons"][k].push(state["sids"][k], frames[k][j]).clone())
            late = late or ev.query()
            torch.cuda.synchronize()
        return late
    behind_delay(delay, run, "online " + which)
    for k in (0, 1):
        for j in range(steps):
            assert got[k][j].cpu().numpy().tobytes() == want[k][j].cpu().numpy().tobytes(), \
                "stabilizer %d, step %d differs from its serial run" % (k, j)


# ---------------------------------------------------------------------------------------------------------------------
# 4. calibration keeps its word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["undo", "debug-mode0", "debug-mode1"])
def test_calibration_waits_for_the_stream(ctx, delay, synthetic_weights, how):
    """On a non-blocking stream: delay, float16 forward -> F_a, the recalibration, float16 forward -> F_b.  F_a is the forward
    on the weights it was issued against, F_b the one on the new weights; the two differ."""
    from coupe.dvsg_amd.networks import LocNet
    torch = _torch()
    lib = ctx.lib
    net = LocNet(synthetic_weights)      # a handle of its own: calibration mutates it
    B, H, W = 2, 64, 96
    x = _t(inputs.window_frames(71, B, H, W))
    F = [torch.empty((B, 25, 2), device="cuda") for _ in range(2)]
    ws = _guarded(ctx.ws_bytes(B, H, W))
    side = torch.cuda.Stream()
    s = side.cuda_stream
    torch.cuda.synchronize()

    def forward(out):
        lib.call("dvsg_locnet_forward_f16", net.handle, x.data_ptr(), B, H, W, out.data_ptr(), ws.ptr(), ws.nbytes, s)

    def calibrate():
        lib.call("dvsg_locnet_calibrate_f16", net.handle, x.data_ptr(), B, H, W, ws.ptr(), ws.nbytes, s)

    def change():
        if how == "undo":
            lib.call("dvsg_locnet_calibrate_f16", net.handle, None, 0, 0, 0, ws.ptr(), ws.nbytes, s)
        else:
            lib.call("dvsg_debug_calibrate_f16_weights", net.handle, x.data_ptr(), B, H, W, int(how[-1]), ws.ptr(), ws.nbytes, s)
    # the two references, each forward run alone
    calibrate()
    forward(F[0])
    side.synchronize()
    want_a = F[0].clone()
    change()
    side.synchronize()
    forward(F[0])
    side.synchronize()
    want_b = F[0].clone()
    assert not torch.equal(_bits(want_a), _bits(want_b)), "the two states give one F_t: the test would pass vacuously"

    def run(scale):
        calibrate()
        torch.cuda.synchronize()
        for t in F:
            _poison(t)
        torch.cuda.synchronize()
        ev = delay.enqueue(side, scale)
        forward(F[0])
        done = ev.query()
        change()
        forward(F[1])
        return done
    behind_delay(delay, run, how)
    assert ws.intact()
    assert torch.equal(_bits(F[0]), _bits(want_a)), "the forward queued before the recalibration ran on rewritten weights"
    assert torch.equal(_bits(F[1]), _bits(want_b)), "the forward after the recalibration is not the recalibrated one"
