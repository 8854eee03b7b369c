"""GPU: the crop to the valid region -- dvsg_tps_coverage_f32 (crop_scan_kernel), the zoomed warps
(tps_warp_zoom_kernel through dvsg_tps_warp_zoom_f32 / dvsg_tps_render_zoom_u8), the two entries on a network handle, and
stabilize_clip(crop=...).

What is exact is asserted exactly: the scan's integers against tests/crop_ref.py on the x_s, y_s that the zoomed warp itself
wrote for the same coord, T and zoom; zoom == 1 against the plain entry points, bit for bit; the zoomed warp's pixels against
the float32 oracle's sampler A at the GPU's own coordinates, bit for bit.

The zoomed GRID is held to a float64 evaluation at float64(float32(z)) x_t, float64(float32(z)) y_t (the products exact in
float64) with the grid bound of tests/test_tps_f64.py (link 2) extended by the one rounding the kernel adds to each
coordinate.  Derivation (u = 2^-24): the kernel forms x' = fl(z x_t) = X (1 + d), |d| <= u, X = z x_t, and likewise y'; from
there on it is tps_warp_kernel on (x', y'), so it is within E(x', y') -- link 2's bound, whose terms are evaluated at X, Y
here; the difference is second order and inside that bound's factor 1.01 -- of the exact map AT (x', y').  The exact map
moves between (X, Y) and (x', y') by at most
    |T_1| u |X| + |T_2| u |Y| + sum_k |T_k| |r_k(x', y') - r_k(X, Y)|,
and r = d2 ln(d2 + eps) has dr/dx = 2 dx (ln(d2 + eps) + d2 / (d2 + eps)), |dr/dx| <= 2 |dx| (|L| + 1), L = ln(d2 + eps), so
    |r_k(x', y') - r_k(X, Y)| <= 1.01 x 2 u (|dx_k| |X| + |dy_k| |Y|) (|L_k| + 1)
(mean value theorem; the derivative changes by a relative ~u |X| / |dx| over the step except within u |X| of a control point,
where |dx| (|L| + 1) <= 15 |dx| is below 1e-6 and the term is negligible against the (P + 4) u S of link 2; 1.01 covers it).
    E_zoom = E_link2(X, Y) + 1.01 u (|T_1 X| + |T_2 Y| + 2 sum_k |T_k| (|dx_k| |X| + |dy_k| |Y|) (|L_k| + 1)).
Nothing in it was fitted to a GPU result; every case prints its worst ratio to the bound (`CROP zoomed grid ...`)."""
import ctypes

import numpy as np
import pytest

import crop_ref
import inputs as tin
import test_tps_f64 as tps

pytestmark = pytest.mark.gpu

F32 = np.float32
KT = 256                                                     # kThreads of warp_device.h: columns per workgroup
# (out_h, out_w, src_H, src_W, B, P): out_h 2 / 5 / 8 / 37 = no, partial, whole, several 4-row groups; out_w 2 / 64 / KT + 3 /
# 2 KT + 1 = one, partial, several column workgroups; sources equal to and different from the output; B 1 / 3; P 3 / 25 / 61
CASES = [(2, 2, 5, 7, 1, 3), (5, 64, 5, 64, 3, 25), (8, KT + 3, 9, 300, 3, 61), (37, 2 * KT + 1, 37, 2 * KT + 1, 1, 25),
         (37, 64, 20, 31, 3, 3), (5, 2 * KT + 1, 12, 17, 1, 61), (8, 2, 8, 2, 3, 25), (2, KT + 3, 6, 9, 3, 25)]
IDS = ["%dx%d-src%dx%d-B%d-P%d" % c for c in CASES]
ZOOMS = np.array([0.8125, 0.93, 0.5], dtype=F32)             # a different z per sample; 0.93 is not a short binary fraction


def test_cases_cover_the_shapes_the_kernel_branches_on():
    assert {c[0] for c in CASES} == {2, 5, 8, 37} and {c[1] for c in CASES} == {2, 64, KT + 3, 2 * KT + 1}
    assert {c[4] for c in CASES} == {1, 3} and {c[5] for c in CASES} == {3, 25, 61}
    assert any(c[:2] == c[2:4] for c in CASES) and any(c[:2] != c[2:4] for c in CASES)


def _sync():
    import torch
    torch.cuda.synchronize()


def case_T(kind, case, seed=0):
    """(coord [B,P,2], T [B,2,P+3]) float32: `near` the identity (a solved T of small vectors), `out` (zoomed out and
    shifted: most of the frame leaves the source), `nan` (the near T with sample 0's affine x row NaN)"""
    oh, ow, sh, sw, B, P = case
    coord = tps.control_points(P, B, True, seed=oh + ow + P)
    T = tps.grid_T(coord, 0.03, 0.0, seed=seed + oh * 31 + ow)
    if kind == "out":
        T = T.copy()
        T[:, 0, :3] = (0.9, 2.2, 0.1)
        T[:, 1, :3] = (-0.4, -0.1, 1.9)
    elif kind == "nan":
        T = T.copy()
        T[0, 0, 1] = np.nan
    return coord, np.ascontiguousarray(T, dtype=F32)


def gpu_warp_zoom(U, coord, T, z, oh, ow, want_xy=True):
    """dvsg_tps_warp_zoom_f32 (z = None: zoom NULL) with every output between sentinels -> (out or None, x_s, y_s [B,oh*ow])"""
    import torch
    from coupe.dvsg_amd import _lib
    B, P = T.shape[0], T.shape[2] - 3
    c, t = tps._dev(coord), tps._dev(T)
    zd = tps._dev(np.asarray(z, dtype=F32)) if z is not None else None
    H, W, C = (U.shape[1:] if U is not None else (1, 1, 1))
    u = tps._dev(U) if U is not None else None
    n = B * oh * ow
    out = tps.Guarded(n * C * 4, c.device) if U is not None else None
    gx = tps.Guarded(n * 4, c.device) if want_xy else None
    gy = tps.Guarded(n * 4, c.device) if want_xy else None
    _lib.call("dvsg_tps_warp_zoom_f32", u.data_ptr() if u is not None else None, c.data_ptr(), t.data_ptr(),
              zd.data_ptr() if zd is not None else None, B, H, W, C, P, oh, ow, out.ptr() if out else None,
              gx.ptr() if gx else None, gy.ptr() if gy else None, tps._stream())
    _sync()
    for g in (out, gx, gy):
        assert g is None or g.intact(), "wrote past an output"
    f = torch.float32
    return (out.view(f, (B, oh, ow, C)).cpu().numpy() if out else None,
            gx.view(f, (B, oh * ow)).cpu().numpy() if gx else None, gy.view(f, (B, oh * ow)).cpu().numpy() if gy else None)


def cover_bytes(B, oh, ow):
    from coupe.dvsg_amd import _lib
    need = ctypes.c_size_t()
    _lib.call("dvsg_tps_coverage_workspace_bytes", B, oh, ow, ctypes.byref(need))
    return need.value


def gpu_cover(coord, T, z, sh, sw, oh, ow, fill=0x5A, short=0, net=None, F=None):
    """dvsg_tps_coverage_f32 (or, with net and F, dvsg_tps_coverage_net_f32) with outputs and workspace pre-filled with
    `fill` bytes and guarded -> (n_border, key_min int32 [B], T written by the net form or None)"""
    import torch
    from coupe.dvsg_amd import _lib
    B = T.shape[0] if F is None else F.shape[0]
    dev = torch.device("cuda:0")
    need = cover_bytes(B, oh, ow)
    ws = tps.Guarded(need, dev)
    gn, gk = tps.Guarded(B * 4, dev), tps.Guarded(B * 4, dev)
    for g in (ws, gn, gk):
        g.body.fill_(fill)
    zd = tps._dev(np.asarray(z, dtype=F32)) if z is not None else None
    zp = zd.data_ptr() if zd is not None else None
    Tout = None
    if F is None:
        c, t = tps._dev(coord), tps._dev(T)
        _lib.call("dvsg_tps_coverage_f32", c.data_ptr(), t.data_ptr(), zp, B, T.shape[2] - 3, sh, sw, oh, ow, gn.ptr(), gk.ptr(),
                  ws.ptr(), need - short, tps._stream())
    else:
        Fd = tps._dev(F)
        Tout = tps.Guarded(B * 56 * 4, dev)
        _lib.call("dvsg_tps_coverage_net_f32", net.handle, Fd.data_ptr(), zp, B, sh, sw, oh, ow, Tout.ptr(), gn.ptr(), gk.ptr(),
                  ws.ptr(), need - short, tps._stream())
    _sync()
    for g in (ws, gn, gk, Tout):
        assert g is None or g.intact(), "wrote past a buffer"
    i32 = torch.int32
    return (gn.view(i32, (B,)).cpu().numpy(), gk.view(i32, (B,)).cpu().numpy(),
            Tout.view(torch.float32, (B, 2, 28)).cpu().numpy() if Tout else None)


# ---------------------------------------------------------------------------------------------------------------------
# the scan is the warp's map

@pytest.mark.parametrize("kind", ["near", "out", "nan"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scan_counts_what_the_zoomed_warp_maps(case, kind):
    oh, ow, sh, sw, B, P = case
    coord, T = case_T(kind, case)
    for z in (None, ZOOMS[:B]):
        _, xs, ys = gpu_warp_zoom(None, coord, T, z, oh, ow)
        want_n, want_k = crop_ref.scan(xs, ys, sh, sw, oh, ow)
        n, k, _ = gpu_cover(coord, T, z, sh, sw, oh, ow)
        assert n.tolist() == want_n.tolist() and k.tolist() == want_k.tolist(), (kind, z, n, want_n, k, want_k)
        if kind == "nan":
            assert n[0] == oh * ow and k[0] == min(crop_ref.keys(oh, ow).min(), crop_ref.INT32_MAX)
        if kind == "near" and min(sh, sw) > 2 and min(oh, ow) > 2 and z is not None:
            assert (n < oh * ow).all(), "a zoomed near-identity map must keep pixels"
    if kind == "out":
        assert (want_n > 0).all()


def test_scan_is_deterministic_needs_no_zeroing_and_checks_its_workspace():
    from coupe.dvsg_amd._lib import DvsgError
    case = CASES[2]
    oh, ow, sh, sw, B, P = case
    coord, T = case_T("out", case)
    a = gpu_cover(coord, T, ZOOMS[:B], sh, sw, oh, ow, fill=0x5A)
    b = gpu_cover(coord, T, ZOOMS[:B], sh, sw, oh, ow, fill=0x5A)
    c = gpu_cover(coord, T, ZOOMS[:B], sh, sw, oh, ow, fill=0xFF)
    assert a[0].tolist() == b[0].tolist() == c[0].tolist() and a[1].tolist() == b[1].tolist() == c[1].tolist()
    with pytest.raises(DvsgError, match="workspace"):
        gpu_cover(coord, T, ZOOMS[:B], sh, sw, oh, ow, short=1)
    assert cover_bytes(B, oh, ow) == B * 2 * 2 * 8           # one (count, key) pair per workgroup: 2 column x 2 row groups


def test_short_workspace_launches_nothing(synthetic_weights):
    """the outputs keep their garbage: an error return, not a launch -- for the plain and the net entry"""
    import torch
    from coupe.dvsg_amd import _lib
    net = tps._net(synthetic_weights)
    oh, ow, B = 8, KT + 3, 2
    coord, T = tps._dev(tin.v_src(B)), torch.zeros((B, 2, 28), device="cuda")
    F = torch.zeros((B, 25, 2), device="cuda")
    need = cover_bytes(B, oh, ow)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.full((2, B), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    s = tps._stream()
    Tn = torch.full((B, 2, 28), 7.0, device="cuda")
    rc = lib.dvsg_tps_coverage_net_f32(net.handle, F.data_ptr(), None, B, oh, ow, oh, ow, Tn.data_ptr(), out[0].data_ptr(),
                                       out[1].data_ptr(), ws.data_ptr(), need - 1, s)
    _sync()
    assert rc != 0 and (out == 0x5A5A5A5A).all() and (Tn == 7.0).all()
    assert lib.dvsg_tps_coverage_f32(coord.data_ptr(), T.data_ptr(), None, B, 25, oh, ow, oh, ow, out[0].data_ptr(),
                                     out[1].data_ptr(), ws.data_ptr(), need - 1, s) != 0
    _sync()
    assert (out == 0x5A5A5A5A).all()


# ---------------------------------------------------------------------------------------------------------------------
# zoom == 1 changes nothing

@pytest.mark.parametrize("C", [3, 1, 2])
def test_zoom_one_is_the_plain_warp_bit_for_bit(C):
    H, W, oh, ow, B, P = 20, 31, 37, KT + 3, 3, 25
    coord, T = case_T("near", (oh, ow, H, W, B, P))
    U = tps.make_frames("noise", B, H, W, C, seed=C)
    want = tps.gpu_warp(U, coord, T, oh, ow)
    for z in (np.ones(B, dtype=F32), None):
        got = gpu_warp_zoom(U, coord, T, z, oh, ow)
        for g, w, name in zip(got, want, ("out", "x_s", "y_s")):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), name


def gpu_render_zoom(net, F, src, flip, z, u8_W, u8_x0):
    import torch
    from coupe.dvsg_amd import _lib
    n, H, W = src.shape[:3]
    Fd, s = tps._dev(F), tps._dev(src)
    zd = tps._dev(np.asarray(z, dtype=F32)) if z is not None else None
    T = tps.Guarded(n * 56 * 4, s.device)
    o32 = tps.Guarded(n * H * W * 12, s.device)
    o8 = tps.Guarded(n * H * u8_W * 3, s.device)
    o8.body.fill_(0x5A)
    _lib.call("dvsg_tps_render_zoom_u8", net.handle, Fd.data_ptr(), s.data_ptr(), n, H, W, int(flip),
              zd.data_ptr() if zd is not None else None, T.ptr(), o32.ptr(), o8.ptr(), u8_W, u8_x0, tps._stream())
    _sync()
    for g in (T, o32, o8):
        assert g.intact(), "wrote past an output"
    return (T.view(torch.float32, (n, 2, 28)).cpu().numpy(), o32.view(torch.float32, (n, H, W, 3)).cpu().numpy(),
            o8.view(torch.uint8, (n, H, u8_W, 3)).cpu().numpy())


def _render_inputs(H, W, B=3):
    rng = np.random.default_rng(H + W)
    src = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return src, tps.vectors(B, 25, 0.05, 0.0, seed=W)


@pytest.mark.parametrize("flip", [0, 1])
def test_render_zoom_one_is_the_plain_render_bit_for_bit(synthetic_weights, flip):
    net = tps._net(synthetic_weights)
    H, W = 37, KT + 3
    src, F = _render_inputs(H, W)
    want = tps.gpu_render(net, F, src, flip, True, W + 9, 5)
    for z in (None, np.ones(3, dtype=F32)):
        got = gpu_render_zoom(net, F, src, flip, z, W + 9, 5)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "T"
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "float32 output"
        assert np.array_equal(got[2], want[2]), "uint8 output"


# ---------------------------------------------------------------------------------------------------------------------
# zoom != 1

def zoom_grid_reference(T, coord, oh, ow, z):
    """(ref, E) [B,2,oh,ow] float64: the map at float64(float32(z_b)) x the float32 grid and E_zoom of this file's docstring"""
    T = np.asarray(T, dtype=np.float64)
    c = np.asarray(coord, dtype=F32).astype(np.float64)
    B, P = T.shape[0], T.shape[2] - 3
    ref = np.empty((B, 2, oh, ow))
    E = np.empty_like(ref)
    for b in range(B):
        X, Y = crop_ref.zoomed_axes(oh, ow, z[b])
        X, Y = X[None, :], Y[:, None]
        cb = c[b % c.shape[0]]
        acc = [T[b, k, 0] + T[b, k, 1] * X + T[b, k, 2] * Y for k in range(2)]
        S = [np.abs(T[b, k, 0]) + np.abs(T[b, k, 1] * X) + np.abs(T[b, k, 2] * Y) for k in range(2)]
        Z = [np.abs(T[b, k, 1] * X) + np.abs(T[b, k, 2] * Y) for k in range(2)]
        D = [0.0, 0.0]
        for q in range(P):
            dx, dy = X - cb[q, 0], Y - cb[q, 1]
            d2 = np.square(dx) + np.square(dy)
            L = np.log(d2 + tps.EPS32)
            r = d2 * L
            dr = tps.U24 * (tps.GRID_A * d2 * (np.abs(L) + 1.0) + tps.GRID_B * d2 + tps.GRID_C * np.abs(r))
            dz = 2.0 * (np.abs(dx) * np.abs(X) + np.abs(dy) * np.abs(Y)) * (np.abs(L) + 1.0)
            for k in range(2):
                t = T[b, k, 3 + q]
                acc[k] = acc[k] + t * r
                S[k] = S[k] + np.abs(t * r)
                D[k] = D[k] + abs(t) * dr
                Z[k] = Z[k] + abs(t) * dz
        for k in range(2):
            ref[b, k] = acc[k]
            E[b, k] = tps.SECOND * (D[k] + (P + 4) * tps.U24 * S[k]) + tps.SECOND * tps.U24 * Z[k]
    return ref, E


def test_zoom_reference_at_one_is_the_grid_reference_of_the_tps_file():
    case = CASES[1]
    coord, T = case_T("near", case)
    ref, E = zoom_grid_reference(T, coord, case[0], case[1], np.ones(3, dtype=F32))
    r0, E0 = tps.grid_reference(T, coord, case[0], case[1])
    assert np.array_equal(ref, r0) and (E >= E0).all()


@pytest.mark.parametrize("kind", ["near", "out"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zoomed_grid_against_float64(case, kind):
    oh, ow, sh, sw, B, P = case
    coord, T = case_T(kind, case)
    z = ZOOMS[:B]
    _, xs, ys = gpu_warp_zoom(None, coord, T, z, oh, ow)
    ref, E = zoom_grid_reference(T, coord, oh, ow, z)
    nbad, worst, at = tps.check_grid(xs, ys, ref, E)
    print("CROP zoomed grid %s %s: worst / bound %.3f at (b, k, row, column) %s" % (IDS[CASES.index(case)], kind, worst, at))
    assert nbad == 0, (nbad, worst, at)


@pytest.mark.parametrize("H,W,oh,ow,C,P", [(20, 31, 37, KT + 3, 3, 25), (9, 300, 8, 2 * KT + 1, 1, 61), (5, 7, 5, 64, 2, 3)])
def test_zoomed_pixels_are_sampler_a_at_the_gpu_s_own_coordinates(H, W, oh, ow, C, P):
    B = 3
    coord = tps.control_points(P, B, True, seed=H * W + C)
    T = tps.sampler_T(B, P, H, W, seed=oh * ow + P)
    T[1] = case_T("near", (oh, ow, H, W, B, P))[1][1]
    U = tps.make_frames("noise", B, H, W, C, seed=C * 100 + H)
    out, xs, ys = gpu_warp_zoom(U, coord, T, ZOOMS, oh, ow)
    out2, _, _ = gpu_warp_zoom(U, coord, T, ZOOMS, oh, ow, want_xy=False)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    nbad, worst, neq, where = tps.check_sampler(out, U, xs, ys)
    assert nbad == 0 and neq == 0, (nbad, worst, neq, where[:4].tolist())
    n, k, _ = gpu_cover(coord, T, ZOOMS, H, W, oh, ow)
    want = crop_ref.scan(xs, ys, H, W, oh, ow)
    assert n.tolist() == want[0].tolist() and k.tolist() == want[1].tolist()


def test_zoomed_render_is_the_zoomed_warp_of_the_converted_frames(synthetic_weights):
    from oracle import frames as ofr
    net = tps._net(synthetic_weights)
    H, W = 37, KT + 3
    src, F = _render_inputs(H, W)
    for flip in (0, 1):
        T, o32, o8 = gpu_render_zoom(net, F, src, flip, ZOOMS, W + 9, 5)
        rgb = src[..., ::-1] if flip else src
        U = (rgb.astype(np.float64) / 255.0).astype(F32)
        want, _, _ = gpu_warp_zoom(U, tin.v_src(3), T, ZOOMS, H, W)
        assert np.array_equal(o32.view(np.uint32), want.view(np.uint32))
        want8 = ofr.to_uint8(np.clip((o32[..., ::-1] if flip else o32).astype(np.float64), 0.0, None))
        assert np.array_equal(o8[:, :, 5:5 + W], want8)
        assert (o8[:, :, :5] == 0x5A).all() and (o8[:, :, 5 + W:] == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------------------
# the entries on a network handle

@pytest.mark.parametrize("oh,ow,sh,sw", [(37, KT + 3, 37, KT + 3), (5, 64, 48, 80)])
def test_net_scan_uses_the_render_s_T_and_counts_like_the_plain_scan(synthetic_weights, oh, ow, sh, sw):
    net = tps._net(synthetic_weights)
    B = 3
    F = tps.vectors(B, 25, 0.05, 0.0, seed=oh)
    F[1] = tps.vectors(1, 25, 0.5, 0.0, seed=1)[0]
    T_render = tps.T_of(net, F)
    for z in (None, ZOOMS):
        n, k, T = gpu_cover(None, None, z, sh, sw, oh, ow, net=net, F=F)
        assert np.array_equal(T.view(np.uint32), T_render.view(np.uint32))
        n2, k2, _ = gpu_cover(tin.v_src(B), T, z, sh, sw, oh, ow)
        assert n.tolist() == n2.tolist() and k.tolist() == k2.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the clip driver

N_CLIP, MH, MW = 12, 32, 64


def _model(weights, H, W):
    from coupe.dvsg_amd.model import StabNet
    model = StabNet(H, W).load_weights(weights)
    model.get_evaluation_model(7)
    return model


@pytest.fixture(scope="module")
def clip_state(synthetic_weights):
    """the model, a 12-frame float32 clip at model size, the parent's stabilised frames, and the loop's own F_t / pool,
    re-run here with the driver's building blocks (stabilize_clip does not return F_t)"""
    import torch
    from coupe.dvsg_amd import clip
    model = _model(synthetic_weights, MH, MW)
    frames = tin.smooth_frames(5, N_CLIP, MH, MW)
    base = clip.stabilize_clip(model, None, frames)
    table = torch.from_numpy(clip.window_index_table(N_CLIP)).cuda()
    pool = torch.empty((2 * N_CLIP, MH, MW, 3), device="cuda")
    pool[:N_CLIP] = torch.from_numpy(frames).cuda()
    F = torch.empty((N_CLIP, 25, 2), device="cuda")
    for k in range(N_CLIP):
        model.locnet.stabilize_ring(pool, table[k:k + 1], pool[N_CLIP + k:N_CLIP + k + 1], F[k:k + 1], precision=model.precision)
    _sync()
    assert np.array_equal(pool[N_CLIP:].cpu().numpy().view(np.uint32), base.view(np.uint32)), "the test's loop is not the driver's"
    return dict(model=model, frames=frames, base=base, F=F.cpu().numpy(), pool=pool)


def _border_mask(model, F, H, W):
    """bool [N,H,W]: the pixels of the plain H x W grid that sampler A leaves black on an H x W frame, from the x_s, y_s the
    warp writes for the T of F_t"""
    n = F.shape[0]
    _, xs, ys = gpu_warp_zoom(None, tin.v_src(n), tps.T_of(model.locnet, F), None, H, W)
    return ~crop_ref.valid(xs.reshape(n, H, W), ys.reshape(n, H, W), H, W)


def test_clip_without_crop_is_the_parent_s_output(clip_state):
    from coupe.dvsg_amd import clip
    s = clip_state
    out, side = clip.stabilize_clip(s["model"], None, s["frames"], side_by_side=True, crop=None)
    assert np.array_equal(out.view(np.uint32), s["base"].view(np.uint32))
    out1 = clip.stabilize_clip(s["model"], None, s["frames"], crop=1.0)
    assert np.array_equal(out1.view(np.uint32), s["base"].view(np.uint32)), "crop=1.0 at model size must be the uncropped frames"


def test_clip_auto_crop(clip_state):
    from coupe.dvsg_amd import clip
    s = clip_state
    model, F = s["model"], s["F"]
    info = {}
    out, side = clip.stabilize_clip(model, None, s["frames"], crop="auto", crop_info=info, side_by_side=True)
    scan = clip.crop_scan(model, F, (MH, MW))
    print("CROP clip: max |F_t| %.3g, free %s, zoom %.6f" % (float(np.abs(F).max()), np.round(scan["free"], 4).tolist(), info["zoom"]))
    assert np.array_equal(info["free"], scan["free"]), "the loop's F_t changed"
    assert info["zoom"] == float(clip.crop_zoom(scan["free"], out_hw=(MH, MW))) == info["cropping_ratio"]
    assert info["zoom"] == float(crop_ref.crop_zoom(scan["free"], out_hw=(MH, MW)))
    assert (info["border_pixels"] == 0).all(), info
    assert len(info["limited"]) == 0
    # the frames are per-frame dvsg_tps_warp_zoom_f32 calls with the T of F_t
    T = tps.T_of(model.locnet, F)
    z = np.array([info["zoom"]], dtype=F32)
    for k in range(N_CLIP):
        want, _, _ = gpu_warp_zoom(s["frames"][k:k + 1], tin.v_src(1), T[k:k + 1], z, MH, MW, want_xy=False)
        assert np.array_equal(out[k].view(np.uint32), want[0].view(np.uint32)), k
    from oracle import frames as ofr
    assert np.array_equal(side[:, :, :MW], ofr.to_uint8(s["frames"])) and np.array_equal(side[:, :, MW:], ofr.to_uint8(out))
    # every uncropped frame has border pixels, where the scan's predicate says (cancelled weights: |v| at the rounding of
    # the blend, the frames are ~0.5); the crop has none, and its last row and column are filled
    bad = _border_mask(model, F, MH, MW)
    assert bad.reshape(N_CLIP, -1).sum(1).tolist() == scan["border_pixels"].tolist() and (scan["border_pixels"] > 0).all()
    assert (np.abs(s["base"][bad]) < 1e-5).all()
    assert (out[:, -1].max(axis=(1, 2)) > 1e-2).all() and (out[:, :, -1].max(axis=(1, 2)) > 1e-2).all()
    # the loop's state is what it was: a second uncropped run gives the parent's frames
    assert np.array_equal(clip.stabilize_clip(model, None, s["frames"]).view(np.uint32), s["base"].view(np.uint32))


def test_clip_auto_crop_at_source_resolution(synthetic_weights, clip_state):
    import torch
    from coupe.dvsg_amd import clip
    model = clip_state["model"]
    H0, W0 = 48, 80
    src = (tin.smooth_frames(9, N_CLIP, H0, W0) * 255).astype(np.uint8)
    base, base_side = clip.stabilize_clip(model, None, src, source_res=True, side_by_side=True, as_uint8=True)
    info = {}
    out, side = clip.stabilize_clip(model, None, src, source_res=True, side_by_side=True, as_uint8=True, crop="auto", crop_info=info)
    out32 = clip.stabilize_clip(model, None, src, source_res=True, crop=info["zoom"])
    assert out.shape == (N_CLIP, H0, W0, 3) and out.dtype == np.uint8
    assert np.array_equal(side[:, :, :W0], src) and np.array_equal(side[:, :, W0:], out)
    assert (info["border_pixels"] == 0).all() and len(info["limited"]) == 0 and 0.5 < info["zoom"] < 1.0
    assert (out[:, -1].max(axis=(1, 2)) > 0).all() and (out[:, :, -1].max(axis=(1, 2)) > 0).all()
    # the F_t of the loop: the uncropped source render's T is what the crop's render wrote, so render per frame with it
    model_frames = clip.stabilize_clip(model, None, src)     # the loop at model size, untouched by source_res and crop
    assert model_frames.shape == (N_CLIP, MH, MW, 3)
    # recover F_t by running the loop's blocks as the fixture does
    table = torch.from_numpy(clip.window_index_table(N_CLIP)).cuda()
    pool = torch.empty((2 * N_CLIP, MH, MW, 3), device="cuda")
    from coupe.dvsg_amd import _lib
    sd = tps._dev(src)
    _lib.call("dvsg_frames_resize_u8_f32", sd.data_ptr(), N_CLIP, H0, W0, 0, pool.data_ptr(), MH, MW, 0, 0, 0, tps._stream())
    F = torch.empty((N_CLIP, 25, 2), device="cuda")
    for k in range(N_CLIP):
        model.locnet.stabilize_ring(pool, table[k:k + 1], pool[N_CLIP + k:N_CLIP + k + 1], F[k:k + 1], precision=model.precision)
    _sync()
    assert np.array_equal(pool[N_CLIP:].cpu().numpy().view(np.uint32), model_frames.view(np.uint32))
    F = F.cpu().numpy()
    scan = clip.crop_scan(model, F, (H0, W0))
    assert np.array_equal(scan["free"], info["free"]) and info["zoom"] == float(clip.crop_zoom(scan["free"], out_hw=(H0, W0)))
    # the uncropped render is black where the predicate says, on every frame (which rows and columns depends on F_t)
    bad = _border_mask(model, F, H0, W0)
    assert bad.reshape(N_CLIP, -1).sum(1).tolist() == scan["border_pixels"].tolist() and scan["border_pixels"].sum() > 0
    assert (base[bad] == 0).all()
    z = np.full(N_CLIP, info["zoom"], dtype=F32)
    _, want32, want8 = gpu_render_zoom(model.locnet, F, src, 0, z, W0, 0)
    assert np.array_equal(out, want8) and np.array_equal(out32.view(np.uint32), want32.view(np.uint32))


def test_a_large_motion_is_limited_by_crop_min(clip_state):
    import torch
    from coupe.dvsg_amd import clip
    s = clip_state
    F = torch.from_numpy(s["F"]).cuda()
    scale, info = 1.0, {}
    for _ in range(12):                                       # F_t scaled up until a frame asks for less than crop_min
        info = {}
        clip._choose_zoom(s["model"], (F * scale).contiguous(), (MH, MW), "auto", None, 0.75, info)
        if len(info["limited"]):
            break
        scale *= 2.0
    assert len(info["limited"]) and info["zoom"] == 0.75
    margin = 2.0 / (MH - 1)
    assert info["limited"].tolist() == np.nonzero(info["free"] - margin < 0.75)[0].tolist()


def test_errors_are_python_errors(clip_state):
    from coupe.dvsg_amd import clip
    from coupe.dvsg_amd._lib import DvsgError
    s = clip_state
    for bad in ("tight", 0.0, -0.5, 1.5, float("nan"), True, [0.9]):
        with pytest.raises(ValueError):
            clip.stabilize_clip(s["model"], None, s["frames"], crop=bad)
    with pytest.raises(ValueError):
        clip.stabilize_clip(s["model"], None, s["frames"], crop="auto", crop_min=0.0)
    with pytest.raises(ValueError):
        clip.crop_scan(s["model"], s["F"], (1, 8))
    with pytest.raises(ValueError):
        clip.crop_scan(s["model"], s["F"], (MH, MW), out_hw=(8, 1))
    with pytest.raises(ValueError):
        clip.crop_scan(s["model"], s["F"], (MH, MW), out_hw=(50000, 50000))      # D >= 2^31 - 1: refused on the host
    with pytest.raises(ValueError):
        clip.crop_scan(s["model"], s["F"][:, :24], (MH, MW))
    with pytest.raises(ValueError):
        clip.crop_scan(s["model"], s["F"], (MH, MW), zoom=[0.9, 0.8])
    coord, T = case_T("near", CASES[1])
    with pytest.raises(DvsgError):                            # the C entry refuses the same shapes with a status
        gpu_cover(coord, T, None, 5, 64, 1, 64)
    with pytest.raises(DvsgError):
        cover_bytes(1, 46342, 46342)
