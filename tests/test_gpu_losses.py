"""GPU checks of the fused test-time losses (dvsg_loss_*, coupe.dvsg_amd.trainer).

1. Per pixel: the fused image term's `pred` and mask plane are the bits of dvsg_tps_warp_f32 on u and on ones; the SURF
   kernel's gathered coordinates are the bits of its x_s / y_s.
2. Sums: every per-pixel term is formed in NumPy float32, op by op in the reference's order, from the outputs of the existing
   entry points (dvsg_tps_warp_f32, dvsg_flow_warp_f32) and summed in float64; the kernel's numerator and denominator lie
   within 1.06 d 2^-24 sum|term| of that.  The kernels accumulate in float64 (loss_kernels.hip), so d = D_ADDS = 1.
3. Against the reference's arithmetic: the same losses from tests/losses_ref.py on the oracle's warps.  The yardstick is D,
   the distance between the oracle's loss and the loss computed from the existing kernels' outputs, both summed in float64
   (sampler A's border discontinuities put a few O(1) pixel differences between any float32 evaluation and the oracle); the
   fused result must be within D plus the summation bound of item 2, propagated through num / den -- nothing else is
   allowed for.  Both losses form their per-pixel terms in float32 like the TF graph and like item 2: with float64 terms a
   case where the warps agree exactly (D = 0, the 1 x 1 frames) would measure the reference's own float32 term rounding, up
   to 2^-24 (|pred m| + |gt m|) / |pred m - gt m| per term, against a bound that holds no such allowance.
   D is printed per case (run with -s).  Measured on these inputs: temporal term D = 0 in all 27 cases; image term D = 0
   (1 x 1), 5.4e-9 / 2.1e-8 (5 x 7, B = 1 / 3), 1.2e-8 / 2.4e-8 (33 x 65), 4.3e-9 / 2.7e-7 (288 x 512), 2.9e-8 (4 x 720 x 1280)
   on losses of 0.006 ... 0.12.
5. Reproducibility: the same call twice, on one and on two streams, returns identical bits.

No pixel is masked out or skipped anywhere.  Item 4 (build_loss_train on the graph of StabNet.get_train_model, the
clip driver, two ranks, the no-three-channel-mask bookkeeping) is tests/test_gpu_score.py; build_loss_train on VALUES is
checked here."""
import numpy as np
import pytest
import torch

import inputs
import losses_ref as L

pytestmark = pytest.mark.gpu

D_ADDS = 1                      # float32 additions on the longest path of the kernels' summation: none, they add in float64
EPS = 1.06 * D_ADDS * 2.0 ** -24

SHAPES = [(1, 1), (5, 7), (33, 65), (288, 512)]
CASES = [(B, H, W) for (H, W) in SHAPES for B in (1, 3)] + [(4, 720, 1280)]
FLOWS = ("cfg3", "constant", "border")


def make_flow(kind, seed, B, H, W):
    if kind == "cfg3":
        return inputs.smooth_flow(seed, B, H, W)
    if kind == "constant":
        return np.broadcast_to(np.array([2.5, -1.25], np.float32), (B, H, W, 2)).copy()
    f = np.empty((B, H, W, 2), np.float32)      # +-40 px: every pixel near a border crosses it
    f[..., 0] = np.where((np.arange(W) % 2 == 0)[None, None, :], 40.0, -40.0)
    f[..., 1] = np.where((np.arange(H) % 2 == 0)[None, :, None], -40.25, 40.5)
    return f


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def within(got, want, bound):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    return bool(np.all(np.abs(got - want) <= bound))


def setup(B, H, W, seed=3):
    from coupe.dvsg_amd import trainer
    from coupe.dvsg_amd.ThinPlateSpline import ThinPlateSpline
    u = inputs.smooth_frames(seed, B, H, W)
    gt = inputs.smooth_frames(seed + 1, B, H, W)
    F = inputs.control_vectors(seed, B, scale=0.08)   # large enough to push border pixels outside the frame
    V = inputs.v_src(B)
    c, T = trainer.solve_T(dev(V), dev(F))
    pred, xs, ys = ThinPlateSpline(dev(u), dev(V), dev(F), [H, W])
    ones3, _, _ = ThinPlateSpline(torch.ones((B, H, W, 3), device="cuda"), dev(V), dev(F), [H, W])
    return dict(u=u, gt=gt, F=F, V=V, c=c, T=T, pred=pred, xs=xs, ys=ys, ones3=ones3)


@pytest.fixture(scope="module")
def cache():
    return {}


def case(cache, B, H, W):
    if (B, H, W) not in cache:
        cache.clear()   # one case's tensors at a time
        cache[(B, H, W)] = setup(B, H, W)
    return cache[(B, H, W)]


@pytest.mark.parametrize("B,H,W", CASES)
def test_image_term_bits_sums_and_oracle(cache, B, H, W):
    from coupe.dvsg_amd import trainer
    from oracle import thin_plate_spline as otps
    s = case(cache, B, H, W)
    mean, ps, sums, pred, mask = trainer.image_terms(dev(s["u"]), dev(s["gt"]), s["c"], s["T"], want_pred=True)
    # 1. bits
    assert torch.equal(pred, s["pred"])
    assert torch.equal(s["ones3"][..., 0], s["ones3"][..., 1]) and torch.equal(s["ones3"][..., 0], s["ones3"][..., 2])
    assert torch.equal(mask, s["ones3"][..., 0])
    # 2. sums: float32 terms from the existing kernels' outputs, float64 sums
    p_np, m_np = s["pred"].cpu().numpy(), s["ones3"][..., 0].cpu().numpy()
    num, den, absden = L.masked_mse_sums(p_np, s["gt"], m_np, np.float32)
    sums = sums.cpu().numpy()
    print("image %s: num %s den %s" % ((B, H, W), sums[:, 0], sums[:, 1]))
    assert within(sums[:, 0], num, EPS * num)
    assert within(sums[:, 1], den, EPS * absden)
    # without the optional outputs: the same sums
    mean2, ps2, sums2, _, _ = trainer.image_terms(dev(s["u"]), dev(s["gt"]), s["c"], s["T"])
    assert np.array_equal(sums2.cpu().numpy(), sums) and torch.equal(ps2, ps) and torch.equal(mean2, mean)
    # 3. the oracle's arithmetic
    o_pred, _, _ = otps.ThinPlateSpline(s["u"], s["V"], s["F"], [H, W])
    o_mask, _, _ = otps.ThinPlateSpline(np.ones((B, H, W, 3), np.float32), s["V"], s["F"], [H, W])
    loss_o = L.masked_MSE(o_pred, s["gt"], o_mask[..., 0], np.float32)
    loss_k = L.masked_MSE(p_np, s["gt"], m_np, np.float32)   # float64 sums from the existing kernels' outputs
    D = abs(loss_o - loss_k)
    fused64 = float(np.mean(L.div_no_nan(sums[:, 0], sums[:, 1])))
    safe = np.where(den != 0, den, 1.0)
    sb = float(np.mean(np.where(den != 0, EPS * num / safe + num * EPS * absden / safe ** 2, 0.0)))
    print("image %s: oracle %.9g kernels-f64 %.9g D %.3g fused %.9g bound %.3g" % ((B, H, W), loss_o, loss_k, D, fused64, D + sb))
    assert abs(fused64 - loss_o) <= D + sb
    # the float32 outputs: num and den rounded to float32, one division, one mean -- 4 roundings
    assert abs(float(mean.item()) - fused64) <= 4 * 2.0 ** -24 * abs(fused64)
    assert within(ps.cpu().numpy(), L.div_no_nan(sums[:, 0], sums[:, 1]), 3 * 2.0 ** -24 * np.abs(L.div_no_nan(sums[:, 0], sums[:, 1])))


@pytest.mark.parametrize("kind", FLOWS)
@pytest.mark.parametrize("B,H,W", CASES)
def test_temporal_term_sums_and_oracle(cache, B, H, W, kind):
    from coupe.dvsg_amd import trainer
    from coupe.dvsg_amd.warp_with_optical_flow import tf_warp
    from oracle import warp_with_optical_flow as oflow
    s = case(cache, B, H, W)
    flow = make_flow(kind, 11, B, H, W)
    pred, mask_pred = s["pred"], s["ones3"][..., 0].contiguous()
    gt = s["gt"]                                             # stands for s_t_1_pred
    mask_gt = inputs.smooth_frames(5, B, H, W, C=1)[..., 0]   # any plane in [0,1] serves as s_t_1_pred_mask
    mean, ps, sums = trainer.temporal_terms(pred, dev(gt), mask_pred, dev(mask_gt), dev(flow))
    sums = sums.cpu().numpy()
    # 2. the existing entry point on the frame and on the mask plane (C = 1), float32 terms, float64 sums
    pw = tf_warp(pred, dev(flow), H, W).cpu().numpy()
    mw = tf_warp(mask_pred.unsqueeze(3), dev(flow), H, W).cpu().numpy()[..., 0]
    m32 = mw * mask_gt                                       # trainer.py:250, float32
    num, den, absden = L.masked_mse_sums(pw, gt, m32, np.float32)
    print("temporal %s %s: num %s den %s" % ((B, H, W), kind, sums[:, 0], sums[:, 1]))
    assert within(sums[:, 0], num, EPS * num)
    assert within(sums[:, 1], den, EPS * absden)
    # 3. the oracle's tf_warp on the same inputs
    p_np, mp_np = pred.cpu().numpy(), mask_pred.cpu().numpy()
    o_pw = oflow.tf_warp(p_np, flow, H, W)
    o_mw = oflow.tf_warp(mp_np[..., None], flow, H, W)[..., 0]
    loss_o = L.temporal_loss(o_pw, gt, o_mw, mask_gt, np.float32)
    loss_k = L.temporal_loss(pw, gt, mw, mask_gt, np.float32)
    D = abs(loss_o - loss_k)
    fused64 = float(np.mean(L.div_no_nan(sums[:, 0], sums[:, 1])))
    safe = np.where(den != 0, den, 1.0)
    sb = float(np.mean(np.where(den != 0, EPS * num / safe + num * EPS * absden / safe ** 2, 0.0)))
    print("temporal %s %s: oracle %.9g kernels-f64 %.9g D %.3g fused %.9g" % ((B, H, W), kind, loss_o, loss_k, D, fused64))
    assert abs(fused64 - loss_o) <= D + sb
    assert abs(float(mean.item()) - fused64) <= 4 * 2.0 ** -24 * abs(fused64)


@pytest.mark.parametrize("C,plane", [(3, True), (3, False), (1, False), (5, True)])
@pytest.mark.parametrize("B,H,W", CASES)
def test_masked_mse_sums(B, H, W, C, plane):
    from coupe.dvsg_amd import trainer
    p = inputs.smooth_frames(21, B, H, W, C)
    g = inputs.smooth_frames(22, B, H, W, C)
    m = inputs.smooth_frames(23, B, H, W, 1 if plane else C)
    m = m[..., 0] if plane else m
    m[:, :, : W // 2] = 0.0
    mean, ps, sums = trainer.masked_mse_terms(dev(p), dev(g), dev(m))
    num, den, absden = L.masked_mse_sums(p, g, m, np.float32)
    sums = sums.cpu().numpy()
    assert within(sums[:, 0], num, EPS * num) and within(sums[:, 1], den, EPS * absden)
    want = L.masked_MSE(p, g, m, np.float32)
    assert abs(float(mean.item()) - want) <= 4 * 2.0 ** -24 * abs(want) + 2 * EPS * abs(want)
    zero = trainer.masked_MSE(dev(p), dev(g), torch.zeros_like(dev(m)))
    assert float(zero.item()) == 0.0                         # div_no_nan


@pytest.mark.parametrize("B", [1, 3])
def test_grid_terms(B):
    from coupe.dvsg_amd import trainer
    V = inputs.v_src(B)
    zero = trainer.distortion_loss(dev(V), torch.zeros((B, 25, 2), device="cuda"), 5)
    assert float(zero.item()) == 0.125                       # as written: not 0 at F = 0
    F1 = np.zeros((B, 25, 2), np.float32)
    F1[:, 12, 0] = 0.25
    assert float(trainer.distortion_loss(dev(V), dev(F1), 5).item()) == 0.140625   # every operand exact in float32
    F = inputs.control_vectors(9, B)
    im, dm, ident, dist = trainer.grid_terms(dev(V), dev(F), 5)
    # float32 chains of ~12 ops on O(1) values against float64: 16 roundings
    tol = 16 * 2.0 ** -24
    assert within(dist.cpu().numpy(), L.distortion_per_sample(V, F, 5), tol)
    assert abs(float(dm.item()) - L.distortion_loss(V, F, 5)) <= tol
    assert abs(float(im.item()) - L.identity_loss(F)) <= tol * L.identity_loss(F)
    assert within(ident.cpu().numpy(), np.mean(np.abs(F.astype(np.float64)), axis=(1, 2)), tol)
    assert float(trainer.identity_loss(dev(F)).item()) == float(im.item())


def make_surf(seed, B, N, H, W):
    rng = np.random.default_rng(seed)
    surf = np.zeros((B, 2, N, 2), np.float32)
    n_real = max(1, N - 5)                                   # the last 5 stay zero: padding, counted like the reference does
    surf[:, :, :n_real, 0] = rng.integers(0, W, (B, 2, n_real))
    surf[:, :, :n_real, 1] = rng.integers(0, H, (B, 2, n_real))
    surf[:, 1, 0] = (0, H)                                   # idx = h w: the appended -1
    surf[:, 1, 1] = (W - 1, H - 1)                           # the last pixel
    return surf


@pytest.mark.parametrize("B,H,W", CASES)
def test_surf_term_bits_and_sums(cache, B, H, W):
    from coupe.dvsg_amd import trainer
    s = case(cache, B, H, W)
    N = 50
    surf = make_surf(31, B, N, H, W)
    dims = np.arange(1, B + 1, dtype=np.float32) * 7.0
    dims[0] = 0.0 if B > 1 else 45.0                         # a zero divisor goes through div_no_nan
    mean, ps, sums, coords = trainer.surf_terms(dev(surf), s["T"], s["c"], dev(dims), W, H, want_coords=True)
    xs, ys = s["xs"].cpu().numpy().reshape(B, -1), s["ys"].cpu().numpy().reshape(B, -1)
    with np.errstate(all="ignore"):
        num, got = L.surf_sums(surf, xs, ys, W, H, np.float32)   # gathers from the existing kernel's x_s / y_s
    assert np.array_equal(coords.cpu().numpy(), got)         # 1. bits, the sentinel included
    assert coords[:, 0].cpu().numpy().tolist() == [[-1.0, -1.0]] * B
    sums = sums.cpu().numpy()
    with np.errstate(invalid="ignore"):
        ok = np.abs(sums - num) <= EPS * num
    # H = 1 or W = 1: the reference divides by w - 1 = 0 (:369-370), both sides give the same non-finite sum
    assert np.all(ok | (~np.isfinite(num) & ~np.isfinite(sums)))
    if H > 1 and W > 1:
        want = L.div_no_nan(num, dims.astype(np.float64))
        assert within(ps.cpu().numpy(), want, 3 * 2.0 ** -24 * np.abs(want))
        if B > 1:
            assert float(ps[0].item()) == 0.0
        assert abs(float(mean.item()) - float(np.mean(want))) <= 4 * 2.0 ** -24 * float(np.mean(want))
        assert float(trainer.get_surf_loss(dev(surf), s["T"], s["c"], dev(dims), B, W, H).item()) == float(mean.item())


def loss_inputs(B, H, W):
    ins = dict(u_t=inputs.smooth_frames(41, B, H, W), u_t_1=inputs.smooth_frames(42, B, H, W),
               s_t_gt=inputs.smooth_frames(43, B, H, W), s_t_1_gt=inputs.smooth_frames(44, B, H, W),
               of_t=inputs.smooth_flow(45, B, H, W), surfs_t=make_surf(46, B, 40, H, W), surfs_t_1=make_surf(47, B, 40, H, W),
               surfs_dim_t=np.full(B, 35.0, np.float32), surfs_dim_t_1=np.full(B, 35.0, np.float32))
    outs = dict(F_t=inputs.control_vectors(48, B), F_t_1=inputs.control_vectors(49, B), V_src=inputs.v_src(B),
                num_control_points=5)
    return {k: dev(v) for k, v in ins.items()}, {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in outs.items()}


def test_build_loss_train_equals_the_term_by_term_calls_and_builds_no_mask3():
    from coupe.dvsg_amd import trainer
    B, H, W = 3, 33, 65
    ins, outs = loss_inputs(B, H, W)
    coefs = dict(image=2.0, identity=0.5, temporal=3.0, surf=0.25, distortion=1.5)
    trainer.stats.clear()
    loss = trainer.build_loss_train(ins, outs, coefs=coefs)
    assert trainer.stats['mask3'] == 0                       # no [B,H,W,3] mask was built or taken apart
    assert list(loss) == ['image', 'identity', 'temporal', 'surf', 'distortion', 'total']
    c_t, T_t = trainer.solve_T(outs['V_src'], outs['F_t'])
    c_1, T_1 = trainer.solve_T(outs['V_src'], outs['F_t_1'])
    i1 = trainer.image_terms(ins['u_t_1'], ins['s_t_1_gt'], c_1, T_1, True)
    i0 = trainer.image_terms(ins['u_t'], ins['s_t_gt'], c_t, T_t, True)
    want = dict(image=i1[0] + i0[0],
                identity=trainer.identity_loss(outs['F_t']) + trainer.identity_loss(outs['F_t_1']),
                temporal=trainer.temporal_loss(i0[3], i1[3], i0[4], i1[4], ins['of_t'], H, W),
                surf=trainer.get_surf_loss(ins['surfs_t_1'], T_1, c_1, ins['surfs_dim_t_1'], B, W, H)
                + trainer.get_surf_loss(ins['surfs_t'], T_t, c_t, ins['surfs_dim_t'], B, W, H),
                distortion=trainer.distortion_loss(outs['V_src'], outs['F_t_1'], 5)
                + trainer.distortion_loss(outs['V_src'], outs['F_t'], 5))
    for k, v in want.items():
        assert float(loss[k].item()) == float(v.item()), k
    total = sum(np.float32(coefs[k]) * np.float32(loss[k].item()) for k in want)
    assert abs(float(loss['total'].item()) - float(total)) <= 8 * 2.0 ** -24 * abs(float(total))
    only = trainer.build_loss_train(ins, outs, loss_applied=('identity', 'distortion'))
    assert list(only) == ['identity', 'distortion', 'total'] and trainer.stats['pred'] == 4   # no frames warped for these


def test_same_call_twice_and_on_two_streams_gives_identical_bits():
    from coupe.dvsg_amd import trainer
    B, H, W = 3, 288, 512
    ins, outs = loss_inputs(B, H, W)

    def run():
        loss = trainer.build_loss_train(ins, outs)
        c, T = trainer.solve_T(outs['V_src'], outs['F_t'])
        img = trainer.image_terms(ins['u_t'], ins['s_t_gt'], c, T, True)
        tmp = trainer.temporal_terms(img[3], ins['s_t_1_gt'], img[4], img[4], ins['of_t'])
        return [v.clone() for v in loss.values()] + [img[1], img[2], tmp[1], tmp[2]]

    a = run()
    b = run()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = run()
    with torch.cuda.stream(s2):
        d = run()
    torch.cuda.synchronize()
    for other in (b, c, d):
        for x, y in zip(a, other):
            assert torch.equal(x, y)
