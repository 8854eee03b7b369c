"""GPU: the float16 variant of localizationNet (BASELINE.json configs[4] "fp16 MFMA convs").
float16 storage cannot be bit-compatible with the float32 reference; this file STATES the measured
error against the float32 oracle (tolerances are ~3x the values observed on MI355X) and checks the
properties that must still hold exactly.

The float16 mode keeps ACTIVATIONS in float16 and the conv weights as float16 hi / lo pairs
(w ~ hi + 2^-11 lo, two MFMAs per product): a plain float16 weight is wrong by up to 2^-12 relative
in the same way at every pixel, an error the global average pool cannot average away -- it was 9/10
of the mode's F_t error (2.0e-5 at 720p, warped pixels 1.5e-3).  With the pairs: F_t 1.7e-6, source
grid 3e-3 px, warped pixels 3.9e-4 at 720p, the same as the float32 path end to end."""
import numpy as np
import pytest

import inputs
from oracle import networks as onet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net(synthetic_weights):
    import torch
    assert torch.cuda.is_available()
    from coupe.dvsg_amd.networks import LocNet
    return LocNet(synthetic_weights)


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 70, 100), (3, 33, 47)])   # 47: rows that are not 16-byte aligned
def test_f16_stages_track_the_f32_oracle(net, synthetic_weights, B, H, W):
    x = inputs.window_frames(301, B, H, W)
    taps = {}
    F_ref = onet.localizationNet(x, 25, synthetic_weights, taps=taps)
    names = ["conv1", "pool1", "block1/unit_3", "block2/unit_4", "block3/unit_6", "block4/unit_3"]
    stages = [0, 1, 4, 8, 14, 17]
    for stage, name in zip(stages, names):
        act = net.tap(x, stage, precision="f16").cpu().numpy()
        ref = taps[name]
        assert act.shape == ref.shape
        rel = np.abs(act - ref).max() / np.abs(ref).max()
        # float16 has an 11-bit significand: ~5e-4 per rounding of an activation, over up to 50 layers
        assert rel < 1e-2, "%s: relative error %.3g" % (name, rel)
    F = net.forward(x, precision="f16").cpu().numpy()
    err = np.abs(F - F_ref).max()
    assert err < 5e-5, "F_t error %.3g (|F| ~ %.3g)" % (err, np.abs(F_ref).max())
    F32 = net.forward(x, precision="f32").cpu().numpy()
    assert np.abs(F32 - F_ref).max() <= 1e-5          # the f32 path is untouched by the f16 weights


def test_f16_stabilize_and_determinism(net, synthetic_weights):
    import torch
    from coupe.dvsg_amd.model import Session, StabNet
    from oracle import model as omodel
    from oracle.thin_plate_spline import border_discontinuity_mask
    B, H, W = 2, 72, 128
    x = inputs.window_frames(311, B, H, W)
    u = x[..., 18:]
    model = StabNet(H, W).load_weights(synthetic_weights)
    model.precision = "f16"
    ins, outs = model.get_evaluation_model(7)
    feed = {ins["patches_t"]: x, ins["u_t"]: u}
    got, F, xs, ys = Session().run([outs["s_t_pred"], outs["F_t"], outs["x_offset_t"], outs["y_offset_t"]], feed)
    again = Session().run(outs["s_t_pred"], feed)
    assert np.array_equal(got, again)                  # deterministic
    ref, rF, rx, ry = omodel.StabNet(H, W).run(synthetic_weights, x, u, fetch=("s_t_pred", "F_t", "x_offset_t", "y_offset_t"))
    gerr = max(np.abs(xs - rx).max() * W / 2, np.abs(ys - ry).max() * H / 2)
    mask = border_discontinuity_mask(rx, ry, H, W, delta=0.2).reshape(B, H, W)
    perr = np.abs(got - ref).max(axis=3)[~mask].max()
    # stated values for the float16 path on these small frames (float32 path: < 2e-2 px, < 3e-3)
    assert gerr < 5e-2, "grid error %.3g px" % gerr
    assert perr < 6e-3, "pixel error %.3g" % perr


def test_f16_meets_the_pixel_tolerance_at_720p(synthetic_weights):
    """BASELINE.json's tolerance (warped-frame max abs error < 1e-3) for the float16 mode at 1280x720,
    two windows end to end against the float32 CPU oracle: F_t < 1e-5 (measured 1.7e-6), source grid
    < 2e-2 px (3e-3), pixels < 1e-3 (3.9e-4) outside the counted sampler-A border-discontinuity pixels.
    With plain float16 weights (dvsg_debug_set_option("f16_split", 0)) the same numbers are 2.0e-5,
    9.7e-3 px and 1.5e-3: the hi / lo weight pairs are what closes the gap."""
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.model import Session, StabNet
    from oracle import thin_plate_spline as otps
    from oracle.cnn_torch import TorchLocNet
    B, H, W = 2, 720, 1280
    x = inputs.window_frames(7, B, H, W)
    u = np.ascontiguousarray(x[..., 18:])
    model = StabNet(H, W).load_weights(synthetic_weights)
    model.precision = "f16"
    ins, outs = model.get_evaluation_model(7)
    fetch = [outs["s_t_pred"], outs["F_t"], outs["x_offset_t"], outs["y_offset_t"]]
    pred, F, xs, ys = Session().run(fetch, {ins["patches_t"]: x, ins["u_t"]: u})
    F_ref = TorchLocNet(synthetic_weights).forward(x)
    r_pred, r_xs, r_ys = otps.ThinPlateSpline(u, inputs.v_src(B), F_ref, (H, W))
    border = otps.border_discontinuity_mask(r_xs, r_ys, H, W, delta=3e-2).reshape(B, H, W)
    ferr = np.abs(F - F_ref).max()
    gerr = max(np.abs(xs - r_xs).max() * W / 2, np.abs(ys - r_ys).max() * H / 2)
    perr = np.abs(pred - r_pred).max(axis=3)[~border].max()
    print("f16 (hi/lo weights) at 720p: F_t %.2e, grid %.2e px, pixels %.2e" % (ferr, gerr, perr))
    assert ferr < 1e-5 and gerr < 2e-2 and perr < 1e-3 and border.mean() < 0.01
    _lib.call("dvsg_debug_set_option", b"f16_split", 0)
    try:
        F_plain = Session().run(outs["F_t"], {ins["patches_t"]: x, ins["u_t"]: u})
    finally:
        _lib.call("dvsg_debug_set_option", b"f16_split", 1)
    assert np.abs(F_plain - F_ref).max() > 3 * ferr          # plain float16 weights are what it costs


def test_conv_gemm_f16_layer(net):
    """One 3x3 and one 1x1 layer through dvsg_conv_gemm_f16 against float32 math on the same
    (float16-rounded) operands: only the float32 accumulation order differs.  Then the same layers
    with float32 weights given as hi / lo float16 pairs (dvsg_conv_gemm_f16s) against float32 math on
    the UNROUNDED weights, small batch (split-K) and large (plain tiles, stream-K tail)."""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    for k, stride, cin, cout, h, w in [(3, 1, 64, 64, 20, 28), (3, 2, 128, 128, 21, 17), (1, 1, 256, 64, 9, 13)]:
        B = 2
        x = (torch.rand((B, h, w, cin), generator=g, device=dev) - 0.3).half()
        K = k * k * cin
        wt = ((torch.rand((cout, K), generator=g, device=dev) - 0.5) * (2.0 / K ** 0.5)).half()
        bias = torch.rand((cout,), generator=g, device=dev) - 0.5
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        res = (torch.rand((B, ho, wo, cout), generator=g, device=dev) - 0.5).half()
        y = torch.empty((B, ho, wo, cout), device=dev, dtype=torch.float16)
        _lib.call("dvsg_conv_gemm_f16", x.data_ptr(), wt.data_ptr(), bias.data_ptr(), res.data_ptr(), y.data_ptr(),
                  B, h, w, cin, cout, k, stride, 1, 1, 0, 0, torch.cuda.current_stream().cuda_stream)
        w4 = wt.float().reshape(cout, k, k, cin).permute(0, 3, 1, 2)
        ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w4, bias, stride=stride, padding=k // 2)
        ref = torch.relu(ref.permute(0, 2, 3, 1) + res.float())
        err = float((y.float() - ref).abs().max())
        assert err < 4e-3 * max(1.0, float(ref.abs().max())), (k, stride, cin, err)
        # hi / lo pairs of float32 weights
        w32 = (torch.rand((cout, K), generator=g, device=dev) - 0.5) * (2.0 / K ** 0.5)
        hi = w32.half()
        lo = ((w32 - hi.float()) * 2048.0).half()
        ws = torch.stack([hi.reshape(cout // 64, 64, K), lo.reshape(cout // 64, 64, K)], 1).reshape(2 * cout, K).contiguous()
        scratch = torch.empty(160 << 20, dtype=torch.uint8, device=dev)   # tickets + slabs + room for the packed weight copies
        for Bs in (2, 40):
            xs = (torch.rand((Bs, h, w, cin), generator=g, device=dev) - 0.3).half()
            rs = (torch.rand((Bs, ho, wo, cout), generator=g, device=dev) - 0.5).half()
            ys = torch.empty((Bs, ho, wo, cout), device=dev, dtype=torch.float16)
            _lib.call("dvsg_conv_gemm_f16s", xs.data_ptr(), ws.data_ptr(), bias.data_ptr(), rs.data_ptr(), ys.data_ptr(),
                      Bs, h, w, cin, cout, k, stride, 1, 1, scratch.data_ptr(), scratch.numel(),
                      torch.cuda.current_stream().cuda_stream)
            w4 = w32.reshape(cout, k, k, cin).permute(0, 3, 1, 2)
            ref = torch.nn.functional.conv2d(xs.float().permute(0, 3, 1, 2), w4, bias, stride=stride, padding=k // 2)
            ref = torch.relu(ref.permute(0, 2, 3, 1) + rs.float())
            # what is left is the float16 rounding of the OUTPUT (2^-11 relative) and summation order
            err = float((ys.float() - ref).abs().max())
            assert err < 1.2e-3 * max(1.0, float(ref.abs().max())), (k, stride, cin, Bs, err)
            y16 = torch.empty_like(ys)   # against plain float16 weights the pairs must be clearly closer in the mean
            _lib.call("dvsg_conv_gemm_f16", xs.data_ptr(), w32.half().contiguous().data_ptr(), bias.data_ptr(), rs.data_ptr(),
                      y16.data_ptr(), Bs, h, w, cin, cout, k, stride, 1, 1, 0, 0, torch.cuda.current_stream().cuda_stream)
            assert float((ys.float() - ref).abs().mean()) <= float((y16.float() - ref).abs().mean())


@pytest.mark.parametrize("B,H,W", [(2, 70, 100), (1, 33, 47), (3, 64, 96)])
def test_f16_fused_block1_kernel_matches_the_unfused_layers(net, B, H, W):
    """Block 1's conv2 + conv3 (+ the opening unit's shortcut conv) run as one kernel in the float16 mode too
    (conv_fused.hip); against the same layers as separate launches only the rounding sites of the float32 sums move
    (K order of conv2, one fold of hi + lo instead of two)."""
    from coupe.dvsg_amd import _lib
    x = inputs.window_frames(321, B, H, W)
    try:
        _lib.call("dvsg_debug_set_option", b"fuse_conv", 0)
        plain = [net.tap(x, s, precision="f16").cpu().numpy() for s in (2, 3, 4)]
        F_plain = net.forward(x, precision="f16").cpu().numpy()
    finally:
        _lib.call("dvsg_debug_set_option", b"fuse_conv", 1)
    fused = [net.tap(x, s, precision="f16").cpu().numpy() for s in (2, 3, 4)]
    F_fused = net.forward(x, precision="f16").cpu().numpy()
    for name, a, b in zip(("unit_1 (shortcut fused)", "unit_2", "unit_3 (stride 2)"), fused, plain):
        assert a.shape == b.shape
        rel = np.abs(a - b).max() / np.abs(b).max()
        assert rel < 2e-3, "%s: %.3g" % (name, rel)      # float16 activations: 4.9e-4 per rounding
        # (the fused opening unit keeps its shortcut in the float32 accumulators where the separate launch stores it as
        # float16: outputs one float16 ulp apart, on average a third of an ulp -- which the following units inherit)
        assert np.abs(a - b).mean() / np.abs(b).mean() < 1e-3, name
    assert np.abs(F_fused - F_plain).max() < 5e-5     # the bound of either path against the oracle at these sizes
    assert np.array_equal(F_fused, net.forward(x, precision="f16").cpu().numpy())   # deterministic


def test_f16_fused_block1_kernels_agree_at_full_frames(net):
    """conv3x3_1x1_f16h_kernel (block 1's stride-1 units: a kernel row's three taps from one staged run of pixels, the
    weights one stream through a three-slot ring behind COUNTED waits) against conv3x3_1x1_f16_kernel on a 3840x2160
    window, ten runs each unit: the same products in the same order, so bit for bit -- and a wait that lets a tap start on
    weights still in flight shows here (it did: ~10 wrong tiles of 16 000 per run with vmcnt(4) instead of vmcnt(2) at
    tap 7, invisible at the small shapes of the test above)."""
    import torch
    from coupe.dvsg_amd import _lib
    import os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    x = bench.gpu_windows(1, 2160, 3840, 50, torch.device("cuda:0"))
    try:
        for stage in (2, 3):      # the opening unit (shortcut fused), the second unit (residual)
            _lib.call("dvsg_debug_set_option", b"fused_hreuse", 0)
            ref = net.tap(x, stage, precision="f16").clone()
            _lib.call("dvsg_debug_set_option", b"fused_hreuse", 1)
            for rep in range(10):
                got = net.tap(x, stage, precision="f16")
                assert torch.equal(got, ref), "stage %d run %d: %d values differ" % (stage, rep, int((got != ref).sum()))
    finally:
        _lib.call("dvsg_debug_set_option", b"fused_hreuse", 1)


def test_wide_f16_tiles_match_float32_math_and_the_128_tiles():
    """conv_gemm_wide16.hip (256 x 128 tiles, 32-k weight stages from a packed copy, activation rows of 128 or 64 bytes:
    what dvsg_conv_gemm_f16s runs for launches of >= 256 tiles) forced onto small ragged layers -- M not a multiple of 256, stride 2, residual of the output's shape and the
    subsampled `shortcut`, no residual, no ReLU -- against float32 math on the unrounded weights, and against the
    128 x 128 kernel (same products; the K order within a layer differs by the stage depth)."""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    st = torch.cuda.current_stream().cuda_stream
    scratch = torch.empty(160 << 20, dtype=torch.uint8, device=dev)   # tickets + slabs + room for the packed weight copies
    cases = [  # k, stride, cin, cout, B, h, w, residual mode (0 none, 1 same shape, 2 subsampled input-sized), relu
        (3, 1, 64, 64, 3, 21, 29, 1, 1), (3, 2, 128, 128, 2, 23, 31, 0, 1), (1, 1, 256, 128, 5, 9, 13, 1, 0),
        (1, 1, 64, 256, 2, 37, 41, 2, 1), (3, 1, 256, 256, 1, 16, 16, 1, 1), (1, 1, 512, 64, 7, 5, 3, 0, 1),
        # 3x3 stride 1: images narrower than a tile (a tile spans many rows and several images), one-pixel-wide and
        # one-row images, M = 254 k + 1 (a last tile of one pixel), M < one tile
        (3, 1, 64, 64, 5, 7, 5, 1, 1), (3, 1, 128, 64, 3, 9, 1, 0, 1), (3, 1, 64, 128, 2, 1, 300, 0, 0), (3, 1, 64, 64, 1, 15, 17, 0, 1),
        (3, 1, 128, 128, 1, 127, 4, 1, 1), (3, 1, 64, 64, 1, 3, 3, 0, 1), (3, 1, 512, 128, 2, 30, 33, 0, 1)]
    try:
        for k, stride, cin, cout, B, h, w, rmode, relu in cases:
            K = k * k * cin
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            x = (torch.rand((B, h, w, cin), generator=g, device=dev) - 0.3).half()
            w32 = (torch.rand((cout, K), generator=g, device=dev) - 0.5) * (2.0 / K ** 0.5)
            hi = w32.half()
            lo = ((w32 - hi.float()) * 2048.0).half()
            ws = torch.stack([hi.reshape(cout // 64, 64, K), lo.reshape(cout // 64, 64, K)], 1).reshape(2 * cout, K).contiguous()
            bias = torch.rand((cout,), generator=g, device=dev) - 0.5
            res_stride = 1
            if rmode == 1:
                res = (torch.rand((B, ho, wo, cout), generator=g, device=dev) - 0.5).half()
                res_at = res
            elif rmode == 2:   # residual tensor twice the output's size, sampled at every other pixel
                res_stride = 2
                res = (torch.rand((B, 2 * (ho - 1) + 1, 2 * (wo - 1) + 1, cout), generator=g, device=dev) - 0.5).half()
                res_at = res[:, ::2, ::2, :]
            else:
                res, res_at = None, None
            outs = {}
            # wide tiles for everything, with 128-byte activation rows (the default of K >= 256, forced for all) / with 64-byte
            # rows and packed weight stages / with 64-byte rows and the weights from their [rows][K] layout; never wide
            # ... and, first, with a 3x3 stride-1 layer's three taps of a kernel row from one staged run (the default there)
            for key, thr, arows, packed, hreuse in ((1, 1, 2, 1, 1), ("rows128", 1, 2, 1, 0), ("rows64", 1, 0, 1, 0),
                                                    ("unpacked", 1, 0, 0, 0), (1 << 30, 1 << 30, 1, 1, 1)):
                _lib.call("dvsg_debug_set_option", b"wide16_min_tiles", thr)
                _lib.call("dvsg_debug_set_option", b"wide16_arows", arows)
                _lib.call("dvsg_debug_set_option", b"wide16_packed", packed)
                _lib.call("dvsg_debug_set_option", b"wide16_hreuse", hreuse)
                y = torch.full((B, ho, wo, cout), float("nan"), device=dev, dtype=torch.float16)
                _lib.call("dvsg_conv_gemm_f16s", x.data_ptr(), ws.data_ptr(), bias.data_ptr(), res.data_ptr() if res is not None else 0,
                          y.data_ptr(), B, h, w, cin, cout, k, stride, relu, res_stride, scratch.data_ptr(), scratch.numel(), st)
                outs[key] = y.float()
            w4 = w32.reshape(cout, k, k, cin).permute(0, 3, 1, 2)
            ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w4, bias, stride=stride, padding=k // 2).permute(0, 2, 3, 1)
            if res_at is not None:
                ref = ref + res_at.float()
            if relu:
                ref = torch.relu(ref)
            scale = max(1.0, float(ref.abs().max()))
            case = (k, stride, cin, cout, B, h, w, rmode, relu)
            assert bool(torch.isfinite(outs[1]).all()), case
            assert float((outs[1] - ref).abs().max()) < 1.2e-3 * scale, case          # float16 rounding of the output
            assert float((outs[1] - outs[1 << 30]).abs().max()) < 1.0e-3 * scale, case   # one float16 ulp of the output
            assert float((outs[1] - outs[1 << 30]).abs().mean()) < 2e-5 * scale, case
            # packing moves bytes, not sums: the same bits; the 128-byte-row kernel visits a 3x3 layer's K in another order
            assert torch.equal(outs["rows64"], outs["unpacked"]), case
            assert float((outs["rows64"] - ref).abs().max()) < 1.2e-3 * scale, case
            assert float((outs["rows128"] - ref).abs().max()) < 1.2e-3 * scale, case
            if k == 1:
                assert torch.equal(outs[1], outs["rows64"]) and torch.equal(outs["rows128"], outs["rows64"]), case
            else:
                assert float((outs[1] - outs["rows64"]).abs().max()) < 1.0e-3 * scale, case
                assert float((outs["rows128"] - outs["rows64"]).abs().max()) < 1.0e-3 * scale, case
    finally:
        _lib.call("dvsg_debug_set_option", b"wide16_min_tiles", 128)
        _lib.call("dvsg_debug_set_option", b"wide16_arows", 1)
        _lib.call("dvsg_debug_set_option", b"wide16_packed", 1)
        _lib.call("dvsg_debug_set_option", b"wide16_hreuse", 1)


def test_calibrated_float16_mode(synthetic_weights):
    """dvsg_locnet_calibrate_f16: plain float16 weights in blocks 2-4, re-rounded with error feedback against the mean
    activation of their input channels (measured on OTHER frames than the ones tested: two 288x512 windows).  F_t at 720p
    against a float64 CPU evaluation of the graph: < 3e-6 (measured 2.0-2.6e-6; hi / lo pairs everywhere 1.4-1.9e-6,
    round-to-nearest plain weights 1.9e-5), the pixel tolerance of BASELINE.json still met, deterministic across two
    calibrations, and undone by calibrate_f16(None)."""
    import torch
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    from oracle import model as omodel
    from oracle.cnn_torch import TorchLocNet
    from oracle.thin_plate_spline import ThinPlateSpline as ostn
    from oracle.thin_plate_spline import border_discontinuity_mask
    H, W = 720, 1280
    net = LocNet(synthetic_weights)
    oracle = TorchLocNet(synthetic_weights, dtype=torch.float64)
    calib = inputs.window_frames(991, 2, 288, 512)
    tests = [inputs.window_frames(seed, 1, H, W) for seed in (7, 77)]
    refs = [oracle.forward(x) for x in tests]
    xs = [torch.from_numpy(x).cuda() for x in tests]
    paired = [net.forward(x, precision="f16") for x in xs]
    e_pairs = max(np.abs(F.cpu().numpy() - r).max() for F, r in zip(paired, refs))
    net.calibrate_f16(calib)
    cal = [net.forward(x, precision="f16") for x in xs]
    e_cal = max(np.abs(F.cpu().numpy() - r).max() for F, r in zip(cal, refs))
    # what the calibration replaces: the same layers on round-to-nearest plain weights
    ws, nbytes = net.workspace(2, 288, 512)
    cd = torch.from_numpy(calib).cuda()
    _lib.call("dvsg_debug_calibrate_f16_weights", net.handle, cd.data_ptr(), 2, 288, 512, 0, ws.data_ptr(), nbytes,
              torch.cuda.current_stream().cuda_stream)
    e_rtn = max(np.abs(net.forward(x, precision="f16").cpu().numpy() - r).max() for x, r in zip(xs, refs))
    net.calibrate_f16(calib)
    again = [net.forward(x, precision="f16") for x in xs]
    print("float16 mode F_t error at 720p vs float64: pairs %.2e, calibrated plain (blocks 2-4) %.2e, round-to-nearest plain %.2e"
          % (e_pairs, e_cal, e_rtn))
    assert e_pairs < 2.5e-6 and e_cal < 3e-6 and e_rtn > 3 * e_cal
    assert all(torch.equal(a, b) for a, b in zip(cal, again))                 # the calibration itself is deterministic
    # end to end in pixels (one window): the warp on the calibrated F_t against the float64 F_t's frame
    x = tests[0]
    out = torch.empty((1, H, W, 3), device="cuda")
    F = torch.empty((1, 25, 2), device="cuda")
    net.stabilize(xs[0], xs[0][..., 18:].contiguous(), out, F, precision="f16")
    rpred, rx, ry = ostn(x[..., 18:], np.tile(omodel.v_src()[None], (1, 1, 1)), refs[0].astype(np.float32), (H, W))
    border = border_discontinuity_mask(rx, ry, H, W, delta=3e-2).reshape(1, H, W)
    perr = np.abs(out.cpu().numpy() - rpred).max(axis=3)[~border].max()
    assert perr < 1e-3, perr
    net.calibrate_f16(None)
    assert all(torch.equal(net.forward(x, precision="f16"), p) for x, p in zip(xs, paired))   # undone: the paired mode's bits
    # the float32 path never sees any of it
    assert np.abs(net.forward(xs[0], precision="f32").cpu().numpy() - refs[0]).max() <= 1e-5


def test_calibration_leaves_the_options_alone(synthetic_weights):
    """dvsg_locnet_calibrate_f16 leaves the "fuse_conv" switch as it found it: after a calibration the float32 opening unit of block 1 (tap stage 2: the call returns after that unit) ends in
    conv3x3_1x1_kernel (family 4 of dvsg_debug_last_conv_kernel) with the option at 1, in conv_gemm_kernel (0) with it at 0.
    40 x 72 frames: a pooled map of 10 x 18, every unit runs, blocks 3-4 on maps of a few pixels."""
    import ctypes
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    net = LocNet(synthetic_weights)
    x = inputs.window_frames(41, 1, 40, 72)
    fields = (ctypes.c_int * 6)()
    try:
        for fuse, family in ((1, 4), (0, 0)):
            _lib.call("dvsg_debug_set_option", b"fuse_conv", fuse)
            net.calibrate_f16(x)
            net.tap(x, 2, precision="f32")
            _lib.call("dvsg_debug_last_conv_kernel", fields, 6)
            assert fields[0] == family, "fuse_conv %d: block 1's opening unit ended in kernel family %d" % (fuse, fields[0])
    finally:
        _lib.call("dvsg_debug_set_option", b"fuse_conv", 1)
        net.calibrate_f16(None)


def test_plain_float16_layers_on_the_wide_tiles():
    """A layer WITHOUT the lo piece (`dvsg_conv_gemm_f16`; in the network: `f16_split=0` or a layer cleared in
    `f16_pair_mask`) with Cout % 128 == 0 and Cin % 64 == 0 runs, from `wide16_min_tiles` tiles on, in the SPLIT = false
    instantiations of conv_gemm_wide16.hip -- `acc_lo` holds channels 64..127 of a 128-channel tile and the epilogue
    runs both halves.  Forced onto small ragged layers: against float32 math on the float16-rounded weights, and against
    the 128 x 128 kernel (`conv_variant=5`), residual modes 0 / 1 / 2, with and without ReLU."""
    import torch
    from coupe.dvsg_amd import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(15)
    st = torch.cuda.current_stream().cuda_stream
    scratch = torch.empty(160 << 20, dtype=torch.uint8, device=dev)   # tickets + slabs + room for the packed weight copies
    cases = [  # k, stride, cin, cout, B, h, w, residual mode (0 none, 1 same shape, 2 subsampled input-sized), relu
        (3, 2, 128, 128, 2, 23, 31, 0, 1), (1, 1, 256, 128, 5, 9, 13, 1, 0), (1, 1, 64, 256, 2, 37, 41, 2, 1),
        (3, 1, 256, 256, 1, 16, 16, 1, 1), (3, 1, 64, 128, 2, 1, 300, 0, 0), (3, 1, 128, 128, 1, 127, 4, 1, 1),
        (3, 1, 512, 128, 2, 30, 33, 0, 1), (1, 1, 128, 512, 3, 17, 19, 1, 1), (1, 1, 512, 128, 1, 1, 1, 0, 0),
        (1, 2, 256, 512, 2, 21, 23, 0, 0), (3, 1, 64, 128, 5, 7, 5, 2, 1)]
    try:
        for k, stride, cin, cout, B, h, w, rmode, relu in cases:
            K = k * k * cin
            ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
            x = (torch.rand((B, h, w, cin), generator=g, device=dev) - 0.3).half()
            w16 = ((torch.rand((cout, K), generator=g, device=dev) - 0.5) * (2.0 / K ** 0.5)).half()
            bias = torch.rand((cout,), generator=g, device=dev) - 0.5
            res_stride = 1
            if rmode == 1:
                res = (torch.rand((B, ho, wo, cout), generator=g, device=dev) - 0.5).half()
                res_at = res
            elif rmode == 2:
                res_stride = 2
                res = (torch.rand((B, 2 * (ho - 1) + 1, 2 * (wo - 1) + 1, cout), generator=g, device=dev) - 0.5).half()
                res_at = res[:, ::2, ::2, :]
            else:
                res, res_at = None, None
            outs = {}
            # plain weights from their [Cout][K] layout (no scratch), from the stage-packed copies the network keeps (scratch
            # given: 128-byte activation rows / a 3x3 kernel row's taps from one staged run where they apply, forced for
            # every K with arows = 2), and on the 128 x 128 kernel
            for key, variant, thr, arows, scr in (("wide", 0, 1, 1, 0), ("wide_rows64", 0, 1, 0, 0), ("packed", 0, 1, 2, 1),
                                                  ("packed_rows64", 0, 1, 0, 1), ("t128", 5, 128, 1, 0)):
                _lib.call("dvsg_debug_set_option", b"conv_variant", variant)
                _lib.call("dvsg_debug_set_option", b"wide16_min_tiles", thr)
                _lib.call("dvsg_debug_set_option", b"wide16_arows", arows)
                y = torch.full((B, ho, wo, cout), float("nan"), device=dev, dtype=torch.float16)
                _lib.call("dvsg_conv_gemm_f16", x.data_ptr(), w16.data_ptr(), bias.data_ptr(), res.data_ptr() if res is not None else 0,
                          y.data_ptr(), B, h, w, cin, cout, k, stride, relu, res_stride, scratch.data_ptr() if scr else 0,
                          scratch.numel() if scr else 0, st)
                outs[key] = y.float()
            w4 = w16.float().reshape(cout, k, k, cin).permute(0, 3, 1, 2)
            ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w4, bias, stride=stride, padding=k // 2).permute(0, 2, 3, 1)
            if res_at is not None:
                ref = ref + res_at.float()
            if relu:
                ref = torch.relu(ref)
            scale = max(1.0, float(ref.abs().max()))
            case = (k, stride, cin, cout, B, h, w, rmode, relu)
            if k == 1 or stride == 2:    # packing moves bytes, not sums (a 3x3 stride-1 layer with packed copies takes the kernel
                assert torch.equal(outs["packed_rows64"], outs["wide_rows64"]), case   # that visits K in another order)
            else:
                assert float((outs["packed_rows64"] - outs["wide_rows64"]).abs().max()) < 1.0e-3 * scale, case
            for key in ("wide", "wide_rows64", "packed", "packed_rows64", "t128"):
                assert bool(torch.isfinite(outs[key]).all()), (key, case)
                assert float((outs[key] - ref).abs().max()) < 1.2e-3 * scale, (key, case)     # float16 rounding of the output
            assert float((outs["wide"] - outs["t128"]).abs().max()) < 1.0e-3 * scale, case   # one float16 ulp of the output
            assert float((outs["wide"] - outs["t128"]).abs().mean()) < 2e-5 * scale, case
            assert float((outs["wide_rows64"] - outs["t128"]).abs().mean()) < 2e-5 * scale, case
    finally:
        _lib.call("dvsg_debug_set_option", b"conv_variant", 0)
        _lib.call("dvsg_debug_set_option", b"wide16_min_tiles", 128)
        _lib.call("dvsg_debug_set_option", b"wide16_arows", 1)


def test_f16_pair_mask_through_the_wide_plain_tiles(net, synthetic_weights):
    """A non-trivial `f16_pair_mask`: blocks 2-4 without the lo piece (0x1111 keeps block 1's four layer kinds), their
    layers forced onto the wide plain-weight tiles.  F_t stays bounded against the oracle -- a broken SPLIT = false kernel
    gives errors of O(|F|) -- and agrees with the same mask on the 128 x 128 kernels to float32 re-association + one
    float16 rounding per activation."""
    import torch
    from coupe.dvsg_amd import _lib
    x = inputs.window_frames(331, 2, 96, 160)
    F_ref = onet.localizationNet(x, 25, synthetic_weights)
    xt = torch.from_numpy(x).cuda()
    F = {}
    try:
        _lib.call("dvsg_debug_set_option", b"f16_pair_mask", 0x1111)
        for key, variant, thr in (("wide", 0, 1), ("t128", 5, 128)):
            _lib.call("dvsg_debug_set_option", b"conv_variant", variant)
            _lib.call("dvsg_debug_set_option", b"wide16_min_tiles", thr)
            F[key] = net.forward(xt, precision="f16").cpu().numpy()
    finally:
        _lib.call("dvsg_debug_set_option", b"f16_pair_mask", 0xFFFF)
        _lib.call("dvsg_debug_set_option", b"conv_variant", 0)
        _lib.call("dvsg_debug_set_option", b"wide16_min_tiles", 128)
    full = net.forward(xt, precision="f16").cpu().numpy()
    e_wide, e_128, e_full = (np.abs(v - F_ref).max() for v in (F["wide"], F["t128"], full))
    print("f16_pair_mask 0x1111: F_t error wide plain tiles %.3g, 128x128 kernels %.3g, all pairs %.3g (|F| %.3g)"
          % (e_wide, e_128, e_full, np.abs(F_ref).max()))
    assert e_full < 5e-5
    assert e_wide < 5e-4 and e_128 < 5e-4          # plain float16 weights cost ~10x the pairs' error, not more
    assert np.abs(F["wide"] - F["t128"]).max() < 1e-4


@pytest.mark.parametrize("source", ["window", "ring_f32", "ring_u8"])
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 70, 100), (3, 33, 47), (1, 8, 8), (1, 1, 1), (2, 30, 600), (1, 100, 301)])
def test_conv1_f16_kernels_agree(net, source, B, H, W):
    """The three float16 conv1 kernels -- one output row per workgroup (conv1_variant 3), two rows with the kernel rows
    visited as two chains (4 = the default of small launches), and the marching, wave-specialised kernel of the big
    launches (5 forces it here: bands of three quads, so a frame is cut into several bands and the last quad / band is
    ragged) -- multiply the same float16 operands and accumulate in float32; the kernel-row order differs between the
    first and the other two (0..6 against 0, 2, 4, 6, 1, 3, 5), so those agree to float32 re-association -- one float16
    ulp of the output -- and the last two, which add the same products in the same order, bit for bit."""
    import torch
    from coupe.dvsg_amd import _lib
    rng = np.random.default_rng(H * 1000 + W)
    if source == "window":
        x = torch.from_numpy(inputs.window_frames(77, B, H, W)).cuda()
        run = lambda: net.tap(x, 0, precision="f16")
    else:
        n = 9
        pool = (rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8) if source == "ring_u8"
                else rng.uniform(0, 1, (n, H, W, 3)).astype(np.float32))
        pool = torch.from_numpy(pool).cuda()
        table = torch.from_numpy(rng.integers(0, n, (B, 7)).astype(np.int32)).cuda()
        run = lambda: net.forward_ring(pool, table, precision="f16", stage=0)
    outs = {}
    try:
        for v in (3, 4, 5):
            _lib.call("dvsg_debug_set_option", b"conv1_variant", v)
            outs[v] = run().clone()
    finally:
        _lib.call("dvsg_debug_set_option", b"conv1_variant", 0)
    assert torch.equal(outs[4], outs[5]), "pair vs marching kernel: max diff %g" % float((outs[4] - outs[5]).abs().max())
    ref = outs[3]
    # one float16 ulp of the value, plus the float32 re-association noise of a 1029-term sum that cancels to ~0 in front
    # of the ReLU (absolute: relative to the tensor's scale, not to the value)
    tol = 2.0 ** -10 * ref.abs() + 1e-5 * float(ref.abs().max())
    bad = (outs[4] - ref).abs() > tol
    assert not bool(bad.any()), "%d values off, worst %g" % (int(bad.sum()), float(((outs[4] - ref).abs() - tol).max()))
