#!/usr/bin/env python3
"""Cost of the fused test-time losses (dvsg_loss_image_f32, dvsg_loss_temporal_f32) against the composition of the entry
points that existed before them, at B=16 720p and B=16 512x288.

image:    fused (prediction and mask plane NOT written)  vs  dvsg_tps_warp_f32 on u and on ones + torch reductions
temporal: fused                                          vs  dvsg_flow_warp_f32 on the frame and on the three-channel mask
                                                             + torch product and reductions
Device events around `--reps` repetitions of each, median of 5 rounds.  Algorithmic bytes per pixel: image 24, temporal 40
(pred 12 + mask 4 + flow 8 + gt 12 + mask_gt 4).  One JSON line per measurement.

    python tools/loss_bench.py [--reps 10] [--shapes 16x720x1280,16x288x512] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="16x720x1280,16x288x512")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.reps < 1:
        raise SystemExit("--reps must be >= 1")
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd import _lib, trainer
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs the GPU")
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def s():
        return torch.cuda.current_stream().cuda_stream

    def timed(fn):
        """median over 5 rounds of the device time of args.reps calls of fn, per call (ms)"""
        fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            per.append(a.elapsed_time(b) / args.reps)
        return sorted(per)[2]

    def masked_mse_torch(pred, gt, mask):   # trainer.py:233-243 in eager torch, as a user composes it today
        d = pred * mask - gt * mask
        return torch.mean(torch.nan_to_num((d * d).sum(dim=(1, 2, 3)) / mask.sum(dim=(1, 2, 3)), nan=0.0, posinf=0.0))

    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        one = inputs.smooth_frames(1, 2, H, W)
        u = torch.from_numpy(one[:1]).cuda().expand(B, -1, -1, -1).contiguous()
        gt = torch.from_numpy(one[1:]).cuda().expand(B, -1, -1, -1).contiguous()
        flow = torch.from_numpy(inputs.smooth_flow(2, 1, H, W)).cuda().expand(B, -1, -1, -1).contiguous()
        V = torch.from_numpy(inputs.v_src(B)).cuda()
        F = torch.from_numpy(inputs.control_vectors(3, B)).cuda()
        c, T = trainer.solve_T(V, F)
        ones = torch.ones_like(u)
        pred, mask3 = torch.empty_like(u), torch.empty_like(u)
        warp_p, warp_m = torch.empty_like(u), torch.empty_like(u)
        ps, mean = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
        ws = trainer._workspace(B, H, W, u)
        px = float(B * H * W)

        def image_fused():
            _lib.call("dvsg_loss_image_f32", u.data_ptr(), c.data_ptr(), T.data_ptr(), gt.data_ptr(), B, H, W, 25, 0, 0,
                      ps.data_ptr(), mean.data_ptr(), 0, ws.data_ptr(), ws.numel() * 8, s())

        def image_composed():
            _lib.call("dvsg_tps_warp_f32", u.data_ptr(), c.data_ptr(), T.data_ptr(), B, H, W, 3, 25, H, W, pred.data_ptr(), 0, 0, s())
            _lib.call("dvsg_tps_warp_f32", ones.data_ptr(), c.data_ptr(), T.data_ptr(), B, H, W, 3, 25, H, W, mask3.data_ptr(), 0, 0,
                      s())
            return masked_mse_torch(pred, gt, mask3)
        plane = torch.empty((B, H, W), device="cuda")

        def image_fused_out():   # with pred and the mask plane written (24 + 16 B/px): what build_loss_train runs for `temporal`
            _lib.call("dvsg_loss_image_f32", u.data_ptr(), c.data_ptr(), T.data_ptr(), gt.data_ptr(), B, H, W, 25, pred.data_ptr(),
                      plane.data_ptr(), ps.data_ptr(), mean.data_ptr(), 0, ws.data_ptr(), ws.numel() * 8, s())

        def image_warps():       # the two warp launches of the composition alone, no reduction
            _lib.call("dvsg_tps_warp_f32", u.data_ptr(), c.data_ptr(), T.data_ptr(), B, H, W, 3, 25, H, W, pred.data_ptr(), 0, 0, s())
            _lib.call("dvsg_tps_warp_f32", ones.data_ptr(), c.data_ptr(), T.data_ptr(), B, H, W, 3, 25, H, W, mask3.data_ptr(), 0, 0,
                      s())
        t_f, t_o, t_c, t_w = timed(image_fused), timed(image_fused_out), timed(image_composed), timed(image_warps)
        emit({"what": "image", "B": B, "H": H, "W": W, "fused_us": 1e3 * t_f, "fused_with_outputs_us": 1e3 * t_o,
              "composed_us": 1e3 * t_c, "composed_warps_only_us": 1e3 * t_w, "speedup": t_c / t_f,
              "speedup_with_outputs": t_c / t_o, "fused_alg_TBps": 24.0 * px / (t_f * 1e-3) / 1e12,
              "fused_with_outputs_alg_TBps": 40.0 * px / (t_o * 1e-3) / 1e12})
        image_composed()
        mask_plane = mask3[..., 0].contiguous()

        def temporal_fused():
            _lib.call("dvsg_loss_temporal_f32", pred.data_ptr(), mask_plane.data_ptr(), flow.data_ptr(), gt.data_ptr(),
                      mask_plane.data_ptr(), B, H, W, ps.data_ptr(), mean.data_ptr(), 0, ws.data_ptr(), ws.numel() * 8, s())

        def temporal_composed():
            _lib.call("dvsg_flow_warp_f32", pred.data_ptr(), flow.data_ptr(), B, H, W, 3, warp_p.data_ptr(), s())
            _lib.call("dvsg_flow_warp_f32", mask3.data_ptr(), flow.data_ptr(), B, H, W, 3, warp_m.data_ptr(), s())
            return masked_mse_torch(warp_p, gt, warp_m * mask3)

        def temporal_warps():
            _lib.call("dvsg_flow_warp_f32", pred.data_ptr(), flow.data_ptr(), B, H, W, 3, warp_p.data_ptr(), s())
            _lib.call("dvsg_flow_warp_f32", mask3.data_ptr(), flow.data_ptr(), B, H, W, 3, warp_m.data_ptr(), s())
        t_f, t_c, t_w = timed(temporal_fused), timed(temporal_composed), timed(temporal_warps)
        emit({"what": "temporal", "B": B, "H": H, "W": W, "fused_us": 1e3 * t_f, "composed_us": 1e3 * t_c,
              "composed_warps_only_us": 1e3 * t_w, "speedup": t_c / t_f,
              "fused_alg_TBps": 40.0 * px / (t_f * 1e-3) / 1e12, "hbm_peak_TBps": 8.0})
        del u, gt, flow, ones, pred, mask3, warp_p, warp_m
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
