#!/usr/bin/env python3
"""Cost of the crop's two device pieces at a size a user would run: 64 frames of 1920 x 1080.

scan:    dvsg_tps_coverage_net_f32 (T, map, predicate and reduction fused; x_s / y_s never written)  vs  the composition
         available without it: dvsg_tps_warp_f32 grid-only (x_s, y_s written: 8 B per pixel) + the predicate and the two
         reductions in torch.  The two are checked to give the same integers before anything is timed.
render:  dvsg_tps_render_zoom_u8  vs  dvsg_tps_render_u8 (uint8 source -> uint8 output), the same F_t.
The versions of a pair ALTERNATE inside every round; device events around `--reps` calls; 7 rounds, median and spread
(min .. max) per call.  One JSON line per measurement.

    python tools/crop_bench.py [--frames 64] [--height 1080] [--width 1920] [--reps 5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.model import V_SRC
    from coupe.dvsg_amd.networks import LocNet
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("crop_bench needs the GPU")
    n, H, W = args.frames, args.height, args.width
    net = LocNet(make_synthetic_weights(seed=0))
    s = lambda: torch.cuda.current_stream().cuda_stream
    F = torch.from_numpy(inputs.control_vectors(3, n, scale=0.03)).cuda()
    src = torch.from_numpy((inputs.smooth_frames(2, 1, H, W, factor=32) * 255).astype(np.uint8)).cuda().repeat(n, 1, 1, 1).contiguous()
    zoom = torch.full((n,), 0.9, device="cuda")
    T = torch.empty((n, 2, 28), device="cuda")
    V = torch.from_numpy(np.ascontiguousarray(np.tile(V_SRC[None], (n, 1, 1)))).cuda()
    res = torch.empty((2, n), dtype=torch.int32, device="cuda")
    need = ctypes.c_size_t()
    _lib.call("dvsg_tps_coverage_workspace_bytes", n, H, W, ctypes.byref(need))
    ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device="cuda")
    xs, ys = torch.empty((n, H, W), device="cuda"), torch.empty((n, H, W), device="cuda")
    out8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    i = torch.arange(H, device="cuda").view(1, H, 1)
    j = torch.arange(W, device="cuda").view(1, 1, W)
    key = torch.maximum((2 * j - (W - 1)).abs() * (H - 1), (2 * i - (H - 1)).abs() * (W - 1)).to(torch.int32)
    big = torch.tensor(2 ** 31 - 1, dtype=torch.int32, device="cuda")

    def fused():
        _lib.call("dvsg_tps_coverage_net_f32", net.handle, F.data_ptr(), None, n, H, W, H, W, T.data_ptr(), res[0].data_ptr(),
                  res[1].data_ptr(), ws.data_ptr(), ws.numel() * 8, s())
        return res

    def composed():
        _lib.call("dvsg_tps_warp_f32", None, V.data_ptr(), T.data_ptr(), n, 1, 1, 1, 25, H, W, None, xs.data_ptr(), ys.data_ptr(), s())
        x = ((xs + 1.0) * float(W)) / 2.0
        y = ((ys + 1.0) * float(H)) / 2.0
        bad = ~((x >= 0) & (x < W - 1) & (y >= 0) & (y < H - 1))
        return torch.stack([bad.sum((1, 2)).to(torch.int32), torch.where(bad, key, big).amin((1, 2))])

    def render_plain():
        _lib.call("dvsg_tps_render_u8", net.handle, F.data_ptr(), src.data_ptr(), n, H, W, 0, T.data_ptr(), None, out8.data_ptr(), W, 0, s())

    def render_zoom():
        _lib.call("dvsg_tps_render_zoom_u8", net.handle, F.data_ptr(), src.data_ptr(), n, H, W, 0, zoom.data_ptr(), T.data_ptr(), None,
                  out8.data_ptr(), W, 0, s())

    a, b = fused().clone(), composed()
    torch.cuda.synchronize()
    if not torch.equal(a, b):
        raise SystemExit("fused scan and composition disagree: %s vs %s" % (a[:, :4].tolist(), b[:, :4].tolist()))
    lines = []

    def pair(name_a, fa, name_b, fb, what):
        for f in (fa, fb, fa, fb):
            f()
        torch.cuda.synchronize()
        per = {name_a: [], name_b: []}
        for _ in range(7):
            for name, f in ((name_a, fa), (name_b, fb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                per[name].append(e0.elapsed_time(e1) / args.reps)
        for name in (name_a, name_b):
            v = sorted(per[name])
            rec = dict(what=what, version=name, frames=n, height=H, width=W, ms_median=round(v[3], 4), ms_min=round(v[0], 4),
                       ms_max=round(v[-1], 4), us_per_frame=round(1e3 * v[3] / n, 2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)

    pair("fused dvsg_tps_coverage_net_f32", fused, "dvsg_tps_warp_f32 grid-only + torch", composed, "scan")
    pair("dvsg_tps_render_u8", render_plain, "dvsg_tps_render_zoom_u8", render_zoom, "render u8->u8")
    pair("fused dvsg_tps_coverage_net_f32", fused, "dvsg_tps_render_u8", render_plain, "scan vs one render")
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
