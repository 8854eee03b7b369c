#!/usr/bin/env python3
"""Cost of rendering at a delivery size (include/dvsg_amd.h, "Output size") against what a user had before it, on the same
build: NV12, 1080p -> 720p, 4K -> 1080p and 4K -> 720p, both filters, n = 1.

scaled:  dvsg_tps_render_zoom_nv12 through LocNet.view(out_size=...): ONE launch (behind the T launch), sy x sx map and
         filter evaluations per output sample, 1 / (sx sy) of the bytes stored.
route:   the route before it: dvsg_tps_render_zoom_nv12 at source size, then a device resize of both planes
         (torch.nn.functional.interpolate(mode="area") on float copies, rounded back to bytes).
source:  the source-size render of that route alone.
The three ALTERNATE inside every round; device events around `--reps` calls; `--rounds` rounds; median and spread
(min .. max) per call.  One JSON line per measurement; the expectation under test is "scaled is not slower than source
beyond the spread".

    python tools/scaled_bench.py [--reps 20] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = (("1080p->720p", (1080, 1920), (720, 1280)), ("4K->1080p", (2160, 3840), (1080, 1920)),
         ("4K->720p", (2160, 3840), (720, 1280)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as Fn
    import inputs
    import nv12_ref
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet, scaled_factors
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("scaled_bench needs the GPU")
    net = LocNet(make_synthetic_weights(seed=0))
    s = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for name, (H, W), (oh, ow) in CASES:
        src = torch.from_numpy(nv12_ref.smooth_batch(7, 1, H, W).buf).cuda()
        F = torch.from_numpy(inputs.control_vectors(11, 1)).cuda()
        zoom = torch.full((1,), 0.9, device="cuda")
        T = torch.empty((1, 2, 28), device="cuda")
        full = torch.empty_like(src)
        small = torch.empty((1, 3 * oh // 2, ow), dtype=torch.uint8, device="cuda")
        resized = torch.empty_like(small)
        for filt in ("bilinear", "bicubic"):
            plain, view = net.view(filt), net.view(filt, out_size=(oh, ow))

            def render(handle, out, h, w):
                _lib.call("dvsg_tps_render_zoom_nv12", handle, F.data_ptr(), src.data_ptr(), src.data_ptr() + H * W, W,
                          3 * H // 2 * W, 1, H, W, zoom.data_ptr(), T.data_ptr(), out.data_ptr(), out.data_ptr() + h * w, w,
                          3 * h // 2 * w, s())

            def scaled():
                render(view, small, oh, ow)

            def source():
                render(plain, full, H, W)

            def route():
                source()
                y = Fn.interpolate(full[:, :H].unsqueeze(1).float(), size=(oh, ow), mode="area")
                resized[:, :oh] = (y + 0.5).clamp_(0, 255).to(torch.uint8)[:, 0]
                uv = full[:, H:].view(1, H // 2, W // 2, 2).permute(0, 3, 1, 2).float()
                c = Fn.interpolate(uv, size=(oh // 2, ow // 2), mode="area")
                resized[:, oh:] = (c + 0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).reshape(1, oh // 2, ow)

            fns = (("scaled", scaled), ("route", route), ("source", source))
            for _, fn in fns:
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k, _ in fns}
            for _ in range(args.rounds):
                for k, fn in fns:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    ms[k].append(a.elapsed_time(b) / args.reps)
            # the two results show the same picture: the mean absolute luma difference, in bytes
            diff = float((small[:, :oh].float() - resized[:, :oh].float()).abs().mean())
            sy, sx = scaled_factors((H, W), (oh, ow))
            rec = dict(case=name, filter=filt, factors=[sy, sx], reps=args.reps, rounds=args.rounds,
                       luma_mean_abs_diff_scaled_vs_route=round(diff, 3))
            for k in ms:
                v = np.array(ms[k])
                rec[k + "_ms"] = dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4),
                                      max=round(float(v.max()), 4))
            rec["scaled_over_source"] = round(rec["scaled_ms"]["median"] / rec["source_ms"]["median"], 3)
            rec["scaled_over_route"] = round(rec["scaled_ms"]["median"] / rec["route_ms"]["median"], 3)
            emit(rec)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
