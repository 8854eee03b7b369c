#!/usr/bin/env python3
"""Cost of the NV12 path against the RGB route an NV12 user had before it, on the same build: 1080p and 4K, n = 1 and 16.

ingest:  dvsg_frames_ingest_nv12 (convert + resize fused, into the 512 x 288 pool)
         vs  dvsg_frames_nv12_to_rgb_u8 (source-size RGB written) + dvsg_frames_ingest_u8.
render:  dvsg_tps_render_nv12 (NV12 in, NV12 out; the T launch and ONE launch for both planes)
         vs  dvsg_tps_render_u8 on the RGB frame the route above wrote (uint8 RGB out; an encoder would still need NV12,
         which that route does not produce -- its cost is NOT in the RGB figure).
route:   ingest + render of each side: what one online step adds around the stabilise call.
The fused ingest is checked bit for bit against the two-launch route before anything is timed.  The versions of a pair
ALTERNATE inside every round; device events around `--reps` calls; 7 rounds; median and spread (min .. max) per call.
One JSON line per measurement.

--render-filter bicubic renders through a bicubic view of the network (both renders; every record names the filter).

--border NAME renders through a view with that border mode instead (every record names it); --border all keeps the pairs
above on "black" and adds, per size and n, both renders through a view of EVERY border mode, alternating inside every
round, and the copy that OnlineStabilizer(border="keep") adds per frame (a clone of the stream's output surface).

--strength S, --rigidity R, --shape-model NAME render through a SHAPED view (include/dvsg_amd.h, "Warp shaping": one kernel
in the place of the one that forms T, no launch added); every record names the three values.

    python tools/nv12_bench.py [--reps 20] [--render-filter bilinear|bicubic] [--border black|replicate|mirror|keep|all]
                               [--strength S] [--rigidity R] [--shape-model affine|similarity|translation] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model-height", type=int, default=288)
    ap.add_argument("--model-width", type=int, default=512)
    ap.add_argument("--render-filter", default="bilinear", choices=["bilinear", "bicubic"])
    ap.add_argument("--border", default="black", choices=["black", "replicate", "mirror", "keep", "all"])
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--rigidity", type=float, default=0.0)
    ap.add_argument("--shape-model", default="affine", choices=["affine", "similarity", "translation"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import inputs
    import nv12_ref
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import RENDER_BORDERS, LocNet
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("nv12_bench needs the GPU")
    net = LocNet(make_synthetic_weights(seed=0))
    border = "black" if args.border == "all" else args.border
    shape = (args.strength, args.rigidity, args.shape_model)
    handle = net.view(args.render_filter, border, *shape)
    s = lambda: torch.cuda.current_stream().cuda_stream
    h, w, M = args.model_height, args.model_width, 1   # BT.709
    lines = []

    def pair(what, n, H, W, versions):
        for _ in range(3):
            for _, f in versions:
                f()
        torch.cuda.synchronize()
        per = {name: [] for name, _ in versions}
        for _ in range(7):
            for name, f in versions:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                per[name].append(e0.elapsed_time(e1) / args.reps)
        for name, _ in versions:
            v = sorted(per[name])
            rec = dict(what=what, version=name, render_filter=args.render_filter, border=name if name in RENDER_BORDERS else border,
                       strength=args.strength, rigidity=args.rigidity, shape_model=args.shape_model, frames=n, height=H, width=W, ms_median=round(v[3], 4), ms_min=round(v[0], 4),
                       ms_max=round(v[-1], 4), us_per_frame=round(1e3 * v[3] / n, 2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)

    for H, W in ((1080, 1920), (2160, 3840)):
        one = torch.from_numpy(nv12_ref.smooth_batch(2, 1, H, W).buf).cuda()
        for n in (1, 16):
            src = one.repeat(n, 1, 1).contiguous()                       # packed [n, 3H/2, W]
            y, uv, fs = src.data_ptr(), src.data_ptr() + H * W, 3 * H // 2 * W
            out = torch.empty_like(src)
            rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
            out8 = torch.empty_like(rgb)
            pool = torch.zeros((n, h, w, 3), device="cuda")
            pool2 = torch.zeros_like(pool)
            slots = torch.arange(n, dtype=torch.int32, device="cuda")
            F = torch.from_numpy(inputs.control_vectors(3, n, scale=0.03)).cuda()
            T = torch.empty((n, 2, 28), device="cuda")

            def ingest_nv12():
                _lib.call("dvsg_frames_ingest_nv12", y, uv, W, fs, n, H, W, M, pool.data_ptr(), n, slots.data_ptr(), h, w, s())

            def ingest_rgb():
                _lib.call("dvsg_frames_nv12_to_rgb_u8", y, uv, W, fs, n, H, W, M, 0, rgb.data_ptr(), s())
                _lib.call("dvsg_frames_ingest_u8", rgb.data_ptr(), n, H, W, 0, pool2.data_ptr(), n, slots.data_ptr(), h, w, None,
                          0, 0, s())

            def render_nv12():
                _lib.call("dvsg_tps_render_nv12", handle, F.data_ptr(), y, uv, W, fs, n, H, W, T.data_ptr(), out.data_ptr(),
                          out.data_ptr() + H * W, W, fs, s())

            def render_rgb():
                _lib.call("dvsg_tps_render_u8", handle, F.data_ptr(), rgb.data_ptr(), n, H, W, 0, T.data_ptr(), None,
                          out8.data_ptr(), W, 0, s())

            def route_nv12():
                ingest_nv12()
                render_nv12()

            def route_rgb():
                ingest_rgb()
                render_rgb()

            ingest_nv12()
            ingest_rgb()
            torch.cuda.synchronize()
            if not torch.equal(pool, pool2):
                raise SystemExit("fused ingest and the two-launch route disagree at %dx%d n=%d" % (W, H, n))
            pair("ingest", n, H, W, [("dvsg_frames_ingest_nv12", ingest_nv12),
                                     ("dvsg_frames_nv12_to_rgb_u8 + dvsg_frames_ingest_u8", ingest_rgb)])
            pair("render", n, H, W, [("dvsg_tps_render_nv12", render_nv12), ("dvsg_tps_render_u8 (u8 -> u8)", render_rgb)])
            pair("ingest + render", n, H, W, [("nv12", route_nv12), ("rgb route", route_rgb)])
            if args.border == "all":
                def through(call, name):
                    view = net.view(args.render_filter, name, *shape)
                    if call == "nv12":
                        return lambda: _lib.call("dvsg_tps_render_nv12", view, F.data_ptr(), y, uv, W, fs, n, H, W, T.data_ptr(),
                                                 out.data_ptr(), out.data_ptr() + H * W, W, fs, s())
                    return lambda: _lib.call("dvsg_tps_render_u8", view, F.data_ptr(), rgb.data_ptr(), n, H, W, 0, T.data_ptr(),
                                             None, out8.data_ptr(), W, 0, s())
                pair("render borders: dvsg_tps_render_nv12", n, H, W,
                     [(b, through("nv12", b)) for b in RENDER_BORDERS] + [("keep's copy (clone)", out.clone)])
                pair("render borders: dvsg_tps_render_u8", n, H, W,
                     [(b, through("u8", b)) for b in RENDER_BORDERS] + [("keep's copy (clone)", out8.clone)])
            del src, out, rgb, out8
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
