#!/usr/bin/env python3
"""Cost of the P010 path against the NV12 path of the same build: 1080p and 4K, n = 1 and 16, 512 x 288 pool.

render:  dvsg_tps_render_nv12 through a P010 view (16-bit words in and out, twice the bytes)
         vs  dvsg_tps_render_nv12 through the same view without the property (NV12), bilinear and bicubic.
ingest:  the high-byte copy (`src[..., 1::2]` into a buffer) + dvsg_frames_ingest_nv12, what
         OnlineStabilizer(frame_format="p010") does,  vs  dvsg_frames_ingest_nv12 on an NV12 frame.
The versions of a pair ALTERNATE inside every round; device events around `--reps` calls; 7 rounds; median and spread
(min .. max) per call.  One JSON line per measurement; the P010 line of a pair carries `ratio`, its median over the NV12 one.

    python tools/p010_bench.py [--reps 20] [--out FILE]
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
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import inputs
    import nv12_ref
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("p010_bench needs the GPU")
    net = LocNet(make_synthetic_weights(seed=0))
    s = lambda: torch.cuda.current_stream().cuda_stream
    h, w, M = args.model_height, args.model_width, 1   # BT.709
    lines = []

    def pair(what, n, H, W, versions, **more):
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
        base = sorted(per[versions[0][0]])[3]
        for name, _ in versions:
            v = sorted(per[name])
            rec = dict(what=what, version=name, frames=n, height=H, width=W, ms_median=round(v[3], 4), ms_min=round(v[0], 4),
                       ms_max=round(v[-1], 4), us_per_frame=round(1e3 * v[3] / n, 2), **more)
            if name != versions[0][0]:
                rec["ratio"] = round(v[3] / base, 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)

    for H, W in ((1080, 1920), (2160, 3840)):
        one = torch.from_numpy(nv12_ref.smooth_batch(2, 1, H, W).buf).cuda()
        for n in (1, 16):
            src8 = one.repeat(n, 1, 1).contiguous()                                   # NV12 [n, 3H/2, W]
            src10 = torch.stack([torch.zeros_like(src8), src8], dim=-1).reshape(n, 3 * H // 2, 2 * W).contiguous()   # byte << 8
            out8, out10 = torch.empty_like(src8), torch.empty_like(src10)
            hi = torch.empty_like(src8)
            pool = torch.zeros((n, h, w, 3), device="cuda")
            pool2 = torch.zeros_like(pool)
            slots = torch.arange(n, dtype=torch.int32, device="cuda")
            F = torch.from_numpy(inputs.control_vectors(3, n, scale=0.03)).cuda()
            T = torch.empty((n, 2, 28), device="cuda")
            fs = 3 * H // 2 * W

            def ingest8():
                _lib.call("dvsg_frames_ingest_nv12", src8.data_ptr(), src8.data_ptr() + H * W, W, fs, n, H, W, M, pool.data_ptr(), n,
                          slots.data_ptr(), h, w, s())

            def ingest10():
                hi.copy_(src10[..., 1::2])
                _lib.call("dvsg_frames_ingest_nv12", hi.data_ptr(), hi.data_ptr() + H * W, W, fs, n, H, W, M, pool2.data_ptr(), n,
                          slots.data_ptr(), h, w, s())

            ingest8()
            ingest10()
            torch.cuda.synchronize()
            if not torch.equal(pool, pool2):
                raise SystemExit("the high bytes of the P010 frames are not the NV12 frames at %dx%d n=%d" % (W, H, n))
            pair("ingest", n, H, W, [("dvsg_frames_ingest_nv12", ingest8), ("high-byte copy + dvsg_frames_ingest_nv12", ingest10)])
            for filt in ("bilinear", "bicubic"):
                v8, v10 = net.view(filt), net.view(filt, surface="p010")

                def render8():
                    _lib.call("dvsg_tps_render_nv12", v8, F.data_ptr(), src8.data_ptr(), src8.data_ptr() + H * W, W, fs, n, H, W,
                              T.data_ptr(), out8.data_ptr(), out8.data_ptr() + H * W, W, fs, s())

                def render10():
                    _lib.call("dvsg_tps_render_nv12", v10, F.data_ptr(), src10.data_ptr(), src10.data_ptr() + 2 * H * W, 2 * W, 2 * fs,
                              n, H, W, T.data_ptr(), out10.data_ptr(), out10.data_ptr() + 2 * H * W, 2 * W, 2 * fs, s())
                pair("render", n, H, W, [("nv12", render8), ("p010", render10)], render_filter=filt)
            del src8, src10, out8, out10, hi
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
