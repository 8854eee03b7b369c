#!/usr/bin/env python3
"""Cost of stabilised frames at source resolution (OnlineStabilizer(source_res=True), dvsg_tps_render_u8).

1. The render alone against the path it replaces at the source size -- dvsg_frames_u8_to_f32, dvsg_tps_warp_f32,
   dvsg_frames_f32_to_u8, three launches -- for uint8 output, on n frames of each source size: device events around
   `--reps` repetitions of each (median of 5 rounds), and the render's kernel time from the library's dvsg_prof_* class 6
   (TPS grid + sampler A) with its algorithmic bytes.
2. End to end: K = 1, 4, 16 streams of device-resident uint8 frames of each source size through one OnlineStabilizer
   with a 512x288 model, uint8 output (as_uint8), source_res off and on: aggregate frames/s over the host clock around
   the timed steps (which end in a synchronise).
One JSON line per measurement.

--render-filter bicubic measures the renders through a bicubic view of the network (every record names its filter).

--border NAME measures them through a view with that border mode (every record names it); --border all runs part 1 once
per border mode and part 2's source_res runs once per border mode ("keep" includes its copy of the output surface).

--strength S, --rigidity R, --shape-model NAME measure them through a SHAPED view (include/dvsg_amd.h, "Warp shaping": one
kernel in the place of the one that forms T, no launch added); every record names the three values.

    python tools/source_res_bench.py [--steps 30] [--warmup 5] [--sources 1080x1920,2160x3840] [--streams 1,4,16]
                                     [--render-filter bilinear|bicubic] [--border black|replicate|mirror|keep|all]
                                     [--strength S] [--rigidity R] [--shape-model affine|similarity|translation] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=4, help="frames per render launch in part 1")
    ap.add_argument("--model", default="288x512")
    ap.add_argument("--sources", default="1080x1920,2160x3840")
    ap.add_argument("--streams", default="1,4,16")
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--render-filter", default="bilinear", choices=["bilinear", "bicubic"])
    ap.add_argument("--border", default="black", choices=["black", "replicate", "mirror", "keep", "all"])
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--rigidity", type=float, default=0.0)
    ap.add_argument("--shape-model", default="affine", choices=["affine", "similarity", "translation"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 1 or args.reps < 1:
        raise SystemExit("--steps, --warmup and --reps must be >= 1")
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.model import V_SRC, StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("source_res_bench needs the GPU")
    lib = _lib.load()
    h, w = (int(v) for v in args.model.split("x"))
    model = StabNet(h, w).load_weights(make_synthetic_weights(seed=0))
    model.get_evaluation_model(7)
    model.precision = args.precision
    borders = ["black", "replicate", "mirror", "keep"] if args.border == "all" else [args.border]
    shape = dict(strength=args.strength, rigidity=args.rigidity, shape_model=args.shape_model)
    lines = []

    def emit(rec):
        rec.update(shape)
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

    banks = {}
    for size in args.sources.split(","):
        H0, W0 = (int(v) for v in size.split("x"))
        # 8 distinct uint8 frames of this size on the device
        bank = torch.from_numpy((inputs.smooth_frames(11, 8, H0, W0, factor=32) * 255).astype(np.uint8)).cuda()
        banks[size] = bank
        # ---- 1. the render against the three-launch composition
        n = args.n
        src = bank[:n].contiguous()
        F = torch.from_numpy(inputs.control_vectors(12, n)).cuda()
        T = torch.empty((n, 2, 28), device="cuda")
        u8 = torch.empty((n, H0, W0, 3), dtype=torch.uint8, device="cuda")
        U = torch.empty((n, H0, W0, 3), device="cuda")
        warp = torch.empty_like(U)
        coord = torch.from_numpy(np.ascontiguousarray(np.tile(V_SRC[None], (n, 1, 1)))).cuda()

        def three():
            _lib.call("dvsg_frames_u8_to_f32", src.data_ptr(), n * H0 * W0, 1, U.data_ptr(), s())
            _lib.call("dvsg_tps_warp_f32", U.data_ptr(), coord.data_ptr(), T.data_ptr(), n, H0, W0, 3, 25, H0, W0,
                      warp.data_ptr(), 0, 0, s())
            _lib.call("dvsg_frames_f32_to_u8", warp.data_ptr(), n, H0, W0, 1, u8.data_ptr(), W0, 0, s())
        for border in borders:
            handle = model.locnet.view(args.render_filter, border, **shape)

            def render():
                _lib.call("dvsg_tps_render_u8", handle, F.data_ptr(), src.data_ptr(), n, H0, W0, 1, T.data_ptr(), 0,
                          u8.data_ptr(), W0, 0, s())
            t_render, t_three = timed(render), timed(three)
            # the render's warp kernel alone (class 6), with its algorithmic bytes
            _lib.check(lib.dvsg_prof_begin(6), "dvsg_prof_begin")
            for _ in range(args.reps):
                render()
            ms, cnt, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
            _lib.check(lib.dvsg_prof_end(ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)),
                       "dvsg_prof_end")
            k_ms = ms.value / max(cnt.value, 1)
            emit({"what": "render_vs_three_launches", "render_filter": args.render_filter, "border": border, "H0": H0, "W0": W0,
                  "n": n, "render_us_per_frame": 1e3 * t_render / n, "three_launch_us_per_frame": 1e3 * t_three / n,
                  "speedup": t_three / t_render, "render_kernel_us_per_frame": 1e3 * k_ms / n,
                  "render_kernel_GBps": by.value / max(cnt.value, 1) / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None})
    # ---- 2. end to end
    for size, bank in banks.items():
        H0, W0 = (int(v) for v in size.split("x"))
        for K in (int(v) for v in args.streams.split(",")):
            for source_res, border in [(False, "black")] + [(True, b) for b in borders]:
                on = OnlineStabilizer(model, max_streams=K, as_uint8=True, source_res=source_res,
                                      render_filter=args.render_filter if source_res else "bilinear", border=border,
                                      **(shape if source_res else {}))
                sids = [on.open() for _ in range(K)]

                def feed(k):
                    return {sid: bank[(k + 3 * i) % 8] for i, sid in enumerate(sids)}
                for k in range(args.warmup):
                    on.step(feed(k))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(args.steps):
                    on.step(feed(args.warmup + k))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                emit({"what": "online", "render_filter": on.render_filter, "border": border, "model": [h, w], "H0": H0,
                      "W0": W0, "K": K, "source_res": source_res,
                      "precision": args.precision, "steps": args.steps, "frames_per_s": K * args.steps / dt,
                      "ms_per_frame": 1e3 * dt / (K * args.steps)})
                del on
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
