#!/usr/bin/env python3
"""Throughput of online streams (coupe.dvsg_amd.online) against the one-clip loop (clip.stabilize_clip).

For each size (720p and the reference's 512x288) and precision (f32, f32x3): K = 1, 4, 16 streams of same-size uint8
frames already on the device go through one OnlineStabilizer in lockstep -- one batched
dvsg_stabilize_ring_inplace_f32 call per step -- and the aggregate frames/s (K x steps over the host clock around
the timed steps, which end in a synchronise) and the median step time (device events around each step) are reported.
stabilize_clip on one clip of the same frames is the K = 1 reference.  One JSON line per measurement.

    python tools/online_bench.py [--steps 40] [--warmup 6] [--sizes 720x1280,288x512] [--precisions f32,f32x3] [--out FILE]

--crop: the cost of OnlineStabilizer(crop=...) per step instead.  K streams of device-resident 1080p frames (--source),
NV12 surfaces and RGB uint8 with source_res (--formats; also p010, nv16, p210), through a 512x288 f32 model: one OnlineStabilizer per variant
(--variants none,0.9,auto: crop=None, a fixed zoom, the per-stream ratchet), all warmed up, then --rounds rounds in each of
which every variant in turn runs --steps steps between device events, so the variants alternate inside a round.  One JSON
line per (format, K, variant): the median, smallest and largest step over all rounds.  "none" passes no crop argument at
all, so the same file measures a tree from before the option.

    python tools/online_bench.py --crop [--source 1080x1920] [--formats nv12,rgb] [--variants none,0.9,auto] [--rounds 5]

--scene-cut [THR]: the cost of OnlineStabilizer(scene_cut=THR) per step (default 0.75).  For each size of --sizes and each
K of --streams, same-size uint8 frames on the device through the first precision of --precisions: one OnlineStabilizer with
the option off and one with it on, measured like --crop (warmed up, the two alternating inside each of --rounds rounds).  One
JSON line per (size, K, variant) with the cuts the run detected.  "off" passes no scene argument at all, so
`--scene-cut --variants off` of this file measures a tree from before the option.

    python tools/online_bench.py --scene-cut [0.75] [--sizes 720x1280,288x512] [--variants off,on] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--sizes", default="720x1280,288x512")
    ap.add_argument("--precisions", default="f32,f32x3")
    ap.add_argument("--streams", default="1,4,16")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--crop", action="store_true", help="measure the per-step cost of OnlineStabilizer(crop=...)")
    ap.add_argument("--source", default="1080x1920")
    ap.add_argument("--formats", default="nv12,rgb")
    ap.add_argument("--variants", default=None, help="--crop: none,0.9,auto (default: all); --scene-cut: off,on")
    ap.add_argument("--scene-cut", type=float, nargs="?", const=0.75, default=None, metavar="THR",
                    help="measure the per-step cost of OnlineStabilizer(scene_cut=THR)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 1:
        raise SystemExit("--steps and --warmup must be >= 1")
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd.clip import stabilize_clip
    from coupe.dvsg_amd.model import Session, StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("online_bench needs the GPU")
    weights = make_synthetic_weights(seed=0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def flush():
        if args.out:
            with open(args.out, "a") as f:
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")

    if args.crop or args.scene_cut is not None:
        if args.crop:
            args.variants = args.variants or "none,0.9,auto"
            crop_legs(args, weights, emit)
        else:
            args.variants = args.variants or "off,on"
            scene_legs(args, weights, emit)
        flush()
        return

    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        model = StabNet(H, W).load_weights(weights)
        model.get_evaluation_model(7)
        # 8 distinct uint8 frames on the device; stream s at step k reads frame (k + 3 s) % 8
        bank = torch.from_numpy((inputs.smooth_frames(11, 8, H, W) * 255).astype(np.uint8)).cuda()
        for prec in args.precisions.split(","):
            model.precision = prec
            # the one-clip loop: batch 1, a clip of warmup + steps frames on the device, timed after a warm-up clip
            n = args.warmup + args.steps
            clip = bank[torch.arange(n) % 8].contiguous()
            stabilize_clip(model, Session(), clip[:args.warmup])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stabilize_clip(model, Session(), clip)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit({"what": "stabilize_clip", "H": H, "W": W, "precision": prec, "K": 1, "frames": n,
                  "frames_per_s": n / dt, "ms_per_frame": 1e3 * dt / n})
            for K in (int(v) for v in args.streams.split(",")):
                on = OnlineStabilizer(model, max_streams=K)
                sids = [on.open() for _ in range(K)]

                def feed(k):
                    return {sid: bank[(k + 3 * s) % 8] for s, sid in enumerate(sids)}
                for k in range(args.warmup):
                    on.step(feed(k))
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                t0 = time.perf_counter()
                for k in range(args.steps):
                    ev[k][0].record()
                    on.step(feed(args.warmup + k))
                    ev[k][1].record()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                step_ms = sorted(a.elapsed_time(b) for a, b in ev)
                emit({"what": "online", "H": H, "W": W, "precision": prec, "K": K, "steps": args.steps,
                      "frames_per_s": K * args.steps / dt, "median_step_ms": step_ms[len(step_ms) // 2],
                      "min_step_ms": step_ms[0], "max_step_ms": step_ms[-1], "ms_per_frame": 1e3 * dt / (K * args.steps),
                      "pool_frames": int(on.pool.shape[0])})
                del on
                torch.cuda.empty_cache()
    flush()


def crop_legs(args, weights, emit):
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    H0, W0 = (int(v) for v in args.source.split("x"))
    h, w = 288, 512
    model = StabNet(h, w).load_weights(weights)
    model.get_evaluation_model(7)
    model.precision = "f32"
    variants = args.variants.split(",")
    for fmt in args.formats.split(","):
        # 8 distinct frames on the device; stream s at step k reads frame (k + 3 s) % 8
        if fmt in ("nv12", "p010", "nv16", "p210"):   # surfaces: 4:2:2 has H0 chroma rows; words are byte << 8
            rows_c = H0 if fmt in ("nv16", "p210") else H0 // 2
            y = 16 + inputs.smooth_frames(11, 8, H0, W0, C=1, factor=32)[..., 0] * 219
            c = 16 + inputs.smooth_frames(12, 8, rows_c, W0 // 2, C=2, factor=32) * 224
            bank = torch.from_numpy(np.concatenate([y, c.reshape(8, rows_c, W0)], axis=1).astype(np.uint8)).cuda()
            if fmt in ("p010", "p210"):
                bank = torch.stack([torch.zeros_like(bank), bank], dim=-1).reshape(8, H0 + rows_c, 2 * W0).contiguous()
            base = dict(frame_format=fmt)
        else:
            bank = torch.from_numpy((inputs.smooth_frames(11, 8, H0, W0, factor=32) * 255).astype(np.uint8)).cuda()
            base = dict(source_res=True, as_uint8=True)
        for K in (int(v) for v in args.streams.split(",")):
            stabs = []
            for v in variants:
                kw = dict(base) if v == "none" else dict(base, crop="auto" if v == "auto" else float(v))
                on = OnlineStabilizer(model, max_streams=K, **kw)
                stabs.append((v, on, [on.open() for _ in range(K)], []))
            _alternate(stabs, bank, args)
            for v, on, sids, times in stabs:
                t = sorted(times)
                rec = {"what": "online_crop", "format": fmt, "source_H": H0, "source_W": W0, "H": h, "W": w, "precision": "f32",
                       "K": K, "crop": v, "rounds": args.rounds, "steps_per_round": args.steps,
                       "median_step_ms": t[len(t) // 2], "min_step_ms": t[0], "max_step_ms": t[-1],
                       "p10_step_ms": t[len(t) // 10], "p90_step_ms": t[(9 * len(t)) // 10]}
                if v == "auto":
                    rec["zoom"] = [float(on.crop_state(sid)["zoom"]) for sid in sids][:4]
                emit(rec)
            del stabs
            torch.cuda.empty_cache()


def _alternate(stabs, bank, args):
    """Warm every (variant, stabiliser, stream ids, times) of `stabs` up, then --rounds rounds in each of which every variant
    in turn runs --steps steps between device events; the step times in ms are appended to `times`.  Stream s at step k
    reads frame (k + 3 s) % 8 of `bank`."""
    import torch
    for _, on, sids, _ in stabs:
        for k in range(args.warmup):
            on.step({sid: bank[(k + 3 * s) % 8] for s, sid in enumerate(sids)})
    torch.cuda.synchronize()
    step_no = 0
    for r in range(args.rounds):
        for _, on, sids, times in stabs:   # the variants alternate inside the round
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for k in range(args.steps):
                feed = {sid: bank[(step_no + k + 3 * s) % 8] for s, sid in enumerate(sids)}
                ev[k][0].record()
                on.step(feed)
                ev[k][1].record()
            torch.cuda.synchronize()
            times.extend(a.elapsed_time(b) for a, b in ev)
        step_no += args.steps


def scene_legs(args, weights, emit):
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    variants = args.variants.split(",")
    if any(v not in ("off", "on") for v in variants):
        raise SystemExit("--scene-cut takes --variants off, on or off,on")
    prec = args.precisions.split(",")[0]
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        model = StabNet(H, W).load_weights(weights)
        model.get_evaluation_model(7)
        model.precision = prec
        bank = torch.from_numpy((inputs.smooth_frames(11, 8, H, W) * 255).astype(np.uint8)).cuda()
        for K in (int(v) for v in args.streams.split(",")):
            stabs = []
            for v in variants:
                on = OnlineStabilizer(model, max_streams=K, **(dict(scene_cut=args.scene_cut) if v == "on" else {}))
                stabs.append((v, on, [on.open() for _ in range(K)], []))
            _alternate(stabs, bank, args)
            for v, on, sids, times in stabs:
                t = sorted(times)
                rec = {"what": "online_scene", "H": H, "W": W, "precision": prec, "K": K,
                       "scene_cut": args.scene_cut if v == "on" else "off", "rounds": args.rounds,
                       "steps_per_round": args.steps, "median_step_ms": t[len(t) // 2], "min_step_ms": t[0],
                       "max_step_ms": t[-1], "p10_step_ms": t[len(t) // 10], "p90_step_ms": t[(9 * len(t)) // 10]}
                if v == "on":
                    rec["cuts"] = sum(on.scene_state(sid)["cuts"] for sid in sids)
                emit(rec)
            del stabs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
