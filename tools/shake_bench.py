#!/usr/bin/env python3
"""Cost of the shake measurement (dvsg_shake_measure_u8, DESIGN section 5, "Shake measurement") at the sizes it is meant for:
1080p reduced by 4 and 4K reduced by 8, both 270 x 480 reduced planes with 264 blocks at radius 12, n = 64 frames per call.

call:     device events on the legacy default stream around the call (the wait, the three launches and the two copies to the
          host) and the host clock around the same call; 7 rounds after 2 warm-up calls; median and spread (min .. max), per
          call and per pair.
kernels:  the entry point is synchronous, so no event can be put between its launches: the three kernels' times come from a
          run of their own under rocprofv3 (`--kernels-only`, a few calls, nothing timed):
              rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/shake_bench.py --kernels-only
              python tools/stats_sum.py DIR
          Every record here carries `reduce_bytes`, what shake_reduce_kernel reads and writes per call, to set against that
          kernel's time.
numpy:    tests/shake_ref.py on the first pairs of the same clip on the host's cores, seconds per pair, its rows compared
          with the device's -- a statement of scale, not a requirement.
motion:   with --motion, dvsg_shake_motion_u8 (shake.measure_motion, "Shake motion" in DESIGN section 5) beside the existing call
          on the same planes: the two are timed in turn within every round, by the same events and clock, and their records
          carry `call`; the kernels-only run makes three calls of each, so the trace holds shake_global_kernel and
          shake_motion_kernel side by side.  Columns 0 - 3 of the new rows are compared with the existing call's.
One JSON line per measurement.

    python tools/shake_bench.py [--rounds 7] [--frames 64] [--numpy-pairs 2] [--motion] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (("1080p", 1080, 1920), ("4K", 2160, 3840))


def wandering_clip(np, shake_ref, seed, n, H, W, f):
    """n frames of H x W: a texture (17 f / 4-wide box) seen through a window that walks by up to 6 reduced pixels a frame"""
    pad = 8 * f
    big = shake_ref.texture(seed, H + 2 * pad, W + 2 * pad, box=17 * f // 4 | 1)
    rng = np.random.RandomState(seed)
    steps = rng.randint(-6 * f, 6 * f + 1, size=(n, 2))
    pos = np.zeros(2, dtype=np.int64)
    frames = []
    for t in range(n):
        pos = np.clip(pos + steps[t], -pad, pad) if t else pos
        frames.append(shake_ref.shifted(big, int(pos[0]), int(pos[1]), H, W, pad))
    return np.stack(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--numpy-pairs", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="three calls per size and nothing else: the run rocprofv3 traces")
    ap.add_argument("--motion", action="store_true", help="also time dvsg_shake_motion_u8 on the same planes, in turn with the other")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import shake_ref
    from coupe.dvsg_amd import shake
    if not torch.cuda.is_available():
        raise SystemExit("shake_bench needs the GPU")
    lines = []

    def emit(**record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    def stats(values):
        values = sorted(values)
        return dict(median=values[len(values) // 2], min=values[0], max=values[-1])

    n = args.frames
    for name, H, W in SIZES:
        f, my, mx = shake.geometry(H, W)
        clip = wandering_clip(np, shake_ref, 5, n, H, W, f)
        dev = torch.from_numpy(clip).cuda()
        kw = dict(chunk=n)
        calls = [("dvsg_shake_measure_u8", shake.measure)] + ([("dvsg_shake_motion_u8", shake.measure_motion)] if args.motion else [])
        for _ in range(3 if args.kernels_only else 2):
            track = shake.measure(dev, **kw)
            if args.motion:
                motion = shake.measure_motion(dev, **kw)
        if args.motion and motion.rows[:, :4].tolist() != track.vectors.tolist():
            raise SystemExit("%s: columns 0 - 3 of the motion rows differ from dvsg_shake_measure_u8's" % name)
        if args.kernels_only:
            continue
        h, w = H // f, W // f
        common = dict(size=name, H=H, W=W, factor=f, frames=n, pairs=n - 1, blocks=((h - 2 * my) // 16) * ((w - 2 * mx) // 16),
                      radius=12, reduce_bytes=n * (h * f * w * f + h * w), lost=int((track.vectors[:, 3] == 0).sum()))
        event_ms, host_ms = {c: [] for c, _ in calls}, {c: [] for c, _ in calls}
        for _ in range(args.rounds):
            for c, fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                fn(dev, **kw)
                t1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize()
                event_ms[c].append(e0.elapsed_time(e1))
                host_ms[c].append(1e3 * (t1 - t0))
        for c, _ in calls:
            extra = dict(call=c, **common) if args.motion else common
            for what, values in (("device events around the call", event_ms[c]), ("host clock around the call", host_ms[c])):
                s = stats(values)
                emit(what=what, unit="ms", per_call=s, per_pair={k: v / (n - 1) for k, v in s.items()}, rounds=args.rounds, **extra)
        if args.motion:
            fit = [shake.motion_figures(r, f)["fit"] for r in motion.rows]
            emit(what="motion rows", size=name, pairs=n - 1, fit=sum(fit), inliers=stats([int(v) for v in motion.rows[:, 4]]))
        seconds = []
        for t in range(1, args.numpy_pairs + 1):
            t0 = time.perf_counter()
            vectors, _ = shake_ref.measure(clip[t - 1:t + 1], f, 12, my, mx, 256, 8)
            seconds.append(time.perf_counter() - t0)
            if vectors[0].tolist() != track.vectors[t - 1].tolist():
                raise SystemExit("pair %d: NumPy %s, device %s" % (t, vectors[0].tolist(), track.vectors[t - 1].tolist()))
        if seconds:
            emit(what="tests/shake_ref.py on the host, same rows as the device", unit="s", per_pair=stats(seconds),
                 pairs_timed=len(seconds), **{k: common[k] for k in ("size", "H", "W", "factor", "blocks", "radius")})
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
