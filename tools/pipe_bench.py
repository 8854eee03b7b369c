#!/usr/bin/env python3
"""Throughput of pipe.stabilize_pipes from memory to memory, against OnlineStabilizer.step on device-resident frames.

No disk and no codec: a source copies the next of a few seeded I420 frames into the buffer it is handed (what reading a
pipe costs at least: one copy), a sink copies the frame it is handed into a scratch buffer.  For each size (1080p, 4K), each
number of inputs (1, 4) and each depth (1, 3), `stabilize_pipes` runs --frames frames per input through a 512x288 f32 model
with synthetic weights; the host clock runs around the whole call (set-up, threads and the last write included).  The depths
alternate inside each of --rounds rounds.  Next to them the ceiling: the same frames as NV12 tensors on the device, the same
number of streams, through `OnlineStabilizer.step` and a synchronise -- no upload, no repack, no download.  One JSON line per
case, with every round's figure and the median.

--bits 10: the same frames as a 10-bit source (C420p10 bytes, every sample the 8-bit one << 2), through
OnlineStabilizer(frame_format="p010"); every record names the bit depth.

    python tools/pipe_bench.py [--sizes 1920x1080,3840x2160] [--inputs 1,4] [--depths 3,1] [--frames 96] [--rounds 3] [--bits 8|10]
                               [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class MemorySource(object):
    """n frames, cycling through `bank` [m, 3 H / 2, W] (10-bit: [m, 3 H / 2, 2 W]; stream s starts at frame 3 s)."""

    def __init__(self, bank, n, s, bits=8):
        self.bank, self.n, self.k, self.s = bank, n, 0, 3 * s
        self.layout = "i420p10" if bits == 10 else "i420"
        self.height, self.width = 2 * bank.shape[1] // 3, bank.shape[2] // (2 if bits == 10 else 1)
        self.frame_shape = tuple(bank.shape[1:])

    def readinto(self, buf):
        import numpy as np
        if self.k == self.n:
            return False
        np.copyto(buf, self.bank[(self.k + self.s) % len(self.bank)])
        self.k += 1
        return True


class MemorySink(object):
    def __init__(self, shape, bits=8):
        import numpy as np
        self.layout = "i420p10" if bits == 10 else "i420"
        self.scratch, self.frames = np.empty(shape, np.uint8), 0

    def write(self, frame):
        import numpy as np
        np.copyto(self.scratch, frame)
        self.frames += 1


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160", help="WxH,...")
    ap.add_argument("--inputs", default="1,4")
    ap.add_argument("--depths", default="3,1")
    ap.add_argument("--frames", type=int, default=96, help="per input and run")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--bits", type=int, default=8, choices=[8, 10])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import nv12_ref
    from coupe.dvsg_amd import y4m
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    from coupe.dvsg_amd.pipe import stabilize_pipes
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("pipe_bench needs the GPU")
    model = StabNet(288, 512).load_weights(make_synthetic_weights(seed=0))
    model.get_evaluation_model(7)
    model.precision = "f32"
    depths = [int(v) for v in args.depths.split(",")]

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    for size in args.sizes.split(","):
        W0, H0 = (int(v) for v in size.lower().split("x"))
        nv12 = torch.from_numpy(nv12_ref.smooth_batch(21, 4, H0, W0).buf)
        bank = y4m.nv12_to_i420(nv12).numpy()
        if args.bits == 10:   # planar samples b << 2 as little-endian words; on the device P010 words, b << 8
            bank = np.ascontiguousarray((bank.astype(np.uint16) << 2).astype("<u2")).view(np.uint8)
            nv12 = torch.stack([torch.zeros_like(nv12), nv12], dim=-1).reshape(nv12.shape[0], nv12.shape[1], -1).contiguous()
        nv12_dev = nv12.cuda()
        matrix = y4m.default_yuv_matrix(H0)
        for K in (int(v) for v in args.inputs.split(",")):
            def run(depth, n):
                sources = [MemorySource(bank, n, s, args.bits) for s in range(K)]
                sinks = [MemorySink(bank.shape[1:], args.bits) for _ in range(K)]
                t0 = time.perf_counter()
                stats = stabilize_pipes(model, sources, sinks, depth=depth)
                dt = time.perf_counter() - t0
                assert [s["frames"] for s in stats] == [n] * K and all(s.frames == n for s in sinks)
                return K * n / dt

            def ceiling(n):
                on = OnlineStabilizer(model, max_streams=K, frame_format="p010" if args.bits == 10 else "nv12", yuv_matrix=matrix)
                sids = [on.open() for _ in range(K)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(n):
                    on.step({sid: nv12_dev[(k + 3 * s) % len(nv12_dev)] for s, sid in enumerate(sids)})
                torch.cuda.synchronize()
                return K * n / (time.perf_counter() - t0)

            for d in depths:
                run(d, args.warmup)
            ceiling(args.warmup)
            rates = {d: [] for d in depths}
            top = []
            for _ in range(args.rounds):
                for d in depths:
                    rates[d].append(run(d, args.frames))
                top.append(ceiling(args.frames))
            base = dict(W=W0, H=H0, bits=args.bits, inputs=K, frames_per_input=args.frames, rounds=args.rounds, model="512x288 f32")
            for d in depths:
                emit(dict(base, what="stabilize_pipes", depth=d, frames_per_s=median(rates[d]), runs=rates[d]))
            emit(dict(base, what="device_resident_step", frames_per_s=median(top), runs=top))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
