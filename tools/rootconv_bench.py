#!/usr/bin/env python3
"""conv1 alone at several window lengths: B = 16 at 1280 x 720 from a float32 frame ring, S = 1, 5, 7, 8, 9 and 16.

S = 7 is the tuned conv1_kernel; every other S runs rootconv_kernel (cin a kernel argument).  Each line reports ms per
launch from the library's own class-0 hipEvent pairs (dvsg_prof_begin(0)) and TFLOP/s from the hook's own FLOP count
(2 x B x Ho x Wo x 64 x 49 x 3 S), alternating the window lengths over --rounds rounds so that drift shows as spread.
--end-to-end adds OnlineStabilizer at S = 5 against S = 7: ms per step, 720p, one stream.
--only S --reps N: one window length, N launches and nothing else (a counter run: rocprofv3 --pmc ... -- python this)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coupe.dvsg_amd import _lib                              # noqa: E402
from coupe.dvsg_amd.networks import LocNet                   # noqa: E402
from coupe.dvsg_amd.weights import make_synthetic_weights    # noqa: E402

WINDOWS = (1, 5, 7, 8, 9, 16)


def conv1_only(net, pool, table, reps):
    """`reps` stage-0 taps (conv1, then the copy of its output) -> (ms per conv1 launch, TFLOP/s)"""
    net.forward_ring(pool, table, stage=0)
    torch.cuda.synchronize()
    _lib.call("dvsg_prof_begin", 0)
    for _ in range(reps):
        net.forward_ring(pool, table, stage=0)
    ms, n, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    _lib.call("dvsg_prof_end", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by))
    assert n.value == reps, (n.value, reps)
    return ms.value / n.value, fl.value / ms.value / 1e9


def skip_of(S):
    """S strictly increasing offsets that end at 32, like the reference's [0, 16, 24, 28, 30, 31, 32]"""
    return tuple(int(round(v)) for v in np.linspace(0, 32, S)) if S > 1 else (0,)


def end_to_end(S, steps, H, W):
    from coupe.dvsg_amd.model import StabNet
    from coupe.dvsg_amd.online import OnlineStabilizer
    model = StabNet(H, W).load_weights(make_synthetic_weights(seed=0, c_in=3 * S))
    model.get_evaluation_model(S)
    on = OnlineStabilizer(model, skip_length=skip_of(S))
    sid = on.open()
    frames = torch.rand((8, H, W, 3), device="cuda")
    for k in range(8):
        on.push(sid, frames[k])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        on.push(sid, frames[k % 8])
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    B, H, W = args.batch, args.height, args.width
    windows = (args.only,) if args.only else WINDOWS
    gen = torch.Generator(device="cuda").manual_seed(1234)
    n_pool = B + max(windows)
    pool = torch.rand((n_pool, H, W, 3), generator=gen, device="cuda")
    nets, tables = {}, {}
    for S in windows:
        nets[S] = LocNet(make_synthetic_weights(seed=0, c_in=3 * S))
        tables[S] = (torch.arange(B, dtype=torch.int32, device="cuda")[:, None]
                     + torch.arange(S, dtype=torch.int32, device="cuda")[None, :]).contiguous()
    if args.only:
        for _ in range(args.reps):
            nets[args.only].forward_ring(pool, tables[args.only], stage=0)
        torch.cuda.synchronize()
        return
    seen = {S: [] for S in windows}
    for _ in range(args.rounds):
        for S in windows:
            seen[S].append(conv1_only(nets[S], pool, tables[S], args.reps))
    base = max(t for _, t in seen[7])
    for S in windows:
        ms = [m for m, _ in seen[S]]
        tf = [t for _, t in seen[S]]
        print(json.dumps({"what": "conv1", "S": S, "B": B, "H": H, "W": W, "kernel": "conv1_kernel" if S == 7 else "rootconv_kernel",
                          "ms_per_launch": round(min(ms), 4), "ms_spread": round(max(ms) - min(ms), 4),
                          "tflops": round(max(tf), 2), "of_S7": round(max(tf) / base, 3)}))
    if args.end_to_end:
        del nets
        torch.cuda.empty_cache()
        for S in (7, 5, 7, 5):
            print(json.dumps({"what": "online_step", "S": S, "H": H, "W": W, "streams": 1,
                              "ms_per_step": round(end_to_end(S, args.steps, H, W), 3)}))


if __name__ == "__main__":
    main()
