#!/usr/bin/env python3
"""Cost of 4:2:2 frames against 4:2:0 frames of the same luma size on the same build: NV16 against NV12 and P210 against
P010, 1080p and 4K, n = 1 and 4, bilinear and bicubic, at source size and 4K -> 1080p.

render:  dvsg_tps_render_zoom_nv12 (zoom 0.9) through `LocNet.view(..., chroma="422")`  vs  the same view without the
         property.  A 4:2:2 frame has 2 samples per luma sample where a 4:2:0 frame has 1.5, so 4 / 3 of the samples are
         read and written; every record carries that figure as `samples_ratio` and the measured `ratio` beside it.
ingest:  the even-chroma-row gather + dvsg_frames_ingest_nv12, what OnlineStabilizer(frame_format="nv16" | "p210") does,
         vs  what "nv12" | "p010" does (dvsg_frames_ingest_nv12; the high-byte copy first for words).
The versions of a pair ALTERNATE inside every round; device events around `--reps` calls; 7 rounds; median and spread
(min .. max) per call.  One JSON line per measurement; the 4:2:2 line of a pair carries `ratio`, its median over the 4:2:0 one.

    python tools/yuv422_bench.py [--reps 20] [--out FILE]
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
    import numpy as np
    import torch
    import inputs
    from coupe.dvsg_amd import _lib
    from coupe.dvsg_amd.networks import LocNet
    from coupe.dvsg_amd.weights import make_synthetic_weights
    if not torch.cuda.is_available():
        raise SystemExit("yuv422_bench needs the GPU")
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
                rec["samples_ratio"] = round(4.0 / 3.0, 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)

    def surface(H, W, rows_c, words):
        """one smooth frame [H + rows_c, bps W] on the device: Y, then rows_c rows of interleaved UV; words: byte << 8"""
        y = 16 + inputs.smooth_frames(2, 1, H, W, C=1, factor=32)[..., 0] * 219
        c = 16 + inputs.smooth_frames(3, 1, rows_c, W // 2, C=2, factor=32) * 224
        f = torch.from_numpy(np.concatenate([y, c.reshape(1, rows_c, W)], axis=1).astype(np.uint8)).cuda()
        return torch.stack([torch.zeros_like(f), f], dim=-1).reshape(1, H + rows_c, 2 * W).contiguous() if words else f

    for H, W in ((1080, 1920), (2160, 3840)):
        for words in (False, True):
            bps = 2 if words else 1
            names = ("p010", "p210") if words else ("nv12", "nv16")
            one420, one422 = surface(H, W, H // 2, words), surface(H, W, H, words)
            for n in (1, 4):
                src420, src422 = one420.repeat(n, 1, 1).contiguous(), one422.repeat(n, 1, 1).contiguous()
                seen = torch.empty((n, 3 * H // 2, W), dtype=torch.uint8, device="cuda")
                picked = torch.cat([torch.arange(H), torch.arange(H, 2 * H, 2)]).cuda()   # Y rows, then the even chroma rows
                pool = torch.zeros((n, h, w, 3), device="cuda")
                slots = torch.arange(n, dtype=torch.int32, device="cuda")
                F = torch.from_numpy(inputs.control_vectors(3, n, scale=0.03)).cuda()
                zoom = torch.full((n,), 0.9, device="cuda")
                T = torch.empty((n, 2, 28), device="cuda")

                def ingest(src, c422):
                    def f():
                        x = src
                        if words or c422:
                            hi = src[..., 1::2] if words else src
                            if c422:
                                torch.index_select(hi, 1, picked, out=seen)
                            else:
                                seen.copy_(hi)
                            x = seen
                        _lib.call("dvsg_frames_ingest_nv12", x.data_ptr(), x.data_ptr() + H * W, W, 3 * H // 2 * W, n, H, W, M,
                                  pool.data_ptr(), n, slots.data_ptr(), h, w, s())
                    return f
                pair("ingest", n, H, W, [(names[0], ingest(src420, False)), (names[1], ingest(src422, True))])
                sizes = [(H, W)] + ([(1080, 1920)] if H == 2160 else [])
                for oh, ow in sizes:
                    for filt in ("bilinear", "bicubic"):
                        kw = dict(surface="p010" if words else "nv12", out_size=None if (oh, ow) == (H, W) else (oh, ow))
                        v420, v422 = net.view(filt, **kw), net.view(filt, chroma="422", **kw)
                        out420 = torch.empty((n, 3 * oh // 2, bps * ow), dtype=torch.uint8, device="cuda")
                        out422 = torch.empty((n, 2 * oh, bps * ow), dtype=torch.uint8, device="cuda")

                        def render(view, src, out):
                            pitch, opitch = bps * W, bps * ow
                            fs, ofs = int(src.shape[1]) * pitch, int(out.shape[1]) * opitch

                            def f():
                                _lib.call("dvsg_tps_render_zoom_nv12", view, F.data_ptr(), src.data_ptr(), src.data_ptr() + H * pitch,
                                          pitch, fs, n, H, W, zoom.data_ptr(), T.data_ptr(), out.data_ptr(),
                                          out.data_ptr() + oh * opitch, opitch, ofs, s())
                            return f
                        pair("render", n, H, W, [(names[0], render(v420, src420, out420)), (names[1], render(v422, src422, out422))],
                             render_filter=filt, out_height=oh, out_width=ow)
                        del out420, out422
                del src420, src422, seen
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
