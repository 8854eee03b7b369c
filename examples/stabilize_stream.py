#!/usr/bin/env python3
"""Live use of the drop-in: frames arrive one at a time (a camera or a decoder) for one or several streams, and each
step returns every stream's stabilised frame (eval.py:93-124, online).  Decoding is host I/O and not part of this
example: a seeded synthetic uint8 source stands in for it, BGR and larger than the model's size as cv2 would hand
it over (eval.py:76-81 resizes it).  For real footage, `python -m coupe.dvsg_amd.pipe` runs this loop between a decoder and
an encoder that speak uncompressed Y4M or raw NV12 over pipes (coupe/dvsg_amd/pipe.py).

    python examples/stabilize_stream.py [--streams 2] [--frames 48] [--height 288] [--width 512] [--precision f32|f32x3]

--format nv12: the source hands over NV12 surfaces [3 H0 / 2, W0] as a hardware decoder does (built on the host here) and
each step returns the stabilised surfaces at source size in the same layout, ready for an encoder.

--format p010: the same for 10-bit surfaces (HEVC Main10 from a hardware decoder): uint16 [3 H0 / 2, W0], the sample in
each word's high 10 bits; all ten bits come back warped, the network looks at the words' high bytes.

--format nv16 | p210: 4:2:2 surfaces (camera originals, mezzanine files), uint8 [2 H0, W0] and uint16 [2 H0, W0]: H0 rows of Y,
then H0 rows of interleaved U V.  Every chroma row comes back warped; the network looks at the even ones.

--crop auto|Z: the frames come back without sampler A's black border.  Z in (0, 1] is a fixed zoom; "auto" keeps one zoom
per stream on the device and only ever lowers it (OnlineStabilizer(crop="auto")); the zoom each stream has reached is
printed at the end.

--scene-cut THR: every stream notices its own scene cuts on the device and restarts its history (and its crop zoom) at the
cut frame (OnlineStabilizer(scene_cut=THR), THR in (0, 1]; 0.75 separates the two synthetic scenes).  The synthetic source
then cuts from a dark scene to a bright one half way through; the frame each stream's cut was detected at is printed from
`scene_state`.

--skip-length 0,16,24,28,32: another window (the reference's `skip_length`, config.py:48): S strictly increasing frame offsets,
1 <= S <= 16.  The window length belongs to the checkpoint -- its root conv has 3 S input channels -- so the synthetic
checkpoint is made for it (15 channels for the five offsets above; the default is the reference's seven).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from coupe.dvsg_amd.model import StabNet                    # noqa: E402
from coupe.dvsg_amd.online import OnlineStabilizer          # noqa: E402
from coupe.dvsg_amd.weights import make_synthetic_weights   # noqa: E402


def _scene(x, k, cut_at):
    """Frame k of a source in [0, 1]: as it is, or with a cut at frame `cut_at` the dark scene [0.05, 0.45] before it and the
    bright scene [0.55, 0.95] from it on."""
    if cut_at is None:
        return x
    return (0.05 if k < cut_at else 0.55) + 0.4 * x


def synthetic_source(seed, n, h, w, cut_at=None):
    """Yields n BGR uint8 frames [h,w,3], one at a time."""
    import inputs
    bank = inputs.smooth_frames(seed, 8, h, w)[..., ::-1]
    for k in range(n):
        yield np.ascontiguousarray((_scene(bank[k % 8], k, cut_at) * 255).astype(np.uint8))


def synthetic_nv12_source(seed, n, h, w, cut_at=None, rows_c=None):
    """Yields n NV12 frames [3h/2, w] uint8 (h rows of Y, h/2 rows of U0 V0 U1 V1 ...), limited range, one at a time.
    rows_c=h: NV16 frames [2h, w], h chroma rows."""
    import inputs
    rows_c = h // 2 if rows_c is None else rows_c
    y = inputs.smooth_frames(seed, 8, h, w, C=1)[..., 0]
    c = (16 + inputs.smooth_frames(seed + 100, 8, rows_c, w // 2, C=2) * 224).reshape(8, rows_c, w)
    for k in range(n):
        yk = 16 + _scene(y[k % 8], k, cut_at) * 219
        yield np.ascontiguousarray(np.concatenate([yk, c[k % 8]], axis=0).astype(np.uint8))


def synthetic_p010_source(seed, n, h, w, cut_at=None, rows_c=None):
    """Yields n P010 frames [3h/2, w] uint16 (the sample in the high 10 bits, limited range 64 .. 940 / 960), one at a time.
    rows_c=h: P210 frames [2h, w], h chroma rows."""
    import inputs
    rows_c = h // 2 if rows_c is None else rows_c
    y = inputs.smooth_frames(seed, 8, h, w, C=1)[..., 0]
    c = (64 + inputs.smooth_frames(seed + 100, 8, rows_c, w // 2, C=2) * 896).reshape(8, rows_c, w)
    for k in range(n):
        yk = 64 + _scene(y[k % 8], k, cut_at) * 876
        yield np.ascontiguousarray(np.concatenate([yk, c[k % 8]], axis=0).astype(np.uint16) << 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--height", type=int, default=288)    # config.py:12-13
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--precision", default="f32", choices=["f32", "f32x3", "f32s", "f16"])
    ap.add_argument("--format", default="rgb", choices=["rgb", "nv12", "p010", "nv16", "p210"])
    ap.add_argument("--crop", default=None, help="'auto' or a zoom in (0, 1]")
    ap.add_argument("--scene-cut", type=float, default=None, metavar="THR", help="detect scene cuts: a threshold in (0, 1]")
    ap.add_argument("--render-filter", default="bilinear", choices=["bilinear", "bicubic"],
                    help="filter of the source-size render; bicubic with --format rgb turns source_res on")
    ap.add_argument("--border", default="black", choices=["black", "replicate", "mirror", "keep"],
                    help="what the source-size render makes of samples outside the source; anything but black with "
                    "--format rgb turns source_res on, and keep drops the side-by-side frame")
    ap.add_argument("--strength", type=float, default=1.0,
                    help="fraction of the network's warp the source-size render applies, in [0, 1]; anything but 1 with "
                    "--format rgb turns source_res on (as --rigidity does)")
    ap.add_argument("--rigidity", type=float, default=0.0,
                    help="pull of the rendered warp towards its --shape-model fit, in [0, 1]: 1 renders a warp that cannot wobble")
    ap.add_argument("--shape-model", default="affine", choices=["affine", "similarity", "translation"])
    ap.add_argument("--out-size", default=None, metavar="WxH",
                    help="render every stream at this delivery size with an area filter (at most 4x smaller than the source "
                    "per axis); with --format rgb it turns source_res on and drops the side-by-side frame")
    ap.add_argument("--skip-length", default=None, metavar="A,B,...",
                    help="the window's frame offsets, oldest first (default: the reference's 0,16,24,28,30,31,32)")
    args = ap.parse_args()
    window = dict(skip_length=tuple(int(v) for v in args.skip_length.split(","))) if args.skip_length else {}
    S = len(window["skip_length"]) if window else 7
    scene = dict(scene_cut=args.scene_cut) if args.scene_cut is not None else {}
    cut_at = args.frames // 2 if scene else None
    crop = args.crop if args.crop in (None, "auto") else float(args.crop)
    net = StabNet(args.height, args.width).load_weights(make_synthetic_weights(seed=0, c_in=3 * S))
    net.get_evaluation_model(S)
    net.precision = args.precision
    nv12 = args.format in ("nv12", "p010", "nv16", "p210")   # a decoder's surfaces: two planes, rendered at source size
    shape = dict(strength=args.strength, rigidity=args.rigidity, shape_model=args.shape_model)
    shaped = args.strength != 1.0 or args.rigidity != 0.0
    out_size = None
    if args.out_size is not None:
        ow, oh = (int(v) for v in args.out_size.lower().split("x"))
        out_size = (oh, ow)
    if nv12:
        stab = OnlineStabilizer(net, max_streams=args.streams, frame_format=args.format, yuv_matrix="bt709", crop=crop,
                                render_filter=args.render_filter, border=args.border, out_size=out_size, **shape, **scene,
                                **window)
        make = synthetic_nv12_source if args.format in ("nv12", "nv16") else synthetic_p010_source
        if args.format in ("nv16", "p210"):   # 4:2:2: as many chroma rows as luma rows
            frames_420 = make

            def make(seed, n, h, w, cut_at):
                return frames_420(seed, n, h, w, cut_at, rows_c=h)
    else:
        stab = OnlineStabilizer(net, max_streams=args.streams, channel_order="bgr",
                                side_by_side=args.border != "keep" and out_size is None, as_uint8=True, crop=crop,
                                source_res=args.render_filter != "bilinear" or args.border != "black" or shaped
                                or out_size is not None,
                                render_filter=args.render_filter, border=args.border, out_size=out_size, **shape, **scene,
                                **window)
        make = synthetic_source
    H0, W0 = args.height * 3 // 2, args.width * 3 // 2
    if nv12:
        H0, W0 = H0 // 2 * 2, W0 // 2 * 2   # NV12 needs even sizes
    sources = {stab.open(): make(s + 1, args.frames, H0, W0, cut_at) for s in range(args.streams)}
    lat = []
    for k in range(args.frames):
        frames = {sid: next(src) for sid, src in sources.items()}
        t0 = time.perf_counter()
        outs = stab.step(frames)            # NumPy in -> NumPy out: the step has finished when it returns
        lat.append(time.perf_counter() - t0)
        if k == 0 and nv12:
            out = next(iter(outs.values()))
            print("per stream and step: stabilised %s surface" % args.format.upper(), out.shape, out.dtype)
        elif k == 0 and not stab.side_by_side:
            out = next(iter(outs.values()))
            print("per stream and step: stabilised", out.shape, out.dtype)
        elif k == 0:
            out, side = next(iter(outs.values()))
            print("per stream and step: stabilised", out.shape, out.dtype, "| side-by-side", side.shape, side.dtype)
        for sid in sources if scene else ():
            st = stab.scene_state(sid)
            if k > 0 and st["frames_since_cut"] == 1:
                print("stream %d: cut detected at frame %d (the source cuts at %d)" % (sid, k, cut_at))
    for sid in list(sources):
        if crop is not None:
            print("stream %d: zoom %.4f" % (sid, stab.crop_state(sid)["zoom"]))
        if scene:
            st = stab.scene_state(sid)
            print("stream %d: %d cut(s), %d frames since the last, last score %.3f"
                  % (sid, st["cuts"], st["frames_since_cut"], st["score"]))
        stab.close(sid)
    lat = np.array(lat[1:] if len(lat) > 1 else lat) * 1e3
    print("%d stream(s) of %dx%d, %s: median %.2f ms per step (%.2f ms per frame), %.1f frames/s in all"
          % (args.streams, args.width, args.height, args.precision, np.median(lat), np.median(lat) / args.streams,
             args.streams * 1e3 / np.median(lat)))


if __name__ == "__main__":
    main()
