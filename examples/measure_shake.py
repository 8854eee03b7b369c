#!/usr/bin/env python3
"""How much steadier is the output?  Stabilise the seeded synthetic clip (as examples/stabilize_clip.py does) and print the
no-reference shake figures of the input and of the output, and their jitter ratio (coupe.dvsg_amd.shake: block matching
between consecutive luma planes, on the device), then the roll, zoom and wobble that a similarity fitted to the same block
vectors shows (shake.measure_motion).  With the seeded synthetic checkpoint the ratio says nothing about a
trained model: give --ckpt for that.

    python examples/measure_shake.py [--frames 16] [--height 288] [--width 512] [--ckpt DIR] [--precision f32|f32x3|f32s|f16]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from coupe.dvsg_amd import shake                         # noqa: E402
from coupe.dvsg_amd.clip import stabilize_clip           # noqa: E402
from coupe.dvsg_amd.model import Session, StabNet        # noqa: E402
from coupe.dvsg_amd.weights import make_synthetic_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--ckpt", default=None, help="reference checkpoint directory (with its `checkpoints` index)")
    ap.add_argument("--precision", default="f32", choices=["f32", "f32x3", "f32s", "f16"])
    args = ap.parse_args()
    import inputs
    frames = (inputs.smooth_frames(1, args.frames, args.height, args.width) * 255).astype(np.uint8)   # RGB uint8 [N, H, W, 3]
    net = StabNet(args.height, args.width)
    net.precision = args.precision
    net.get_evaluation_model(7)
    if args.ckpt:
        net.load_ckpt(args.ckpt, by_score=True)
    else:
        net.load_weights(make_synthetic_weights(seed=0))
    stabilised = stabilize_clip(net, Session(), frames, as_uint8=True)
    # the same geometry for both; the margin keeps the output's black border out of the blocks
    motion_before = shake.measure_motion(shake.luma_of(frames, "rgb"))
    motion_after = shake.measure_motion(shake.luma_of(np.asarray(stabilised), "rgb"))
    # columns 0 - 3 of a motion row are the row `shake.measure` gives: one pass over the clip serves both
    before, after = (shake.Track(m.rows[:, :4], m.factor, m.size, None) for m in (motion_before, motion_after))
    result = shake.compare(before, after)
    for name, s in (("before", result["a"]), ("after", result["b"])):
        print("%-6s %d pairs, %d lost, speed %s px/frame, jitter %s px/frame" % (name, s["pairs"], s["lost"], s["speed_rms"], s["jitter_rms"]))
    print("jitter ratio after / before:", result["jitter_ratio"])
    motion = shake.compare_motion(motion_before, motion_after)
    for name, s in (("before", motion["a"]), ("after", motion["b"])):
        print("%-6s roll %s deg/frame, roll jitter %s deg/frame, zoom jitter %s %%/frame, wobble %s px, %d of %d pairs unfit" % (
            name, s["roll_rms_deg"], s["roll_jitter_deg"], s["zoom_jitter_pct"], s["wobble_rms"], s["unfit"], s["pairs"]))
    print("roll jitter ratio after / before:", motion["roll_jitter_ratio"])
    print("wobble ratio after / before:", motion["wobble_ratio"])


if __name__ == "__main__":
    main()
