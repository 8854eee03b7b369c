#!/usr/bin/env python3
"""One line per conv1 case: the launch record and the sha1 of the output bytes, for comparing two builds of the library.

The cases are the tests' own tables -- CASES and MARCH_CASES of tests/test_root_head_f64.py (every instantiation of the six
S = 7 kernels), BAND_CASES of tests/test_root_band.py (root_band_kernel) and CASES of tests/test_rootconv_f64.py (every rootconv_kernel instantiation, S = 1, 2, 5, 8, 16) -- with the
tests' seeded inputs; each is one tap-0 network call.  Then the root max pool: stage-1 taps at the shapes FIRST, CORNER and
SINGLE and the six sources of tests/test_root_pool_fused.py, float32 through the band kernel under root_pool 1 (the plain
pool kernel) and 2 (the pool in the band kernel's epilogue), and the float16, f32s and f32x3 precisions' pool kernels.  Run
it once per library in a fresh process,

    DVSG_AMD_LIB=parent/libdvsg_amd.so python tools/conv1_digest.py > parent.txt
    python tools/conv1_digest.py > tree.txt

and compare the two outputs line for line: a change of source text that left the arithmetic and its order alone leaves every
line as it was (profiles/r18_conv1_digest.log)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_root_head_f64 as rh                              # noqa: E402
import test_rootconv_f64 as rc                               # noqa: E402
import test_root_band as rb                                  # noqa: E402
import test_root_pool_fused as rp                            # noqa: E402
from coupe.dvsg_amd.weights import make_synthetic_weights    # noqa: E402


def line(name, rec, y):
    print("%s | %s | %s" % (name, " ".join("%d" % v for v in rec), hashlib.sha1(y.numpy().tobytes()).hexdigest()), flush=True)


def main():
    from coupe.dvsg_amd import _lib
    sys.stderr.write("library: %s\n" % _lib.LIB_PATH)      # (not on stdout: the two outputs are compared whole)
    dev = torch.device("cuda:0")
    weights = make_synthetic_weights(seed=0)
    for case in rh.CASES + rh.MARCH_CASES:
        prec, variant, kind, masked, off_grid, (B, H, W), inputs, exp = case
        net, _ = rh._net(weights, inputs == "pos")
        src, tab, mask, n, _, _ = rh.place_inputs(case, dev)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        try:
            rh._set_variant(variant)
            y, rec = rh.run_net(net, prec, kind, masked, src, tab, mask, n, B, H, W, 0, B * Ho * Wo * 64)
        finally:
            rh._set_variant(0)
        line(rh.case_id(case), rec, y)
    for shape, off, kind, inputs in rb.BAND_CASES:      # root_band_kernel, forced at the parity tests' small shapes
        case = ("f32", 6, kind, 0, off, shape, inputs, None)
        net, _ = rh._net(weights, False)
        src, tab, mask, n, _, _ = rh.place_inputs(case, dev)
        (B, H, W), Ho, Wo = shape, (shape[1] - 1) // 2 + 1, (shape[2] - 1) // 2 + 1
        try:
            rh._set_variant(6)
            y, rec = rh.run_net(net, "f32", kind, 0, src, tab, None, n, B, H, W, 0, B * Ho * Wo * 64)
        finally:
            rh._set_variant(0)
        line(rh.case_id(case), rec, y)
    for case in rc.CASES:
        prec, S, kind, masked, off_grid, (B, H, W), inputs = case
        net, _ = rc.net_for(S, inputs == "pos")
        src_h, table_h, _, mk = rc.make_inputs(case)
        src = rh.Placed(src_h, dev, (1 if kind == 2 else 4) if off_grid else 0)
        tab = rh.Placed(table_h, dev) if kind else None
        mask = rh.Placed(mk, dev) if masked else None
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y, rec = rh.run_net(net, prec, kind, masked, src, tab, mask, B * S, B, H, W, 0, B * Ho * Wo * 64)
        line(rc.case_id(case), rec, y)
    # stage-1 taps: the root max pool.  Float32 through the forced band kernel, as its own kernel (root_pool 1:
    # maxpool_kernel<float>) and in the band kernel's epilogue (root_pool 2: root_band_pool_kernel + root_pool_seams_kernel),
    # then the other precisions' pools behind the library's own conv1 (maxpool_h8_kernel, maxpool_p_kernel, and
    # maxpool_kernel<float> again for f32x3; maxpool_kernel<_Float16> cannot be reached by a network call: rh.UNREACHABLE)
    for shape in (rp.FIRST, rp.CORNER, rp.SINGLE):
        B, Hp, Wp = rp._pooled_dims(shape)
        for kind, off in rp.SRC_CASES:
            case = ("f32", 6, kind, 0, off, shape, "wide" if kind == 1 else "u8", None)
            net, _ = rh._net(weights, False)
            src, tab, mask, n, _, _ = rh.place_inputs(case, dev)
            runs = [("f32", 6, 1), ("f32", 6, 2), ("f16", 0, 0), ("f32s", 0, 0), ("f32x3", 0, 0)]
            for prec, variant, root_pool in runs:
                rp._set(b"conv1_variant", variant)
                rp._set(b"root_pool", root_pool)
                try:
                    y, rec = rh.run_net(net, prec, kind, 0, src, tab, None, n, B, shape[1], shape[2], 1, B * Hp * Wp * 64)
                finally:
                    rp._set(b"conv1_variant", 0)
                    rp._set(b"root_pool", 0)
                line("pool1-%s-v%d-rp%d-%s%s-%dx%dx%d" % ((prec, variant, root_pool, ("win", "ringf", "ringu")[kind],
                                                           "-off" if off else "") + shape), rec, y)


if __name__ == "__main__":
    main()
