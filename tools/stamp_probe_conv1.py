#!/usr/bin/env python3
"""Per-workgroup phase times of the float32 conv1 kernels from a -DDVSG_STAMPS build (see tools/README.md):
   DVSG_AMD_LIB=build/lib_stamps.so [PROBE_REP=20] [PROBE_VARIANT=7] python tools/stamp_probe_conv1.py [B H W]
The stamps are those of the last of PROBE_REP launches (default 3).  PROBE_VARIANT sets conv1_variant: the library's own
choice (0) is root_band_kernel at big launches and conv1_kernel otherwise; 6 / 7 force the one or the other.
PROBE_STAGE=1 taps the root max pool instead of conv1: the band kernel then is root_band_pool_kernel (the pool in its
epilogue) and root_pool_seams_kernel follows it; the stamps are the band kernel's either way."""
import ctypes, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from coupe.dvsg_amd import _lib
from coupe.dvsg_amd.networks import LocNet
from coupe.dvsg_amd.weights import make_synthetic_weights

B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (16, 720, 1280)
dev = torch.device("cuda:0")
net = LocNet(make_synthetic_weights(seed=0))
x = bench.gpu_windows(B, H, W, 1, dev)
lib = _lib.load()
if os.environ.get("PROBE_VARIANT"):
    _lib.call("dvsg_debug_set_option", b"conv1_variant", int(os.environ["PROBE_VARIANT"]))
stage = int(os.environ.get("PROBE_STAGE", "0"))
for _ in range(int(os.environ.get("PROBE_REP", "3"))):
    net.tap(x, stage)   # stops after conv1 (0) or the root max pool (1)
torch.cuda.synchronize()
rec = (ctypes.c_int * 9)()
_lib.call("dvsg_debug_last_root_kernel", rec, 9)
band = rec[0] == 7
Ho, wtiles = (H + 1) // 2, -(-((W + 1) // 2) // 128)
n = min(65536, B * wtiles * (rec[4] if band else Ho))
buf = np.zeros((65536, 8), dtype=np.uint64)
assert lib.dvsg_debug_read_conv1_stamps(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(buf.nbytes)) == 0
st = buf[:n].astype(np.float64)
life, real = st[:, 6], st[:, 7] / 100.0
clk = np.median(life / real)
q = lambda a: "med %8.0f  p10 %8.0f  p90 %8.0f  share of lifetime %.3f" % (
    np.median(a), np.percentile(a, 10), np.percentile(a, 90), np.median(a / life))
if band:
    print("%s B=%d %dx%d: %d bands of <= %d row pairs, %d workgroups sampled, in-kernel clock %.0f MHz" %
          ("root_band_pool_kernel" if rec[6] == 4 else "root_band_kernel", B, W, H, rec[4], rec[5], n, clk))
    names = ["band prologue (index setup)", "barrier 1 (per step: everyone's MFMAs + own loads landed)",
             "scale + LDS stores of the input rows", "barrier 2 (per step and pair)", "load issue", "epilogues (both rows' transposes + stores)",
             "lifetime"]
    rows = 2 * rec[5]
else:
    print("conv1_kernel B=%d %dx%d: %d workgroups sampled, in-kernel clock %.0f MHz" % (B, W, H, n, clk))
    names = ["prologue + first load issue", "barrier 1 (7x: mates' MFMAs + own loads landed)", "scale + LDS stores (7x)", "barrier 2 (7x)",
             "load issue (6x)", "start -> end of MFMA loops", "lifetime"]
    rows = 1
for i, nm in enumerate(names):
    print("%-58s %s" % (nm, q(st[:, i])))
if not band:
    print("%-58s %s" % ("epilogue (lifetime - end of MFMA loops)", q(st[:, 6] - st[:, 5])))
mf = 7 * 148 * 64.0
print("MFMA issue cycles per wave and output row: %.0f alone, %.0f with the wave that shares its SIMD" % (mf, 2 * mf))
print("MFMA share of the lifetime if the pipe were never idle: %.3f (a workgroup of %d output rows per wave slot)" %
      (2 * mf * (rows / 2 if band else 1) / np.median(life), rows))
