#!/usr/bin/env python3
"""A/B the conv1 kernel variants inside the full network (class-0 hipEvent timing), five rounds of each in turn:
   python tools/conv1_ab.py [variant ...]     (default: 0 7 -- the library's own choice against the one-row kernel)"""
import ctypes, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from coupe.dvsg_amd import _lib
from coupe.dvsg_amd.networks import LocNet
from coupe.dvsg_amd.weights import make_synthetic_weights

variants = [int(v) for v in sys.argv[1:]] or [0, 7]
dev = torch.device("cuda:0")
B, H, W = 16, 720, 1280
net = LocNet(make_synthetic_weights(0))
x = bench.gpu_windows(B, H, W, 1234, dev)
ref = None
rec = (ctypes.c_int * 9)()
ms_of = {v: [] for v in variants}
for rnd in range(5):
    for v in variants:
        _lib.call("dvsg_debug_set_option", b"conv1_variant", v)
        net.forward(x)
        torch.cuda.synchronize()
        _lib.call("dvsg_prof_begin", 0)
        for _ in range(3):
            F = net.forward(x)
        ms, n, fl, by = ctypes.c_double(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        _lib.call("dvsg_prof_end", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by))
        _lib.call("dvsg_debug_last_root_kernel", rec, 9)
        if ref is None:
            ref = F.clone()
        ms_of[v].append(ms.value / n.value)
        print("round %d conv1_variant=%d (family %d, NW %d, bands %d)  %.3f ms/launch  %.1f TFLOP/s  maxdiff vs first %.2e" %
              (rnd, v, rec[0], rec[1], rec[4], ms.value / n.value, fl.value / ms.value / 1e9, float((F - ref).abs().max())))
for v in variants:
    t = sorted(ms_of[v])
    print("conv1_variant=%d: median %.3f ms, range %.3f .. %.3f" % (v, t[len(t) // 2], t[0], t[-1]))
