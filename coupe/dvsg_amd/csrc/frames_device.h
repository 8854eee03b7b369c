// Device helpers of the frame-format kernels shared by frames.hip and nv12.hip: the pool-slot rule and the tap rule of
// the cv2-style bilinear resize.  Both translation units are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace dvsg {
namespace {

// A pool slot is a frame index in [0, n_pool); a kernel given slots skips (ingest) or zero-fills (egress) a frame whose
// slot lies outside, so a bad slot never addresses memory outside the pool.
__device__ __forceinline__ bool slot_ok(int s, int n_pool) { return s >= 0 && s < n_pool; }

// cv2.resize(src_float64, (out_w, out_h)) with the default INTER_LINEAR, restated from OpenCV's
// published resize algorithm (OpenCV is not part of the reference tree nor of this image: parity
// unpinned against cv2; held bit for bit by a second restatement and within a derived bound by torch's float64
// bilinear interpolation, tests/test_frames_f64.py; OpenCV's spelling of the scale, 1. / (dw / sw), gives the
// same float32 coordinates as sw / dw for all sizes tried, tests/test_frames_ref_cpu.py):
// pixel centres at (d + 0.5) * scale - 0.5; the fractional weight is computed AND kept
// as float32; taps left of 0 / right of the last column clamp with weight 0; the row pass runs
// first (float64 accumulate), then the column pass.  Input is the uint8 frame (eval.py:80 divides by
// 255. in float64 first), output the float32 TF is fed.
struct ResizeTap {
  int s0, s1;
  float w1;
};
__device__ __forceinline__ ResizeTap resize_tap(int d, double scale, int n_src) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= n_src - 1) {
    s = n_src - 1;
    f = 0.f;
  }
  ResizeTap t;
  t.s0 = s;
  t.s1 = s + 1 < n_src ? s + 1 : n_src - 1;
  t.w1 = f;
  return t;
}

}  // namespace
}  // namespace dvsg
