// The area filter of the renders at a delivery size (a view of dvsg_locnet_view_create_scaled; include/dvsg_amd.h, "Output
// size"), shared by warp_kernels.hip (uint8 RGB) and nv12.hip (NV12 and P010 planes).  An output sample is the row-major
// float32 average of sy x sx VIRTUAL samples, each of them the view's filter and border at the map of dvsg_tps_warp_zoom_f32
// on the virtual grid.  Both translation units are compiled with -ffp-contract=off: every operation rounds on its own.
//
// Work split: a workgroup owns kThreads output columns and kTpsRows virtual rows, i.e. scaled_rows_per_group(sy) = 4 / sy
// whole output rows (4, 2, 1, 1: sy = 3 computes four virtual rows and uses three), so ONE tps_stage serves all the rows a
// thread evaluates and tps_map_rows is called once per virtual column.  A thread owns one output column: it evaluates the map
// of its sx virtual columns (4 rows each, registers xs[q][r]), then walks the virtual rows; per virtual row the taps of all
// sx virtual samples (4 sx loads for sampler A, 4 sx row loads for the cubic) are issued before the first blend.  sx and sy
// are runtime arguments -- every loop is unrolled to 4 with a uniform guard, so the arrays keep compile-time indices and
// live in registers -- and the kernels are instantiated per filter, border and sample type only.
#pragma once
#include "warp_device.h"

namespace dvsg {
namespace {

// max(1, ceil(src / out)): the supersampling factor of one axis
inline int scaled_factor(int src, int out) { return src > out ? (src + out - 1) / out : 1; }
// whole output rows in the kTpsRows virtual rows of a workgroup
__host__ __device__ inline int scaled_rows_per_group(int sy) { return sy == 1 ? 4 : (sy == 2 ? 2 : 1); }

// A plane's sample as the float32 image dvsg_tps_warp_f32 would be given.  Luma / RGB: (float)((double)Y / 255.0); chroma
// (C == 2): (float)(((double)c - 128.0) / 255.0).  One correctly rounded float32 division of the exact integer gives the
// same value for every byte (exhaustive on the host: tests/test_nv12_cpu.py; the luma case is load_pix<C>(const uint8_t *)'s).
// S = uint16_t: a P010 plane, the 10-bit rule of warp_device.h's sample_f32.
template <int C, typename S = uint8_t>
__device__ __forceinline__ Pix<C> load_plane(const S *__restrict__ p) {
  Pix<C> r;
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] = load_sample<S, C == 2>(p + c);
  return r;
}

// sample_a_load on a plane whose rows are `pitch` bytes apart: its coordinate, index and weight expressions in its order,
// C samples of type S per pixel.  The indices are clipped into the plane, so every tap address lies inside it.
template <int C, typename S = uint8_t>
__device__ __forceinline__ void plane_a_load(const uint8_t *__restrict__ img, size_t pitch, int H, int W, float xs, float ys,
                                             TapsA<C> &t) {
  const float x = ((xs + 1.0f) * (float)W) / 2.0f;  // :48
  const float y = ((ys + 1.0f) * (float)H) / 2.0f;  // :49
  int x0 = f2i(floorf(x));
  int y0 = f2i(floorf(y));
  int x1 = x0 + 1;
  int y1 = y0 + 1;
  x0 = clampi(x0, 0, W - 1);  // :57-60
  x1 = clampi(x1, 0, W - 1);
  y0 = clampi(y0, 0, H - 1);
  y1 = clampi(y1, 0, H - 1);
  const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
  t.wa = (x1f - x) * (y1f - y);  // :85-88
  t.wb = (x1f - x) * (y - y0f);
  t.wc = (x - x0f) * (y1f - y);
  t.wd = (x - x0f) * (y - y0f);
  constexpr int kStep = C * kSampleBytes<S>;   // bytes from one sample to the next
  t.a = load_plane<C, S>(reinterpret_cast<const S *>(img + (size_t)y0 * pitch + x0 * kStep));  // (x0,y0)
  t.b = load_plane<C, S>(reinterpret_cast<const S *>(img + (size_t)y1 * pitch + x0 * kStep));  // (x0,y1)
  t.c = load_plane<C, S>(reinterpret_cast<const S *>(img + (size_t)y0 * pitch + x1 * kStep));  // (x1,y0)
  t.d = load_plane<C, S>(reinterpret_cast<const S *>(img + (size_t)y1 * pitch + x1 * kStep));  // (x1,y1)
}

// The map of one output column's virtual samples: xs[q][r], ys[q][r] of virtual column sx j + q (q < sx) and virtual rows
// i0v .. i0v + 3, the bits of tps_warp_zoom_kernel on a grid with these steps (z = 1.0f where the call has no zoom: the plain
// kernel's bits).  sp / sdy / sa: tps_stage<true, true> at i0v, behind the caller's barrier.
__device__ __forceinline__ void scaled_map(const float4 *sp, const float4 *sdy, const float *sa, int P, int j, int sx,
                                           float step_x, float step_y, int i0v, float z, float (&xs)[4][4], float (&ys)[4][4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int r = 0; r < 4; ++r) xs[q][r] = ys[q][r] = 0.0f;
    if (q < sx) {
      const float x_t = z * (-1.0f + step_x * (float)(sx * j + q));  // tf.linspace: start + step * i (:94), zoomed
      tps_map_rows<true, true>(sp, sdy, sa, P, x_t, step_y, i0v, xs[q], ys[q], z);
    }
  }
}

// The averages of one output column: n_v = (output rows of this workgroup) sy virtual rows (<= 4) of a plane of ph x pw pixels
// of C samples of type S (rows `pitch` bytes apart; kBias = chroma is C == 2, as in render_plane).  store(io, v) receives
// output row io (0-based within the workgroup) and its C averaged float32 values, before any byte rule.
// kBorder: DVSG_BORDER_BLACK, _REPLICATE or _MIRROR (KEEP at another size is refused by the entry points).
template <int C, bool kCubic, int kBorder, typename S, typename Store>
__device__ __forceinline__ void scaled_average(const uint8_t *__restrict__ src, size_t pitch, int ph, int pw, int sx, int sy,
                                               int n_v, const float (&xs)[4][4], const float (&ys)[4][4], Store &&store) {
  static_assert(kBorder != DVSG_BORDER_KEEP, "DVSG_BORDER_KEEP has no scaled render");
  const float count = (float)(sx * sy);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
  int p = 0, io = 0;   // the virtual row within its output row; the output row
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r >= n_v) break;
    float v[4][C];
    if constexpr (kCubic) {
      CubicTaps<C, S> ct[4];
      // which path a plane takes is decided outside the columns, and DVSG_CUBIC_BYTE_TAPS sends every plane down the byte
      // path, as in cubic_load_rows
#ifndef DVSG_CUBIC_BYTE_TAPS
      const bool wide = pw >= 4;
#else
      const bool wide = false;
#endif
      if (wide) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < sx) cubic_load<C, true, kBorder, S>(src, pitch, ph, pw, xs[q][r], ys[q][r], ct[q]);   // 4 sx row loads in flight
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < sx) cubic_load<C, false, kBorder, S>(src, pitch, ph, pw, xs[q][r], ys[q][r], ct[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < sx) cubic_blend<C, C == 2, kBorder, S>(ct[q], v[q]);
    } else {
      TapsA<C> taps[4];
      [[maybe_unused]] bool use[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < sx) {   // 4 sx tap loads in flight
          if constexpr (kBorder != DVSG_BORDER_BLACK)
            border_a_load<C, C == 2, kBorder, S>(src, pitch, ph, pw, xs[q][r], ys[q][r], taps[q], use[q]);
          else
            plane_a_load<C, S>(src, pitch, ph, pw, xs[q][r], ys[q][r], taps[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < sx) {
          sample_a_blend<C>(taps[q], C, v[q]);
          if constexpr (kBorder != DVSG_BORDER_BLACK) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[q][c] = use[q] ? v[q][c] : 0.0f;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < sx) {
        const bool first = p == 0 && q == 0;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = first ? v[q][c] : acc[c] + v[q][c];
      }
    }
    if (++p == sy) {
      float o[C];
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = acc[c] / count;
      store(io, o);
      p = 0;
      ++io;
    }
  }
}

}  // namespace
}  // namespace dvsg
