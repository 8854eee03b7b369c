// Device functions of the geometric warps shared by warp_kernels.hip and loss_kernels.hip: the three samplers' address /
// weight / blend steps and the thin-plate-spline map.  Both translation units are compiled with -ffp-contract=off (the
// reference graph is a chain of separately rounded float32 ops), and a pixel gets the same bits from either.
#pragma once
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace dvsg {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxPts = 61;  // P + 3 <= 64

// ----------------------------------------------------------------------------------------
// Samplers.
// ----------------------------------------------------------------------------------------
template <int C>
struct Pix {
  float v[C];
};

template <int C>
__device__ __forceinline__ Pix<C> load_pix(const float *__restrict__ p) {
  Pix<C> r;
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] = p[c];
  return r;
}
// a uint8 frame: the pixel as eval.py:80 hands it to the graph, float32(v / 255.) -- the float64 quotient rounded
// once.  A correctly rounded float32 division gives the same value for all 256 bytes (exhaustive:
// tests/test_frames_cpu.py); hipcc's `/` is correctly rounded (no -ffast-math in this build).
template <int C>
__device__ __forceinline__ Pix<C> load_pix(const uint8_t *__restrict__ p) {
  Pix<C> r;
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] = (float)p[c] / 255.0f;
  return r;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Guarded float -> int conversion (floor already applied): out-of-range source coordinates
// are garbage in the reference too (tf.cast saturates to INT_MIN on x86); keep it defined.
__device__ __forceinline__ int f2i(float f) {
  f = f < -1073741824.f ? -1073741824.f : (f > 1073741824.f ? 1073741824.f : f);
  return (int)f;
}

// Sampler A (ThinPlateSpline.py:30-90): normalised (xs, ys) -> (x+1)*W/2, indices clipped to
// the image BEFORE the weights are formed, so out-of-range taps coincide and cancel.
template <int C>
struct TapsA {  // loaded taps (x0,y0) (x0,y1) (x1,y0) (x1,y1) and their weights
  Pix<C> a, b, c, d;
  float wa, wb, wc, wd;
};
template <>
struct TapsA<0> {  // generic channel count: the blend reads through the tap pointers
  const float *pa, *pb, *pc, *pd;
  float wa, wb, wc, wd;
};

// Address + weight computation and the four tap loads; the loads are only ISSUED here, so the
// caller can do other work before sample_a_blend() needs them.
template <int C, typename TU = float>
__device__ __forceinline__ void sample_a_load(const TU *__restrict__ img /* [H,W,C] of this sample */,
                                              int H, int W, int Cn, float xs, float ys, TapsA<C> &t) {
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
  const TU *pa = img + ((size_t)y0 * W + x0) * Cn;  // (x0,y0)
  const TU *pb = img + ((size_t)y1 * W + x0) * Cn;  // (x0,y1)
  const TU *pc = img + ((size_t)y0 * W + x1) * Cn;  // (x1,y0)
  const TU *pd = img + ((size_t)y1 * W + x1) * Cn;  // (x1,y1)
  if constexpr (C > 0) {
    t.a = load_pix<C>(pa);
    t.b = load_pix<C>(pb);
    t.c = load_pix<C>(pc);
    t.d = load_pix<C>(pd);
  } else {
    t.pa = pa; t.pb = pb; t.pc = pc; t.pd = pd;
  }
}

// Does sample_a_load blend four DISTINCT taps at (xs, ys)?  The same float32 coordinate and index expressions in the same
// order; the sample is valid iff neither clip moved an index onto its neighbour, (x1 - x0) (y1 - y0) == 1 after the clip,
// i.e. 0 <= x < W - 1 and 0 <= y < H - 1.  Everywhere else two taps coincide, their weights cancel and the blend is 0 up to
// its own rounding: the black border of a stabilised frame.  NaN is tested on its own (no float -> int conversion decides it) and is
// invalid.  W == 1 or H == 1: no sample is valid.
__device__ __forceinline__ bool sample_a_valid(int H, int W, float xs, float ys) {
  const float x = ((xs + 1.0f) * (float)W) / 2.0f;  // :48
  const float y = ((ys + 1.0f) * (float)H) / 2.0f;  // :49
  if (x != x || y != y) return false;
  int x0 = f2i(floorf(x));
  int y0 = f2i(floorf(y));
  int x1 = x0 + 1;
  int y1 = y0 + 1;
  x0 = clampi(x0, 0, W - 1);  // :57-60
  x1 = clampi(x1, 0, W - 1);
  y0 = clampi(y0, 0, H - 1);
  y1 = clampi(y1, 0, H - 1);
  return (x1 - x0) * (y1 - y0) == 1;
}

template <int C>
__device__ __forceinline__ void sample_a_blend(const TapsA<C> &t, int Cn, float *__restrict__ dst) {
  if constexpr (C > 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = ((t.wa * t.a.v[c] + t.wb * t.b.v[c]) + t.wc * t.c.v[c]) + t.wd * t.d.v[c];  // :89
  } else {
    for (int c = 0; c < Cn; ++c) dst[c] = ((t.wa * t.pa[c] + t.wb * t.pb[c]) + t.wc * t.pc[c]) + t.wd * t.pd[c];
  }
}

// ----------------------------------------------------------------------------------------
// The sample type S of a plane of the source-size renders: uint8_t (RGB, NV12) or uint16_t (P010: a little-endian word whose
// high 10 bits are the sample, s = word >> 6; the low 6 bits are ignored on input and written as 0).  kBias: a chroma plane,
// centred on the neutral value.  One correctly rounded float32 division of the exact integer, as for the bytes; for all
// 1024 values it equals (float)((double)s / 1023.0) (exhaustive on the host: tests/test_p010_cpu.py).
// ----------------------------------------------------------------------------------------
template <typename S>
constexpr int kSampleBytes = (int)sizeof(S);

// the sample `s` (a byte, or a word already shifted down) as the float32 image the filters blend
template <typename S, bool kBias>
__device__ __forceinline__ float sample_f32(int s) {
  if constexpr (kSampleBytes<S> == 1) return kBias ? (float)(s - 128) / 255.0f : (float)s / 255.0f;
  else return kBias ? (float)(s - 512) / 1023.0f : (float)s / 1023.0f;
}

// the same from the plane's memory
template <typename S, bool kBias>
__device__ __forceinline__ float load_sample(const S *__restrict__ p) {
  if constexpr (kSampleBytes<S> == 1) return kBias ? (float)((int)p[0] - 128) / 255.0f : (float)p[0] / 255.0f;
  else return sample_f32<S, kBias>((int)(p[0] >> 6));
}

// a P010 word from a blended value: clamp(floor((double)v * 1023.0 + half), 0, 1023) << 6, half = 0.5 (luma) or 512.5
// (chroma), in both filters; NaN gives 0.  Luma rounds to NEAREST here where the NV12 bilinear render truncates: at 10 bits
// truncation is no round trip (include/dvsg_amd.h, "P010 frames").
__device__ __forceinline__ uint16_t p010_word(float v, double half) {
  const double d = (double)v * 1023.0 + half;
  return (uint16_t)((d >= 1023.0 ? 1023 : (d > 0.0 ? (int)d : 0)) << 6);
}

// ----------------------------------------------------------------------------------------
// The border modes of the source-size renders (a view of dvsg_locnet_view_create_border; the header's "Border modes").  A
// mode decides what an INVALID sample becomes and nothing else: DVSG_BORDER_KEEP does not store it, DVSG_BORDER_REPLICATE
// and DVSG_BORDER_MIRROR evaluate the handle's filter at the coordinate moved into the plane.  The kernels with a border
// are instantiations of their own (kBorder != 0); DVSG_BORDER_BLACK is the kernels that were there before.
// ----------------------------------------------------------------------------------------
// x (sampler A's pixel coordinate, not NaN) moved into [0, m], m = (float)(pw - 1): one reflection about the edge it left
// by (MIRROR), then the clamp.  A coordinate already inside keeps its value.
template <int kBorder>
__device__ __forceinline__ float border_coord(float x, float m) {
  if constexpr (kBorder == DVSG_BORDER_MIRROR) x = x < 0.0f ? -x : (x > m ? (m + m) - x : x);
  return fminf(fmaxf(x, 0.0f), m);
}

// sample_a_load for a plane of samples S (ph x pw samples of C, rows `pitch` bytes apart; kBias: chroma, sample_f32's) under a
// border mode.  The taps are x0 = floor(xc) and min(x0 + 1, pw - 1), the upper weight from the UNclipped index -- sampler
// A's clipped weights would cancel on the edge -- so a valid sample (xc == x, no index clipped) gets sampler A's taps and
// weights, bit for bit, and one set of four loads serves valid and invalid samples without a divergent branch.  `use`: the
// blend is the sample's value -- KEEP: the sample is valid (else nothing is stored); REPLICATE / MIRROR: the coordinate is
// no NaN (else the black value).  Every address lies inside the plane's used bytes.
template <int C, bool kBias, int kBorder, typename S = uint8_t>
__device__ __forceinline__ void border_a_load(const uint8_t *__restrict__ img, size_t pitch, int ph, int pw, float xs, float ys,
                                              TapsA<C> &t, bool &use) {
  const float x = ((xs + 1.0f) * (float)pw) / 2.0f;  // :48
  const float y = ((ys + 1.0f) * (float)ph) / 2.0f;  // :49
  const bool nan = x != x || y != y;
  use = kBorder == DVSG_BORDER_KEEP ? sample_a_valid(ph, pw, xs, ys) : !nan;
  const float xc = nan ? 0.0f : border_coord<kBorder>(x, (float)(pw - 1));
  const float yc = nan ? 0.0f : border_coord<kBorder>(y, (float)(ph - 1));
  const float x0f = floorf(xc), y0f = floorf(yc);
  const int x0 = min((int)x0f, pw - 1), y0 = min((int)y0f, ph - 1);   // (in range already wherever (float)(pw - 1) is exact)
  const int x1 = min(x0 + 1, pw - 1), y1 = min(y0 + 1, ph - 1);
  const float wx0 = (x0f + 1.0f) - xc, wx1 = xc - x0f, wy0 = (y0f + 1.0f) - yc, wy1 = yc - y0f;
  t.wa = wx0 * wy0;  // :85-88
  t.wb = wx0 * wy1;
  t.wc = wx1 * wy0;
  t.wd = wx1 * wy1;
  constexpr size_t kStep = (size_t)C * kSampleBytes<S>;   // bytes from one sample to the next
  const S *pa = reinterpret_cast<const S *>(img + (size_t)y0 * pitch + (size_t)x0 * kStep);  // (x0,y0)
  const S *pb = reinterpret_cast<const S *>(img + (size_t)y1 * pitch + (size_t)x0 * kStep);  // (x0,y1)
  const S *pc = reinterpret_cast<const S *>(img + (size_t)y0 * pitch + (size_t)x1 * kStep);  // (x1,y0)
  const S *pd = reinterpret_cast<const S *>(img + (size_t)y1 * pitch + (size_t)x1 * kStep);  // (x1,y1)
#pragma unroll
  for (int c = 0; c < C; ++c) {
    t.a.v[c] = load_sample<S, kBias>(pa + c);
    t.b.v[c] = load_sample<S, kBias>(pb + c);
    t.c.v[c] = load_sample<S, kBias>(pc + c);
    t.d.v[c] = load_sample<S, kBias>(pd + c);
  }
}

// ----------------------------------------------------------------------------------------
// The bicubic filter of the source-size renders (a view with DVSG_RENDER_BICUBIC): sampler A's coordinates and validity,
// OpenCV's INTER_CUBIC weights (A = -0.75), 4 x 4 taps with edge-replicated indices, rows blended first.  Every operation
// is a separately rounded float32 one in the order the header states; tests/bicubic_ref.py restates it in NumPy.
// A plane is ph x pw samples of C bytes whose rows are `pitch` bytes apart.
//
// Tap fetch: the 4 taps of a row are 4 C contiguous bytes, so a row is ONE load of C dwords at byte granularity (gfx950
// serves a global load at any alignment) instead of 4 C byte loads: 16 loads of 4 / 8 / 12 bytes per thread and 4 rows, C
// packed registers each -- 64 taps in flight in 16 C VGPRs.  The window starts at column clamp(x0 - 1, 0, pw - 4), so it
// lies wholly inside the row's pw C used bytes wherever the row has 4 samples; at the two edges (x0 = 0, x0 = pw - 2: the
// window is one column off the taps) the replicated taps are picked out of it in registers (CubicTaps::d).  A plane with
// pw < 4 has no such window and takes one byte load per tap component, column indices clamped: the same packed layout.
// No load touches a byte outside the row's pw C used bytes.  A plane of 16-bit samples (S = uint16_t) is the same with
// words for bytes: a row of the window is 8 C contiguous bytes, one load of 2 C dwords, two samples to a register.  DVSG_CUBIC_BYTE_TAPS (a build switch for the A/B of DESIGN
// 5.bicubic, never set in the product) sends every plane down the byte path.
// ----------------------------------------------------------------------------------------
template <int C, typename S = uint8_t>
struct CubicTaps {
  uint32_t raw[4][C * kSampleBytes<S>];   // row r: sample k C + c (a byte or a 16-bit word) = component c of window column k
  float wx[4], wy[4];
  int d;                // taps' first column minus the window's: -1, 0 or 1 (2 too under a border mode: x0 = pw - 1)
  bool valid;           // the blend is the sample's value (else 0.0f); under a border mode: border_a_load's `use`
};

// w[k] for the taps at floor(x) - 1 + k, t = x - floor(x)
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
  const float u = t + 1.0f;
  w[0] = ((-0.75f * u - -3.75f) * u + -6.0f) * u - -3.0f;   // ((A u - 5A) u + 8A) u - 4A
  w[1] = ((1.25f * t - 2.25f) * t) * t + 1.0f;               // ((A + 2) t - (A + 3)) t t + 1
  const float v = 1.0f - t;
  w[2] = ((1.25f * v - 2.25f) * v) * v + 1.0f;
  w[3] = ((1.0f - w[0]) - w[1]) - w[2];
}

// C dwords from any byte address (C <= 4)
template <int C>
__device__ __forceinline__ void load_bytes_x4(const uint8_t *__restrict__ p, uint32_t (&raw)[C]) {
  if constexpr (C == 1) {
    typedef uint32_t u32_a1 __attribute__((aligned(1)));
    raw[0] = *reinterpret_cast<const u32_a1 *>(p);
  } else {
    typedef uint32_t u32xc __attribute__((ext_vector_type(C)));
    typedef u32xc u32xc_a1 __attribute__((aligned(1)));
    const u32xc v = *reinterpret_cast<const u32xc_a1 *>(p);
#pragma unroll
    for (int c = 0; c < C; ++c) raw[c] = v[c];
  }
}

// Coordinates, validity, weights, and the 4 row loads (only ISSUED here, like sample_a_load).  kWide: pw >= 4.
// kBorder: steps 3-5 at the coordinate moved into the plane (border_coord; a NaN loads from (0, 0) and blends to 0.0f).
template <int C, bool kWide, int kBorder = DVSG_BORDER_BLACK, typename S = uint8_t>
__device__ __forceinline__ void cubic_load(const uint8_t *__restrict__ img, size_t pitch, int ph, int pw, float xs, float ys,
                                           CubicTaps<C, S> &t) {
  constexpr int kB = kSampleBytes<S>, kPer = 4 / kB;   // bytes of a sample, samples to a dword
  float x = ((xs + 1.0f) * (float)pw) / 2.0f;  // sampler A's (:48-49)
  float y = ((ys + 1.0f) * (float)ph) / 2.0f;
  t.valid = sample_a_valid(ph, pw, xs, ys);
  int x0, y0;
  if constexpr (kBorder == DVSG_BORDER_BLACK) {
    // a valid sample has 0 <= x0 <= pw - 2 and 0 <= y0 <= ph - 2; an invalid one stores 0 and only needs addresses inside the plane
    x0 = t.valid ? f2i(floorf(x)) : 0, y0 = t.valid ? f2i(floorf(y)) : 0;
  } else {
    const bool nan = x != x || y != y;
    if constexpr (kBorder != DVSG_BORDER_KEEP) t.valid = !nan;
    x = nan ? 0.0f : border_coord<kBorder>(x, (float)(pw - 1));
    y = nan ? 0.0f : border_coord<kBorder>(y, (float)(ph - 1));
    x0 = min((int)floorf(x), pw - 1), y0 = min((int)floorf(y), ph - 1);   // 0 <= x0 <= pw - 1
  }
  cubic_weights(x - (float)x0, t.wx);   // x - x0 is exact
  cubic_weights(y - (float)y0, t.wy);
  if constexpr (kWide) {
    const int xw = clampi(x0 - 1, 0, pw - 4);
    t.d = x0 - 1 - xw;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      load_bytes_x4<C * kB>(img + (size_t)clampi(y0 - 1 + r, 0, ph - 1) * pitch + (size_t)xw * (C * kB), t.raw[r]);
    return;
  }
  t.d = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint8_t *row = img + (size_t)clampi(y0 - 1 + r, 0, ph - 1) * pitch;
#pragma unroll
    for (int c = 0; c < C * kB; ++c) t.raw[r][c] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const S *p = reinterpret_cast<const S *>(row + (size_t)clampi(x0 - 1 + k, 0, pw - 1) * (C * kB));
#pragma unroll
      for (int c = 0; c < C; ++c) t.raw[r][(k * C + c) / kPer] |= (uint32_t)p[c] << (8 * kB * ((k * C + c) % kPer));
    }
  }
}

// cubic_load for the rows i0 .. i0 + n_rows - 1 (n_rows <= 4) of one output column: every load of the thread in flight
// together.  Which path a plane takes is decided once, outside the rows (a load under a per-row branch is waited for there).
template <int C, int kBorder = DVSG_BORDER_BLACK, typename S = uint8_t>
__device__ __forceinline__ void cubic_load_rows(const uint8_t *__restrict__ img, size_t pitch, int ph, int pw, int n_rows,
                                                const float (&xs)[4], const float (&ys)[4], CubicTaps<C, S> (&ct)[4]) {
#ifndef DVSG_CUBIC_BYTE_TAPS
  if (pw >= 4) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r >= n_rows) break;
      cubic_load<C, true, kBorder, S>(img, pitch, ph, pw, xs[r], ys[r], ct[r]);
    }
    return;
  }
#endif
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r >= n_rows) break;
    cubic_load<C, false, kBorder, S>(img, pitch, ph, pw, xs[r], ys[r], ct[r]);
  }
}

// v[c] of one pixel; kBias: the chroma plane's samples (sample_f32).  An invalid pixel is exactly 0.
// kBorder: the window may be two columns off the taps (x0 = pw - 1: the taps are columns pw - 2, pw - 1, pw - 1, pw - 1).
template <int C, bool kBias, int kBorder = DVSG_BORDER_BLACK, typename S = uint8_t>
__device__ __forceinline__ void cubic_blend(const CubicTaps<C, S> &t, float (&v)[C]) {
  constexpr int kB = kSampleBytes<S>, kPer = 4 / kB;
  float h[4][C];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float p[4][C];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t raw = t.raw[r][(k * C + c) / kPer] >> (8 * kB * ((k * C + c) % kPer));
        p[k][c] = sample_f32<S, kBias>(kB == 1 ? (int)(raw & 0xffu) : (int)((raw & 0xffffu) >> 6));
      }
    }
    if (t.d != 0) {   // the window is one column off the taps: edge replicate
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float a = p[0][c], b = p[1][c], e = p[2][c], f = p[3][c];
        if constexpr (kBorder != DVSG_BORDER_BLACK) {
          p[0][c] = t.d < 0 ? a : (t.d == 2 ? e : b);
          p[1][c] = t.d < 0 ? a : (t.d == 2 ? f : e);
        } else {
          p[0][c] = t.d < 0 ? a : b;
          p[1][c] = t.d < 0 ? a : e;
        }
        p[2][c] = t.d < 0 ? b : f;
        p[3][c] = t.d < 0 ? e : f;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) h[r][c] = ((t.wx[0] * p[0][c] + t.wx[1] * p[1][c]) + t.wx[2] * p[2][c]) + t.wx[3] * p[3][c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float s = ((t.wy[0] * h[0][c] + t.wy[1] * h[1][c]) + t.wy[2] * h[2][c]) + t.wy[3] * h[3][c];
    v[c] = t.valid ? s : 0.0f;
  }
}

// the bicubic render's bytes round to nearest: clamp(floor((double)v * 255.0 + bias + 0.5), 0, 255), bias 0 (RGB, luma) or
// 128 (chroma); NaN gives 0
__device__ __forceinline__ uint8_t cubic_u8(float v, double half) {
  const double d = (double)v * 255.0 + half;
  return d >= 255.0 ? (uint8_t)255 : (d > 0.0 ? (uint8_t)(int)d : (uint8_t)0);
}

// Samplers B and C share this tail (spatial_transformer.py:517-562,
// warp_with_optical_flow.py:128-173): (x, y) in unpadded pixel units, clamped to [-1,W] /
// [-1,H], +1 into the zero-ringed image, floor, upper index min()-ed, weights from the
// UNclamped x0+1.  The ring is never materialised: a tap on it reads as 0.
template <int C>
struct TapsB {  // loaded taps (x0,y0) (x1,y0) (x0,y1) (x1,y1), weights, and which taps are on the ring
  Pix<C> a, b, c, d;
  float w00, w01, w10, w11;
  bool v00, v01, v10, v11;
};
template <>
struct TapsB<0> {  // generic channel count: the blend reads through the tap pointers
  const float *p00, *p01, *p10, *p11;
  float w00, w01, w10, w11;
  bool v00, v01, v10, v11;
};

// Address / weight computation and the four tap loads (only ISSUED here, so a thread can put the taps
// of several pixels in flight before it blends the first one).  A tap on the ring reads as 0: the
// loads are unconditional, from indices clamped into the image, and the ring is applied in the blend
// as a select -- a predicated load that feeds arithmetic makes the compiler wait for each load in turn.
// weights, ring flags and the (clamped) tap coordinates of one sample; shared by the image samplers and the mask plane
struct PadGeom {
  float w00, w01, w10, w11;
  bool v00, v01, v10, v11;
  int xa, xb, ya, yb;   // tap coordinates clamped into the image (what an unconditional global load may touch)
  int x0, y0;           // the lower tap in the zero-ringed image's coordinates (image pixel x0 - 1, y0 - 1), in [0, W + 1] / [0, H + 1]
};
__device__ __forceinline__ PadGeom padded_geom(int H, int W, float x, float y) {
  PadGeom g;
  const float wf = (float)W, hf = (float)H;
  x = fminf(fmaxf(x, -1.0f), wf);  // (W-1)+1
  y = fminf(fmaxf(y, -1.0f), hf);
  x = x + 1.0f;
  y = y + 1.0f;
  const float x0f = floorf(x), y0f = floorf(y);
  const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const int x1 = (int)fminf(x1f, wf + 1.0f);
  const int y1 = (int)fminf(y1f, hf + 1.0f);
  g.w00 = (x1f - x) * (y1f - y);
  g.w01 = (x - x0f) * (y1f - y);
  g.w10 = (x1f - x) * (y - y0f);
  g.w11 = (x - x0f) * (y - y0f);
  const bool vx0 = x0 >= 1 && x0 <= W, vx1 = x1 >= 1 && x1 <= W;
  const bool vy0 = y0 >= 1 && y0 <= H, vy1 = y1 >= 1 && y1 <= H;
  g.v00 = vx0 && vy0; g.v01 = vx1 && vy0; g.v10 = vx0 && vy1; g.v11 = vx1 && vy1;
  g.xa = clampi(x0 - 1, 0, W - 1); g.xb = clampi(x1 - 1, 0, W - 1);
  g.ya = clampi(y0 - 1, 0, H - 1); g.yb = clampi(y1 - 1, 0, H - 1);
  g.x0 = x0; g.y0 = y0;
  return g;
}

template <int C>
__device__ __forceinline__ void sample_padded_load_geom(const float *__restrict__ img, int W, int Cn, const PadGeom &g,
                                                        TapsB<C> &t);

template <int C>
__device__ __forceinline__ void sample_padded_load(const float *__restrict__ img, int H, int W, int Cn, float x,
                                                   float y, TapsB<C> &t) {
  sample_padded_load_geom<C>(img, W, Cn, padded_geom(H, W, x, y), t);
}

// the same from a geometry the caller already holds: several images sampled at one position (loss_kernels.hip's temporal
// term blends a frame and a mask plane with one set of taps and weights)
template <int C>
__device__ __forceinline__ void sample_padded_load_geom(const float *__restrict__ img, int W, int Cn, const PadGeom &g,
                                                        TapsB<C> &t) {
  t.w00 = g.w00; t.w01 = g.w01; t.w10 = g.w10; t.w11 = g.w11;
  t.v00 = g.v00; t.v01 = g.v01; t.v10 = g.v10; t.v11 = g.v11;
  const float *p00 = img + ((long)g.ya * W + g.xa) * Cn;
  const float *p01 = img + ((long)g.ya * W + g.xb) * Cn;
  const float *p10 = img + ((long)g.yb * W + g.xa) * Cn;
  const float *p11 = img + ((long)g.yb * W + g.xb) * Cn;
  if constexpr (C > 0) {
    t.a = load_pix<C>(p00);
    t.b = load_pix<C>(p01);
    t.c = load_pix<C>(p10);
    t.d = load_pix<C>(p11);
  } else {
    t.p00 = p00; t.p01 = p01; t.p10 = p10; t.p11 = p11;
  }
}

template <int C>
__device__ __forceinline__ void sample_padded_blend(const TapsB<C> &t, int Cn, float *__restrict__ dst) {
  if constexpr (C > 0) {
#pragma unroll
    for (int c = 0; c < C; ++c)
      dst[c] = ((t.w00 * (t.v00 ? t.a.v[c] : 0.f) + t.w01 * (t.v01 ? t.b.v[c] : 0.f)) + t.w10 * (t.v10 ? t.c.v[c] : 0.f)) +
               t.w11 * (t.v11 ? t.d.v[c] : 0.f);
  } else {
    for (int c = 0; c < Cn; ++c) {
      const float a = t.v00 ? t.p00[c] : 0.f;
      const float bq = t.v01 ? t.p01[c] : 0.f;
      const float cq = t.v10 ? t.p10[c] : 0.f;
      const float d = t.v11 ? t.p11[c] : 0.f;
      dst[c] = ((t.w00 * a + t.w01 * bq) + t.w10 * cq) + t.w11 * d;
    }
  }
}

template <int C>
__device__ __forceinline__ void store_pix(float *__restrict__ out, size_t pix, int Cn,
                                          const float *__restrict__ v) {
  if constexpr (C == 3) {
    // one 12-byte store per lane (global_store_dwordx3 needs only 4-byte alignment): a wave writes
    // 768 contiguous bytes with one instruction instead of three stride-12 dword stores
    typedef float floatx3 __attribute__((ext_vector_type(3)));
    typedef floatx3 floatx3_a4 __attribute__((aligned(4)));
    *reinterpret_cast<floatx3_a4 *>(out + pix * 3) = floatx3{v[0], v[1], v[2]};
  } else if constexpr (C > 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[pix * C + c] = v[c];
  } else {
    for (int c = 0; c < Cn; ++c) out[pix * Cn + c] = v[c];
  }
}

constexpr int kMaxGenericC = 64;

// ----------------------------------------------------------------------------------------
// The thin-plate-spline map of one output column and kTpsRows consecutive rows (ThinPlateSpline.py:92-129), shared by
// tps_warp_kernel and the loss kernels: every caller gets the same bits for the same pixel.
// ----------------------------------------------------------------------------------------
typedef float floatx2 __attribute__((ext_vector_type(2)));

constexpr int kTpsRows = 4;
constexpr float kLn2 = 0x1.62e43p-1f;

// Thread t < P stages control point t as {px, py, T[0][3+t] ln 2, T[1][3+t] ln 2} and -- kRowTerms -- (y_t[r] - py)^2 of the
// rows i0 .. i0 + 3; threads 64 .. 69 stage the affine part T[0][0..2], T[1][0..2].  The caller's barrier follows.
// kZoom: the output grid scaled about its centre, y_t' = z y_t (one more float32 multiply; z == 1.0f gives y_t's bits).
template <bool kRowTerms, bool kZoom = false>
__device__ __forceinline__ void tps_stage(const float *coord, long coord_bstride, const float *T,
                                          int b, int P, int t, int i0, float step_y, float4 *sp, float4 *sdy, float *sa,
                                          float z = 1.0f) {
  const int n = P + 3;
  if (t < P) {
    const float px = coord[b * coord_bstride + t * 2], py = coord[b * coord_bstride + t * 2 + 1];
    sp[t] = make_float4(px, py, T[((size_t)b * 2) * n + 3 + t] * kLn2, T[((size_t)b * 2 + 1) * n + 3 + t] * kLn2);
    if constexpr (kRowTerms) {
      float dy2[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float y_t = -1.0f + step_y * (float)(i0 + r);
        if constexpr (kZoom) y_t = z * y_t;
        const float dy = y_t - py;  // :96
        dy2[r] = dy * dy;
      }
      sdy[t] = make_float4(dy2[0], dy2[1], dy2[2], dy2[3]);
    }
  } else if (t >= 64 && t < 70) {
    const int q = t - 64;
    sa[q] = T[((size_t)b * 2 + q / 3) * n + q % 3];
  }
}

// One control point's basis term for column x_t and four rows -- c = {px, py, T0 ln 2, T1 ln 2}, q = (y_t[r] - py)^2 --
// added to xs2 / ys2 (:104-105, :129).  The packed form and its operation order are what every caller's bits rest on.
__device__ __forceinline__ void tps_basis_point(const float4 c, const float4 q, float x_t, floatx2 (&xs2)[2], floatx2 (&ys2)[2]) {
  const float dx = x_t - c.x;
  const float dx2 = dx * dx;
  const floatx2 dxx = {dx2, dx2};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const floatx2 dyy = h == 0 ? floatx2{q.x, q.y} : floatx2{q.z, q.w};
    const floatx2 d2 = dxx + dyy;                        // :104
    const floatx2 e = d2 + floatx2{1e-6f, 1e-6f};
    const floatx2 l2 = {__builtin_amdgcn_logf(e.x), __builtin_amdgcn_logf(e.y)};
    const floatx2 rk = d2 * l2;                          // :105 up to the factor ln 2 carried by c.z / c.w
    xs2[h] = __builtin_elementwise_fma(floatx2{c.z, c.z}, rk, xs2[h]);
    ys2[h] = __builtin_elementwise_fma(floatx2{c.w, c.w}, rk, ys2[h]);
  }
}

// (x_s, y_s) of column x_t, rows i0 .. i0 + 3.  kRowTerms: (y_t - py)^2 comes from sdy (the rows are the workgroup's);
// otherwise it is formed here from sp[k].y by the same two operations (a thread with rows of its own: the SURF gather).
// kZoom: x_t is the caller's zoomed column z x_t already; the rows are scaled here, y_t' = z y_t, as tps_stage scales them.
template <bool kRowTerms, bool kZoom = false>
__device__ __forceinline__ void tps_map_rows(const float4 *sp, const float4 *sdy, const float *sa, int P, float x_t,
                                             float step_y, int i0, float (&xs)[4], float (&ys)[4], float z = 1.0f) {
  floatx2 xs2[2], ys2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // T . [1, x_t, y_t, ...] accumulated in k order (:129)
    floatx2 yy = {-1.0f + step_y * (float)(i0 + 2 * h), -1.0f + step_y * (float)(i0 + 2 * h + 1)};
    if constexpr (kZoom) yy = z * yy;
    const float ax = sa[0] + sa[1] * x_t, ay = sa[3] + sa[4] * x_t;
    xs2[h] = floatx2{ax, ax} + sa[2] * yy;
    ys2[h] = floatx2{ay, ay} + sa[5] * yy;
  }
  for (int k = 0; k < P; ++k) {
    const float4 c = sp[k];
    float4 q;
    if constexpr (kRowTerms) {
      q = sdy[k];
    } else {
      float dy2[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float y_t = -1.0f + step_y * (float)(i0 + r);
        if constexpr (kZoom) y_t = z * y_t;
        const float dy = y_t - c.y;  // :96
        dy2[r] = dy * dy;
      }
      q = make_float4(dy2[0], dy2[1], dy2[2], dy2[3]);
    }
    tps_basis_point(c, q, x_t, xs2, ys2);
  }
  xs[0] = xs2[0].x; xs[1] = xs2[0].y; xs[2] = xs2[1].x; xs[3] = xs2[1].y;
  ys[0] = ys2[0].x; ys[1] = ys2[0].y; ys[2] = ys2[1].x; ys[3] = ys2[1].y;
}

inline float lin_step(int n) { return n > 1 ? (1.0f - (-1.0f)) / (float)(n - 1) : 0.0f; }

// launch(kZoom, kCubic, kBorder) with the three as compile-time constants: the instantiation of a border render kernel that
// a handle's filter and border (REPLICATE, MIRROR or KEEP; the entry point has checked it) and the presence of zoom select
template <typename F>
inline void for_render_border(bool zoom, bool cubic, int border, F &&launch) {
  auto with_border = [&](auto kBorder) {
    if (zoom && cubic) launch(std::true_type(), std::true_type(), kBorder);
    else if (zoom) launch(std::true_type(), std::false_type(), kBorder);
    else if (cubic) launch(std::false_type(), std::true_type(), kBorder);
    else launch(std::false_type(), std::false_type(), kBorder);
  };
  switch (border) {
    case DVSG_BORDER_REPLICATE: with_border(std::integral_constant<int, DVSG_BORDER_REPLICATE>()); break;
    case DVSG_BORDER_MIRROR: with_border(std::integral_constant<int, DVSG_BORDER_MIRROR>()); break;
    default: with_border(std::integral_constant<int, DVSG_BORDER_KEEP>()); break;
  }
}

}  // namespace
}  // namespace dvsg
