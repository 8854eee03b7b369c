// NV12 as a frame format of its own (include/dvsg_amd.h, "NV12 frames"): what a hardware decoder hands over and an
// encoder takes -- a full-size Y plane and a half-size interleaved UV plane, rows `pitch` bytes apart.
//
//   nv12_to_rgb_kernel      Y, UV -> packed RGB / BGR uint8.  Integer arithmetic with shift 20 (OpenCV's published
//                           COLOR_YUV2RGB_NV12 scheme; OpenCV is not part of this image: parity with cv2 unpinned, as for
//                           the resize), chroma of luma pixel (i, j) = sample (i / 2, j / 2), no interpolation.  Exact.
//   ingest_nv12_kernel      that conversion followed by frames_u8_to_f32_kernel's (float)(double(v) / 255.0), into pool
//   ingest_nv12_resize_kernel  slots; and followed by resize_u8_kernel's float64 bilinear: each output pixel converts its
//                           (at most four) taps in registers, the source-size RGB image never exists.
//   nv12_render_kernel      both planes warped by one normalised TPS map with sampler A, each at its own size: luma as a
//                           1-channel image (H, W), chroma as a 2-channel image (H/2, W/2) centred on 128, so that sampler
//                           A's black border is luma 0, chroma 128 (neutral) and not a green edge.  One launch renders both
//                           planes of every frame: blockIdx.x runs over the luma tiles, then the chroma tiles.
//   nv12_render_zoom_kernel that render on the output grid scaled about its centre by zoom[frame] (the crop of a live
//                           stream): tps_stage / tps_map_rows with kZoom, x_t' = z x_t.  A kernel of its own, so that
//                           nv12_render_kernel keeps its instructions.
//   nv12_render_cubic_kernel  both of the above through a bicubic view (dvsg_locnet_view_create): the same tiles and map, the
//                           4 x 4-tap filter of warp_device.h behind it, bytes rounded to nearest.
//   Every render kernel takes the chroma plane's rows as an argument, ch (the scaled one: och for the output too), worked out
//   on the host with the tile counts and lin_step: H / 2 for a 4:2:0 handle, H for a DVSG_CHROMA_422 view ("Chroma sampling").
//   nv12_render_scaled_kernel  the render through a scaled view (dvsg_locnet_view_create_scaled): output planes of another size,
//                           each sample the float32 average of sy x sx samples of that map and filter (scaled_device.h), for
//                           NV12 and P010, both filters, the black, replicate and mirror borders.
//
// Every kernel is bit-identical to a composition of pinned entry points (stated at each); this translation unit is compiled
// with -ffp-contract=off like frames.hip and warp_kernels.hip.  The map comes from tps_stage / tps_map_rows and the blend from
// sample_a_blend (warp_device.h); only the tap ADDRESSES are formed here, because a plane's rows are `pitch` bytes apart.
#include <cstdint>

#include "frames_device.h"
#include "scaled_device.h"
#include "warp_device.h"

namespace dvsg {
namespace {

// int(round(c * 2**20)) of the matrix's decimals; row = DVSG_YUV_*
struct YuvCoef {
  int cy, cvr, cvg, cug, cub;
};
constexpr YuvCoef kYuv[2] = {
    {1220542, 1673527, -852492, -409993, 2116026},   // BT.601 limited: 1.164, 1.596, -0.813, -0.391, 2.018 (OpenCV's)
    {1220945, 1879825, -558796, -223608, 2215014},   // BT.709 limited: 1.164384, 1.792741, -0.532909, -0.213249, 2.112402
};

struct Rgb {
  int c[3];   // R, G, B in [0, 255]
};

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// int32 throughout: |sum| < 2^30; >> on a negative int is arithmetic
__device__ __forceinline__ Rgb yuv_to_rgb(int Y, int U, int V, const YuvCoef k) {
  const int y = max(0, Y - 16) * k.cy, u = U - 128, v = V - 128;
  Rgb o;
  o.c[0] = sat8((y + k.cvr * v + (1 << 19)) >> 20);
  o.c[1] = sat8((y + k.cvg * v + k.cug * u + (1 << 19)) >> 20);
  o.c[2] = sat8((y + k.cub * u + (1 << 19)) >> 20);
  return o;
}

// the planes of a batch of frames
struct Nv12 {
  const uint8_t *y, *uv;
  size_t pitch, frame_stride;
};

// 4 consecutive bytes of a row: one dword load where the address allows, byte loads otherwise; `n` (2 or 4) are valid
__device__ __forceinline__ uint32_t load4(const uint8_t *p, int n) {
  if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
  uint32_t w = 0;
  for (int i = 0; i < n; ++i) w |= (uint32_t)p[i] << (8 * i);
  return w;
}

// One thread converts a block of 2 rows x 4 columns (8 luma bytes, 2 UV pairs in; 24 bytes out); the last block of a row
// holds 2 columns when W % 4 == 2.  blockIdx.y is the frame.
__global__ __launch_bounds__(kThreads) void nv12_to_rgb_kernel(Nv12 s, int H, int W, YuvCoef k, int flip,
                                                               uint8_t *__restrict__ dst) {
  const size_t f = blockIdx.y;
  const uint8_t *yp = s.y + f * s.frame_stride, *uvp = s.uv + f * s.frame_stride;
  const int per_row = (W + 3) / 4;
  const size_t nblocks = (size_t)(H / 2) * per_row;
  for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < nblocks; g += (size_t)gridDim.x * kThreads) {
    const int bi = (int)(g / per_row);
    const int j0 = 4 * (int)(g - (size_t)bi * per_row);
    const int ncol = W - j0 < 4 ? W - j0 : 4;
    const uint32_t cw = load4(uvp + (size_t)bi * s.pitch + j0, ncol);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = 2 * bi + r;
      const uint32_t yw = load4(yp + (size_t)i * s.pitch + j0, ncol);
      uint8_t o[12];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int sh = 16 * (q >> 1);
        const Rgb p = yuv_to_rgb((yw >> (8 * q)) & 255, (cw >> sh) & 255, (cw >> (sh + 8)) & 255, k);
        o[3 * q] = (uint8_t)p.c[flip ? 2 : 0];
        o[3 * q + 1] = (uint8_t)p.c[1];
        o[3 * q + 2] = (uint8_t)p.c[flip ? 0 : 2];
      }
      uint8_t *d = dst + ((f * H + i) * W + j0) * 3;
      if (ncol == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
        uint32_t *d4 = reinterpret_cast<uint32_t *>(d);
#pragma unroll
        for (int w = 0; w < 3; ++w)
          d4[w] = (uint32_t)o[4 * w] | ((uint32_t)o[4 * w + 1] << 8) | ((uint32_t)o[4 * w + 2] << 16) | ((uint32_t)o[4 * w + 3] << 24);
      } else {
        for (int e = 0; e < 3 * ncol; ++e) d[e] = o[e];
      }
    }
  }
}

// Same size: one thread converts 4 consecutive pixels of a row (4 luma bytes, 2 UV pairs in; 48 bytes out), the values of
// frames_u8_to_f32_kernel on the converted bytes.  Frame blockIdx.y goes to pool frame slots[blockIdx.y].
__global__ __launch_bounds__(kThreads) void ingest_nv12_kernel(Nv12 s, int H, int W, YuvCoef k, float *__restrict__ pool,
                                                               const int *__restrict__ slots, int n_pool) {
  const size_t f = blockIdx.y;
  const int sl = slots[f];
  if (!slot_ok(sl, n_pool)) return;
  const uint8_t *yp = s.y + f * s.frame_stride, *uvp = s.uv + f * s.frame_stride;
  float *dst = pool + (size_t)sl * H * W * 3;
  const int per_row = (W + 3) / 4;
  const size_t ngroups = (size_t)H * per_row;
  for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * kThreads) {
    const int i = (int)(g / per_row);
    const int j0 = 4 * (int)(g - (size_t)i * per_row);
    const int ncol = W - j0 < 4 ? W - j0 : 4;
    const uint32_t yw = load4(yp + (size_t)i * s.pitch + j0, ncol);
    const uint32_t cw = load4(uvp + (size_t)(i >> 1) * s.pitch + j0, ncol);
    float v[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int sh = 16 * (q >> 1);
      const Rgb p = yuv_to_rgb((yw >> (8 * q)) & 255, (cw >> sh) & 255, (cw >> (sh + 8)) & 255, k);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * q + c] = (float)((double)p.c[c] / 255.0);
    }
    float *d = dst + ((size_t)i * W + j0) * 3;
    if (ncol == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
      float4 *d4 = reinterpret_cast<float4 *>(d);
      d4[0] = make_float4(v[0], v[1], v[2], v[3]);
      d4[1] = make_float4(v[4], v[5], v[6], v[7]);
      d4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
      for (int e = 0; e < 3 * ncol; ++e) d[e] = v[e];
    }
  }
}

// RGB of luma pixel (i, j) of a frame
__device__ __forceinline__ Rgb nv12_pixel(const uint8_t *yp, const uint8_t *uvp, size_t pitch, int i, int j, const YuvCoef k) {
  const uint8_t *c = uvp + (size_t)(i >> 1) * pitch + (j & ~1);
  return yuv_to_rgb(yp[(size_t)i * pitch + j], c[0], c[1], k);
}

// resize_u8_kernel (flip = 0, no uint8 half) on the converted frame: the same tap rule, the same float64 operations in the
// same order; the four taps are converted here instead of read from an RGB image.
__global__ __launch_bounds__(kThreads) void ingest_nv12_resize_kernel(Nv12 s, int n, int sh, int sw, YuvCoef k,
                                                                      float *__restrict__ dst, int dh, int dw,
                                                                      const int *__restrict__ slots, int n_pool) {
  const double scale_x = (double)sw / dw, scale_y = (double)sh / dh;
  const size_t total = (size_t)n * dh * dw;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const int dx = (int)(e % dw);
    const size_t t = e / dw;
    const int dy = (int)(t % dh);
    const size_t f = t / dh;
    const int sl = slots[f];
    if (!slot_ok(sl, n_pool)) continue;
    const size_t de = ((size_t)sl * dh + dy) * dw + dx;
    const ResizeTap tx = resize_tap(dx, scale_x, sw), ty = resize_tap(dy, scale_y, sh);
    const uint8_t *yp = s.y + f * s.frame_stride, *uvp = s.uv + f * s.frame_stride;
    const Rgb q00 = nv12_pixel(yp, uvp, s.pitch, ty.s0, tx.s0, k), q01 = nv12_pixel(yp, uvp, s.pitch, ty.s0, tx.s1, k);
    const Rgb q10 = nv12_pixel(yp, uvp, s.pitch, ty.s1, tx.s0, k), q11 = nv12_pixel(yp, uvp, s.pitch, ty.s1, tx.s1, k);
    const double a1 = (double)tx.w1, a0 = (double)(1.f - tx.w1);
    const double b1 = (double)ty.w1, b0 = (double)(1.f - ty.w1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p00 = (double)q00.c[c] / 255.0, p01 = (double)q01.c[c] / 255.0;
      const double p10 = (double)q10.c[c] / 255.0, p11 = (double)q11.c[c] / 255.0;
      const double h0 = __dadd_rn(__dmul_rn(p00, a0), __dmul_rn(p01, a1));
      const double h1 = __dadd_rn(__dmul_rn(p10, a0), __dmul_rn(p11, a1));
      const double v = __dadd_rn(__dmul_rn(h0, b0), __dmul_rn(h1, b1));
      dst[de * 3 + c] = (float)v;
    }
  }
}

// ----------------------------------------------------------------------------------------
// Render.
// ----------------------------------------------------------------------------------------
// load_plane / plane_a_load -- a plane's samples as the float32 image dvsg_tps_warp_f32 would be given, and sample_a_load on
// a plane whose rows are `pitch` bytes apart -- are scaled_device.h's: the scaled kernels of warp_kernels.hip use them too.

// chroma back to a byte: clamp(floor((double)v * 255.0 + 128.5), 0, 255); NaN gives 0 like to_u8
__device__ __forceinline__ uint8_t chroma_u8(float v) {
  const double d = (double)v * 255.0 + 128.5;
  return d >= 255.0 ? (uint8_t)255 : (d > 0.0 ? (uint8_t)(int)d : (uint8_t)0);
}

// The C P010 words of one output pixel at d (2-byte aligned): luma one 16-bit store, chroma one dword store where d allows.
template <int C>
__device__ __forceinline__ void store_words(uint8_t *__restrict__ d, const float (&v)[C]) {
  if constexpr (C == 1) {
    *reinterpret_cast<uint16_t *>(d) = p010_word(v[0], 0.5);
  } else {
    const uint16_t u = p010_word(v[0], 512.5), w = p010_word(v[1], 512.5);
    if ((reinterpret_cast<uintptr_t>(d) & 3) == 0) {
      *reinterpret_cast<uint32_t *>(d) = (uint32_t)u | ((uint32_t)w << 16);
    } else {
      reinterpret_cast<uint16_t *>(d)[0] = u;
      reinterpret_cast<uint16_t *>(d)[1] = w;
    }
  }
}

// One output column and kTpsRows rows of one plane (ph x pw pixels of C samples of type S), source and output of the same size.
// kCubic (a bicubic view): the bicubic filter of warp_device.h behind the same map, bytes rounded to nearest.
// kBorder (a view with a border mode): what an invalid sample becomes (warp_device.h, "border modes").
// S = uint16_t (a P010 view): the samples and the words of warp_device.h's sample_f32 / p010_word in both filters; the
// planes' addresses are 2-byte aligned (tps_render_nv12_check).
template <int C, bool kCubic = false, int kBorder = DVSG_BORDER_BLACK, typename S = uint8_t>
__device__ __forceinline__ void render_plane(const uint8_t *__restrict__ src, size_t pitch, int ph, int pw, int i0, int j,
                                             const float (&xs)[4], const float (&ys)[4], uint8_t *__restrict__ out,
                                             size_t out_pitch) {
  if constexpr (kCubic) {
    CubicTaps<C, S> ct[4];
    cubic_load_rows<C, kBorder, S>(src, pitch, ph, pw, ph - i0, xs, ys, ct);  // all 16 row loads in flight
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + r;
      if (i >= ph) break;
      if constexpr (kBorder == DVSG_BORDER_KEEP) {
        if (!ct[r].valid) continue;   // the caller's bytes stay
      }
      float v[C];
      cubic_blend<C, C == 2, kBorder, S>(ct[r], v);
      uint8_t *d = out + (size_t)i * out_pitch + (size_t)j * (C * kSampleBytes<S>);
      if constexpr (kSampleBytes<S> == 2) {
        store_words<C>(d, v);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = cubic_u8(v[c], C == 2 ? 128.5 : 0.5);
      }
    }
    return;
  }
  TapsA<C> taps[4];
  [[maybe_unused]] bool use[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (i0 + r >= ph) break;
    if constexpr (kBorder != DVSG_BORDER_BLACK)
      border_a_load<C, C == 2, kBorder, S>(src, pitch, ph, pw, xs[r], ys[r], taps[r], use[r]);
    else
      plane_a_load<C, S>(src, pitch, ph, pw, xs[r], ys[r], taps[r]);  // all 16 tap loads in flight
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + r;
    if (i >= ph) break;
    if constexpr (kBorder == DVSG_BORDER_KEEP) {
      if (!use[r]) continue;   // the caller's bytes stay
    }
    float v[C];
    sample_a_blend<C>(taps[r], C, v);
    if constexpr (kBorder != DVSG_BORDER_BLACK) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = use[r] ? v[c] : 0.0f;
    }
    uint8_t *d = out + (size_t)i * out_pitch + (size_t)j * (C * kSampleBytes<S>);
    if constexpr (kSampleBytes<S> == 2) {
      store_words<C>(d, v);
    } else if constexpr (C == 1) {
      d[0] = to_u8((double)v[0]);
    } else {
      const uint8_t u = chroma_u8(v[0]), w = chroma_u8(v[1]);
      if ((reinterpret_cast<uintptr_t>(d) & 1) == 0) {
        *reinterpret_cast<uint16_t *>(d) = (uint16_t)((uint16_t)u | ((uint16_t)w << 8));
      } else {
        d[0] = u;
        d[1] = w;
      }
    }
  }
}

// blockIdx.y: the frame.  blockIdx.x: the luma tiles (kThreads columns x kTpsRows rows, row-major, gx_l per row group), then
// from n_l on the chroma tiles (gx_c per row group).  A tile's map is dvsg_tps_warp_f32's on a grid of the plane's size.
__global__ __launch_bounds__(kThreads) void nv12_render_kernel(Nv12 s, const float *__restrict__ coord,
                                                               const float *__restrict__ T, int H, int W, int P,
                                                               float sx_l, float sy_l, float sx_c, float sy_c, int gx_l,
                                                               int n_l, int gx_c, int ch, uint8_t *__restrict__ out_y,
                                                               uint8_t *__restrict__ out_uv, size_t out_pitch,
                                                               size_t out_frame_stride) {
  __shared__ float4 sp[64];
  __shared__ float4 sdy[64];
  __shared__ float sa[6];
  const int b = blockIdx.y, t = threadIdx.x;
  int id = blockIdx.x;
  const bool chroma = id >= n_l;
  if (chroma) id -= n_l;
  const int gx = chroma ? gx_c : gx_l;
  const int i0 = (id / gx) * kTpsRows;
  const int ph = chroma ? ch : H, pw = chroma ? W / 2 : W;
  const float step_x = chroma ? sx_c : sx_l, step_y = chroma ? sy_c : sy_l;
  tps_stage<true>(coord, 0, T, b, P, t, i0, step_y, sp, sdy, sa);
  __syncthreads();
  const int j = (id % gx) * kThreads + t;
  if (j >= pw) return;
  const float x_t = -1.0f + step_x * (float)j;  // tf.linspace: start + step * i (:94)
  float xs[4], ys[4];
  tps_map_rows<true>(sp, sdy, sa, P, x_t, step_y, i0, xs, ys);
  const size_t in_off = (size_t)b * s.frame_stride, out_off = (size_t)b * out_frame_stride;
  if (chroma)
    render_plane<2>(s.uv + in_off, s.pitch, ph, pw, i0, j, xs, ys, out_uv + out_off, out_pitch);
  else
    render_plane<1>(s.y + in_off, s.pitch, ph, pw, i0, j, xs, ys, out_y + out_off, out_pitch);
}

// nv12_render_kernel on the zoomed grid: each plane is dvsg_tps_warp_zoom_f32 on it, bit for bit (tps_warp_zoom_kernel's
// z = zoom[b], y_t' = z y_t in the staging and the row terms, x_t' = z x_t here).
__global__ __launch_bounds__(kThreads) void nv12_render_zoom_kernel(Nv12 s, const float *__restrict__ coord,
                                                                    const float *__restrict__ T,
                                                                    const float *__restrict__ zoom, int H, int W, int P,
                                                                    float sx_l, float sy_l, float sx_c, float sy_c,
                                                                    int gx_l, int n_l, int gx_c, int ch, uint8_t *__restrict__ out_y,
                                                                    uint8_t *__restrict__ out_uv, size_t out_pitch,
                                                                    size_t out_frame_stride) {
  __shared__ float4 sp[64];
  __shared__ float4 sdy[64];
  __shared__ float sa[6];
  const int b = blockIdx.y, t = threadIdx.x;
  int id = blockIdx.x;
  const bool chroma = id >= n_l;
  if (chroma) id -= n_l;
  const int gx = chroma ? gx_c : gx_l;
  const int i0 = (id / gx) * kTpsRows;
  const int ph = chroma ? ch : H, pw = chroma ? W / 2 : W;
  const float step_x = chroma ? sx_c : sx_l, step_y = chroma ? sy_c : sy_l;
  const float z = zoom[b];
  tps_stage<true, true>(coord, 0, T, b, P, t, i0, step_y, sp, sdy, sa, z);
  __syncthreads();
  const int j = (id % gx) * kThreads + t;
  if (j >= pw) return;
  const float x_t = z * (-1.0f + step_x * (float)j);
  float xs[4], ys[4];
  tps_map_rows<true, true>(sp, sdy, sa, P, x_t, step_y, i0, xs, ys, z);
  const size_t in_off = (size_t)b * s.frame_stride, out_off = (size_t)b * out_frame_stride;
  if (chroma)
    render_plane<2>(s.uv + in_off, s.pitch, ph, pw, i0, j, xs, ys, out_uv + out_off, out_pitch);
  else
    render_plane<1>(s.y + in_off, s.pitch, ph, pw, i0, j, xs, ys, out_y + out_off, out_pitch);
}

// One tile of one plane of a frame for the kernels that are templates: nv12_render_kernel's tiles and map (kZoom: those of
// nv12_render_zoom_kernel; zoom is read by that form only), render_plane<C, kCubic, kBorder, S> behind the map.
template <typename S, bool kZoom, bool kCubic, int kBorder>
__device__ __forceinline__ void render_tile(const Nv12 &s, const float *__restrict__ coord, const float *__restrict__ T,
                                            const float *__restrict__ zoom, int H, int W, int P, float sx_l, float sy_l,
                                            float sx_c, float sy_c, int gx_l, int n_l, int gx_c, int ch, uint8_t *__restrict__ out_y,
                                            uint8_t *__restrict__ out_uv, size_t out_pitch, size_t out_frame_stride) {
  __shared__ float4 sp[64];
  __shared__ float4 sdy[64];
  __shared__ float sa[6];
  const int b = blockIdx.y, t = threadIdx.x;
  int id = blockIdx.x;
  const bool chroma = id >= n_l;
  if (chroma) id -= n_l;
  const int gx = chroma ? gx_c : gx_l;
  const int i0 = (id / gx) * kTpsRows;
  const int ph = chroma ? ch : H, pw = chroma ? W / 2 : W;
  const float step_x = chroma ? sx_c : sx_l, step_y = chroma ? sy_c : sy_l;
  float z = 1.0f;
  if constexpr (kZoom) z = zoom[b];
  tps_stage<true, kZoom>(coord, 0, T, b, P, t, i0, step_y, sp, sdy, sa, z);
  __syncthreads();
  const int j = (id % gx) * kThreads + t;
  if (j >= pw) return;
  float x_t = -1.0f + step_x * (float)j;  // tf.linspace: start + step * i (:94)
  if constexpr (kZoom) x_t = z * x_t;
  float xs[4], ys[4];
  tps_map_rows<true, kZoom>(sp, sdy, sa, P, x_t, step_y, i0, xs, ys, z);
  const size_t in_off = (size_t)b * s.frame_stride, out_off = (size_t)b * out_frame_stride;
  if (chroma)
    render_plane<2, kCubic, kBorder, S>(s.uv + in_off, s.pitch, ph, pw, i0, j, xs, ys, out_uv + out_off, out_pitch);
  else
    render_plane<1, kCubic, kBorder, S>(s.y + in_off, s.pitch, ph, pw, i0, j, xs, ys, out_y + out_off, out_pitch);
}

// The NV12 render through a bicubic view: render_tile with the bicubic filter.  A kernel of its own: the two above stay
// the instructions they were.
template <bool kZoom>
__global__ __launch_bounds__(kThreads) void nv12_render_cubic_kernel(Nv12 s, const float *__restrict__ coord,
                                                                     const float *__restrict__ T,
                                                                     const float *__restrict__ zoom, int H, int W, int P,
                                                                     float sx_l, float sy_l, float sx_c, float sy_c,
                                                                     int gx_l, int n_l, int gx_c, int ch, uint8_t *__restrict__ out_y,
                                                                     uint8_t *__restrict__ out_uv, size_t out_pitch,
                                                                     size_t out_frame_stride) {
  render_tile<uint8_t, kZoom, true, DVSG_BORDER_BLACK>(s, coord, T, zoom, H, W, P, sx_l, sy_l, sx_c, sy_c, gx_l, n_l, gx_c, ch, out_y,
                                                       out_uv, out_pitch, out_frame_stride);
}

// The NV12 render through a view with a border mode (dvsg_locnet_view_create_border; kBorder = DVSG_BORDER_REPLICATE,
// _MIRROR or _KEEP), for either filter: render_tile with the border mode.  Kernels of their own again: a handle with
// DVSG_BORDER_BLACK launches the three kernels above.
template <bool kZoom, bool kCubic, int kBorder>
__global__ __launch_bounds__(kThreads) void nv12_render_border_kernel(Nv12 s, const float *__restrict__ coord,
                                                                      const float *__restrict__ T,
                                                                      const float *__restrict__ zoom, int H, int W, int P,
                                                                      float sx_l, float sy_l, float sx_c, float sy_c,
                                                                      int gx_l, int n_l, int gx_c, int ch, uint8_t *__restrict__ out_y,
                                                                      uint8_t *__restrict__ out_uv, size_t out_pitch,
                                                                      size_t out_frame_stride) {
  static_assert(kBorder != DVSG_BORDER_BLACK, "DVSG_BORDER_BLACK is the kernels without a border parameter");
  render_tile<uint8_t, kZoom, kCubic, kBorder>(s, coord, T, zoom, H, W, P, sx_l, sy_l, sx_c, sy_c, gx_l, n_l, gx_c, ch, out_y, out_uv,
                                               out_pitch, out_frame_stride);
}

// The render through a P010 view (dvsg_locnet_view_create_surface): the planes are 16-bit words (include/dvsg_amd.h, "P010
// frames"), pitch and frame strides still in bytes, for every filter, border and zoom: render_tile with S = uint16_t.
// Kernels of their own: a handle without the property launches the 8-bit kernels above, whose instructions stay.
template <bool kZoom, bool kCubic, int kBorder>
__global__ __launch_bounds__(kThreads) void p010_render_kernel(Nv12 s, const float *__restrict__ coord,
                                                               const float *__restrict__ T, const float *__restrict__ zoom,
                                                               int H, int W, int P, float sx_l, float sy_l, float sx_c,
                                                               float sy_c, int gx_l, int n_l, int gx_c, int ch,
                                                               uint8_t *__restrict__ out_y, uint8_t *__restrict__ out_uv,
                                                               size_t out_pitch, size_t out_frame_stride) {
  render_tile<uint16_t, kZoom, kCubic, kBorder>(s, coord, T, zoom, H, W, P, sx_l, sy_l, sx_c, sy_c, gx_l, n_l, gx_c, ch, out_y, out_uv,
                                                out_pitch, out_frame_stride);
}

// One output pixel's C samples at d from its float32 values: render_plane's output rules (bilinear luma truncates, chroma
// rounds at 128.5, the bicubic bytes and the P010 words round to nearest).
template <int C, bool kCubic, typename S>
__device__ __forceinline__ void store_sample(uint8_t *__restrict__ d, const float (&v)[C]) {
  if constexpr (kSampleBytes<S> == 2) {
    store_words<C>(d, v);
  } else if constexpr (kCubic) {
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = cubic_u8(v[c], C == 2 ? 128.5 : 0.5);
  } else if constexpr (C == 1) {
    d[0] = to_u8((double)v[0]);
  } else {
    const uint8_t u = chroma_u8(v[0]), w = chroma_u8(v[1]);
    if ((reinterpret_cast<uintptr_t>(d) & 1) == 0) {
      *reinterpret_cast<uint16_t *>(d) = (uint16_t)((uint16_t)u | ((uint16_t)w << 8));
    } else {
      d[0] = u;
      d[1] = w;
    }
  }
}

// The render through a scaled view (dvsg_locnet_view_create_scaled; include/dvsg_amd.h, "Output size"): planes of (H, W) /
// (H / 2, W / 2) in, (oh, ow) / (oh / 2, ow / 2) out, each output sample the float32 average of sy x sx virtual samples
// (scaled_device.h).  blockIdx.y: the frame.  blockIdx.x: the luma tiles (kThreads output columns x 4 / sy output rows,
// row-major, gx_l per row group), then from n_l on the chroma tiles.  step_*: lin_step of the planes' VIRTUAL grids.  zoom may
// be NULL (z = 1.0f).  Kernels of their own: a handle without the property launches the kernels above.
template <typename S, bool kCubic, int kBorder>
__global__ __launch_bounds__(kThreads) void nv12_render_scaled_kernel(Nv12 s, const float *__restrict__ coord,
                                                                      const float *__restrict__ T,
                                                                      const float *__restrict__ zoom, int H, int W, int P,
                                                                      int oh, int ow, int sx, int sy, float sx_l, float sy_l,
                                                                      float sx_c, float sy_c, int gx_l, int n_l, int gx_c, int ch, int och,
                                                                      uint8_t *__restrict__ out_y, uint8_t *__restrict__ out_uv,
                                                                      size_t out_pitch, size_t out_frame_stride) {
  __shared__ float4 sp[64];
  __shared__ float4 sdy[64];
  __shared__ float sa[6];
  const int b = blockIdx.y, t = threadIdx.x;
  int id = blockIdx.x;
  const bool chroma = id >= n_l;
  if (chroma) id -= n_l;
  const int gx = chroma ? gx_c : gx_l;
  const int rows = scaled_rows_per_group(sy);
  const int io0 = (id / gx) * rows, i0v = io0 * sy;   // the first output row and its first virtual row
  const int ph = chroma ? ch : H, pw = chroma ? W / 2 : W;
  const int po = chroma ? och : oh, qo = chroma ? ow / 2 : ow;
  const float step_x = chroma ? sx_c : sx_l, step_y = chroma ? sy_c : sy_l;
  const float z = zoom ? zoom[b] : 1.0f;
  tps_stage<true, true>(coord, 0, T, b, P, t, i0v, step_y, sp, sdy, sa, z);
  __syncthreads();
  const int j = (id % gx) * kThreads + t;
  if (j >= qo) return;
  float xs[4][4], ys[4][4];
  scaled_map(sp, sdy, sa, P, j, sx, step_x, step_y, i0v, z, xs, ys);
  const int n_v = min(rows, po - io0) * sy;
  const size_t in_off = (size_t)b * s.frame_stride, out_off = (size_t)b * out_frame_stride;
  if (chroma) {
    uint8_t *const d0 = out_uv + out_off + (size_t)io0 * out_pitch + (size_t)j * (2 * kSampleBytes<S>);
    scaled_average<2, kCubic, kBorder, S>(s.uv + in_off, s.pitch, ph, pw, sx, sy, n_v, xs, ys, [&](int io, const float (&v)[2]) {
      store_sample<2, kCubic, S>(d0 + (size_t)io * out_pitch, v);
    });
  } else {
    uint8_t *const d0 = out_y + out_off + (size_t)io0 * out_pitch + (size_t)j * kSampleBytes<S>;
    scaled_average<1, kCubic, kBorder, S>(s.y + in_off, s.pitch, ph, pw, sx, sy, n_v, xs, ys, [&](int io, const float (&v)[1]) {
      store_sample<1, kCubic, S>(d0 + (size_t)io * out_pitch, v);
    });
  }
}

inline int grid_for(size_t items, int cap = 1 << 16) {
  const size_t b = (items + kThreads - 1) / kThreads;
  return (int)(b < (size_t)cap ? (b ? b : 1) : (size_t)cap);
}

// the layout of a batch of NV12 frames (see the header)
int check_nv12(const char *fn, const char *what, const void *y, const void *uv, size_t pitch, size_t frame_stride, int n, int H,
               int W) {
  DVSG_REQUIRE(y && uv, "%s: NULL %s plane", fn, what);
  DVSG_REQUIRE(n >= 1 && n <= 65535, "%s: n=%d outside [1, 65535]", fn, n);
  DVSG_REQUIRE(H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "%s: NV12 frames are even-sized and at least 4x4, got H=%d W=%d",
               fn, H, W);
  DVSG_REQUIRE((long)H * W < (1L << 31), "%s: frame %dx%d too large", fn, H, W);
  DVSG_REQUIRE(pitch >= (size_t)W, "%s: %s pitch=%zu < W=%d", fn, what, pitch, W);
  DVSG_REQUIRE(n == 1 || frame_stride >= (size_t)H * pitch, "%s: %s frame_stride=%zu < H * pitch = %zu", fn, what, frame_stride,
               (size_t)H * pitch);
  return DVSG_OK;
}

// what P010 frames ask on top of check_nv12: W samples are 2 W bytes of a row, and every address is a word's
int check_p010(const char *fn, const char *what, const void *y, const void *uv, size_t pitch, size_t frame_stride, int n, int W) {
  DVSG_REQUIRE(pitch >= 2 * (size_t)W, "%s: %s pitch=%zu < 2 W = %zu (P010: 2 bytes per sample)", fn, what, pitch, 2 * (size_t)W);
  DVSG_REQUIRE(pitch % 2 == 0, "%s: %s pitch=%zu is odd (P010 words are 2-byte aligned)", fn, what, pitch);
  DVSG_REQUIRE(n == 1 || frame_stride % 2 == 0, "%s: %s frame_stride=%zu is odd (P010 words are 2-byte aligned)", fn, what,
               frame_stride);
  DVSG_REQUIRE(reinterpret_cast<uintptr_t>(y) % 2 == 0, "%s: %s y plane pointer is not 2-byte aligned", fn, what);
  DVSG_REQUIRE(reinterpret_cast<uintptr_t>(uv) % 2 == 0, "%s: %s uv plane pointer is not 2-byte aligned", fn, what);
  return DVSG_OK;
}

int check_matrix(const char *fn, int matrix) {
  DVSG_REQUIRE(matrix == DVSG_YUV_BT601_LIMITED || matrix == DVSG_YUV_BT709_LIMITED,
               "%s: matrix=%d is neither DVSG_YUV_BT601_LIMITED (0) nor DVSG_YUV_BT709_LIMITED (1)", fn, matrix);
  return DVSG_OK;
}

}  // namespace

int tps_render_nv12_check(const char *fn, const float *F_t, const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride,
                          int n, int H, int W, const float *T, const uint8_t *out_y, const uint8_t *out_uv, size_t out_pitch,
                          size_t out_frame_stride, int out_H, int out_W) {
  DVSG_REQUIRE(F_t && T, "%s: NULL pointer", fn);
  if (int rc = check_nv12(fn, "source", y, uv, pitch, frame_stride, n, H, W)) return rc;
  if (out_H == 0 && out_W == 0) out_H = H, out_W = W;
  if (out_H != H || out_W != W) {   // a scaled view: the output planes are those of an (out_H, out_W) frame
    DVSG_REQUIRE(out_H >= 4 && out_H % 2 == 0, "%s: out_H=%d of the scaled view is odd or below 4 (NV12 / P010 output)", fn, out_H);
    DVSG_REQUIRE(out_W >= 4 && out_W % 2 == 0, "%s: out_W=%d of the scaled view is odd or below 4 (NV12 / P010 output)", fn, out_W);
  }
  return check_nv12(fn, "output", out_y, out_uv, out_pitch, out_frame_stride, n, out_H, out_W);
}

int tps_render_p010_check(const char *fn, const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int W,
                          const uint8_t *out_y, const uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, int out_W) {
  if (int rc = check_p010(fn, "source", y, uv, pitch, frame_stride, n, W)) return rc;
  return check_p010(fn, "output", out_y, out_uv, out_pitch, out_frame_stride, n, out_W ? out_W : W);
}

// What a scaled view asks of a render of (H, W) frames at (out_H, out_W) != (H, W), before any device work: at most 4 virtual
// samples per axis, and no DVSG_BORDER_KEEP (the caller's bytes have no counterpart at another size).
int render_scaled_check(const char *fn, int H, int W, int out_H, int out_W, int render_border) {
  const int sy = scaled_factor(H, out_H), sx = scaled_factor(W, out_W);
  DVSG_REQUIRE(sy <= 4, "%s: out_H=%d of the scaled view is a %dx minification of src_H=%d; more than 4x is not served", fn, out_H,
               sy, H);
  DVSG_REQUIRE(sx <= 4, "%s: out_W=%d of the scaled view is a %dx minification of src_W=%d; more than 4x is not served", fn, out_W,
               sx, W);
  DVSG_REQUIRE(render_border != DVSG_BORDER_KEEP,
               "%s: render_border=DVSG_BORDER_KEEP on a scaled view whose size %dx%d differs from the source's %dx%d", fn, out_H,
               out_W, H, W);
  return DVSG_OK;
}

// the arguments have passed tps_render_nv12_check (and, for DVSG_SURFACE_P010, tps_render_p010_check)
int tps_render_nv12_impl(const char *fn, const double *winv_cols, const float *coord, const float *F_t, const float *zoom,
                         const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int H, int W, int P, float *T,
                         uint8_t *out_y, uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, void *stream,
                         const RenderView &view) {
  const int render_border = view.border, out_H = view.out_h, out_W = view.out_w;
  const bool cubic = view.filter == DVSG_RENDER_BICUBIC, p010 = view.surface_format == DVSG_SURFACE_P010;
  // the chroma plane's rows ("Chroma sampling"): H / 2 of a 4:2:0 frame, H of a 4:2:2 one; its columns are W / 2 in both
  const bool c422 = view.chroma_format == DVSG_CHROMA_422;
  const int ch = c422 ? H : H / 2;
  // the planes' samples per luma sample, 1 + the chroma share (1 / 2, or 1 for 4:2:2), times the bytes of a sample
  const double bytes = (c422 ? 2.0 : 1.5) * (p010 ? 2.0 : 1.0);
  if ((out_H || out_W) && (out_H != H || out_W != W)) {   // a scaled view at another size: kernels of their own
    if (int rc = render_scaled_check(fn, H, W, out_H, out_W, render_border)) return rc;
    const int sy = scaled_factor(H, out_H), sx = scaled_factor(W, out_W), rows = scaled_rows_per_group(sy);
    const int gx_l = ceil_div(out_W, kThreads), gx_c = ceil_div(out_W / 2, kThreads);
    const int och = c422 ? out_H : out_H / 2;
    const long n_l = (long)gx_l * ceil_div(out_H, rows), n_c = (long)gx_c * ceil_div(och, rows);
    DVSG_REQUIRE(n_l + n_c < (1L << 31), "%s: frame %dx%d too large", fn, out_H, out_W);
    if (int rc = tps_apply_impl(winv_cols, coord, F_t, 1, n, P, T, stream, view.shape)) return rc;
    hipStream_t s = as_stream(stream);
    // algorithmic bytes: the source planes once in, the output planes once out
    ProfScope prof(kClsTpsWarp, s, 0.0, bytes * n * ((double)H * W + (double)out_H * out_W));
    const dim3 grid((unsigned)(n_l + n_c), n);
    auto launch = [&](auto kS, auto kCubic, auto kBorder) {
      hipLaunchKernelGGL((nv12_render_scaled_kernel<decltype(kS), kCubic(), kBorder()>), grid, dim3(kThreads), 0, s,
                         Nv12{y, uv, pitch, frame_stride}, coord, T, zoom, H, W, P, out_H, out_W, sx, sy, lin_step(sx * out_W),
                         lin_step(sy * out_H), lin_step(sx * (out_W / 2)), lin_step(sy * och), gx_l, (int)n_l, gx_c, ch, och,
                         out_y, out_uv, out_pitch, out_frame_stride);
    };
    auto with_border = [&](auto kS, auto kCubic) {
      if (render_border == DVSG_BORDER_REPLICATE) launch(kS, kCubic, std::integral_constant<int, DVSG_BORDER_REPLICATE>());
      else if (render_border == DVSG_BORDER_MIRROR) launch(kS, kCubic, std::integral_constant<int, DVSG_BORDER_MIRROR>());
      else launch(kS, kCubic, std::integral_constant<int, DVSG_BORDER_BLACK>());
    };
    auto with_filter = [&](auto kS) {
      if (cubic) with_border(kS, std::true_type());
      else with_border(kS, std::false_type());
    };
    if (p010) with_filter(uint16_t());
    else with_filter(uint8_t());
    return check_launch("nv12_render_scaled_kernel");
  }
  const int gx_l = ceil_div(W, kThreads), gx_c = ceil_div(W / 2, kThreads);
  const long n_l = (long)gx_l * ceil_div(H, kTpsRows), n_c = (long)gx_c * ceil_div(ch, kTpsRows);
  DVSG_REQUIRE(n_l + n_c < (1L << 31), "dvsg_tps_render_nv12: frame %dx%d too large", H, W);
  if (int rc = tps_apply_impl(winv_cols, coord, F_t, 1, n, P, T, stream, view.shape)) return rc;
  hipStream_t s = as_stream(stream);
  // algorithmic bytes: both planes once in, once out
  ProfScope prof(kClsTpsWarp, s, 0.0, 2.0 * bytes * n * H * W);
  const dim3 grid((unsigned)(n_l + n_c), n);
  // every kernel below but the plain one: the same grid of workgroups and one argument list for every surface, filter, border and zoom
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, Nv12{y, uv, pitch, frame_stride}, coord, T, zoom, H, W, P, lin_step(W),
                       lin_step(H), lin_step(W / 2), lin_step(ch), gx_l, (int)n_l, gx_c, ch, out_y, out_uv, out_pitch,
                       out_frame_stride);
  };
  if (p010) {   // a P010 view
    auto launch_p010 = [&](auto kZoom, auto kCubic, auto kBorder) { launch(p010_render_kernel<kZoom(), kCubic(), kBorder()>); };
    if (render_border != DVSG_BORDER_BLACK) {
      for_render_border(zoom != nullptr, cubic, render_border, launch_p010);
    } else {
      const std::integral_constant<int, DVSG_BORDER_BLACK> black;
      if (zoom && cubic) launch_p010(std::true_type(), std::true_type(), black);
      else if (zoom) launch_p010(std::true_type(), std::false_type(), black);
      else if (cubic) launch_p010(std::false_type(), std::true_type(), black);
      else launch_p010(std::false_type(), std::false_type(), black);
    }
    return check_launch("p010_render_kernel");
  }
  if (render_border != DVSG_BORDER_BLACK) {   // a view with a border mode
    for_render_border(zoom != nullptr, cubic, render_border, [&](auto kZoom, auto kCubic, auto kBorder) {
      launch(nv12_render_border_kernel<kZoom(), kCubic(), kBorder()>);
    });
    return check_launch("nv12_render_border_kernel");
  }
  if (cubic) {   // a bicubic view: 16 taps per sample
    if (zoom) launch(nv12_render_cubic_kernel<true>);
    else launch(nv12_render_cubic_kernel<false>);
    return check_launch("nv12_render_cubic_kernel");
  }
  if (zoom) {   // dvsg_tps_render_zoom_nv12: on the zoomed output grid
    launch(nv12_render_zoom_kernel);
    return check_launch("nv12_render_zoom_kernel");
  }
  hipLaunchKernelGGL(nv12_render_kernel, grid, dim3(kThreads), 0, s, Nv12{y, uv, pitch, frame_stride}, coord, T, H, W, P,
                     lin_step(W), lin_step(H), lin_step(W / 2), lin_step(ch), gx_l, (int)n_l, gx_c, ch, out_y, out_uv, out_pitch,
                     out_frame_stride);
  return check_launch("nv12_render_kernel");
}

}  // namespace dvsg

using namespace dvsg;

extern "C" {

int dvsg_frames_nv12_to_rgb_u8(const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int H, int W,
                               int matrix, int channel_flip, uint8_t *dst, void *stream) {
  const char *fn = "dvsg_frames_nv12_to_rgb_u8";
  DVSG_REQUIRE(dst, "%s: NULL dst", fn);
  if (int rc = check_nv12(fn, "source", y, uv, pitch, frame_stride, n, H, W)) return rc;
  if (int rc = check_matrix(fn, matrix)) return rc;
  const size_t blocks = (size_t)(H / 2) * ((W + 3) / 4);
  hipLaunchKernelGGL(nv12_to_rgb_kernel, dim3(grid_for(blocks), n), dim3(kThreads), 0, as_stream(stream),
                     Nv12{y, uv, pitch, frame_stride}, H, W, kYuv[matrix], channel_flip ? 1 : 0, dst);
  return check_launch("nv12_to_rgb_kernel");
}

int dvsg_frames_ingest_nv12(const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int src_H, int src_W,
                            int matrix, float *pool, int n_pool, const int32_t *slots, int dst_H, int dst_W, void *stream) {
  const char *fn = "dvsg_frames_ingest_nv12";
  DVSG_REQUIRE(pool && slots, "%s: NULL pointer", fn);
  if (int rc = check_nv12(fn, "source", y, uv, pitch, frame_stride, n, src_H, src_W)) return rc;
  if (int rc = check_matrix(fn, matrix)) return rc;
  DVSG_REQUIRE(n_pool > 0 && dst_H > 0 && dst_W > 0, "%s: bad shape n_pool=%d dst=%dx%d", fn, n_pool, dst_H, dst_W);
  const Nv12 s{y, uv, pitch, frame_stride};
  if (src_H == dst_H && src_W == dst_W) {
    const size_t groups = (size_t)src_H * ((src_W + 3) / 4);
    hipLaunchKernelGGL(ingest_nv12_kernel, dim3(grid_for(groups), n), dim3(kThreads), 0, as_stream(stream), s, src_H, src_W,
                       kYuv[matrix], pool, slots, n_pool);
    return check_launch("ingest_nv12_kernel");
  }
  hipLaunchKernelGGL(ingest_nv12_resize_kernel, dim3(grid_for((size_t)n * dst_H * dst_W)), dim3(kThreads), 0, as_stream(stream),
                     s, n, src_H, src_W, kYuv[matrix], pool, dst_H, dst_W, slots, n_pool);
  return check_launch("ingest_nv12_resize_kernel");
}

}  // extern "C"
