// The root's max pool as kernels of its own (conv1.hip describes the root; the float32 band kernel may pool in its
// epilogue instead: conv1_f32.hip), one per tensor format.
#include "cnn_device.h"
#include "cnn_kernels.h"

namespace dvsg {
namespace {

// ----------------------------------------------------------------------------------------
// 3x3 / stride 2 max pool with TF 'SAME' padding (pad_before = pad_total / 2: nothing on
// the top/left for even sizes).  One thread = one output pixel x 4 channels.
// ----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T *__restrict__ x, T *__restrict__ y, int H, int W,
                                                     int C4, int Ho, int Wo, int pad_top, int pad_left,
                                                     size_t total) {
  // one element per thread; each XCD takes a contiguous range of blocks so that the output rows
  // sharing an input row (3x3 window, stride 2) read it out of the same L2
  {
    const size_t e = (size_t)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (e >= total) return;
    const int c4 = (int)(e % C4);
    size_t t = e / C4;
    const int wo = (int)(t % Wo);
    t /= Wo;
    const int ho = (int)(t % Ho);
    const size_t b = t / Ho;
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int hi = 2 * ho - pad_top + i;
      if (hi < 0 || hi >= H) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int wi = 2 * wo - pad_left + j;
        if (wi < 0 || wi >= W) continue;
        const float4 v = load4(x + (((b * H + hi) * W + wi) * C4 + c4) * 4);
        m.x = fmaxf(m.x, v.x);
        m.y = fmaxf(m.y, v.y);
        m.z = fmaxf(m.z, v.z);
        m.w = fmaxf(m.w, v.w);
      }
    }
    store4(y + e * 4, m);
  }
}

// float16 tensors, 8 channels = 16 bytes per thread: with 4 channels a thread moves 8-byte pieces and the kernel ran
// at 3.2 TB/s of algorithmic traffic where the float32 one reaches 5.1 (comparisons in float16 are exact: max of
// representable values)
__global__ __launch_bounds__(256) void maxpool_h8_kernel(const _Float16 *__restrict__ x, _Float16 *__restrict__ y, int H,
                                                         int W, int C8, int Ho, int Wo, int pad_top, int pad_left,
                                                         size_t total) {
  const size_t e = (size_t)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const int c8 = (int)(e % C8);
  size_t t = e / C8;
  const int wo = (int)(t % Wo);
  t /= Wo;
  const int ho = (int)(t % Ho);
  const size_t b = t / Ho;
  halfx8 m;
#pragma unroll
  for (int q = 0; q < 8; ++q) m[q] = (_Float16)(-INFINITY);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int hi = 2 * ho - pad_top + i;
    if (hi < 0 || hi >= H) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int wi = 2 * wo - pad_left + j;
      if (wi < 0 || wi >= W) continue;
      const halfx8 v = *reinterpret_cast<const halfx8 *>(x + (((b * H + hi) * W + wi) * C8 + c8) * 8);
#pragma unroll
      for (int q = 0; q < 8; ++q) m[q] = v[q] > m[q] ? v[q] : m[q];
    }
  }
  *reinterpret_cast<halfx8 *>(y + e * 8) = m;
}

// max pool on a P-format tensor ("f32s"): the pieces are joined (exact), compared, and the maximum's pieces stored
__global__ __launch_bounds__(256) void maxpool_p_kernel(const void *__restrict__ x, void *__restrict__ y, int H, int W,
                                                       int C4, int Ho, int Wo, int pad_top, int pad_left, size_t total) {
  const size_t e = (size_t)xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const int c4 = (int)(e % C4);
  size_t t = e / C4;
  const int wo = (int)(t % Wo);
  t /= Wo;
  const int ho = (int)(t % Ho);
  const size_t b = t / Ho;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int hi = 2 * ho - pad_top + i;
    if (hi < 0 || hi >= H) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int wi = 2 * wo - pad_left + j;
      if (wi < 0 || wi >= W) continue;
      const float4 v = load4_p(x, (((b * H + hi) * W + wi) * C4 + c4) * 4);
      m.x = fmaxf(m.x, v.x);
      m.y = fmaxf(m.y, v.y);
      m.z = fmaxf(m.z, v.z);
      m.w = fmaxf(m.w, v.w);
    }
  }
  store4_p(y, e * 4, m);
}

}  // namespace

int launch_maxpool(int prec, const void *x, void *y, int B, int H, int W, int C, int Ho, int Wo, int pad_top,
                   int pad_left, hipStream_t s) {
  DVSG_REQUIRE(C % 4 == 0 && (prec != kF32S || C % 32 == 0), "maxpool: C=%d must be a multiple of 4 (32 in the f32s format)", C);
  const size_t total = (size_t)B * Ho * Wo * (C / 4);
  const size_t want = (total + 255) / 256;
  DVSG_REQUIRE(want < (1u << 31), "maxpool: %zu blocks do not fit a grid", want);
  const int blocks = (int)want;
  ProfScope prof(kClsMaxpool, s, 0.0, (double)elem_size(prec) * C * ((double)B * H * W + (double)B * Ho * Wo));
  g_last_root_kernel[kRootMaxpool] = prec == kF32S ? 3 : (prec == kF16 ? (C % 8 == 0 ? 2 : 1) : 0);
  if (prec == kF32S)
    hipLaunchKernelGGL(maxpool_p_kernel, dim3(blocks), dim3(256), 0, s, x, y, H, W, C / 4, Ho, Wo, pad_top, pad_left, total);
  else if (prec == kF16 && C % 8 == 0) {
    const size_t total8 = total / 2;
    hipLaunchKernelGGL(maxpool_h8_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, s, static_cast<const _Float16 *>(x),
                       static_cast<_Float16 *>(y), H, W, C / 8, Ho, Wo, pad_top, pad_left, total8);
  } else if (prec == kF16)
    hipLaunchKernelGGL(maxpool_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, static_cast<const _Float16 *>(x),
                       static_cast<_Float16 *>(y), H, W, C / 4, Ho, Wo, pad_top, pad_left, total);
  else
    hipLaunchKernelGGL(maxpool_kernel<float>, dim3(blocks), dim3(256), 0, s, static_cast<const float *>(x),
                       static_cast<float *>(y), H, W, C / 4, Ho, Wo, pad_top, pad_left, total);
  return check_launch("maxpool_kernel");
}

}  // namespace dvsg
