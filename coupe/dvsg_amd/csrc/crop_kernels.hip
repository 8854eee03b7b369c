// The valid region of a stabilised frame as a gfx950 HIP kernel: which output pixels of the thin-plate-spline warp does
// sampler A fill from four distinct taps, and how far from the centre is the nearest one it does not?
//
// Sampler A clips its tap indices before it forms the weights (ThinPlateSpline.py:57-60, sample_a_load), so a sample outside
// 0 <= x < W - 1, 0 <= y < H - 1 blends coincident taps with cancelling weights and is 0 up to the rounding of the blend: the
// black border.  The scan is the warp without its taps -- tps_warp_kernel's thread layout (one output column, kTpsRows rows), the map of
// tps_stage / tps_map_rows on the zoomed grid, then sample_a_valid -- followed by a per-frame reduction; x_s and y_s never
// reach memory.  This translation unit is compiled with -ffp-contract=off like warp_kernels.hip: a pixel's (x_s, y_s) are
// the bits dvsg_tps_warp_zoom_f32 gives for the same T and zoom.
//
// Per frame: n_border, the number of invalid pixels, and key_min, the minimum over them of the INTEGER key
//     key(i, j) = max(|2 j - (out_w - 1)| (out_h - 1), |2 i - (out_h - 1)| (out_w - 1)),
// which is D = (out_h - 1)(out_w - 1) times the pixel's normalised Chebyshev distance from the centre; INT32_MAX when no
// pixel is invalid.  Integer sums and minima do not depend on the order they are taken in.  They are reduced as the loss
// kernels reduce: per thread, across the wave by __shfl_xor, across the workgroup's waves through LDS, one partial per
// workgroup into the caller's workspace, and a second small launch over a frame's partials.  No atomics; every output
// element is written, so nothing has to be zeroed beforehand.
#include <climits>

#include "warp_device.h"

namespace dvsg {
namespace {

constexpr int kWaves = kThreads / 64;

struct Cover {
  int n, key;   // invalid pixels, their smallest key
};

// workgroup reduction of (sum, min); thread 0 holds the result
__device__ __forceinline__ Cover block_cover(Cover v) {
  __shared__ int red[2 * kWaves];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v.n += __shfl_xor(v.n, off);
    v.key = min(v.key, __shfl_xor(v.key, off));
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
    red[2 * (t >> 6)] = v.n;
    red[2 * (t >> 6) + 1] = v.key;
  }
  __syncthreads();
  Cover r{0, INT_MAX};
  if (t == 0) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      r.n += red[2 * w];
      r.key = min(r.key, red[2 * w + 1]);
    }
  }
  return r;
}

__global__ __launch_bounds__(kThreads) void crop_scan_kernel(const float *__restrict__ coord, long coord_bstride,
                                                             const float *__restrict__ T, const float *__restrict__ zoom,
                                                             int H, int W, int P, int out_h, int out_w, float step_x,
                                                             float step_y, Cover *__restrict__ partial) {
  __shared__ float4 sp[64];
  __shared__ float4 sdy[64];
  __shared__ float sa[6];
  const int b = blockIdx.z, t = threadIdx.x;
  const int i0 = blockIdx.y * kTpsRows;
  const float z = zoom ? zoom[b] : 1.0f;   // 1.0f x v == v: the plain grid's bits
  tps_stage<true, true>(coord, coord_bstride, T, b, P, t, i0, step_y, sp, sdy, sa, z);
  __syncthreads();
  const int jr = blockIdx.x * kThreads + t;
  const bool col_ok = jr < out_w;
  const int j = col_ok ? jr : out_w - 1;   // columns behind the grid repeat its last one and add nothing
  const float x_t = z * (-1.0f + step_x * (float)j);
  float xs[4], ys[4];
  tps_map_rows<true, true>(sp, sdy, sa, P, x_t, step_y, i0, xs, ys, z);
  const int kx = abs(2 * j - (out_w - 1)) * (out_h - 1);
  Cover acc{0, INT_MAX};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + r;
    if (col_ok && i < out_h && !sample_a_valid(H, W, xs[r], ys[r])) {   // rows behind the grid add nothing
      acc.n += 1;
      acc.key = min(acc.key, max(kx, abs(2 * i - (out_h - 1)) * (out_w - 1)));
    }
  }
  const Cover s = block_cover(acc);
  if (t == 0) partial[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// a frame's partials: lane l takes partials l, l + 256, ...; then block_cover
__global__ __launch_bounds__(kThreads) void crop_finish_kernel(const Cover *__restrict__ partial, int per_sample,
                                                               int *__restrict__ n_border, int *__restrict__ key_min) {
  const int b = blockIdx.x;
  Cover acc{0, INT_MAX};
  for (int k = threadIdx.x; k < per_sample; k += kThreads) {
    const Cover v = partial[(size_t)b * per_sample + k];
    acc.n += v.n;
    acc.key = min(acc.key, v.key);
  }
  const Cover s = block_cover(acc);
  if (threadIdx.x == 0) {
    n_border[b] = s.n;
    key_min[b] = s.key;
  }
}

// The zoom controller of a live stream (dvsg_crop_ratchet_f32): one thread per frame of the step, float64 throughout (this
// translation unit is compiled with -ffp-contract=off), one rounding to float32 at the end.  state[slot] is read and written
// by the one thread whose frame names the slot (distinct slots are the caller's contract): no atomics.
__global__ __launch_bounds__(kThreads) void crop_ratchet_kernel(const int *__restrict__ key_a, int D_a,
                                                                const int *__restrict__ key_b, int D_b,
                                                                const int *__restrict__ slots, int n, float *state,
                                                                int n_state, double margin, double crop_min, double recover,
                                                                float *__restrict__ zoom, double *__restrict__ free_out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int sl = slots[i];
  if (sl < 0 || sl >= n_state) return;
  double fr = (double)min(key_a[i], D_a) / (double)D_a;
  if (key_b) {
    const double fb = (double)min(key_b[i], D_b) / (double)D_b;
    fr = fb < fr ? fb : fr;
  }
  double target = fr - margin;
  target = target > crop_min ? target : crop_min;
  target = target < 1.0 ? target : 1.0;
  const double held = (double)state[sl] + recover;
  const float z = (float)(target < held ? target : held);
  state[sl] = z;
  zoom[i] = z;
  free_out[i] = fr;
}

int cover_partials(int out_h, int out_w) { return ceil_div(out_w, kThreads) * ceil_div(out_h, kTpsRows); }

int check_cover_shape(const char *fn, int B, int out_h, int out_w) {
  DVSG_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d outside [1, 65535]", fn, B);
  DVSG_REQUIRE(out_h >= 2 && out_w >= 2, "%s: the output grid %dx%d needs two rows and two columns (a key is a distance "
               "from the centre over the half extent)", fn, out_h, out_w);
  DVSG_REQUIRE((long)(out_h - 1) * (out_w - 1) < (long)INT_MAX && (long)out_h * out_w < (1L << 31) && (out_h + 3) / 4 <= 65535,
               "%s: the output grid %dx%d is too large ((out_h - 1)(out_w - 1) must stay below 2^31 - 1)", fn, out_h, out_w);
  return DVSG_OK;
}

}  // namespace

int tps_coverage_impl(const char *fn, const float *coord, long coord_bstride, const float *T, const float *zoom, int B, int P,
                      int src_H, int src_W, int out_h, int out_w, int32_t *n_border, int32_t *key_min, void *workspace,
                      size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(coord && T && n_border && key_min, "%s: NULL pointer", fn);
  DVSG_REQUIRE(P >= 1 && P <= kMaxPts, "%s: P=%d outside [1,%d]", fn, P, kMaxPts);
  DVSG_REQUIRE(src_H >= 1 && src_W >= 1, "%s: source size %dx%d must be positive", fn, src_H, src_W);
  if (int rc = check_cover_shape(fn, B, out_h, out_w)) return rc;
  DVSG_REQUIRE(workspace, "%s: NULL workspace", fn);
  if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return fail(DVSG_ERR_WORKSPACE, "%s: workspace must be 8-byte aligned", fn);
  const int per_sample = cover_partials(out_h, out_w);
  const size_t need = (size_t)B * per_sample * sizeof(Cover);
  if (workspace_bytes < need)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (dvsg_tps_coverage_workspace_bytes)", fn,
                workspace_bytes, need);
  hipStream_t s = as_stream(stream);
  Cover *partial = static_cast<Cover *>(workspace);
  dim3 grid(ceil_div(out_w, kThreads), ceil_div(out_h, kTpsRows), B);
  {
    // algorithmic bytes: the partials, written once and read once (the map itself touches no image)
    ProfScope prof(kClsTpsWarp, s, 0.0, 2.0 * (double)need);
    hipLaunchKernelGGL(crop_scan_kernel, grid, dim3(kThreads), 0, s, coord, coord_bstride, T, zoom, src_H, src_W, P, out_h,
                       out_w, lin_step(out_w), lin_step(out_h), partial);
    if (int rc = check_launch("crop_scan_kernel")) return rc;
    hipLaunchKernelGGL(crop_finish_kernel, dim3(B), dim3(kThreads), 0, s, partial, per_sample, n_border, key_min);
  }
  return check_launch("crop_finish_kernel");
}

}  // namespace dvsg

using namespace dvsg;

extern "C" {

int dvsg_tps_coverage_workspace_bytes(int B, int out_h, int out_w, size_t *bytes) {
  DVSG_REQUIRE(bytes, "dvsg_tps_coverage_workspace_bytes: NULL bytes");
  if (int rc = check_cover_shape("dvsg_tps_coverage_workspace_bytes", B, out_h, out_w)) return rc;
  *bytes = (size_t)B * cover_partials(out_h, out_w) * sizeof(Cover);
  return DVSG_OK;
}

int dvsg_tps_coverage_f32(const float *coord, const float *T, const float *zoom, int B, int P, int src_H, int src_W, int out_h,
                          int out_w, int32_t *n_border, int32_t *key_min, void *workspace, size_t workspace_bytes,
                          void *stream) {
  return tps_coverage_impl("dvsg_tps_coverage_f32", coord, (long)P * 2, T, zoom, B, P, src_H, src_W, out_h, out_w, n_border,
                           key_min, workspace, workspace_bytes, stream);
}

int dvsg_crop_ratchet_f32(const int32_t *key_min_a, int D_a, const int32_t *key_min_b, int D_b, const int32_t *state_slots,
                          int n, float *state, int n_state, double margin, double crop_min, double recover, float *zoom,
                          double *free_out, void *stream) {
  const char *fn = "dvsg_crop_ratchet_f32";
  DVSG_REQUIRE(key_min_a && state_slots && state && zoom && free_out, "%s: NULL pointer", fn);
  DVSG_REQUIRE(n >= 1 && n_state >= 1, "%s: n=%d and n_state=%d must be >= 1", fn, n, n_state);
  DVSG_REQUIRE(D_a >= 1 && (!key_min_b || D_b >= 1), "%s: D_a=%d, D_b=%d must be >= 1 (D = (out_h - 1)(out_w - 1))", fn, D_a,
               D_b);
  DVSG_REQUIRE(margin >= 0.0, "%s: margin=%g must be >= 0", fn, margin);
  DVSG_REQUIRE(crop_min > 0.0 && crop_min <= 1.0, "%s: crop_min=%g outside (0, 1]", fn, crop_min);
  DVSG_REQUIRE(recover >= 0.0, "%s: recover=%g must be >= 0", fn, recover);
  hipLaunchKernelGGL(crop_ratchet_kernel, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, as_stream(stream), key_min_a, D_a,
                     key_min_b, D_b, state_slots, n, state, n_state, margin, crop_min, recover, zoom, free_out);
  return check_launch("crop_ratchet_kernel");
}

}  // extern "C"
