// The reference's test-time losses (trainer.py:95-123, 233-323, 363-386) as gfx950 HIP kernels: the score
// `errs_total_test['total']` that ranks checkpoints (main.py:198-221).  Forward only.
//
// Every per-pixel term is the chain of separately rounded float32 ops of the TF graph (this translation unit is compiled
// with -ffp-contract=off, like warp_kernels.hip, whose device functions it shares through warp_device.h: a pixel's
// prediction, mask and source coordinates are the bits dvsg_tps_warp_f32 / dvsg_flow_warp_f32 give).  The SUMS follow the
// library's rules: no atomics; every term is widened to float64 and added in a fixed order -- per thread, then across the
// wave by __shfl_xor, then across the workgroup's waves through LDS, one partial per workgroup into the caller's
// workspace, and a second small launch that adds a sample's partials in index order.  A float64 sum of n float32 terms is
// off by at most n 2^-53 of sum |term|: far below one float32 rounding, so the result does not depend on n.
#include <algorithm>

#include "warp_device.h"

namespace dvsg {
namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kMseMaxBlocks = 1024;   // partials per sample of the stand-alone masked_MSE
constexpr int kMsePerThread = 8;

struct Sum2 {
  double num, den;
};

// workgroup sum of (num, den) in a fixed order; thread 0 holds the result
__device__ __forceinline__ Sum2 block_sum(Sum2 v) {
  __shared__ double red[2 * kWaves];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v.num += __shfl_xor(v.num, off);
    v.den += __shfl_xor(v.den, off);
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
    red[2 * (t >> 6)] = v.num;
    red[2 * (t >> 6) + 1] = v.den;
  }
  __syncthreads();
  Sum2 r{0.0, 0.0};
  if (t == 0) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      r.num += red[2 * w];
      r.den += red[2 * w + 1];
    }
  }
  return r;
}

// masked_MSE's per-pixel term (trainer.py:234-237) over the 3 channels of one pixel, mask m the same in each
__device__ __forceinline__ void mse_terms3(const float *pred, const Pix<3> &gt, float m, Sum2 &acc) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float pm = pred[c] * m;   // :234
    const float gm = gt.v[c] * m;   // :235
    const float d = pm - gm;        // :237 squared_difference
    acc.num += (double)(d * d);
    acc.den += (double)m;           // :242 reduce_sum(mask) counts the plane once per channel
  }
}

// ----------------------------------------------------------------------------------------
// Image term (trainer.py:100-101, model.py:81-85): masked_MSE(TPS(u), gt, TPS(ones)).  tps_warp_kernel's thread layout and
// map; the mask is sampler A on ones -- the four weights formed after the index clip, added in the blend's order.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loss_image_kernel(const float *__restrict__ U, const float *__restrict__ coord,
                                                              const float *__restrict__ T, const float *__restrict__ gt,
                                                              int H, int W, int P, float step_x, float step_y,
                                                              float *__restrict__ pred_out, float *__restrict__ mask_out,
                                                              Sum2 *__restrict__ partial) {
  __shared__ float4 sp[64];
  __shared__ float4 sdy[64];
  __shared__ float sa[6];
  const int b = blockIdx.z, t = threadIdx.x;
  const int i0 = blockIdx.y * kTpsRows;
  tps_stage<true>(coord, (long)P * 2, T, b, P, t, i0, step_y, sp, sdy, sa);
  __syncthreads();
  const int jr = blockIdx.x * kThreads + t;
  const bool col_ok = jr < W;
  const int j = col_ok ? jr : W - 1;   // columns behind the image repeat its last one and add nothing
  const float x_t = -1.0f + step_x * (float)j;
  const float *img = U + (size_t)b * H * W * 3;
  float xs[4], ys[4];
  tps_map_rows<true>(sp, sdy, sa, P, x_t, step_y, i0, xs, ys);
  TapsA<3> taps[4];
  Pix<3> g[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = min(i0 + r, H - 1);
    sample_a_load<3, float>(img, H, W, 3, xs[r], ys[r], taps[r]);
    g[r] = load_pix<3>(gt + (((size_t)b * H + i) * W + j) * 3);
  }
  Sum2 acc{0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + r;
    const bool ok = col_ok && i < H;
    float v[3];
    sample_a_blend<3>(taps[r], 3, v);
    const TapsA<3> &q = taps[r];
    const float m = ((q.wa + q.wb) + q.wc) + q.wd;   // ThinPlateSpline.py:89 on an image of ones
    Sum2 a{0.0, 0.0};
    mse_terms3(v, g[r], m, a);
    if (ok) {
      acc.num += a.num;
      acc.den += a.den;
      const size_t pix = ((size_t)b * H + i) * W + j;
      if (pred_out) store_pix<3>(pred_out, pix, 3, v);
      if (mask_out) mask_out[pix] = m;
    }
  }
  const Sum2 s = block_sum(acc);
  if (t == 0) partial[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// ----------------------------------------------------------------------------------------
// Temporal term (trainer.py:245-250): masked_MSE(tf_warp(pred), gt, tf_warp(mask_pred) * mask_gt).  The gather form of
// stn_kernel<kFlow>: a thread owns a column and 4 rows; taps and weights of a pixel are formed once from the flow and
// blend the frame's three channels and the mask plane; nothing warped is written.
// ----------------------------------------------------------------------------------------
constexpr int kTmpRows = 4;

__global__ __launch_bounds__(kThreads) void loss_temporal_kernel(const float *__restrict__ pred,
                                                                 const float *__restrict__ mask_pred,
                                                                 const float *__restrict__ flow, const float *__restrict__ gt,
                                                                 const float *__restrict__ mask_gt, int H, int W,
                                                                 Sum2 *__restrict__ partial) {
  const int b = blockIdx.z, t = threadIdx.x;
  const int i0 = blockIdx.y * kTmpRows;
  const int jr = blockIdx.x * kThreads + t;
  const bool col_ok = jr < W;
  const int j = col_ok ? jr : W - 1;
  const size_t img_pix = (size_t)b * H * W;
  const float *img = pred + img_pix * 3;
  const float *mpl = mask_pred + img_pix;
  float2 fl[kTmpRows];
#pragma unroll
  for (int r = 0; r < kTmpRows; ++r) {
    const int i = min(i0 + r, H - 1);
    fl[r] = reinterpret_cast<const float2 *>(flow)[img_pix + (size_t)i * W + j];
  }
  TapsB<3> tp[kTmpRows];
  TapsB<1> tm[kTmpRows];
  Pix<3> g[kTmpRows];
  float mg[kTmpRows];
#pragma unroll
  for (int r = 0; r < kTmpRows; ++r) {
    const int i = min(i0 + r, H - 1);
    const float x = (float)j + fl[r].x;   // warp_with_optical_flow.py:117-119
    const float y = (float)i + fl[r].y;
    const PadGeom pg = padded_geom(H, W, x, y);
    sample_padded_load_geom<3>(img, W, 3, pg, tp[r]);
    sample_padded_load_geom<1>(mpl, W, 1, pg, tm[r]);
    const size_t pix = img_pix + (size_t)i * W + j;
    g[r] = load_pix<3>(gt + pix * 3);
    mg[r] = mask_gt[pix];
  }
  Sum2 acc{0.0, 0.0};
#pragma unroll
  for (int r = 0; r < kTmpRows; ++r) {
    const bool ok = col_ok && i0 + r < H;
    float v[3], mw[1];
    sample_padded_blend<3>(tp[r], 3, v);
    sample_padded_blend<1>(tm[r], 1, mw);
    const float m = mw[0] * mg[r];   // trainer.py:250
    Sum2 a{0.0, 0.0};
    mse_terms3(v, g[r], m, a);
    if (ok) {
      acc.num += a.num;
      acc.den += a.den;
    }
  }
  const Sum2 s = block_sum(acc);
  if (t == 0) partial[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// ----------------------------------------------------------------------------------------
// Stand-alone masked_MSE (trainer.py:233-243) on [B,n] elements, n = H W C; the mask has n elements per sample, or n / C
// (a plane counted C times).  Workgroup `blk` of a sample takes elements blk * 256 + t + k * 256 * nblk.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loss_mse_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                            const float *__restrict__ mask, long n, int C, int mask_is_plane,
                                                            Sum2 *__restrict__ partial) {
  const int b = blockIdx.y, t = threadIdx.x;
  const long stride = (long)gridDim.x * kThreads;
  const long first = (long)blockIdx.x * kThreads + t;
  const long nm = mask_is_plane ? n / C : n;
  Sum2 acc{0.0, 0.0};
  for (long e0 = first; e0 < n; e0 += stride * kMsePerThread) {
    float p[kMsePerThread], g[kMsePerThread], m[kMsePerThread];
#pragma unroll
    for (int k = 0; k < kMsePerThread; ++k) {   // unconditional loads from clamped indices
      const long e = min(e0 + k * stride, n - 1);
      p[k] = pred[b * n + e];
      g[k] = gt[b * n + e];
      m[k] = mask[b * nm + (mask_is_plane ? e / C : e)];
    }
#pragma unroll
    for (int k = 0; k < kMsePerThread; ++k) {
      const float pm = p[k] * m[k];
      const float gm = g[k] * m[k];
      const float d = pm - gm;
      const bool ok = e0 + k * stride < n;
      acc.num += ok ? (double)(d * d) : 0.0;
      acc.den += ok ? (double)m[k] : 0.0;
    }
  }
  const Sum2 s = block_sum(acc);
  if (t == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// tf.div_no_nan in float32 of the two float32-rounded sums (trainer.py:242)
__device__ __forceinline__ float div_no_nan(float a, float b) { return b != 0.f ? a / b : 0.f; }

// A sample's partials added in index order: lane l takes partials l, l + 256, ...; then block_sum.
__global__ __launch_bounds__(kThreads) void loss_finish_kernel(const Sum2 *__restrict__ partial, int per_sample,
                                                               float *__restrict__ per_sample_out, double *__restrict__ sums) {
  const int b = blockIdx.x, t = threadIdx.x;
  Sum2 acc{0.0, 0.0};
  for (int k = t; k < per_sample; k += kThreads) {
    const Sum2 v = partial[(size_t)b * per_sample + k];
    acc.num += v.num;
    acc.den += v.den;
  }
  const Sum2 s = block_sum(acc);
  if (t == 0) {
    per_sample_out[b] = div_no_nan((float)s.num, (float)s.den);
    if (sums) {
      sums[2 * b] = s.num;
      sums[2 * b + 1] = s.den;
    }
  }
}

// tf.reduce_mean over the batch of up to two per-sample vectors (one wave; float64, index order per lane then shuffles)
__global__ __launch_bounds__(64) void loss_batch_mean_kernel(const float *__restrict__ a, float *__restrict__ mean_a,
                                                             const float *__restrict__ b2, float *__restrict__ mean_b, int B) {
  const int t = threadIdx.x;
  double sa = 0.0, sb = 0.0;
  for (int k = t; k < B; k += 64) {
    sa += (double)a[k];
    if (b2) sb += (double)b2[k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sa += __shfl_xor(sa, off);
    sb += __shfl_xor(sb, off);
  }
  if (t == 0) {
    *mean_a = (float)(sa / (double)B);
    if (b2) *mean_b = (float)(sb / (double)B);
  }
}

// ----------------------------------------------------------------------------------------
// Grid terms, one workgroup per sample.  identity (trainer.py:105-106): mean |F| over [P,2].  distortion_loss
// (trainer.py:252-323) as written: V_src mapped to [0,1] (:272), the four get_sp_term triangles (:275-321) with
// M_rot = [[0,1],[-1,0]] (:255).  Thread = one cell of the (n-1) x (n-1) grid, its four terms in float32 op by op; thread 0
// adds the cells in index order (float64).
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ float sp_term(const float *vs, const float *vs0, const float *vs1, const float *v, const float *v0,
                                         const float *v1) {
  // :254  s = sqrt(sum (v_src - v_src_1)^2) / sqrt(sum (v_src_0 - v_src_1)^2)
  const float a0 = vs[0] - vs1[0], a1 = vs[1] - vs1[1];
  const float c0 = vs0[0] - vs1[0], c1 = vs0[1] - vs1[1];
  const float s = sqrtf(a0 * a0 + a1 * a1) / sqrtf(c0 * c0 + c1 * c1);
  const float d0 = v0[0] - v1[0], d1 = v0[1] - v1[1];   // :256
  const float r0 = 0.f * d0 + 1.f * d1;                  // :261 M_rot . (v_0 - v_1)
  const float r1 = -1.f * d0 + 0.f * d1;
  const float e0 = (v[0] - v1[0]) - s * r0;              // :266
  const float e1 = (v[1] - v1[1]) - s * r1;
  return e0 * e0 + e1 * e1;
}

__global__ __launch_bounds__(64) void loss_grid_kernel(const float *__restrict__ V_src, const float *__restrict__ F, int n,
                                                       float *__restrict__ identity, float *__restrict__ distortion) {
  __shared__ float vs[64 * 2], vv[64 * 2], absf[64 * 2], term[4][64];
  const int b = blockIdx.x, t = threadIdx.x, P = n * n;
  if (t < P) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float f = F[((size_t)b * P + t) * 2 + c];
      const float s = (V_src[((size_t)b * P + t) * 2 + c] + 1.0f) / 2.0f;   // :272
      vs[t * 2 + c] = s;
      vv[t * 2 + c] = s + f;                                                // :273
      absf[t * 2 + c] = fabsf(f - 0.f);                                     // :105 |F - identity|
    }
  }
  __syncthreads();
  const int m = n - 1;
  if (t < m * m) {
    const int i = t / m, j = t % m;
    const int p00 = (i * n + j) * 2, p01 = (i * n + j + 1) * 2, p10 = ((i + 1) * n + j) * 2, p11 = ((i + 1) * n + j + 1) * 2;
    term[0][t] = sp_term(vs + p00, vs + p11, vs + p10, vv + p00, vv + p11, vv + p10);   // :275-285
    term[1][t] = sp_term(vs + p01, vs + p10, vs + p11, vv + p01, vv + p10, vv + p11);   // :287-297
    term[2][t] = sp_term(vs + p10, vs + p01, vs + p00, vv + p10, vv + p01, vv + p00);   // :299-309
    term[3][t] = sp_term(vs + p11, vs + p00, vs + p01, vv + p11, vv + p00, vv + p01);   // :311-321
  }
  __syncthreads();
  if (t == 0) {
    float mean[4];
    for (int q = 0; q < 4; ++q) {
      double s = 0.0;
      for (int k = 0; k < m * m; ++k) s += (double)term[q][k];
      mean[q] = (float)(s / (double)(m * m));   // :266 reduce_mean over the cells
    }
    if (distortion) distortion[b] = (((mean[0] + mean[1]) + mean[2]) + mean[3]) / 4.0f;   // :323
    double s = 0.0;
    for (int k = 0; k < 2 * P; ++k) s += (double)absf[k];
    if (identity) identity[b] = (float)(s / (double)(2 * P));
  }
}

// ----------------------------------------------------------------------------------------
// SURF term (trainer.py:363-386), one workgroup per sample.  x_offset / y_offset are not materialised: the TPS map is
// evaluated at the N flat indices idx = x + y w only, by the functions tps_warp_kernel uses for that pixel (row group
// i0 = 4 (i / 4), the pixel's row of the four).  idx == h w reads the appended -1 (:364-365); an index outside [0, h w]
// (an error in tf.batch_gather) is clamped into it.  All N points count, padded ones included.
// A point costs the map of its whole row group -- 4 x P logs for the one row kept -- which is nothing at N ~ 50 with one
// workgroup per sample; a caller with thousands of points per sample wants a one-row form of tps_map_rows first.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void loss_surf_kernel(const float *__restrict__ surf, const float *__restrict__ surfs_dim,
                                                             const float *__restrict__ coord, const float *__restrict__ T,
                                                             int N, int H, int W, int P, float step_x, float step_y,
                                                             float *__restrict__ coords_out, float *__restrict__ per_sample,
                                                             double *__restrict__ sums) {
  __shared__ float4 sp[64];
  __shared__ float sa[6];
  const int b = blockIdx.x, t = threadIdx.x;
  tps_stage<false>(coord, (long)P * 2, T, b, P, t, 0, step_y, sp, nullptr, sa);
  __syncthreads();
  const float *un = surf + ((size_t)b * 2 + 0) * N * 2;   // :368 surf[:, 0]
  const float *st = surf + ((size_t)b * 2 + 1) * N * 2;   // :374 surf[:, 1]
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  Sum2 acc{0.0, 0.0};
  for (int k = t; k < N; k += kThreads) {
    const float fidx = st[k * 2] + st[k * 2 + 1] * (float)W;   // :377
    int idx = f2i(fidx);
    idx = clampi(idx, 0, H * W);
    const bool sentinel = idx == H * W;
    const int pix = sentinel ? H * W - 1 : idx;
    const int i = pix / W, j = pix - i * W;
    const int i0 = i & ~(kTpsRows - 1), r = i & (kTpsRows - 1);
    const float x_t = -1.0f + step_x * (float)j;
    float xs[4], ys[4];
    tps_map_rows<false>(sp, nullptr, sa, P, x_t, step_y, i0, xs, ys);
    float tx = xs[0], ty = ys[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      tx = r == q ? xs[q] : tx;
      ty = r == q ? ys[q] : ty;
    }
    tx = sentinel ? -1.0f : tx;
    ty = sentinel ? -1.0f : ty;
    const float ux = (un[k * 2] / wm1) * 2.0f - 1.0f;       // :369
    const float uy = (un[k * 2 + 1] / hm1) * 2.0f - 1.0f;   // :370
    const float dx = tx - ux, dy = ty - uy;                  // :383
    acc.num += (double)(dx * dx);
    acc.num += (double)(dy * dy);
    if (coords_out) {
      coords_out[((size_t)b * N + k) * 2] = tx;
      coords_out[((size_t)b * N + k) * 2 + 1] = ty;
    }
  }
  const Sum2 s = block_sum(acc);
  if (t == 0) {
    per_sample[b] = div_no_nan((float)s.num, surfs_dim[b]);   // :384
    if (sums) sums[b] = s.num;
  }
}

int grid_partials(int H, int W) { return ceil_div(W, kThreads) * ceil_div(H, kTpsRows); }

size_t workspace_need(int B, int H, int W) {
  return (size_t)B * (size_t)std::max(grid_partials(H, W), kMseMaxBlocks) * sizeof(Sum2);
}

int check_loss_args(const char *fn, int B, long H, long W, const void *per_sample, const void *mean) {
  DVSG_REQUIRE(per_sample && mean, "%s: NULL per_sample / mean", fn);
  DVSG_REQUIRE(B > 0 && H > 0 && W > 0, "%s: sizes must be positive (B=%d H=%ld W=%ld)", fn, B, H, W);
  DVSG_REQUIRE(B <= 65535, "%s: B=%d exceeds the grid limit 65535", fn, B);
  DVSG_REQUIRE(H * W < (1L << 31) / 4 && (H + 3) / 4 <= 65535, "%s: image too large", fn);
  return DVSG_OK;
}

int check_workspace(const char *fn, int B, int H, int W, const void *workspace, size_t workspace_bytes) {
  DVSG_REQUIRE(workspace, "%s: NULL workspace", fn);
  if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return fail(DVSG_ERR_WORKSPACE, "%s: workspace must be 8-byte aligned", fn);
  const size_t need = workspace_need(B, H, W);
  if (workspace_bytes < need)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (dvsg_loss_workspace_bytes)", fn, workspace_bytes, need);
  return DVSG_OK;
}

int finish(const Sum2 *partial, int per_sample_n, int B, float *per_sample, float *mean, double *sums, hipStream_t s,
           const char *what) {
  hipLaunchKernelGGL(loss_finish_kernel, dim3(B), dim3(kThreads), 0, s, partial, per_sample_n, per_sample, sums);
  hipLaunchKernelGGL(loss_batch_mean_kernel, dim3(1), dim3(64), 0, s, (const float *)per_sample, mean, (const float *)nullptr,
                     (float *)nullptr, B);
  return check_launch(what);
}

}  // namespace
}  // namespace dvsg

using namespace dvsg;

extern "C" {

int dvsg_loss_workspace_bytes(int B, int H, int W, size_t *bytes) {
  DVSG_REQUIRE(bytes, "dvsg_loss_workspace_bytes: NULL bytes");
  DVSG_REQUIRE(B > 0 && H > 0 && W > 0, "dvsg_loss_workspace_bytes: sizes must be positive (B=%d H=%d W=%d)", B, H, W);
  *bytes = workspace_need(B, H, W);
  return DVSG_OK;
}

int dvsg_loss_image_f32(const float *U, const float *coord, const float *T, const float *gt, int B, int H, int W, int P,
                        float *pred, float *mask, float *per_sample, float *mean, double *sums, void *workspace,
                        size_t workspace_bytes, void *stream) {
  const char *fn = "dvsg_loss_image_f32";
  DVSG_REQUIRE(U && coord && T && gt, "%s: NULL pointer", fn);
  DVSG_REQUIRE(P >= 1 && P <= kMaxPts, "%s: P=%d outside [1,%d]", fn, P, kMaxPts);
  if (int rc = check_loss_args(fn, B, H, W, per_sample, mean)) return rc;
  if (int rc = check_workspace(fn, B, H, W, workspace, workspace_bytes)) return rc;
  hipStream_t s = as_stream(stream);
  Sum2 *partial = static_cast<Sum2 *>(workspace);
  dim3 grid(ceil_div(W, kThreads), ceil_div(H, kTpsRows), B);
  hipLaunchKernelGGL(loss_image_kernel, grid, dim3(kThreads), 0, s, U, coord, T, gt, H, W, P, lin_step(W), lin_step(H), pred,
                     mask, partial);
  return finish(partial, grid_partials(H, W), B, per_sample, mean, sums, s, "loss_image_kernel");
}

int dvsg_loss_temporal_f32(const float *pred, const float *mask_pred, const float *flow, const float *gt, const float *mask_gt,
                           int B, int H, int W, float *per_sample, float *mean, double *sums, void *workspace,
                           size_t workspace_bytes, void *stream) {
  const char *fn = "dvsg_loss_temporal_f32";
  DVSG_REQUIRE(pred && mask_pred && flow && gt && mask_gt, "%s: NULL pointer", fn);
  DVSG_REQUIRE(reinterpret_cast<uintptr_t>(flow) % 8 == 0, "%s: flow must be 8-byte aligned (read as float2)", fn);
  if (int rc = check_loss_args(fn, B, H, W, per_sample, mean)) return rc;
  if (int rc = check_workspace(fn, B, H, W, workspace, workspace_bytes)) return rc;
  hipStream_t s = as_stream(stream);
  Sum2 *partial = static_cast<Sum2 *>(workspace);
  dim3 grid(ceil_div(W, kThreads), ceil_div(H, kTmpRows), B);
  hipLaunchKernelGGL(loss_temporal_kernel, grid, dim3(kThreads), 0, s, pred, mask_pred, flow, gt, mask_gt, H, W, partial);
  return finish(partial, grid_partials(H, W), B, per_sample, mean, sums, s, "loss_temporal_kernel");
}

int dvsg_loss_masked_mse_f32(const float *pred, const float *gt, const float *mask, int B, int H, int W, int C,
                             int mask_is_plane, float *per_sample, float *mean, double *sums, void *workspace,
                             size_t workspace_bytes, void *stream) {
  const char *fn = "dvsg_loss_masked_mse_f32";
  DVSG_REQUIRE(pred && gt && mask, "%s: NULL pointer", fn);
  DVSG_REQUIRE(C >= 1 && C <= kMaxGenericC, "%s: C=%d outside [1,%d]", fn, C, kMaxGenericC);
  if (int rc = check_loss_args(fn, B, H, W, per_sample, mean)) return rc;
  if (int rc = check_workspace(fn, B, H, W, workspace, workspace_bytes)) return rc;
  hipStream_t s = as_stream(stream);
  Sum2 *partial = static_cast<Sum2 *>(workspace);
  const long n = (long)H * W * C;
  const int nblk = std::min(ceil_div(n, (long)kThreads * kMsePerThread), kMseMaxBlocks);
  hipLaunchKernelGGL(loss_mse_kernel, dim3(nblk, B), dim3(kThreads), 0, s, pred, gt, mask, n, C, mask_is_plane ? 1 : 0, partial);
  return finish(partial, nblk, B, per_sample, mean, sums, s, "loss_mse_kernel");
}

int dvsg_loss_grid_f32(const float *V_src, const float *F, int B, int num_control_points, float *identity, float *identity_mean,
                       float *distortion, float *distortion_mean, void *stream) {
  const char *fn = "dvsg_loss_grid_f32";
  DVSG_REQUIRE(V_src && F && identity && identity_mean && distortion && distortion_mean, "%s: NULL pointer", fn);
  DVSG_REQUIRE(B > 0, "%s: B=%d must be positive", fn, B);
  DVSG_REQUIRE(num_control_points >= 2 && num_control_points * num_control_points <= kMaxPts,
               "%s: num_control_points=%d outside [2,7]", fn, num_control_points);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(loss_grid_kernel, dim3(B), dim3(64), 0, s, V_src, F, num_control_points, identity, distortion);
  hipLaunchKernelGGL(loss_batch_mean_kernel, dim3(1), dim3(64), 0, s, (const float *)identity, identity_mean,
                     (const float *)distortion, distortion_mean, B);
  return check_launch("loss_grid_kernel");
}

int dvsg_loss_surf_f32(const float *surf, const float *surfs_dim, const float *coord, const float *T, int B, int N, int H, int W,
                       int P, float *coords, float *per_sample, float *mean, double *sums, void *stream) {
  const char *fn = "dvsg_loss_surf_f32";
  DVSG_REQUIRE(surf && surfs_dim && coord && T, "%s: NULL pointer", fn);
  DVSG_REQUIRE(N > 0 && N < (1 << 24), "%s: N=%d outside [1, 2^24)", fn, N);
  DVSG_REQUIRE(P >= 1 && P <= kMaxPts, "%s: P=%d outside [1,%d]", fn, P, kMaxPts);
  if (int rc = check_loss_args(fn, B, H, W, per_sample, mean)) return rc;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(loss_surf_kernel, dim3(B), dim3(kThreads), 0, s, surf, surfs_dim, coord, T, N, H, W, P, lin_step(W),
                     lin_step(H), coords, per_sample, sums);
  hipLaunchKernelGGL(loss_batch_mean_kernel, dim3(1), dim3(64), 0, s, (const float *)per_sample, mean, (const float *)nullptr,
                     (float *)nullptr, B);
  return check_launch("loss_surf_kernel");
}

}  // extern "C"
