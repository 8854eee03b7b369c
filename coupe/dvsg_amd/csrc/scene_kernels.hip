// Scene cuts of live streams as gfx950 HIP kernels (dvsg_scene_step_f32): one luma histogram per input frame, the distance to
// the stream's previous histogram, the decision, and the step's slot rows, all on the device.
//
// A stream's ring (include/dvsg_amd.h, ONLINE) holds span + 1 stabilised frames of history and the network's window reaches
// span frames back, so after a cut the window would mix two scenes for span steps.  A detected cut at frame f restarts the ring
// at f: the device-side step count k of the ring goes back to 0, so f is step 0 of eval.py:93-94 (every window entry the input
// slot), the rows that follow are stream_window_row(k, base) with k counted from f, and the crop zoom of the ring goes back to
// crop_start.  HISTORY SLOTS THAT STILL HOLD THE OLD SCENE ARE NEVER READ: step k >= 1 after a restart reads the history slots
// of frames max(k + skip[s] - span, 0) in 0 .. k - 1 of the new run, each written by an earlier step of that run, and writes
// slot k % (span + 1); nothing is cleared because nothing stale is reachable.
//
// The statistic is integer after one quantisation, so its bar is bit equality with the NumPy restatement (tests/scene_ref.py).
// This translation unit is compiled with -ffp-contract=off: the luma's five float32 operations are rounded one by one.
//     Y = fl(fl(fl(0.299f r) + fl(0.587f g)) + fl(0.114f b));  q = clamp((int)floorf(fl(Y 255f) + 0.5f), 0, 255), NaN -> 0
//     bin = q >> 2 (64 bins, int32 counts);  S = sum_b |cur[b] - prev[b]| in [0, 2 H W];  cut <=> k >= max(1, min_len) and S >= thr
//
// Three launches, stream-ordered, nothing synchronised:
//   scene_zero_kernel    zeroes the workspace ([B,64] int32).  A kernel, not hipMemsetAsync: a memset node captured into a
//                        HIP graph did not take effect on the second and later replays on ROCm 7.2 (cnn_kernels.h,
//                        launch_zero_tickets), and the histograms of a replayed step would add up.
//   scene_hist_kernel    grid (blocks per frame, B).  A frame is 3 H W contiguous floats: four pixels are three 16-byte loads.
//                        The pixels in front of the first 16-byte boundary (at most 3; a frame of an odd pixel count starts
//                        anywhere) and behind the last whole quad (at most 3) take a scalar path in block 0 -- no padding.
//                        Every wave counts into its own 64-bin LDS histogram with LDS integer atomics; the block merges its
//                        waves once and adds each non-zero bin to the workspace with one global (device-scope) int32 atomic.
//                        All sums are integer: the result does not depend on the order the adds arrive in.
//   scene_decide_kernel  one wave per row, lane = bin: |cur - prev| reduced across the wave by __shfl_xor, lane 0 decides and
//                        writes the scalars, lanes < S write the table row, every lane stores its bin of the new state.
//                        The launch boundary is what makes the first kernel's atomics visible here.
#include <climits>
#include <cstdint>

#include "common.h"

namespace dvsg {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 64;
constexpr int kQuadsPerThread = 4;     // quads a thread takes when the frame is large enough to fill the blocks
constexpr int kMaxBlocksPerFrame = 256;
constexpr int kMaxSkip = 16;
constexpr int kStateInts = DVSG_SCENE_STATE_INTS;
static_assert(kStateInts == 4 + kBins, "state row: k, cuts, S, 0, then the previous histogram");

struct SkipTable {
  int v[kMaxSkip];
};

__device__ __forceinline__ int luma_bin(float r, float g, float b) {
  const float y = (0.299f * r + 0.587f * g) + 0.114f * b;
  const float t = y * 255.0f + 0.5f;
  if (!(t >= 0.0f)) return 0;          // negative, -inf and NaN
  if (t >= 256.0f) return kBins - 1;   // +inf included
  return (int)floorf(t) >> 2;          // t in [0, 256): q = floor(t) in [0, 255]
}

// pool frame of ring r's input slot, or -1 when the ring or the slot is out of range
__device__ __forceinline__ long scene_input_slot(int r, int n_state, int span, int n_pool) {
  if (r < 0 || r >= n_state) return -1;
  const long slot = (long)r * (span + 2) + span + 1;
  return slot < (long)n_pool ? slot : -1;
}

__global__ __launch_bounds__(kThreads) void scene_zero_kernel(int *__restrict__ hist, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) hist[i] = 0;
}

__global__ __launch_bounds__(kThreads) void scene_hist_kernel(const float *__restrict__ pool, int n_pool, int n_pix,
                                                              const int *__restrict__ rings, int n_state, int span,
                                                              int *__restrict__ hist) {
  __shared__ int sh[kWaves][kBins];
  const int b = blockIdx.y, t = threadIdx.x;
  const long slot = scene_input_slot(rings[b], n_state, span, n_pool);
  if (slot < 0) return;   // uniform over the block
  sh[t >> 6][t & 63] = 0;
  __syncthreads();
  int *mine = sh[t >> 6];
  const float *frame = pool + (size_t)slot * 3 * (size_t)n_pix;
  // pixel p starts at float 3 p: the first p with a 16-byte aligned address is (a mod 4), a the frame's offset in floats
  const int a = (int)((reinterpret_cast<uintptr_t>(frame) >> 2) & 3);
  const int head = a < n_pix ? a : n_pix;
  const int n_quads = (n_pix - head) >> 2;
  const int tail = (n_pix - head) & 3;
  const float4 *q4 = reinterpret_cast<const float4 *>(frame + 3 * head);
  for (int q = blockIdx.x * kThreads + t; q < n_quads; q += gridDim.x * kThreads) {
    const float4 u = q4[3 * (size_t)q], v = q4[3 * (size_t)q + 1], w = q4[3 * (size_t)q + 2];
    atomicAdd(&mine[luma_bin(u.x, u.y, u.z)], 1);
    atomicAdd(&mine[luma_bin(u.w, v.x, v.y)], 1);
    atomicAdd(&mine[luma_bin(v.z, v.w, w.x)], 1);
    atomicAdd(&mine[luma_bin(w.y, w.z, w.w)], 1);
  }
  if (blockIdx.x == 0 && t < head + tail) {   // at most 6 pixels of the frame
    const int p = t < head ? t : n_pix - tail + (t - head);
    atomicAdd(&mine[luma_bin(frame[3 * (size_t)p], frame[3 * (size_t)p + 1], frame[3 * (size_t)p + 2])], 1);
  }
  __syncthreads();
  if (t < kBins) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += sh[w][t];
    if (c) atomicAdd(&hist[b * kBins + t], c);
  }
}

__global__ __launch_bounds__(kBins) void scene_decide_kernel(const int *__restrict__ hist, const int *__restrict__ rings,
                                                             int n_pool, SkipTable skip, int S, int *state, int n_state,
                                                             int thr_count, int min_len, float *zoom_state, float crop_start,
                                                             int *__restrict__ table, int *__restrict__ out_slots,
                                                             int *__restrict__ cut) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int span = skip.v[S - 1], hist_slots = span + 1;
  const int r = rings[b];
  if (scene_input_slot(r, n_state, span, n_pool) < 0) {   // the skipped-slot convention: no state is touched
    if (lane < S) table[b * S + lane] = -1;
    if (lane == 0) {
      out_slots[b] = -1;
      cut[b] = 0;
    }
    return;
  }
  int *st = state + (size_t)r * kStateInts;
  int k = st[0];
  const int cur = hist[b * kBins + lane];
  int d = k == 0 ? 0 : abs(cur - st[4 + lane]);   // no previous histogram at a ring's first frame
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
  const bool is_cut = k >= (min_len > 1 ? min_len : 1) && d >= thr_count;
  if (is_cut) k = 0;
  const int base = r * (span + 2);
  if (lane < S) {
    int e = base + hist_slots;                    // the input slot: every entry at step 0, the last entry always
    if (k > 0 && lane < S - 1) {
      const int j = k + skip.v[lane] - span;
      e = base + (j > 0 ? j : 0) % hist_slots;
    }
    table[b * S + lane] = e;
  }
  st[4 + lane] = cur;
  if (lane == 0) {
    out_slots[b] = base + k % hist_slots;
    cut[b] = is_cut ? 1 : 0;
    if (is_cut && zoom_state) zoom_state[r] = crop_start;
    st[0] = k + 1;
    st[1] += is_cut ? 1 : 0;
    st[2] = d;
    st[3] = 0;
  }
}

int check_scene_batch(const char *fn, int B) {
  DVSG_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d outside [1, 65535]", fn, B);
  return DVSG_OK;
}

}  // namespace
}  // namespace dvsg

using namespace dvsg;

extern "C" {

int dvsg_scene_workspace_bytes(int B, size_t *bytes) {
  const char *fn = "dvsg_scene_workspace_bytes";
  DVSG_REQUIRE(bytes, "%s: NULL bytes", fn);
  if (int rc = check_scene_batch(fn, B)) return rc;
  *bytes = (size_t)B * kBins * sizeof(int32_t);
  return DVSG_OK;
}

int dvsg_scene_step_f32(const float *pool, int n_pool, int H, int W, const int32_t *rings, int B, const int32_t *skip_host,
                        int S, int32_t *state, int n_state, int thr_count, int min_len, float *zoom_state, float crop_start,
                        int32_t *table, int32_t *out_slots, int32_t *cut, void *workspace, size_t workspace_bytes,
                        void *stream) {
  const char *fn = "dvsg_scene_step_f32";
  DVSG_REQUIRE(pool && rings && skip_host && state && table && out_slots && cut, "%s: NULL pointer", fn);
  if (int rc = check_scene_batch(fn, B)) return rc;
  DVSG_REQUIRE(S >= 1 && S <= kMaxSkip, "%s: S=%d outside [1, %d]", fn, S, kMaxSkip);
  DVSG_REQUIRE(n_pool >= 1 && n_state >= 1, "%s: n_pool=%d and n_state=%d must be >= 1", fn, n_pool, n_state);
  DVSG_REQUIRE(H >= 1 && W >= 1, "%s: frame size %dx%d must be positive", fn, H, W);
  DVSG_REQUIRE(2 * (long)H * W <= (long)INT_MAX, "%s: frame %dx%d too large: 2 H W must stay below 2^31 (S is an int32)", fn,
               H, W);
  const int n_pix = H * W;
  DVSG_REQUIRE(thr_count >= 1 && thr_count <= 2 * n_pix, "%s: thr_count=%d outside [1, 2 H W = %d]", fn, thr_count,
               2 * n_pix);
  DVSG_REQUIRE(min_len >= 0, "%s: min_len=%d must be >= 0", fn, min_len);
  SkipTable skip{};
  for (int s = 0; s < S; ++s) {
    skip.v[s] = skip_host[s];
    DVSG_REQUIRE(skip.v[s] >= 0 && (s == 0 || skip.v[s] > skip.v[s - 1]) && skip.v[s] < (1 << 20),
                 "%s: skip[%d]=%d: the skip lengths must be >= 0, increase strictly and stay below 2^20", fn, s, skip.v[s]);
  }
  const int span = skip.v[S - 1];
  DVSG_REQUIRE((long)n_state * (span + 2) <= (long)INT_MAX, "%s: n_state=%d rings of %d frames overflow an int32 slot", fn,
               n_state, span + 2);
  DVSG_REQUIRE(workspace, "%s: NULL workspace", fn);
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace must be 16-byte aligned", fn);
  const size_t need = (size_t)B * kBins * sizeof(int32_t);
  if (workspace_bytes < need)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (dvsg_scene_workspace_bytes)", fn, workspace_bytes,
                need);
  hipStream_t s = as_stream(stream);
  int *hist = static_cast<int *>(workspace);
  hipLaunchKernelGGL(scene_zero_kernel, dim3(ceil_div(B * kBins, kThreads)), dim3(kThreads), 0, s, hist, B * kBins);
  if (int rc = check_launch("scene_zero_kernel")) return rc;
  const int per_frame = ceil_div(n_pix, 4 * kQuadsPerThread * kThreads);
  dim3 grid(per_frame < kMaxBlocksPerFrame ? per_frame : kMaxBlocksPerFrame, B);
  hipLaunchKernelGGL(scene_hist_kernel, grid, dim3(kThreads), 0, s, pool, n_pool, n_pix, rings, n_state, span, hist);
  if (int rc = check_launch("scene_hist_kernel")) return rc;
  hipLaunchKernelGGL(scene_decide_kernel, dim3(B), dim3(kBins), 0, s, hist, rings, n_pool, skip, S, state, n_state, thr_count,
                     min_len, zoom_state, crop_start, table, out_slots, cut);
  return check_launch("scene_decide_kernel");
}

}  // extern "C"
