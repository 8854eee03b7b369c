// Shake measurement as gfx950 HIP kernels (dvsg_shake_measure_u8): the global motion between consecutive luma planes by block
// matching, integer work on bytes from the first kernel to the last.  The rule is stated in include/dvsg_amd.h ("SHAKE") and
// restated in NumPy in tests/shake_ref.py; after the one integer reduction every value is exact, so the bar is bit equality.
//
// Three launches on the legacy default stream, for all n frames and n - 1 pairs of a call at once:
//   shake_reduce_kernel  grid (column tiles x h, n).  A workgroup makes up to kSegBytes / f bytes of one reduced row: the f
//                        source rows of the tile are staged in LDS, each at the offset its global address has within 16 bytes,
//                        so every whole 16-byte unit of a row is one 16-byte load and one 16-byte LDS store; the bytes in front
//                        of the first and behind the last whole unit take a scalar path.  Nothing is padded and no byte
//                        outside the row's W used bytes is read.  Then one thread per reduced byte sums its f x f bytes.
//   shake_match_kernel   grid (n_blk, n - 1), one workgroup per block and pair.  The 16 x 16 block of the current plane and the
//                        (16 + 2R)^2 window of the previous one are staged in LDS once (the window at a row pitch of
//                        2R / 4 + 5 dwords).  A lane owns the candidates c = lane, lane + 256, ...: per block row it reads the
//                        five window dwords that hold its 16 bytes, forms the four dwords at its byte offset with
//                        v_alignbyte_b32 and accumulates |a - b| over them with v_sad_u8 against the block's dwords (an LDS
//                        broadcast).  All (2R + 1)^2 SADs stay in LDS as 16-bit values; the minimum is a reduction of one
//                        packed 64-bit key per lane, (S, dy^2 + dx^2, candidate index) from the high bits down, which is the
//                        order (S, dy^2 + dx^2, dy, dx); thread 0 reads the four neighbours back and writes the block's row.
//                        R is a run-time argument.
//   shake_global_kernel  grid (n - 1), one workgroup per pair: the block rows into LDS (an invalid block as INT_MAX), then the
//                        two lower medians by rank counting -- the rank of entry i is the number of entries below it plus the
//                        equal ones in front of it, so exactly one entry has rank (n_valid - 1) / 2.
// dvsg_shake_motion_u8 ("SHAKE MOTION", tests/shake_motion_ref.py) is the same call with another third launch:
//   shake_motion_kernel  grid (n - 1), one workgroup per pair: the same rows and medians (pair_medians, shared with
//                        shake_global_kernel), then every lane gates its blocks against the medians and adds up the nine sums
//                        of the similarity fit in int64 registers; __shfl_xor inside a wave, LDS across the four waves, thread
//                        0 writes the 13 values.  Integers only and no atomics: the order of the additions cannot matter.
#include <climits>
#include <cstdint>

#include "common.h"

namespace dvsg {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlock = 16;              // blocks are 16 x 16 on the reduced plane
constexpr int kMaxRadius = 16;
constexpr int kMaxFactor = 16;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxFrames = 4096;
constexpr int kMaxSide = 16384;
constexpr int kSegBytes = 2048;         // source bytes of one row that a reduce workgroup stages
constexpr int kSegPitch = kSegBytes + 32;   // + the row's offset within 16 bytes (at most 15), rounded to 16
constexpr int kMaxWinPitch = 2 * kMaxRadius / 4 + 5;   // dwords
constexpr int kMaxCand = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);

struct Geometry {
  int h, w, ny, nx, n_blk;
  size_t plane_stride;   // bytes from one reduced plane to the next: h w rounded up to 16
  size_t blocks_off, vectors_off, bytes;
  size_t motion_bytes;   // of dvsg_shake_motion_u8: int64 [n - 1, 13] at vectors_off in place of the vectors
};

__global__ __launch_bounds__(kThreads) void shake_reduce_kernel(const uint8_t *__restrict__ luma, size_t pitch,
                                                                size_t frame_stride, int h, int w, int f, int tiles,
                                                                uint8_t *__restrict__ red, size_t plane_stride) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sh[];   // [f][kSegPitch]
  const int t = threadIdx.x;
  const int tile = blockIdx.x % tiles, i = blockIdx.x / tiles, frame = blockIdx.y;
  const int tile_w = kSegBytes / f;                    // reduced bytes per tile
  const int c0 = tile * tile_w;
  const int cols = min(tile_w, w - c0);
  const int seg = cols * f;                            // source bytes per row, <= kSegBytes
  const uint8_t *src0 = luma + (size_t)frame * frame_stride + (size_t)i * f * pitch + (size_t)c0 * f;
  for (int k = 0; k < f; ++k) {
    const uint8_t *src = src0 + k * pitch;
    const int a = (int)(reinterpret_cast<uintptr_t>(src) & 15);
    uint8_t *dst = sh + k * kSegPitch + a;             // dst and src agree mod 16
    const int head = min((16 - a) & 15, seg);
    const int units = (seg - head) >> 4;
    const int tail = seg - head - (units << 4);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (int u = t; u < units; u += kThreads) d4[u] = s4[u];
    if (t < head) dst[t] = src[t];
    if (t >= 32 && t - 32 < tail) dst[seg - tail + (t - 32)] = src[seg - tail + (t - 32)];
  }
  __syncthreads();
  const int area = f * f;
  for (int c = t; c < cols; c += kThreads) {
    int sum = 0;
    for (int k = 0; k < f; ++k) {
      const uint8_t *row = sh + k * kSegPitch + (int)(reinterpret_cast<uintptr_t>(src0 + k * pitch) & 15) + c * f;
      for (int j = 0; j < f; ++j) sum += row[j];
    }
    red[(size_t)frame * plane_stride + (size_t)i * w + c0 + c] = (uint8_t)((sum + area / 2) / area);
  }
}

__device__ __forceinline__ int floor_div(int a, int b) {   // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void shake_match_kernel(const uint8_t *__restrict__ red, size_t plane_stride, int w,
                                                               int nx, int n_blk, int R, int margin_y, int margin_x,
                                                               int texture, int32_t *__restrict__ blocks) {
  __shared__ uint32_t cur[kBlock * kBlock / 4];
  __shared__ uint32_t win[(kBlock + 2 * kMaxRadius) * kMaxWinPitch];
  __shared__ uint16_t sad[kMaxCand];
  __shared__ unsigned long long wave_key[kWaves];
  const int t = threadIdx.x;
  const int blk = blockIdx.x, pair = blockIdx.y;
  const int y0 = margin_y + kBlock * (blk / nx), x0 = margin_x + kBlock * (blk % nx);
  const uint8_t *prev_plane = red + (size_t)pair * plane_stride;
  const uint8_t *cur_plane = prev_plane + plane_stride;
  const int side = kBlock + 2 * R;          // rows and used bytes per row of the window
  const int wp = 2 * R / 4 + 5;             // its row pitch in dwords: 4 wp >= side + 1
  const int D = 2 * R + 1, n_cand = D * D;
  {
    const uint8_t *p = cur_plane + (size_t)(y0 + (t >> 4)) * w + x0 + (t & 15);
    reinterpret_cast<uint8_t *>(cur)[t] = *p;
  }
  uint8_t *win_b = reinterpret_cast<uint8_t *>(win);
  for (int idx = t; idx < side * wp * 4; idx += kThreads) {
    const int r = idx / (wp * 4), c = idx - r * (wp * 4);
    win_b[idx] = c < side ? prev_plane[(size_t)(y0 - R + r) * w + (x0 - R + c)] : (uint8_t)0;
  }
  __syncthreads();
  unsigned long long best = ~0ull;
  for (int c = t; c < n_cand; c += kThreads) {
    const int cy = c / D, cx = c - cy * D;          // dy + R, dx + R
    const uint32_t shift = (uint32_t)(cx & 3);
    const uint32_t *wrow = win + cy * wp + (cx >> 2);
    uint32_t s = 0;
#pragma unroll 4
    for (int i = 0; i < kBlock; ++i) {
      const uint32_t w0 = wrow[0], w1 = wrow[1], w2 = wrow[2], w3 = wrow[3], w4 = wrow[4];
      s = __builtin_amdgcn_sad_u8(cur[4 * i + 0], __builtin_amdgcn_alignbyte(w1, w0, shift), s);
      s = __builtin_amdgcn_sad_u8(cur[4 * i + 1], __builtin_amdgcn_alignbyte(w2, w1, shift), s);
      s = __builtin_amdgcn_sad_u8(cur[4 * i + 2], __builtin_amdgcn_alignbyte(w3, w2, shift), s);
      s = __builtin_amdgcn_sad_u8(cur[4 * i + 3], __builtin_amdgcn_alignbyte(w4, w3, shift), s);
      wrow += wp;
    }
    sad[c] = (uint16_t)s;                           // at most 256 * 255 = 65280
    const int dy = cy - R, dx = cx - R;
    const unsigned long long key = ((unsigned long long)s << 21) | ((unsigned long long)(dy * dy + dx * dx) << 11) | (unsigned)c;
    best = key < best ? key : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off);
    best = o < best ? o : best;
  }
  if ((t & 63) == 0) wave_key[t >> 6] = best;
  __syncthreads();                                  // the SAD table is complete as well
  if (t != 0) return;
#pragma unroll
  for (int k = 1; k < kWaves; ++k) best = wave_key[k] < best ? wave_key[k] : best;
  const int c = (int)(best & 2047u);
  const int cy = c / D, cx = c - cy * D;
  int vx = 0, vy = 0, valid = 0;
  if (cy > 0 && cy < D - 1 && cx > 0 && cx < D - 1) {   // not on the search boundary: the four neighbours exist
    const int s0 = sad[c], sxm = sad[c - 1], sxp = sad[c + 1], sym = sad[c - D], syp = sad[c + D];
    const int curv_x = sxm - 2 * s0 + sxp, curv_y = sym - 2 * s0 + syp;
    const int need = texture > 1 ? texture : 1;
    if (curv_x >= need && curv_y >= need) {
      vx = 16 * (cx - R) + floor_div(16 * (sxm - sxp) + curv_x, 2 * curv_x);
      vy = 16 * (cy - R) + floor_div(16 * (sym - syp) + curv_y, 2 * curv_y);
      valid = 1;
    }
  }
  int32_t *row = blocks + ((size_t)pair * n_blk + blk) * 3;
  row[0] = vx;
  row[1] = vy;
  row[2] = valid;
}

// The block rows of one pair into LDS (an invalid block as INT_MAX in both) and the two lower medians into median[0..1] by
// rank counting; returns n_valid.  Ends with the barrier that publishes the medians and the rows.
__device__ __forceinline__ int pair_medians(const int32_t *__restrict__ rows, int n_blk, int *vx, int *vy, int *median,
                                            int *counts) {
  const int t = threadIdx.x;
  int mine = 0;
  for (int i = t; i < n_blk; i += kThreads) {
    const int ok = rows[3 * i + 2];
    vx[i] = ok ? rows[3 * i] : INT_MAX;
    vy[i] = ok ? rows[3 * i + 1] : INT_MAX;
    mine += ok;
  }
  if (t < 2) median[t] = 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
  if ((t & 63) == 0) counts[t >> 6] = mine;
  __syncthreads();
  int valid = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) valid += counts[k];
  const int target = (valid - 1) / 2;
  for (int i = t; i < n_blk && valid > 0; i += kThreads) {
    const int a = vx[i], b = vy[i];
    if (a == INT_MAX) continue;
    int ra = 0, rb = 0;
    for (int j = 0; j < n_blk; ++j) {
      const int p = vx[j], q = vy[j];
      ra += (p < a || (p == a && j < i)) ? 1 : 0;
      rb += (q < b || (q == b && j < i)) ? 1 : 0;
    }
    if (ra == target) median[0] = a;
    if (rb == target) median[1] = b;
  }
  __syncthreads();
  return valid;
}

__global__ __launch_bounds__(kThreads) void shake_global_kernel(const int32_t *__restrict__ blocks, int n_blk, int min_blocks,
                                                                int32_t *__restrict__ vectors) {
  __shared__ int vx[kMaxBlocks], vy[kMaxBlocks];
  __shared__ int median[2], counts[kWaves];
  const int t = threadIdx.x, pair = blockIdx.x;
  const int valid = pair_medians(blocks + (size_t)pair * n_blk * 3, n_blk, vx, vy, median, counts);
  if (t == 0) {
    const int ok = valid >= min_blocks ? 1 : 0;
    int32_t *row = vectors + (size_t)pair * 4;
    row[0] = ok ? median[0] : 0;
    row[1] = ok ? median[1] : 0;
    row[2] = valid;
    row[3] = ok;
  }
}

constexpr int kMotionSums = 9;            // n_in, Sx, Sy, Su, Sv, Sxx, Sxu, Sxv, Suu
constexpr int kMotionRow = 4 + kMotionSums;
constexpr int kMaxGate = 1 << 20;

__global__ __launch_bounds__(kThreads) void shake_motion_kernel(const int32_t *__restrict__ blocks, int n_blk, int nx,
                                                                int min_blocks, int gate, long long *__restrict__ motion) {
  __shared__ int vx[kMaxBlocks], vy[kMaxBlocks];
  __shared__ int median[2], counts[kWaves];
  __shared__ long long wave_sum[kWaves][kMotionSums];
  const int t = threadIdx.x, pair = blockIdx.x;
  const int valid = pair_medians(blocks + (size_t)pair * n_blk * 3, n_blk, vx, vy, median, counts);
  const int ok = valid >= min_blocks ? 1 : 0;
  const int gx = ok ? median[0] : 0, gy = ok ? median[1] : 0;
  const int ny = n_blk / nx;
  long long s[kMotionSums];
#pragma unroll
  for (int k = 0; k < kMotionSums; ++k) s[k] = 0;
  for (int i = t; i < n_blk && ok; i += kThreads) {
    const int u = vx[i], v = vy[i];
    if (u == INT_MAX || abs(u - gx) > gate || abs(v - gy) > gate) continue;   // |u|, |v| <= 248: no overflow
    const int a = i / nx, c = i - a * nx;
    const int X = 2 * c - (nx - 1), Y = 2 * a - (ny - 1);                      // |X|, |Y| <= 2047: the products fit an int
    s[0] += 1;
    s[1] += X;
    s[2] += Y;
    s[3] += u;
    s[4] += v;
    s[5] += X * X + Y * Y;
    s[6] += X * u + Y * v;
    s[7] += X * v - Y * u;
    s[8] += u * u + v * v;
  }
#pragma unroll
  for (int k = 0; k < kMotionSums; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
    if ((t & 63) == 0) wave_sum[t >> 6][k] = s[k];
  }
  __syncthreads();
  if (t != 0) return;
  long long *row = motion + (size_t)pair * kMotionRow;
  row[0] = gx;
  row[1] = gy;
  row[2] = valid;
  row[3] = ok;
#pragma unroll
  for (int k = 0; k < kMotionSums; ++k) {
    long long sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += wave_sum[w][k];
    row[4 + k] = sum;
  }
}

size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// Everything about the geometry that can be refused, before any HIP call; fills g.
int shake_geometry(const char *fn, int n, int H, int W, int factor, int radius, int margin_y, int margin_x, Geometry *g) {
  DVSG_REQUIRE(n >= 2 && n <= kMaxFrames, "%s: n=%d outside [2, %d] (a pair needs two frames; feed long clips in chunks)", fn, n,
               kMaxFrames);
  DVSG_REQUIRE(H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide, "%s: frame size %dx%d outside [1, %d]", fn, H, W, kMaxSide);
  DVSG_REQUIRE(factor >= 1 && factor <= kMaxFactor, "%s: factor=%d outside [1, %d]", fn, factor, kMaxFactor);
  DVSG_REQUIRE(radius >= 1 && radius <= kMaxRadius, "%s: radius=%d outside [1, %d]", fn, radius, kMaxRadius);
  DVSG_REQUIRE(margin_y >= radius && margin_x >= radius, "%s: margin_y=%d and margin_x=%d must be at least radius=%d", fn,
               margin_y, margin_x, radius);
  g->h = H / factor;
  g->w = W / factor;
  const int rows = g->h - 2 * margin_y, cols = g->w - 2 * margin_x;
  g->ny = rows > 0 ? rows / kBlock : 0;
  g->nx = cols > 0 ? cols / kBlock : 0;
  const long n_blk = (long)g->ny * g->nx;
  DVSG_REQUIRE(n_blk >= 1, "%s: no 16 x 16 block fits: the reduced plane is %dx%d (factor=%d) with margins %d, %d", fn, g->h, g->w,
               factor, margin_y, margin_x);
  DVSG_REQUIRE(n_blk <= kMaxBlocks, "%s: %ld blocks (%d x %d), at most %d: raise factor=%d", fn, n_blk, g->ny, g->nx, kMaxBlocks,
               factor);
  g->n_blk = (int)n_blk;
  g->plane_stride = round16((size_t)g->h * g->w);
  g->blocks_off = (size_t)n * g->plane_stride;
  g->vectors_off = g->blocks_off + round16((size_t)(n - 1) * g->n_blk * 3 * sizeof(int32_t));
  g->bytes = g->vectors_off + (size_t)(n - 1) * 4 * sizeof(int32_t);
  g->motion_bytes = g->vectors_off + (size_t)(n - 1) * kMotionRow * sizeof(int64_t);
  return DVSG_OK;
}

// What both calls check after their NULL pointers, before any HIP call; `need` is g.bytes or g.motion_bytes of the geometry
// it fills and `query` the function that reports it.
int shake_check(const char *fn, const char *query, size_t Geometry::*need, size_t pitch, size_t frame_stride, int n, int H, int W,
                int factor, int radius, int margin_y, int margin_x, int texture, int min_blocks, const void *workspace,
                size_t workspace_bytes, Geometry *g) {
  if (int rc = shake_geometry(fn, n, H, W, factor, radius, margin_y, margin_x, g)) return rc;
  DVSG_REQUIRE(pitch >= (size_t)W, "%s: pitch=%zu below W=%d", fn, pitch, W);
  DVSG_REQUIRE(frame_stride >= (size_t)(H - 1) * pitch + (size_t)W, "%s: frame_stride=%zu below a frame's (H - 1) pitch + W = %zu",
               fn, frame_stride, (size_t)(H - 1) * pitch + (size_t)W);
  DVSG_REQUIRE(texture >= 0, "%s: texture=%d must be >= 0", fn, texture);
  DVSG_REQUIRE(min_blocks >= 1, "%s: min_blocks=%d must be >= 1", fn, min_blocks);
  DVSG_REQUIRE(workspace, "%s: NULL workspace", fn);
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace must be 16-byte aligned", fn);
  if (workspace_bytes < g->*need)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", fn, workspace_bytes, g->*need, query);
  return DVSG_OK;
}

// The wait for the device and the two launches that both calls share: the reduced planes and the block rows.
int shake_blocks(const Geometry &g, const uint8_t *luma, size_t pitch, size_t frame_stride, int n, int factor, int radius,
                 int margin_y, int margin_x, int texture, uint8_t *red, int32_t *blocks) {
  DVSG_HIP(hipDeviceSynchronize());   // whatever stream made the planes has finished
  const int tile_w = kSegBytes / factor;
  const int tiles = ceil_div(g.w, tile_w);
  hipLaunchKernelGGL(shake_reduce_kernel, dim3((unsigned)tiles * g.h, n), dim3(kThreads), (size_t)factor * kSegPitch, nullptr, luma,
                     pitch, frame_stride, g.h, g.w, factor, tiles, red, g.plane_stride);
  if (int rc = check_launch("shake_reduce_kernel")) return rc;
  hipLaunchKernelGGL(shake_match_kernel, dim3(g.n_blk, n - 1), dim3(kThreads), 0, nullptr, red, g.plane_stride, g.w, g.nx, g.n_blk,
                     radius, margin_y, margin_x, texture, blocks);
  return check_launch("shake_match_kernel");
}

}  // namespace
}  // namespace dvsg

using namespace dvsg;

extern "C" {

int dvsg_shake_workspace_bytes(int n, int H, int W, int factor, int radius, int margin_y, int margin_x, size_t *bytes) {
  const char *fn = "dvsg_shake_workspace_bytes";
  DVSG_REQUIRE(bytes, "%s: NULL bytes", fn);
  Geometry g;
  if (int rc = shake_geometry(fn, n, H, W, factor, radius, margin_y, margin_x, &g)) return rc;
  *bytes = g.bytes;
  return DVSG_OK;
}

int dvsg_shake_measure_u8(const uint8_t *luma, size_t pitch, size_t frame_stride, int n, int H, int W, int factor, int radius,
                          int margin_y, int margin_x, int texture, int min_blocks, int32_t *vectors_host, int32_t *blocks_host,
                          void *workspace, size_t workspace_bytes) {
  const char *fn = "dvsg_shake_measure_u8";
  DVSG_REQUIRE(luma && vectors_host, "%s: NULL pointer", fn);
  Geometry g;
  if (int rc = shake_check(fn, "dvsg_shake_workspace_bytes", &Geometry::bytes, pitch, frame_stride, n, H, W, factor, radius, margin_y,
                           margin_x, texture, min_blocks, workspace, workspace_bytes, &g))
    return rc;
  uint8_t *red = static_cast<uint8_t *>(workspace);
  int32_t *blocks = reinterpret_cast<int32_t *>(red + g.blocks_off);
  int32_t *vectors = reinterpret_cast<int32_t *>(red + g.vectors_off);
  const int pairs = n - 1;
  if (int rc = shake_blocks(g, luma, pitch, frame_stride, n, factor, radius, margin_y, margin_x, texture, red, blocks)) return rc;
  hipLaunchKernelGGL(shake_global_kernel, dim3(pairs), dim3(kThreads), 0, nullptr, blocks, g.n_blk, min_blocks, vectors);
  if (int rc = check_launch("shake_global_kernel")) return rc;
  // hipMemcpy waits for the legacy default stream
  DVSG_HIP(hipMemcpy(vectors_host, vectors, (size_t)pairs * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (blocks_host)
    DVSG_HIP(hipMemcpy(blocks_host, blocks, (size_t)pairs * g.n_blk * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DVSG_OK;
}

int dvsg_shake_motion_workspace_bytes(int n, int H, int W, int factor, int radius, int margin_y, int margin_x, size_t *bytes) {
  const char *fn = "dvsg_shake_motion_workspace_bytes";
  DVSG_REQUIRE(bytes, "%s: NULL bytes", fn);
  Geometry g;
  if (int rc = shake_geometry(fn, n, H, W, factor, radius, margin_y, margin_x, &g)) return rc;
  *bytes = g.motion_bytes;
  return DVSG_OK;
}

int dvsg_shake_motion_u8(const uint8_t *luma, size_t pitch, size_t frame_stride, int n, int H, int W, int factor, int radius,
                         int margin_y, int margin_x, int texture, int min_blocks, int gate, int64_t *motion_host,
                         int32_t *blocks_host, void *workspace, size_t workspace_bytes) {
  const char *fn = "dvsg_shake_motion_u8";
  DVSG_REQUIRE(luma, "%s: NULL luma", fn);
  DVSG_REQUIRE(motion_host, "%s: NULL motion_host", fn);
  DVSG_REQUIRE(gate >= 0 && gate <= kMaxGate, "%s: gate=%d outside [0, %d]", fn, gate, kMaxGate);
  Geometry g;
  if (int rc = shake_check(fn, "dvsg_shake_motion_workspace_bytes", &Geometry::motion_bytes, pitch, frame_stride, n, H, W, factor,
                           radius, margin_y, margin_x, texture, min_blocks, workspace, workspace_bytes, &g))
    return rc;
  uint8_t *red = static_cast<uint8_t *>(workspace);
  int32_t *blocks = reinterpret_cast<int32_t *>(red + g.blocks_off);
  long long *motion = reinterpret_cast<long long *>(red + g.vectors_off);
  const int pairs = n - 1;
  if (int rc = shake_blocks(g, luma, pitch, frame_stride, n, factor, radius, margin_y, margin_x, texture, red, blocks)) return rc;
  hipLaunchKernelGGL(shake_motion_kernel, dim3(pairs), dim3(kThreads), 0, nullptr, blocks, g.n_blk, g.nx, min_blocks, gate, motion);
  if (int rc = check_launch("shake_motion_kernel")) return rc;
  // hipMemcpy waits for the legacy default stream
  DVSG_HIP(hipMemcpy(motion_host, motion, (size_t)pairs * kMotionRow * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (blocks_host)
    DVSG_HIP(hipMemcpy(blocks_host, blocks, (size_t)pairs * g.n_blk * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DVSG_OK;
}

}  // extern "C"
