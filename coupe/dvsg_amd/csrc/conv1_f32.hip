// The root conv in exact float32 (conv1.hip describes the root): one output row per workgroup (conv1_kernel), row pairs
// in bands with or without the max pool in the epilogue (root_band_kernel, root_band_pool_kernel) and that pool's seams
// (root_pool_seams_kernel), and the kernel for any other window length (rootconv_kernel).
#include "conv1_device.h"
#include "conv1_internal.h"

namespace dvsg {
namespace {

static_assert(C1_TILE == kConv1Tile, "conv1.hip sizes the grid's column tiles by kConv1Tile");
#ifdef DVSG_STAMPS  // diagnostic build (tools/stamp_probe_conv1.py): this file's stamp buffer, read by dvsg_debug_read_conv1_stamps
__device__ unsigned long long g_c1_stamps[8 * 65536];
#endif

template <int NW, typename TO, int SRC>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW / 2, NW / 2)))
void conv1_kernel(const Conv1Src src, const float *__restrict__ wt1, const float *__restrict__ bias,
                  TO *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles) {
  constexpr int NT = 64 * NW;
  constexpr int MI = 4 / (NW / 2);                       // 32-pixel MFMA blocks per wave: 2 or 1
  constexpr int IN4 = (C1_SEG_PAD / 4 + NT - 1) / NT;    // 6 or 3 groups of four elements per thread per kernel row
  constexpr int WLOADS = (C1_WELEMS / 4 + NT - 1) / NT;  // 10 or 5 float4
  static_assert(C1_TILE * C1_LDC <= C1_WELEMS, "epilogue tile must fit in the weight stage");
  __shared__ __attribute__((aligned(16))) float w_s[C1_WELEMS];
  __shared__ __attribute__((aligned(16))) float in_s[C1_SEG_PAD];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  const Conv1Tile tile = conv1_tile(wtiles, Ho);
  const int b = tile.b, ho = tile.ho, wo0 = tile.wo0;

  typedef typename Conv1RowSel<NT, IN4, SRC>::type Row;
  Row row;
  row.init(src, tid, b, wo0, H, W, C1_SEG_PAD);
  if constexpr (Row::kRing) {   // elements the scatter never writes (the zero tap's slot, the tail) must be finite
    for (int e = tid; e < C1_SEG_PAD; e += NT) in_s[e] = 0.f;
  }
  typename Row::Data rd;
  floatx4 w_reg[WLOADS];
  auto load_stage = [&](int kh) __attribute__((always_inline)) {
    row.load(rd, 2 * ho + kh - 3);
    const floatx4 *wsrc = reinterpret_cast<const floatx4 *>(wt1 + (size_t)kh * C1_WELEMS);
#pragma unroll
    for (int i = 0; i < WLOADS; ++i) {
      const int q = tid + NT * i;
      w_reg[i] = wsrc[q < C1_WELEMS / 4 ? q : 0];
    }
  };
  auto store_stage = [&]() __attribute__((always_inline)) {
    if constexpr (Row::kRing) {
      row.scatter(rd, [&](int e, float v) __attribute__((always_inline)) { in_s[e] = v; });
    } else {
#pragma unroll
      for (int i = 0; i < IN4; ++i) {
        const int q = tid + NT * i;
        const floatx4 v = row.scaled(rd, i);
        if (q < C1_SEG_PAD / 4) reinterpret_cast<floatx4 *>(in_s)[q] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < WLOADS; ++i) {
      const int q = tid + NT * i;
      if (q < C1_WELEMS / 4) reinterpret_cast<floatx4 *>(w_s)[q] = w_reg[i];
    }
  };

  // Two accumulators per block, even and odd taps: 1029 products through ONE float32 accumulator are 518 dependent
  // roundings of a partial sum that, when the products share a sign, grows to the value itself -- measured 37.8 x 2^-24 of
  // the value against float64 (tests/test_root_head_f64.py), past tau(K) = 36.1.  Two chains of half the length and half
  // the magnitude, added once in the epilogue, halve that, and give the matrix pipe 2 MI independent chains.
  floatx16 acc[MI], acc2[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[mi][q] = acc2[mi][q] = 0.f;

#ifdef DVSG_STAMPS
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long t_begin = C1_STAMP(), r_begin = __builtin_amdgcn_s_memrealtime();
#endif
  load_stage(0);
#ifdef DVSG_STAMPS
  st[0] = C1_STAMP() - t_begin;  // prologue (index setup) + first load issue
#endif
  for (int kh = 0; kh < 7; ++kh) {
#ifdef DVSG_STAMPS  // (each stamp drains lgkmcnt: the phase times below are upper bounds)
    const unsigned long long s0 = C1_STAMP();
    __syncthreads();
    const unsigned long long s1 = C1_STAMP();
    store_stage();
    const unsigned long long s2 = C1_STAMP();
    __syncthreads();
    const unsigned long long s3 = C1_STAMP();
    if (kh + 1 < 7) load_stage(kh + 1);
    const unsigned long long s4 = C1_STAMP();
    st[1] += s1 - s0;  // barrier 1 (+ vmcnt(0): the prefetched row and weights)
    st[2] += s2 - s1;  // scale + LDS stores
    st[3] += s3 - s2;  // barrier 2
    st[4] += s4 - s3;  // issue of the next row's loads
#else
    __syncthreads();  // everyone is done reading the previous kernel row
    store_stage();
    __syncthreads();
    if (kh + 1 < 7) load_stage(kh + 1);
#endif
    __builtin_amdgcn_sched_barrier(0);  // prefetch stays ahead of the MFMA loop
    const float *a0 = in_s + 2 * kConv1Cin * (wm * 32 * MI + r) + 2 * h;
    const float *bp = w_s + (wn * 32 + r) * kConv1Ld + 2 * h;
    // software-pipelined: the operands of step u + 1 are requested before the MFMAs of step u are issued (the
    // compiler's own schedule waits for each step's reads with nothing else in flight)
    constexpr int STEPS = kConv1Kpad / 4, PAIRS = (STEPS + 1) / 2;   // two steps per request: one ds_read2_b64 per operand
    float2 va[2][2][MI], vb[2][2];
    auto read_pair = [&](int slot, int g) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (2 * g + j >= STEPS) break;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          va[slot][j][mi] = *reinterpret_cast<const float2 *>(a0 + mi * (2 * kConv1Cin * 32) + 4 * (2 * g + j));
        vb[slot][j] = *reinterpret_cast<const float2 *>(bp + 4 * (2 * g + j));
      }
    };
    read_pair(0, 0);
#pragma unroll
    for (int g = 0; g < PAIRS; ++g) {
      if (g + 1 < PAIRS) read_pair((g + 1) & 1, g + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (2 * g + j >= STEPS) break;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[mi] = mfma32(va[g & 1][j][mi].x, vb[g & 1][j].x, acc[mi]);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc2[mi] = mfma32(va[g & 1][j][mi].y, vb[g & 1][j].y, acc2[mi]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

#ifdef DVSG_STAMPS
  const unsigned long long t_loop_end = C1_STAMP();
#endif
  // ---- epilogue: transpose through the (idle) weight stage so stores are float4s along channels
  float *Cs = w_s;
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
    C1_TILE_PUT(Cs, wm * 32 * MI + mi * 32, wn * 32, acc[mi][q] + acc2[mi][q]);
  __syncthreads();
  TO *yrow = y + (((size_t)b * Ho + ho) * Wo + wo0) * 64 + 4 * (tid & 15);
  conv1_tile_out<NT / 16>(Cs, conv1_tile_bias(bias, tid), tid, wo0, Wo,
                          [&](int row, float4 v) __attribute__((always_inline)) { store4(yrow + (size_t)row * 64, v); });
#ifdef DVSG_STAMPS
  if (tid == 0 && blockIdx.x < 65536) {
    unsigned long long *o = g_c1_stamps + (size_t)blockIdx.x * 8;
    const unsigned long long t_end = C1_STAMP();
    o[0] = st[0]; o[1] = st[1]; o[2] = st[2]; o[3] = st[3]; o[4] = st[4];
    o[5] = t_loop_end - t_begin;            // up to the end of the last MFMA loop
    o[6] = t_end - t_begin;                 // lifetime (stores issued, not necessarily landed)
    o[7] = __builtin_amdgcn_s_memrealtime() - r_begin;
  }
#endif
}

// ----------------------------------------------------------------------------------------
// conv1 in exact float32 for big launches: one workgroup of 8 waves per CU owns a 128-pixel column tile and walks down a
// BAND of output-row pairs (ho, ho + 1).  A wave is (row of the pair, pixel half, channel half) with two 32-pixel MFMA
// blocks: conv1_kernel<4, float, SRC>'s wave, operands, instruction and order of summation -- kh ascending, steps
// ascending, even taps into one chain and odd taps into the other, the chains joined once, then bias and ReLU -- so every
// output element is that kernel's, bit for bit (tests/test_root_band.py).  What differs is what surrounds the MFMA loops:
//   * step t = 0..6 of a pair is kernel row kh = t of BOTH rows: the upper row reads input row 2 ho + t - 3, the lower
//     one input row 2 ho + t - 1.  Input row 2 ho - 3 + i (i = 0..8) is the lower row's operand at step i - 2 and the upper
//     row's at step i: nine input rows and seven weight rows staged per pair where two one-row tiles stage fourteen of each;
//   * three input-row slots (row i in slot i mod 3: step t reads rows t and t + 2, row t + 1 waits in the third) and two
//     weight-row buffers: 3 x 21 952 + 2 x 38 400 = 142 656 bytes, one workgroup per CU.  Weight row t + 1 goes from its
//     prefetch registers into the idle buffer in the middle of step t's MFMAs, behind no barrier of its own; input row
//     t + 3 is fetched under step t's MFMAs and written into the slot step t frees, between the step's two barriers: 3
//     ds_write_b128 per thread there where the one-row kernel writes 16;
//   * the index set-up (Row::init depends on the column tile only) runs once per band, the next pair's first three rows and
//     first weight row are requested before the pair's output leaves (as soon as the accumulators have given up their
//     registers), and the epilogue is the shared one, a transpose tile per row in the two weight buffers.
// A band's last pair may have no lower row (Ho odd): its waves multiply rows that Row::load clamps into the image and
// nothing of theirs is stored.  Band `i` of a column tile holds ppb pairs if i < nbig, else ppb - 1 (launch_conv1).
// ----------------------------------------------------------------------------------------
constexpr int RB_NT = 512;
constexpr int RB_IN4 = (C1_SEG_PAD / 4 + RB_NT - 1) / RB_NT;     // 3 groups of four elements per thread and input row
constexpr int RB_WLOADS = (C1_WELEMS / 4 + RB_NT - 1) / RB_NT;   // 5 float4 per thread and weight row
constexpr int RB_SLOTS = 3;
constexpr size_t RB_LDS = sizeof(float) * (size_t)(2 * C1_WELEMS + RB_SLOTS * C1_SEG_PAD);   // 142 656 bytes
static_assert(RB_LDS <= 160 * 1024, "the band kernel's LDS must fit a CU");

// root_band_pool_kernel (root_band_kernel.inc with RB_POOL, the same text otherwise): the root's 3x3 / stride 2 max pool in the pair's epilogue, for Ho and Wo even (TF 'SAME' then
// pads nothing on the top and the left: pooled element (r, c) is the max of conv rows 2r .. 2r + 2 x columns 2c .. 2c + 2
// that exist).  Pooled row r is pair r and the upper row of pair r + 1, and a column tile's 128 conv columns are its 64
// pooled columns plus, for the last of them, column 0 of the tile to the right.  At a pair's epilogue both rows sit in the
// transpose tiles; thread (pooled column lc, channels 4 col4 .. + 3) forms, after conv1_tile_out's own bias and ReLU per
// tap, the 3-wide maxima `hu` and `hl` of the upper and the lower row over the tile's own columns, finishes pooled row
// p - 1 as max(carry, hu) and leaves carry = max(hu, hl) for the pair after this one.  The carry, 64 pooled columns x 64
// channels, lives in 16 KB of LDS behind the input slots (159 040 bytes in all) and every entry is read and written by
// one thread only: no barrier.  In registers it would be 8 VGPRs alive through the MFMA loops, where the frame ring's
// instantiations stand at 252 and 253 of 256 registers already, and through the pooled tensor it would be a second store and a
// load per element (profiles/r26_root_pool_resources.txt).
// What another workgroup owns is never waited for.  The pooled elements that need it are stored as the max over the taps
// this workgroup owns -- column 64 j + 63 of tile j where conv column 128 (j + 1) exists, and a band's last pooled row
// where the next band's first conv row exists -- and the conv values a neighbour misses go to their ordinary places in
// the conv1 output tensor `y`, of which nothing else is written: conv column 128 j of every row for j >= 1, and the first
// conv row of every band but the first.  root_pool_seams_kernel finishes those elements on the same stream.
// The max of values that are never NaN (ReLU: fmaxf(NaN, 0) = 0) with -0 < +0 (v_max_f32) does not depend on the order
// of the taps: every pooled element is maxpool_kernel's, bit for bit (tests/test_root_pool_fused.py).
constexpr int RB_CARRY = 64 * 64;                                // floats: one horizontally pooled row of a tile
constexpr size_t RB_POOL_LDS = RB_LDS + sizeof(float) * RB_CARRY;   // 159 040 bytes
static_assert(RB_POOL_LDS <= 160 * 1024, "the pooling band kernel's LDS must fit a CU");

#define RB_KERNEL root_band_kernel
#define RB_POOL 0
#include "root_band_kernel.inc"
#undef RB_KERNEL
#undef RB_POOL
#define RB_KERNEL root_band_pool_kernel
#define RB_POOL 1
#include "root_band_kernel.inc"
#undef RB_KERNEL
#undef RB_POOL

// The pooled elements root_band_pool_kernel left as partial maxima, finished from the conv values it stored for them (`a`,
// the conv1 output tensor's addresses).  One thread = one pooled pixel x 4 channels, in two ranges:
//   [0, n_col): the column seams -- (b, r, s) with pooled column c = 64 s + 63, s < ncs = the column tiles but the last.  The
//     taps missing are conv column 2c + 2 = 128 (s + 1) of rows 2r, 2r + 1 and 2r + 2; if r is also the last row of a band
//     but the last, conv row 2r + 2 at columns 2c and 2c + 1 too;
//   [n_col, total): the row seams -- (b, k, c) with pooled row r = (first pair of band k + 1) - 1, k < bands - 1, every c but
//     the column seams: conv row 2r + 2 at columns 2c, 2c + 1 and, inside the row, 2c + 2.
// Band i starts at pair i ppb - max(i - nbig, 0), as in the band kernel.  In place: each element is read and written by its
// own thread.
__global__ __launch_bounds__(256) void root_pool_seams_kernel(const float *__restrict__ a, float *__restrict__ y, int Ho, int Wo,
                                                             int ncs, int bands, int ppb, int nbig, size_t n_col,
                                                             size_t total) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int Hp = Ho >> 1, Wp = Wo >> 1;
  const int c4 = (int)(e & 15);
  auto band_start = [&](int i) { return i * ppb - (i > nbig ? i - nbig : 0); };
  int r, c;
  size_t b;
  bool col_seam, row_seam;
  if (e < n_col) {
    size_t t = e >> 4;
    c = 64 * (int)(t % ncs) + 63;
    t /= ncs;
    r = (int)(t % Hp);
    b = t / Hp;
    const int p = r + 1, full = nbig * ppb;   // is pair p the first of a band?
    const int i = p < full ? p / ppb : nbig + (p - full) / (ppb > 1 ? ppb - 1 : 1);
    col_seam = true;
    row_seam = p < Hp && i < bands && band_start(i) == p;
  } else {
    size_t t = (e - n_col) >> 4;
    c = (int)(t % Wp);
    t /= Wp;
    r = band_start((int)(t % (bands - 1)) + 1) - 1;
    b = t / (bands - 1);
    if (r < 0 || r + 1 >= Hp) return;              // (no band starts there: launch_conv1's bands never do)
    if ((c & 63) == 63 && 2 * c + 2 < Wo) return;  // the first range's
    col_seam = false;
    row_seam = true;
  }
  float *const out = y + ((b * Hp + r) * Wp + c) * 64 + 4 * c4;
  float4 m = load4(out);
  auto take = [&](int hi, int wi) {
    const float4 v = load4(a + ((b * Ho + hi) * Wo + wi) * 64 + 4 * c4);
    m.x = fmaxf(m.x, v.x);
    m.y = fmaxf(m.y, v.y);
    m.z = fmaxf(m.z, v.z);
    m.w = fmaxf(m.w, v.w);
  };
  if (col_seam) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (2 * r + i < Ho) take(2 * r + i, 2 * c + 2);
  }
  if (row_seam) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (2 * c + j < Wo && !(col_seam && j == 2)) take(2 * r + 2, 2 * c + j);
  }
  store4(out, m);
}

// ----------------------------------------------------------------------------------------
// The root conv for any other window length: 7x7 / stride 2 / pad 3, cin = 3 S -> 64, 1 <= S <= kRootMaxFrames, cin a
// kernel ARGUMENT.  It is conv1_kernel<4, float, SRC> generalised: the same tile (128 output pixels of one output row x 64
// channels, 4 waves as 2 x 2, two 32-pixel MFMA blocks per wave), the same exact float32 products on
// v_mfma_f32_32x32x2_f32 in two chains per block (even / odd taps, joined once in the epilogue), the same scale_RGB in the
// load stage (x * 255 - mean_g, two roundings; with a mask (x * m) * 255 - mean_g on the first 3 (S - 1) channels; the pad
// ring 0 in the SCALED domain; a table index outside [0, n_pool) a frame of raw zeros), the tile decode and the epilogue
// are the shared ones (conv1_tile, C1_TILE_PUT, conv1_tile_out).
//
// LDS, sized per launch from cin (rootconv_lds_bytes): the raw row segment of 261 pixels at a pitch of
// rootconv_pitch(cin) floats, and the kernel row's weights [64][rootconv_ld(cin)].
// Pitch rule: lane r of an A fragment reads 8 bytes at float offset 2 pitch r + const, which visits every even bank once
// over r = 0..31 exactly when pitch is odd.  cin odd (S odd): pitch = cin, the 7 cin taps of a pixel are one contiguous run,
// as in conv1_kernel.  cin even (S even): pitch = cin + 1, one pad float behind each pixel's channels; the run of a pixel
// then is 7 pitch long with a zero WEIGHT at every pad position (make_conv1 lays the weight rows out at the same pitch) and
// the pad floats are zeroed once, so the layout costs 1 / (cin + 1) more MFMA steps (2 % at S = 16, 14 % at S = 2) and no
// conflict.  The weight rows' stride is 2 x odd like kConv1Ld.
//
// Staging is by (pixel, frame) items of three floats, frame-major: consecutive lanes take consecutive pixels of one frame
// (12-byte neighbours in a frame ring, LDS stores `pitch` floats apart: conflict-free).  It runs between the two barriers
// of a kernel row, not prefetched into registers as conv1_kernel does (the item count depends on S); for small S several
// workgroups share a CU and overlap it, at S = 16 it is ~1/8 of a row's MFMA time.  The aligned bit of SRC changes nothing
// here (every load is a dword or a byte); it is kept because SRC is the launch record's vocabulary.
// ----------------------------------------------------------------------------------------
struct PPieces {};   // TO of the f32s precision: the output stored as float16 pieces (P format, store4_p)

constexpr int rootconv_seg(int cin) { return C1_RING_PX * rootconv_pitch(cin) + 4; }   // floats; the last A read ends at 254 pitch + kpad
constexpr int rootconv_wstage(int cin) { return 64 * rootconv_ld(cin) > C1_TILE * C1_LDC ? 64 * rootconv_ld(cin) : C1_TILE * C1_LDC; }
constexpr size_t rootconv_lds_bytes(int cin) { return sizeof(float) * (size_t)(rootconv_wstage(cin) + rootconv_seg(cin)); }
static_assert(rootconv_lds_bytes(3 * kRootMaxFrames) <= 160 * 1024, "the largest window must fit one workgroup's LDS");

template <typename TO, int SRC>
__global__ __launch_bounds__(256)
void rootconv_kernel(const Conv1Src src, const float *__restrict__ wt1, const float *__restrict__ bias, void *__restrict__ y,
                     int H, int W, int Ho, int Wo, int wtiles, int cin) {
  constexpr int NT = 256, MI = 2;
  constexpr int kKind = SRC >> kSrcKindShift & 3;
  constexpr bool kMasked = (SRC & kSrcMasked) != 0;
  static_assert(SRC >= 0 && SRC < 16 && kKind <= kSrcRingU8, "no such conv1 source");
  extern __shared__ __attribute__((aligned(16))) float rc_lds[];
  const int S = cin / 3, pitch = rootconv_pitch(cin), ldw = rootconv_ld(cin), steps = rootconv_kpad(cin) / 4;
  const int welems = 64 * ldw, seg = rootconv_seg(cin);
  float *w_s = rc_lds;
  float *in_s = rc_lds + rootconv_wstage(cin);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  const Conv1Tile tile = conv1_tile(wtiles, Ho);
  const int b = tile.b, ho = tile.ho, wo0 = tile.wo0;

  for (int e = tid; e < seg; e += NT) in_s[e] = 0.f;   // the pad floats and the tail stay zero: they meet zero weights

  const float *mplane = nullptr;
  if constexpr (kMasked) mplane = src.mask + (size_t)b * H * W;
  const int items = C1_RING_PX * S;
  // kernel row kh: input row 2 ho + kh - 3, scaled, into in_s; the row's weights into w_s
  auto stage = [&](int kh) __attribute__((always_inline)) {
    const int hi = 2 * ho + kh - 3;
    const bool row_ok = hi >= 0 && hi < H;   // uniform
    for (int q = tid; q < items; q += NT) {
      const int f = q / C1_RING_PX, p = q - f * C1_RING_PX;
      const int col = 2 * wo0 - 3 + p;
      float a[3] = {0.f, 0.f, 0.f};
      if (row_ok && col >= 0 && col < W) {
        const size_t px = (size_t)hi * W + col;
        float m = 1.0f;
        bool masked = false;
        if constexpr (kMasked) {
          masked = f < S - 1;   // the newest frame is never masked (eval_train.py:62)
          if (masked) m = mplane[px];
        }
        float s3[3];   // the raw value times 255
        if constexpr (kKind == kSrcWindow) {
          const float *x = static_cast<const float *>(src.base) + ((size_t)b * H * W + px) * cin + 3 * f;
#pragma unroll
          for (int j = 0; j < 3; ++j) s3[j] = masked ? (x[j] * m) * 255.0f : x[j] * 255.0f;
        } else {
          const int fi = src.table[b * S + f];
          const bool frame_ok = fi >= 0 && fi < src.n_pool;   // a missing frame is a frame of raw zeros
          const size_t e0 = ((size_t)(frame_ok ? fi : 0) * H * W + px) * 3;
          if constexpr (kKind == kSrcRingU8) {
            const uint8_t *x = static_cast<const uint8_t *>(src.base) + e0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const float v = (float)x[j];   // == f32(v / 255.) * 255.f exactly (Conv1RingRow)
              if (masked) {
                const float q0 = v * (1.0f / 255.0f);
                const float xf = __builtin_fmaf(__builtin_fmaf(-q0, 255.0f, v), 1.0f / 255.0f, q0);   // f32(v / 255.), correctly rounded
                s3[j] = (xf * m) * 255.0f;
              } else {
                s3[j] = v;
              }
            }
          } else {
            const float *x = static_cast<const float *>(src.base) + e0;
#pragma unroll
            for (int j = 0; j < 3; ++j) s3[j] = masked ? (x[j] * m) * 255.0f : x[j] * 255.0f;
          }
          if (!frame_ok) s3[0] = s3[1] = s3[2] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int c = 3 * f + j, g = (c >= S) + (c >= 2 * S);   // raw group c / S gets the mean of scaled group 2 - g
          a[j] = s3[j] - (g == 0 ? 123.68f : (g == 1 ? 116.779f : 103.939f));
        }
      }
      float *dst = in_s + p * pitch + 3 * f;
      dst[0] = a[0];
      dst[1] = a[1];
      dst[2] = a[2];
    }
    const floatx4 *wsrc = reinterpret_cast<const floatx4 *>(wt1 + (size_t)kh * welems);
    for (int q = tid; q < welems / 4; q += NT) reinterpret_cast<floatx4 *>(w_s)[q] = wsrc[q];
  };

  floatx16 acc[MI], acc2[MI];   // even and odd taps (conv1_kernel)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[mi][q] = acc2[mi][q] = 0.f;

  const float *a0 = in_s + 2 * pitch * (wm * 32 * MI + r) + 2 * h;
  const float *a1 = a0 + 2 * pitch * 32;
  const float *bp = w_s + (wn * 32 + r) * ldw + 2 * h;
  for (int kh = 0; kh < 7; ++kh) {
    __syncthreads();   // everyone is done reading the previous kernel row (the first time: the zeros have landed)
    stage(kh);
    __syncthreads();
    auto step = [&](int u) __attribute__((always_inline)) {
      const float2 x0 = *reinterpret_cast<const float2 *>(a0 + 4 * u);
      const float2 x1 = *reinterpret_cast<const float2 *>(a1 + 4 * u);
      const float2 wv = *reinterpret_cast<const float2 *>(bp + 4 * u);
      acc[0] = mfma32(x0.x, wv.x, acc[0]);
      acc[1] = mfma32(x1.x, wv.x, acc[1]);
      acc2[0] = mfma32(x0.y, wv.y, acc2[0]);
      acc2[1] = mfma32(x1.y, wv.y, acc2[1]);
    };
    int u = 0;
    for (; u + 1 < steps; u += 2) {   // two steps per trip: the reads of the second are issued under the MFMAs of the first
      step(u);
      step(u + 1);
    }
    if (u < steps) step(u);
  }

  // ---- epilogue: conv1_kernel's, through the weight stage (at least C1_TILE * C1_LDC floats: rootconv_wstage)
  float *Cs = w_s;
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
    C1_TILE_PUT(Cs, wm * 32 * MI + mi * 32, wn * 32, acc[mi][q] + acc2[mi][q]);
  __syncthreads();
  const size_t e0 = (((size_t)b * Ho + ho) * Wo + wo0) * 64 + 4 * (tid & 15);
  conv1_tile_out<NT / 16>(Cs, conv1_tile_bias(bias, tid), tid, wo0, Wo, [&](int row, float4 v) __attribute__((always_inline)) {
    if constexpr (std::is_same<TO, PPieces>::value)
      store4_p(y, e0 + (size_t)row * 64, v);
    else
      store4(static_cast<TO *>(y) + e0 + (size_t)row * 64, v);
  });
}

}  // namespace

// Bands of root_band_kernel, one workgroup per CU: among 3 .. 6 rounds of the 256 CUs the number of bands per column tile
// and image whose workgroups fill their last round best (the fewest rounds on a tie), with at least 3 x 256 workgroups and
// at least 4 row pairs per band -- B = 16 at 1280 x 720: 80 column tiles x 16 bands = 1280 workgroups, five rounds exactly.
// 0 = do not use the kernel.  A function of (B, Ho, wtiles) alone: every source of one shape takes the same kernel.
// *pairs_per_band is the longest band, *nbig the number of bands of that length (the others hold one pair less).
int root_bands(int B, int Ho, int wtiles, int *pairs_per_band, int *nbig) {
  const int pairs = (Ho + 1) / 2;
  const long cols = (long)B * wtiles;
  int best = 0;
  double best_fill = 0.0;
  for (int rounds = 3; rounds <= 6; ++rounds) {
    const long fit = 256L * rounds / cols, bands = fit < pairs / 4 ? fit : pairs / 4;
    if (bands < 1 || cols * bands < 3 * 256) continue;
    const double fill = (double)(cols * bands) / (256.0 * rounds);
    if (fill > best_fill) {
      best_fill = fill;
      best = (int)bands;
    }
  }
  if (best > 0) {
    const int ppb = (pairs + best - 1) / best;
    if (pairs_per_band) *pairs_per_band = ppb;
    if (nbig) *nbig = pairs - best * (ppb - 1);
  }
  return best;
}

bool launch_conv1_f32(const Conv1Choice &c, const Conv1Args &a, int cin, void *pooled) {
  const Conv1Src &src = a.src;
  const float *const wt1 = a.wt.f32, *const bias = a.wt.bias;
  void *const y = a.y;
  const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, wtiles = a.wtiles;
  hipStream_t s = a.s;
  const dim3 grid((unsigned)((long)wtiles * Ho * a.B));
  switch (c.family) {
    case kConv1Rootconv: {
      const size_t lds = rootconv_lds_bytes(cin);
      return with_conv1_src<true>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        if (c.to == 1)
          hipLaunchKernelGGL((rootconv_kernel<_Float16, S>), grid, dim3(256), lds, s, src, wt1, bias, y, H, W, Ho, Wo, wtiles, cin);
        else if (c.to == 2)
          hipLaunchKernelGGL((rootconv_kernel<PPieces, S>), grid, dim3(256), lds, s, src, wt1, bias, y, H, W, Ho, Wo, wtiles, cin);
        else
          hipLaunchKernelGGL((rootconv_kernel<float, S>), grid, dim3(256), lds, s, src, wt1, bias, y, H, W, Ho, Wo, wtiles, cin);
      });
    }
    case kConv1Band: {
      const int bands = c.bands, ppb = c.per_band, nbig = c.nbig;
      const dim3 bgrid((unsigned)((long)wtiles * bands * a.B));
      return with_conv1_src<false>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        if (c.fuse_pool)
          hipLaunchKernelGGL((root_band_pool_kernel<S>), bgrid, dim3(RB_NT), RB_POOL_LDS, s, src, wt1, bias, static_cast<float *>(y),
                             static_cast<float *>(pooled), H, W, Ho, Wo, wtiles, bands, ppb, nbig);
        else
          hipLaunchKernelGGL((root_band_kernel<S>), bgrid, dim3(RB_NT), RB_LDS, s, src, wt1, bias, static_cast<float *>(y), H, W, Ho,
                             Wo, wtiles, bands, ppb, nbig);
      });
    }
    case kConv1OneRow:
      if (c.nw == 8 || c.to == 1) {   // the 8-wave and the float16-output forms: window tensors, staged element-wise
        if (c.src != 0) return false;
        if (c.nw == 8)
          hipLaunchKernelGGL((conv1_kernel<8, float, 0>), grid, dim3(512), 0, s, src, wt1, bias, static_cast<float *>(y), H, W, Ho,
                             Wo, wtiles);
        else
          hipLaunchKernelGGL((conv1_kernel<4, _Float16, 0>), grid, dim3(256), 0, s, src, wt1, bias, static_cast<_Float16 *>(y), H, W,
                             Ho, Wo, wtiles);
        return true;
      }
      return with_conv1_src<true>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        hipLaunchKernelGGL((conv1_kernel<4, float, S>), grid, dim3(256), 0, s, src, wt1, bias, static_cast<float *>(y), H, W, Ho, Wo,
                           wtiles);
      });
    default:
      return false;
  }
}

int prepare_rootconv() {
  const int bytes = (int)rootconv_lds_bytes(3 * kRootMaxFrames);
  hipError_t err = hipSuccess;
  auto raise = [&](const void *fn) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (err == hipSuccess) err = e;
  };
  for (int src = 0; src < 16; ++src)
    with_conv1_src<true>(src, [&](auto src_c) {
      constexpr int S = decltype(src_c)::value;
      raise(reinterpret_cast<const void *>(&rootconv_kernel<float, S>));
      raise(reinterpret_cast<const void *>(&rootconv_kernel<_Float16, S>));
      raise(reinterpret_cast<const void *>(&rootconv_kernel<PPieces, S>));
    });
  DVSG_HIP(err);
  return DVSG_OK;
}

int prepare_root_band() {
  hipError_t err = hipSuccess;
  for (int src = 0; src < 16; ++src)
    with_conv1_src<false>(src, [&](auto src_c) {
      constexpr int S = decltype(src_c)::value;
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&root_band_kernel<S>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)RB_LDS);
      if (err == hipSuccess) err = e;
      const hipError_t ep = hipFuncSetAttribute(reinterpret_cast<const void *>(&root_band_pool_kernel<S>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)RB_POOL_LDS);
      if (err == hipSuccess) err = ep;
    });
  DVSG_HIP(err);
  return DVSG_OK;
}

#ifdef DVSG_STAMPS
extern "C" int dvsg_debug_read_conv1_stamps(void *host, size_t bytes) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_c1_stamps), bytes) == hipSuccess ? 0 : -3;
}
#endif

int launch_root_pool_seams(const RootPool &pool, const void *conv_taps, int B, int Ho, int Wo, hipStream_t s) {
  DVSG_REQUIRE(pool.fused && Ho % 2 == 0 && Wo % 2 == 0 && pool.bands >= 1, "root pool seams: no fused root launch to finish");
  const int Hp = Ho / 2, Wp = Wo / 2, ncs = ceil_div(Wo, C1_TILE) - 1;
  const size_t n_col = (size_t)B * Hp * ncs * 16, total = n_col + (size_t)B * (pool.bands - 1) * Wp * 16;
  g_last_root_kernel[kRootMaxpool] = 4;
  if (total == 0) return DVSG_OK;   // one column tile, one band: the band kernel's pooled rows are whole
  const size_t want = (total + 255) / 256;
  DVSG_REQUIRE(want < (1u << 31), "root pool seams: %zu blocks do not fit a grid", want);
  ProfScope prof(kClsMaxpool, s, 0.0, 4.0 * 4.0 * (double)total * 5.0);   // (about: a partial and ~3 taps in, one element out)
  hipLaunchKernelGGL(root_pool_seams_kernel, dim3((unsigned)want), dim3(256), 0, s, static_cast<const float *>(conv_taps),
                     static_cast<float *>(pool.pooled), Ho, Wo, ncs, pool.bands, pool.ppb, pool.nbig, n_col, total);
  return check_launch("root_pool_seams_kernel");
}

}  // namespace dvsg
