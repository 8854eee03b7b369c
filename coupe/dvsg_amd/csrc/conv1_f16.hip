// The root conv on the float16 matrix cores (conv1.hip describes the root).  The float16 precision's kernels: one output
// row per workgroup, two, and the marching kernel of the big launches; and the f32s precision's conv1_split_kernel, whose
// products are formed from two float16 pieces per operand.  (The split kernel shares this file because the masked frame-ring
// forms of conv1_f16_pair_kernel compile to other register allocations when no second kernel here stages the same rows:
// DESIGN.md section 5.0c-V.)
#include "conv1_device.h"
#include "conv1_internal.h"

namespace dvsg {
namespace {

#ifdef DVSG_STAMPS  // diagnostic build (tools/stamp_probe_march.py): this file's stamp buffer, read by dvsg_debug_read_march_stamps
__device__ unsigned long long g_c1_stamps[8 * 65536];
#endif

// ----------------------------------------------------------------------------------------
// conv1 for the float16 precision: same decomposition (one output row x 128 pixels x 64 channels
// per workgroup, the input row segment staged once per kernel row and read in place as
// overlapping windows), but the scaled input is stored in LDS as float16 and multiplied on
// v_mfma_f32_32x32x16_f16.  A lane's operand is 8 consecutive taps = 16 bytes at byte offset
// 84 pixel + 32 step + 16 h: only 4-byte aligned, so it is fetched as four ds_read_b32
// (21 r mod 32 is a bijection: conflict-free); the weight rows are laid out with a 336-byte
// stride (21 x 16 B) for conflict-free ds_read_b128 and arrive by LDS-DMA.  Both LDS images are
// double-buffered: kernel row kh+1 is fetched while kh is multiplied, one barrier per row.
// The 147 taps of a row are padded to 160 (ten 16-tap MFMA steps) with zero weights.
// ----------------------------------------------------------------------------------------
constexpr int C1H_STEPS = 10;
constexpr int C1H_LD = 168;                        // halfs per weight row in LDS / global
constexpr int C1H_WBYTES = 64 * C1H_LD * 2;        // 21504 bytes per kernel row = 21 LDS-DMA pieces
constexpr int C1H_SEG = 5504;                      // halfs per staged input row (5481 + zero tail)
constexpr int C1H_IN4 = (C1H_SEG / 4 + 255) / 256;     // 6 groups of four elements per thread
typedef const __attribute__((address_space(1))) void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

// Weights of kernel row kh for the one- and two-row kernels (four waves): 21 pieces of 1 KiB, piece j by wave j % 4, straight
// into the LDS image `w_dst`.  (conv1_f16_march_kernel, whose staging waves are waves 4-7, keeps its own unrolled form: its
// vmcnt arithmetic counts on the exact order of its loads.)
__device__ __forceinline__ void weights_dma(const _Float16 *wt1h, int kh, char *w_dst, int wave, int lane) {
  const char *wsrc = reinterpret_cast<const char *>(wt1h) + (size_t)kh * C1H_WBYTES;
  for (int j = wave; j < C1H_WBYTES / 1024; j += 4)
    __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + j * 1024 + lane * 16), (lptr_t)(w_dst + j * 1024), 16, 0, 0);
}
// The row store that follows it -- scatter for rings, else scaled groups rounded once to float16 -- is written out in both
// kernels (and, with its two differences, in the marching kernel): as one function it changed the register counts or more
// than 1 % of the instructions of conv1_f16_kernel<_Float16, 0 / 1> and conv1_f16_pair_kernel<_Float16, 0 / 1 / 8 / 9>
// (profiles/README.md, r18).

template <typename TO, int SRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv1_f16_kernel(const Conv1Src src, const _Float16 *__restrict__ wt1h, const float *__restrict__ bias,
                      TO *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles) {
  static_assert(C1_TILE * C1_LDC * 4 <= 2 * C1H_WBYTES, "epilogue tile must fit in the weight stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * C1H_WBYTES + 2 * C1H_SEG * 2];
  char *w_s = lds;
  char *in_s = lds + 2 * C1H_WBYTES;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;   // wave w: pixels [32 w, 32 w + 32) x all 64 channels (see conv1_split_kernel)

  const Conv1Tile tile = conv1_tile(wtiles, Ho);
  const int b = tile.b, ho = tile.ho, wo0 = tile.wo0;

  typedef typename Conv1RowSel<256, C1H_IN4, SRC>::type Row;
  Row row;
  row.init(src, tid, b, wo0, H, W, C1H_SEG);
  if constexpr (Row::kRing) {   // both images: the zero tap's slot and the tail are read against zero weights
    for (int e = tid; e < C1H_SEG; e += 256) reinterpret_cast<unsigned *>(in_s)[e] = 0u;
    __syncthreads();   // the first scatter writes halves of words other threads zero: the zeros must land first
  }

  typename Row::Data rd;
  auto load_stage = [&](int kh, int buf) __attribute__((always_inline)) {
    weights_dma(wt1h, kh, w_s + buf * C1H_WBYTES, wave, lane);
    row.load(rd, 2 * ho + kh - 3);
  };
  auto store_stage = [&](int buf) __attribute__((always_inline)) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    if constexpr (Row::kRing) {
      _Float16 *dsth = reinterpret_cast<_Float16 *>(in_s + buf * C1H_SEG * 2);
      row.scatter(rd, [&](int e, float v) __attribute__((always_inline)) { dsth[e] = (_Float16)v; });
    } else {
      half4_t *dst = reinterpret_cast<half4_t *>(in_s + buf * C1H_SEG * 2);
#pragma unroll
      for (int i = 0; i < C1H_IN4; ++i) {
        const int q = tid + 256 * i;
        const floatx4 v = row.scaled(rd, i);   // then one rounding to f16
        half4_t hv;
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = (_Float16)v[j];
        if (q < C1H_SEG / 4) dst[q] = hv;
      }
    }
  };

  floatx16 acc[2];   // [channel block]
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[ni][q] = 0.f;

  load_stage(0, 0);
  store_stage(0);
  __syncthreads();
  for (int kh = 0; kh < 7; ++kh) {
    const int buf = kh & 1;
    if (kh + 1 < 7) load_stage(kh + 1, buf ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned *a0 = reinterpret_cast<const unsigned *>(in_s + buf * C1H_SEG * 2) + kConv1Cin * (wave * 32 + r) + 4 * h;
    const char *bp = w_s + buf * C1H_WBYTES + 2 * (r * C1H_LD + 8 * h);
    // software-pipelined one step ahead, like conv1_split_kernel
    struct Frag {
      union {
        unsigned u[4];
        halfx8 v;
      } a;
      halfx8 b[2];
    };
    auto read_frag = [&](Frag &f, int t) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f.a.u[j] = a0[8 * t + j];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) f.b[ni] = *reinterpret_cast<const halfx8 *>(bp + 2 * ni * 32 * C1H_LD + 32 * t);
    };
    Frag fr[2];
    read_frag(fr[0], 0);
#pragma unroll
    for (int t = 0; t < C1H_STEPS; ++t) {
      if (t + 1 < C1H_STEPS) read_frag(fr[(t + 1) & 1], t + 1);
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[t & 1].a.v, fr[t & 1].b[0], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[t & 1].a.v, fr[t & 1].b[1], acc[1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (kh + 1 < 7) store_stage(buf ^ 1);
    __syncthreads();
  }

  float *Cs = reinterpret_cast<float *>(lds);
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
    C1_TILE_PUT(Cs, wave * 32, ni * 32, acc[ni][q]);
  __syncthreads();
  TO *yrow = y + (((size_t)b * Ho + ho) * Wo + wo0) * 64 + 4 * (tid & 15);
  conv1_tile_out<16>(Cs, conv1_tile_bias(bias, tid), tid, wo0, Wo,
                     [&](int row, float4 v) __attribute__((always_inline)) { store4(yrow + (size_t)row * 64, v); });
}

// ----------------------------------------------------------------------------------------
// conv1, float16 precision, TWO output rows per workgroup (rows 2 p and 2 p + 1 of one 128-pixel tile).
//
// Why.  rocprofv3 counters of conv1_f16_kernel at 3840x2160, batch 32 (profiles/r02_f16_pmc_sq.csv): matrix pipe busy
// 27 %, SQ_ACTIVE_INST_ANY / SQ_WAVE_CYCLES = 0.44 with two waves per SIMD -- the SIMDs issue instructions 88 % of the time:
// the kernel is bound by INSTRUCTION ISSUE (and, at 304 KB of L2 -> CU traffic per tile, close to the L2's rate), not by
// the matrix cores or HBM (FETCH_SIZE = the input once).  Per kernel row and wave it issues ~110 VALU (scale_RGB, the
// float16 rounding), 60 LDS fragment reads, 11 memory instructions and 20 MFMAs: 11 other instructions per MFMA.
// Two rows per workgroup attack every term:
//   * the weights of a kernel row (21.5 KB by LDS-DMA) and their fragment reads serve both rows: per MFMA half the weight
//     traffic and half the B reads;
//   * the kernel rows are visited as two chains, kh = 0, 2, 4, 6 and kh = 1, 3, 5.  Within a chain the input row that
//     output row 2 p + 1 needs at step kh (row a + kh + 2) is the one output row 2 p needs at step kh + 2: it stays where
//     it is, and only ONE new input row is staged per step -- 9 stagings per pair of output rows instead of 14;
//   * a step is 40 MFMAs, so the two barriers and the address arithmetic of a step cost half as much per MFMA.
// Staging as in conv1_kernel: the next step's new row(s) are fetched into registers under this step's MFMAs and, after
// the barrier that ends the step, scaled, rounded and stored over the row nobody needs any more; the weights of the next
// step arrive by LDS-DMA in the other weight buffer meanwhile.  LDS: 2 x 21.5 KB of weights + 2 x 11 KB of rows, two
// workgroups per CU, as before.
// ----------------------------------------------------------------------------------------
template <typename TO, int SRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv1_f16_pair_kernel(const Conv1Src src, const _Float16 *__restrict__ wt1h, const float *__restrict__ bias,
                           TO *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles, int hpairs) {
  static_assert(C1_TILE * C1_LDC * 4 <= 2 * C1H_WBYTES, "epilogue tile must fit in the weight stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * C1H_WBYTES + 2 * C1H_SEG * 2];
  char *w_s = lds;
  char *in_s = lds + 2 * C1H_WBYTES;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;   // wave w: pixels [32 w, 32 w + 32) x all 64 channels x both rows

  const Conv1Tile tile = conv1_tile(wtiles, hpairs);
  const int b = tile.b, ho0 = 2 * tile.ho, wo0 = tile.wo0;

  typedef typename Conv1RowSel<256, C1H_IN4, SRC>::type Row;
  Row row;
  row.init(src, tid, b, wo0, H, W, C1H_SEG);
  if constexpr (Row::kRing) {   // both images: the zero tap's slot and the tail are read against zero weights
    for (int e = tid; e < C1H_SEG; e += 256) reinterpret_cast<unsigned *>(in_s)[e] = 0u;
    __syncthreads();   // the first scatter writes halves of words other threads zero: the zeros must land first
  }
  typename Row::Data d0, d1;
  auto store_row = [&](const typename Row::Data &d, int buf) __attribute__((always_inline)) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    if constexpr (Row::kRing) {
      _Float16 *dsth = reinterpret_cast<_Float16 *>(in_s + buf * C1H_SEG * 2);
      row.scatter(d, [&](int e, float v) __attribute__((always_inline)) { dsth[e] = (_Float16)v; });
    } else {
      half4_t *dst = reinterpret_cast<half4_t *>(in_s + buf * C1H_SEG * 2);
#pragma unroll
      for (int i = 0; i < C1H_IN4; ++i) {
        const int q = tid + 256 * i;
        const floatx4 v = row.scaled(d, i);   // then one rounding to f16
        half4_t hv;
#pragma unroll
        for (int j = 0; j < 4; ++j) hv[j] = (_Float16)v[j];
        if (q < C1H_SEG / 4) dst[q] = hv;
      }
    }
  };

  floatx16 acc[2][2];   // [output row][channel block]
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[j][ni][q] = 0.f;

  // input row of (output row ho0 + j, kernel row kh)
  const int a = 2 * ho0 - 3;
  // prologue: rows a, a + 2 and the weights of kernel row 0
  row.load(d0, a);
  row.load(d1, a + 2);
  weights_dma(wt1h, 0, w_s, wave, lane);
  store_row(d0, 0);
  store_row(d1, 1);
  __syncthreads();
  int lo = 0;   // buffer of output row ho0's input row; the other one holds output row ho0 + 1's
  // (seven explicit instances: left to `#pragma unroll` the optimizer gives up on this body and the kernel-row order
  // becomes a table lookup)
  auto step = [&](auto S) __attribute__((always_inline)) {
    constexpr int s = decltype(S)::value;
    constexpr int kOrder[8] = {0, 2, 4, 6, 1, 3, 5, -1};
    constexpr int kh = kOrder[s], khn = kOrder[s + 1];
    constexpr bool chain = khn == kh + 2;        // the next step continues this chain: one new row
    if (khn >= 0) {
      row.load(d0, chain ? a + khn + 2 : a + khn);
      if (!chain) row.load(d1, a + khn + 2);
      weights_dma(wt1h, khn, w_s + ((s + 1) & 1) * C1H_WBYTES, wave, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned *a0 = reinterpret_cast<const unsigned *>(in_s + lo * C1H_SEG * 2) + kConv1Cin * (wave * 32 + r) + 4 * h;
    const unsigned *a1 = reinterpret_cast<const unsigned *>(in_s + (lo ^ 1) * C1H_SEG * 2) + kConv1Cin * (wave * 32 + r) + 4 * h;
    const char *bp = w_s + (s & 1) * C1H_WBYTES + 2 * (r * C1H_LD + 8 * h);
    struct Frag {
      union {
        unsigned u[4];
        halfx8 v;
      } a[2];
      halfx8 b[2];
    };
    auto read_frag = [&](Frag &f, int t) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f.a[0].u[j] = a0[8 * t + j];
        f.a[1].u[j] = a1[8 * t + j];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) f.b[ni] = *reinterpret_cast<const halfx8 *>(bp + 2 * ni * 32 * C1H_LD + 32 * t);
    };
    Frag fr[2];
    read_frag(fr[0], 0);
#pragma unroll
    for (int t = 0; t < C1H_STEPS; ++t) {
      if (t + 1 < C1H_STEPS) read_frag(fr[(t + 1) & 1], t + 1);
      __builtin_amdgcn_sched_barrier(0);
      const Frag &f = fr[t & 1];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[j][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[j].v, f.b[ni], acc[j][ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();   // everyone has read this step's rows; the prefetched row(s) and the next weights have landed
    if (khn >= 0) {
      if (chain) {
        store_row(d0, lo);   // over the row of output row ho0: the other one becomes its row for the next step
        lo ^= 1;
      } else {
        store_row(d0, lo);
        store_row(d1, lo ^ 1);
      }
      __syncthreads();
    }
  };
  step(std::integral_constant<int, 0>{});
  step(std::integral_constant<int, 1>{});
  step(std::integral_constant<int, 2>{});
  step(std::integral_constant<int, 3>{});
  step(std::integral_constant<int, 4>{});
  step(std::integral_constant<int, 5>{});
  step(std::integral_constant<int, 6>{});

  float *Cs = reinterpret_cast<float *>(lds);
  const float4 b4 = conv1_tile_bias(bias, tid);   // once for both rows
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j) __syncthreads();   // the first row's tile has been read
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
      C1_TILE_PUT(Cs, wave * 32, ni * 32, acc[j][ni][q]);
    __syncthreads();
    if (ho0 + j < Ho) {
      TO *yrow = y + (((size_t)b * Ho + ho0 + j) * Wo + wo0) * 64 + 4 * (tid & 15);
      conv1_tile_out<16>(Cs, b4, tid, wo0, Wo,
                         [&](int row, float4 v) __attribute__((always_inline)) { store4(yrow + (size_t)row * 64, v); });
    }
  }
}

// ----------------------------------------------------------------------------------------
// conv1, float16 precision, for the big launches: a workgroup MARCHES down a band of output rows of one 128-pixel
// column tile, four output rows ("quad") at a time, and its eight waves are SPECIALISED --
//
//   waves 0-3  multiply: pixels [32 w, 32 w + 32) x 64 channels x the quad's 4 rows (128 accumulator registers);
//              their instruction stream is fragment reads + MFMAs only (80 MFMAs per step);
//   waves 4-7  stage: fetch the input rows the NEXT step needs, scale_RGB them, round to float16, store them in LDS,
//              and start the LDS-DMA of the next step's weight row.
//
// A wave of each kind shares a SIMD, so the staging arithmetic issues in the shadow of the matrix pipe instead of
// between its MFMAs: conv1_f16_pair_kernel was bound by instruction ISSUE (SQ_ACTIVE_INST_ANY = 0.34 of the wave cycles
// with two waves per SIMD, 6.8 VALU + 1.9 LDS + 3 scalar instructions per MFMA, matrix pipe busy 35 %).
//
// Marching makes the staged rows a SLIDING WINDOW.  A step is one kernel row kh for the quad's four output rows
// r0 .. r0 + 3, which need the input rows a + kh + {0, 2, 4, 6} (a = 2 r0 - 3).  The steps of a quad run as two chains,
// kh = 0, 2, 4, 6 and kh = 1, 3, 5; a chain's window moves up by one input row of its parity per step and -- because the
// next quad starts 8 input rows further down -- continues seamlessly from quad to quad.  So every input row is staged
// ONCE per column tile (8 stagings per quad = 2 per output row; the one-row kernel staged 7, the pair kernel 4.5), into
// one of two rings of five row buffers (odd and even input rows): four rows of the current window + the one being
// filled.  The weights of a kernel row serve four output rows (a quarter of the weight traffic and B-fragment reads per
// MFMA of the one-row kernel).  One barrier per step is the only synchronisation: what step s + 1 needs is staged during
// step s.
//
// The MFMA operands are swapped against the other conv1 kernels (A = weights, B = pixels), so a lane ends up with 16
// CHANNELS of one pixel: bias, ReLU, the float16 rounding and 8-byte stores happen from the accumulators, with no LDS
// transpose (there is no LDS left for one: 10 x 11 KB of rows + 2 x 21.5 KB of weights = 153 KB, one workgroup per CU).
// Used when the launch gives every CU several bands (launch_conv1); small launches keep conv1_f16_pair_kernel.
// ----------------------------------------------------------------------------------------
constexpr int C1M_QUAD = 4;                         // output rows per quad
constexpr int C1M_RING = 5;                         // row buffers per parity
constexpr int C1M_LDS = 2 * C1M_RING * C1H_SEG * 2 + 2 * C1H_WBYTES;   // 153 088 bytes

template <int SRC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv1_f16_march_kernel(const Conv1Src src, const _Float16 *__restrict__ wt1h, const float *__restrict__ bias,
                            _Float16 *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles, int bands, int quads_per_band) {
  __shared__ __attribute__((aligned(16))) char lds[C1M_LDS];
  char *w_s = lds;                                   // [2][C1H_WBYTES]
  char *in_s = lds + 2 * C1H_WBYTES;                 // [2 parities][C1M_RING][C1H_SEG halves]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const bool stager = wave >= 4;
  const int r = lane & 31, h = lane >> 5;

  const Conv1Tile tile = conv1_tile(wtiles, bands);  // an XCD takes neighbouring column tiles / bands of one image
  const int b = tile.b, band = tile.ho, wo0 = tile.wo0;
  const int rb0 = band * quads_per_band * C1M_QUAD;                       // first output row of the band
  const int nq = min(quads_per_band, (Ho - rb0 + C1M_QUAD - 1) / C1M_QUAD);
  const int nsteps = 7 * nq;
  // step s: quad s / 7, kernel row kOrder[s % 7]; its window of input rows starts at 2 (rb0 + 4 quad) - 3 + kh
  auto window_of = [&](int s) __attribute__((always_inline)) -> int {
    const int quad = s / 7, ks = s - 7 * quad;
    const int kh = ks < 4 ? 2 * ks : 2 * ks - 7;
    return 2 * (rb0 + C1M_QUAD * quad) - 3 + kh;
  };
  // ring slot (in halves from in_s) of input row `row`: odd rows (the even-kh chain) in the first ring
  auto slot_of = [&](int row) __attribute__((always_inline)) -> int {
    const int u = (row + 64) >> 1;                   // rows >= -3: non-negative
    return (((row & 1) ? 0 : C1M_RING) + u % C1M_RING) * C1H_SEG;
  };

  if (stager) {
    // ------------------------------------------------------------------------------ staging waves
    // Their few instructions go first when both waves of a SIMD are ready (s_setprio): with the default oldest-first
    // arbitration the staging wave -- the younger one -- only issues while the multiplying wave is stalled, and a step takes
    // 5550 cycles instead of 4950 (stamps, tools/stamp_probe_march.py).  The multiplying waves raise their own priority for
    // the flush, where they have no MFMAs to hide behind.
    __builtin_amdgcn_s_setprio(2);
    const int st = tid - 256;
    typedef typename Conv1RowSel<256, C1H_IN4, SRC>::type Row;
    Row row;
    row.init(src, st, b, wo0, H, W, C1H_SEG);
    if constexpr (Row::kRing) {   // the zero tap's slot and the tails of all ten row buffers meet zero weights: finite
      for (int e = st; e < C1M_RING * C1H_SEG; e += 256) reinterpret_cast<unsigned *>(in_s)[e] = 0u;
    }
    __syncthreads();              // (every wave of the workgroup: nobody's first row store may be overtaken by the zeroing)
    // (this kernel's form of weights_dma: unrolled, over waves 4-7, in the load order step_barrier counts on)
    auto march_weights_dma = [&](int kh, int wbuf) __attribute__((always_inline)) {
      const char *wsrc = reinterpret_cast<const char *>(wt1h) + (size_t)kh * C1H_WBYTES;
#pragma unroll
      for (int i = 0; i < (C1H_WBYTES / 1024 + 3) / 4; ++i) {   // 21 pieces of 1 KiB over the 4 staging waves
        const int j = wave - 4 + 4 * i;
        if (j < C1H_WBYTES / 1024)
          __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + j * 1024 + lane * 16), (lptr_t)(w_s + wbuf * C1H_WBYTES + j * 1024),
                                           16, 0, 0);
      }
    };
    auto store_row = [&](const typename Row::Data &dd, int input_row) __attribute__((always_inline)) {
      typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
      _Float16 *base = reinterpret_cast<_Float16 *>(in_s) + slot_of(input_row);
      if constexpr (Row::kRing) {
        // element 0 is the zero tap's slot: the scatter never writes it, but `flush_quad` below transposes conv1 OUTPUTS
        // through halves [0, 5120) of the even ring slots -- a stale output there meets a zero weight and must be finite;
        // a float16 output that overflowed to inf would turn the tile's first pixel of a later quad into NaN.  One lane
        // rewrites it with every staged row (the window path below rewrites the whole segment anyway).
        if (st == 0) base[0] = (_Float16)0.f;
        row.scatter(dd, [&](int e, float v) __attribute__((always_inline)) { base[e] = (_Float16)v; });
      } else {
        half4_t *dst = reinterpret_cast<half4_t *>(base);
#pragma unroll
        for (int i = 0; i < C1H_IN4; ++i) {
          const int q = st + 256 * i;
          const floatx4 v = row.scaled(dd, i);
          if (q < C1H_SEG / 4) dst[q] = __builtin_convertvector(v, half4_t);
        }
      }
    };
    // What a step needs that the steps before it have not staged: the top n rows of its window.  The first step of a chain
    // in the band's FIRST quad: the whole window (4 rows); kh = 1 of a later quad: two rows (its chain has three steps for
    // four output rows); every other step: one row.  ks is a compile-time constant wherever it matters (14 unrolled steps
    // per loop iteration): the per-step code has no data-dependent branches left but "first quad of the band?".
    auto row_base = [&](int quad) __attribute__((always_inline)) -> int { return 2 * (rb0 + C1M_QUAD * quad) - 3; };
    // The staging is pipelined TWO steps deep: during step s the rows of step s + 1 -- fetched during step s - 1 -- are
    // scaled and stored, and the global loads of step s + 2's rows are issued (into the other of two register sets), so a
    // row has a whole step (~1.3 us) to arrive.  One step deep, every step waited for the memory latency of its own rows.
    typename Row::Data setA[2], setB[2];
    // fetch (into a register set) the top rows of the window of step (quad, KS); returns how many (<= 2)
    auto issue = [&](auto KS, int quad, typename Row::Data *set) __attribute__((always_inline)) -> int {
      constexpr int ks = decltype(KS)::value;
      constexpr int kh = ks < 4 ? 2 * ks : 2 * ks - 7;
      const int top = row_base(quad) + kh + 6;
      row.load(set[0], top);
      if (ks == 4 || (ks == 0 && quad == 0)) {
        row.load(set[1], top - 2);
        return 2;
      }
      return 1;
    };
    // scale, round and store the rows of step (quad, KS) out of their register set, then start the LDS-DMA of its weight row
    auto commit = [&](auto KS, int quad, const typename Row::Data *set) __attribute__((always_inline)) {
      constexpr int ks = decltype(KS)::value;
      constexpr int kh = ks < 4 ? 2 * ks : 2 * ks - 7;
      const int top = row_base(quad) + kh + 6;
      store_row(set[0], top);
      if (ks == 4 || (ks == 0 && quad == 0)) store_row(set[1], top - 2);
      if ((ks == 0 || ks == 4) && quad == 0) {   // the band's first window of a chain: its two older rows, on the spot
        typename Row::Data extra[2];
        row.load(extra[0], top - 4);
        row.load(extra[1], top - 6);
        store_row(extra[0], top - 4);
        store_row(extra[1], top - 6);
      }
      march_weights_dma(kh, (7 * quad + ks) & 1);
    };
    // End of a step for a staging wave: its LDS stores and everything OLDER than the `newer` row loads it has just issued
    // (this step's weight DMA in particular) must have landed; the row loads themselves stay in flight across the barrier
    // -- __syncthreads() would wait for them too (vmcnt(0)) and put their latency back into every step.  A row is
    // kLoadsPerRow load instructions when the rows are on the aligned grid; otherwise the count is data dependent and the
    // wave waits for everything.
    constexpr int kLoadsPerRow = (SRC & 1) ? C1H_IN4 : 0;
    auto step_barrier = [&](int newer_rows) __attribute__((always_inline)) {
      if (kLoadsPerRow > 0 && newer_rows == 2) {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * kLoadsPerRow) : "memory");
      } else if (kLoadsPerRow > 0 && newer_rows == 1) {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kLoadsPerRow) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    };
    // (the fences keep the program order the vmcnt arithmetic of step_barrier counts on: weight DMA, THEN the new row loads)
    auto order_fence = [&]() __attribute__((always_inline)) {
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    };
#ifdef DVSG_STAMPS
    unsigned long long st_work = 0, st_wait = 0, st_load = 0, st_t = C1_STAMP();
#endif
    typedef std::integral_constant<int, 0> K0;
    typedef std::integral_constant<int, 1> K1;
    issue(K0{}, 0, setA);
    commit(K0{}, 0, setA);
    order_fence();
    int inflight = nsteps > 1 ? issue(K1{}, 0, setB) : 0;
    order_fence();
    step_barrier(inflight);
#ifdef DVSG_STAMPS
    st_t = C1_STAMP();
#endif
    // One step of the staging waves, K = 0..13 within a pair of quads: during step s = (quad, ks) store step s + 1's rows
    // (in the set of the other parity, fetched a step ago) and fetch step s + 2's into this parity's set.
    auto stager_step = [&](auto KK, int quad_pair) __attribute__((always_inline)) -> bool {
      constexpr int K = decltype(KK)::value;
      constexpr int ks = K % 7, ks1 = (K + 1) % 7, ks2 = (K + 2) % 7;
      const int quad = quad_pair + K / 7, quad1 = quad_pair + (K + 1) / 7, quad2 = quad_pair + (K + 2) / 7;
      const int sidx = 7 * quad + ks;
      if (sidx >= nsteps) return false;
      typename Row::Data *cur = (K & 1) ? setA : setB;    // step s + 1's rows
      typename Row::Data *nxt = (K & 1) ? setB : setA;    // step s + 2's rows go here
#ifdef DVSG_STAMPS
      { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long n_ = C1_STAMP(); st_load += n_ - st_t; st_t = n_; }
#endif
      if (sidx + 1 < nsteps) commit(std::integral_constant<int, ks1>{}, quad1, cur);
      order_fence();
      const int fl = sidx + 2 < nsteps ? issue(std::integral_constant<int, ks2>{}, quad2, nxt) : 0;
      order_fence();
#ifdef DVSG_STAMPS
      { const unsigned long long n_ = C1_STAMP(); st_work += n_ - st_t; st_t = n_; }
#endif
      step_barrier(fl);
#ifdef DVSG_STAMPS
      { const unsigned long long n_ = C1_STAMP(); st_wait += n_ - st_t; st_t = n_; }
#endif
      return true;
    };
    for (int qp = 0; qp < nq; qp += 2) {
#define C1M_STEP(K) if (!stager_step(std::integral_constant<int, K>{}, qp)) break;
      C1M_STEP(0) C1M_STEP(1) C1M_STEP(2) C1M_STEP(3) C1M_STEP(4) C1M_STEP(5) C1M_STEP(6)
      C1M_STEP(7) C1M_STEP(8) C1M_STEP(9) C1M_STEP(10) C1M_STEP(11) C1M_STEP(12) C1M_STEP(13)
#undef C1M_STEP
    }
#ifdef DVSG_STAMPS
    if (tid == 256 && blockIdx.x < 65536) {
      g_c1_stamps[(size_t)blockIdx.x * 8 + 4] = st_work;   // staging wave: loads issued + rows stored + DMA issued, all steps
      g_c1_stamps[(size_t)blockIdx.x * 8 + 5] = st_wait;   // staging wave: waiting at the step barriers
      g_c1_stamps[(size_t)blockIdx.x * 8 + 7] = st_load;   // staging wave: waiting for the rows fetched a step earlier
    }
#endif
    return;
  }

  // -------------------------------------------------------------------------------- multiplying waves
  floatx16 acc[C1M_QUAD][2];   // [output row of the quad][channel block]; rows = channels (A = weights), columns = pixels
#pragma unroll
  for (int j = 0; j < C1M_QUAD; ++j)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[j][ni][q] = 0.f;
  // bias of the 32 channels a lane ends up with: 32 ni + 8 g + 4 h + {0..3}
  float4 bias4[2][4];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int g = 0; g < 4; ++g) bias4[ni][g] = *reinterpret_cast<const float4 *>(bias + 32 * ni + 8 * g + 4 * h);
  __syncthreads();                                   // pairs with the staging waves' barrier after the LDS zeroing
  // A quad's results: bias, ReLU, float16 -- and a TRANSPOSE through LDS, because a lane holds 16 channels of ONE pixel
  // and storing them as they are (8 bytes per lane, 32 different cache lines per instruction) took 13 500 cycles per quad,
  // a quarter of the kernel.  Space: two row buffers of the even-row ring that are dead between the quad's last step
  // (kh = 5: window a + 5 .. a + 11) and the staging for the next quad's kh = 1 (window a + 9 .. a + 15), i.e. the
  // slots of rows a + 5 and a + 7; each wave transposes its own 32 pixels there, half a row's channels at a time, and
  // writes 16 bytes per lane (64 contiguous bytes per pixel).  No barrier: LDS operations of one wave complete in order.
  auto flush_quad = [&](int quad) __attribute__((always_inline)) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    // unit = (output row j, channel block ni): 32 pixels x 32 channels = 2 KB, 80-byte pixel stride (16-byte aligned reads,
    // 20 r mod 64 banks: conflict-free 8-byte writes); two buffers per wave, so that unit u + 1 is written while unit u's
    // reads are in flight -- the LDS round trips of the 8 units of a quad overlap instead of adding up
    constexpr int PXS = 40;                           // halves per pixel
    constexpr int UNIT = 32 * PXS;                    // halves per buffer
    _Float16 *tb = reinterpret_cast<_Float16 *>(in_s) + slot_of(2 * (rb0 + C1M_QUAD * quad) - 3 + (wave < 2 ? 5 : 7)) +
                   (wave & 1) * (2 * UNIT);
    const int cpx = lane >> 2, chunk = lane & 3;      // read side: 16 pixels per pass, 4 chunks of 16 bytes per pixel
    auto write_unit = [&](int u) __attribute__((always_inline)) {
      const int j = u >> 1, ni = u & 1;
      _Float16 *dst = tb + (u & 1) * UNIT + r * PXS + 4 * h;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bb = bias4[ni][g];
        floatx4 v = {acc[j][ni][4 * g], acc[j][ni][4 * g + 1], acc[j][ni][4 * g + 2], acc[j][ni][4 * g + 3]};
        v = v + floatx4{bb.x, bb.y, bb.z, bb.w};
        v = __builtin_elementwise_max(v, floatx4{0.f, 0.f, 0.f, 0.f});
        *reinterpret_cast<half4_t *>(dst + 8 * g) = __builtin_convertvector(v, half4_t);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][ni][4 * g + q] = 0.f;
      }
    };
    halfx8 rd[2][2];
    auto read_unit = [&](int u) __attribute__((always_inline)) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
        rd[u & 1][pass] = *reinterpret_cast<const halfx8 *>(tb + (u & 1) * UNIT + (16 * pass + cpx) * PXS + 8 * chunk);
    };
    auto store_unit = [&](int u) __attribute__((always_inline)) {
      const int j = u >> 1, ni = u & 1;
      const int ho = rb0 + C1M_QUAD * quad + j;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int pxo = wo0 + 32 * wave + 16 * pass + cpx;
#ifdef DVSG_FLUSH_NOSTORE   // (diagnostic: what do the global stores of the flush cost?)
        if (ho < -1 && pxo < Wo)
#else
        if (ho < Ho && pxo < Wo)
#endif
          *reinterpret_cast<halfx8 *>(y + (((size_t)b * Ho + ho) * Wo + pxo) * 64 + 32 * ni + 8 * chunk) = rd[u & 1][pass];
      }
    };
    // software pipeline: a unit's reads are issued a whole unit of arithmetic before the stores that need them (the LDS is
    // ~70 % busy with the other SIMDs' fragment reads: a round trip is several hundred cycles).  LDS operations of one wave
    // complete in order, so read_unit(u) sees write_unit(u) and write_unit(u + 2) cannot overtake read_unit(u).
    __builtin_amdgcn_s_setprio(3);
    write_unit(0);
    write_unit(1);
    read_unit(0);
#pragma unroll
    for (int u = 0; u < 2 * C1M_QUAD; ++u) {
      if (u + 1 < 2 * C1M_QUAD) read_unit(u + 1);
      if (u + 2 < 2 * C1M_QUAD) write_unit(u + 2);
      store_unit(u);
    }
    __builtin_amdgcn_s_setprio(0);
  };
  __syncthreads();                                   // the first window and weight row are in place
#ifdef DVSG_STAMPS
  unsigned long long m_work = 0, m_wait = 0, m_flush = 0, m_t = C1_STAMP();
  const unsigned long long m_begin = m_t;
#endif
  for (int s = 0; s < nsteps; ++s) {
    const int quad = s / 7, ks = s - 7 * quad;
    if (ks == 0 && quad > 0) flush_quad(quad - 1);
#ifdef DVSG_STAMPS
    { const unsigned long long n_ = C1_STAMP(); m_flush += n_ - m_t; m_t = n_; }
#endif
    const int w0 = window_of(s);
    // LDS byte offsets of this lane's fragments, each in ONE register (laundered through an empty asm), so that the ten
    // t-steps differ by the read instruction's own offset field (<= 1020 bytes); left alone the compiler keeps "lane part +
    // (LDS base + t offset)" and spends a v_add_u32 per read -- 80 VALU slots per step on the port the MFMAs issue through
    typedef const __attribute__((address_space(3))) unsigned *lds_u32_t;
    typedef const __attribute__((address_space(3))) halfx8 *lds_h8_t;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)lds;
    unsigned pix_off[C1M_QUAD];
#pragma unroll
    for (int j = 0; j < C1M_QUAD; ++j) {
      pix_off[j] = lds0 + 2 * C1H_WBYTES + 2 * slot_of(w0 + 2 * j) + 4 * (kConv1Cin * (wave * 32 + r) + 4 * h);
      asm volatile("" : "+v"(pix_off[j]));
    }
    unsigned w_off = lds0 + (s & 1) * C1H_WBYTES + 2 * (r * C1H_LD + 8 * h);
    asm volatile("" : "+v"(w_off));
    struct Frag {
      union {
        unsigned u[4];
        halfx8 v;
      } p[C1M_QUAD];
      halfx8 w[2];
    };
    auto read_frag = [&](Frag &f, int t) __attribute__((always_inline)) {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) f.w[ni] = *(lds_h8_t)(size_t)(w_off + 2 * ni * 32 * C1H_LD + 32 * t);
#pragma unroll
      for (int j = 0; j < C1M_QUAD; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) f.p[j].u[q] = *(lds_u32_t)(size_t)(pix_off[j] + 4 * (8 * t + q));
    };
    Frag fr[2];
    read_frag(fr[0], 0);
#pragma unroll
    for (int t = 0; t < C1H_STEPS; ++t) {
      if (t + 1 < C1H_STEPS) read_frag(fr[(t + 1) & 1], t + 1);
      const Frag &f = fr[t & 1];
#pragma unroll
      for (int j = 0; j < C1M_QUAD; ++j)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[j][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.w[ni], f.p[j].v, acc[j][ni], 0, 0, 0);
      // This wave is the only one that multiplies on its SIMD, so the next fragments' 10 LDS reads must issue BETWEEN this
      // step's MFMAs -- each of which keeps the matrix pipe busy for 32 cycles -- not in front of them: grouped
      // [reads][8 MFMAs] a t-step took 350 cycles instead of 256.
#define C1M_GROUP(NREADS)                                                      \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); /* one MFMA */            \
  __builtin_amdgcn_sched_group_barrier(0x100, NREADS, 0); /* LDS reads */
      C1M_GROUP(2) C1M_GROUP(2) C1M_GROUP(1) C1M_GROUP(1) C1M_GROUP(1) C1M_GROUP(1) C1M_GROUP(1) C1M_GROUP(1)
#undef C1M_GROUP
    }
#ifdef DVSG_STAMPS
    { const unsigned long long n_ = C1_STAMP(); m_work += n_ - m_t; m_t = n_; }
#endif
    __syncthreads();
#ifdef DVSG_STAMPS
    { const unsigned long long n_ = C1_STAMP(); m_wait += n_ - m_t; m_t = n_; }
#endif
  }
  flush_quad(nq - 1);
#ifdef DVSG_STAMPS
  if (tid == 0 && blockIdx.x < 65536) {
    unsigned long long *o = g_c1_stamps + (size_t)blockIdx.x * 8;
    o[0] = m_work;    // multiplying wave: fragment reads + MFMAs, all steps
    o[1] = m_wait;    // multiplying wave: waiting at the step barriers
    o[2] = m_flush;   // multiplying wave: bias / ReLU / stores between quads
    o[3] = (unsigned long long)nsteps;
    o[6] = C1_STAMP() - m_begin;
  }
#endif
}

// ----------------------------------------------------------------------------------------
// conv1 for the "f32s" precision: conv1_kernel's decomposition and staging (one output row x 128 pixels x
// 64 channels per workgroup, the input row segment prefetched into registers under the previous kernel
// row's MFMAs, scale_RGB applied while staging, overlapping windows read in place), with the products
// formed on the float16 matrix cores from two float16 pieces per operand (cnn_kernels.h, conv_gemm.hip).
// The scaled input is split ONCE, when it is staged -- hi = f16(v), lo = f16(v - hi), two float16 images
// of the row in LDS, together as large as the float32 row was -- so the 7 overlapping windows and the two
// channel halves that read an element do not split it again: a lane's operand is 8 consecutive taps =
// 16 bytes at byte offset 84 pixel + 32 step + 16 h of either image, four ds_read_b32 (21 r mod 32 is a
// bijection: conflict-free).  The weights' pieces sit in LDS as two [64][168]-half images per kernel row
// (336-byte rows: conflict-free ds_read_b128), prefetched through registers like the input.  The scaled
// input reaches +-150, which would amplify the absolute error of an unscaled lo weight piece, so here
// lo_w = f16((w - hi_w) x 2^11) and its products accumulate apart, folded in with 2^-11 at the end.
// Ten 16-tap steps per kernel row (147 taps padded to 160 with zero weights): 60 MFMAs of 32 cycles per
// wave and kernel row where the exact kernel issues 150 of 64.
// ----------------------------------------------------------------------------------------
constexpr int C1S_SEG = 5504;                        // halves per staged image of the row (1 + 5481 + tail; reads reach 5495)
constexpr int C1S_IN4 = (C1S_SEG / 4 + 255) / 256;     // 6 groups of four elements per thread
constexpr int C1S_WHALFS = 2 * 64 * kConv1LdH;       // halves per kernel row: hi image, then lo image
constexpr int C1S_WBYTES = C1S_WHALFS * 2;           // 43008

template <typename TO, int SRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv1_split_kernel(const Conv1Src src, const _Float16 *__restrict__ wt1s, const float *__restrict__ bias,
                        TO *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles) {
  constexpr int NT = 256;
  constexpr int WLOADS = (C1S_WBYTES / 16 + NT - 1) / NT;    // 11 float4
  static_assert(C1_TILE * C1_LDC * 4 <= C1S_WBYTES, "epilogue tile must fit in the weight stage");
  __shared__ __attribute__((aligned(16))) char w_s[C1S_WBYTES];
  __shared__ __attribute__((aligned(16))) unsigned in_hi[C1S_SEG / 2], in_lo[C1S_SEG / 2];  // half2 per word
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;   // wave w: pixels [32 w, 32 w + 32) x all 64 channels (two 32-channel blocks):
                                            // an activation fragment is read once for both blocks (the LDS is this kernel's bound)

  const Conv1Tile tile = conv1_tile(wtiles, Ho);
  const int b = tile.b, ho = tile.ho, wo0 = tile.wo0;

  typedef typename Conv1RowSel<NT, C1S_IN4, SRC>::type Row;
  Row row;
  row.init(src, tid, b, wo0, H, W, C1S_SEG);
  if constexpr (Row::kRing) {
    for (int e = tid; e < C1S_SEG / 2; e += NT) in_hi[e] = in_lo[e] = 0u;
  }
  typename Row::Data rd;
  floatx4 w_reg[WLOADS];
  auto load_stage = [&](int kh) __attribute__((always_inline)) {
    row.load(rd, 2 * ho + kh - 3);
    const floatx4 *wsrc = reinterpret_cast<const floatx4 *>(wt1s + (size_t)kh * C1S_WHALFS);
#pragma unroll
    for (int i = 0; i < WLOADS; ++i) {
      const int q = tid + NT * i;
      w_reg[i] = wsrc[q < C1S_WBYTES / 16 ? q : 0];
    }
  };
  auto store_stage = [&]() __attribute__((always_inline)) {
    typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
    if constexpr (Row::kRing) {
      row.scatter(rd, [&](int e, float v) __attribute__((always_inline)) {
        const _Float16 hv = (_Float16)v;
        reinterpret_cast<_Float16 *>(in_hi)[e] = hv;
        reinterpret_cast<_Float16 *>(in_lo)[e] = (_Float16)(v - (float)hv);
      });
    } else {
#pragma unroll
      for (int i = 0; i < C1S_IN4; ++i) {
        const int q = tid + NT * i;
        const floatx4 v = row.scaled(rd, i);   // then the two pieces
        half4_t hv, lv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          hv[j] = (_Float16)v[j];
          lv[j] = (_Float16)(v[j] - (float)hv[j]);
        }
        if (q < C1S_SEG / 4) {
          reinterpret_cast<half4_t *>(in_hi)[q] = hv;
          reinterpret_cast<half4_t *>(in_lo)[q] = lv;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WLOADS; ++i) {
      const int q = tid + NT * i;
      if (q < C1S_WBYTES / 16) reinterpret_cast<floatx4 *>(w_s)[q] = w_reg[i];
    }
  };

  floatx16 acc[2], accl[2];   // [channel block]
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[ni][q] = accl[ni][q] = 0.f;

  load_stage(0);
  for (int kh = 0; kh < 7; ++kh) {
    __syncthreads();  // everyone is done reading the previous kernel row
    store_stage();
    __syncthreads();
    if (kh + 1 < 7) load_stage(kh + 1);
    __builtin_amdgcn_sched_barrier(0);  // prefetch stays ahead of the MFMA loop
    // word index of the lane's first tap pair: (42 pixel + 8 h) / 2
    const int a0 = kConv1Cin * (wave * 32 + r) + 4 * h;
    const _Float16 *bhi0 = reinterpret_cast<const _Float16 *>(w_s) + r * kConv1LdH + 8 * h;
    const _Float16 *blo0 = bhi0 + 64 * kConv1LdH;
    // software-pipelined: the fragments of step t + 1 are requested before the MFMAs of step t are issued (left to
    // itself the compiler waits for each pair of steps' reads with nothing in flight)
    struct Frag {
      union {
        unsigned u[4];
        halfx8 v;
      } ahi, alo;
      halfx8 bhi[2], blo[2];
    };
    auto read_frag = [&](Frag &f, int t) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f.ahi.u[j] = in_hi[a0 + 8 * t + j];
        f.alo.u[j] = in_lo[a0 + 8 * t + j];
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        f.bhi[ni] = *reinterpret_cast<const halfx8 *>(bhi0 + ni * 32 * kConv1LdH + 16 * t);
        f.blo[ni] = *reinterpret_cast<const halfx8 *>(blo0 + ni * 32 * kConv1LdH + 16 * t);
      }
    };
    Frag fr[2];
    read_frag(fr[0], 0);
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      if (t + 1 < 10) read_frag(fr[(t + 1) & 1], t + 1);
      __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the MFMAs that do not need them
      const Frag &f = fr[t & 1];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ahi.v, f.bhi[ni], acc[ni], 0, 0, 0);
        acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.alo.v, f.bhi[ni], acc[ni], 0, 0, 0);
        accl[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.ahi.v, f.blo[ni], accl[ni], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: fold the scaled lo products in, transpose through the (idle) weight stage
  float *Cs = reinterpret_cast<float *>(w_s);
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
    C1_TILE_PUT(Cs, wave * 32, ni * 32, acc[ni][q] + accl[ni][q] * (1.0f / 2048.0f));
  __syncthreads();
  const int col4 = tid & 15;
  conv1_tile_out<16>(Cs, conv1_tile_bias(bias, tid), tid, wo0, Wo, [&](int row, float4 v) __attribute__((always_inline)) {
    store4_p(y, (((size_t)b * Ho + ho) * Wo + wo0 + row) * 64 + 4 * col4, v);   // float16 pieces (cnn_device.h)
  });
}

}  // namespace

// Bands of the marching kernel: the launch must give each of the 256 CUs (one workgroup each) several bands' worth of
// work, and a band should be long enough to amortise its first window (4 + 4 rows staged with nothing to multiply): at
// least 3 workgroups per CU with >= 4 quads (16 output rows) per band, else 0 = do not use the kernel.  Returns the number
// of bands per column tile and image; *quads_per_band the quads of each.
int march_bands(int B, int Ho, int wtiles, int *quads_per_band) {
  const int quads = (Ho + C1M_QUAD - 1) / C1M_QUAD;
  const long cols = (long)B * wtiles;
  for (int qpb = 8; qpb >= 4; --qpb) {               // 32 .. 16 output rows per band
    const int bands = (quads + qpb - 1) / qpb;
    if (cols * bands >= 3 * 256) {
      if (quads_per_band) *quads_per_band = qpb;
      return bands;
    }
  }
  return 0;
}

static_assert(C1M_QUAD == kConv1MarchQuad, "choose_conv1 sizes the forced bands by the quad");

bool launch_conv1_f16_mfma(const Conv1Choice &c, const Conv1Args &a) {
  const Conv1Src &src = a.src;
  const _Float16 *const wt1h = a.wt.f16;   // the float16 precision's image; conv1_split_kernel reads a.wt.pieces
  const float *const bias = a.wt.bias;
  const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo, wtiles = a.wtiles;
  hipStream_t s = a.s;
  const dim3 grid((unsigned)((long)wtiles * Ho * a.B));
  switch (c.family) {
    case kConv1F16:
      return with_conv1_src<false>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        hipLaunchKernelGGL((conv1_f16_kernel<_Float16, S>), grid, dim3(256), 0, s, src, wt1h, bias, static_cast<_Float16 *>(a.y), H, W,
                           Ho, Wo, wtiles);
      });
    case kConv1F16March: {
      const int bands = c.bands, qpb = c.per_band;
      const dim3 mgrid((unsigned)((long)wtiles * bands * a.B));
      return with_conv1_src<false>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        hipLaunchKernelGGL((conv1_f16_march_kernel<S>), mgrid, dim3(512), 0, s, src, wt1h, bias, static_cast<_Float16 *>(a.y), H, W, Ho,
                           Wo, wtiles, bands, qpb);
      });
    }
    case kConv1F16Pair: {
      const int hpairs = (Ho + 1) / 2;
      const dim3 pgrid((unsigned)((long)wtiles * hpairs * a.B));
      return with_conv1_src<true>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        hipLaunchKernelGGL((conv1_f16_pair_kernel<_Float16, S>), pgrid, dim3(256), 0, s, src, wt1h, bias, static_cast<_Float16 *>(a.y),
                           H, W, Ho, Wo, wtiles, hpairs);
      });
    }
    case kConv1Split:   // f32s: float32 in and out, the products from float16 pieces
      return with_conv1_src<true>(c.src, [&](auto src_c) {
        constexpr int S = decltype(src_c)::value;
        hipLaunchKernelGGL((conv1_split_kernel<float, S>), grid, dim3(256), 0, s, src, a.wt.pieces, bias, static_cast<float *>(a.y),
                           H, W, Ho, Wo, wtiles);
      });
    default:
      return false;
  }
}

#ifdef DVSG_STAMPS
extern "C" int dvsg_debug_read_march_stamps(void *host, size_t bytes) {   // conv1_f16_march_kernel's (tools/stamp_probe_march.py)
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_c1_stamps), bytes) == hipSuccess ? 0 : -3;
}
#endif

}  // namespace dvsg
