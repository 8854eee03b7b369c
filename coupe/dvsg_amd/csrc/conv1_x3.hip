// The root conv of the f32x3 precision (conv1.hip describes the root): conv1_x3_kernel, its products formed on the bfloat16
// matrix cores from three bfloat16 pieces per operand.
#include "conv1_device.h"
#include "conv1_internal.h"

namespace dvsg {
namespace {

// ----------------------------------------------------------------------------------------
// "f32x3" conv1: float32 in, float32 out, every product from THREE bfloat16 pieces per operand (conv_gemm_tile.h, X3: all 24
// bits of both operands, six of the nine cross terms, the five small ones in their own accumulators).  Built like
// conv1_split_kernel: the scaled input row is split ONCE while it is staged -- three bfloat16 images of the row in LDS, 33 KB
// -- so the loop holds LDS reads and MFMAs only (a split in registers would be ~40 VALU per fragment that the matrix pipe
// does not hide, tools/x3_overlap_probe.hip).  The weight pieces of a kernel row are 3 x 64 x 160 bfloat16 = 61 KB, too many
// for two workgroups per CU next to the input images: a kernel row is staged as two HALVES of 80 taps (5 MFMA steps each,
// [piece][64][88] bfloat16 = 33 KB; 176-byte rows: 11 sixteen-byte slots, odd, so a ds_read_b128 lane group is conflict-free),
// 14 stages per tile, the input images restaged at every other one.
// ----------------------------------------------------------------------------------------
constexpr int C1X_SEG = 5504;                        // bfloat16 per staged image of the row (1 + 5481 + tail; reads reach 5495)
constexpr int C1X_IN4 = (C1X_SEG / 4 + 255) / 256;     // 6 groups of four elements per thread
constexpr int C1X_WBYTES = kConv1X3StageElems * 2;   // 33 792 bytes per half kernel row
constexpr int C1X_WS = C1_TILE * C1_LDC * 4;         // the weight stage also holds the epilogue's transpose tile (34 816)
static_assert(C1X_WS >= C1X_WBYTES, "weight stage smaller than a half kernel row");

template <int SRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv1_x3_kernel(const Conv1Src src, const unsigned short *__restrict__ wt1x, const float *__restrict__ bias,
                     float *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles) {
  constexpr int NT = 256;
  constexpr int WLOADS = (C1X_WBYTES / 16 + NT - 1) / NT;    // 9 float4
  __shared__ __attribute__((aligned(16))) char w_s[C1X_WS];
  __shared__ __attribute__((aligned(16))) unsigned in_p[3][C1X_SEG / 2];  // two bfloat16 per word
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;   // wave w: pixels [32 w, 32 w + 32) x all 64 channels (two 32-channel blocks)

  const Conv1Tile tile = conv1_tile(wtiles, Ho);
  const int b = tile.b, ho = tile.ho, wo0 = tile.wo0;

  typedef typename Conv1RowSel<NT, C1X_IN4, SRC>::type Row;
  Row row;
  row.init(src, tid, b, wo0, H, W, C1X_SEG);
  if constexpr (Row::kRing) {
    for (int e = tid; e < C1X_SEG / 2; e += NT) in_p[0][e] = in_p[1][e] = in_p[2][e] = 0u;
  }
  typename Row::Data rd;
  floatx4 w_reg[WLOADS];
  auto load_stage = [&](int st) __attribute__((always_inline)) {   // stage st: kernel row st / 2, taps [80 (st & 1), + 80)
    if ((st & 1) == 0) row.load(rd, 2 * ho + (st >> 1) - 3);
    const floatx4 *wsrc = reinterpret_cast<const floatx4 *>(wt1x + (size_t)st * kConv1X3StageElems);
#pragma unroll
    for (int i = 0; i < WLOADS; ++i) {
      const int q = tid + NT * i;
      w_reg[i] = wsrc[q < C1X_WBYTES / 16 ? q : 0];
    }
  };
  auto pieces = [](float v, __bf16 &p1, __bf16 &p2, __bf16 &p3) __attribute__((always_inline)) {
    p1 = (__bf16)v;
    const float r1 = v - (float)p1;
    p2 = (__bf16)r1;
    p3 = (__bf16)(r1 - (float)p2);
  };
  auto store_stage = [&](int st) __attribute__((always_inline)) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    if ((st & 1) == 0) {
      if constexpr (Row::kRing) {
        row.scatter(rd, [&](int e, float v) __attribute__((always_inline)) {
          __bf16 p1, p2, p3;
          pieces(v, p1, p2, p3);
          reinterpret_cast<__bf16 *>(in_p[0])[e] = p1;
          reinterpret_cast<__bf16 *>(in_p[1])[e] = p2;
          reinterpret_cast<__bf16 *>(in_p[2])[e] = p3;
        });
      } else {
#pragma unroll
        for (int i = 0; i < C1X_IN4; ++i) {
          const int q = tid + NT * i;
          const floatx4 v = row.scaled(rd, i);   // then the three pieces
          bf16x4 v1, v2, v3;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            __bf16 p1, p2, p3;
            pieces(v[j], p1, p2, p3);
            v1[j] = p1; v2[j] = p2; v3[j] = p3;
          }
          if (q < C1X_SEG / 4) {
            reinterpret_cast<bf16x4 *>(in_p[0])[q] = v1;
            reinterpret_cast<bf16x4 *>(in_p[1])[q] = v2;
            reinterpret_cast<bf16x4 *>(in_p[2])[q] = v3;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WLOADS; ++i) {
      const int q = tid + NT * i;
      if (q < C1X_WBYTES / 16) reinterpret_cast<floatx4 *>(w_s)[q] = w_reg[i];
    }
  };

  floatx16 acc[2], accs[2];   // [channel block]: the large cross term, the five small ones
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[ni][q] = accs[ni][q] = 0.f;

  load_stage(0);
  for (int st = 0; st < 14; ++st) {
    __syncthreads();  // everyone is done reading the previous stage
    store_stage(st);
    __syncthreads();
    if (st + 1 < 14) load_stage(st + 1);
    __builtin_amdgcn_sched_barrier(0);  // prefetch stays ahead of the MFMA loop
    // word index of the lane's first tap pair: (42 pixel + 80 (st & 1) + 8 h) / 2
    const int a0 = kConv1Cin * (wave * 32 + r) + 40 * (st & 1) + 4 * h;
    const __bf16 *b0 = reinterpret_cast<const __bf16 *>(w_s) + r * kConv1X3Ld + 8 * h;
    // software-pipelined: the activation fragments of step t + 1 (4-byte-aligned reads, the slow ones) are requested before the
    // MFMAs of step t are issued; the weight fragments of a step are read when it starts (holding two steps of them as well
    // spills the ring and masked sources' staging registers)
    struct Frag {
      union {
        unsigned u[4];
        bf16x8 v;
      } a[3];
    };
    auto read_a = [&](Frag &f, int t) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) f.a[p].u[j] = in_p[p][a0 + 8 * t + j];
    };
    // (the ring and masked sources hold more staging registers: one set of fragments there, or the kernel spills)
    constexpr bool PIPE = SRC < 2;
    Frag fr[PIPE ? 2 : 1];
    if (PIPE) read_a(fr[0], 0);
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      bf16x8 bw[3][2];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          bw[p][ni] = *reinterpret_cast<const bf16x8 *>(b0 + (p * 64 + ni * 32) * kConv1X3Ld + 16 * t);
      if (PIPE) {
        if (t + 1 < 5) read_a(fr[(t + 1) & 1], t + 1);
      } else {
        read_a(fr[0], t);
      }
      __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the MFMAs that do not need them
      const Frag &f = fr[PIPE ? (t & 1) : 0];
#define DVSG_C1X_TERM(C, PA, PB) \
  _Pragma("unroll") for (int ni = 0; ni < 2; ++ni) C[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[PA].v, bw[PB][ni], C[ni], 0, 0, 0)
      DVSG_C1X_TERM(accs, 2, 0);
      DVSG_C1X_TERM(accs, 0, 2);
      DVSG_C1X_TERM(accs, 1, 1);
      DVSG_C1X_TERM(accs, 1, 0);
      DVSG_C1X_TERM(accs, 0, 1);
      DVSG_C1X_TERM(acc, 0, 0);
#undef DVSG_C1X_TERM
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: join the two accumulators, transpose through the (idle) weight stage
  float *Cs = reinterpret_cast<float *>(w_s);
  __syncthreads();
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
    C1_TILE_PUT(Cs, wave * 32, ni * 32, acc[ni][q] + accs[ni][q]);
  __syncthreads();
  const int col4 = tid & 15;
  conv1_tile_out<16>(Cs, conv1_tile_bias(bias, tid), tid, wo0, Wo, [&](int row, float4 v) __attribute__((always_inline)) {
    store4(y + (((size_t)b * Ho + ho) * Wo + wo0 + row) * 64 + 4 * col4, v);
  });
}

}  // namespace

bool launch_conv1_x3(const Conv1Choice &c, const Conv1Args &a) {
  if (c.family != kConv1X3) return false;
  const dim3 grid((unsigned)((long)a.wtiles * a.Ho * a.B));
  return with_conv1_src<true>(c.src, [&](auto src_c) {
    constexpr int S = decltype(src_c)::value;
    hipLaunchKernelGGL((conv1_x3_kernel<S>), grid, dim3(256), 0, a.s, a.src, a.wt.x3, a.wt.bias, static_cast<float *>(a.y), a.H, a.W,
                       a.Ho, a.Wo, a.wtiles);
  });
}

}  // namespace dvsg
