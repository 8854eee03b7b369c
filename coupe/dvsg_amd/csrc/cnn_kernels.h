// Launch interface of the localizationNet kernels (conv_gemm.hip, conv1.hip and the conv1_*.hip kernel files, root_pool.hip, head.hip),
// used by locnet.hip.
//
// `Precision` is the network's notion: what an entry point was asked for, and the storage of the activations between layers.
//   kF32   float32 activations / weights, exact-f32 matrix cores (v_mfma_f32_32x32x2_f32): the path of record
//   kF32S  4 bytes per value and float32 accumulation, but every product is formed on the float16 matrix cores from two
//          float16 pieces per operand (22 significant bits for |x| >= 2^-3, absolute step 2^-24 below: the second piece is
//          unscaled; conv_gemm.hip), and the activation tensors between the layers hold those pieces (P format, cnn_device.h);
//          values must stay inside float16's range (|x| < 65504), which post-BatchNorm activations and BN-folded
//          weights do by orders of magnitude
//   kF16   float16 activations, v_mfma_f32_32x32x16_f16 with float32 accumulation; bias, accumulators and the dense head
//          stay float32
//   kF32X  ("f32x3") float32 tensors everywhere, exactly as kF32; inside the 52 conv GEMMs every product is formed on the
//          bfloat16 matrix cores from THREE bfloat16 pieces per operand -- all 24 significant bits of both float32 operands,
//          at any magnitude -- as six v_mfma_f32_32x32x16_bf16 with float32 accumulation (conv_gemm_tile.h, X3)
// `ConvMath` is one conv launch's: what it multiplies, which fixes the weight image it reads (ConvWeights) and the tensors'
// element type (storage_of).  kF16 has two: a layer's weights as float16 hi / lo pairs or as one plain float16 (locnet.hip's
// pair policy chooses per layer).  All five share the kernels through template parameters.
#pragma once
#include <type_traits>

#include "common.h"

namespace dvsg {

enum Precision { kF32 = 0, kF16 = 1, kF32S = 2, kF32X = 3 };
constexpr size_t elem_size(int prec) { return prec == kF16 ? 2 : 4; }
// kMathF32       float32 tensors and weight rows, exact products
// kMathF32S      P-format tensors; weights [Cout][K/32][32 hi halves | 32 lo halves], products from float16 pieces
// kMathF32X      float32 tensors; weights are the layer's packed bfloat16 piece stages (launch_pack_x3)
// kMathF16Pairs  float16 tensors; weights stacked [Cout/64][128][K] (64 hi rows, then 64 lo rows)
// kMathF16Plain  float16 tensors; weights [Cout][K] float16
enum ConvMath { kMathF32, kMathF32S, kMathF32X, kMathF16Pairs, kMathF16Plain };
constexpr Precision storage_of(ConvMath m) { return m == kMathF32S ? kF32S : m == kMathF16Pairs || m == kMathF16Plain ? kF16 : kF32; }
constexpr ConvMath math_of(int prec, bool pairs) {
  return prec == kF16 ? (pairs ? kMathF16Pairs : kMathF16Plain) : prec == kF32S ? kMathF32S : prec == kF32X ? kMathF32X : kMathF32;
}
constexpr size_t elem_size(ConvMath m) { return elem_size((int)storage_of(m)); }
static_assert(storage_of(kMathF32) == kF32 && storage_of(kMathF32X) == kF32 && storage_of(kMathF32S) == kF32S &&
              storage_of(kMathF16Pairs) == kF16 && storage_of(kMathF16Plain) == kF16, "ConvMath -> storage format");
static_assert(math_of(kF32, false) == kMathF32 && math_of(kF32, true) == kMathF32 && math_of(kF32S, false) == kMathF32S &&
              math_of(kF32S, true) == kMathF32S && math_of(kF32X, false) == kMathF32X && math_of(kF32X, true) == kMathF32X &&
              math_of(kF16, true) == kMathF16Pairs && math_of(kF16, false) == kMathF16Plain, "(Precision, pairs) -> ConvMath");
static_assert(elem_size(kMathF32) == 4 && elem_size(kMathF32S) == 4 && elem_size(kMathF32X) == 4 &&
              elem_size(kMathF16Pairs) == 2 && elem_size(kMathF16Plain) == 2, "ConvMath -> bytes per tensor element");

// One layer's weights as a ConvMath reads them: the row matrix, and for the float16 maths optionally its rows packed stage
// by stage for conv_gemm_wide16.hip (launch_pack_wide16): order 0, order 1 (its 128-byte-activation-row kernel) and order 2
// (its 3x3 stride-1 kernel: a kernel row's taps from one staged run)
struct ConvWeights {
  const void *rows = nullptr, *packed = nullptr, *packed_a = nullptr, *packed_h = nullptr;
};

// Implicit-GEMM convolution (1x1 or 3x3, NHWC, C_in % 64 == 0 (f16) / 32 (f32), C_out % 64 == 0):
//   y[m, n] = act( sum_k A[m, k] * wt[n, k] + bias[n] (+ res[...]) )
// with m = (b, ho, wo), k = (kh, kw, c).  The weights are [C_out][K] in the math's layout (K contiguous, BN scale folded in).
struct ConvGemm {
  ConvMath math;      // what is multiplied; x, res, y are tensors of storage_of(math)
  const void *x;      // [B,H,W,Cin]
  ConvWeights w;
  const float *bias;  // [Cout]
  const void *res;    // optional residual [B,res_H,res_W,Cout], sampled at (ho*res_stride, wo*res_stride)
  void *y;            // [B,Ho,Wo,Cout]
  int B, H, W, Cin, Ho, Wo, Cout;
  int ksize, stride, pad;
  int res_H, res_W, res_stride;
  int relu;
  // 4-byte storage only (0 / -1 = the dense defaults): x and res may be column ranges of wider tensors -- ldx, res_ld elements
  // between two pixels -- and, with relu == 0, output channels >= relu_from get the ReLU all the same: a unit's `shortcut`
  // (no ReLU) and `conv1` (ReLU) read the same input and run as ONE launch over their concatenated weight rows (locnet.hip)
  int ldx = 0, res_ld = 0, relu_from = -1;
  // optional split-K scratch (small batches): partial-tile slabs and kSplitKMaxTiles zeroed int tickets
  void *splitk_scratch = nullptr;
  size_t splitk_scratch_bytes = 0;
  int *splitk_counters = nullptr;
};
constexpr int kSplitKMaxTiles = 512;                                   // tickets one launch may use
constexpr size_t kSplitKSlabBytes = (size_t)512 * 2 * 128 * 128 * 4;   // 64 MiB: 512 workgroups x 2 partial 128x128 f32 tiles (stream-K tail)
int launch_conv_gemm(const ConvGemm &p, hipStream_t s);
// diagnostic record of the last conv_gemm_kernel launch (dvsg_debug_last_conv_config): T (0 float32 tensors, 1 float16),
// BN, WM, WN, KS, RELU, RES, MODE, SPLIT, X3, ksplit, streamk_tail, mt_fast; T = -1 when the last launch_conv_gemm call did
// not end in conv_gemm_kernel (g_last_conv_kernel then names the kernel that ran) or there was none.  Host-only; written by
// launch_cfg
constexpr int kConvConfigFields = 13;
extern int g_last_conv_config[kConvConfigFields];
// diagnostic record of the last conv kernel launch of any family (dvsg_debug_last_conv_kernel): family (0 conv_gemm_kernel,
// 1 conv_wide16_kernel, 2 conv_wide16a_kernel, 3 conv_wide16h_kernel, 4 conv3x3_1x1_kernel, 5 conv3x3_1x1_x3_kernel,
// 6 conv3x3_1x1_f16_kernel, 7 conv3x3_1x1_f16h_kernel), the family's template arguments in declaration order padded with -1
// (family 0: all -1, its details are g_last_conv_config), and for families 1-3 where the weight stages came from (0 the
// [rows][K] layout, 1 the packed copy), else -1.  Reset by launch_conv_gemm, launch_conv_wide16 and the launch_conv3x3_1x1*
// calls, written where they issue the launch.  Host-only
constexpr int kConvKernelFields = 6;
extern int g_last_conv_kernel[kConvKernelFields];
inline void record_conv_kernel(int family, int a0 = -1, int a1 = -1, int a2 = -1, int a3 = -1, int wsrc = -1) {
  const int rec[kConvKernelFields] = {family, a0, a1, a2, a3, wsrc};
  for (int i = 0; i < kConvKernelFields; ++i) g_last_conv_kernel[i] = rec[i];
}
inline void reset_conv_kernel() { record_conv_kernel(-1); }
// Run-time (relu, res) -> compile-time constants, for the conv kernels' RELU and RES template arguments: calls
// f(std::bool_constant<RELU>, std::integral_constant<int, RES>) with RES = 0 (no residual), 1 (a tensor of the output's
// shape) or 2 (slim `subsample`: any other value of res)
template <typename F>
void with_relu_res(bool relu, int res, F &&f) {
  auto with_res = [&](auto relu_c) {
    if (res == 0) f(relu_c, std::integral_constant<int, 0>{});
    else if (res == 1) f(relu_c, std::integral_constant<int, 1>{});
    else f(relu_c, std::integral_constant<int, 2>{});
  };
  if (relu) with_res(std::true_type{});
  else with_res(std::false_type{});
}
// f32x3 weights: float32 wt [rows][K] (rows % 64 == 0, K % 32 == 0) -> per group of 64 rows and 32-k stage three 4 KB planes
// of bfloat16 pieces [64 rows][32 k] (p1 = bf16(w), p2 = bf16(w - p1), p3 = bf16(w - p1 - p2)), row R's 16-byte chunk c at
// position c ^ ((R >> 2) & 3): 6 bytes per weight, [rows / 64][K / 32][3][64][32]
inline size_t x3_packed_bytes(int rows, int K) { return (size_t)rows * K * 6; }
int launch_pack_x3(const float *wt, void *out, int rows, int K, hipStream_t s);
// float16 mode, big launches: 256 x 128 tiles with 64-byte K stages (conv_gemm_wide16.hip); called by launch_conv_gemm
int launch_conv_wide16(const ConvGemm &p, hipStream_t s);
// weights packed for that kernel: every 32-k stage of a 128-row tile contiguous, in the LDS image's chunk order
size_t wide16_packed_bytes(int rows, int Cin, int ksize);
int launch_pack_wide16(const void *wt, void *out, int rows, int Cin, int ksize, int order, hipStream_t s);
// Zeroes n split-K / stream-K tickets with a KERNEL: a hipMemsetAsync captured into a HIP graph (memset node) did not
// take effect on the second and later replays of the graph on ROCm 7.2 (tests/test_gpu_cnn.py::test_a_step_replays_...).
int launch_zero_tickets(int *tickets, size_t n, hipStream_t s);
// conv2 (3x3, Cin -> 64, stride 1/2, pad 1, + bias + ReLU) followed by conv3 (1x1, 64 -> Cout, + bias +
// residual + ReLU) of a bottleneck unit whose middle width is 64 (block 1), fused: the [M,64]
// intermediate stays in LDS.
struct ConvFused {
  // every math but kMathF16Plain (the float16 kernels multiply by the stacked pairs only); x, res / sc_x, y are tensors of
  // storage_of(math) and wt2, wt3, sc_wt the layers' ConvWeights::rows for it.  kMathF32X: the residual is a tensor (no fused
  // shortcut), conv_fused_x3.hip
  ConvMath math = kMathF32;
  const void *x;       // [B,H,W,Cin]
  const void *wt2;     // [64][9*Cin]
  const float *bias2;  // [64]
  const void *wt3;     // [Cout][64]
  const float *bias3;  // [Cout]
  const void *res;     // [B,res_H,res_W,Cout], sampled at (ho*res_stride, wo*res_stride); NULL with sc_x
  void *y;             // [B,Ho,Wo,Cout]
  int B, H, W, Cin, Ho, Wo, Cout;
  int stride;
  int res_H, res_W, res_stride;
  // the unit that opens a block: residual = 1x1 `shortcut` conv (+ BN) of the unit's input, computed in the
  // kernel from sc_x [B,Ho,Wo,sc_cin] (stride 1), sc_wt [Cout][sc_cin], sc_bias [Cout]; the tensor never exists
  const void *sc_x = nullptr;
  const void *sc_wt = nullptr;
  const float *sc_bias = nullptr;
  int sc_cin = 0;
};
int launch_conv3x3_1x1_x3(const ConvFused &p, hipStream_t s);
bool conv_fusable(int prec, int Cin, int Cmid, int Cout, int ksize);   // a predicate of precision and shape alone
int launch_conv3x3_1x1(const ConvFused &p, hipStream_t s);

// conv1: 7x7 stride 2, explicit pad 3, C_in = 21 -> 64, with scale_RGB fused into the LDS
// load stage (networks.py:6-16 + slim conv2d_same root).  wt1 is [7][64][kConv1Ld] float32:
// per kernel row kh, per output channel, a zero tap and then the 7*21 (kw, c) taps in memory order
// of the input row (tap k at index k + 1: the kernels stage the input row from one element before the
// window, which is a 16-byte boundary of the row), BN scale folded, channel-group reversal folded.
constexpr int kConv1Cin = 21;
constexpr int kConv1K = 7 * kConv1Cin;   // 147 taps per kernel row
constexpr int kConv1Kpad = 148;          // zero tap + 147, a whole number of 4-k MFMA steps
constexpr int kConv1Ld = 150;            // LDS / global row stride (2*odd: conflict-free ds_read_b64)
// wt1h (float16 precision only): the same row as [7][64][kConv1LdH] float16, zero-padded to 160.
constexpr int kConv1LdH = 168;
// wt1s ("f32s" precision only): float16 pieces [7][2][64][kConv1LdH], same tap positions: hi = f16(w), lo = f16((w - hi) * 2^11).
// conv1's input: the window tensor [B,H,W,21] float32 the reference feeds (eval.py:106-110), or -- SURVEY.md 8f-1/-2 --
// a pool of RGB frames [n_pool,H,W,3] (float32 in [0,1], or raw uint8 whose / 255. is fused) plus the table [B,7] of
// the pool frame in each window slot, oldest to newest: the np.concatenate of eval.py:103-104 happens in the load stage.
// wt1x ("f32x3" precision only): bfloat16 pieces [14][3][64][kConv1X3Ld]: stage 2 kh + half holds taps [80 half, 80 half + 80)
// of kernel row kh (position p = tap + 1 behind the zero tap, as in wt1h; positions 148..159 zero) as three piece planes,
// p1 = bf16(w), p2 = bf16(w - p1), p3 = bf16(w - p1 - p2); rows zero-padded from 80 to 88.
constexpr int kConv1X3Ld = 88;
constexpr int kConv1X3StageElems = 3 * 64 * kConv1X3Ld;   // 16 896 bfloat16 per half kernel row
// Any other window length S (cin = 3 S, 1 <= S <= kRootMaxFrames) runs rootconv_kernel, which takes cin as an argument and
// reads the float32 image only: wt1 is then [7][64][rootconv_ld(cin)], tap (kw, c) of kernel row kh at kw * pitch + c with
// pitch = rootconv_pitch(cin) -- the LDS pixel pitch, cin made odd (see the kernel) -- and zeros everywhere else.
constexpr int kRootMaxFrames = 16;
constexpr int rootconv_pitch(int cin) { return cin | 1; }
constexpr int rootconv_kpad(int cin) { return (7 * rootconv_pitch(cin) + 3) & ~3; }   // a whole number of 4-k MFMA steps
constexpr int rootconv_ld(int cin) { return rootconv_kpad(cin) + 2; }                 // 2 x odd, like kConv1Ld
// diagnostic record of the root and the head of the last network call (dvsg_debug_last_root_kernel): conv1 family (0
// conv1_kernel, 1 conv1_f16_kernel, 2 conv1_f16_pair_kernel, 3 conv1_f16_march_kernel, 4 conv1_split_kernel, 5
// conv1_x3_kernel, 6 rootconv_kernel: cin != 21, 7 root_band_kernel), its template arguments NW, TO (0 float, 1 _Float16, 2
// the P format: rootconv_kernel only), SRC (-1 where the family has none; rootconv_kernel records NW = 4, root_band_kernel
// NW = 8 and TO = 0), the marching kernel's bands and quads_per_band or the band kernel's bands and (longest band's) row
// pairs per band (else -1), the max pool kernel (0 maxpool_kernel<float>, 1 maxpool_kernel<_Float16>, 2
// maxpool_h8_kernel, 3 maxpool_p_kernel, 4 root_pool_seams_kernel: family 7 then was root_band_pool_kernel, the pool in
// conv1's epilogue), the average pool kernel (0 avgpool_partial_kernel<float>, 1 <_Float16>, 2
// avgpool_partial_p_kernel) and the number of dense batch chunks.  Reset to -1 by forward(), written where launch_conv1,
// launch_maxpool, launch_root_pool_seams, launch_avgpool_partial and forward() issue the launches.  Host-only
constexpr int kRootKernelFields = 9;
enum RootKernelField { kRootConv1 = 0, kRootNW, kRootTO, kRootSRC, kRootBands, kRootQuads, kRootMaxpool, kRootAvgpool,
                       kRootDenseChunks };
extern int g_last_root_kernel[kRootKernelFields];
inline void reset_root_kernel() {
  for (int i = 0; i < kRootKernelFields; ++i) g_last_root_kernel[i] = -1;
}
inline void record_conv1_kernel(int family, int nw, int to, int src, int bands = -1, int quads = -1) {
  const int rec[6] = {family, nw, to, src, bands, quads};
  for (int i = 0; i < 6; ++i) g_last_root_kernel[i] = rec[i];
}
enum Conv1SrcKind { kSrcWindow = 0, kSrcRingF32 = 1, kSrcRingU8 = 2 };
// SRC, the conv1 kernels' template argument and the launch record's field: where the input comes from and how it is staged
constexpr int kSrcAligned = 1;     // bit 0: rows on the 16-byte (4-byte for uint8) grid
constexpr int kSrcKindShift = 1;   // bits 1-2: the Conv1SrcKind
constexpr int kSrcMasked = 8;      // bit 3: the history channels are multiplied by src.mask (eval_train.py's graph)
constexpr int conv1_src(int kind, bool aligned, bool masked) {
  return (kind << kSrcKindShift) | (aligned ? kSrcAligned : 0) | (masked ? kSrcMasked : 0);
}
struct Conv1Src {
  const void *base;   // window tensor, or frame pool
  const int *table;   // ring: [B,S] pool indices (device), S = cin / 3; an index outside [0, n_pool) stages zeros
  int n_pool;
  const float *mask = nullptr;   // optional [B,H,W]: eval_train.py:43-45,53-64 -- the 3 (S - 1) history channels of window b are multiplied
                                 // by mask[b] (one plane: the warp of an all-ones image is the same in every channel) in the load stage
};
// conv1's weight images (the layouts above); the images a precision does not use may be NULL, and cin != 21 has `f32` only
struct Conv1Weights {
  const float *f32;            // wt1
  const _Float16 *f16;         // wt1h
  const _Float16 *pieces;      // wt1s
  const unsigned short *x3;    // wt1x
  const float *bias;           // [64]
};
// The root max pool inside conv1: where `pool` is given (the caller has checked: float32, no pad on the pool's top and left,
// nobody reads conv1's output) and launch_conv1 takes the band kernel, it may run root_band_pool_kernel instead (debug
// option root_pool) -- the pooled tensor goes to `pooled`, whole but for the elements on a tile or band seam, and of `y` only
// the conv values those elements still miss are written.  `fused` then is set and launch_root_pool_seams must follow on the
// same stream in place of launch_maxpool; otherwise conv1 ran as without `pool`.
struct RootPool {
  void *pooled;                     // [B, Ho / 2, Wo / 2, 64] float32
  bool fused = false;               // out
  int bands = 0, ppb = 0, nbig = 0; // out: the launch's band split, which decides the row seams
};
int launch_conv1(int out_prec, const Conv1Src &src, int src_kind, const Conv1Weights &wt, void *y, int B, int H, int W, int Ho,
                 int Wo, int cin, hipStream_t s, RootPool *pool = nullptr);
// finishes the seam elements of a fused launch from the conv values in `conv_taps` (launch_conv1's y); records max pool kernel 4
int launch_root_pool_seams(const RootPool &pool, const void *conv_taps, int B, int Ho, int Wo, hipStream_t s);
// rootconv_kernel declares its LDS per launch (up to 140 KB at cin = 48): raises every instantiation's dynamic LDS limit.
// Called once per handle by dvsg_locnet_create for cin != 21, outside any stream operation
int prepare_rootconv();
// root_band_kernel (float32, cin = 21, big unmasked launches) declares 142 656 bytes of LDS, root_band_pool_kernel 159 040:
// raises their instantiations' dynamic LDS limits.  Called once per handle by dvsg_locnet_create for cin == 21, outside any stream operation
int prepare_root_band();

// 3x3 stride-2 TF-SAME max pool (slim resnet root), C % 8 == 0.
int launch_maxpool(int prec, const void *x, void *y, int B, int H, int W, int C, int Ho, int Wo, int pad_top,
                   int pad_left, hipStream_t s);

// Global average pool as float32 partial sums: part[b][s][c] = sum over the s-th slice of HW.
constexpr int kPoolSplits = 8;
int launch_avgpool_partial(int prec, const void *x, float *part, int B, int HW, int C, hipStream_t s);

// Element-wise float16 -> float32 (parity taps of a float16 run).
int launch_f16_to_f32(const void *x, float *y, size_t n, hipStream_t s);
// P format ("f32s" activations: float16 pieces, cnn_device.h) <-> float32; n % 32 == 0.
int launch_p_to_f32(const void *x, float *y, size_t n, hipStream_t s);
int launch_f32_to_p(const float *x, void *y, size_t n, hipStream_t s);

// Dense layer on split partial sums (see head.hip); float32 throughout.
constexpr int kDenseSplits = 8;
int launch_dense(const float *xin, int s_in, const float *bias_in, float scale_in, int lrelu_in,
                 const float *W, float *out_part, int B, int K, int N, hipStream_t s);
// out[b][n] = scale * sum_s part[b][s][n] + bias[n] (bias may be NULL)
int launch_dense_finalize(const float *part, int s_in, float scale, const float *bias, float *out, int B,
                          int N, hipStream_t s);

}  // namespace dvsg
