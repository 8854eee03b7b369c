// Root of resnet_v1_50 (slim `conv2d_same(64, 7, stride=2)` + BatchNorm + ReLU, then
// `max_pool2d(3x3, stride 2, SAME)`) with scale_RGB (networks.py:6-16) fused into conv1's
// load stage.
//
// This file decides which kernel a root conv runs (choose_conv1) and starts it (launch_conv1); it holds no kernel.  The
// kernels are in conv1_f32.hip, conv1_f16.hip and conv1_x3.hip, the max pool's in root_pool.hip, and the device text they
// share -- the staged input row, the tile decode, the epilogue -- in conv1_device.h.
//
// conv1: 7x7 / stride 2 / pad 3, 21 -> 64.
//
// A workgroup owns 128 consecutive output pixels of one output row and all 64 channels.
// For kernel row kh the 7*21 = 147 taps of an output pixel are ONE contiguous run of the
// input row, and neighbouring output pixels start 42 floats apart: the raw input row
// segment (261 px * 21 ch = 5481 floats, 22 KB) is staged once in LDS and every A fragment
// is read from it in place as lds[42 * pixel + k] -- overlapping windows, no im2col, each
// input byte fetched once per kernel row.  42 r mod 64 visits every even bank once over
// r = 0..31, so the ds_read_b64 fragment reads are conflict-free as they stand; the weight
// rows use a stride of 150 floats (2 x odd) for the same reason.
//
// scale_RGB: y = 255 x - mean, channel groups reversed.  The zero padding of conv2d_same
// happens AFTER scale_RGB, so pad taps must be 0 in the scaled domain: the scale is applied
// per element while staging (valid elements only), and the group reversal is a permutation
// of conv1's input channels that is folded into the weights at load time (locnet.hip).
//
// NW waves per workgroup: NW/2 along the pixels x 2 along the channels.
#include <cstdint>

#include "conv1_internal.h"

namespace dvsg {

int g_last_root_kernel[kRootKernelFields] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};

namespace {

// What launch_conv1 runs: a function of its arguments alone -- no HIP call, no global read or written.  `aligned` and
// `masked` are the bits of SRC beside the source kind, of `wt` only which images exist is looked at, `pool_offered` says
// that the caller would take the root max pool from the band kernel's epilogue (RootPool, cnn_kernels.h), and `opt` is
// where conv1_variant (Conv1Variant) and root_pool are read.  The caller has checked cin and that out_prec has its piece
// weights.
Conv1Choice choose_conv1(int out_prec, int cin, int src_kind, bool aligned, bool masked, const Conv1Weights &wt, int B, int Ho,
                         int Wo, bool pool_offered, const DebugOptions &opt) {
  const int SRC = conv1_src(src_kind, aligned, masked);
  const int wtiles = ceil_div(Wo, kConv1Tile);
  const int variant = opt.conv1_variant;
  const bool f16 = out_prec == kF16 && wt.f16 != nullptr;   // the float16 kernels need their weight image
  if (cin != kConv1Cin) {   // any other window length: one kernel for every precision, whatever conv1_variant says
    return {kConv1Rootconv, 4, out_prec == kF16 ? 1 : (out_prec == kF32S ? 2 : 0), SRC};
  }
  // the piece precisions have one kernel each, whatever the A/B switch says
  if (out_prec == kF32X) return {kConv1X3, -1, -1, SRC};
  if (out_prec == kF32S) return {kConv1Split, -1, 0, SRC};
  if (f16 && variant == kConv1VarF16OneRow && !masked)   // A/B: one output row per workgroup, never with a mask
    return {kConv1F16, -1, 1, SRC};
  if (f16 && variant != kConv1VarF32ToF16 && variant != kConv1VarNoMarch && !masked &&
      (variant == kConv1VarMarch || march_bands(B, Ho, wtiles, nullptr) > 0)) {   // (a masked window -- eval_train.py's
    // graph -- takes the two-row kernel below: same products in the same order)
    // big launches: marching, wave-specialised workgroups (conv1_f16_march_kernel), one per CU
    // (conv1_variant 5 forces it at any size, bands of <= 3 quads: the parity tests run it on small frames)
    int qpb = 0;
    int bands = march_bands(B, Ho, wtiles, &qpb);
    if (variant == kConv1VarMarch) {
      qpb = 3;
      bands = ((Ho + kConv1MarchQuad - 1) / kConv1MarchQuad + qpb - 1) / qpb;
    }
    return {kConv1F16March, -1, -1, SRC, bands, qpb};
  }
  if (f16 && variant != kConv1VarF32ToF16)   // two output rows per workgroup (conv1_f16_pair_kernel)
    return {kConv1F16Pair, -1, 1, SRC};
  if (out_prec == kF16) {   // conv1_variant 2: f32 multiply, f16 output (window tensors only)
    Conv1Choice c{kConv1OneRow, 4, 1, 0};
    c.window_only = true;
    return c;
  }
  if (!masked && (variant == kConv1VarBand || (variant == kConv1VarAuto && root_bands(B, Ho, wtiles, nullptr, nullptr) > 0))) {
    // big float32 launches: row pairs in bands, one workgroup per CU (root_band_kernel); a masked source takes the one-row
    // kernel below, like the float16 marching kernel's.  (conv1_variant 6 forces it at any size, bands of <= 3 pairs: the
    // parity tests run it on small frames; 7 never takes it)
    int ppb = 0, nbig = 0;
    int bands = root_bands(B, Ho, wtiles, &ppb, &nbig);
    if (variant == kConv1VarBand) {
      ppb = 3;
      bands = nbig = ((Ho + 1) / 2 + ppb - 1) / ppb;
    }
    Conv1Choice c{kConv1Band, 8, 0, SRC, bands, ppb, nbig};
    // the root max pool in the pairs' epilogues (root_band_pool_kernel), where the caller offers it and the pool pads
    // nothing on the top and the left (Ho and Wo even): root_pool 0 fuses where the band kernel is the library's own
    // choice, 2 wherever it runs, 1 never
    c.fuse_pool = pool_offered && Ho % 2 == 0 && Wo % 2 == 0 &&
                  (opt.root_pool == 2 || (opt.root_pool == 0 && variant == kConv1VarAuto));
    return c;
  }
  if (variant != kConv1VarAuto && variant != kConv1VarOneRow && src_kind == kSrcWindow && !masked)
    return {kConv1OneRow, 8, 0, 0};
  return {kConv1OneRow, 4, 0, SRC};
}

}  // namespace

int launch_conv1(int out_prec, const Conv1Src &src, int src_kind, const Conv1Weights &wt, void *y, int B, int H, int W, int Ho,
                 int Wo, int cin, hipStream_t s, RootPool *pool) {
  if (pool) pool->fused = false;
  DVSG_REQUIRE(cin % 3 == 0 && cin >= 3 && cin <= 3 * kRootMaxFrames, "conv1: %d input channels", cin);
  const int wtiles = ceil_div(Wo, kConv1Tile);
  const long blocks = (long)wtiles * Ho * B;
  DVSG_REQUIRE(blocks > 0 && blocks < (1L << 31), "conv1: grid of %ld workgroups out of range", blocks);
  DVSG_REQUIRE((long)W * cin < (1L << 31), "conv1: input row too long");
  DVSG_REQUIRE(src_kind == kSrcWindow || (src.table && src.n_pool > 0), "conv1: a frame ring needs its index table");
  const double in_bytes = src_kind == kSrcRingU8 ? 1.0 : 4.0;   // each window element once (ring frames are shared by windows:
  ProfScope prof(kClsConv1, s, 2.0 * (double)B * Ho * Wo * 64 * 49 * cin,   // an upper bound of the algorithmic read)
                 in_bytes * (double)B * H * W * cin + (double)elem_size(out_prec) * B * Ho * Wo * 64);
  // rows that start on 16-byte boundaries (4-byte for uint8 frames): the staged segment then consists of whole aligned groups
  const bool aligned = W % 4 == 0 && reinterpret_cast<uintptr_t>(src.base) % (src_kind == kSrcRingU8 ? 4 : 16) == 0;
  const int SRC = conv1_src(src_kind, aligned, src.mask != nullptr);
  if (cin != kConv1Cin) {   // rootconv_kernel reads the float32 image only
    DVSG_REQUIRE(wt.f32, "conv1: no float32 weight image");
  } else {
    // the f32s activations are float16 pieces (P format): only conv1_split_kernel writes them, whatever the A/B switch says
    // (the float32 kernel's output would be read back as pieces: silent garbage)
    if (out_prec == kF32S && !wt.pieces) return fail(DVSG_ERR_UNSUPPORTED, "conv1: the f32s precision needs the piece weights");
    if (out_prec == kF32X && !wt.x3) return fail(DVSG_ERR_UNSUPPORTED, "conv1: the f32x3 precision needs the bfloat16 piece weights");
  }

  const Conv1Choice c = choose_conv1(out_prec, cin, src_kind, aligned, src.mask != nullptr, wt, B, Ho, Wo, pool != nullptr, g_opt);
  if (c.window_only)
    DVSG_REQUIRE(src_kind == kSrcWindow && !src.mask, "conv1: conv1_variant 2 takes an unmasked window tensor");
  if (c.fuse_pool) {
    pool->fused = true;
    pool->bands = c.bands;
    pool->ppb = c.per_band;
    pool->nbig = c.nbig;
  }
  // c.src names one of the kernels' instantiations.  Unreachable from the ABI when not: every entry point passes one of
  // the three Conv1SrcKind values, or checks the kind it is given (dvsg_locnet_forward_masked)
  const Conv1Args a{src, wt, y, B, H, W, Ho, Wo, wtiles, s};
  bool legal = false;
  switch (c.family) {
    case kConv1OneRow:
    case kConv1Rootconv:
    case kConv1Band:
      legal = launch_conv1_f32(c, a, cin, c.fuse_pool ? pool->pooled : nullptr);
      break;
    case kConv1F16:
    case kConv1F16Pair:
    case kConv1F16March:
    case kConv1Split:
      legal = launch_conv1_f16_mfma(c, a);
      break;
    case kConv1X3:
      legal = launch_conv1_x3(c, a);
      break;
  }
  DVSG_REQUIRE(legal, "conv1: no kernel for source %d", SRC);
  record_conv1_kernel(c.family, c.nw, c.to, c.src, c.bands, c.per_band);
  return check_launch(c.family == kConv1Rootconv ? "rootconv_kernel" : "conv1_kernel");
}

}  // namespace dvsg
