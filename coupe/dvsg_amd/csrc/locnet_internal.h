// The network handle (dvsg_locnet_t) and the host structs it is made of, shared by locnet.hip (which fills the handle and runs
// the network) and views.cpp (the views of a handle and the entry points that read a handle's render properties).
#pragma once
#include <atomic>
#include <vector>

#include "cnn_kernels.h"

namespace dvsg {

struct ConvLayer {
  int ksize, cin, cout, stride;
  bool relu;
  float *wt = nullptr;        // device, [cout][k*k*cin] float32 (conv1: [7][64][kConv1Ld])
  _Float16 *wt16 = nullptr;   // device, same layout in float16 (not for conv1)
  _Float16 *wt16s = nullptr;  // device, float16 hi / lo pairs [cout/64][128][k*k*cin] (conv_gemm.hip SPLIT; not for conv1)
  _Float16 *wt16p = nullptr;  // device, wt16s packed stage by stage for conv_gemm_wide16.hip (cin % 64 == 0 layers)
  _Float16 *wt16pa = nullptr; // device, the same in the order of its 128-byte-activation-row kernel
  _Float16 *wt16ph = nullptr; // device, the same in the order of its 3x3 stride-1 kernel (3x3 layers only)
  _Float16 *wt16q = nullptr, *wt16qa = nullptr, *wt16qh = nullptr;   // device, the PLAIN copy wt16 packed the same three ways
                              // (cin % 64 == 0, cout % 128 == 0 layers: what runs when a layer has no lo piece)
  _Float16 *wt32s = nullptr;  // device, "f32s" pieces [cout][k*k*cin/32][32 hi | 32 lo] (conv_gemm.hip SPLIT, T = float; not for conv1)
  unsigned short *wt3x = nullptr;  // device, "f32x3" bfloat16 pieces, packed stage by stage (launch_pack_x3; not for conv1)
  float *bias = nullptr;      // device, [cout] float32
  // the weight image a math multiplies by: the one place that pairs the two up
  ConvWeights image(ConvMath math) const {
    switch (math) {
      case kMathF32S: return {wt32s};
      case kMathF32X: return {wt3x};
      case kMathF16Pairs: return {wt16s, wt16p, wt16pa, wt16ph};
      case kMathF16Plain: return {wt16, wt16q, wt16qa, wt16qh};
      default: return {wt};
    }
  }
  Conv1Weights conv1_images() const { return {wt, wt16, wt32s, wt3x, bias}; }   // (conv1 keeps its images in the same members)
};

struct Unit {
  int block;   // 0..3
  int base, depth, stride;
  bool has_shortcut;
  ConvLayer shortcut, c1, c2, c3;
  // units that open blocks 2-4: `shortcut` and `conv1` read the same input -- their weight rows concatenated along N
  // ([shortcut | conv1], float32 and f32s pieces) run as ONE launch (forward(), "concat_sc")
  ConvLayer cat;
  bool has_cat = false;
};

}  // namespace dvsg

struct dvsg_locnet {
  int c_in = 0;
  dvsg::ConvLayer conv1;
  std::vector<dvsg::Unit> units;
  float *dense_w[4] = {nullptr, nullptr, nullptr, nullptr};
  float *dense_b[4] = {nullptr, nullptr, nullptr, nullptr};
  float *v_src = nullptr;  // [25,2] model.py:105-110
  double *winv = nullptr;  // [25][28]: columns of the TPS system's inverse for v_src (see tps_apply_kernel)
  // float16 mode: which layers multiply by hi / lo weight PAIRS (bit 4 * kind + block, see DebugOptions::f16_pair_mask).  All of them
  // until dvsg_locnet_calibrate_f16 has re-rounded the plain copies of blocks 2-4 with error feedback: then block 1 only.
  int f16_pair_mask = 0xFFFF;
  // what the last calibrate_f16 of this handle re-rounded against (dvsg_debug_calibration_means): the channel means mu
  // [48][2048] that redo() read and the rows summed per slot; 1.0 and 0 rows where no means were measured (a new handle,
  // mode 0, mode 1)
  std::vector<double> calib_mu = std::vector<double>((size_t)48 * 2048, 1.0);
  double calib_rows[48] = {0};
  std::vector<void *> allocs;
  // A VIEW (views.cpp) is one of these with nothing in it but `parent` and its own `view`: every entry point reads the network
  // and the TPS constants through base() at call time, so a later calibration of the parent is seen through its views.
  // n_views: the live views of a parent, which dvsg_locnet_destroy refuses to pull the network from under.
  const dvsg_locnet *parent = nullptr;
  dvsg::RenderView view;   // what the handle tells the renders (common.h); a plain handle's is the default
  mutable std::atomic<int> n_views{0};
};

// the handle that owns the network `net` shows: itself, or a view's parent
static inline const dvsg_locnet *base(const dvsg_locnet *net) { return net && net->parent ? net->parent : net; }
