// Between conv1.hip, which decides what the root conv runs, and the files that hold the kernels (conv1_f32.hip,
// conv1_f16.hip, conv1_x3.hip): the choice and one launch function per file.  Nothing here is locnet.hip's business;
// what it programs against is cnn_kernels.h.
#pragma once
#include "cnn_kernels.h"

namespace dvsg {
#pragma GCC visibility push(hidden)   // internal to the library: none of this is an exported name

// The conv1 family of the launch record (g_last_root_kernel[kRootConv1], cnn_kernels.h): the record's own numbers
enum Conv1Family {
  kConv1OneRow = 0,     // conv1_kernel
  kConv1F16 = 1,        // conv1_f16_kernel
  kConv1F16Pair = 2,    // conv1_f16_pair_kernel
  kConv1F16March = 3,   // conv1_f16_march_kernel
  kConv1Split = 4,      // conv1_split_kernel
  kConv1X3 = 5,         // conv1_x3_kernel
  kConv1Rootconv = 6,   // rootconv_kernel: cin != 21
  kConv1Band = 7        // root_band_kernel / root_band_pool_kernel
};

// What one launch_conv1 call runs (choose_conv1, conv1.hip).  nw, to, src, bands and per_band are the launch record's
// fields as record_conv1_kernel takes them; src also names the instantiation (conv1_kernel's 8-wave and float16-output
// forms exist for SRC 0 only, whatever the rows' alignment).
struct Conv1Choice {
  Conv1Family family;
  int nw, to, src;
  int bands = -1;      // marching and band kernels: bands per column tile and image
  int per_band = -1;   // quads (marching kernel) or row pairs (band kernel) of the longest band
  int nbig = 0;        // band kernel: the number of bands of that length
  bool fuse_pool = false;     // band kernel: root_band_pool_kernel, the max pool in the pairs' epilogues
  bool window_only = false;   // conv1_variant 2: the launch is an error unless the source is an unmasked window tensor
};

// The tensors and sizes of a launch_conv1 call, as the kernels take them
struct Conv1Args {
  const Conv1Src &src;
  const Conv1Weights &wt;
  void *y;
  int B, H, W, Ho, Wo, wtiles;
  hipStream_t s;
};

// One per kernel file: starts the kernel that `c` names (a family of that file).  False, and no launch, when c.src is not
// an instantiation of the family.  `pooled` is the pooled tensor of a fused launch (c.fuse_pool).
bool launch_conv1_f32(const Conv1Choice &c, const Conv1Args &a, int cin, void *pooled);   // families 0, 6 and 7
// conv1_f16.hip, the kernels on the float16 matrix cores: the float16 precision's three and f32s's conv1_split_kernel
bool launch_conv1_f16_mfma(const Conv1Choice &c, const Conv1Args &a);                     // families 1, 2, 3 and 4
bool launch_conv1_x3(const Conv1Choice &c, const Conv1Args &a);                           // family 5

// Output pixels of a row per workgroup, every conv1 kernel's tile (C1_TILE, conv1_device.h): launch_conv1 counts column tiles
constexpr int kConv1Tile = 128;
// The band policies (pure functions of the shape), next to their kernels
constexpr int kConv1MarchQuad = 4;   // output rows per quad of conv1_f16_march_kernel
int march_bands(int B, int Ho, int wtiles, int *quads_per_band);
int root_bands(int B, int Ho, int wtiles, int *pairs_per_band, int *nbig);

#pragma GCC visibility pop
}  // namespace dvsg
