// Shared host-side helpers for libdvsg_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../../include/dvsg_amd.h"

namespace dvsg {

// Thread-local last-error text returned by dvsg_last_error_string().
char *error_buffer();
int fail(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Check the launch itself (invalid configuration etc.); execution errors surface at the
// caller's next synchronisation, as for any stream-ordered API.
inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(DVSG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return DVSG_OK;
}

#define DVSG_REQUIRE(cond, ...)                                  \
  do {                                                           \
    if (!(cond)) return ::dvsg::fail(DVSG_ERR_INVALID_ARG, __VA_ARGS__); \
  } while (0)

#define DVSG_HIP(call)                                                                     \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return ::dvsg::fail(DVSG_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));    \
  } while (0)

// warp_kernels.hip internals shared with locnet.hip and views.cpp (coord_bstride in floats; 0 = broadcast)
int tps_solve_impl(const float *coord, long coord_bstride, const float *rhs, int rhs_is_vector, int B,
                   int P, float *T, int *n_singular, void *stream);
// constant control points (the evaluation graph's V_src): W^-1 once, then a matrix-vector product per frame
int tps_inverse_columns(const float *coord, int P, double *winv_cols, float *scratch, void *stream);
// A handle's warp shape (dvsg_locnet_view_create_shaped; include/dvsg_amd.h, "Warp shaping").  The default is every other
// handle's: unshaped.
struct RenderShape {
  int model = DVSG_SHAPE_AFFINE;
  float strength = 1.0f, rigidity = 0.0f;
  bool shaped() const { return !(strength == 1.0f && rigidity == 0.0f); }
};
// shape.shaped() (rhs = F_t, rhs_is_vector, P == 25 only): tps_shape_apply_kernel in tps_apply_kernel's place, T of F'
int tps_apply_impl(const double *winv_cols, const float *coord, const float *rhs, int rhs_is_vector, int B, int P,
                   float *T, void *stream, RenderShape shape = RenderShape());
int tps_warp_impl(const float *U, const float *coord, long coord_bstride, const float *T, int B, int H,
                  int W, int C, int P, int out_h, int out_w, float *out, float *x_s, float *y_s,
                  void *stream, const float *zoom = nullptr /* [B] device: the zoomed grid of tps_warp_zoom_kernel */);

int tps_warp_ring_impl(const void *pool, int pool_is_u8, int n_pool, const int *table, int tstride, const float *coord,
                       long coord_bstride, const float *T, int B, int H, int W, int P, float *out, float *x_s, float *y_s,
                       void *stream, const int *out_index = nullptr);

// What a handle tells the source-size renders: a plain handle's values by default, a view's own otherwise (views.cpp makes
// them; include/dvsg_amd.h says what each one means).  filter and border are read by the four renders, shape by them, by
// dvsg_tps_coefficients_f32 and by dvsg_tps_coverage_net_f32.
struct RenderView {
  int filter = DVSG_RENDER_BILINEAR;
  int border = DVSG_BORDER_BLACK;
  RenderShape shape;
  int surface_format = DVSG_SURFACE_NV12;   // read by dvsg_tps_render_nv12 / _zoom_nv12 alone
  int chroma_format = DVSG_CHROMA_420;      // likewise: the chroma plane is (H, W / 2) for DVSG_CHROMA_422 ("Chroma sampling")
  int out_h = 0, out_w = 0;                 // read by the four renders alone; (0, 0): the source's size
};
// dvsg_tps_render_u8 and, with zoom [B] on the device, dvsg_tps_render_zoom_u8 (winv_cols / coord: the handle's W^-1 columns
// and V_src)
int tps_render_impl(const double *winv_cols, const float *coord, const float *F_t, const float *zoom, const uint8_t *src, int B,
                    int H, int W, int P, int channel_flip, float *T, float *out_f32, uint8_t *out_u8, int u8_W, int u8_x0,
                    void *stream, const RenderView &view);
// nv12.hip: dvsg_tps_render_nv12 and, with zoom [n] on the device, dvsg_tps_render_zoom_nv12.  The check makes no HIP call
// and reads no handle (fn: the entry point its messages name; out_H, out_W: a scaled view's output size, (0, 0) for the
// source's); the launch half assumes it passed.  tps_render_p010_check: what a P010 view (dvsg_locnet_view_create_surface)
// asks on top of it, once the handle may be read -- planes of 16-bit words, pitch >= 2 W, pitches, frame strides and plane
// pointers 2-byte aligned (out_W: a scaled view's output width, 0 for W); no HIP call either.
int tps_render_nv12_check(const char *fn, const float *F_t, const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride,
                          int n, int H, int W, const float *T, const uint8_t *out_y, const uint8_t *out_uv, size_t out_pitch,
                          size_t out_frame_stride, int out_H, int out_W);
int tps_render_p010_check(const char *fn, const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int W,
                          const uint8_t *out_y, const uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, int out_W);
int tps_render_nv12_impl(const char *fn, const double *winv_cols, const float *coord, const float *F_t, const float *zoom,
                         const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int H, int W, int P, float *T,
                         uint8_t *out_y, uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, void *stream,
                         const RenderView &view);
// nv12.hip: what a scaled view (dvsg_locnet_view_create_scaled) asks of a render of (H, W) frames at another size
// (out_H, out_W): at most 4 virtual samples per axis, no DVSG_BORDER_KEEP.  No HIP call.
int render_scaled_check(const char *fn, int H, int W, int out_H, int out_W, int render_border);
// crop_kernels.hip: the fused coverage scan of dvsg_tps_coverage_f32 (coord_bstride in floats; 0 = broadcast)
int tps_coverage_impl(const char *fn, const float *coord, long coord_bstride, const float *T, const float *zoom, int B, int P,
                      int src_H, int src_W, int out_h, int out_w, int32_t *n_border, int32_t *key_min, void *workspace,
                      size_t workspace_bytes, void *stream);

// The values of the debug option conv1_variant (DebugOptions below; read by choose_conv1, conv1.hip)
enum Conv1Variant {
  kConv1VarAuto = 0,
  kConv1VarEightWaves = 1,   // float32 kernel with 8 waves
  kConv1VarF32ToF16 = 2,     // float16 output from the float32 multiply
  kConv1VarF16OneRow = 3,    // float16, one output row per workgroup
  kConv1VarNoMarch = 4,      // float16: never the marching kernel
  kConv1VarMarch = 5,        // float16: always the marching kernel
  kConv1VarBand = 6,         // float32: always the band kernel (unmasked sources)
  kConv1VarOneRow = 7        // float32: always the one-row kernel
};

// The diagnostic A/B switches of dvsg_debug_set_option, one member per option name, at their defaults.  One instance,
// g_opt (api_common.cpp); the launch policies read its members.  Host-only, not synchronised: tests and tools set a
// switch between calls, never during one.
struct DebugOptions {
  int conv_variant = 0;        // 0 = auto, 1 = 4 waves, 2 = 8 waves, 3 = no split-K, 4 = 64-wide tiles only,
                               // 5 = no 256 x 128 float16 tiles, 6 = no stream-K tail (conv_gemm.hip)
  int conv1_variant = 0;       // 0 = auto; 1 = float32 kernel with 8 waves; 2 = float16 output from the float32 multiply;
                               // 3 = float16, one output row per workgroup; 4 = never the marching kernel; 5 = always;
                               // float32: 6 = always the band kernel (unmasked sources), 7 = always the one-row kernel
  int root_pool = 0;           // float32 root max pool in the band kernel's epilogue (root_band_pool_kernel + seam kernel): 0 = where
                               // the band kernel is the library's own choice, 1 = never, 2 = wherever the band kernel runs
  int wide16_min_tiles = 128;  // float16 mode: 256 x 128 tiles from this many of them (a quarter of a round of 512 workgroups).
                               // Round 2 measured 256 (128 and below lost at batch 1-2 with the kernels of then); with packed
                               // weight stages, 128-byte activation rows and the 3x3 row reuse 128 is -0.5 % at batch 16, -4.5 %
                               // at batch 4 (720p), equal at batch 1; 64 and 32 lose 4-27 % at batch 1-4
  int wide16_packed = 1;       // 0: weight stages fetched from the [rows][K] layout
  int wide16_arows = 1;        // 0 = 64-byte activation rows everywhere (conv_wide16_kernel), 2 = 128-byte rows for K = 128
                               // too (tests)
  int wide16_hreuse = 1;       // 0: 3x3 stride-1 layers through conv_wide16a_kernel
  int fused_hreuse = 1;        // 0: block 1's stride-1 units through conv3x3_1x1_f16_kernel
  int fuse_conv = 1;           // 0 turns the fused block-1 path off
  int fuse_shortcut = 1;       // block 1's shortcut conv inside the fused conv2 + conv3 kernel (0: A/B)
  int concat_sc = 1;           // blocks 2-4's opening units: shortcut + conv1 as one launch (0: A/B)
  int x3_conv1 = 1;            // 0: the f32x3 precision with the float32 conv1 kernel (A/B)
  int x3_fuse = 3;             // A/B of block 1's fusion in the f32x3 precision (forward())
  int f16_split = 1;           // float16 precision: conv weights as hi / lo float16 pairs (default) or plain float16 (A/B only:
                               // 0; 9/10 of the plain mode's F_t error is the weights' rounding)
  // Which layers of the float16 mode carry the lo piece: bit 4 * kind + block (kind 0 = a unit's conv1, 1 = conv2, 2 = conv3,
  // 3 = shortcut; block 0..3).  A plain float16 weight is off by up to 2^-12 relative at every pixel alike, an error the global
  // average pool does not average away; how much of it reaches F_t depends on the layer (tools/f16_pair_sweep.py measures
  // every block x kind).  A layer without the lo piece runs half the MFMAs and, in the big launches, 128 channels per tile.
  int f16_pair_mask = 0xFFFF;
  int flow_tiled = 1;          // 0 = tf_warp by global gathers (stn_kernel<kFlow>), 1 = column strips streamed through LDS,
                               // workgroups in XCD-aware order (default), 2 = the same in plain dispatch order
  int flow_rounds = 4;         // rounds of resident workgroups the strip kernel's bands aim at
  int warp_xcd = 0;            // XCD-aware workgroup order of the sampler kernels; 0: plain dispatch order (A/B)
};
extern DebugOptions g_opt;

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// np.uint8(x * 255.) of eval.py:112: the product is float64 and the cast truncates toward zero.
// (NumPy leaves out-of-range casts undefined; here they saturate to 0 / 255, NaN gives 0.)
// Shared by the frame egress (frames.hip) and the uint8 form of the TPS warp (warp_kernels.hip).
__device__ __forceinline__ uint8_t to_u8(double x) {
  const double d = x * 255.0;
  return d >= 255.0 ? (uint8_t)255 : (d > 0.0 ? (uint8_t)(int)d : (uint8_t)0);
}

}  // namespace dvsg

// ---- optional roctx ranges (tracing) ------------------------------------------------
// With DVSG_ROCTX=1 in the environment every stage of the evaluation graph (conv1, pool1, each bottleneck unit, head,
// tps_solve, tps_warp) opens a roctx range around its launches, so `rocprofv3 --kernel-trace --marker-trace` attributes
// the kernels of a step to stages and units instead of to kernel names only.  The roctx library is looked up with dlopen
// at the first range (no link-time dependency); without the variable a range is one relaxed load.
namespace dvsg {
struct MarkerRange {
  explicit MarkerRange(const char *name);
  ~MarkerRange();
  MarkerRange(const MarkerRange &) = delete;
  MarkerRange &operator=(const MarkerRange &) = delete;
  bool open_;
};
}  // namespace dvsg

// ---- optional per-kernel-class timing (bench.py roofline leg; see dvsg_prof_begin) ----------
namespace dvsg {
enum KernelClass {
  kClsConv1 = 0,   // conv1_kernel (7x7/2 + scale_RGB)
  kClsConv3x3 = 1, // conv_gemm_kernel<*,3,..>
  kClsConv1x1 = 2, // conv_gemm_kernel<*,1,..>
  kClsMaxpool = 3,
  kClsHead = 4,    // avgpool + dense
  kClsTpsSolve = 5,
  kClsTpsWarp = 6,
  kClsStn = 7,     // flow / sampler B / affine / projective / elastic
  kClsFused = 8,   // conv3x3_1x1_kernel (block 1's conv2 + conv3)
  kNumCls = 9
};
// RAII: when profiling is armed for `cls`, brackets the launches issued in its lifetime with a
// hipEvent pair on `s` and books their algorithmic FLOPs / bytes.  Otherwise a no-op.
struct ProfScope {
  ProfScope(int cls, hipStream_t s, double flops, double bytes);
  ~ProfScope();
  int idx_;
  hipStream_t s_;
  hipEvent_t stop_ = nullptr;
};
}  // namespace dvsg
