/*
 * dvsg_amd.h -- C ABI of libdvsg_amd.so: the MI355X (gfx950) implementation of the
 * coupe.DVSG per-frame inference hot path.
 *
 * The reference has no FFI / plugin interface: its boundary is a set of Python callables
 * taking TF tensors.  Each entry point below replaces the TF
 * sub-graph built by the reference function it cites; the Python facade
 * (the coupe.dvsg_amd Python package) keeps the reference's names / argument order / return tuples and
 * forwards to these.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (DVSG_OK) or a negative dvsg_status; it never throws or
 *     aborts across the ABI.  dvsg_last_error_string() describes the calling thread's last
 *     failure.
 *   - every tensor argument is a CALLER-OWNED DEVICE pointer to dense float32 data in the
 *     reference's layout (NHWC images, values as the reference feeds them) unless a
 *     parameter is documented as "host".
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All
 *     calls are asynchronous and stream-ordered; none allocates, frees or synchronises.
 *     Calls on distinct streams are re-entrant as long as their output / workspace buffers
 *     are distinct.  tests/test_gpu_streams.py holds every entry point with a `stream` to this:
 *     captured into a HIP graph and replayed on fresh values, and in pairs on two streams of one
 *     handle.  The four source-size renders are held to it through every view constructor below (filter, border,
 *     shape, surface format, output size, chroma format), and while another thread makes and destroys views.
 *     The exceptions say "synchronous" in their own comment (the float16 calibration:
 *     it waits for `stream`, in every mode, before it rewrites the handle's weights).  Found
 *     with that module and fixed: dvsg_scene_step_f32 zeroed its histograms with a memset node,
 *     which did not take effect on the second and later replays of a captured step (it is a
 *     kernel now); the undo form of dvsg_locnet_calibrate_f16 and modes 0 / 1 of
 *     dvsg_debug_calibrate_f16_weights did not wait for `stream`, so a float16 forward still
 *     queued there ran on the rewritten weights; and the Python facade's LocNet.workspace kept
 *     one buffer for all streams, breaking the distinct-workspace condition on its callers'
 *     behalf (it is keyed by stream now).
 *   - optional outputs may be NULL.
 */
#ifndef DVSG_AMD_H
#define DVSG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVSG_ABI_VERSION 1

typedef enum dvsg_status {
  DVSG_OK = 0,
  DVSG_ERR_INVALID_ARG = -1, /* NULL pointer, non-positive size, unsupported shape        */
  DVSG_ERR_HIP = -2,         /* a HIP runtime call failed; see dvsg_last_error_string()    */
  DVSG_ERR_WORKSPACE = -3,   /* workspace too small or misaligned                          */
  DVSG_ERR_WEIGHTS = -4,     /* checkpoint array missing / wrong shape                     */
  DVSG_ERR_UNSUPPORTED = -5  /* valid request this build does not implement                */
} dvsg_status;

int dvsg_abi_version(void);
const char *dvsg_last_error_string(void);
/* "gfx950" -- the only code object in the library. */
const char *dvsg_target_arch(void);

/* ---------------------------------------------------------------------------------------
 * Thin-plate-spline transformer: ThinPlateSpline.py:4-170, ThinPlateSpline2.py:4-170.
 * ------------------------------------------------------------------------------------- */

/* `_solve_system` (ThinPlateSpline.py:143-166).  coord [B,P,2]; rhs [B,P,2] is `vector`
 * when rhs_is_vector != 0 (T solves for coord+vector, ThinPlateSpline.py:161) or `target`
 * (ThinPlateSpline2.py:160).  T [B,2,P+3].  3 <= P <= 61.  The 28x28 system is assembled in
 * float32 exactly as the reference does and solved in float64 (partial pivoting), which
 * lands inside the reference's own float32 LU noise. */
int dvsg_tps_solve_f32(const float *coord, const float *rhs, int rhs_is_vector, int B, int P,
                       float *T, void *stream);

/* As above, for callers that want tf.matrix_inverse's error behaviour (ThinPlateSpline.py:159
 * raises InvalidArgument "Input is not invertible" on repeated / collinear control points): the
 * number of samples whose system has a pivot below 1e-13 x max|W| is ADDED to the device int
 * *n_singular (zero it first; read it after the stream has run).  Either way such a sample's T is
 * NaN, never a finite garbage map. */
int dvsg_tps_solve_checked_f32(const float *coord, const float *rhs, int rhs_is_vector, int B, int P,
                               float *T, int *n_singular, void *stream);

/* `_transform` + `_meshgrid` + `_interpolate` fused (ThinPlateSpline.py:30-141): for every
 * output pixel evaluate [1, x_t, y_t, r_0..r_{P-1}], (x_s, y_s) = T . basis, then sampler A
 * (coords scaled by W/2, indices clipped BEFORE the weights).  U [B,H,W,C]; coord [B,P,2];
 * T [B,2,P+3]; out [B,out_h,out_w,C]; x_s, y_s [B*out_h*out_w] (optional).  The [B,P+3,H*W]
 * basis the reference materialises never exists.  U == NULL && out == NULL: grid only. */
int dvsg_tps_warp_f32(const float *U, const float *coord, const float *T, int B, int H, int W,
                      int C, int P, int out_h, int out_w, float *out, float *x_s, float *y_s,
                      void *stream);

/* ---------------------------------------------------------------------------------------
 * Optical-flow warp: warp_with_optical_flow.py:96-176 `tf_warp` (sampler C).
 * im [B,H,W,C], flow [B,H,W,2] in pixels (dx, dy), out [B,H,W,C].
 * ------------------------------------------------------------------------------------- */
int dvsg_flow_warp_f32(const float *im, const float *flow, int B, int H, int W, int C,
                       float *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Spatial transformers: spatial_transformer.py.
 * ------------------------------------------------------------------------------------- */

/* `bilinear_interp` (spatial_transformer.py:496-563, sampler B) from explicit normalised
 * coordinates x_s, y_s [B*out_h*out_w]. */
int dvsg_stn_sample_f32(const float *im, const float *x_s, const float *y_s, int B, int H,
                        int W, int C, int out_h, int out_w, float *out, void *stream);

/* AffineTransformer._transform (spatial_transformer.py:74-91), theta [B,6]; when im and out
 * are non-NULL the sampler B gather is fused.  x_s / y_s optional. */
int dvsg_grid_affine_f32(const float *theta, const float *im, int B, int H, int W, int C,
                         int out_h, int out_w, float *out, float *x_s, float *y_s, void *stream);

/* ProjectiveTransformer._transform (spatial_transformer.py:423-452), theta [B,8] (the 9th
 * entry is 1), tf.div_no_nan by z. */
int dvsg_grid_projective_f32(const float *theta, const float *im, int B, int H, int W, int C,
                             int out_h, int out_w, float *out, float *x_s, float *y_s,
                             void *stream);

/* ElasticTransformer constants (spatial_transformer.py:313-362): HOST outputs
 * source_points [2,n] and L_inv [n,n+3] (= transpose(inverse(L)[:,3:])) for an
 * grid_size x grid_size control grid, n = grid_size^2 <= 61. */
int dvsg_elastic_constants_f32(int grid_size, float *source_points_host, float *L_inv_host);

/* ElasticTransformer._transform (spatial_transformer.py:276-296): theta_abs [B,2,n] are the
 * absolute control point positions (source_points + theta), L_inv [n,n+3] and
 * source_points [2,n] are DEVICE copies of the constants above.  The
 * [n+3, H*W] `right_mat` is evaluated on the fly, basis order [x; y; 1; U_0..U_{n-1}]. */
int dvsg_grid_elastic_f32(const float *theta_abs, const float *L_inv, const float *source_points,
                          int n, const float *im, int B, int H, int W, int C, int out_h,
                          int out_w, float *out, float *x_s, float *y_s, void *stream);

/* `scale_RGB` (networks.py:6-16): y = 255 x - mean with the three channel GROUPS reversed.
 * C must be a multiple of 3. */
int dvsg_scale_rgb_f32(const float *rgb, int B, int H, int W, int C, float *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * localizationNet: networks.py:30-46 (slim resnet_v1_50 + 4 dense layers).
 * ------------------------------------------------------------------------------------- */
typedef struct dvsg_locnet dvsg_locnet_t;

/* Build the immutable device-side network from HOST arrays named like the reference's
 * checkpoint (ckpt_manager.py:42; `stabNet/localizationNet/...`, with or without `:0`).
 * dims is [n_arrays][4] (unused trailing entries ignored), ndims[i] in 1..4.  Unknown names
 * are ignored; a missing or mis-shaped array is DVSG_ERR_WEIGHTS (the reference silently
 * runs on random weights instead, ckpt_manager.py:21-22).  BatchNorm (eps 1e-5, moving
 * statistics) is folded into per-channel scale/shift here.  Allocates device memory.
 * The window length is the checkpoint's: conv1/weights [7,7,c_in,64] with c_in = 3 S loads for 1 <= S <= 16 (the
 * reference's `sample_num`, config.py:47); any other c_in is DVSG_ERR_UNSUPPORTED, decided before any device work.
 * S = 7 runs the conv1 kernels tuned for it; any other S runs one root-conv kernel that takes c_in as an argument
 * (exact float32 products, the output converted to the precision's format: see the precision paragraphs below). */
int dvsg_locnet_create(int n_arrays, const char *const *names, const float *const *host_data,
                       const int *ndims, const int64_t *dims, dvsg_locnet_t **net);
int dvsg_locnet_destroy(dvsg_locnet_t *net);
/* input channels of the loaded conv1: 3 S for a window of S frames (21 for the 7-frame window) */
int dvsg_locnet_in_channels(const dvsg_locnet_t *net);
/* bytes of scratch `forward` needs for a [B,H,W,c_in] batch (256-byte aligned). */
int dvsg_locnet_workspace_bytes(const dvsg_locnet_t *net, int B, int H, int W, size_t *bytes);

/* Views and the render filter.  The filter of the four source-size renders (dvsg_tps_render_u8, dvsg_tps_render_zoom_u8,
 * dvsg_tps_render_nv12, dvsg_tps_render_zoom_nv12) is a property of the immutable handle they are given, not an argument
 * and not a setter: one network shared by several stabilisers, threads, streams and captured graphs renders with the
 * filter of the handle each call passes.  Both functions are host-side: no stream, no device work.
 *   dvsg_locnet_view_create  a VIEW of `net`: the same network and TPS constants, nothing copied, with its own render
 *          filter (DVSG_RENDER_BILINEAR or DVSG_RENDER_BICUBIC).  Every entry point that takes a dvsg_locnet_t accepts a
 *          view, and everything but the four renders -- and, for a SHAPED view ("Warp shaping" below), the two other
 *          entry points that turn F_t into T through a handle, dvsg_tps_coverage_net_f32 and dvsg_tps_coefficients_f32 --
 *          behaves exactly as on the parent, bit for bit.  A view resolves to
 *          its parent at call time (it copies no pointers), so a later dvsg_locnet_calibrate_f16 of the parent is seen
 *          through its views; calibrating THROUGH a view is DVSG_ERR_INVALID_ARG.  A view of a view is a view of the
 *          parent.  dvsg_locnet_destroy(view) frees the view only; destroying a parent that still has views is
 *          DVSG_ERR_INVALID_ARG and destroys nothing.  An unknown filter or a NULL pointer is DVSG_ERR_INVALID_ARG,
 *          decided before anything is allocated.
 *   dvsg_locnet_render_filter  the handle's filter: 0 for every handle of dvsg_locnet_create (and for NULL).
 *
 * DVSG_RENDER_BILINEAR: sampler A, what the renders' own paragraphs below describe.
 * DVSG_RENDER_BICUBIC: what a render launch does after T is written changes; T and the TPS map do not.  For every sample
 * of a plane -- ph x pw samples of C components: the RGB image (C = 3), NV12 luma (C = 1), NV12 chroma (C = 2, ph = H / 2,
 * pw = W / 2) -- x_s, y_s are the bits the grid-only form of dvsg_tps_warp_zoom_f32 (U == NULL, out == NULL, coord =
 * V_src, the same T and zoom, out = the plane's size) gives.  Every float32 operation below is rounded on its own.
 *   1. x = ((x_s + 1) * (float)pw) / 2, y = ((y_s + 1) * (float)ph) / 2: sampler A's coordinates.
 *   2. The sample is valid iff sampler A blends four distinct taps there: 0 <= x < pw - 1, 0 <= y < ph - 1, not NaN.  An
 *      invalid sample is exactly 0.0f (byte 0 for RGB and luma, 128 for chroma, 0.0f in out_f32): the set of valid
 *      samples is the bilinear render's, so dvsg_tps_coverage_* and the crop need no change.  A plane with pw == 1 or
 *      ph == 1 has no valid sample and is rendered all invalid.
 *   3. x0 = (int)floorf(x), t = x - (float)x0 (exact).  With A = -0.75 (OpenCV's published INTER_CUBIC kernel; parity
 *      with cv2 unpinned): u = t + 1, w0 = ((A u - 5A) u + 8A) u - 4A; w1 = ((1.25f t - 2.25f) t) t + 1; v = 1 - t,
 *      w2 = ((1.25f v - 2.25f) v) v + 1; w3 = ((1 - w0) - w1) - w2.  The same for y with y0.
 *   4. Taps: columns x0 - 1 .. x0 + 2, rows y0 - 1 .. y0 + 2, each index clamped into the plane (edge replicate); a
 *      sample's value is what the bilinear path blends: (float)b / 255.0f, chroma (float)((int)b - 128) / 255.0f.
 *   5. Rows first: h_r = ((w0 p0 + w1 p1) + w2 p2) + w3 p3, then v = ((wy0 h0 + wy1 h1) + wy2 h2) + wy3 h3.
 *   6. The overshoot of a cubic is not clamped in float32 (out_f32).  Bytes round to NEAREST -- the weights sum to 1
 *      only up to rounding, and truncation would make flat areas flicker between k - 1 and k --:
 *      clamp(floor((double)v * 255.0 + 0.5), 0, 255), chroma clamp(floor((double)v * 255.0 + 128.5), 0, 255); NaN gives 0.
 *      channel_flip, u8_W / u8_x0, pitch / frame_stride and the NULL-output rules are the bilinear render's.
 * No load of the bicubic kernels touches a byte outside the pw * C used bytes of the source row it reads (not the pitch
 * padding, not the next frame). */
#define DVSG_RENDER_BILINEAR 0
#define DVSG_RENDER_BICUBIC 1
int dvsg_locnet_view_create(const dvsg_locnet_t *net, int render_filter, dvsg_locnet_t **view);
int dvsg_locnet_render_filter(const dvsg_locnet_t *net);

/* Border modes.  What the four source-size renders make of an INVALID sample (step 2 above) is, like the filter, a
 * property of the handle they are given: a view carries a filter AND a border.  Both functions are host-side: no stream,
 * no device work, everything decided before anything is allocated.
 *   dvsg_locnet_view_create_border  dvsg_locnet_view_create with a border mode; dvsg_locnet_view_create(net, f, &v) is
 *          dvsg_locnet_view_create_border(net, f, DVSG_BORDER_BLACK, &v).  The view rules are the ones above: a view of a
 *          view is a view of the parent with the filter and border of ITS arguments (nothing inherited), calibrating
 *          through a view and destroying a parent with live views are refused.  An unknown border is
 *          DVSG_ERR_INVALID_ARG ("render_border=<n>").
 *   dvsg_locnet_render_border  the handle's border: 0 for every handle of dvsg_locnet_create, for NULL, and for the
 *          views of dvsg_locnet_view_create.
 * A border mode decides what an invalid sample becomes and nothing else: the set of valid samples, T, the TPS map, the
 * coverage scan (dvsg_tps_coverage_*) and the crop's zoom are the same bits for every mode.  The rule is applied per
 * plane of ph x pw samples (RGB, NV12 luma, NV12 chroma); x, y and validity are steps 1-2 of the bicubic paragraph, i.e.
 * sampler A's coordinates, for both filters.  Every float32 operation is rounded on its own.
 *   Valid samples.  The bits of DVSG_BORDER_BLACK, for every mode and filter.
 *   Black (DVSG_BORDER_BLACK).  The renders as their own paragraphs and the filter's describe them: an invalid sample is
 *      byte 0 (RGB, luma) / 128 (chroma).  The launches of a handle with border 0 are the kernels without a border.
 *   Keep (DVSG_BORDER_KEEP).  An invalid sample, NaN included, is NOT WRITTEN: out_u8 / out_f32, out_y / out_uv keep what
 *      the caller left there.  Each plane decides on its own validity (a luma sample may be written where the chroma
 *      sample over it is not).  Row bytes beyond W and columns outside [u8_x0, u8_x0 + W) remain unwritten, as always.
 *   Replicate (DVSG_BORDER_REPLICATE) and mirror (DVSG_BORDER_MIRROR).  A NaN coordinate (x or y) gives the black value
 *      (0.0f; byte 0 / 128).  Otherwise, with m = (float)(pw - 1): xr = x (replicate), or
 *      xr = x < 0 ? -x : (x > m ? (m + m) - x : x) (mirror: ONE reflection); xc = fminf(fmaxf(xr, 0), m); the same for y
 *      with ph.  The sample is the handle's filter evaluated at (xc, yc):
 *        bilinear  x0 = (int)floorf(xc); taps x0 and min(x0 + 1, pw - 1); weights (x0f + 1) - xc and xc - x0f -- the upper
 *                  weight from the UNclipped index (sampler A's clipped weights would cancel on the edge) --; the same
 *                  for y; wa = wx0 wy0 on (x0, y0), wb = wx0 wy1 on (x0, y1), wc = wx1 wy0 on (x1, y0), wd = wx1 wy1 on
 *                  (x1, y1); v = ((wa a + wb b) + wc c) + wd d, sampler A's blend; bytes truncate as in the bilinear
 *                  render (chroma rounds at 128.5 as it does there).  On a valid sample this IS sampler A, bit for bit.
 *        bicubic   steps 3-6 of the bicubic paragraph at (xc, yc): its taps are edge-replicated already, its bytes round
 *                  to nearest.
 *      A plane with pw == 1 or ph == 1 is filled from its single column or row.  No load touches a byte outside the
 *      pw * C used bytes of the source row it reads. */
#define DVSG_BORDER_BLACK 0
#define DVSG_BORDER_REPLICATE 1
#define DVSG_BORDER_MIRROR 2
#define DVSG_BORDER_KEEP 3
int dvsg_locnet_view_create_border(const dvsg_locnet_t *net, int render_filter, int render_border, dvsg_locnet_t **view);
int dvsg_locnet_render_border(const dvsg_locnet_t *net);

/* Warp shaping: strength and rigidity.  How much of the network's F_t a render applies is, like the filter and the border,
 * a property of the handle: a view carries a filter, a border AND a shape (model, strength, rigidity).  Both functions are
 * host-side: no stream, no device work, everything decided before anything is allocated.
 *   dvsg_locnet_view_create_shaped  dvsg_locnet_view_create_border with a shape.  shape_model is DVSG_SHAPE_AFFINE,
 *          _SIMILARITY or _TRANSLATION; strength and rigidity lie in [0, 1] (NaN is refused).  An unknown model, filter or
 *          border, a value outside [0, 1] or a NULL pointer is DVSG_ERR_INVALID_ARG; the message names the argument and its
 *          value ("shape_model=<n>", "strength=<x>", "rigidity=<x>").  The view rules are the ones above: a view of a view is
 *          a view of the parent with the filter, border and shape of ITS arguments (nothing inherited), calibrating through
 *          a view and destroying a parent with live views are refused.
 *   dvsg_locnet_render_shape  the handle's shape into the three pointers (each may be NULL); always DVSG_OK.  It is
 *          (DVSG_SHAPE_AFFINE, 1.0f, 0.0f) for NULL, for every handle of dvsg_locnet_create and for every view of
 *          dvsg_locnet_view_create and dvsg_locnet_view_create_border.
 * A view with strength == 1.0f && rigidity == 0.0f is UNSHAPED whatever its model: its launches and its bits are exactly
 * those of dvsg_locnet_view_create_border(net, render_filter, render_border).
 *
 * The rule, per frame.  d_i = F_t[i] (float32, i = 0..24), p_i = V_src[i], the constant 5 x 5 grid with coordinates 0,
 * +-0.5 and +-1: sum p = 0, sum px py = 0, sum px^2 = sum py^2 = 12.5, sum |p|^2 = 25.  Everything is float64, every
 * operation rounded on its own (no contraction), every sum runs sequentially over i = 0..24 from 0.0.
 *   Means.        mx = (sum dx_i) / 25.0, my = (sum dy_i) / 25.0.
 *   Translation.  L_i = (mx, my).
 *   Similarity.   a = (sum (px_i dx_i + py_i dy_i)) / 25.0, b = (sum (px_i dy_i - py_i dx_i)) / 25.0;
 *                 L_ix = (mx + a px_i) - b py_i, L_iy = (my + b px_i) + a py_i.
 *   Affine.       axx = (sum px_i dx_i) / 12.5, axy = (sum py_i dx_i) / 12.5, ayx = (sum px_i dy_i) / 12.5,
 *                 ayy = (sum py_i dy_i) / 12.5; L_ix = (mx + axx px_i) + axy py_i, L_iy = (my + ayx px_i) + ayy py_i.
 *   Shaped displacement.  s = (double)strength, k = 1.0 - (double)rigidity;
 *                 F'_i = (float)(s * (L_i + k * (d_i - L_i))), one rounding to nearest per component.
 * L is the least-squares fit of the model to the 25 displacements (the grid's moments above make the normal equations
 * diagonal).  A NaN in a frame's F_t makes that frame's F' NaN at all 25 points, in the component it stands in (it enters
 * that component's mean) and, with DVSG_SHAPE_SIMILARITY, in the other as well (a and b sum both); other frames are unaffected.
 *
 * The contract.  An entry point given a shaped view v and F_t writes and uses exactly what it would if given the unshaped
 * view with v's filter and border and F', bit for bit: T and every output.  The entry points that read the shape are the
 * ones that turn F_t into T through a handle: dvsg_tps_render_u8, dvsg_tps_render_zoom_u8, dvsg_tps_render_nv12,
 * dvsg_tps_render_zoom_nv12, dvsg_tps_coverage_net_f32 and dvsg_tps_coefficients_f32 -- so the coverage scan of a shaped
 * view counts the border its render draws.  Every other entry point (dvsg_locnet_forward_*, dvsg_stabilize_*, the ring
 * and the masked entry points) behaves on a shaped view exactly as on the parent: the recurrence never sees the shape.
 * A shaped view launches one kernel in the place of the one that forms T (F' stays in shared memory; F_t is not written):
 * the count of launches is that of the unshaped view. */
#define DVSG_SHAPE_AFFINE 0
#define DVSG_SHAPE_SIMILARITY 1
#define DVSG_SHAPE_TRANSLATION 2
int dvsg_locnet_view_create_shaped(const dvsg_locnet_t *net, int render_filter, int render_border, int shape_model,
                                   float strength, float rigidity, dvsg_locnet_t **view);
int dvsg_locnet_render_shape(const dvsg_locnet_t *net, int *shape_model, float *strength, float *rigidity);

/* P010 frames: the surface format.  Whether the planes that dvsg_tps_render_nv12 and dvsg_tps_render_zoom_nv12 read and
 * write hold 8-bit samples (NV12) or 10-bit samples in 16-bit words (P010: what a hardware decoder hands over for HEVC
 * Main10) is, like the filter, the border and the shape, a property of the handle: no entry point is added for it.  Both
 * functions are host-side: no stream, no device work, everything decided before anything is allocated.
 *   dvsg_locnet_view_create_surface  a view of `net`'s parent that carries `net`'s OWN filter, border and shape -- these
 *          are INHERITED here, unlike in the three constructors above, whose views have what their arguments say and
 *          nothing else (and so DVSG_SURFACE_NV12) -- and the given surface format.  The view rules are the ones above: a
 *          view of a view is a view of the parent, calibrating through a view and destroying a parent with live views are
 *          refused.  An unknown format or a NULL pointer is DVSG_ERR_INVALID_ARG ("surface_format=<n>").
 *   dvsg_locnet_render_surface  the handle's format: 0 for NULL, for every handle of dvsg_locnet_create and for every view
 *          of dvsg_locnet_view_create, _border and _shaped.
 * ONLY dvsg_tps_render_nv12 and dvsg_tps_render_zoom_nv12 read the format.  Every other entry point -- dvsg_tps_render_u8,
 * dvsg_tps_render_zoom_u8, dvsg_tps_coverage_net_f32, dvsg_tps_coefficients_f32 and all the rest -- behaves on a P010 view
 * exactly as on the same view without the property, bit for bit.  dvsg_frames_nv12_to_rgb_u8 and dvsg_frames_ingest_nv12 take
 * no handle and are 8-bit only: the network sees 10-bit footage through the NV12 surface made of each word's high byte.
 *
 * Given a DVSG_SURFACE_P010 view, the two renders take P010 surfaces through their existing arguments:
 *   Layout.  A Y plane and an interleaved UV plane (U0 V0 U1 V1 ...) of 16-bit LITTLE-ENDIAN words, placed by y, uv, pitch
 *          and frame_stride as for NV12.  W and H count samples; pitch and frame_stride count BYTES.  A sample is
 *          s = word >> 6, in [0, 1023]; the low 6 bits are ignored on input and written as 0.
 *   Checks, before any device work.  The NV12 rules with pitch >= 2 W in the place of pitch >= W; pitch, frame_stride (where
 *          n > 1) and the four plane pointers are 2-byte aligned.  DVSG_ERR_INVALID_ARG; the message names the argument.
 *   Per plane.  Each plane is an image of its own size under the same normalised TPS map, as for NV12; T is written as
 *          dvsg_tps_render_u8 writes it.  Every float32 operation is rounded on its own, in both filters; NaN gives word 0.
 *            luma    C = 1, (H, W):          in (float)s / 1023.0f,
 *                                            out clamp(floor((double)v * 1023.0 + 0.5), 0, 1023) << 6;
 *            chroma  C = 2, (H / 2, W / 2):  in (float)((int)s - 512) / 1023.0f,
 *                                            out clamp(floor((double)v * 1023.0 + 512.5), 0, 1023) << 6.
 *          The bilinear render is dvsg_tps_warp_f32 / dvsg_tps_warp_zoom_f32 on those float images, bit for bit.  An
 *          invalid sample under DVSG_BORDER_BLACK is luma word 0 and chroma word 512 << 6, the neutral value.
 *   Luma rounds to NEAREST in the bilinear render too, where NV12 luma truncates.  Truncation is no round trip at 10 bits:
 *          floor((double)((float)s / 1023.0f) * 1023.0) comes back one low for 519 of the 1024 values (the float32 quotient
 *          lies below s / 1023 for those), so an identity warp would darken half the codes.  Rounding to nearest and the
 *          chroma rule are exact for all 1024 values, and (float)s / 1023.0f equals (float)((double)s / 1023.0) for all of
 *          them (tests/test_p010_cpu.py holds the three counts).
 *   Bicubic, the three border modes, zoom and shaping apply as their paragraphs above state, with the sample rule of step 4
 *          and the output rule of step 6 replaced by the two lines above (the bilinear evaluation under REPLICATE / MIRROR
 *          rounds like every P010 output).  "No load touches a byte outside the used bytes of the source row" means the
 *          2 pw C bytes of a row.  Bytes beyond 2 W of an output row and bytes between frames are never written.
 *   A handle without the property launches the kernels it launched before; the P010 kernels are instantiations of their own. */
#define DVSG_SURFACE_NV12 0
#define DVSG_SURFACE_P010 1
int dvsg_locnet_view_create_surface(const dvsg_locnet_t *net, int surface_format, dvsg_locnet_t **view);
int dvsg_locnet_render_surface(const dvsg_locnet_t *net);

/* Output size: rendering at a delivery size.  The size of the frames that the four source-size renders WRITE is, like the
 * filter, the border, the shape and the surface format, a property of the handle: no entry point is added for it.  Both
 * functions are host-side: no stream, no device work, everything decided before anything is allocated.
 *   dvsg_locnet_view_create_scaled  a view of `net`'s parent that carries `net`'s OWN filter, border, shape and surface format
 *          (INHERITED, as in dvsg_locnet_view_create_surface, which now inherits the size as well) and an output size
 *          (out_H, out_W).  out_H == 0 && out_W == 0: "the source's size", an unscaled view.  Otherwise both are >= 1; anything
 *          else, or a NULL pointer, is DVSG_ERR_INVALID_ARG ("out_H=<n>").  The view rules are the ones above.
 *   dvsg_locnet_render_size  the handle's size; always DVSG_OK.  (0, 0) for NULL, for every handle of dvsg_locnet_create and
 *          for every view of dvsg_locnet_view_create, _border and _shaped.  Either pointer may be NULL.
 * ONLY dvsg_tps_render_u8, dvsg_tps_render_zoom_u8, dvsg_tps_render_nv12 and dvsg_tps_render_zoom_nv12 read the size.  Every
 * other entry point -- dvsg_tps_coverage_net_f32, which takes its grid as arguments, dvsg_tps_coefficients_f32 and all the
 * rest -- behaves on a scaled view exactly as on the same view without the property, bit for bit.
 *
 * Given a scaled view, a render reads its source (src_H, src_W) = (H, W) as before and writes frames of (oh, ow) = (out_H, out_W):
 *   Factors.  sy = max(1, ceil(H / oh)), sx = max(1, ceil(W / ow)), in integers, from the two sizes alone (never from zoom).
 *   Planes.  RGB and NV12 / P010 luma (H, W) -> (oh, ow); chroma (H / 2, W / 2) -> (oh / 2, ow / 2) with the same sy, sx.
 *          A plane (ph, pw) -> (po, qo) has the VIRTUAL grid (sy po, sx qo).
 *   Map.   x_s, y_s of every virtual sample are the bits of the grid-only form of dvsg_tps_warp_zoom_f32 (U == NULL,
 *          out == NULL, coord = V_src, the T this call writes, the call's zoom or none, out_h x out_w = the virtual grid).
 *   Value. v[p][q] of a virtual sample is what the view's filter and border give at that (x_s, y_s) on the source plane: the
 *          paragraphs above, unchanged, the float32 value before any byte rule.  An invalid virtual sample under
 *          DVSG_BORDER_BLACK contributes what sampler A or the cubic gives there (0), so the black border fades over one
 *          output pixel.
 *   Average.  Output sample (i, j) averages virtual rows sy i .. sy i + sy - 1 and columns sx j .. sx j + sx - 1, row-major,
 *          every float32 operation rounded on its own: acc = v[0][0]; acc = acc + v[p][q] for the rest;
 *          out = acc / (float)(sx sy).
 *   Output rule.  The plane's existing rule applied to `out`: RGB / luma bytes truncate under bilinear and round to nearest
 *          under bicubic, chroma rounds at 128.5, P010 words round, out_f32 is stored as it is.  T is written exactly as
 *          dvsg_tps_render_u8 writes it.
 *   Buffers.  out_f32 [n, oh, ow, 3]; out_u8 [n, oh, u8_W, 3] in columns [u8_x0, u8_x0 + ow); out_y / out_uv planes of an
 *          (oh, ow) frame with out_pitch >= ow (P010: 2 ow) and out_frame_stride >= oh out_pitch.  Bytes beyond that are never
 *          written.  No load touches a byte outside the used bytes of the source row it reads.
 *   Checks, before any device work; DVSG_ERR_INVALID_ARG, the message names the argument.  sx > 4 or sy > 4 (more than 4x
 *          minification is not served); DVSG_BORDER_KEEP on a view whose size differs from the source's; for the NV12 / P010
 *          renders, out_H or out_W odd or below 4.
 *   Identity.  A scaled view whose size equals the call's (H, W), or is (0, 0), launches the kernels of the same view without
 *          the property, and so produces their bits; the scaled kernels are kernels of their own. */
int dvsg_locnet_view_create_scaled(const dvsg_locnet_t *net, int out_H, int out_W, dvsg_locnet_t **view);
int dvsg_locnet_render_size(const dvsg_locnet_t *net, int *out_H, int *out_W);

/* Chroma sampling: 4:2:2 frames (NV16, and P210 on a DVSG_SURFACE_P010 view).  How many ROWS the interleaved UV plane of the
 * frames that dvsg_tps_render_nv12 and dvsg_tps_render_zoom_nv12 read and write has is, like the filter, the border, the
 * shape, the surface format and the size, a property of the handle: no entry point is added for it.  It is orthogonal to the
 * surface format, which stays "the sample type".  Both functions are host-side: no stream, no device work, everything
 * decided before anything is allocated.
 *   dvsg_locnet_view_create_chroma  a view of `net`'s parent that carries `net`'s OWN filter, border, shape, surface format
 *          and output size (INHERITED, as in dvsg_locnet_view_create_surface and _scaled, which now inherit the chroma format
 *          as well) and the given chroma format.  An unknown value or a NULL pointer is DVSG_ERR_INVALID_ARG
 *          ("chroma_format=<n>"); the value is checked before the handle is read.  The view rules are the ones above.
 *   dvsg_locnet_render_chroma  the handle's value: 0 for NULL, for every handle of dvsg_locnet_create and for every view of
 *          dvsg_locnet_view_create, _border and _shaped.
 * ONLY dvsg_tps_render_nv12 and dvsg_tps_render_zoom_nv12 read the property.  Every other entry point -- dvsg_tps_render_u8,
 * dvsg_tps_render_zoom_u8, dvsg_tps_coverage_net_f32, dvsg_tps_coefficients_f32 and all the rest -- behaves on such a view
 * exactly as on the same view without it, bit for bit.  dvsg_frames_ingest_nv12 takes no handle and is 4:2:0 only: the network
 * sees 4:2:2 footage through the NV12 surface made of the Y plane and the EVEN chroma rows.
 *
 * Given a DVSG_CHROMA_422 view, the two renders take a 4:2:2 frame through their existing arguments:
 *   Layout.  The y plane is as before.  The uv plane is interleaved U0 V0 U1 V1 .. of H ROWS (4:2:0: H / 2), each of W / 2
 *          pairs: W samples, W bytes (P010 words: 2 W bytes), with the same pitch and frame_stride as luma.  A packed tensor is
 *          [n, 2 H, W] (P210: [n, 2 H, 2 W] bytes) with uv = y + H * pitch and frame_stride = 2 H * pitch.
 *   Checks.  The NV12 and P010 ones, unchanged: H and W even and >= 4, the pitch rules, 2-byte alignment for words.
 *   Per plane.  Chroma is an image of (H, W / 2) with C = 2 under the same normalised TPS map: dvsg_tps_warp_f32 / _zoom_f32 on
 *          a grid of that size, bit for bit, for the bilinear filter.  The filter, the border mode, shaping, zoom and the
 *          sample and output rules are those of the view's surface format, as their paragraphs above state with (H, W / 2) in
 *          the place of (H / 2, W / 2).  Luma is what the same view without the property gives, bit for bit.
 *   Scaled.  On a scaled view chroma maps (H, W / 2) -> (oh, ow / 2) with the same sy, sx; the virtual grid is
 *          (sy oh, sx ow / 2).  The scaled view's checks stay: oh, ow even and >= 4, factors <= 4, no DVSG_BORDER_KEEP.
 *   Buffers.  Bytes beyond the used bytes of a row and between frames are never written; no load touches a byte outside the
 *          used bytes of the source row it reads.
 *   4:4:4 is not served: its UV row is 2 W samples, which breaks "both planes use the same pitch" for packed frames.
 *   A handle without the property produces the bytes it produced. */
#define DVSG_CHROMA_420 0
#define DVSG_CHROMA_422 1
int dvsg_locnet_view_create_chroma(const dvsg_locnet_t *net, int chroma_format, dvsg_locnet_t **view);
int dvsg_locnet_render_chroma(const dvsg_locnet_t *net);

/* patches [B,H,W,c_in] in [0,1] -> F_t [B,25,2].  float32 storage, exact-f32 MFMA
 * (v_mfma_f32_32x32x2_f32) accumulation.  c_in != 21: conv1 is the same arithmetic in the root-conv kernel. */
int dvsg_locnet_forward_f32(const dvsg_locnet_t *net, const float *patches, int B, int H, int W,
                            float *F_t, void *workspace, size_t workspace_bytes, void *stream);

/* Debug / parity tap: run the network up to and including `stage` and copy that stage's
 * activation (NHWC float32) to act_out.  Stages: 0 conv1, 1 pool1, 2..17 the 16 bottleneck
 * units in order, 18 pool5 [B,2048].  act_dims receives (h, w, c) on the HOST. */
int dvsg_locnet_forward_tap_f32(const dvsg_locnet_t *net, const float *patches, int B, int H,
                                int W, int stage, float *act_out, size_t act_out_bytes,
                                int *act_dims_host, void *workspace, size_t workspace_bytes,
                                void *stream);

/* The evaluation graph of model.py:98-123 in one call: F_t = localizationNet(patches_t);
 * T = solve(V_src, F_t); s_t_pred = TPS warp of u_t.  V_src is the constant 5x5 grid of
 * model.py:105-110.  s_t_pred [B,H,W,3]; F_t [B,25,2], x_s, y_s [B*H*W] optional. */
int dvsg_stabilize_f32(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B,
                       int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Building block of localizationNet, exposed for layer-level parity tests and micro-benchmarks:
 * slim conv2d (1x1, or 3x3 with pad 1 = conv2d_same) + folded BatchNorm + optional residual +
 * optional ReLU as one implicit-GEMM launch.  x [B,H,W,Cin]; wt [Cout][ksize*ksize*Cin] (k order
 * kh, kw, c; BatchNorm scale already folded in); bias [Cout]; res (optional) is sampled at
 * (ho*res_stride, wo*res_stride) of a [B, (Ho-1)*res_stride+1, (Wo-1)*res_stride+1, Cout] tensor;
 * y [B,Ho,Wo,Cout] with Ho = (H-1)/stride+1.  Cin % 32 == 0, Cout % 64 == 0.
 * scratch (optional, 256-byte aligned; 17 MiB serves split-K, 65 MiB also the stream-K tail): lets
 * launches with few output tiles (batch 1-2) split K over several workgroups per tile, and lets
 * large launches cut the partly filled last round of tiles into equal (tile, K-stage) shares; the
 * partial tiles are summed in K order by the last workgroup to arrive, so results stay bitwise
 * reproducible from run to run. */
int dvsg_conv_gemm_f32(const float *x, const float *wt, const float *bias, const float *res, float *y,
                       int B, int H, int W, int Cin, int Cout, int ksize, int stride, int relu,
                       int res_stride, void *scratch, size_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * float16 variants (BASELINE.json configs[4]: "fp16 MFMA convs").  Same arguments and the same
 * float32 inputs / outputs as the _f32 entry points; inside, activations and conv weights are
 * stored as float16 and the 1x1 / 3x3 convolutions run on v_mfma_f32_32x32x16_f16 with float32
 * accumulation, their weights kept as float16 hi / lo pairs (see dvsg_conv_gemm_f16s: a plain float16
 * weight is off by up to 2^-12 relative at EVERY pixel alike, which the global average pool does not
 * average away -- it was 9/10 of this mode's error in F_t); conv1 multiplies float16 copies of the
 * scaled frames and writes f16 (c_in != 21: conv1 multiplies the float32 scaled frames exactly and rounds only its output to f16); BatchNorm shift, the dense head, the TPS solve and the warp stay float32.  Not bit-compatible with the
 * float32 reference path: tests/test_gpu_f16.py states the measured F_t / pixel error.
 * The workspace of dvsg_locnet_workspace_bytes is sufficient (half of it is used).
 * ------------------------------------------------------------------------------------- */
int dvsg_locnet_forward_f16(const dvsg_locnet_t *net, const float *patches, int B, int H, int W,
                            float *F_t, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_locnet_forward_tap_f16(const dvsg_locnet_t *net, const float *patches, int B, int H,
                                int W, int stage, float *act_out, size_t act_out_bytes,
                                int *act_dims_host, void *workspace, size_t workspace_bytes,
                                void *stream);
int dvsg_stabilize_f16(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B,
                       int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s,
                       void *workspace, size_t workspace_bytes, void *stream);
/* Calibration of the float16 mode (optional; round 4).  The hi / lo weight pairs cost twice the matrix-core work to remove
 * ONE thing: the bias a rounded float16 weight leaves in its output channel through the MEAN of its input channel,
 * sum_k (q_k - w_k) mu_k -- the same at every pixel, so the global average pool keeps it.  Given calibration windows
 * `patches` [B,H,W,c_in] (a few frames of the clip about to be stabilised), this call measures mu per convolution input
 * in one float32 pass and re-rounds the PLAIN float16 copy of every weight of blocks 2-4 to one of its two float16
 * neighbours so that the running sum of (q_k - w_k) mu_k along K stays within half a step ("error feedback"); from then
 * on the float16 entry points of this handle run blocks 2-4 on those plain weights (half the MFMAs) and keep the pairs in
 * block 1.  Measured on MI355X (synthetic checkpoint, 720p, against a float64 CPU evaluation): F_t 2.0-2.6e-6 where the
 * pairs give 1.4-1.9e-6 and round-to-nearest plain weights 1.9e-5; 22 % less time per step (tests/test_gpu_f16.py,
 * tools/f16_ef_masks.py).  The means are those of the calibration windows: frames of other statistics bring part of the
 * bias back (bounded by the plain mode's).  Deterministic (fixed-order sums); synchronous; mutates the handle, so not
 * while another thread runs it.  patches == NULL restores the uncalibrated state (pairs everywhere). */
int dvsg_locnet_calibrate_f16(dvsg_locnet_t *net, const float *patches, int B, int H, int W, void *workspace,
                              size_t workspace_bytes, void *stream);
/* ---------------------------------------------------------------------------------------
 * "f32s": float32 storage, float32 accumulation, float32-equivalent PRODUCTS from the float16 matrix
 * cores.  Same tensors, same workspace, same launch sequence as the *_f32 entry points (the dense head, the
 * TPS solve and the warp are the float32 kernels themselves; the max and average pools join the two pieces of
 * a value, which is exact; c_in != 21: conv1 forms exact float32 products and only stores its output as the two pieces);
 * in conv1 (conv1_split_kernel) and the 52 1x1 / 3x3
 * convolutions every operand enters the matrix cores as two float16 pieces, x ~ f16(x) + f16(x - f16(x))
 * (22 significant bits while |x| >= 2^-3;
 * the second piece is NOT scaled, so below that it falls into float16's subnormal range -- absolute step 2^-24 --
 * and the pair carries about log2(|x|) + 25 bits: 20 at |x| = 0.03, 15 at 1e-3, plain float16's 11 at 1e-4), and a product is three
 * v_mfma_f32_32x32x16_f16 -- a1 w1 + a2 w1 + a1 w2, each
 * exact in float32 -- instead of eight v_mfma_f32_32x32x2_f32.  The activation tensors between the layers
 * (library workspace) hold the two pieces of each value instead of one float32, so they are split once,
 * by the layer that produces them.  Measured against the
 * exact path: stage activations within 2e-6 relative, F_t within 1e-7, i.e. what two float32 GEMMs with
 * different summation orders differ by; every float32 parity test of tests/ also passes in this mode
 * (tests/test_gpu_f32s.py) -- with operands of magnitude 0.03 .. 1 (the synthetic checkpoint, band-limited frames);
 * a checkpoint whose BatchNorm-folded weights or activations are much smaller loses bits as stated above
 * (tests/test_gpu_f32s.py::test_small_operands_lose_bits_as_documented) and is unpinned in this mode.
 * It is NOT the exact float32 arithmetic of the reference and is therefore a
 * separately named precision; dvsg_*_f32 stays the path of record.  Values must stay inside float16's range
 * (|x| < 65504; beyond it a piece is infinite), which BatchNorm-folded weights and post-BatchNorm activations
 * do by orders of magnitude.
 * ------------------------------------------------------------------------------------- */
int dvsg_locnet_forward_f32s(const dvsg_locnet_t *net, const float *patches, int B, int H, int W,
                             float *F_t, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_locnet_forward_tap_f32s(const dvsg_locnet_t *net, const float *patches, int B, int H,
                                 int W, int stage, float *act_out, size_t act_out_bytes,
                                 int *act_dims_host, void *workspace, size_t workspace_bytes,
                                 void *stream);
int dvsg_stabilize_f32s(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B,
                        int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s,
                        void *workspace, size_t workspace_bytes, void *stream);
/* One layer in that mode.  x, res, y are activation tensors in the mode's INTERNAL format: 4 bytes per
 * value, but as the value's two float16 pieces -- flat element e of the dense NHWC tensor (channels % 32
 * == 0) lives in 128-byte group e / 32: 32 hi halves, then 32 lo halves (dvsg_f32_to_pieces /
 * dvsg_pieces_to_f32 convert).  wt_pieces is [Cout][K/32][32 hi halves | 32 lo halves] float16 (hi = f16(w),
 * lo = f16(w - hi)).  A 32-k row stage of either operand is 128 bytes, like a float32 one. */
int dvsg_conv_gemm_f32s(const void *x, const void *wt_pieces, const float *bias, const void *res,
                        void *y, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                        int relu, int res_stride, void *scratch, size_t scratch_bytes, void *stream);
int dvsg_f32_to_pieces(const float *x, void *y, size_t n, void *stream);   /* n % 32 == 0 */
int dvsg_pieces_to_f32(const void *x, float *y, size_t n, void *stream);

/* ---------------------------------------------------------------------------------------
 * "f32x3": float32 tensors everywhere -- boundary, workspace, every activation between the layers, exactly as the *_f32
 * entry points -- and float32 accumulation; inside conv1 and the 52 1x1 / 3x3 convolutions every PRODUCT is formed on the bfloat16
 * matrix cores from THREE bfloat16 pieces per operand, x = x1 + x2 + x3 with x1 = bf16(x), x2 = bf16(x - x1),
 * x3 = bf16(x - x1 - x2) (round to nearest).  bfloat16 has float32's exponent range and 8 significant bits, so the three
 * pieces hold all 24 significant bits of ANY finite float32 operand above 2^-110 -- no magnitude condition, unlike the two
 * float16 pieces of "f32s" -- and each piece product is exact in float32.  Of the nine cross terms of a w the six largest
 * (a1 w1, a1 w2, a2 w1, a2 w2, a1 w3, a3 w1) are accumulated, six v_mfma_f32_32x32x16_bf16 where the exact path issues
 * eight v_mfma_f32_32x32x2_f32 at 2.7 x the matrix-core time; the dropped a2 w3 + a3 w2 + a3 w3 are bounded by 2^-23 |a w|
 * -- one rounding of a float32 multiply; 2^-27 typically.  The large term a1 w1 and the five small ones accumulate in
 * SEPARATE float32 accumulators, joined once per tile: an MFMA adds its 16 products to the accumulator with the bits below the
 * accumulator's last place cut off, a bias that a shared accumulator lets through the network's average pool.
 * Activations are split in registers behind the LDS fragment read (conv1: once while its input row is staged; block 1's
 * fused conv2 + conv3: conv3's operand once per tile); weights once at load (dvsg_locnet_create; dvsg_pack_weights_f32x3 for
 * a single layer).  The pools, the dense head, the TPS solve and the warp are the float32 kernels themselves.  Measured
 * against float64 evaluations it is as close as the exact path is, layer by layer and end to end (tests/test_gpu_f32x3.py,
 * tests/test_f32x3_numerics_cpu.py); bitwise reproducible.  c_in != 21: conv1 is the float32 path's own kernel, bit for bit, and
 * the pieces begin behind it.  A separately named precision: dvsg_*_f32 stays the path whose
 * matrix instructions are float32 ones.
 * ------------------------------------------------------------------------------------- */
int dvsg_locnet_forward_f32x3(const dvsg_locnet_t *net, const float *patches, int B, int H, int W,
                              float *F_t, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_locnet_forward_tap_f32x3(const dvsg_locnet_t *net, const float *patches, int B, int H,
                                  int W, int stage, float *act_out, size_t act_out_bytes,
                                  int *act_dims_host, void *workspace, size_t workspace_bytes,
                                  void *stream);
int dvsg_stabilize_f32x3(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B,
                         int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s,
                         void *workspace, size_t workspace_bytes, void *stream);
/* One layer in that mode: x, res, y float32 as for dvsg_conv_gemm_f32 (Cin % 32 == 0, Cout % 64 == 0); wt_packed is what
 * dvsg_pack_weights_f32x3 makes of the float32 matrix wt [Cout][K] (K = ksize^2 Cin, the layout dvsg_conv_gemm_f32 takes):
 * 6 Cout K bytes, per group of 64 output channels and 32-k stage three 4 KB planes of bfloat16 pieces. */
int dvsg_conv_gemm_f32x3(const float *x, const void *wt_packed, const float *bias, const float *res,
                         float *y, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                         int relu, int res_stride, void *scratch, size_t scratch_bytes, void *stream);
int dvsg_pack_weights_f32x3(const float *wt, void *wt_packed, int Cout, int K, void *stream);
/* dvsg_conv3x3_1x1_f32 (below) in that precision: conv2 (3x3, Cin -> 64, + bias + ReLU) and conv3 (1x1, 64 -> Cout, + bias +
 * residual + ReLU) of a block-1 unit in one kernel, float32 tensors; wt2_packed / wt3_packed are dvsg_pack_weights_f32x3 of the
 * float32 matrices [64][9 Cin] and [Cout][64].  Cin % 32 == 0 (>= 64), Cout % 64 == 0. */
int dvsg_conv3x3_1x1_f32x3(const float *x, const void *wt2_packed, const float *bias2, const void *wt3_packed,
                           const float *bias3, const float *res, float *y, int B, int H, int W, int Cin, int Cout,
                           int stride, int res_stride, void *stream);

/* x, wt, res, y are float16 (Cin % 64 == 0); bias float32. */
int dvsg_conv_gemm_f16(const void *x, const void *wt, const float *bias, const void *res, void *y,
                       int B, int H, int W, int Cin, int Cout, int ksize, int stride, int relu,
                       int res_stride, void *scratch, size_t scratch_bytes, void *stream);
/* The layer as the float16 network runs it: float16 activations against weights kept as float16
 * hi / lo PAIRS, w ~ hi + 2^-11 lo (hi = f16(w), lo = f16((w - hi) * 2048)), i.e. effectively float32
 * weights at twice the matrix-core work and unchanged activation traffic.  wt_split is
 * [Cout/64][128][K]: for each group of 64 output channels 64 rows of hi, then 64 rows of lo.
 * scratch: as for dvsg_conv_gemm_f32 (tickets + 64 MiB of partial-tile slabs); with 3 x (2 Cout K) x 2 more bytes
 * behind them the call also makes the stage-packed weight copies the network's big launches run from
 * (dvsg_locnet_create keeps them per layer); otherwise it reads the weights from wt_split as they are: same results. */
int dvsg_conv_gemm_f16s(const void *x, const void *wt_split, const float *bias, const void *res, void *y,
                        int B, int H, int W, int Cin, int Cout, int ksize, int stride, int relu,
                        int res_stride, void *scratch, size_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Data formats either side of the path (the reference's eval.py driver, which keeps frames in
 * host NumPy arrays; here they stay in HBM).  channel_flip != 0 reverses the three channels of
 * every pixel (cv2's BGR <-> RGB, eval.py:79,113).
 * ------------------------------------------------------------------------------------- */
/* eval.py:80 `frame / 255.` (float64) as TF receives it (float32): dst = (float)((double)src / 255.0).
 * src [n_pixels*3] uint8, dst [n_pixels*3] float32 (16-byte aligned). */
int dvsg_frames_u8_to_f32(const uint8_t *src, size_t n_pixels, int channel_flip, float *dst, void *stream);
/* eval.py:80 with a size change: cv2.resize(frame / 255., (dst_W, dst_H)), default INTER_LINEAR,
 * on float64, result as float32.  src [n,src_H,src_W,3] uint8 -> dst [n,dst_H,dst_W,3] float32.
 * OpenCV is neither in the reference tree nor in this image: restated from its published
 * algorithm, parity unpinned.  u8_dst (optional) [n,dst_H,u8_W,3] receives np.uint8(resized * 255.)
 * -- rendered from the float64 value, as eval.py:112 does for the unstable half of its output
 * video -- in columns [u8_x0, u8_x0 + dst_W), in the channel order of src. */
int dvsg_frames_resize_u8_f32(const uint8_t *src, int n, int src_H, int src_W, int channel_flip, float *dst,
                              int dst_H, int dst_W, uint8_t *u8_dst, int u8_W, int u8_x0, void *stream);
/* eval.py:103-104 `np.concatenate(total_frames[sample_idx], axis=2)` for B windows at once:
 * patches[b, y, x, 3 s + c] = pool[idx[b*S + s], y, x, c].  pool [n_pool,H,W,3] float32, idx [B*S]
 * int32 ON THE DEVICE, patches [B,H,W,3S] float32 (16-byte aligned).  An index outside
 * [0, n_pool) reads as a frame of zeros. */
int dvsg_window_gather_f32(const float *pool, int n_pool, int H, int W, const int32_t *idx, int B, int S,
                           float *patches, void *stream);

/* ---------------------------------------------------------------------------------------
 * The evaluation graph fed straight from a FRAME RING: what eval.py:76-81,103-110 does on the
 * host -- frames / 255., np.concatenate of the S window frames on the channel axis (S = dvsg_locnet_in_channels / 3;
 * 7 in the reference's configuration), u_t = the newest of them -- happens inside conv1's load stage and the warp's tap
 * loads, so the [B,H,W,3S] window tensor never exists.
 *   pool   [n_pool,H,W,3] RGB frames on the device: float32 in [0,1] (dvsg_stabilize_ring_f32; e.g. the history of
 *          eval.py:93-124, whose write-back of s_t_pred is a float frame), or the raw uint8 frames
 *          (dvsg_stabilize_ring_u8: eval_train.py's clips, independent windows; 4x less input traffic).  uint8:
 *          float32(v / 255.) * 255 == v exactly for every byte value, so conv1's scaled input float(v) - mean is
 *          bit-identical to the float path's on the converted frame.
 *   table  [B,S] int32 ON THE DEVICE, S = dvsg_locnet_in_channels / 3: pool frame of window slot s of window b, oldest to newest (the `sample_idx`
 *          of eval.py:103; coupe.dvsg_amd.clip.window_index_table builds it for a whole clip).  u_t of window b is
 *          frame table[b][S-1].  An index outside [0, n_pool) reads as a frame of zeros (dvsg_window_gather_f32).
 *   precision  DVSG_PRECISION_F32 (the reference's arithmetic: bit-identical to dvsg_window_gather_f32 +
 *          dvsg_stabilize_f32 on the same frames), DVSG_PRECISION_F16, DVSG_PRECISION_F32S (same as the *_f16 / *_f32s
 *          entry points on the gathered window).
 * Outputs, workspace and stream as dvsg_stabilize_f32; s_t_pred may be a frame of `pool` itself only if no window
 * of this call reads it (eval.py:116 writes the result back into the history AFTER the step).
 * dvsg_locnet_forward_ring: the CNN alone from a ring -- F_t [B,25,2] into `out` (stage = -1), or the parity tap of
 * `stage` (0..18, see dvsg_locnet_forward_tap_f32) with its [h,w,c] in act_dims_host.
 * ------------------------------------------------------------------------------------- */
#define DVSG_PRECISION_F32 0
#define DVSG_PRECISION_F16 1
#define DVSG_PRECISION_F32S 2
#define DVSG_PRECISION_F32X3 3
int dvsg_stabilize_ring_f32(const dvsg_locnet_t *net, int precision, const float *pool, int n_pool,
                            const int32_t *table, int B, int H, int W, float *s_t_pred, float *F_t, float *x_s,
                            float *y_s, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_stabilize_ring_u8(const dvsg_locnet_t *net, int precision, const uint8_t *pool, int n_pool,
                           const int32_t *table, int B, int H, int W, float *s_t_pred, float *F_t, float *x_s,
                           float *y_s, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_locnet_forward_ring(const dvsg_locnet_t *net, int precision, const void *pool, int pool_is_u8, int n_pool,
                             const int32_t *table, int B, int H, int W, int stage, float *out, size_t out_bytes,
                             int *act_dims_host, void *workspace, size_t workspace_bytes, void *stream);
/* ---------------------------------------------------------------------------------------
 * ONLINE streams (eval.py:93-124 one frame at a time; coupe.dvsg_amd.online): each stream owns span + 2 consecutive
 * frames of a float32 pool from `base` (span = skip_length[-1] = 32): span + 1 HISTORY slots, stabilised frame j in
 * base + j % (span + 1), and one INPUT slot base + span + 1 holding the unstable frame of the current step.  The window
 * of step k:  k == 0: every entry the input slot (eval.py:93-94);  k >= 1: entry s < 6 the history slot of frame
 * max(k + skip[s] - span, 0) (frame 0 stands for the prepended copies after the write-back of eval.py:118-120), entry 6
 * the input slot.  Step k writes its result into the history slot of frame k, which no window of step k reads (it
 * held frame k - span - 1).  Several streams share one call: one table row and one out slot per stream.
 *   dvsg_stabilize_ring_inplace_f32  dvsg_stabilize_ring_f32 whose s_t_pred of window b is written into pool frame
 *          out_slots[b] (int32 [B] ON THE DEVICE) -- bit-identical to the contiguous s_t_pred of that call, in every
 *          DVSG_PRECISION_*.  An out slot outside [0, n_pool) stores no frame (F_t, x_s, y_s are still written).
 *          Contract, NOT checked on the device: the out slots of one call are distinct, and no entry of this call's
 *          `table` names any of them.
 *   dvsg_frames_ingest_u8  frame i of src [n,src_H,src_W,3] uint8 into pool frame slots[i] (int32 [n] on the device):
 *          dvsg_frames_u8_to_f32's conversion when the size is (dst_H, dst_W) -- u8_dst must then be NULL, the uint8
 *          half is rendered from the float32 slot by dvsg_frames_f32_to_u8_slots --, dvsg_frames_resize_u8_f32's resize
 *          (and optional u8_dst [n,dst_H,u8_W,3]) otherwise.  Same values as those two, bit for bit.  A slot outside
 *          [0, n_pool) is skipped.  n <= 65535.
 *   dvsg_frames_f32_to_u8_slots  dvsg_frames_f32_to_u8 of frame i = pool frame slots[i] (int32 [n] on the device) into
 *          row band i of dst; a slot outside [0, n_pool) reads as a frame of zeros.
 *   dvsg_tps_render_u8  the stabilised frame at SOURCE resolution: F_t [n,25,2] (the F_t of a dvsg_stabilize_* call,
 *          e.g. dvsg_stabilize_ring_inplace_f32 on the same stream) -> T [n,2,28] (written: the T of dvsg_stabilize_*
 *          for that F_t, bit for bit), then frame i of src [n,src_H,src_W,3] uint8 warped at its own size: out_f32
 *          [n,src_H,src_W,3] and/or out_u8 [n,src_H,u8_W,3] in columns [u8_x0, u8_x0 + src_W).  out_f32 is
 *          dvsg_tps_warp_f32(dvsg_frames_u8_to_f32(src, channel_flip), V_src, T, out = (src_H, src_W)) bit for bit
 *          (RGB), out_u8 is dvsg_frames_f32_to_u8(out_f32, channel_flip) (the channel order of src).  Either output may
 *          be NULL, not both.  n <= 65535.
 * ------------------------------------------------------------------------------------- */
int dvsg_stabilize_ring_inplace_f32(const dvsg_locnet_t *net, int precision, float *pool, int n_pool,
                                    const int32_t *table, const int32_t *out_slots, int B, int H, int W, float *F_t,
                                    float *x_s, float *y_s, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_frames_ingest_u8(const uint8_t *src, int n, int src_H, int src_W, int channel_flip, float *pool, int n_pool,
                          const int32_t *slots, int dst_H, int dst_W, uint8_t *u8_dst, int u8_W, int u8_x0, void *stream);
int dvsg_frames_f32_to_u8_slots(const float *pool, int n_pool, const int32_t *slots, int n, int H, int W, int channel_flip,
                                uint8_t *dst, int dst_W, int dst_x0, void *stream);
int dvsg_tps_render_u8(const dvsg_locnet_t *net, const float *F_t, const uint8_t *src, int n, int src_H, int src_W,
                       int channel_flip, float *T, float *out_f32, uint8_t *out_u8, int u8_W, int u8_x0, void *stream);
/* ---------------------------------------------------------------------------------------
 * ONLINE streams, SCENE CUTS (coupe.dvsg_amd.online, scene_cut=threshold): a live stream cuts, and after a cut the window of
 * the next span steps would mix two scenes.  dvsg_scene_step_f32 notices the cut on the device and restarts the ring's
 * history at that frame; it WRITES the step's `table` and `out_slots` for dvsg_stabilize_ring_inplace_f32, so the host
 * uploads ring numbers only and nothing is synchronised.  A cut at a stream's frame f is close() + open() onto the same ring
 * + push(f): f is step 0 (every window entry the input slot), the rows that follow count k from f, and the crop zoom of the
 * ring restarts.  History slots that still hold the old scene are never read: step k >= 1 of the new run reads frames
 * 0 .. k - 1 of that run only.
 *   The statistic, of pool frame base + span + 1 (the ring's input slot, float32 RGB at the model's size, after ingest --
 *   the same for uint8, float and NV12 sources), every float32 operation rounded on its own:
 *       Y   = fl(fl(fl(0.299f r) + fl(0.587f g)) + fl(0.114f b))
 *       q   = clamp((int)floorf(fl(Y 255f) + 0.5f), 0, 255), NaN -> 0;   bin = q >> 2: 64 bins of int32 counts over H W pixels
 *       S   = sum over bins |cur - prev|, an int32 in [0, 2 H W];  S = 0 at a ring's first frame (k == 0: no previous)
 *       cut <=> k >= max(1, min_len) and S >= thr_count              thr_count = ceil(threshold 2 H W), the host's, in float64
 *   Integer after the one quantisation: exact, the same on every run, in whatever order the workgroups arrive.
 *   state  int32 [n_state, DVSG_SCENE_STATE_INTS] on the device, row r of ring r: [0] k, the frames since the ring's last
 *          start (open, reset or cut); [1] the cuts so far; [2] the last S; [3] 0; [4, 68) the previous histogram.  A row
 *          of zeros is a ring before its first frame.  k is an int32: restart a ring before 2^31 - 1 frames.
 *   dvsg_scene_step_f32  per row b of the step, with r = rings[b] (int32 [B] ON THE DEVICE), span = skip_host[S - 1]
 *          (skip_host: the S skip lengths, int32 on the HOST, >= 0 and strictly increasing) and base = r (span + 2):
 *            1. the histogram of pool frame base + span + 1;  2. the decision above;
 *            3. on a cut: k = 0, state[r][1] += 1, and zoom_state[r] = crop_start when zoom_state (float32 [n_state], the
 *               state of dvsg_crop_ratchet_f32) is not NULL;
 *            4. table[b] [S] = the window of step k (ONLINE above), out_slots[b] = base + k % (span + 1), cut[b] = 0 / 1;
 *            5. state[r] = (k + 1, cuts, S, 0, the current histogram).
 *          A ring outside [0, n_state), or one whose input slot lies outside [0, n_pool), gets a table row of -1, an out
 *          slot of -1 and cut 0 and touches no state (the skipped-slot convention of dvsg_crop_ratchet_f32; an out slot
 *          of -1 makes dvsg_stabilize_ring_inplace_f32 store no frame).  The rings of one call must be distinct: the
 *          caller's contract, not checked on the device.  Checked before any device work: NULL pointers (zoom_state may
 *          be NULL), 1 <= B <= 65535, 1 <= S <= 16, 2 H W < 2^31, 1 <= thr_count <= 2 H W, min_len >= 0.  workspace:
 *          dvsg_scene_workspace_bytes(B) bytes, 16-byte aligned (DVSG_ERR_WORKSPACE if short): [B,64] int32, zeroed by the
 *          call.  Three launches: a fill of the workspace (a kernel: a captured memset node does not replay), the histogram
 *          pass (16-byte loads, one LDS histogram per wave, one global int32 atomic per non-zero bin and workgroup; pixels off the 16-byte grid at either end of a frame take a scalar
 *          path, nothing is padded) and the decision pass (one wave per row, lane = bin).  The pool is only read.
 * ------------------------------------------------------------------------------------- */
#define DVSG_SCENE_STATE_INTS 68
int dvsg_scene_workspace_bytes(int B, size_t *bytes);
int dvsg_scene_step_f32(const float *pool, int n_pool, int H, int W, const int32_t *rings, int B, const int32_t *skip_host,
                        int S, int32_t *state, int n_state, int thr_count, int min_len, float *zoom_state, float crop_start,
                        int32_t *table, int32_t *out_slots, int32_t *cut, void *workspace, size_t workspace_bytes,
                        void *stream);
/* ---------------------------------------------------------------------------------------
 * SHAKE MOTION (coupe.dvsg_amd.shake.measure_motion): roll, zoom and wobble of a clip from the same block vectors.  The median
 * of "SHAKE" sees translation only: under a roll the left blocks move up and the right ones down, and the median is about 0.
 * This call fits a similarity (translation + roll + zoom) to the blocks that agree with the median and reports, per pair, the
 * exact integer sums from which roll, zoom and the residual of the fit (wobble) follow on the host.  "SHAKE" is the next
 * section; read it first.
 * dvsg_shake_motion_u8 is synchronous and takes no stream: its result is a small HOST array, so it has to wait for
 * the device whatever its interface.  In order: 1. every argument is checked before any HIP call; 2. the call waits for the
 * device (hipDeviceSynchronize: whatever stream wrote the planes has finished); 3. it launches three kernels on the legacy
 * default stream; 4. it copies the results to the host and returns.  It allocates and frees nothing.
 *   luma, pitch, frame_stride, n, H, W, factor, radius, margin_y, margin_x, texture, min_blocks, blocks_host: as for
 *                 dvsg_shake_measure_u8.
 *   gate          in sixteenths of a reduced pixel, 0 <= gate <= 2^20: how far a block's vector may lie from the pair's median,
 *                 per axis, and still enter the fit.
 *   motion_host   int64 [n - 1, 13] on the HOST: row t - 1 describes frame t against frame t - 1.
 *   workspace     caller-owned device memory, 16-byte aligned, dvsg_shake_motion_workspace_bytes(...) bytes
 *                 (DVSG_ERR_WORKSPACE if short or misaligned, before any device work): the reduced planes, the per-block
 *                 results and the device copy of the rows.  No state survives a call.
 *   The rule.  Integer arithmetic throughout; tests/shake_motion_ref.py restates it in NumPy and the bar is bit equality.
 *   1. - 5. are those of "SHAKE", unchanged: the reduce, the blocks, the match, validity and the sixteenth-pel step, and the
 *      pair's [gx, gy, n_valid, ok].  Then, per pair:
 *   6. Block coordinates.  Block (a, c) of the ny x nx grid has X = 2c - (nx - 1) and Y = 2a - (ny - 1): integers in units of
 *      8 reduced pixels, with zero at the centre of the block grid.
 *   7. Inliers.  A block is an inlier iff it is valid, the pair is ok, |vx - gx| <= gate and |vy - gy| <= gate.  The gate keeps
 *      independently moving objects out of the fit and lets through the spread that roll and zoom cause at the edges.
 *   8. Sums over the inliers, exact, int64:  n_in;  Sx = sum X;  Sy = sum Y;  Su = sum vx;  Sv = sum vy;
 *      Sxx = sum (X*X + Y*Y);  Sxu = sum (X*vx + Y*vy);  Sxv = sum (X*vy - Y*vx);  Suu = sum (vx*vx + vy*vy).
 *      A side is at most 16384, so |X|, |Y| <= 1022, and |v| <= 248: every sum stays below 2^29 at any size the call accepts.
 *      The row is int64 all the same: the products the host makes of the sums (N * Sxx, Pn * Pn) are not.
 *   9. The row is [gx, gy, n_valid, ok, n_in, Sx, Sy, Su, Sv, Sxx, Sxu, Sxv, Suu].  Everything from n_in on is 0 when the pair
 *      is not ok.
 *   10. Checked before any device work (DVSG_ERR_INVALID_ARG, the message names the argument): gate outside [0, 2^20], NULL
 *      luma / motion_host / workspace / bytes, and everything dvsg_shake_measure_u8 checks; the workspace against
 *      dvsg_shake_motion_workspace_bytes (DVSG_ERR_WORKSPACE).
 *   The figures (coupe.dvsg_amd.shake.motion_figures; exact rationals, then one division and one square root each).  With
 *   N = n_in:  Pn = N*Sxu - Sx*Su - Sy*Sv;  Rn = N*Sxv - Sx*Sv + Sy*Su;  Qn = N*Sxx - Sx*Sx - Sy*Sy;  Vn = N*Suu - Su*Su - Sv*Sv.
 *   A pair is fit iff it is ok, N >= max(min_blocks, 3) and Qn > 0.  Then zoom = Pn / (128 Qn), the fractional size change per
 *   frame, and roll = Rn / (128 Qn) in radians per frame (small angles: exactly scale * sin); 128 = 16 sixteenths x 8 pixels per
 *   coordinate unit, and the signs follow the vectors' convention, cur[y][x] looks like prev[y+dy][x+dx].
 *   rss = (Vn*Qn - Pn*Pn - Rn*Rn) / (N*Qn) in sixteenths squared, clamped at 0; the pair's wobble is (f / 16) sqrt(rss / N)
 *   source pixels, the RMS distance of an inlier's vector from the fitted similarity.
 *   What the figures are not: an affine or projective fit; a threshold for "steady" or "wobbly" (the matcher has a wobble
 *   floor of its own, see DESIGN); anything about motion beyond the radius.
 *   Kernels (shake_kernels.hip): the reduction and the matcher of "SHAKE", untouched, then shake_motion_kernel in the place
 *   of the medians' kernel: one workgroup per pair, the same rows in LDS and the same rank counting, then every lane gates its
 *   blocks and adds up the nine sums in int64 registers; wave shuffles, LDS across the four waves, no atomics.
 * ------------------------------------------------------------------------------------- */
int dvsg_shake_motion_workspace_bytes(int n, int H, int W, int factor, int radius, int margin_y, int margin_x, size_t *bytes);
int dvsg_shake_motion_u8(const uint8_t *luma, size_t pitch, size_t frame_stride, int n, int H, int W, int factor, int radius,
                         int margin_y, int margin_x, int texture, int min_blocks, int gate, int64_t *motion_host,
                         int32_t *blocks_host, void *workspace, size_t workspace_bytes);
/* ---------------------------------------------------------------------------------------
 * SHAKE (coupe.dvsg_amd.shake): how much a clip moves from frame to frame, measured from its own luma planes -- no ground
 * truth, no model.  The global motion of every pair of consecutive frames by block matching, in sixteenths of a reduced
 * pixel.  dvsg_shake_measure_u8 is synchronous and takes no stream: its result is a small HOST array, so it has to wait for
 * the device whatever its interface.  In order: 1. every argument is checked before any HIP call; 2. the call waits for the
 * device (hipDeviceSynchronize: whatever stream wrote the planes has finished); 3. it launches three kernels on the legacy
 * default stream; 4. it copies the results to the host and returns.  It allocates and frees nothing.
 *   luma          n planes of H x W bytes ON THE DEVICE: row i of frame t at luma + t * frame_stride + i * pitch, W bytes used
 *                 -- the Y plane of an NV12 / NV16 batch is passed as it lies.  Only those bytes are read.
 *   vectors_host  int32 [n - 1, 4] on the HOST: row t - 1 describes frame t against frame t - 1.
 *   blocks_host   int32 [n - 1, n_blk, 3] on the HOST, or NULL.
 *   workspace     caller-owned device memory, 16-byte aligned, dvsg_shake_workspace_bytes(...) bytes (DVSG_ERR_WORKSPACE if
 *                 short or misaligned, before any device work): the reduced planes, the per-block results and the device copy
 *                 of the vectors.
 *   The rule.  All of it is integer arithmetic; tests/shake_ref.py restates it in NumPy and the bar is bit equality.
 *   1. Reduce.  With f = factor >= 1, h = H / f and w = W / f (integer division, trailing rows and columns dropped):
 *      r[i][j] = (sum of the f x f bytes + f*f/2) / (f*f), in uint8.  For f = 1 this is the plane itself.
 *   2. Blocks.  Blocks are 16 x 16 on the reduced plane.  Counts: ny = (h - 2*margin_y) / 16, nx = (w - 2*margin_x) / 16,
 *      n_blk = ny*nx.  Block (a, c) has its top-left at (margin_y + 16a, margin_x + 16c); it is row a*nx + c of blocks_host.
 *      Requirements: 1 <= radius <= 16, both margins >= radius, 1 <= n_blk <= 2048.  An n_blk above 2048 is
 *      DVSG_ERR_INVALID_ARG, and the text names factor.
 *   3. Match.  For a block of frame t at (y0, x0) and every (dy, dx) in [-R, R]^2:
 *      S(dy,dx) = sum over the 256 pixels |cur[y0+i][x0+j] - prev[y0+i+dy][x0+j+dx]|, which is at most 65280.
 *      The best candidate is the minimum under the order (S, dy*dy + dx*dx, dy, dx).  Equal SADs resolve to the shortest
 *      vector, then the smallest dy, then the smallest dx.  So cur[y][x] looks like prev[y+dy][x+dx]: the vector says where
 *      the content came from.
 *   4. Validity and the sixteenth-pel step.  A block is invalid when its best candidate lies on the search boundary
 *      (|dy| == R or |dx| == R).  Otherwise, with S0 the best SAD, Sxm / Sxp its left / right neighbours and Sym / Syp its
 *      upper / lower ones: cx = Sxm - 2*S0 + Sxp, and cy likewise, both >= 0.  The block is valid iff cx >= max(texture, 1)
 *      and cy >= max(texture, 1).  Flat blocks and blocks with edges in one direction only drop out here.
 *      vx = 16*dx + floor((16*(Sxm - Sxp) + cx) / (2*cx)), and vy likewise.  The division is a floor with a possibly
 *      negative numerator.  The fraction lies in [-8, 8].  Invalid blocks report (0, 0, 0); valid ones report (vx, vy, 1).
 *   5. Global vector of a pair.  n_valid counts the valid blocks, and ok = n_valid >= min_blocks (min_blocks >= 1).
 *      gx is the lower median of vx over the valid blocks: the element of rank (n_valid - 1) / 2 in sorted order.  gy is the
 *      same for vy, independently.  The row is [gx, gy, n_valid, ok], with gx = gy = 0 when not ok.  Units are sixteenths
 *      of a reduced pixel per frame.
 *   Checked before any device work (DVSG_ERR_INVALID_ARG, the message names the argument): NULL luma / vectors_host /
 *   workspace / bytes, 2 <= n <= 4096 (feed longer clips in chunks that overlap by one frame), 1 <= H, W <= 16384,
 *   1 <= factor <= 16, the requirements of 2., pitch >= W, frame_stride >= (H - 1) pitch + W, texture >= 0, min_blocks >= 1.
 *   What the figure is not: motion beyond the radius is lost, not measured; a scene cut gives one meaningless row.
 *   Kernels (shake_kernels.hip): the reduction (16-byte loads over every whole 16-byte unit of a row, a scalar path at the
 *   ragged ends, nothing padded), the matcher (one workgroup per block and pair; block and window staged in LDS once,
 *   v_sad_u8 on dwords formed with v_alignbyte_b32, all SADs kept in LDS as 16-bit values, the minimum one packed key per
 *   lane) and the medians (one workgroup per pair, rank counting).
 * ------------------------------------------------------------------------------------- */
int dvsg_shake_workspace_bytes(int n, int H, int W, int factor, int radius, int margin_y, int margin_x, size_t *bytes);
int dvsg_shake_measure_u8(const uint8_t *luma, size_t pitch, size_t frame_stride, int n, int H, int W, int factor, int radius,
                          int margin_y, int margin_x, int texture, int min_blocks, int32_t *vectors_host, int32_t *blocks_host,
                          void *workspace, size_t workspace_bytes);
/* ---------------------------------------------------------------------------------------
 * NV12 frames (coupe.dvsg_amd.online, frame_format="nv12"): what a hardware decoder hands over and an encoder takes.
 * Layout of a batch of n frames of H x W (H, W even, >= 4):
 *   y   uint8: row i of frame f at y + f * frame_stride + i * pitch, W bytes used;
 *   uv  uint8: row i of frame f at uv + f * frame_stride + i * pitch, W bytes used: U0 V0 U1 V1 ..., H / 2 rows;
 *   pitch  the row pitch in bytes, >= W; frame_stride in bytes (>= H * pitch when n > 1; both planes use the same two).
 * A packed tensor [n, 3 H / 2, W] has uv = y + H * pitch, pitch = W, frame_stride = 3 H / 2 * W; a decoder surface with an
 * aligned luma height passes its own uv pointer.  Outputs are described the same way (out_y, out_uv, out_pitch,
 * out_frame_stride) and must not overlap the inputs; bytes of a row beyond W are never written.
 *
 * YUV -> RGB is integer arithmetic with shift 20, exact and the same on every run (OpenCV's published COLOR_YUV2RGB_NV12
 * scheme; OpenCV is not on the build machine: parity with cv2 is unpinned, as for the resize).  The chroma of luma pixel
 * (i, j) is the sample (i / 2, j / 2), replicated, no interpolation.  On int32 (the sums stay below 2^30; >> arithmetic):
 *     y = max(0, Y - 16) * CY;  u = U - 128;  v = V - 128
 *     R = sat8((y + CVR * v           + 2^19) >> 20)
 *     G = sat8((y + CVG * v + CUG * u + 2^19) >> 20)
 *     B = sat8((y + CUB * u           + 2^19) >> 20)
 *   matrix                      CY       CVR      CVG      CUG      CUB     = int(round(c * 2^20)) of
 *   DVSG_YUV_BT601_LIMITED (0)  1220542  1673527  -852492  -409993  2116026   1.164, 1.596, -0.813, -0.391, 2.018 (OpenCV's)
 *   DVSG_YUV_BT709_LIMITED (1)  1220945  1879825  -558796  -223608  2215014   1.164384, 1.792741, -0.532909, -0.213249,
 *                                                                            2.112402
 *   dvsg_frames_nv12_to_rgb_u8  the conversion into dst [n,H,W,3] uint8, RGB, or BGR with channel_flip.  n <= 65535.
 *   dvsg_frames_ingest_nv12  frame i into float32 pool frame slots[i] (int32 [n] on the device) at (dst_H, dst_W), RGB:
 *          bit-identical to dvsg_frames_nv12_to_rgb_u8(channel_flip = 0) followed by dvsg_frames_ingest_u8(channel_flip = 0,
 *          u8_dst = NULL), on the same-size path ((float)(v / 255.) of the float64 quotient) and on the resize path (the
 *          cv2-style float64 bilinear of dvsg_frames_resize_u8_f32: same tap rule, same operations in the same order).  The
 *          source-size RGB image never exists: each output pixel converts its (at most four) taps.  A slot outside
 *          [0, n_pool) skips its frame.  n <= 65535.
 *   dvsg_tps_render_nv12  the stabilised frame at source resolution, NV12 in and out: F_t [n,25,2] -> T [n,2,28] (written
 *          exactly as dvsg_tps_render_u8 writes it, bit for bit), then ONE launch that warps both planes of all n frames.
 *          Each plane is an image of its own size warped by the same normalised TPS map with sampler A, i.e.
 *          dvsg_tps_warp_f32(plane, V_src, T, out = the plane's size) bit for bit on
 *            luma    C = 1, (H, W):          in (float)((double)Y / 255.0),          out np.uint8(v * 255.) (float64
 *                                            product, truncation, saturating: dvsg_frames_f32_to_u8's rule);
 *            chroma  C = 2, (H / 2, W / 2):  in (float)(((double)c - 128.0) / 255.0), out clamp(floor((double)v * 255.0 +
 *                                            128.5), 0, 255).
 *          Both byte round trips are exact.  Chroma is warped centred on 128, so sampler A's black border (coincident
 *          taps) is luma 0 with neutral chroma 128.  The chroma grid is corner-aligned like the luma grid (tf.linspace at
 *          each plane's size), within one luma pixel of left-sited chroma.  No zoom (dvsg_tps_render_zoom_nv12).  n <= 65535.
 *   dvsg_tps_render_zoom_nv12  dvsg_tps_render_nv12 on the output grid scaled about its centre by zoom[i] (float32 [n] ON THE
 *          DEVICE, one value per frame; see CROP below): each plane is dvsg_tps_warp_zoom_f32(plane, V_src, T, zoom, out =
 *          the plane's size) bit for bit, with the byte rules, the layout, the argument checks and the n <= 65535 of
 *          dvsg_tps_render_nv12; T is written as dvsg_tps_render_u8 writes it.  zoom[i] == 1.0f gives dvsg_tps_render_nv12's
 *          bytes; zoom NULL: dvsg_tps_render_nv12 itself.
 * Every argument is checked before the first launch.
 * dvsg_frames_nv12_to_rgb_u8 and dvsg_frames_ingest_nv12 take no handle and are 8-bit only.  The two renders read and write
 * P010 surfaces (10-bit samples in 16-bit words) when the handle they are given is a DVSG_SURFACE_P010 view: "P010 frames" above.
 * ------------------------------------------------------------------------------------- */
#define DVSG_YUV_BT601_LIMITED 0
#define DVSG_YUV_BT709_LIMITED 1
int dvsg_frames_nv12_to_rgb_u8(const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int H, int W,
                               int matrix, int channel_flip, uint8_t *dst, void *stream);
int dvsg_frames_ingest_nv12(const uint8_t *y, const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int src_H,
                            int src_W, int matrix, float *pool, int n_pool, const int32_t *slots, int dst_H, int dst_W,
                            void *stream);
int dvsg_tps_render_nv12(const dvsg_locnet_t *net, const float *F_t, const uint8_t *y, const uint8_t *uv, size_t pitch,
                         size_t frame_stride, int n, int H, int W, float *T, uint8_t *out_y, uint8_t *out_uv,
                         size_t out_pitch, size_t out_frame_stride, void *stream);
int dvsg_tps_render_zoom_nv12(const dvsg_locnet_t *net, const float *F_t, const uint8_t *y, const uint8_t *uv, size_t pitch,
                              size_t frame_stride, int n, int H, int W, const float *zoom, float *T, uint8_t *out_y,
                              uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, void *stream);
/* ---------------------------------------------------------------------------------------
 * CROP to the valid region (coupe.dvsg_amd.clip.stabilize_clip(crop=...)).  Sampler A clips its tap indices before it forms
 * the weights, so an output pixel whose source sample lies outside 0 <= x < W - 1, 0 <= y < H - 1 (x = ((x_s + 1) W) / 2 in
 * float32, as the sampler takes it) blends coincident taps with cancelling weights and is 0 (up to the rounding of that sum): the black border of a
 * stabilised frame.  A pixel is VALID iff its four taps are distinct after the clip, (x1 - x0)(y1 - y0) == 1; NaN is invalid.
 * The crop is a ZOOM of the output grid about its centre, x_t' = z x_t, y_t' = z y_t (one float32 multiply each on
 * tf.linspace's values; z = 1.0f gives the plain entry points' bits), composed into the TPS map, so every output pixel is
 * still interpolated exactly once.  zoom is float32 [B] ON THE DEVICE, one value per sample.
 *   dvsg_tps_coverage_f32  one fused scan: the TPS map of dvsg_tps_warp_zoom_f32 (same bits for the same coord, T, zoom),
 *          the validity test against a source of src_H x src_W, and per sample b
 *            n_border[b]  int32: the number of invalid output pixels;
 *            key_min[b]   int32: the minimum over the invalid pixels (i, j) of
 *                         key = max(|2 j - (out_w - 1)| (out_h - 1), |2 i - (out_h - 1)| (out_w - 1)),
 *                         INT32_MAX when none is invalid.  With D = (out_h - 1)(out_w - 1), key / D is the pixel's
 *                         normalised Chebyshev distance from the centre: every pixel with key < key_min is valid, the
 *                         largest centred rectangle of the frame's aspect ratio that holds no border.
 *          x_s / y_s never reach memory.  Integer results: exact, the same on every run; the outputs need no zeroing.
 *          zoom NULL = 1.  out_h, out_w >= 2, D < 2^31 - 1, B <= 65535.  workspace: dvsg_tps_coverage_workspace_bytes
 *          bytes, 8-byte aligned (one partial per workgroup; DVSG_ERR_WORKSPACE if short, before any launch).
 *   dvsg_tps_warp_zoom_f32  dvsg_tps_warp_f32 on the zoomed grid: same thread layout, same outputs, the grid-only form
 *          (U == NULL && out == NULL) included.  zoom NULL: dvsg_tps_warp_f32 itself.
 *   dvsg_tps_coverage_net_f32  F_t [n,25,2] -> T [n,2,28] (written: the T of dvsg_tps_render_u8 for that F_t, bit for
 *          bit), then dvsg_tps_coverage_f32 on that T with the handle's V_src.
 *   dvsg_tps_render_zoom_u8  dvsg_tps_render_u8 on the zoomed grid; zoom NULL: dvsg_tps_render_u8 itself.
 *   dvsg_tps_coefficients_f32  F_t [n,25,2] -> T [n,2,28] alone, exactly as dvsg_tps_render_u8 writes it: for
 *          dvsg_tps_warp_zoom_f32 on frames that no scan or render has written T for (a fixed zoom at the model's size).
 *   dvsg_crop_ratchet_f32  the zoom of LIVE streams (coupe.dvsg_amd.online, crop="auto"), kept on the device so that a step
 *          synchronises nothing.  For the n frames of a step: key_min_a [n] int32 with D_a = (out_h - 1)(out_w - 1) of its
 *          scan; optionally key_min_b [n] with D_b, a second plane's scan (NULL: absent; NV12 passes luma and chroma);
 *          state_slots [n] int32, frame i's index into state, float32 [n_state].  Per frame i, in float64, every
 *          operation rounded on its own:
 *              free   = min(key_a, D_a) / D_a;  with b: free = min(free, min(key_b, D_b) / D_b)
 *              target = min(max(free - margin, crop_min), 1.0)
 *              z      = min(target, (double)state[slot] + recover)
 *              state[slot] = zoom[i] = (float)z        one rounding to nearest;  free_out[i] = free (float64)
 *          A slot outside [0, n_state) skips its frame (nothing of it is written).  The slots of one call must be
 *          distinct (the caller's contract; coupe.dvsg_amd.online checks it on the host).  margin >= 0, 0 < crop_min <= 1,
 *          recover >= 0, D >= 1, checked before the launch.  recover = 0 is a pure ratchet: a stream's zoom only ever
 *          shrinks, and from a state of 1 it ends at crop_zoom(all frees, margin, crop_min) of the whole stream bit for
 *          bit, because min and max commute and the float32 rounding is monotone.  One thread per frame, no atomics.
 * ------------------------------------------------------------------------------------- */
int dvsg_tps_coverage_workspace_bytes(int B, int out_h, int out_w, size_t *bytes);
int dvsg_tps_coverage_f32(const float *coord, const float *T, const float *zoom, int B, int P, int src_H, int src_W,
                          int out_h, int out_w, int32_t *n_border, int32_t *key_min, void *workspace,
                          size_t workspace_bytes, void *stream);
int dvsg_tps_warp_zoom_f32(const float *U, const float *coord, const float *T, const float *zoom, int B, int H, int W,
                           int C, int P, int out_h, int out_w, float *out, float *x_s, float *y_s, void *stream);
int dvsg_tps_coverage_net_f32(const dvsg_locnet_t *net, const float *F_t, const float *zoom, int n, int src_H, int src_W,
                              int out_h, int out_w, float *T, int32_t *n_border, int32_t *key_min, void *workspace,
                              size_t workspace_bytes, void *stream);
int dvsg_tps_render_zoom_u8(const dvsg_locnet_t *net, const float *F_t, const uint8_t *src, int n, int src_H, int src_W,
                            int channel_flip, const float *zoom, float *T, float *out_f32, uint8_t *out_u8, int u8_W,
                            int u8_x0, void *stream);
int dvsg_tps_coefficients_f32(const dvsg_locnet_t *net, const float *F_t, int n, float *T, void *stream);
int dvsg_crop_ratchet_f32(const int32_t *key_min_a, int D_a, const int32_t *key_min_b, int D_b, const int32_t *state_slots,
                          int n, float *state, int n_state, double margin, double crop_min, double recover, float *zoom,
                          double *free_out, void *stream);
/* ---------------------------------------------------------------------------------------
 * eval_train.py's evaluation graph (eval_train.py:25-51): unlike model.py's, its CNN input is
 * `patches_masked_t = patches_t * mask` (:43-45), where `random_mask` (:53-64, = model.py:156-167) warps an all-ones
 * image of the 3 (S - 1) history channels (18 of 21 in the reference) with ProjectiveTransformer and a near-identity homography H and leaves the newest
 * frame's 3 channels unmasked; the TPS warp still samples the UNMASKED u_t (:48).
 *   dvsg_random_mask_plane_f32  theta [B,8] (the homography of :55-57 AFTER its scale and identity offset; the
 *          reference draws it with tf.random_uniform inside the graph, here the caller supplies it) -> mask [B,H,W]:
 *          ProjectiveTransformer(out_size).transform(ones, theta) -- grid (spatial_transformer.py:423-452) and
 *          sampler B's blend (:545-562) on taps that read 1 inside the image and 0 on the zero ring.  The warp of an
 *          all-ones image is the same in every channel, so ONE plane stands for `random_masks_t[..., :18]`.
 *   dvsg_stabilize_masked_f32 / dvsg_stabilize_ring_masked_{f32,u8}: dvsg_stabilize_* / dvsg_stabilize_ring_* with that
 *          plane multiplied into the 3 (S - 1) history channels INSIDE conv1's load stage ((x * m) * 255 - mean, three
 *          roundings like the TF ops); neither a [B,H,W,3S] product tensor nor a multiply launch exists.  A plane of
 *          exact ones reproduces the unmasked entry points bit for bit.  precision: DVSG_PRECISION_*.
 *   dvsg_locnet_forward_masked: the CNN alone (stage -1: F_t into `out`) or a parity tap (stage 0..18) from a masked
 *          source; src_kind 0 = window tensor [B,H,W,3S], 1 = float32 frame pool + table, 2 = uint8 frame pool + table.
 * ------------------------------------------------------------------------------------- */
int dvsg_random_mask_plane_f32(const float *theta, int B, int H, int W, float *mask, void *stream);
int dvsg_stabilize_masked_f32(const dvsg_locnet_t *net, int precision, const float *patches_t, const float *u_t,
                              const float *mask, int B, int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s,
                              void *workspace, size_t workspace_bytes, void *stream);
int dvsg_stabilize_ring_masked_f32(const dvsg_locnet_t *net, int precision, const float *pool, int n_pool,
                                   const int32_t *table, const float *mask, int B, int H, int W, float *s_t_pred, float *F_t,
                                   float *x_s, float *y_s, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_stabilize_ring_masked_u8(const dvsg_locnet_t *net, int precision, const uint8_t *pool, int n_pool,
                                  const int32_t *table, const float *mask, int B, int H, int W, float *s_t_pred, float *F_t,
                                  float *x_s, float *y_s, void *workspace, size_t workspace_bytes, void *stream);
int dvsg_locnet_forward_masked(const dvsg_locnet_t *net, int precision, const void *src, int src_kind, int n_pool,
                               const int32_t *table, const float *mask, int B, int H, int W, int stage, float *out,
                               size_t out_bytes, int *act_dims_host, void *workspace, size_t workspace_bytes, void *stream);
/* eval.py:112 `np.uint8(x * 255.)`: float64 product, truncation toward zero (values outside
 * [0, 256) saturate; NumPy leaves them undefined).  src [n,H,W,3] float32 is written into columns
 * [dst_x0, dst_x0 + W) of dst [n,H,dst_W,3] uint8 -- dst_W = 2 W and dst_x0 = 0 / W give the
 * reference's side-by-side layout, dst_W = W and dst_x0 = 0 a plain frame. */
int dvsg_frames_f32_to_u8(const float *src, int n, int H, int W, int channel_flip, uint8_t *dst, int dst_W,
                          int dst_x0, void *stream);
/* same for frames the caller holds as float64 (the dtype of eval.py's history list) */
int dvsg_frames_f64_to_u8(const double *src, int n, int H, int W, int channel_flip, uint8_t *dst, int dst_W,
                          int dst_x0, void *stream);

/* Second building block: conv2 (3x3, pad 1, stride 1 or 2, Cin -> 64, + bias + ReLU) and conv3 (1x1,
 * 64 -> Cout, + bias + residual + ReLU) of a block-1 bottleneck unit as one kernel; the [M,64]
 * intermediate never leaves the chip.  float32.  x [B,H,W,Cin] (Cin % 32 == 0, >= 64); wt2 [64][9*Cin]
 * (k order kh, kw, c); wt3 [Cout][64] (Cout % 128 == 0); res / y as in dvsg_conv_gemm_f32. */
int dvsg_conv3x3_1x1_f32(const float *x, const float *wt2, const float *bias2, const float *wt3, const float *bias3,
                         const float *res, float *y, int B, int H, int W, int Cin, int Cout, int stride, int res_stride,
                         void *stream);

/* Diagnostic A/B switches for kernel experiments, process-global; an unknown name is DVSG_ERR_INVALID_ARG.  The 18
 * names and their defaults: "conv_variant" 0, "conv1_variant" 0 (0 = the launch policy's own choice of kernel; in
 * float32, 6 = root_band_kernel -- row pairs in bands, one workgroup per CU -- at any size for unmasked sources, in bands of at
 * most 3 pairs, and 7 = the one-row conv1_kernel at any size: the two are equal bit for bit), "root_pool" 0 (float32, conv1's
 * output of even height and width and not tapped: the root max pool in the band kernel's epilogue, root_band_pool_kernel +
 * root_pool_seams_kernel, 0 = where the band kernel is the policy's own choice, 1 = never, 2 = wherever the band kernel
 * runs; equal to the separate max pool bit for bit), "fuse_conv" 1,
 * "fuse_shortcut" 1, "concat_sc" 1 (block 1's conv2 + conv3 in one kernel, its shortcut conv in that kernel too, the
 * shortcut + conv1 of blocks 2-4's opening units as one launch; 0 selects the separate launches), "x3_conv1" 1, "x3_fuse" 3
 * (the f32x3 precision's own conv1 kernel and block-1 fusion; 0 the float32 kernel / never fused), "f16_split" 1,
 * "f16_pair_mask" 0xFFFF (float16 mode: hi / lo weight pairs, and the layers that carry them), for the float16 mode's big
 * launches "wide16_min_tiles" (tiles from which the 256 x 128 geometry runs: 128), "wide16_packed" / "wide16_arows" /
 * "wide16_hreuse" / "fused_hreuse" (1: weight stages from the packed copy, 128-byte activation rows, a 3x3 kernel row's taps
 * from one staged run, the same in block 1's fused kernel; 0 selects the kernel each replaced), "flow_tiled" 1, "flow_rounds"
 * 4 (dvsg_flow_warp_f32 on RGB frames: column strips streamed through LDS, 0 = global gathers; rounds of resident workgroups
 * its bands aim at), "warp_xcd" 0 (0: the sampler kernels' workgroups in plain dispatch order).
 * Results do not depend on them beyond float32 re-association. */
int dvsg_debug_set_option(const char *name, int value);
/* What the last dvsg_conv_gemm_* call (or conv launch of a network call) ran, recorded on the host when it was launched; no
 * synchronisation.  fields (n >= 13): T (0: float32 tensors, 1: float16), BN (tile width 64 / 128), WM, WN (wave layout), KS
 * (1 / 3), RELU, RES (0 none, 1 full-size, 2 subsampled), MODE (0 plain, 1 split-K, 2 stream-K), SPLIT (f32s pieces / float16
 * hi-lo rows), X3 (f32x3), ksplit (slices per tile), streamk_tail (tiles shared as stream-K units), mt_fast (tile order).
 * T = -1: that call ran no conv_gemm_kernel (dvsg_debug_last_conv_kernel then names the kernel that ran), or none was made. */
int dvsg_debug_last_conv_config(int *fields, int n);
/* Which conv kernel the last dvsg_conv_gemm_* / fused call (or conv launch of a network call) ran, recorded on the host when
 * it was launched; no synchronisation.  fields (n >= 6): family (0 conv_gemm_kernel, 1 conv_wide16_kernel, 2
 * conv_wide16a_kernel, 3 conv_wide16h_kernel, 4 conv3x3_1x1_kernel, 5 conv3x3_1x1_x3_kernel, 6 conv3x3_1x1_f16_kernel, 7
 * conv3x3_1x1_f16h_kernel; -1 none), then the family's template arguments in declaration order padded with -1 to four
 * fields (family 0: all -1, see dvsg_debug_last_conv_config), then for families 1-3 where the weight stages came from (0 the
 * [rows][K] layout, 1 the packed copy), else -1. */
int dvsg_debug_last_conv_kernel(int *fields, int n);
/* Which root and head kernels the last network call (dvsg_locnet_forward_*, dvsg_stabilize_*, their ring / masked / tap
 * forms) ran, recorded on the host when they were launched; no synchronisation.  fields (n >= 9): conv1 family (0 conv1_kernel,
 * 1 conv1_f16_kernel, 2 conv1_f16_pair_kernel, 3 conv1_f16_march_kernel, 4 conv1_split_kernel, 5 conv1_x3_kernel, 6
 * rootconv_kernel: every launch of a handle whose c_in is not 21, recorded with NW = 4, 7 root_band_kernel: big unmasked
 * float32 launches, recorded with NW = 8 and TO = 0), its template
 * arguments NW, TO (0 float, 1 _Float16, 2 the float16 pieces of "f32s": family 6 only) and SRC (2 x source kind + rows on the 16-byte grid + 8 x masked), -1 where the family
 * has none; the marching kernel's bands and quads_per_band, or the band kernel's bands and the row pairs of its longest band
 * (else -1); the max pool kernel (0 maxpool_kernel<float>, 1
 * maxpool_kernel<_Float16>, 2 maxpool_h8_kernel, 3 maxpool_p_kernel); the average pool kernel (0 avgpool_partial_kernel<float>,
 * 1 avgpool_partial_kernel<_Float16>, 2 avgpool_partial_p_kernel); the number of dense batch chunks of <= 16 samples.  A
 * field is -1 when the call stopped (parity tap) before that launch, or none was made. */
int dvsg_debug_last_root_kernel(int *fields, int n);
/* Block 1's fused conv2 + conv3 (dvsg_conv3x3_1x1_f32) in any precision, as the network runs it.  prec: 0 float32 (weights
 * [rows][K]), 1 float16 (x, res, sc_x, y float16; weights the stacked [rows/64][128][K] hi / lo rows of dvsg_conv_gemm_f16s),
 * 2 f32s (x, res, sc_x, y in pieces; weights [rows][K/32][32 hi | 32 lo]), 3 f32x3 (float32 tensors; weights
 * dvsg_pack_weights_f32x3).  With sc_x non-NULL the residual is the 1x1 shortcut conv sc_x [B,Ho,Wo,sc_cin] x sc_wt
 * [Cout][sc_cin] + sc_bias, computed in the kernel, and res is ignored.  The option "fused_hreuse" selects the float16
 * kernel as in the network. */
int dvsg_debug_conv3x3_1x1(int prec, const void *x, const void *wt2, const float *bias2, const void *wt3, const float *bias3,
                           const void *res, const void *sc_x, const void *sc_wt, const float *sc_bias, int sc_cin, void *y,
                           int B, int H, int W, int Cin, int Cout, int stride, int res_stride, void *stream);
/* The A/B form of dvsg_locnet_calibrate_f16 (tools/f16_ef_sweep.py): re-rounds the plain float16 weight copies and leaves
 * the pair policy to "f16_pair_mask".  mode 0: round to nearest (what dvsg_locnet_create makes); 1: error feedback with
 * mu = 1 (measured: useless -- channel means are far from uniform); 2: calibrated channel means.  Synchronous like it, in
 * every mode: it waits for `stream` before it rewrites the weights. */
int dvsg_debug_calibrate_f16_weights(dvsg_locnet_t *net, const float *patches, int B, int H, int W, int mode, void *workspace,
                                     size_t workspace_bytes, void *stream);
/* What the last calibration of this handle re-rounded against (dvsg_locnet_calibrate_f16, dvsg_debug_calibrate_f16_weights),
 * copied to host memory: means [48][2048] float64, slot 3 u + {0: unit u's input (conv1, shortcut), 1: conv1's output
 * (conv2), 2: conv2's output (conv3)}, u = 0..15 in network order, and rows [48] float64, the pixels summed per slot.  They
 * are the values the weights were chosen by, kept in the handle, not a second measurement.  Channels past a slot's tensor
 * hold 0 and are never read.  A new handle, mode 0, patches == NULL and mode 1 leave every mean at the 1.0 the rule then
 * uses, and every row count at 0.  No device work. */
int dvsg_debug_calibration_means(const dvsg_locnet_t *net, double *means, double *rows);
/* The PLAIN float16 copy of one convolution's folded weights as the handle holds it now (what a float16 layer without the
 * hi / lo pair multiplies; its stage-packed copies are made from it): unit 0..15 in network order, kind 0 conv1, 1 conv2,
 * 2 conv3, 3 shortcut (DVSG_ERR_INVALID_ARG where the unit has none).  dims [3] receives cout, K = ksize^2 cin and cin;
 * w16 (host memory, [cout][K] float16, k = (kh, kw, c); w16_bytes its size) may be NULL to ask for dims alone.
 * Synchronous. */
int dvsg_debug_plain_weights_f16(const dvsg_locnet_t *net, int unit, int kind, void *w16, size_t w16_bytes, int *dims);

/* ---------------------------------------------------------------------------------------
 * Test-time losses: trainer.py:95-123 `build_loss_train` on get_train_model(is_train = False), the score
 * errs_total_test['total'] that ranks checkpoints (main.py:198-221).  Forward only; the `cor` term (correlationNet) is not
 * built.  Every per-pixel term is the TF graph's chain of separately rounded float32 ops on the bits dvsg_tps_warp_f32 /
 * dvsg_flow_warp_f32 give for that pixel; every sum is a float64 sum of those float32 terms in a fixed order (per thread,
 * wave shuffles, LDS across waves, one partial per workgroup in `workspace`, a second launch over the partials): no atomics,
 * bitwise reproducible.  Each entry writes the per-sample values per_sample [B] (tf.div_no_nan of the two sums rounded to
 * float32, trainer.py:242) and their batch mean mean [1] (trainer.py:243).  sums (optional) receives the float64 sums
 * themselves.  workspace: 8-byte aligned, dvsg_loss_workspace_bytes(B, H, W) bytes, private to the call until it has run.
 * ------------------------------------------------------------------------------------- */
int dvsg_loss_workspace_bytes(int B, int H, int W, size_t *bytes);

/* loss['image'] of one frame (trainer.py:100-101, 233-243; model.py:81-85): masked_MSE(pred, gt, mask) with
 * pred = ThinPlateSpline(U) and mask = ThinPlateSpline(ones), both from ONE evaluation of the map per pixel.  U, gt
 * [B,H,W,3]; coord [B,P,2]; T [B,2,P+3] (dvsg_tps_solve_f32).  The mask is one plane (the reference's three channels are
 * equal): sampler A's four weights, formed after the index clip, added in the blend's order.  pred [B,H,W,3] and mask
 * [B,H,W] are optional outputs, bit-identical to dvsg_tps_warp_f32 on U and on ones; sums [B][2] = {sum_c (pred m - gt m)^2,
 * sum_c m}. */
int dvsg_loss_image_f32(const float *U, const float *coord, const float *T, const float *gt, int B, int H, int W, int P,
                        float *pred, float *mask, float *per_sample, float *mean, double *sums, void *workspace,
                        size_t workspace_bytes, void *stream);

/* `temporal_loss` (trainer.py:245-250): masked_MSE(tf_warp(pred), gt, tf_warp(mask_pred) * mask_gt).  pred, gt [B,H,W,3];
 * mask_pred, mask_gt planes [B,H,W]; flow [B,H,W,2] in pixels, 8-byte aligned (a status otherwise).  Sampler C's taps and weights of a pixel are formed once and
 * blend the three channels and the mask plane; nothing warped is written (40 algorithmic bytes per pixel).  sums [B][2]. */
int dvsg_loss_temporal_f32(const float *pred, const float *mask_pred, const float *flow, const float *gt, const float *mask_gt,
                           int B, int H, int W, float *per_sample, float *mean, double *sums, void *workspace,
                           size_t workspace_bytes, void *stream);

/* `masked_MSE` (trainer.py:233-243).  pred, gt [B,H,W,C]; mask [B,H,W,C], or -- mask_is_plane != 0 -- [B,H,W] counted C
 * times.  C <= 64.  sums [B][2]. */
int dvsg_loss_masked_mse_f32(const float *pred, const float *gt, const float *mask, int B, int H, int W, int C,
                             int mask_is_plane, float *per_sample, float *mean, double *sums, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The two grid terms of one frame.  identity (trainer.py:105-106): mean |F| over [P,2].  `distortion_loss`
 * (trainer.py:252-323) exactly as written: V_src mapped to [0,1], the four get_sp_term triangles, M_rot = [[0,1],[-1,0]];
 * two of the four pair a triangle with the other rotation sense, so the value at F = 0 on the 5 x 5 grid is 0.125, not 0.
 * V_src, F [B,P,2], P = num_control_points^2, 2 <= num_control_points <= 7.  identity, distortion [B]; the means [1]. */
int dvsg_loss_grid_f32(const float *V_src, const float *F, int B, int num_control_points, float *identity, float *identity_mean,
                       float *distortion, float *distortion_mean, void *stream);

/* `get_surf_loss` (trainer.py:363-386) without x_offset / y_offset: the TPS map (coord, T as above, grid H x W) is evaluated
 * at the N flat indices idx = int(x + y W) of surf[:,1] only, to the bits dvsg_tps_warp_f32 writes to x_s / y_s there;
 * idx == H W reads the appended -1 (:364-365), an index outside [0, H W] is clamped into it.  surf [B,2,N,2] float32 pixel
 * positions ([:,0] unstable, [:,1] stable); surfs_dim [B] float32, the divisor (:384).  All N points count, padded ones
 * included.  coords [B,N,2] (optional): the gathered (x, y).  sums [B]: the float64 sum of squared differences. */
int dvsg_loss_surf_f32(const float *surf, const float *surfs_dim, const float *coord, const float *T, int B, int N, int H, int W,
                       int P, float *coords, float *per_sample, float *mean, double *sums, void *stream);

/* ---------------------------------------------------------------------------------------
 * Measurement hook (bench.py's roofline leg; not part of the reference surface).  While
 * armed for one kernel class, every launch of that class made by this library is bracketed
 * by a hipEvent pair on the launch stream.  dvsg_prof_end synchronises on those events and
 * returns the summed durations, the launch count and the algorithmic FLOPs / bytes of those
 * launches.  Classes: 0 conv1 (7x7/2 + scale_RGB), 1 conv 3x3, 2 conv 1x1, 3 max pool,
 * 4 head (avg pool + dense), 5 TPS solve, 6 TPS grid + sampler A, 7 flow / STN samplers,
 * 8 block 1's fused conv2 + conv3.
 * Process-global and not thread-safe: arm it only around single-threaded benchmark code.
 * ------------------------------------------------------------------------------------- */
/* 1 if DVSG_ROCTX=1 was set when the library first looked and a roctx library could be loaded: every stage of the
 * evaluation graph (dvsg/conv1, dvsg/pool1, dvsg/block<b>/unit_<u>, dvsg/head, dvsg/tps) then opens a roctx range
 * around its launches, for `rocprofv3 --kernel-trace --marker-trace` (tracing). */
int dvsg_markers_enabled(void);
int dvsg_prof_begin(int kernel_class);
int dvsg_prof_end(double *total_ms, int *launches, double *flops, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* DVSG_AMD_H */
