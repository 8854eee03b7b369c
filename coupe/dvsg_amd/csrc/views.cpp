// The views of a network handle and the entry points that read a handle's render properties (host only, no kernel): the
// table of scaled views, the six view constructors and their getters, dvsg_locnet_destroy, the four source-size renders,
// dvsg_tps_coefficients_f32 and dvsg_tps_coverage_net_f32.  A handle's properties are one RenderView (common.h); a new one is
// a member there, a line in check_view, a constructor and a getter here.
#include <mutex>
#include <unordered_map>
#include <utility>

#include "locnet_internal.h"

using namespace dvsg;

// The views that carry an output size other than (0, 0), by address.  dvsg_tps_render_nv12 / _zoom_nv12 check every argument
// before they read the handle (a caller's garbage pointer with a bad pitch is refused, not followed), and what the output
// planes must hold depends on the view's size: looking the POINTER up here tells them without reading through it.  Any
// other pointer has (0, 0), the source's size.
// INVARIANT: the table and the handles' out_h / out_w always agree.  make_view is the one place that writes either, once
// per view and before the constructor hands the view out; a view's fields never change afterwards; dvsg_locnet_destroy
// erases the entry before it frees the view.  So a live view v has g_scaled_views[v] == (v->view.out_h, v->view.out_w) if that
// is not (0, 0) and no entry otherwise, and the RGB renders (which read the fields) and the NV12 renders (which read the table)
// see one size.  g_n_scaled counts the entries: while no scaled view exists a render takes no lock.
static std::mutex g_scaled_mutex;
static std::unordered_map<const dvsg_locnet *, std::pair<int, int>> g_scaled_views;
static std::atomic<int> g_n_scaled{0};

static void scaled_view_size(const dvsg_locnet *net, int *out_h, int *out_w) {
  *out_h = *out_w = 0;
  if (g_n_scaled.load(std::memory_order_acquire) == 0) return;
  std::lock_guard<std::mutex> lock(g_scaled_mutex);
  const auto it = g_scaled_views.find(net);
  *out_h = it == g_scaled_views.end() ? 0 : it->second.first;
  *out_w = it == g_scaled_views.end() ? 0 : it->second.second;
}

// every field of a view, from its values alone; fn: the constructor its messages name
static int check_view(const char *fn, const RenderView &rv) {
  DVSG_REQUIRE(rv.filter == DVSG_RENDER_BILINEAR || rv.filter == DVSG_RENDER_BICUBIC,
               "%s: render_filter=%d is neither DVSG_RENDER_BILINEAR (0) nor DVSG_RENDER_BICUBIC (1)", fn, rv.filter);
  DVSG_REQUIRE(rv.border >= DVSG_BORDER_BLACK && rv.border <= DVSG_BORDER_KEEP,
               "%s: render_border=%d is none of DVSG_BORDER_BLACK (0), _REPLICATE (1), _MIRROR (2), _KEEP (3)", fn, rv.border);
  DVSG_REQUIRE(rv.shape.model >= DVSG_SHAPE_AFFINE && rv.shape.model <= DVSG_SHAPE_TRANSLATION,
               "%s: shape_model=%d is none of DVSG_SHAPE_AFFINE (0), _SIMILARITY (1), _TRANSLATION (2)", fn, rv.shape.model);
  DVSG_REQUIRE(rv.shape.strength >= 0.0f && rv.shape.strength <= 1.0f, "%s: strength=%g outside [0, 1]", fn,
               (double)rv.shape.strength);
  DVSG_REQUIRE(rv.shape.rigidity >= 0.0f && rv.shape.rigidity <= 1.0f, "%s: rigidity=%g outside [0, 1]", fn,
               (double)rv.shape.rigidity);
  DVSG_REQUIRE(rv.surface_format == DVSG_SURFACE_NV12 || rv.surface_format == DVSG_SURFACE_P010,
               "%s: surface_format=%d is neither DVSG_SURFACE_NV12 (0) nor DVSG_SURFACE_P010 (1)", fn, rv.surface_format);
  DVSG_REQUIRE(rv.chroma_format == DVSG_CHROMA_420 || rv.chroma_format == DVSG_CHROMA_422,
               "%s: chroma_format=%d is neither DVSG_CHROMA_420 (0) nor DVSG_CHROMA_422 (1)", fn, rv.chroma_format);
  if (!(rv.out_h == 0 && rv.out_w == 0)) {
    DVSG_REQUIRE(rv.out_h >= 1, "%s: out_H=%d (with out_W=%d) is neither >= 1 nor, together with out_W, 0", fn, rv.out_h, rv.out_w);
    DVSG_REQUIRE(rv.out_w >= 1, "%s: out_W=%d (with out_H=%d) is neither >= 1 nor, together with out_H, 0", fn, rv.out_w, rv.out_h);
  }
  return DVSG_OK;
}

// The one place that makes a view: a view of net's parent (a view of a view is a view of the parent) that carries `rv` whole.
// Everything is decided before anything is allocated; a size is registered in the table before the view is handed out.
static int make_view(const char *fn, const dvsg_locnet_t *net, const RenderView &rv, dvsg_locnet_t **view) {
  if (int rc = check_view(fn, rv)) return rc;
  dvsg_locnet *v = new dvsg_locnet();
  v->calib_mu = std::vector<double>();   // (a view keeps no calibration record of its own)
  v->parent = base(net);
  v->view = rv;
  v->parent->n_views.fetch_add(1);
  if (rv.out_h || rv.out_w) {
    std::lock_guard<std::mutex> lock(g_scaled_mutex);
    g_scaled_views[v] = std::make_pair(rv.out_h, rv.out_w);
    g_n_scaled.store((int)g_scaled_views.size(), std::memory_order_release);
  }
  *view = v;
  return DVSG_OK;
}

// The constructors by value: filter, border and shape are the arguments', everything else a plain handle's (on a view they
// inherit nothing).  make_view checks the values before it reads the handle.
static int view_by_value(const char *fn, const dvsg_locnet_t *net, dvsg_locnet_t **view, int filter, int border,
                         RenderShape shape = RenderShape()) {
  DVSG_REQUIRE(net, "%s: NULL net", fn);
  DVSG_REQUIRE(view, "%s: NULL view", fn);
  *view = nullptr;
  RenderView rv;
  rv.filter = filter;
  rv.border = border;
  rv.shape = shape;
  return make_view(fn, net, rv, view);
}

// The inheriting constructors: net's OWN view with the one property that `set` writes replaced.  The argument is checked
// alone first, in a default view: the handle is read after that.
template <typename Set>
static int view_inheriting(const char *fn, const dvsg_locnet_t *net, dvsg_locnet_t **view, Set set) {
  DVSG_REQUIRE(net, "%s: NULL net", fn);
  DVSG_REQUIRE(view, "%s: NULL view", fn);
  *view = nullptr;
  RenderView rv;
  set(rv);
  if (int rc = check_view(fn, rv)) return rc;
  rv = net->view;
  set(rv);
  return make_view(fn, net, rv, view);
}

// the two NV12 renders; fn: the one its messages name.  Every argument is checked before the handle is read; a P010 view's
// further checks follow, before any device work.
static int render_nv12(const char *fn, const dvsg_locnet_t *net, const float *F_t, const float *zoom, const uint8_t *y,
                       const uint8_t *uv, size_t pitch, size_t frame_stride, int n, int H, int W, float *T, uint8_t *out_y,
                       uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, void *stream) {
  DVSG_REQUIRE(net, "%s: NULL net", fn);
  int oh = 0, ow = 0;
  scaled_view_size(net, &oh, &ow);   // by the pointer's value: the handle itself is not read yet
  if (int rc = tps_render_nv12_check(fn, F_t, y, uv, pitch, frame_stride, n, H, W, T, out_y, out_uv, out_pitch, out_frame_stride,
                                     oh, ow))
    return rc;
  const RenderView &rv = net->view;   // the first read of the handle; its size is the table's (the invariant above)
  if (rv.surface_format == DVSG_SURFACE_P010)
    if (int rc = tps_render_p010_check(fn, y, uv, pitch, frame_stride, n, W, out_y, out_uv, out_pitch, out_frame_stride, ow))
      return rc;
  return tps_render_nv12_impl(fn, base(net)->winv, base(net)->v_src, F_t, zoom, y, uv, pitch, frame_stride, n, H, W, 25, T, out_y,
                              out_uv, out_pitch, out_frame_stride, stream, rv);
}

// the two RGB renders
static int render_u8(const char *fn, const dvsg_locnet_t *net, const float *F_t, const float *zoom, const uint8_t *src, int n,
                     int src_H, int src_W, int channel_flip, float *T, float *out_f32, uint8_t *out_u8, int u8_W, int u8_x0,
                     void *stream) {
  DVSG_REQUIRE(net, "%s: NULL net", fn);
  return tps_render_impl(base(net)->winv, base(net)->v_src, F_t, zoom, src, n, src_H, src_W, 25, channel_flip, T, out_f32, out_u8,
                         u8_W, u8_x0, stream, net->view);
}

extern "C" {

int dvsg_locnet_destroy(dvsg_locnet_t *net) {
  if (!net) return DVSG_OK;
  if (net->parent) {   // a view owns nothing
    net->parent->n_views.fetch_sub(1);
    if (net->view.out_h || net->view.out_w) {
      std::lock_guard<std::mutex> lock(g_scaled_mutex);
      g_scaled_views.erase(net);
      g_n_scaled.store((int)g_scaled_views.size(), std::memory_order_release);
    }
    delete net;
    return DVSG_OK;
  }
  const int views = net->n_views.load();
  DVSG_REQUIRE(views == 0, "dvsg_locnet_destroy: the handle still has %d view(s); destroy them first", views);
  for (void *p : net->allocs) (void)hipFree(p);
  delete net;
  return DVSG_OK;
}

int dvsg_locnet_view_create(const dvsg_locnet_t *net, int render_filter, dvsg_locnet_t **view) {
  return view_by_value("dvsg_locnet_view_create", net, view, render_filter, DVSG_BORDER_BLACK);
}

int dvsg_locnet_view_create_border(const dvsg_locnet_t *net, int render_filter, int render_border, dvsg_locnet_t **view) {
  return view_by_value("dvsg_locnet_view_create_border", net, view, render_filter, render_border);
}

int dvsg_locnet_view_create_shaped(const dvsg_locnet_t *net, int render_filter, int render_border, int shape_model,
                                   float strength, float rigidity, dvsg_locnet_t **view) {
  RenderShape shape;
  shape.model = shape_model;
  shape.strength = strength;
  shape.rigidity = rigidity;
  return view_by_value("dvsg_locnet_view_create_shaped", net, view, render_filter, render_border, shape);
}

int dvsg_locnet_view_create_surface(const dvsg_locnet_t *net, int surface_format, dvsg_locnet_t **view) {
  return view_inheriting("dvsg_locnet_view_create_surface", net, view, [=](RenderView &rv) { rv.surface_format = surface_format; });
}

// ("Output size" in the header)
int dvsg_locnet_view_create_scaled(const dvsg_locnet_t *net, int out_H, int out_W, dvsg_locnet_t **view) {
  return view_inheriting("dvsg_locnet_view_create_scaled", net, view, [=](RenderView &rv) { rv.out_h = out_H, rv.out_w = out_W; });
}

// ("Chroma sampling")
int dvsg_locnet_view_create_chroma(const dvsg_locnet_t *net, int chroma_format, dvsg_locnet_t **view) {
  return view_inheriting("dvsg_locnet_view_create_chroma", net, view, [=](RenderView &rv) { rv.chroma_format = chroma_format; });
}

// the getters; a NULL handle has a plain handle's values
static RenderView view_of(const dvsg_locnet_t *net) { return net ? net->view : RenderView(); }

int dvsg_locnet_render_filter(const dvsg_locnet_t *net) { return view_of(net).filter; }

int dvsg_locnet_render_border(const dvsg_locnet_t *net) { return view_of(net).border; }

int dvsg_locnet_render_shape(const dvsg_locnet_t *net, int *shape_model, float *strength, float *rigidity) {
  const RenderShape shape = view_of(net).shape;
  if (shape_model) *shape_model = shape.model;
  if (strength) *strength = shape.strength;
  if (rigidity) *rigidity = shape.rigidity;
  return DVSG_OK;
}

int dvsg_locnet_render_surface(const dvsg_locnet_t *net) { return view_of(net).surface_format; }

int dvsg_locnet_render_chroma(const dvsg_locnet_t *net) { return view_of(net).chroma_format; }

int dvsg_locnet_render_size(const dvsg_locnet_t *net, int *out_H, int *out_W) {
  if (out_H) *out_H = view_of(net).out_h;
  if (out_W) *out_W = view_of(net).out_w;
  return DVSG_OK;
}

// Source-resolution render of an online step: the T of dvsg_stabilize_* for F_t (tps_apply_kernel on the handle's W^-1
// columns and V_src, bit for bit), then the uint8 source frames warped by it at their own size.
int dvsg_tps_render_u8(const dvsg_locnet_t *net, const float *F_t, const uint8_t *src, int n, int src_H, int src_W,
                       int channel_flip, float *T, float *out_f32, uint8_t *out_u8, int u8_W, int u8_x0, void *stream) {
  return render_u8("dvsg_tps_render_u8", net, F_t, nullptr, src, n, src_H, src_W, channel_flip, T, out_f32, out_u8, u8_W, u8_x0,
                   stream);
}

// dvsg_tps_render_u8 on the output grid scaled about its centre by zoom[i] (NULL: dvsg_tps_render_u8 itself)
int dvsg_tps_render_zoom_u8(const dvsg_locnet_t *net, const float *F_t, const uint8_t *src, int n, int src_H, int src_W,
                            int channel_flip, const float *zoom, float *T, float *out_f32, uint8_t *out_u8, int u8_W,
                            int u8_x0, void *stream) {
  return render_u8("dvsg_tps_render_zoom_u8", net, F_t, zoom, src, n, src_H, src_W, channel_flip, T, out_f32, out_u8, u8_W, u8_x0,
                   stream);
}

// dvsg_tps_render_u8 for NV12 frames (nv12.hip): the same T, then both planes warped at their own sizes in one launch.
int dvsg_tps_render_nv12(const dvsg_locnet_t *net, const float *F_t, const uint8_t *y, const uint8_t *uv, size_t pitch,
                         size_t frame_stride, int n, int H, int W, float *T, uint8_t *out_y, uint8_t *out_uv, size_t out_pitch,
                         size_t out_frame_stride, void *stream) {
  return render_nv12("dvsg_tps_render_nv12", net, F_t, nullptr, y, uv, pitch, frame_stride, n, H, W, T, out_y, out_uv, out_pitch,
                     out_frame_stride, stream);
}

// dvsg_tps_render_nv12 on the output grid scaled about its centre by zoom[i] (NULL: dvsg_tps_render_nv12 itself)
int dvsg_tps_render_zoom_nv12(const dvsg_locnet_t *net, const float *F_t, const uint8_t *y, const uint8_t *uv, size_t pitch,
                              size_t frame_stride, int n, int H, int W, const float *zoom, float *T, uint8_t *out_y,
                              uint8_t *out_uv, size_t out_pitch, size_t out_frame_stride, void *stream) {
  return render_nv12("dvsg_tps_render_zoom_nv12", net, F_t, zoom, y, uv, pitch, frame_stride, n, H, W, T, out_y, out_uv, out_pitch,
                     out_frame_stride, stream);
}

// T alone, as dvsg_tps_render_u8 writes it: for a zoomed warp of frames that need no scan first (a fixed crop)
int dvsg_tps_coefficients_f32(const dvsg_locnet_t *net, const float *F_t, int n, float *T, void *stream) {
  DVSG_REQUIRE(net && F_t && T, "dvsg_tps_coefficients_f32: NULL pointer");
  DVSG_REQUIRE(n >= 1, "dvsg_tps_coefficients_f32: n=%d must be >= 1", n);
  const RenderShape shape = net->view.shape;   // the handle's own; the network is the parent's
  net = base(net);
  return tps_apply_impl(net->winv, net->v_src, F_t, 1, n, 25, T, stream, shape);
}

// The coverage scan of a clip's F_t rows: the T of dvsg_stabilize_* / dvsg_tps_render_u8 for F_t (written), then
// dvsg_tps_coverage_f32 on it with V_src.  Shapes and workspace are checked before the first launch.
int dvsg_tps_coverage_net_f32(const dvsg_locnet_t *net, const float *F_t, const float *zoom, int n, int src_H, int src_W,
                              int out_h, int out_w, float *T, int32_t *n_border, int32_t *key_min, void *workspace,
                              size_t workspace_bytes, void *stream) {
  const char *fn = "dvsg_tps_coverage_net_f32";
  DVSG_REQUIRE(net && F_t && T && n_border && key_min, "%s: NULL pointer", fn);
  size_t need = 0;
  if (int rc = dvsg_tps_coverage_workspace_bytes(n, out_h, out_w, &need)) return rc;
  DVSG_REQUIRE(src_H >= 1 && src_W >= 1, "%s: source size %dx%d must be positive", fn, src_H, src_W);
  DVSG_REQUIRE(workspace, "%s: NULL workspace", fn);
  if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0 || workspace_bytes < need)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed, 8-byte aligned (dvsg_tps_coverage_workspace_bytes)",
                fn, workspace_bytes, need);
  const RenderShape shape = net->view.shape;   // the scan counts the border the shaped render draws
  net = base(net);
  if (int rc = tps_apply_impl(net->winv, net->v_src, F_t, 1, n, 25, T, stream, shape)) return rc;
  return tps_coverage_impl(fn, net->v_src, 0, T, zoom, n, 25, src_H, src_W, out_h, out_w, n_border, key_min, workspace,
                           workspace_bytes, stream);
}

}  // extern "C"
