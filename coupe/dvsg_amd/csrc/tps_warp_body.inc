// The body of tps_warp_kernel and tps_warp_zoom_kernel (warp_kernels.hip), included inside both.  The including kernel
// declares the parameters documented there, `constexpr bool kZoom` and `constexpr bool kCubic`; names it has no parameter for
// (zoom; u_index, u_stride, n_pool, out_index) it declares as constants.  kCubic (tps_render_cubic_kernel: uint8 RGB in,
// the uint8 output form) swaps what follows the map -- sampler A's four taps -- for the bicubic filter of warp_device.h; the
// map, the thread layout and the output addresses are this one text's.  `constexpr int kBorder` (tps_render_border_kernel,
// the same uint8 form): what an invalid sample becomes (warp_device.h, "border modes"); DVSG_BORDER_BLACK drops every
// border statement.
  constexpr bool kU8Out = std::is_same<TO, uint8_t>::value;
  static_assert(!kU8Out || (C == 3 && std::is_same<TU, uint8_t>::value), "the uint8 output form reads uint8 RGB frames");
  __shared__ float4 sp[64];      // {px, py, T[0][3+k], T[1][3+k]}
  __shared__ float4 sdy[64];     // (y_t[r] - py)^2 for the 4 rows of this workgroup
  __shared__ float sa[6];        // T[0][0..2], T[1][0..2]
  const int b = blockIdx.z;
  const int n = P + 3;
  const int t = threadIdx.x;
  const int i0 = blockIdx.y * kTpsRows;
  float z = 1.0f;
  if constexpr (kZoom) z = zoom[b];
  if (t < P) {
    const float px = coord[b * coord_bstride + t * 2], py = coord[b * coord_bstride + t * 2 + 1];
    sp[t] = make_float4(px, py, T[((size_t)b * 2) * n + 3 + t] * kLn2, T[((size_t)b * 2 + 1) * n + 3 + t] * kLn2);
    float dy2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float y_t = -1.0f + step_y * (float)(i0 + r);
      if constexpr (kZoom) y_t = z * y_t;
      const float dy = y_t - py;  // :96
      dy2[r] = dy * dy;
    }
    sdy[t] = make_float4(dy2[0], dy2[1], dy2[2], dy2[3]);
  } else if (t >= 64 && t < 70) {
    const int q = t - 64;
    sa[q] = T[((size_t)b * 2 + q / 3) * n + q % 3];
  }
  __syncthreads();
  const int j = blockIdx.x * kThreads + t;
  if (j >= out_w) return;
  float x_t = -1.0f + step_x * (float)j;  // tf.linspace: start + step * i (:94)
  if constexpr (kZoom) x_t = z * x_t;
  int frame = b;
  bool frame_ok = true;
  if (u_index) {
    frame = u_index[(size_t)b * u_stride];
    frame_ok = frame >= 0 && frame < n_pool;
    if (!frame_ok) frame = 0;
  }
  const TU *img = U ? U + (size_t)frame * H * W * Cn : nullptr;
  size_t out_frame = b;
  if (out_index) {
    const int o = out_index[b];
    if (o < 0 || o >= n_pool) out = nullptr;
    out_frame = (size_t)o;
  }

  floatx2 xs2[2], ys2[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // T . [1, x_t, y_t, ...] accumulated in k order (:129)
    floatx2 yy = {-1.0f + step_y * (float)(i0 + 2 * h), -1.0f + step_y * (float)(i0 + 2 * h + 1)};
    if constexpr (kZoom) yy = z * yy;
    const float ax = sa[0] + sa[1] * x_t, ay = sa[3] + sa[4] * x_t;
    xs2[h] = floatx2{ax, ax} + sa[2] * yy;
    ys2[h] = floatx2{ay, ay} + sa[5] * yy;
  }
  for (int k = 0; k < P; ++k) tps_basis_point(sp[k], sdy[k], x_t, xs2, ys2);
  const float xs[4] = {xs2[0].x, xs2[0].y, xs2[1].x, xs2[1].y};
  const float ys[4] = {ys2[0].x, ys2[0].y, ys2[1].x, ys2[1].y};
  if constexpr (kCubic) {
    if (!out && !out_rgb) return;
    CubicTaps<3> ct[4];
    cubic_load_rows<3, kBorder>(img, (size_t)W * 3, H, W, out_h - i0, xs, ys, ct);  // all 16 row loads in flight
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + r;
      if (i >= out_h) break;
      if constexpr (kBorder == DVSG_BORDER_KEEP) {
        if (!ct[r].valid) continue;   // the caller's bytes stay
      }
      float v[3];
      cubic_blend<3, false, kBorder>(ct[r], v);
      if (out_rgb) {
        const float rgb[3] = {v[flip ? 2 : 0], v[1], v[flip ? 0 : 2]};
        store_pix<3>(out_rgb, (out_frame * out_h + i) * out_w + j, 3, rgb);
      }
      if (out) {
        uint8_t *d = out + ((out_frame * out_h + i) * out_row + out_x0 + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = cubic_u8(v[c], 0.5);
      }
    }
    return;
  }
  if constexpr (kBorder != DVSG_BORDER_BLACK) {   // sampler A's blend of the taps the border mode picks
    if (!out && !out_rgb) return;
    TapsA<3> taps[4];
    bool use[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (i0 + r >= out_h) break;
      border_a_load<3, false, kBorder>(img, (size_t)W * 3, H, W, xs[r], ys[r], taps[r], use[r]);  // all 16 tap loads in flight
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + r;
      if (i >= out_h) break;
      if constexpr (kBorder == DVSG_BORDER_KEEP) {
        if (!use[r]) continue;   // the caller's bytes stay
      }
      float v[3];
      sample_a_blend<3>(taps[r], 3, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = use[r] ? v[c] : 0.0f;
      if (out_rgb) {
        const float rgb[3] = {v[flip ? 2 : 0], v[1], v[flip ? 0 : 2]};
        store_pix<3>(out_rgb, (out_frame * out_h + i) * out_w + j, 3, rgb);
      }
      if (out) {
        uint8_t *d = out + ((out_frame * out_h + i) * out_row + out_x0 + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = to_u8((double)v[c]);
      }
    }
    return;
  }
  TapsA<C> taps[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + r;
    if (i >= out_h) break;
    const size_t pix = ((size_t)b * out_h + i) * out_w + j;
    if (xs_out) xs_out[pix] = xs[r];
    if (ys_out) ys_out[pix] = ys[r];
    if (img) sample_a_load<C, TU>(img, H, W, Cn, xs[r], ys[r], taps[r]);  // all 16 tap loads in flight
  }
  if constexpr (kU8Out) {
    if (!img || (!out && !out_rgb)) return;
  } else {
    if (!img || !out) return;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + r;
    if (i >= out_h) break;
    float v[C > 0 ? C : kMaxGenericC];
    sample_a_blend<C>(taps[r], Cn, v);
    if constexpr (C > 0) {
      if (!frame_ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.f;
      }
    }
    if constexpr (kU8Out) {
      if (out_rgb) {
        const float rgb[3] = {v[flip ? 2 : 0], v[1], v[flip ? 0 : 2]};
        store_pix<3>(out_rgb, (out_frame * out_h + i) * out_w + j, 3, rgb);
      }
      if (out) {
        uint8_t *d = out + ((out_frame * out_h + i) * out_row + out_x0 + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = to_u8((double)v[c]);
      }
    } else {
      store_pix<C>(out, (out_frame * out_h + i) * out_w + j, Cn, v);
    }
  }
