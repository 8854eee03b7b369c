// The pixel decomposition and tap masks of the rows this lane stages in conv_wide16_kernel and conv_wide16a_kernel
// (conv_gemm_wide16.hip), included in both.  The including kernel declares, besides its parameters and indices,
// `constexpr int kRows` -- the rows an LDS-DMA instruction writes, this lane row `lrow` of them at chunk position `lpos` --
// and `swz(row)`, the chunk swizzle of a row: position lpos receives global chunk lpos ^ swz(row).
  long a_off[AG];        // element offset of the pixel's (kh = 0, kw = 0, c = chunk) tap
  unsigned a_mask[AG];   // bit kh: input row valid, bit 4 + kw: input column valid
  const bool dense = KS == 1 && p.stride == 1;   // a 1x1 / stride 1 layer is a row-major GEMM (conv_gemm.hip)
#pragma unroll
  for (int i = 0; i < AG; ++i) {
    const int row = kRows * (wave + NW * i) + lrow;
    const int chunk = lpos ^ swz(row);
    const int m = m0 + row;
    const int mm = m < p.M ? m : 0;
    if (dense) {
      a_off[i] = (long)mm * p.Cin + 8 * chunk;
      a_mask[i] = m < p.M ? 0x11u : 0u;
      continue;
    }
    const Pixel px = pixel_of(mm, p.Ho, p.Wo);
    const int hi0 = px.ho * p.stride - p.pad, wi0 = px.wo * p.stride - p.pad;
    a_off[i] = (((long)px.b * p.H + hi0) * p.W + wi0) * p.Cin + 8 * chunk;
    unsigned mk = 0;
    if (m < p.M) {
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        if (hi0 + q >= 0 && hi0 + q < p.H) mk |= 1u << q;
        if (wi0 + q >= 0 && wi0 + q < p.W) mk |= 16u << q;
      }
    }
    a_mask[i] = mk;
  }
