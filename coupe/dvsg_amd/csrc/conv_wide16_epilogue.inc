// The epilogue of conv_wide16_kernel, conv_wide16a_kernel and conv_wide16h_kernel (conv_gemm_wide16.hip), included at the
// end of each: 64 output channels at a time, rounds of 128 pixels through a [128][64] float32 transpose in the (idle) stage
// buffers (SPLIT: one channel half, hi + 2^-11 lo; plain: two channel halves, the accumulators as they are), then bias
// (+ residual) (+ ReLU) and 8-byte float16 stores.  LDS row i of the tile is pixel m0 + i.  The including kernel declares,
// besides its parameters and indices, `constexpr bool kHalo` -- true in conv_wide16h_kernel: rows 0 and WBM - 1 are only ever
// neighbours, rows 1 .. WHM are stored and m0 may be -1 -- and `stamp`, called at the four stamp points of the diagnostic
// build (NoStamps anywhere else).
  constexpr float kLoScale = 1.0f / 2048.0f;
  float *Cs = reinterpret_cast<float *>(lds);
  const int col4 = tid & 15, row0 = tid >> 4;   // 16 float4 per row, 32 rows per pass
  constexpr int NHALF = SPLIT ? 1 : 2;
#pragma unroll
  for (int ch = 0; ch < NHALF; ++ch) {
  const int n = nt * (SPLIT ? 64 : 128) + 64 * ch + 4 * col4;
  const float4 bias4 = *reinterpret_cast<const float4 *>(p.bias + n);
#pragma unroll
  for (int rho = 0; rho < 2; ++rho) {
    float4 rv[4];
    if (RES != 0) {   // residual of this round's rows: in flight under the two barriers and the transpose
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mr = m0 + 128 * rho + row0 + 32 * i;
        const int m = kHalo && mr < 0 ? 0 : (mr < p.M ? mr : p.M - 1);
        const size_t roff = (RES == 1 ? (size_t)m * p.Cout : subsample_offset(p, m, p.Cout)) + n;
        rv[i] = load4(p.res + roff);
      }
    }
    stamp(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // the stage buffers (first round) / the previous round's rows have been read
    asm volatile("" ::: "memory");
    stamp(1);
    if ((wm >> 1) == rho) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int q = 0; q < 16; ++q)
          Cs[((wm & 1) * 64 + mi * 32 + (q & 3) + 8 * (q >> 2) + 4 * h) * 64 + wn * 32 + r] =
              SPLIT ? acc_hi[mi][q] + acc_lo[mi][q] * kLoScale : (ch == 0 ? acc_hi[mi][q] : acc_lo[mi][q]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stamp(2);
    stamp(3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 32 * i;
      const int pr = 128 * rho + row;
      const int m = m0 + pr;
      if ((!kHalo || (pr >= 1 && pr <= WHM)) && m < p.M) {
        float4 v = *reinterpret_cast<const float4 *>(Cs + row * 64 + 4 * col4);
        v.x += bias4.x; v.y += bias4.y; v.z += bias4.z; v.w += bias4.w;
        if (RES != 0) {
          v.x += rv[i].x; v.y += rv[i].y; v.z += rv[i].z; v.w += rv[i].w;
        }
        if (RELU) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        store4(p.y + (size_t)m * p.Cout + n, v);
      }
    }
  }
  }
