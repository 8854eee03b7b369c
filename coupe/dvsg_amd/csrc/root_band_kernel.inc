// The text of root_band_kernel and root_band_pool_kernel (conv1_f32.hip includes it once for each, and describes both).
// RB_KERNEL is the kernel's name, RB_POOL 0 or 1: with 1 the pair's epilogue forms the root max pool's row instead of storing
// the two conv rows, and the kernel takes the pooled tensor behind `y`.  One text, not a function the two kernels call:
// inlined from a shared __device__ function the plain kernel's register allocation moved in four of its six instantiations,
// and as a second template argument the pool would change the names the launch records and the tests know the kernels by.
template <int SRC>
__global__ __launch_bounds__(RB_NT) __attribute__((amdgpu_waves_per_eu(2, 2)))
void RB_KERNEL(const Conv1Src src, const float *__restrict__ wt1, const float *__restrict__ bias,
#if RB_POOL
               float *__restrict__ y, float *__restrict__ pooled, int H, int W, int Ho, int Wo, int wtiles, int bands, int ppb, int nbig) {
#else
               float *__restrict__ y, int H, int W, int Ho, int Wo, int wtiles, int bands, int ppb, int nbig) {
#endif
  constexpr int NT = RB_NT, MI = 2;
  static_assert(C1_TILE * C1_LDC <= C1_WELEMS, "epilogue tile must fit in a weight buffer");
  extern __shared__ __attribute__((aligned(16))) float rb_lds[];
  float *const w_s = rb_lds;                      // [2][C1_WELEMS]
  float *const in_s = rb_lds + 2 * C1_WELEMS;     // [RB_SLOTS][C1_SEG_PAD]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  const Conv1Tile tile = conv1_tile(wtiles, bands);
  const int b = tile.b, band = tile.ho, wo0 = tile.wo0;
  const int pairs = (Ho + 1) / 2;
  const int p0 = band * ppb - (band > nbig ? band - nbig : 0);
  const int p1 = min(p0 + (band < nbig ? ppb : ppb - 1), pairs);
  if (p0 >= p1) return;

#ifdef DVSG_STAMPS
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long t_begin = C1_STAMP(), r_begin = __builtin_amdgcn_s_memrealtime();
#endif
  typedef typename Conv1RowSel<NT, RB_IN4, SRC>::type Row;
  Row row;
  row.init(src, tid, b, wo0, H, W, C1_SEG_PAD);
  if constexpr (Row::kRing) {   // elements the scatter never writes (the zero tap's slot, the tail) must be finite
    for (int e = tid; e < RB_SLOTS * C1_SEG_PAD; e += NT) in_s[e] = 0.f;
    __syncthreads();
  }
  typename Row::Data rd[3];
  floatx4 w_reg[RB_WLOADS];
  auto load_w = [&](int kh) __attribute__((always_inline)) {
    const floatx4 *wsrc = reinterpret_cast<const floatx4 *>(wt1 + (size_t)kh * C1_WELEMS);
#pragma unroll
    for (int i = 0; i < RB_WLOADS; ++i) {
      const int q = tid + NT * i;
      w_reg[i] = wsrc[q < C1_WELEMS / 4 ? q : 0];
    }
  };
  auto put_w = [&](int i, float *dst) __attribute__((always_inline)) {
    const int q = tid + NT * i;
    if (q < C1_WELEMS / 4) reinterpret_cast<floatx4 *>(dst)[q] = w_reg[i];
  };
  auto put_row = [&](const typename Row::Data &d, float *slot) __attribute__((always_inline)) {
    if constexpr (Row::kRing) {
      row.scatter(d, [&](int e, float v) __attribute__((always_inline)) { slot[e] = v; });
    } else {
#pragma unroll
      for (int i = 0; i < RB_IN4; ++i) {
        const int q = tid + NT * i;
        const floatx4 v = row.scaled(d, i);
        if (q < C1_SEG_PAD / 4) reinterpret_cast<floatx4 *>(slot)[q] = v;
      }
    }
  };
  // the first three input rows and the first weight row of the pair whose upper row is ho_
  auto load_first = [&](int ho_) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 3; ++i) row.load(rd[i], 2 * ho_ - 3 + i);
    load_w(0);
  };
#ifdef DVSG_STAMPS
  st[0] = C1_STAMP() - t_begin;
#endif
  load_first(2 * p0);

  for (int p = p0; p < p1; ++p) {
    const int ho = 2 * p;
#ifdef DVSG_STAMPS
    const unsigned long long f0 = C1_STAMP();
#endif
    // (the barrier that ends the pair before this one freed every slot and both weight buffers)
#pragma unroll
    for (int i = 0; i < RB_WLOADS; ++i) put_w(i, w_s);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      __builtin_amdgcn_sched_barrier(0);   // one row's scatter at a time: interleaved, a frame ring's three run out of registers
      put_row(rd[i], in_s + i * C1_SEG_PAD);
    }
    __builtin_amdgcn_sched_barrier(0);
    floatx16 acc[MI], acc2[MI];   // even and odd taps: see conv1_kernel
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mi][q] = acc2[mi][q] = 0.f;
#ifdef DVSG_STAMPS
    const unsigned long long f1 = C1_STAMP();
    __syncthreads();
    st[2] += f1 - f0;
    st[3] += C1_STAMP() - f1;
#else
    __syncthreads();
#endif

    int s_up = 0;   // slot of the upper row's operand: t mod 3
    for (int t = 0; t < 7; ++t) {
#ifdef DVSG_STAMPS
      const unsigned long long s3 = C1_STAMP();
#endif
      if (t < 6) {
        row.load(rd[0], 2 * ho + t);   // input row i = t + 3 of the pair
        load_w(t + 1);
      }
#ifdef DVSG_STAMPS
      st[4] += C1_STAMP() - s3;
#endif
      __builtin_amdgcn_sched_barrier(0);  // prefetch stays ahead of the MFMA loop
      const int s_lo = s_up == 0 ? 2 : s_up - 1;   // (t + 2) mod 3
      const float *a0 = in_s + (wr ? s_lo : s_up) * C1_SEG_PAD + 2 * kConv1Cin * (wm * 32 * MI + r) + 2 * h;
      const float *bp = w_s + (t & 1) * C1_WELEMS + (wn * 32 + r) * kConv1Ld + 2 * h;
      // kernel row t + 1 into the idle buffer, one store per request from the middle of the loop on.  (At t = 6 the
      // registers still hold kernel row 6 and the idle buffer nothing anyone reads: the stores stay unconditional.)
      float *w_next = w_s + ((t + 1) & 1) * C1_WELEMS;
      // conv1_kernel's loop: the operands of step u + 1 are requested before the MFMAs of step u are issued
      constexpr int STEPS = kConv1Kpad / 4, PAIRS = (STEPS + 1) / 2;   // two steps per request: one ds_read2_b64 per operand
      constexpr int WPUT0 = PAIRS / 2;
      float2 va[2][2][MI], vb[2][2];
      auto read_pair = [&](int slot, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (2 * g + j >= STEPS) break;
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
            va[slot][j][mi] = *reinterpret_cast<const float2 *>(a0 + mi * (2 * kConv1Cin * 32) + 4 * (2 * g + j));
          vb[slot][j] = *reinterpret_cast<const float2 *>(bp + 4 * (2 * g + j));
        }
      };
      read_pair(0, 0);
#pragma unroll
      for (int g = 0; g < PAIRS; ++g) {
        if (g + 1 < PAIRS) read_pair((g + 1) & 1, g + 1);
        if (g >= WPUT0 && g < WPUT0 + RB_WLOADS) put_w(g - WPUT0, w_next);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (2 * g + j >= STEPS) break;
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) acc[mi] = mfma32(va[g & 1][j][mi].x, vb[g & 1][j].x, acc[mi]);
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) acc2[mi] = mfma32(va[g & 1][j][mi].y, vb[g & 1][j].y, acc2[mi]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (t < 6) {
#ifdef DVSG_STAMPS  // (each stamp drains lgkmcnt: the phase times are upper bounds)
        const unsigned long long s0 = C1_STAMP();
        __syncthreads();
        const unsigned long long s1 = C1_STAMP();
        put_row(rd[0], in_s + s_up * C1_SEG_PAD);
        const unsigned long long s2 = C1_STAMP();
        __syncthreads();
        st[1] += s1 - s0;
        st[2] += s2 - s1;
        st[3] += C1_STAMP() - s2;
#else
        __syncthreads();   // everyone is done with input row t
        put_row(rd[0], in_s + s_up * C1_SEG_PAD);
        __syncthreads();
#endif
      }
      s_up = s_up == 2 ? 0 : s_up + 1;
    }

    // ---- epilogue: the next pair's first loads fly under it; one transpose tile per row in the (idle) weight buffers
#ifdef DVSG_STAMPS
    const unsigned long long e0 = C1_STAMP();
#endif
    __syncthreads();
    float *Cs = w_s + wr * C1_WELEMS;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      C1_TILE_PUT(Cs, wm * 32 * MI + mi * 32, wn * 32, acc[mi][q] + acc2[mi][q]);
    __builtin_amdgcn_sched_barrier(0);   // (the accumulators are dead: their registers take the rows in flight)
    if (p + 1 < p1) load_first(ho + 2);
    // (the thread's place in the epilogue is derived here, per pair: held in registers across the band, the addresses and
    // the bias that follow from it push the frame ring's instantiations past 256 registers)
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));
    const float4 b4 = conv1_tile_bias(bias, tid_e);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
#if RB_POOL
    {
      const int col4 = tid_e & 15;
      const int nv = min(C1_TILE, Wo - wo0);   // the tile's conv columns inside the row: even
      const int Hp = Ho >> 1, Wp = Wo >> 1;
      auto tap = [&](int j, int px) __attribute__((always_inline)) {   // conv1_tile_out's value of row j, pixel px
        float4 v = *reinterpret_cast<const float4 *>(w_s + j * C1_WELEMS + px * C1_LDC + 4 * col4);
        v.x = fmaxf(v.x + b4.x, 0.f);
        v.y = fmaxf(v.y + b4.y, 0.f);
        v.z = fmaxf(v.z + b4.z, 0.f);
        v.w = fmaxf(v.w + b4.w, 0.f);
        return v;
      };
      auto max4 = [](float4 a, float4 c) __attribute__((always_inline)) {
        return make_float4(fmaxf(a.x, c.x), fmaxf(a.y, c.y), fmaxf(a.z, c.z), fmaxf(a.w, c.w));
      };
      float *const carry_s = rb_lds + 2 * C1_WELEMS + RB_SLOTS * C1_SEG_PAD;   // [64 pooled columns][64]
      float *const prow = pooled + (((size_t)b * Hp + p) * Wp + (wo0 >> 1)) * 64 + 4 * col4;   // pooled row p of the tile
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int lc = (tid_e >> 4) + 32 * k;
        if (2 * lc >= nv) break;
        const bool third = 2 * lc + 2 < nv;   // (not: the row's end, or the tile's -- the seam kernel's tap)
        float4 hu = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), hl = hu;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (i == 2 && !third) break;
          hu = max4(hu, tap(0, 2 * lc + i));
          hl = max4(hl, tap(1, 2 * lc + i));
        }
        float4 *const cp = reinterpret_cast<float4 *>(carry_s + lc * 64 + 4 * col4);
        if (p > p0) store4(prow - (size_t)Wp * 64 + (size_t)lc * 64, max4(*cp, hu));
        const float4 c = max4(hu, hl);
        if (p + 1 < p1)
          *cp = c;
        else
          store4(prow + (size_t)lc * 64, c);   // the band's last pooled row: whole if it is the image's last
      }
      // what the neighbours miss: this tile's column 0 of both rows (the tile to the left), the band's first conv row (the
      // band above)
      if (wo0 > 0 && tid_e < 32) {
        const int j = tid_e >> 4;
        store4(y + (((size_t)b * Ho + ho + j) * Wo + wo0) * 64 + 4 * col4, tap(j, 0));
      }
      if (p == p0 && p0 > 0) {
        float *yrow = y + (((size_t)b * Ho + ho) * Wo + wo0) * 64 + 4 * col4;
        conv1_tile_out<NT / 16>(w_s, b4, tid_e, wo0, Wo,
                                [&](int row_, float4 v) __attribute__((always_inline)) { store4(yrow + (size_t)row_ * 64, v); });
      }
    }
#else
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (ho + j >= Ho) break;   // a last pair of one row
      float *yrow = y + (((size_t)b * Ho + ho + j) * Wo + wo0) * 64 + 4 * (tid_e & 15);
      conv1_tile_out<NT / 16>(w_s + j * C1_WELEMS, b4, tid_e, wo0, Wo,
                              [&](int row_, float4 v) __attribute__((always_inline)) { store4(yrow + (size_t)row_ * 64, v); });
    }
#endif
    __syncthreads();
#ifdef DVSG_STAMPS
    st[5] += C1_STAMP() - e0;
#endif
  }
#ifdef DVSG_STAMPS
  if (tid == 0 && blockIdx.x < 65536) {
    unsigned long long *o = g_c1_stamps + (size_t)blockIdx.x * 8;
    o[0] = st[0]; o[1] = st[1]; o[2] = st[2]; o[3] = st[3]; o[4] = st[4]; o[5] = st[5];
    o[6] = C1_STAMP() - t_begin;
    o[7] = __builtin_amdgcn_s_memrealtime() - r_begin;
  }
#endif
}

