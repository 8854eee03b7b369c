// Device text that more than one family of root conv kernels uses (conv1_f32.hip, conv1_f16.hip, conv1_x3.hip): the
// staged input row, the tile decode and the transpose-tile epilogue, and the run-time SRC -> template argument switch of
// their launchers.  Everything sits in an unnamed namespace, like the kernels: each file instantiates its own copies.
// Every file that includes this is compiled with -ffp-contract=off (build.sh): scale_RGB's separately rounded ops.
#pragma once
#include <cstdint>
#include <type_traits>
#include <utility>

#include "cnn_device.h"
#include "cnn_kernels.h"

namespace dvsg {
namespace {

// (the tile and scale_RGB are described at the head of conv1.hip)
constexpr int C1_TILE = 128;
constexpr int C1_SEG_PAD = 5488;                              // staged elements: 1 + (2 * 127 + 7) * 21 = 5482, in whole groups of four
constexpr int C1_WELEMS = 64 * kConv1Ld;                      // 9600 floats per kernel row
constexpr int C1_LDC = 68;                                    // epilogue tile row stride

// ----------------------------------------------------------------------------------------
// The staged segment of an input row, shared by the three conv1 kernels.  Element e of the segment is
// input-row float (2 wo0 - 3) * 21 - 1 + e: it starts one element before the first window (the weight rows
// carry a zero tap in front), which is a multiple of four elements of the row, and is fetched as GROUPS
// 16-byte groups per thread (thread tid: groups tid, tid + NT, ...) -- 6 loads per thread and kernel row
// where element-wise fetching issued 22.  When the rows themselves are 16-byte aligned (ALIGNED: W a
// multiple of 4) every group is inside the row or outside it as a whole and the loads are unconditional and
// aligned; otherwise a group inside the row is one 4-byte-aligned dwordx4 load and a group that straddles
// an end of the row goes element by element.  Loads are issued from clamped indices whatever the validity
// (a predicated load whose value feeds arithmetic makes hipcc wait for each load in turn: serialised L2
// round trips); validity is a per-thread bit mask applied when the value is scaled.
// scale_RGB happens here, in float32: x * 255 - mean, two roundings like the TF ops (this file is compiled
// with -ffp-contract=off); element e is raw channel (e - 1) mod 21 of its pixel, group g = c / 7 lands in
// output group 2 - g and gets that group's mean; elements outside the image are 0 in the SCALED domain.
// ----------------------------------------------------------------------------------------
// MASKED (eval_train.py:43-45, 53-64: `patches * mask` in front of the CNN): src.mask is ONE plane [B,H,W] -- the projective
// warp of an all-ones image is the same in each of the 18 history channels -- and the raw value of a staged element of
// channel c < 18 is multiplied by its pixel's mask value before the scale: (x * m) * 255 - mean, three roundings like the
// TF ops.  The four elements of a group belong to at most two neighbouring pixels: two mask loads per group and row.
template <int NT, int GROUPS, bool ALIGNED, bool MASKED = false>
struct Conv1Row {
  static constexpr bool kRing = false;
  typedef float floatx4_u __attribute__((ext_vector_type(4), aligned(4)));
  floatx4 nmean[GROUPS];   // minus the channel-group mean of each element: x * 255 + (-mean) == x * 255 - mean exactly
  long idx[GROUPS];
  unsigned col_ok, full;
  bool fast;               // wave-uniform: every element this wave stages lies inside the image row (or behind the segment's
                           // end, where the weights are zero): no per-element masks -- packed multiply / add / f16 convert,
                           // 1.5 VALU per element where the masked path spends ~7 (SQ_INSTS_VALU: 10 per MFMA in the f16 kernel)
  struct Data {            // one input row in flight (prefetched under the MFMAs of the rows before it)
    floatx4 reg[GROUPS];
    float m0[MASKED ? GROUPS : 1], m1[MASKED ? GROUPS : 1];   // mask values of the group's first / second pixel
    bool row_ok;
  };
  const float *img;      // window b
  long row_elems;
  int H;
  const float *mplane;   // MASKED: mask plane of window b
  int mW;
  int mcol0[MASKED ? GROUPS : 1], mcol1[MASKED ? GROUPS : 1];   // columns (clamped into the row) of the group's two pixels
  unsigned m_first, m_second;   // per element: multiplied by m0 / by m1 (neither: channel >= 18, or not an element of the row)

  __device__ __forceinline__ void init(const Conv1Src &src, int tid, int b, int wo0, int H_, int W, int seg_elems) {
    H = H_;
    row_elems = (long)W * kConv1Cin;
    img = static_cast<const float *>(src.base) + (long)b * H * row_elems;
    const long seg0 = (long)(2 * wo0 - 3) * kConv1Cin - 1;
    col_ok = full = 0;
    if constexpr (MASKED) {
      mplane = src.mask + (long)b * H * W;
      mW = W;
      m_first = m_second = 0;
    }
    bool mine = true;
#pragma unroll
    for (int i = 0; i < GROUPS; ++i) {
      const int e0 = 4 * (tid + NT * i);
      unsigned m = 0;
      if constexpr (MASKED) {
        const long ge0 = seg0 + e0;
        const int c0 = (int)(ge0 >= 0 ? ge0 / kConv1Cin : -((-ge0 + kConv1Cin - 1) / kConv1Cin));   // floor
        mcol0[i] = c0 < 0 ? 0 : (c0 >= W ? W - 1 : c0);
        mcol1[i] = c0 + 1 < 0 ? 0 : (c0 + 1 >= W ? W - 1 : c0 + 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long ge = ge0 + j;
          if (ge < 0 || ge >= row_elems) continue;
          const int col = (int)(ge / kConv1Cin), ch = (int)(ge - (long)col * kConv1Cin);
          if (ch >= kConv1Cin - 3) continue;                     // the newest frame is never masked (eval_train.py:62)
          if (col == c0) m_first |= 1u << (4 * i + j); else m_second |= 1u << (4 * i + j);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + j;
        const long ge = seg0 + e;
        const int g = ((e + kConv1Cin - 1) % kConv1Cin) / (kConv1Cin / 3);
        nmean[i][j] = g == 0 ? -123.68f : (g == 1 ? -116.779f : -103.939f);
        if (e < seg_elems && ge >= 0 && ge < row_elems) m |= 1u << j;
        if (e < seg_elems && !(ge >= 0 && ge < row_elems)) mine = false;   // a pad column this thread must zero
      }
      col_ok |= m << (4 * i);
      if (m == 15u) full |= 1u << i;
      idx[i] = (ALIGNED && m != 15u) ? 0 : seg0 + e0;   // ALIGNED: a group outside the row reads the row's first
    }
    // (elements behind the segment's end are staged as whatever finite value the clamped load returned: they meet zero weights)
    fast = ALIGNED && __builtin_amdgcn_ballot_w64(!mine) == 0;
  }
  // input row `hi` (clamped into the image; `row_ok` remembers whether it was inside)
  __device__ __forceinline__ void load(Data &d, int hi) const {
    d.row_ok = hi >= 0 && hi < H;
    const int hc = hi < 0 ? 0 : (hi >= H ? H - 1 : hi);
    const float *xrow = img + (long)hc * row_elems;
    if constexpr (MASKED) {
      const float *mrow = mplane + (long)hc * mW;
#pragma unroll
      for (int i = 0; i < GROUPS; ++i) {
        d.m0[i] = mrow[mcol0[i]];
        d.m1[i] = mrow[mcol1[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < GROUPS; ++i) {
      if constexpr (ALIGNED) {
        d.reg[i] = *reinterpret_cast<const floatx4 *>(xrow + idx[i]);
      } else if ((full >> i) & 1u) {
        d.reg[i] = *reinterpret_cast<const floatx4_u *>(xrow + idx[i]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) d.reg[i][j] = ((col_ok >> (4 * i + j)) & 1u) ? xrow[idx[i] + j] : 0.f;
      }
    }
  }
  // group i of a row in flight, scaled
  __device__ __forceinline__ floatx4 scaled(const Data &d, int i) const {
    floatx4 x = d.reg[i];
    if constexpr (MASKED) {   // patches * mask (eval_train.py:64), then scale_RGB; a factor of 1.0f is exact
      floatx4 m4;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        m4[j] = ((m_first >> (4 * i + j)) & 1u) ? d.m0[i] : (((m_second >> (4 * i + j)) & 1u) ? d.m1[i] : 1.0f);
      x = x * m4;
    }
    if (fast) {   // (both conditions are uniform over the wave / the workgroup)
      if (!d.row_ok) return floatx4{0.f, 0.f, 0.f, 0.f};
      return x * 255.0f + nmean[i];
    }
    const unsigned ok = d.row_ok ? col_ok : 0u;
    floatx4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((ok >> (4 * i + j)) & 1u) ? x[j] * 255.0f + nmean[i][j] : 0.f;
    return v;
  }
};

// ----------------------------------------------------------------------------------------
// The same staged segment assembled from a FRAME RING instead of a window tensor (SURVEY.md 8f-1/-2,
// eval.py:103-104: `np.concatenate` of the 7 window frames fused into this load stage).  The source is a pool
// of RGB frames [n_pool][H][W][3] -- float32 in [0,1], or the raw uint8 frames, whose `/ 255.` (eval.py:80) is
// fused here too -- and window b consists of the pool frames table[b][0..6], oldest to newest.  Element e of the
// staged segment (pixel p = (e - 1) / 21 of the segment, channel c = 3 f + rgb) is float 3 p' + rgb of row
// `hi` of frame f: per frame the segment is ONE contiguous run of 3 * 261 row elements, fetched in groups of
// four from one pixel before the run (a multiple of four elements of the row, like the window path's "one
// element before"), and each element is scattered to its place in the pixel-major LDS image.  So the LDS
// image, the weights and the MFMA loop are the window kernels' own; only the staging differs: the same number
// of global loads (4 elements each), ds_write_b32 / b16 per element instead of b128 per group.
// uint8: f32(double(v) / 255.) * 255.f == (float)v EXACTLY for all 256 byte values (exhaustive:
// tests/test_frames_cpu.py), so the scaled value float(v) - mean is bit-identical to the float path's
// x * 255 - mean on the converted frame, with one conversion and one subtraction per element.
// An index outside [0, n_pool) stages zeros (raw domain), like dvsg_window_gather_f32.
// ----------------------------------------------------------------------------------------
constexpr int C1_RING_PX = 2 * (C1_TILE - 1) + 7;            // 261 pixels of the input row feed a tile
constexpr int C1_RING_RG = (3 * (C1_RING_PX + 1) + 3) / 4;   // 197 groups of four per frame: one pixel of lead-in + the run
constexpr int C1_RING_GROUPS = 7 * C1_RING_RG;               // 1379

// MASKED: as for Conv1Row -- the groups of the six history frames (window slots 0..5) multiply their raw values by the mask
// plane's value at their pixel.  uint8 frames then need x = float32(v / 255.) itself (eval_train.py:119: the frame
// reader's float64 quotient, rounded once by the feed): q = v * r, q' = fma(fma(-q, 255, v), r, q) with r = f32(1 / 255) is
// that value for all 256 bytes (exhaustive: tests/test_frames_cpu.py), and (x * 1.0f) * 255.f == (float)v exactly.
template <int NT, int GROUPS, typename TS, bool ALIGNED, bool MASKED = false>
struct Conv1RingRow {
  static constexpr bool kRing = true;
  static constexpr bool kU8 = sizeof(TS) == 1;
  static_assert(NT * GROUPS >= C1_RING_GROUPS, "not enough threads x groups for 7 frame runs");
  static_assert(GROUPS <= 8, "per-element masks are 32 bits wide");
  typedef float floatx4_u __attribute__((ext_vector_type(4), aligned(4)));
  floatx4 nmean[GROUPS];   // minus the channel-group mean of each element
  bool fast;               // wave-uniform: no pad column and no missing frame among this wave's elements (see Conv1Row)
  long off[GROUPS];        // element offset of the group in the pool, row 0 of its frame
  int l0[GROUPS];          // LDS element of the first value's PIXEL (channel 3 f of it)
  unsigned phase;          // 2 bits per group: rgb of the group's first value
  unsigned col_ok, st_ok;  // per element: inside the image row / inside the staged segment
  unsigned no_frame;       // per group: its window slot names a frame outside the pool (reads as a frame of zeros)
  struct Data {            // one input row in flight
    floatx4 regf[kU8 ? 1 : GROUPS];
    unsigned regu[kU8 ? GROUPS : 1];
    float m0[MASKED ? GROUPS : 1], m1[MASKED ? GROUPS : 1];
    bool row_ok;
  };
  const TS *pool;
  long row_elems;
  int H;
  const float *mplane;   // MASKED: mask plane of window b
  int mW;
  int mcol0[MASKED ? GROUPS : 1], mcol1[MASKED ? GROUPS : 1];
  unsigned m_first, m_second;   // per element: multiplied by m0 / m1 (a group of the newest frame: neither)

  __device__ __forceinline__ void init(const Conv1Src &src, int tid, int b, int wo0, int H_, int W, int /*seg_elems*/) {
    H = H_;
    row_elems = (long)W * 3;
    pool = static_cast<const TS *>(src.base);
    const long frame_elems = (long)H * row_elems;
    const long r_first = (long)(2 * wo0 - 4) * 3;    // one pixel before the segment: a multiple of 4
    col_ok = st_ok = phase = no_frame = 0;
    if constexpr (MASKED) {
      mplane = src.mask + (long)b * H * W;
      mW = W;
      m_first = m_second = 0;
    }
    bool mine = true;
#pragma unroll
    for (int i = 0; i < GROUPS; ++i) {
      const int q = tid + NT * i;
      const int f = q / C1_RING_RG, g = q - f * C1_RING_RG;
      const bool in_range = q < C1_RING_GROUPS;
      const int fi = in_range ? src.table[b * 7 + f] : -1;
      const bool frame_ok = fi >= 0 && fi < src.n_pool;
      const long r0 = r_first + 4 * g;
      unsigned mc = 0, ms = 0;
      if constexpr (MASKED) {
        const int c0 = (int)(r0 >= 0 ? r0 / 3 : -((-r0 + 2) / 3));   // floor: the group's first pixel
        mcol0[i] = c0 < 0 ? 0 : (c0 >= W ? W - 1 : c0);
        mcol1[i] = c0 + 1 < 0 ? 0 : (c0 + 1 >= W ? W - 1 : c0 + 1);
        if (in_range && f < 6) {                                      // eval_train.py:58,62: the history frames only
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const long r = r0 + j;
            if (r < 0 || r >= row_elems) continue;
            if ((int)(r / 3) == c0) m_first |= 1u << (4 * i + j); else m_second |= 1u << (4 * i + j);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = 4 * g + j;                      // element of the run, lead-in pixel included
        const int c = 3 * f + t % 3;
        const int grp = c / (kConv1Cin / 3);
        nmean[i][j] = grp == 0 ? -123.68f : (grp == 1 ? -116.779f : -103.939f);
        if (in_range && t >= 3 && t < 3 * (C1_RING_PX + 1)) ms |= 1u << j;
        if (in_range && r0 + j >= 0 && r0 + j < row_elems) mc |= 1u << j;
      }
      if (in_range && !frame_ok) no_frame |= 1u << i;   // raw value 0 (scaled: -mean), read from the pool's frame 0 and dropped
      if ((ms & ~mc) != 0 || (in_range && !frame_ok)) mine = false;
      // ALIGNED: a group lies inside the row or outside it as a whole (both ends of the row and the run's start are
      // multiples of four elements); outside it reads row `hc` of the pool's first frame and its values are dropped.
      // Element-wise otherwise.
      const bool whole = mc == 15u;
      if (ALIGNED && !whole) mc = 0;
      col_ok |= mc << (4 * i);
      st_ok |= ms << (4 * i);
      off[i] = (ALIGNED && !whole) ? 0 : (frame_ok ? (long)fi * frame_elems : 0) + r0;
      // value j of the group: t = 4 g + j, pixel t / 3 of the run (the lead-in pixel is -1 of the segment), rgb t % 3,
      // LDS element 1 + 21 (t / 3 - 1) + 3 f + t % 3
      l0[i] = 1 + kConv1Cin * ((4 * g) / 3 - 1) + 3 * f;
      phase |= (unsigned)((4 * g) % 3) << (2 * i);
    }
    fast = __builtin_amdgcn_ballot_w64(!mine) == 0;
  }
  __device__ __forceinline__ void load(Data &d, int hi) const {
    d.row_ok = hi >= 0 && hi < H;
    const int hc = hi < 0 ? 0 : (hi >= H ? H - 1 : hi);
    const long roff = (long)hc * row_elems;
    if constexpr (MASKED) {
      const float *mrow = mplane + (long)hc * mW;
#pragma unroll
      for (int i = 0; i < GROUPS; ++i) {
        d.m0[i] = mrow[mcol0[i]];
        d.m1[i] = mrow[mcol1[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < GROUPS; ++i) {
      const TS *p = pool + off[i] + roff;
      if constexpr (kU8) {
        if constexpr (ALIGNED) {
          d.regu[i] = *reinterpret_cast<const unsigned *>(p);
        } else {
          unsigned w = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if ((col_ok >> (4 * i + j)) & 1u) w |= (unsigned)p[j] << (8 * j);
          d.regu[i] = w;
        }
      } else {
        if constexpr (ALIGNED) {
          d.regf[i] = *reinterpret_cast<const floatx4 *>(p);
        } else if (((col_ok >> (4 * i)) & 15u) == 15u) {
          d.regf[i] = *reinterpret_cast<const floatx4_u *>(p);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) d.regf[i][j] = ((col_ok >> (4 * i + j)) & 1u) ? (float)p[j] : 0.f;
        }
      }
    }
  }
  // every staged element of a row in flight, scaled: put(LDS element index, value)
  template <typename PUT>
  __device__ __forceinline__ void scatter(const Data &d, PUT put) const {
    const unsigned ok = d.row_ok ? col_ok : 0u;
    const bool plain = fast && d.row_ok;   // uniform: no masks to apply
#pragma unroll
    for (int i = 0; i < GROUPS; ++i) {
      const int ph = (phase >> (2 * i)) & 3u;
      floatx4 raw4;
      if constexpr (MASKED) {
        floatx4 m4, x;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          m4[j] = ((m_first >> (4 * i + j)) & 1u) ? d.m0[i] : (((m_second >> (4 * i + j)) & 1u) ? d.m1[i] : 1.0f);
        if constexpr (kU8) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v = (float)((d.regu[i] >> (8 * j)) & 255u);
            const float q = v * (1.0f / 255.0f);
            x[j] = __builtin_fmaf(__builtin_fmaf(-q, 255.0f, v), 1.0f / 255.0f, q);   // f32(v / 255.), correctly rounded
          }
        } else {
          x = d.regf[i];
        }
        raw4 = (x * m4) * 255.0f;
      } else if constexpr (kU8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) raw4[j] = (float)((d.regu[i] >> (8 * j)) & 255u);   // == f32(v / 255.) * 255.f, exactly
      } else {
        raw4 = d.regf[i] * 255.0f;
      }
      const floatx4 sc4 = raw4 + nmean[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v;
        if (plain) {
          v = sc4[j];
        } else {
          const float raw = ((no_frame >> i) & 1u) ? 0.f : raw4[j];
          v = ((ok >> (4 * i + j)) & 1u) ? raw + nmean[i][j] : 0.f;
        }
        const int t = ph + j, step = t / 3;                              // t in 0..5
        if ((st_ok >> (4 * i + j)) & 1u) put(l0[i] + kConv1Cin * step + (t - 3 * step), v);
      }
    }
  }
};

// The staged row of a conv1 kernel's SRC (kSrcAligned, kSrcKindShift, kSrcMasked in cnn_kernels.h): a window tensor's
// Conv1Row, or a frame ring's Conv1RingRow over float32 / uint8 frames.
template <int NT, int GROUPS, int SRC>
struct Conv1RowSel {
  static constexpr int kKind = SRC >> kSrcKindShift & 3;
  static constexpr bool kAligned = (SRC & kSrcAligned) != 0, kMasked = (SRC & kSrcMasked) != 0;
  static_assert(SRC >= 0 && SRC < 16 && kKind <= kSrcRingU8, "no such conv1 source");
  typedef std::conditional_t<kKind == kSrcWindow, Conv1Row<NT, GROUPS, kAligned, kMasked>,
                             Conv1RingRow<NT, (C1_RING_GROUPS + NT - 1) / NT, std::conditional_t<kKind == kSrcRingU8, uint8_t, float>,
                                          kAligned, kMasked>> type;
};

// ----------------------------------------------------------------------------------------
// What the conv1 kernels share beyond the staged row: which tile a workgroup owns, and the way its 128 pixels x 64 channels
// of float32 results leave through a [C1_TILE][C1_LDC] transpose tile in LDS (profiles/r18_conv1_dedup_isa_diff.txt: the
// machine code of every kernel against the hand-written copies these replaced).
// ----------------------------------------------------------------------------------------
struct Conv1Tile {
  int b, ho, wo0;   // window, output row (row pair, band: whatever `rows` counted), first output pixel
};
// Each XCD takes a contiguous range of tiles: the 3-4 output rows that share an input row run on the same L2 (consecutive
// block ids are dealt round-robin over the 8 XCDs).  Column tiles fastest, then `rows` per window.
__device__ __forceinline__ Conv1Tile conv1_tile(int wtiles, int rows) {
  int blk = xcd_remap(blockIdx.x, gridDim.x);
  const int wt_i = blk % wtiles;
  blk /= wtiles;
  const int ho = blk % rows;
  const int b = blk / rows;
  return {b, ho, wt_i * C1_TILE};
}
// A wave's 32 pixels (from PIX0) x 32 channels (from COL0) of the lane (r, h in scope) into the transpose tile Cs: VALUE, an
// expression in q, is register q of the 32x32 MFMA result -- pixel (q & 3) + 8 (q >> 2) + 4 h of the block, channel r.
// (A macro: as a function that takes the value as a callable it moved the register allocation of 92 of the 102 kernels.)
#define C1_TILE_PUT(Cs, PIX0, COL0, VALUE) \
  _Pragma("unroll") for (int q = 0; q < 16; ++q) Cs[(PIX0 + (q & 3) + 8 * (q >> 2) + 4 * h) * C1_LDC + COL0 + r] = VALUE
// The tile's way out: thread tid takes channels 4 (tid & 15) .. + 3 (their bias: conv1_tile_bias) of the pixels tid >> 4,
// + STEP, ... (STEP = threads / 16) that lie inside the output row: bias, ReLU, then store(pixel of the tile, four values).
__device__ __forceinline__ float4 conv1_tile_bias(const float *__restrict__ bias, int tid) {
  return *reinterpret_cast<const float4 *>(bias + 4 * (tid & 15));
}
template <int STEP, typename STORE>
__device__ __forceinline__ void conv1_tile_out(const float *Cs, const float4 b4, int tid, int wo0, int Wo, STORE store) {
  const int col4 = tid & 15, row0 = tid >> 4;
#pragma unroll 4
  for (int row = row0; row < C1_TILE; row += STEP) {
    if (wo0 + row >= Wo) break;
    float4 v = *reinterpret_cast<const float4 *>(Cs + row * C1_LDC + 4 * col4);
    v.x = fmaxf(v.x + b4.x, 0.f);
    v.y = fmaxf(v.y + b4.y, 0.f);
    v.z = fmaxf(v.z + b4.z, 0.f);
    v.w = fmaxf(v.w + b4.w, 0.f);
    store(row, v);
  }
}

#ifdef DVSG_STAMPS  // diagnostic build: per-workgroup phase times; a file whose kernels write stamps declares its own g_c1_stamps
#define C1_STAMP() __builtin_amdgcn_s_memtime()
#endif

// Run-time SRC -> compile-time constant: calls f(std::integral_constant<int, SRC>) for the legal value equal to `src`: every
// Conv1SrcKind, aligned or not, unmasked, and with MASKED_TOO the same six with kSrcMasked.  False, and no call, for any other.
template <int S>
using SrcC = std::integral_constant<int, S>;
template <bool MASKED_TOO, typename F>
bool with_conv1_src(int src, F &&f) {
  auto is = [&](auto c) { return src == c && (f(c), true); };
  if (is(SrcC<conv1_src(kSrcWindow, false, false)>{}) || is(SrcC<conv1_src(kSrcWindow, true, false)>{}) ||
      is(SrcC<conv1_src(kSrcRingF32, false, false)>{}) || is(SrcC<conv1_src(kSrcRingF32, true, false)>{}) ||
      is(SrcC<conv1_src(kSrcRingU8, false, false)>{}) || is(SrcC<conv1_src(kSrcRingU8, true, false)>{}))
    return true;
  if constexpr (MASKED_TOO)
    return is(SrcC<conv1_src(kSrcWindow, false, true)>{}) || is(SrcC<conv1_src(kSrcWindow, true, true)>{}) ||
           is(SrcC<conv1_src(kSrcRingF32, false, true)>{}) || is(SrcC<conv1_src(kSrcRingF32, true, true)>{}) ||
           is(SrcC<conv1_src(kSrcRingU8, false, true)>{}) || is(SrcC<conv1_src(kSrcRingU8, true, true)>{});
  return false;
}

}  // namespace
}  // namespace dvsg
