// Host side of localizationNet (networks.py:30-46) and of the fused evaluation graph
// (model.py:98-123): checkpoint ingestion (BatchNorm folding, weight re-layout for the MFMA
// fragment scheme of conv_gemm.hip / the conv1_*.hip kernels, float16 copies), workspace planning and the
// launch sequence for both storage precisions; with them the calibration of the float16 mode, the conv and fused operator
// entry points and the debug API.  The handle itself is locnet_internal.h's; its views, dvsg_locnet_destroy and the entry
// points that read a handle's render properties (the source-size renders among them) are views.cpp's.
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "locnet_internal.h"

namespace dvsg {
namespace {

constexpr float kBnEps = 1e-5f;  // slim resnet_arg_scope batch_norm_epsilon
const char *kPrefix = "stabNet/localizationNet/";  // model.py:114-117

struct HostArray {
  const float *data;
  int nd;
  int64_t dims[4];
  size_t size() const {
    size_t n = 1;
    for (int i = 0; i < nd; ++i) n *= (size_t)dims[i];
    return n;
  }
};

struct BlockSpec {
  const char *name;
  int base, units, last_stride;
};
const BlockSpec kBlocks[4] = {{"block1", 64, 3, 2}, {"block2", 128, 4, 2}, {"block3", 256, 6, 2}, {"block4", 512, 3, 1}};
const int kDenseDims[4][2] = {{2048, 2048}, {2048, 1024}, {1024, 512}, {512, 50}};

typedef std::map<std::string, HostArray> ArrayMap;

int find(const ArrayMap &m, const std::string &name, std::initializer_list<int64_t> shape, const HostArray **out) {
  auto it = m.find(name);
  if (it == m.end()) return fail(DVSG_ERR_WEIGHTS, "checkpoint array missing: %s", name.c_str());
  const HostArray &a = it->second;
  bool ok = a.nd == (int)shape.size();
  int i = 0;
  for (int64_t s : shape) {
    if (ok && a.dims[i] != s) ok = false;
    ++i;
  }
  if (!ok) {
    std::string want, got;
    for (int64_t s : shape) want += std::to_string(s) + ",";
    for (int j = 0; j < a.nd; ++j) got += std::to_string(a.dims[j]) + ",";
    return fail(DVSG_ERR_WEIGHTS, "checkpoint array %s has shape [%s] expected [%s]", name.c_str(), got.c_str(),
                want.c_str());
  }
  *out = &a;
  return DVSG_OK;
}

// Device memory that lives as long as the handle: registered in net->allocs as soon as it exists, so dvsg_locnet_destroy
// frees it whatever fails afterwards
template <typename T>
int device_alloc(dvsg_locnet *net, size_t bytes, T **ptr) {
  void *p = nullptr;
  DVSG_HIP(hipMalloc(&p, bytes));
  net->allocs.push_back(p);
  *ptr = static_cast<T *>(p);
  return DVSG_OK;
}

template <typename T>
int upload(dvsg_locnet *net, const std::vector<T> &h, T **dev) {
  if (int rc = device_alloc(net, h.size() * sizeof(T), dev)) return rc;
  DVSG_HIP(hipMemcpy(*dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return DVSG_OK;
}

// BatchNorm inference folded to y = conv(x, w * scale) + shift.
int bn_fold(const ArrayMap &m, const std::string &scope, int c, std::vector<float> *scale, std::vector<float> *shift) {
  const HostArray *g, *b, *mu, *var;
  if (int rc = find(m, scope + "/BatchNorm/gamma", {c}, &g)) return rc;
  if (int rc = find(m, scope + "/BatchNorm/beta", {c}, &b)) return rc;
  if (int rc = find(m, scope + "/BatchNorm/moving_mean", {c}, &mu)) return rc;
  if (int rc = find(m, scope + "/BatchNorm/moving_variance", {c}, &var)) return rc;
  scale->resize(c);
  shift->resize(c);
  for (int i = 0; i < c; ++i) {
    const float inv = g->data[i] / std::sqrt(var->data[i] + kBnEps);
    (*scale)[i] = inv;
    (*shift)[i] = b->data[i] - mu->data[i] * inv;
  }
  return DVSG_OK;
}

// (Re)make the stage-packed copies of a layer's float16 row matrix `rows` [nrows][k*k*cin] for conv_gemm_wide16.hip: order 0
// (64-byte activation rows), 1 (128-byte rows), 2 (3x3: a kernel row's taps from one run); a 1x1 layer's K order is the same
// in 0 and 1: one copy.  A copy that exists already is packed again in place
int pack_wide16(dvsg_locnet *net, const ConvLayer &L, const _Float16 *rows, int nrows, _Float16 **p0, _Float16 **pa, _Float16 **ph) {
  auto pack = [&](int order, _Float16 **out) -> int {
    if (!*out)
      if (int rc = device_alloc(net, wide16_packed_bytes(nrows, L.cin, L.ksize), out)) return rc;
    return launch_pack_wide16(rows, *out, nrows, L.cin, L.ksize, order, nullptr);
  };
  if (int rc = pack(0, p0)) return rc;
  if (L.ksize == 1) {
    *pa = *p0;
  } else {
    if (int rc = pack(1, pa)) return rc;
    if (int rc = pack(2, ph)) return rc;
  }
  DVSG_HIP(hipStreamSynchronize(nullptr));
  return DVSG_OK;
}

// ... of a layer's PLAIN float16 weights (round 3 built the packing for the stacked hi / lo rows only, so a layer without the
// lo piece fetched half-line weight rows again)
int pack_plain(dvsg_locnet *net, ConvLayer *L) {
  if (L->cin % 64 != 0 || L->cout % 128 != 0 || !L->wt16) return DVSG_OK;
  return pack_wide16(net, *L, L->wt16, L->cout, &L->wt16q, &L->wt16qa, &L->wt16qh);
}

// Generic conv: HWIO -> [cout][kh][kw][cin] with the BN scale folded in; float32 and float16 copies.
int make_conv(dvsg_locnet *net, const ArrayMap &m, const std::string &scope, ConvLayer *L) {
  const HostArray *w;
  if (int rc = find(m, scope + "/weights", {L->ksize, L->ksize, L->cin, L->cout}, &w)) return rc;
  std::vector<float> scale, shift;
  if (int rc = bn_fold(m, scope, L->cout, &scale, &shift)) return rc;
  const int K = L->ksize * L->ksize * L->cin;
  std::vector<float> wt((size_t)L->cout * K);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < L->cout; ++n) wt[(size_t)n * K + k] = w->data[(size_t)k * L->cout + n] * scale[n];
  std::vector<_Float16> wt16(wt.size());
  for (size_t i = 0; i < wt.size(); ++i) wt16[i] = (_Float16)wt[i];
  // hi / lo pairs: w ~ hi + 2^-11 lo, both float16 (a float16 weight alone is off by up to 2^-12 relative,
  // the same way at every pixel); group g of 64 channels = rows [128 g, 128 g + 64) hi, then 64 rows lo
  std::vector<_Float16> wt16s(2 * wt.size());
  for (int n = 0; n < L->cout; ++n)
    for (int k = 0; k < K; ++k) {
      const float w32 = wt[(size_t)n * K + k];
      const _Float16 hi = (_Float16)w32;
      const _Float16 lo = (_Float16)((w32 - (float)hi) * 2048.0f);
      const size_t row = (size_t)(n / 64) * 128 + n % 64;
      wt16s[row * K + k] = hi;
      wt16s[(row + 64) * K + k] = lo;
    }
  // "f32s" pieces: w ~ hi + lo, hi = f16(w), lo = f16(w - hi) (unscaled: float16 subnormals are inputs the
  // matrix cores keep); a 32-k row stage is 128 bytes like a float32 one: 32 hi halves, then 32 lo halves
  std::vector<_Float16> wt32s(2 * wt.size());
  for (int n = 0; n < L->cout; ++n)
    for (int k = 0; k < K; ++k) {
      const float w32 = wt[(size_t)n * K + k];
      const _Float16 hi = (_Float16)w32;
      const size_t base = ((size_t)n * (K / 32) + k / 32) * 64;
      wt32s[base + k % 32] = hi;
      wt32s[base + 32 + k % 32] = (_Float16)(w32 - (float)hi);
    }
  if (int rc = upload(net, wt, &L->wt)) return rc;
  if (int rc = upload(net, wt16, &L->wt16)) return rc;
  if (int rc = upload(net, wt16s, &L->wt16s)) return rc;
  if (L->cin % 64 == 0 && L->cout % 64 == 0)   // the layers conv_gemm_wide16.hip can take: the stacked pairs, packed
    if (int rc = pack_wide16(net, *L, L->wt16s, 2 * L->cout, &L->wt16p, &L->wt16pa, &L->wt16ph)) return rc;
  if (int rc = pack_plain(net, L)) return rc;
  if (int rc = upload(net, wt32s, &L->wt32s)) return rc;
  if (K % 32 == 0 && L->cout % 64 == 0) {   // "f32x3": three bfloat16 pieces per weight, packed stage by stage
    if (int rc = device_alloc(net, x3_packed_bytes(L->cout, K), &L->wt3x)) return rc;
    if (int rc = launch_pack_x3(L->wt, L->wt3x, L->cout, K, nullptr)) return rc;
    DVSG_HIP(hipStreamSynchronize(nullptr));
  }
  return upload(net, shift, &L->bias);
}

// conv1 (cin = 21): [7][64][kConv1Ld]; within a kernel row a zero tap, then the taps (kw, raw channel c) in input
// memory order (cnn_kernels.h).  scale_RGB's group reversal (networks.py:10-14) is folded here: raw channel
// c multiplies the weight of scaled-tensor channel (2 - c/G) * G + c % G.
int make_conv1(dvsg_locnet *net, const ArrayMap &m, const std::string &scope, ConvLayer *L) {
  const HostArray *w;
  if (int rc = find(m, scope + "/weights", {7, 7, L->cin, 64}, &w)) return rc;
  std::vector<float> scale, shift;
  if (int rc = bn_fold(m, scope, 64, &scale, &shift)) return rc;
  const int cin = L->cin, G = cin / 3;
  if (cin != kConv1Cin) {
    // any other window length (rootconv_kernel): the float32 image only, [7][64][rootconv_ld(cin)], tap (kw, c) at
    // kw * pitch + c -- no zero tap in front; the pad float of an even cin and the row's tail are zero weights
    const int pitch = rootconv_pitch(cin), ld = rootconv_ld(cin);
    std::vector<float> wr((size_t)7 * 64 * ld, 0.f);
    for (int kh = 0; kh < 7; ++kh)
      for (int kw = 0; kw < 7; ++kw)
        for (int c = 0; c < cin; ++c) {
          const int cs = (2 - c / G) * G + c % G;
          for (int n = 0; n < 64; ++n)
            wr[((size_t)kh * 64 + n) * ld + kw * pitch + c] = w->data[(((size_t)kh * 7 + kw) * cin + cs) * 64 + n] * scale[n];
        }
    if (int rc = upload(net, wr, &L->wt)) return rc;
    return upload(net, shift, &L->bias);
  }
  std::vector<float> wt((size_t)7 * 64 * kConv1Ld, 0.f);
  for (int kh = 0; kh < 7; ++kh)
    for (int kw = 0; kw < 7; ++kw)
      for (int c = 0; c < cin; ++c) {
        const int cs = (2 - c / G) * G + c % G;
        for (int n = 0; n < 64; ++n)
          wt[((size_t)kh * 64 + n) * kConv1Ld + 1 + kw * cin + c] =
              w->data[(((size_t)kh * 7 + kw) * cin + cs) * 64 + n] * scale[n];
      }
  std::vector<_Float16> wth((size_t)7 * 64 * kConv1LdH, (_Float16)0.f);
  for (int kh = 0; kh < 7; ++kh)
    for (int n = 0; n < 64; ++n)
      for (int k = 0; k < kConv1K; ++k)
        wth[((size_t)kh * 64 + n) * kConv1LdH + k + 1] = (_Float16)wt[((size_t)kh * 64 + n) * kConv1Ld + k + 1];
  // "f32s" pieces, [7][2][64][kConv1LdH]: hi image then lo image per kernel row, lo scaled by 2^11; tap k sits at
  // k + 1 behind a zero tap (conv1_split_kernel stages the input row from one element before the window)
  std::vector<_Float16> wts((size_t)7 * 2 * 64 * kConv1LdH, (_Float16)0.f);
  for (int kh = 0; kh < 7; ++kh)
    for (int n = 0; n < 64; ++n)
      for (int k = 0; k < kConv1K; ++k) {
        const float w32 = wt[((size_t)kh * 64 + n) * kConv1Ld + k + 1];
        const _Float16 hi = (_Float16)w32;
        wts[(((size_t)kh * 2 + 0) * 64 + n) * kConv1LdH + k + 1] = hi;
        wts[(((size_t)kh * 2 + 1) * 64 + n) * kConv1LdH + k + 1] = (_Float16)((w32 - (float)hi) * 2048.0f);
      }
  // "f32x3" pieces [14][3][64][kConv1X3Ld] bfloat16 (cnn_kernels.h): stage 2 kh + half, position p = tap + 1
  auto bf16_rn = [](float f) -> unsigned short {   // round to nearest even on the upper 16 bits (finite inputs)
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
  };
  auto bf16_val = [](unsigned short hbits) -> float {
    const uint32_t u = (uint32_t)hbits << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  };
  std::vector<unsigned short> wtx((size_t)14 * kConv1X3StageElems, 0);
  for (int kh = 0; kh < 7; ++kh)
    for (int n = 0; n < 64; ++n)
      for (int pos = 1; pos <= kConv1K; ++pos) {
        const float w32 = wt[((size_t)kh * 64 + n) * kConv1Ld + pos];
        const unsigned short p1 = bf16_rn(w32);
        const float r1 = w32 - bf16_val(p1);
        const unsigned short p2 = bf16_rn(r1);
        const unsigned short p3 = bf16_rn(r1 - bf16_val(p2));
        const size_t base = (size_t)(2 * kh + pos / 80) * kConv1X3StageElems + (size_t)n * kConv1X3Ld + pos % 80;
        wtx[base] = p1;
        wtx[base + 64 * kConv1X3Ld] = p2;
        wtx[base + 2 * 64 * kConv1X3Ld] = p3;
      }
  if (int rc = upload(net, wt, &L->wt)) return rc;
  if (int rc = upload(net, wth, &L->wt16)) return rc;
  if (int rc = upload(net, wts, &L->wt32s)) return rc;
  if (int rc = upload(net, wtx, &L->wt3x)) return rc;
  return upload(net, shift, &L->bias);
}

struct Dims {
  int H1, W1, Hp, Wp, pad_top, pad_left;
};

Dims root_dims(int H, int W) {
  Dims d;
  d.H1 = (H - 1) / 2 + 1;  // conv2d_same(7, stride 2): pad 3/3 then VALID
  d.W1 = (W - 1) / 2 + 1;
  d.Hp = (d.H1 + 1) / 2;   // max_pool2d 3x3/2 SAME
  d.Wp = (d.W1 + 1) / 2;
  const int pth = std::max((d.Hp - 1) * 2 + 3 - d.H1, 0), ptw = std::max((d.Wp - 1) * 2 + 3 - d.W1, 0);
  d.pad_top = pth / 2;
  d.pad_left = ptw / 2;
  return d;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

enum LayerKind { kKindC1 = 0, kKindC2 = 1, kKindC3 = 2, kKindSc = 3 };
inline bool f16_pairs(const dvsg_locnet *net, int block, int kind) {
  return g_opt.f16_split && ((g_opt.f16_pair_mask & net->f16_pair_mask) >> (4 * kind + block)) & 1;
}
struct Workspace {
  char *bufA, *bufB, *bufS, *r1, *r2;  // activations (element type = the run's precision)
  float *pool_part, *dpart0, *dpart1, *T, *Ft;
  char *splitk_slabs;  // kSplitKSlabBytes of partial tiles, reused by every split-K launch
  int *splitk_counters;  // kMaxConvLaunches x kSplitKMaxTiles tickets, zeroed once per forward
  size_t total;
};
constexpr int kMaxConvLaunches = 64;

// Sized for float32 activations; the float16 run uses the same plan with half the bytes.
Workspace plan(char *base, int B, int H, int W) {
  const Dims d = root_dims(H, W);
  // Walk the 16 units with forward()'s own (h, w) recurrence: with the ceil in (h - 1) / stride + 1
  // the per-sample element count does NOT shrink monotonically on tiny frames (8x8: block 4 needs
  // 1x1x2048 > 2x2x256), so the buffers are sized by the largest tenant, not by the first one.
  size_t big_el = std::max((size_t)d.H1 * d.W1 * 64, (size_t)d.Hp * d.Wp * 64);  // conv1 out (bufA), pool1 out (bufB)
  size_t small_el = 0;
  {
    int h = d.Hp, w = d.Wp;
    for (const BlockSpec &bs : kBlocks)
      for (int u = 1; u <= bs.units; ++u) {
        const int stride = u == bs.units ? bs.last_stride : 1;
        const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
        small_el = std::max(small_el, (size_t)h * w * bs.base);                  // r1 (conv1 out), r2 <= r1
        big_el = std::max(big_el, (size_t)ho * wo * bs.base * 4);                // unit out, shortcut
        if (u == 1) big_el = std::max(big_el, (size_t)h * w * bs.base * 5);     // [shortcut | conv1] of an opening unit (bufS)
        h = ho; w = wo;
      }
  }
  const size_t big = align256((size_t)B * big_el * sizeof(float));
  const size_t small = align256((size_t)B * small_el * sizeof(float));
  Workspace w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char *p = base + off;
    off += align256(bytes);
    return p;
  };
  w.bufA = take(big);
  w.bufB = take(big);
  w.bufS = take(big);
  w.r1 = take(small);
  w.r2 = take(small);
  w.pool_part = reinterpret_cast<float *>(take((size_t)kPoolSplits * B * 2048 * sizeof(float)));
  w.dpart0 = reinterpret_cast<float *>(take((size_t)kDenseSplits * 16 * 2048 * sizeof(float)));
  w.dpart1 = reinterpret_cast<float *>(take((size_t)kDenseSplits * 16 * 2048 * sizeof(float)));
  w.T = reinterpret_cast<float *>(take((size_t)B * 2 * 28 * sizeof(float)));
  w.Ft = reinterpret_cast<float *>(take((size_t)B * 50 * sizeof(float)));
  w.splitk_slabs = take(kSplitKSlabBytes);
  w.splitk_counters = reinterpret_cast<int *>(take((size_t)kMaxConvLaunches * kSplitKMaxTiles * sizeof(int)));
  w.total = off;
  return w;
}

// What a layer's launch reads and writes (tensors of storage_of(math), batch B): ld = elements between two pixels where the
// tensor is a column range of a wider one, 0 = dense
struct ConvIn { const void *ptr; int H, W, ld = 0; };
struct ConvRes { const void *ptr = nullptr; int H = 0, W = 0, stride = 1, ld = 0; };   // default-constructed: no residual
struct ConvOut { void *ptr; int Ho, Wo; };
// the split-K scratch of a pass and which of its ticket segments the next launch owns
struct ConvScratch { const Workspace &ws; int launch_idx = 0; };
constexpr int kNoReluFrom = -1;   // run_conv's relu_from: with relu false, no output channel gets the ReLU (else those from n on)

int run_conv(const ConvLayer &L, ConvMath math, int B, const ConvIn &x, const ConvOut &y, const ConvRes &res, bool relu,
             int relu_from, ConvScratch *scratch, hipStream_t s) {
  ConvGemm p;
  p.math = math;
  p.splitk_scratch = scratch->ws.splitk_slabs;
  p.splitk_scratch_bytes = kSplitKSlabBytes;
  p.splitk_counters = scratch->ws.splitk_counters + (size_t)(scratch->launch_idx++ % kMaxConvLaunches) * kSplitKMaxTiles;
  if (math == kMathF32X && !L.wt3x)
    return fail(DVSG_ERR_UNSUPPORTED, "f32x3: layer %d -> %d (k = %d) has no packed bfloat16 pieces (K %% 32, Cout %% 64)", L.cin, L.cout, L.ksize);
  p.x = x.ptr; p.w = L.image(math); p.bias = L.bias; p.res = res.ptr; p.y = y.ptr;
  p.B = B; p.H = x.H; p.W = x.W; p.Cin = L.cin; p.Ho = y.Ho; p.Wo = y.Wo; p.Cout = L.cout;
  p.ksize = L.ksize; p.stride = L.stride; p.pad = L.ksize == 3 ? 1 : 0;
  p.ldx = x.ld;
  p.res_H = res.H; p.res_W = res.W; p.res_stride = res.stride; p.res_ld = res.ld;
  p.relu = relu; p.relu_from = relu_from;
  return launch_conv_gemm(p, s);
}

// ---- calibration of the float16 mode's PLAIN weights (dvsg_debug_calibrate_f16_weights) --------------------------------
// With a recorder, forward() adds up every bottleneck unit's three convolution inputs per channel: slot 3 u + {0: the unit's
// input (shortcut, conv1), 1: conv1's output (conv2's input), 2: conv2's output (conv3's input)}.
struct Calib {
  double *sums = nullptr;    // device [16 * 3][2048]
  float *part = nullptr;     // device [kCalibBlocks][2048]: per-block partial sums of the tensor being recorded
  double rows[48] = {0};     // pixels summed per slot
};

// deterministic: block b adds up rows [b chunk, (b + 1) chunk) per channel into part[b][c]; channel_sum_final adds the
// blocks' partial sums in block order (double) onto out[c] -- the same bits from run to run, so the weights re-rounded from
// them are the same bits too
constexpr int kCalibBlocks = 512;
__global__ __launch_bounds__(256) void channel_sum_kernel(const float *__restrict__ x, long M, int C, long chunk,
                                                         float *__restrict__ part) {
  const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < M ? r0 + chunk : M;
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc = 0.f;
    for (long r = r0; r < r1; ++r) acc += x[r * C + c];
    part[(size_t)blockIdx.x * 2048 + c] = acc;
  }
}
__global__ __launch_bounds__(256) void channel_sum_final(const float *__restrict__ part, int nblk, int C, double *__restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double acc = out[c];
  for (int b = 0; b < nblk; ++b) acc += (double)part[(size_t)b * 2048 + c];
  out[c] = acc;
}

int calib_record(Calib *calib, int slot, const void *x, long M, int C, hipStream_t s) {
  if (!calib) return DVSG_OK;
  const long chunk = (M + kCalibBlocks - 1) / kCalibBlocks;
  const int nblk = (int)((M + chunk - 1) / chunk);
  hipLaunchKernelGGL(channel_sum_kernel, dim3(nblk), dim3(256), 0, s, static_cast<const float *>(x), M, C, chunk, calib->part);
  hipLaunchKernelGGL(channel_sum_final, dim3((C + 255) / 256), dim3(256), 0, s, calib->part, nblk, C,
                     calib->sums + (size_t)slot * 2048);
  calib->rows[slot] += (double)M;
  return check_launch("channel_sum_kernel");
}

// Runs the network in precision `precision`; stop_stage < 0 runs everything and writes F_t [B,50].  With `calib` (a float32
// pass) the units' convolution inputs are recorded into it, and block 1 runs unfused: its conv2 output only exists in
// LDS when fused.
int forward(const dvsg_locnet *net, const int precision, const Conv1Src &src, int src_kind, int B, int H, int W, float *F_t, int stop_stage,
            float *act_out, size_t act_out_bytes, int *act_dims, void *workspace, size_t workspace_bytes,
            hipStream_t s, Calib *calib) {
  DVSG_REQUIRE(net && src.base && workspace, "locnet forward: NULL pointer");
  DVSG_REQUIRE(B > 0 && H >= 1 && W >= 1, "locnet forward: bad shape B=%d H=%d W=%d", B, H, W);
  DVSG_REQUIRE(((uintptr_t)workspace & 255) == 0, "locnet forward: workspace must be 256-byte aligned");
  const Workspace ws = plan(static_cast<char *>(workspace), B, H, W);
  if (ws.total > workspace_bytes)
    return fail(DVSG_ERR_WORKSPACE, "locnet forward: workspace %zu bytes < required %zu", workspace_bytes, ws.total);
  net = base(net);   // a view runs its parent's network; the handle is first read here, behind every check
  const Dims d = root_dims(H, W);
  // the activation tensors' storage format.  (f32x3: float32 tensors throughout; conv1, the pools, block 1's fused kernel and
  // the head are the float32 kernels themselves, the conv GEMMs multiply bfloat16 pieces)
  const Precision act = storage_of(math_of(precision, true));

  // parity tap: copy (float32 run) or convert (float16 run) the stage's activation to act_out
  auto tap = [&](int stage, const void *x, int h, int w, int c) -> int {
    if (stage != stop_stage) return 0;
    const size_t n = (size_t)B * h * w * c;
    if (n * sizeof(float) > act_out_bytes)
      return fail(DVSG_ERR_INVALID_ARG, "tap buffer %zu bytes < %zu", act_out_bytes, n * sizeof(float));
    if (act == kF16) {
      if (int rc = launch_f16_to_f32(x, act_out, n, s)) return rc;
    } else if (act == kF32S) {
      if (int rc = launch_p_to_f32(x, act_out, n, s)) return rc;
    } else {
      DVSG_HIP(hipMemcpyAsync(act_out, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    act_dims[0] = h; act_dims[1] = w; act_dims[2] = c;
    return 1;
  };
#define DVSG_TAP(stage, x, h, w, c)            \
  do {                                         \
    int t_ = tap(stage, x, h, w, c);           \
    if (t_ < 0) return t_;                     \
    if (t_ > 0) return DVSG_OK;                \
  } while (0)
#define DVSG_RUN(call)             \
  do {                             \
    if (int rc_ = (call)) return rc_; \
  } while (0)

  // split-K tickets of every conv launch of this pass (each launch owns its own segment)
  DVSG_RUN(launch_zero_tickets(ws.splitk_counters, (size_t)kMaxConvLaunches * kSplitKMaxTiles, s));
  ConvScratch scratch{ws};
  const bool fuse_allowed = g_opt.fuse_conv != 0 && calib == nullptr;   // block 1's conv2 + conv3 in one kernel
  reset_root_kernel();
  // root: conv1 (+ fused scale_RGB; f32 multiply, output in `act`) -> bufA, max pool -> bufB.  Float32, where the pool pads
  // nothing on the top and the left and conv1's output is not tapped: the band kernel may pool in its epilogue (whether it
  // does is launch_conv1's choice), and bufA then holds the seam elements' missing conv values only
  RootPool root_pool{ws.bufB};
  const bool pool_in_conv1 = precision == kF32 && stop_stage != 0 && d.pad_top == 0 && d.pad_left == 0;
  {
  MarkerRange mr("dvsg/conv1");
  DVSG_RUN(launch_conv1(precision == kF32X && g_opt.x3_conv1 ? kF32X : act, src, src_kind, net->conv1.conv1_images(), ws.bufA, B, H, W,
                        d.H1, d.W1, net->c_in, s, pool_in_conv1 ? &root_pool : nullptr));
  }
  DVSG_TAP(0, ws.bufA, d.H1, d.W1, 64);
  {
  MarkerRange mr("dvsg/pool1");
  if (root_pool.fused)
    DVSG_RUN(launch_root_pool_seams(root_pool, ws.bufA, B, d.H1, d.W1, s));
  else
    DVSG_RUN(launch_maxpool(act, ws.bufA, ws.bufB, B, d.H1, d.W1, 64, d.Hp, d.Wp, d.pad_top, d.pad_left, s));
  }
  DVSG_TAP(1, ws.bufB, d.Hp, d.Wp, 64);

  char *X = ws.bufB, *Y = ws.bufA;
  int h = d.Hp, w = d.Wp;
  int stage = 2;
  int unit_in_block = 0, last_block = -1;
  for (const Unit &u : net->units) {
    unit_in_block = u.block == last_block ? unit_in_block + 1 : 1;
    last_block = u.block;
    char range_name[40];
    std::snprintf(range_name, sizeof(range_name), "dvsg/block%d/unit_%d", u.block + 1, unit_in_block);
    MarkerRange mr(range_name);
    const int ho = (h - 1) / u.stride + 1, wo = (w - 1) / u.stride + 1;
    ConvRes res{X, h, w, u.stride};
    // what this unit's layer of `kind` multiplies: the precision's math, in the float16 mode with or without the lo piece
    auto math = [&](int kind) { return math_of(precision, f16_pairs(net, u.block, kind)); };
    const int calib_slot = 3 * (stage - 2);
    DVSG_RUN(calib_record(calib, calib_slot, X, (long)B * h * w, u.c1.cin, s));
    // (float16 mode: the fused kernel multiplies against the stacked hi / lo weights only)
    // (f32x3: block 1's units run conv2 + conv3 in the f32x3 fused kernel, conv_fused_x3.hip, the opening unit's shortcut as
    // its own f32x3 GEMM -- x3_fuse = 3; A/B: 0 never fused, 1 the opening unit only and in the exact float32 kernel with
    // its shortcut, 2 all three in the exact float32 kernel)
    const bool x3_fused = precision == kF32X && g_opt.x3_fuse == 3;
    const bool x3_unfused = precision == kF32X && (g_opt.x3_fuse == 0 || (g_opt.x3_fuse == 1 && !u.has_shortcut));
    const bool fuse23 = fuse_allowed && !x3_unfused && conv_fusable(act, u.c2.cin, u.c2.cout, u.c3.cout, u.c2.ksize) &&
                        (act != kF16 || (f16_pairs(net, u.block, kKindC2) && f16_pairs(net, u.block, kKindC3) &&
                                         (!u.has_shortcut || f16_pairs(net, u.block, kKindSc))));
    // block 1's opening unit: its shortcut conv (64 -> 256) runs inside the fused conv2 + conv3 kernel
    const bool fuse_sc = fuse23 && !x3_fused && u.has_shortcut && u.stride == 1 && u.shortcut.cin == 64 && u.shortcut.cout == 256 &&
                         g_opt.fuse_shortcut;
    // blocks 2-4's opening units, float32 / f32s: shortcut and conv1 as ONE launch over [shortcut | conv1] weight rows; its
    // output [M, depth + base] sits in bufS, the shortcut in columns [0, depth) (conv3's residual, row stride depth + base),
    // conv1's ReLU'd output behind it (conv2's input, same stride).  One launch and one read of the unit's input less.
    const bool cat = u.has_shortcut && !fuse_sc && u.has_cat && act != kF16 && g_opt.concat_sc && !calib && u.stride == 1;
    ConvIn c2_in{ws.r1, h, w};
    if (cat) {
      DVSG_RUN(run_conv(u.cat, math_of(precision, false), B, {X, h, w}, {ws.bufS, h, w}, {}, false, u.shortcut.cout, &scratch, s));
      res = {ws.bufS, ho, wo, 1, u.cat.cout};
      c2_in = {ws.bufS + (size_t)u.shortcut.cout * sizeof(float), h, w, u.cat.cout};   // (f32s: 32 values are 128 bytes too)
    } else {
    if (u.has_shortcut && !fuse_sc) {  // 1x1 conv + BN, no ReLU (stride is 1 wherever depth changes)
      DVSG_RUN(run_conv(u.shortcut, math(kKindSc), B, {X, h, w}, {ws.bufS, ho, wo}, {}, false, kNoReluFrom, &scratch, s));
      res = {ws.bufS, ho, wo, 1};
    }
    DVSG_RUN(run_conv(u.c1, math(kKindC1), B, {X, h, w}, {ws.r1, h, w}, {}, true, kNoReluFrom, &scratch, s));
    }
    if (fuse23) {  // block 1: conv2 + conv3 in one kernel
      ConvFused f;
      // (float16: fuse23 has checked that all of the unit's layers carry the lo piece; f32x3 through the exact float32
      // kernel -- x3_fuse 1, 2 -- is the float32 math)
      f.math = x3_fused ? kMathF32X : math_of(act, true);
      f.x = ws.r1; f.wt2 = u.c2.image(f.math).rows; f.bias2 = u.c2.bias; f.wt3 = u.c3.image(f.math).rows; f.bias3 = u.c3.bias;
      f.res = res.ptr; f.y = Y;
      f.B = B; f.H = h; f.W = w; f.Cin = u.c2.cin; f.Ho = ho; f.Wo = wo; f.Cout = u.c3.cout;
      f.stride = u.c2.stride; f.res_H = res.H; f.res_W = res.W; f.res_stride = res.stride;
      if (fuse_sc) {
        f.res = nullptr;
        f.sc_x = X; f.sc_wt = u.shortcut.image(f.math).rows; f.sc_bias = u.shortcut.bias;
        f.sc_cin = u.shortcut.cin;
      }
      DVSG_RUN(launch_conv3x3_1x1(f, s));
    } else {
      DVSG_RUN(calib_record(calib, calib_slot + 1, ws.r1, (long)B * h * w, u.c2.cin, s));
      DVSG_RUN(run_conv(u.c2, math(kKindC2), B, c2_in, {ws.r2, ho, wo}, {}, true, kNoReluFrom, &scratch, s));
      DVSG_RUN(calib_record(calib, calib_slot + 2, ws.r2, (long)B * ho * wo, u.c3.cin, s));
      DVSG_RUN(run_conv(u.c3, math(kKindC3), B, {ws.r2, ho, wo}, {Y, ho, wo}, res, true, kNoReluFrom, &scratch, s));
    }
    h = ho; w = wo;
    DVSG_TAP(stage, Y, h, w, u.depth);
    ++stage;
    char *tmp = X; X = Y; Y = tmp;
  }

  // global average pool (float32 partial sums), then the float32 dense head in chunks of <= 16
  // samples; partial layouts are [b][split][k] so a batch chunk is a pointer offset.
  MarkerRange mr_head("dvsg/head");
  DVSG_RUN(launch_avgpool_partial(act, X, ws.pool_part, B, h * w, 2048, s));
  const float inv_hw = 1.0f / (float)(h * w);
  if (stop_stage == 18) {
    const size_t bytes = (size_t)B * 2048 * sizeof(float);
    if (bytes > act_out_bytes) return fail(DVSG_ERR_INVALID_ARG, "tap buffer %zu bytes < %zu", act_out_bytes, bytes);
    DVSG_RUN(launch_dense_finalize(ws.pool_part, kPoolSplits, inv_hw, nullptr, act_out, B, 2048, s));
    act_dims[0] = 1; act_dims[1] = 1; act_dims[2] = 2048;
    return DVSG_OK;
  }
  g_last_root_kernel[kRootDenseChunks] = (B + 15) / 16;
  for (int b0 = 0; b0 < B; b0 += 16) {
    const int bc = std::min(16, B - b0);
    float *pa = ws.dpart0, *pb = ws.dpart1;
    DVSG_RUN(launch_dense(ws.pool_part + (size_t)b0 * kPoolSplits * 2048, kPoolSplits, nullptr, inv_hw, 0,
                          net->dense_w[0], pa, bc, 2048, 2048, s));
    DVSG_RUN(launch_dense(pa, kDenseSplits, net->dense_b[0], 1.0f, 1, net->dense_w[1], pb, bc, 2048, 1024, s));
    DVSG_RUN(launch_dense(pb, kDenseSplits, net->dense_b[1], 1.0f, 1, net->dense_w[2], pa, bc, 1024, 512, s));
    DVSG_RUN(launch_dense(pa, kDenseSplits, net->dense_b[2], 1.0f, 1, net->dense_w[3], pb, bc, 512, 50, s));
    DVSG_RUN(launch_dense_finalize(pb, kDenseSplits, 1.0f, net->dense_b[3], F_t + (size_t)b0 * 50, bc, 50, s));
  }
  return DVSG_OK;
#undef DVSG_TAP
#undef DVSG_RUN
}

int forward(const dvsg_locnet *net, int prec, const float *patches, int B, int H, int W, float *F_t, int stop_stage,
            float *act_out, size_t act_out_bytes, int *act_dims, void *workspace, size_t workspace_bytes,
            hipStream_t s, Calib *calib) {
  const Conv1Src src{patches, nullptr, 0};
  return forward(net, prec, src, kSrcWindow, B, H, W, F_t, stop_stage, act_out, act_out_bytes, act_dims, workspace,
                 workspace_bytes, s, calib);
}

// What stabilize() and stabilize_ring() share, behind their own NULL and range checks (`fn` names the caller in the
// messages): F_t = localizationNet(src), T = the TPS of F_t on the constant V_src, then the caller's warp(T).  (Every
// handle's c_in is 3 S, so a mask or a ring fits any of them: S - 1 history frames, tables of S columns.)
template <typename Warp>
int stabilize_from(const char *fn, const dvsg_locnet *net, int prec, const Conv1Src &src, int src_kind,
                   int B, int H, int W, float *F_t, void *workspace, size_t workspace_bytes, void *stream, Warp warp) {
  DVSG_REQUIRE(prec == kF32 || prec == kF16 || prec == kF32S || prec == kF32X, "%s: unknown precision %d", fn, prec);
  const Workspace ws = plan(static_cast<char *>(workspace), B, H, W);
  if (ws.total > workspace_bytes)
    return fail(DVSG_ERR_WORKSPACE, "%s: workspace %zu bytes < required %zu", fn, workspace_bytes, ws.total);
  float *F = F_t ? F_t : ws.Ft;
  if (int rc = forward(net, prec, src, src_kind, B, H, W, F, -1, nullptr, 0, nullptr, workspace, workspace_bytes,
                       as_stream(stream), nullptr))
    return rc;
  // model.py:120: stn(u_t, V_src, F_t, [h, w]) with V_src tiled over the batch (:111); float32
  MarkerRange mr("dvsg/tps");
  net = base(net);
  if (int rc = tps_apply_impl(net->winv, net->v_src, F, 1, B, 25, ws.T, stream)) return rc;
  return warp(net, ws.T);
}

int stabilize(const dvsg_locnet *net, int prec, const float *patches_t, const float *u_t, const float *mask, int B, int H,
              int W, float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace, size_t workspace_bytes,
              void *stream) {
  DVSG_REQUIRE(net && patches_t && u_t && s_t_pred && workspace, "dvsg_stabilize: NULL pointer");
  DVSG_REQUIRE(B > 0 && B <= 65535, "dvsg_stabilize: B=%d out of range", B);
  Conv1Src src{patches_t, nullptr, 0};
  src.mask = mask;   // eval_train.py:43-45: the CNN sees patches * mask, the warp below the unmasked u_t
  return stabilize_from("dvsg_stabilize", net, prec, src, kSrcWindow, B, H, W, F_t, workspace, workspace_bytes, stream,
                        [&](const dvsg_locnet *net, const float *T) {
                          return tps_warp_impl(u_t, net->v_src, 0, T, B, H, W, 3, 25, H, W, s_t_pred, x_s, y_s, stream);
                        });
}

// The evaluation graph fed from a frame ring: window b = pool frames table[b][0..S-1] with S = c_in / 3,
// u_t = its newest frame table[b][S-1]; conv1 assembles the window in its load stage (eval.py:103-104) and, for a uint8 pool, applies the
// / 255. of eval.py:80 there; the warp reads u_t from the pool through the same table.  With out_slots, s_t_pred is the
// float32 pool and sample b's frame lands in its frame out_slots[b] (the history slot of an online stream).
int stabilize_ring(const dvsg_locnet *net, int prec, const void *pool, int pool_is_u8, int n_pool, const int32_t *table,
                   const float *mask, int B, int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace,
                   size_t workspace_bytes, void *stream, const int32_t *out_slots = nullptr) {
  DVSG_REQUIRE(net && pool && table && s_t_pred && workspace, "dvsg_stabilize_ring: NULL pointer");
  DVSG_REQUIRE(B > 0 && B <= 65535 && n_pool > 0, "dvsg_stabilize_ring: B=%d n_pool=%d out of range", B, n_pool);
  Conv1Src src{pool, table, n_pool};
  src.mask = mask;
  return stabilize_from("dvsg_stabilize_ring", net, prec, src,
                        pool_is_u8 ? kSrcRingU8 : kSrcRingF32, B, H, W, F_t, workspace, workspace_bytes, stream,
                        [&](const dvsg_locnet *net, const float *T) {
                          const int S = net->c_in / 3;
                          return tps_warp_ring_impl(pool, pool_is_u8, n_pool, table + (S - 1), S, net->v_src, 0, T, B, H, W, 25,
                                                    s_t_pred, x_s, y_s, stream, out_slots);
                        });
}

int conv_gemm_op(ConvMath math, const void *x, const void *wt, const float *bias, const void *res, void *y, int B,
                 int H, int W, int Cin, int Cout, int ksize, int stride, int relu, int res_stride, void *scratch,
                 size_t scratch_bytes, void *stream) {
  DVSG_REQUIRE(x && wt && bias && y, "dvsg_conv_gemm: NULL pointer");
  DVSG_REQUIRE(!scratch || ((uintptr_t)scratch & 255) == 0, "dvsg_conv_gemm: scratch must be 256-byte aligned");
  DVSG_REQUIRE(B > 0 && H > 0 && W > 0 && stride >= 1 && res_stride >= 1, "dvsg_conv_gemm: bad shape");
  ConvGemm p;
  p.math = math;
  p.x = x; p.w.rows = wt; p.bias = bias; p.res = res; p.y = y;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.Ho = (H - 1) / stride + 1; p.Wo = (W - 1) / stride + 1;
  p.ksize = ksize; p.stride = stride; p.pad = ksize == 3 ? 1 : 0;
  p.res_H = (p.Ho - 1) * res_stride + 1; p.res_W = (p.Wo - 1) * res_stride + 1;
  p.res_stride = res_stride;
  p.relu = relu;
  const size_t cbytes = align256((size_t)kSplitKMaxTiles * sizeof(int));
  if (scratch && scratch_bytes > cbytes) {  // [tickets | partial-tile slabs]
    if (int rc = launch_zero_tickets(static_cast<int *>(scratch), cbytes / sizeof(int), as_stream(stream))) return rc;
    p.splitk_counters = static_cast<int *>(scratch);
    p.splitk_scratch = static_cast<char *>(scratch) + cbytes;
    // the partial-tile slabs own at most kSplitKSlabBytes behind the tickets: whatever the caller's scratch holds beyond
    // that may carry the packed weight copies below, which a slab user sizing itself by this field must never reach
    p.splitk_scratch_bytes = std::min(scratch_bytes - cbytes, align256(kSplitKSlabBytes));
  }
  const bool pairs = math == kMathF16Pairs;
  if (storage_of(math) == kF16 && Cin % 64 == 0 && Cout % (pairs ? 64 : 128) == 0 && (ksize == 1 || ksize == 3) && scratch) {
    // the packed weight copies conv_gemm_wide16.hip prefers (what dvsg_locnet_create makes once per layer), made here on
    // every call behind the tickets and the partial-tile slabs when the caller's scratch has room for them; without
    // them the layer runs from the [rows][K] layout
    const int rows = pairs ? 2 * Cout : Cout;   // stacked hi / lo rows, or plain ones
    const size_t need = align256(wide16_packed_bytes(rows, Cin, ksize));
    const size_t base = cbytes + align256(kSplitKSlabBytes);
    if (scratch_bytes >= base + 3 * need) {
      char *pk = static_cast<char *>(scratch) + base;
      if (int rc = launch_pack_wide16(wt, pk, rows, Cin, ksize, 0, as_stream(stream))) return rc;
      p.w.packed = pk;
      if (ksize == 1) {
        p.w.packed_a = pk;
      } else {
        if (int rc = launch_pack_wide16(wt, pk + need, rows, Cin, ksize, 1, as_stream(stream))) return rc;
        if (int rc = launch_pack_wide16(wt, pk + 2 * need, rows, Cin, ksize, 2, as_stream(stream))) return rc;
        p.w.packed_a = pk + need;
        p.w.packed_h = pk + 2 * need;
      }
    }
  }
  return launch_conv_gemm(p, as_stream(stream));
}

// dvsg_locnet_forward_<prec> / dvsg_locnet_forward_tap_<prec> (`fn` names the entry point in the messages)
int forward_entry(const char *fn, int prec, const dvsg_locnet *net, const float *patches, int B, int H, int W, float *F_t,
                  void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(F_t, "%s: NULL F_t", fn);
  return forward(net, prec, patches, B, H, W, F_t, -1, nullptr, 0, nullptr, workspace, workspace_bytes, as_stream(stream),
                 nullptr);
}

int forward_tap_entry(const char *fn, int prec, const dvsg_locnet *net, const float *patches, int B, int H, int W, int stage,
                      float *act_out, size_t act_out_bytes, int *act_dims_host, void *workspace, size_t workspace_bytes,
                      void *stream) {
  DVSG_REQUIRE(act_out && act_dims_host, "%s: NULL pointer", fn);
  DVSG_REQUIRE(stage >= 0 && stage <= 18, "%s: stage %d outside [0,18]", fn, stage);
  return forward(net, prec, patches, B, H, W, nullptr, stage, act_out, act_out_bytes, act_dims_host, workspace,
                 workspace_bytes, as_stream(stream), nullptr);
}

// The ConvFused of dvsg_conv3x3_1x1_f32, dvsg_conv3x3_1x1_f32x3 and dvsg_debug_conv3x3_1x1, as forward() fills it for block
// 1's units (`fn` names the entry point in the messages).  The residual is the tensor `res`, or, with sc_x, the 1x1
// shortcut conv of sc_x computed in the kernel.
int fused_op(const char *fn, ConvMath math, const void *x, const void *wt2, const float *bias2, const void *wt3, const float *bias3,
             const void *res, const void *sc_x, const void *sc_wt, const float *sc_bias, int sc_cin, void *y, int B, int H,
             int W, int Cin, int Cout, int stride, int res_stride, void *stream) {
  DVSG_REQUIRE(B > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2) && res_stride >= 1,
               "%s: bad shape B=%d H=%d W=%d stride=%d res_stride=%d", fn, B, H, W, stride, res_stride);
  ConvFused f;
  f.math = math;
  f.x = x; f.wt2 = wt2; f.bias2 = bias2; f.wt3 = wt3; f.bias3 = bias3;
  f.res = res; f.y = y;
  f.B = B; f.H = H; f.W = W; f.Cin = Cin; f.Cout = Cout;
  f.Ho = (H - 1) / stride + 1; f.Wo = (W - 1) / stride + 1;
  f.stride = stride;
  f.res_H = (f.Ho - 1) * res_stride + 1; f.res_W = (f.Wo - 1) * res_stride + 1; f.res_stride = res_stride;
  if (sc_x) {
    f.res = nullptr;
    f.sc_x = sc_x; f.sc_wt = sc_wt; f.sc_bias = sc_bias;
    f.sc_cin = sc_cin;
  }
  return launch_conv3x3_1x1(f, as_stream(stream));
}

// dvsg_debug_set_option: every switch's name, its member of g_opt, and what a value is normalised to before it is stored
int opt_any(int v) { return v; }
int opt_flag(int v) { return v != 0; }
int opt_positive(int v) { return v > 0 ? v : 1; }
int opt_mask16(int v) { return v & 0xFFFF; }
constexpr struct {
  const char *name;
  int DebugOptions::*member;
  int (*normalise)(int);
} kDebugOptions[] = {
    {"conv_variant", &DebugOptions::conv_variant, opt_any},
    {"conv1_variant", &DebugOptions::conv1_variant, opt_any},
    {"root_pool", &DebugOptions::root_pool, opt_any},
    {"wide16_min_tiles", &DebugOptions::wide16_min_tiles, opt_any},
    {"wide16_packed", &DebugOptions::wide16_packed, opt_any},
    {"wide16_arows", &DebugOptions::wide16_arows, opt_any},
    {"wide16_hreuse", &DebugOptions::wide16_hreuse, opt_any},
    {"fused_hreuse", &DebugOptions::fused_hreuse, opt_any},
    {"fuse_conv", &DebugOptions::fuse_conv, opt_any},
    {"fuse_shortcut", &DebugOptions::fuse_shortcut, opt_flag},
    {"concat_sc", &DebugOptions::concat_sc, opt_flag},
    {"x3_conv1", &DebugOptions::x3_conv1, opt_any},
    {"x3_fuse", &DebugOptions::x3_fuse, opt_any},
    {"f16_split", &DebugOptions::f16_split, opt_flag},
    {"f16_pair_mask", &DebugOptions::f16_pair_mask, opt_mask16},
    {"flow_tiled", &DebugOptions::flow_tiled, opt_any},
    {"flow_rounds", &DebugOptions::flow_rounds, opt_positive},
    {"warp_xcd", &DebugOptions::warp_xcd, opt_flag},
};

}  // namespace
}  // namespace dvsg

using namespace dvsg;

extern "C" {

int dvsg_locnet_create(int n_arrays, const char *const *names, const float *const *host_data, const int *ndims,
                       const int64_t *dims, dvsg_locnet_t **out) {
  DVSG_REQUIRE(names && host_data && ndims && dims && out && n_arrays > 0, "dvsg_locnet_create: bad arguments");
  *out = nullptr;
  ArrayMap m;
  for (int i = 0; i < n_arrays; ++i) {
    DVSG_REQUIRE(names[i] && host_data[i] && ndims[i] >= 1 && ndims[i] <= 4, "dvsg_locnet_create: bad array %d", i);
    std::string name(names[i]);
    if (name.size() > 2 && name.compare(name.size() - 2, 2, ":0") == 0) name.resize(name.size() - 2);
    HostArray a;
    a.data = host_data[i];
    a.nd = ndims[i];
    for (int j = 0; j < 4; ++j) a.dims[j] = j < a.nd ? dims[(size_t)i * 4 + j] : 1;
    m[name] = a;
  }
  const std::string rn = std::string(kPrefix) + "resnet_v1_50";
  auto it = m.find(rn + "/conv1/weights");
  if (it == m.end()) return fail(DVSG_ERR_WEIGHTS, "checkpoint array missing: %s/conv1/weights", rn.c_str());
  if (it->second.nd != 4) return fail(DVSG_ERR_WEIGHTS, "conv1/weights must be 4-D");
  const int c_in = (int)it->second.dims[2];
  if (c_in < 3 || c_in > 3 * kRootMaxFrames || c_in % 3 != 0)
    return fail(DVSG_ERR_UNSUPPORTED, "conv1 has %d input channels; this build supports windows of S RGB frames, c_in = 3 S, S <= %d",
                c_in, kRootMaxFrames);

  dvsg_locnet *net = new dvsg_locnet();
  net->c_in = c_in;
  int rc = DVSG_OK;
  auto bail = [&](int code) {
    dvsg_locnet_destroy(net);
    return code;
  };
  net->conv1 = ConvLayer{7, c_in, 64, 2, true};
  if ((rc = make_conv1(net, m, rn + "/conv1", &net->conv1))) return bail(rc);
  if ((rc = c_in != kConv1Cin ? prepare_rootconv() : prepare_root_band())) return bail(rc);
  int depth_in = 64;
  for (const BlockSpec &bs : kBlocks) {
    for (int u = 1; u <= bs.units; ++u) {
      Unit unit;
      unit.block = (int)(&bs - kBlocks);
      unit.base = bs.base;
      unit.depth = bs.base * 4;
      unit.stride = u == bs.units ? bs.last_stride : 1;
      unit.has_shortcut = depth_in != unit.depth;
      const std::string sc = rn + "/" + bs.name + "/unit_" + std::to_string(u) + "/bottleneck_v1";
      if (unit.has_shortcut) {
        if (unit.stride != 1) return bail(fail(DVSG_ERR_UNSUPPORTED, "strided shortcut conv not expected in resnet_v1_50"));
        unit.shortcut = ConvLayer{1, depth_in, unit.depth, 1, false};
        if ((rc = make_conv(net, m, sc + "/shortcut", &unit.shortcut))) return bail(rc);
      }
      unit.c1 = ConvLayer{1, depth_in, bs.base, 1, true};
      unit.c2 = ConvLayer{3, bs.base, bs.base, unit.stride, true};
      unit.c3 = ConvLayer{1, bs.base, unit.depth, 1, false};
      if ((rc = make_conv(net, m, sc + "/conv1", &unit.c1))) return bail(rc);
      if ((rc = make_conv(net, m, sc + "/conv2", &unit.c2))) return bail(rc);
      if ((rc = make_conv(net, m, sc + "/conv3", &unit.c3))) return bail(rc);
      if (unit.has_shortcut && unit.shortcut.cin % 64 == 0 && unit.shortcut.cin > 64) {
        // [shortcut rows | conv1 rows]: device-to-device copies of the two layers' float32 rows, f32s pieces and biases
        const ConvLayer &a = unit.shortcut, &b = unit.c1;
        unit.cat = ConvLayer{1, a.cin, a.cout + b.cout, 1, false};
        const size_t ka = (size_t)a.cout * a.cin, kb = (size_t)b.cout * b.cin;
        ConvLayer &c = unit.cat;
        if ((rc = device_alloc(net, (ka + kb) * sizeof(float), &c.wt))) return bail(rc);
        if ((rc = device_alloc(net, 2 * (ka + kb) * sizeof(_Float16), &c.wt32s))) return bail(rc);
        if ((rc = device_alloc(net, (a.cout + b.cout) * sizeof(float), &c.bias))) return bail(rc);
        if ((rc = device_alloc(net, 6 * (ka + kb), &c.wt3x))) return bail(rc);
        hipError_t e = hipMemcpy(c.wt, a.wt, ka * sizeof(float), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(c.wt + ka, b.wt, kb * sizeof(float), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(c.wt32s, a.wt32s, 2 * ka * sizeof(_Float16), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(c.wt32s + 2 * ka, b.wt32s, 2 * kb * sizeof(_Float16), hipMemcpyDeviceToDevice);
        // (the f32x3 packing is by groups of 64 rows: the two layers' packed stages one behind the other)
        if (e == hipSuccess) e = hipMemcpy(c.wt3x, a.wt3x, 6 * ka, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(c.wt3x + 3 * ka, b.wt3x, 6 * kb, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(c.bias, a.bias, a.cout * sizeof(float), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(c.bias + a.cout, b.bias, b.cout * sizeof(float), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return bail(fail(DVSG_ERR_HIP, "concatenating shortcut | conv1: %s", hipGetErrorString(e)));
        unit.has_cat = true;
      }
      net->units.push_back(unit);
      depth_in = unit.depth;
    }
  }
  for (int i = 0; i < 4; ++i) {
    const std::string sc = std::string(kPrefix) + "df/dense" + std::to_string(i + 1);
    const HostArray *W, *b;
    if ((rc = find(m, sc + "/W", {kDenseDims[i][0], kDenseDims[i][1]}, &W))) return bail(rc);
    if ((rc = find(m, sc + "/b", {kDenseDims[i][1]}, &b))) return bail(rc);
    std::vector<float> hw(W->data, W->data + W->size()), hb(b->data, b->data + b->size());
    if ((rc = upload(net, hw, &net->dense_w[i]))) return bail(rc);
    if ((rc = upload(net, hb, &net->dense_b[i]))) return bail(rc);
  }
  std::vector<float> vs(50);  // model.py:105-110: 5x5 grid on [-1,1]^2, x fastest
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) {
      vs[(i * 5 + j) * 2 + 0] = -1.0f + 0.5f * j;
      vs[(i * 5 + j) * 2 + 1] = -1.0f + 0.5f * i;
    }
  if ((rc = upload(net, vs, &net->v_src))) return bail(rc);
  {  // the TPS system of the constant V_src grid is inverted once (float64)
    void *scratch = nullptr;
    if ((rc = device_alloc(net, 25 * 28 * sizeof(double), &net->winv))) return bail(rc);
    if (hipMalloc(&scratch, 13 * 25 * 2 * sizeof(float)) != hipSuccess) return bail(fail(DVSG_ERR_HIP, "hipMalloc failed"));
    rc = tps_inverse_columns(net->v_src, 25, net->winv, static_cast<float *>(scratch), nullptr);
    (void)hipFree(scratch);
    if (rc) return bail(rc);
  }
  *out = net;
  return DVSG_OK;
}

int dvsg_locnet_in_channels(const dvsg_locnet_t *net) { return net ? base(net)->c_in : 0; }

int dvsg_locnet_workspace_bytes(const dvsg_locnet_t *net, int B, int H, int W, size_t *bytes) {
  DVSG_REQUIRE(net && bytes, "dvsg_locnet_workspace_bytes: NULL pointer");
  DVSG_REQUIRE(B > 0 && H > 0 && W > 0, "dvsg_locnet_workspace_bytes: bad shape B=%d H=%d W=%d", B, H, W);
  *bytes = plan(nullptr, B, H, W).total;
  return DVSG_OK;
}

int dvsg_locnet_forward_f32(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, float *F_t,
                            void *workspace, size_t workspace_bytes, void *stream) {
  return forward_entry("dvsg_locnet_forward_f32", kF32, net, patches, B, H, W, F_t, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_f16(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, float *F_t,
                            void *workspace, size_t workspace_bytes, void *stream) {
  return forward_entry("dvsg_locnet_forward_f16", kF16, net, patches, B, H, W, F_t, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_f32s(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, float *F_t,
                             void *workspace, size_t workspace_bytes, void *stream) {
  return forward_entry("dvsg_locnet_forward_f32s", kF32S, net, patches, B, H, W, F_t, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_f32x3(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, float *F_t,
                              void *workspace, size_t workspace_bytes, void *stream) {
  return forward_entry("dvsg_locnet_forward_f32x3", kF32X, net, patches, B, H, W, F_t, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_tap_f32(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, int stage,
                                float *act_out, size_t act_out_bytes, int *act_dims_host, void *workspace,
                                size_t workspace_bytes, void *stream) {
  return forward_tap_entry("dvsg_locnet_forward_tap_f32", kF32, net, patches, B, H, W, stage, act_out, act_out_bytes,
                           act_dims_host, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_tap_f16(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, int stage,
                                float *act_out, size_t act_out_bytes, int *act_dims_host, void *workspace,
                                size_t workspace_bytes, void *stream) {
  return forward_tap_entry("dvsg_locnet_forward_tap_f16", kF16, net, patches, B, H, W, stage, act_out, act_out_bytes,
                           act_dims_host, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_tap_f32s(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, int stage,
                                 float *act_out, size_t act_out_bytes, int *act_dims_host, void *workspace,
                                 size_t workspace_bytes, void *stream) {
  return forward_tap_entry("dvsg_locnet_forward_tap_f32s", kF32S, net, patches, B, H, W, stage, act_out, act_out_bytes,
                           act_dims_host, workspace, workspace_bytes, stream);
}

int dvsg_locnet_forward_tap_f32x3(const dvsg_locnet_t *net, const float *patches, int B, int H, int W, int stage,
                                  float *act_out, size_t act_out_bytes, int *act_dims_host, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  return forward_tap_entry("dvsg_locnet_forward_tap_f32x3", kF32X, net, patches, B, H, W, stage, act_out, act_out_bytes,
                           act_dims_host, workspace, workspace_bytes, stream);
}

int dvsg_conv_gemm_f32(const float *x, const float *wt, const float *bias, const float *res, float *y, int B, int H,
                       int W, int Cin, int Cout, int ksize, int stride, int relu, int res_stride, void *scratch,
                       size_t scratch_bytes, void *stream) {
  return conv_gemm_op(kMathF32, x, wt, bias, res, y, B, H, W, Cin, Cout, ksize, stride, relu, res_stride, scratch,
                      scratch_bytes, stream);
}

int dvsg_conv_gemm_f16(const void *x, const void *wt, const float *bias, const void *res, void *y, int B, int H,
                       int W, int Cin, int Cout, int ksize, int stride, int relu, int res_stride, void *scratch,
                       size_t scratch_bytes, void *stream) {
  return conv_gemm_op(kMathF16Plain, x, wt, bias, res, y, B, H, W, Cin, Cout, ksize, stride, relu, res_stride, scratch,
                      scratch_bytes, stream);
}

int dvsg_conv_gemm_f32s(const void *x, const void *wt_pieces, const float *bias, const void *res, void *y, int B, int H,
                        int W, int Cin, int Cout, int ksize, int stride, int relu, int res_stride, void *scratch,
                        size_t scratch_bytes, void *stream) {
  return conv_gemm_op(kMathF32S, x, wt_pieces, bias, res, y, B, H, W, Cin, Cout, ksize, stride, relu, res_stride, scratch,
                      scratch_bytes, stream);
}

int dvsg_conv_gemm_f32x3(const float *x, const void *wt_packed, const float *bias, const float *res, float *y, int B, int H,
                         int W, int Cin, int Cout, int ksize, int stride, int relu, int res_stride, void *scratch,
                         size_t scratch_bytes, void *stream) {
  return conv_gemm_op(kMathF32X, x, wt_packed, bias, res, y, B, H, W, Cin, Cout, ksize, stride, relu, res_stride, scratch,
                      scratch_bytes, stream);
}

int dvsg_pack_weights_f32x3(const float *wt, void *wt_packed, int Cout, int K, void *stream) {
  return launch_pack_x3(wt, wt_packed, Cout, K, as_stream(stream));
}

int dvsg_f32_to_pieces(const float *x, void *y, size_t n, void *stream) {
  DVSG_REQUIRE(x && y, "dvsg_f32_to_pieces: NULL pointer");
  return launch_f32_to_p(x, y, n, as_stream(stream));
}

int dvsg_pieces_to_f32(const void *x, float *y, size_t n, void *stream) {
  DVSG_REQUIRE(x && y, "dvsg_pieces_to_f32: NULL pointer");
  return launch_p_to_f32(x, y, n, as_stream(stream));
}

int dvsg_conv_gemm_f16s(const void *x, const void *wt_split, const float *bias, const void *res, void *y, int B, int H,
                        int W, int Cin, int Cout, int ksize, int stride, int relu, int res_stride, void *scratch,
                        size_t scratch_bytes, void *stream) {
  return conv_gemm_op(kMathF16Pairs, x, wt_split, bias, res, y, B, H, W, Cin, Cout, ksize, stride, relu, res_stride, scratch,
                      scratch_bytes, stream);
}

int dvsg_conv3x3_1x1_f32(const float *x, const float *wt2, const float *bias2, const float *wt3, const float *bias3,
                         const float *res, float *y, int B, int H, int W, int Cin, int Cout, int stride, int res_stride,
                         void *stream) {
  DVSG_REQUIRE(x && wt2 && bias2 && wt3 && bias3 && res && y, "dvsg_conv3x3_1x1_f32: NULL pointer");
  return fused_op("dvsg_conv3x3_1x1_f32", kMathF32, x, wt2, bias2, wt3, bias3, res, nullptr, nullptr, nullptr, 0, y, B, H, W, Cin,
                  Cout, stride, res_stride, stream);
}

int dvsg_conv3x3_1x1_f32x3(const float *x, const void *wt2_packed, const float *bias2, const void *wt3_packed, const float *bias3,
                           const float *res, float *y, int B, int H, int W, int Cin, int Cout, int stride, int res_stride,
                           void *stream) {
  DVSG_REQUIRE(x && wt2_packed && bias2 && wt3_packed && bias3 && res && y, "dvsg_conv3x3_1x1_f32x3: NULL pointer");
  return fused_op("dvsg_conv3x3_1x1_f32x3", kMathF32X, x, wt2_packed, bias2, wt3_packed, bias3, res, nullptr, nullptr, nullptr, 0,
                  y, B, H, W, Cin, Cout, stride, res_stride, stream);
}

int dvsg_debug_conv3x3_1x1(int prec, const void *x, const void *wt2, const float *bias2, const void *wt3, const float *bias3,
                           const void *res, const void *sc_x, const void *sc_wt, const float *sc_bias, int sc_cin, void *y, int B,
                           int H, int W, int Cin, int Cout, int stride, int res_stride, void *stream) {
  DVSG_REQUIRE(prec >= kF32 && prec <= kF32X, "dvsg_debug_conv3x3_1x1: unknown precision %d", prec);
  DVSG_REQUIRE(x && wt2 && bias2 && wt3 && bias3 && y, "dvsg_debug_conv3x3_1x1: NULL pointer");
  return fused_op("dvsg_debug_conv3x3_1x1", math_of(prec, true), x, wt2, bias2, wt3, bias3, res, sc_x, sc_wt, sc_bias, sc_cin, y, B, H, W,
                  Cin, Cout, stride, res_stride, stream);
}

int dvsg_debug_last_conv_kernel(int *fields, int n) {
  DVSG_REQUIRE(fields && n >= kConvKernelFields, "dvsg_debug_last_conv_kernel: need room for %d fields", kConvKernelFields);
  std::copy(g_last_conv_kernel, g_last_conv_kernel + kConvKernelFields, fields);
  return DVSG_OK;
}

int dvsg_debug_last_root_kernel(int *fields, int n) {
  DVSG_REQUIRE(fields && n >= kRootKernelFields, "dvsg_debug_last_root_kernel: need room for %d fields", kRootKernelFields);
  std::copy(g_last_root_kernel, g_last_root_kernel + kRootKernelFields, fields);
  return DVSG_OK;
}

int dvsg_debug_last_conv_config(int *fields, int n) {
  DVSG_REQUIRE(fields && n >= kConvConfigFields, "dvsg_debug_last_conv_config: need room for %d fields", kConvConfigFields);
  std::copy(g_last_conv_config, g_last_conv_config + kConvConfigFields, fields);
  return DVSG_OK;
}

int dvsg_debug_set_option(const char *name, int value) {
  DVSG_REQUIRE(name, "dvsg_debug_set_option: NULL name");
  for (const auto &o : kDebugOptions)
    if (std::strcmp(name, o.name) == 0) {
      g_opt.*o.member = o.normalise(value);
      return DVSG_OK;
    }
  return fail(DVSG_ERR_INVALID_ARG, "dvsg_debug_set_option: unknown option %s", name);
}

// Error-feedback rounding of the float16 mode's PLAIN weights (the copies a layer without the lo piece multiplies by).
// A float16 weight is off by up to 2^-12 relative, the same way at every pixel: through the mean activation mu_k of its
// input channel that is a BIAS of its output channel, sum_k (q_k - w_k) mu_k, which the global average pool does not
// average away -- 9/10 of the plain mode's F_t error, and what the hi / lo pairs exist to remove (at twice the MFMAs).
// Here every weight is rounded to one of its two float16 neighbours so that the running sum of (q_k - w_k) mu_k along K
// stays within half a step: the bias goes, the zero-mean part -- which the pool does average -- stays.  mu comes from ONE
// float32 pass over `patches` (calibration windows) with block 1's fusion off, recorded per unit and convolution input.
// mode 0: round to nearest again (undo); 1: mu = 1 (A/B: does nothing for F_t -- channel means are far from uniform);
// 2: calibrated means.  Measured (tools/f16_ef_sweep.py, two 720p windows, synthetic checkpoint): plain weights 1.9e-5 ->
// 2.7e-6 (hi / lo pairs everywhere: 1.6e-6), 22 % less time per step.
static int calibrate_f16(dvsg_locnet *net, const float *patches, int B, int H, int W, int mode, void *workspace,
                         size_t workspace_bytes, hipStream_t s) {
  // "synchronous" in every mode: redo() rewrites the weights with blocking copies on the legacy stream, which do not wait for
  // a non-blocking stream, so a float16 forward still queued on the caller's stream would otherwise run on the new weights
  DVSG_HIP(hipStreamSynchronize(s));
  std::vector<double> mu((size_t)48 * 2048, 1.0);
  double rows[48] = {0};
  if (mode == 2) {   // calibrated channel means
    Calib calib;   // the recorder of this pass alone: forward() of other handles and threads never see it
    void *sums = nullptr, *part = nullptr, *F = nullptr;
    hipError_t e = hipMalloc(&sums, 48 * 2048 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&part, (size_t)kCalibBlocks * 2048 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&F, (size_t)B * 50 * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(sums, 0, 48 * 2048 * sizeof(double), s);
    int rc = e == hipSuccess ? DVSG_OK : fail(DVSG_ERR_HIP, "calibration: %s", hipGetErrorString(e));
    if (rc == DVSG_OK) {
      calib.sums = static_cast<double *>(sums);
      calib.part = static_cast<float *>(part);
      rc = forward(net, kF32, patches, B, H, W, static_cast<float *>(F), -1, nullptr, 0, nullptr, workspace, workspace_bytes, s,
                   &calib);   // (with a recorder block 1 runs unfused)
      if (rc == DVSG_OK && hipMemcpyAsync(mu.data(), sums, mu.size() * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(DVSG_ERR_HIP, "copy of the calibration sums failed");
      if (rc == DVSG_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(DVSG_ERR_HIP, "calibration pass failed");
    }
    (void)hipFree(sums);
    (void)hipFree(part);
    (void)hipFree(F);
    if (rc) return rc;
    for (int slot = 0; slot < 48; ++slot)
      for (int c = 0; c < 2048; ++c) mu[(size_t)slot * 2048 + c] = calib.rows[slot] > 0 ? mu[(size_t)slot * 2048 + c] / calib.rows[slot] : 1.0;
    std::copy(calib.rows, calib.rows + 48, rows);
  }
  // kept in the handle, and redo() reads them THERE: what dvsg_debug_calibration_means shows is what the weights were chosen by
  net->calib_mu = mu;
  std::copy(rows, rows + 48, net->calib_rows);
  auto f16_bits = [](_Float16 v) { unsigned short b; std::memcpy(&b, &v, 2); return b; };
  auto f16_from = [](unsigned short b) { _Float16 v; std::memcpy(&v, &b, 2); return v; };
  auto neighbour = [&](_Float16 q, bool up) -> _Float16 {   // next float16 above / below q
    unsigned short b = f16_bits(q);
    if ((b & 0x7fff) == 0) return f16_from(up ? 0x0001 : 0x8001);
    const bool neg = (b & 0x8000) != 0;
    b = (unsigned short)((up != neg) ? b + 1 : b - 1);
    return f16_from(b);
  };
  auto redo = [&](ConvLayer &L, const double *m) -> int {
    const int K = L.ksize * L.ksize * L.cin;
    std::vector<float> wt((size_t)L.cout * K);
    DVSG_HIP(hipMemcpy(wt.data(), L.wt, wt.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<_Float16> q16(wt.size());
    for (int n = 0; n < L.cout; ++n) {
      double E = 0.0;
      for (int k = 0; k < K; ++k) {
        const float w32 = wt[(size_t)n * K + k];
        const _Float16 q0 = (_Float16)w32;
        _Float16 q = q0;
        if (mode != 0 && (float)q0 != w32) {
          const _Float16 other = neighbour(q0, (float)q0 < w32);
          const double mk = m[k % L.cin];                  // k = (kh, kw, c): the channel's mean for every tap
          const double e0 = E + ((double)(float)q0 - w32) * mk, e1 = E + ((double)(float)other - w32) * mk;
          const bool take = std::fabs(e1) < std::fabs(e0) && std::isfinite((float)other);
          q = take ? other : q0;
          E = take ? e1 : e0;
        }
        q16[(size_t)n * K + k] = q;
      }
    }
    DVSG_HIP(hipMemcpy(L.wt16, q16.data(), q16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    return pack_plain(net, &L);
  };
  int ui = 0;
  for (Unit &u : net->units) {
    const double *mx = net->calib_mu.data() + (size_t)(3 * ui) * 2048;
    if (u.has_shortcut) if (int rc = redo(u.shortcut, mx)) return rc;
    if (int rc = redo(u.c1, mx)) return rc;
    if (int rc = redo(u.c2, mx + 2048)) return rc;
    if (int rc = redo(u.c3, mx + 2 * 2048)) return rc;
    ++ui;
  }
  return DVSG_OK;
}

int dvsg_locnet_calibrate_f16(dvsg_locnet_t *net, const float *patches, int B, int H, int W, void *workspace,
                              size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(net && workspace, "dvsg_locnet_calibrate_f16: NULL pointer");
  DVSG_REQUIRE(!net->parent, "dvsg_locnet_calibrate_f16: net is a view; calibrate its parent");
  if (!patches) {   // undo: round-to-nearest plain copies, pairs everywhere
    net->f16_pair_mask = 0xFFFF;
    return calibrate_f16(net, nullptr, 0, 0, 0, 0, workspace, workspace_bytes, as_stream(stream));
  }
  DVSG_REQUIRE(B > 0 && H > 0 && W > 0, "dvsg_locnet_calibrate_f16: bad shape B=%d H=%d W=%d", B, H, W);
  if (int rc = calibrate_f16(net, patches, B, H, W, 2, workspace, workspace_bytes, as_stream(stream))) return rc;
  net->f16_pair_mask = 0x1111;   // block 1 (whose fused kernels multiply by the stacked pairs) keeps them; blocks 2-4 run plain
  return DVSG_OK;
}

int dvsg_debug_calibrate_f16_weights(dvsg_locnet_t *net, const float *patches, int B, int H, int W, int mode, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(net && patches && workspace && mode >= 0 && mode <= 2, "dvsg_debug_calibrate_f16_weights: bad arguments");
  DVSG_REQUIRE(!net->parent, "dvsg_debug_calibrate_f16_weights: net is a view; calibrate its parent");
  return calibrate_f16(net, patches, B, H, W, mode, workspace, workspace_bytes, as_stream(stream));
}

int dvsg_debug_calibration_means(const dvsg_locnet_t *net, double *means, double *rows) {
  DVSG_REQUIRE(net && means && rows, "dvsg_debug_calibration_means: NULL pointer");
  net = base(net);
  std::copy(net->calib_mu.begin(), net->calib_mu.end(), means);
  std::copy(net->calib_rows, net->calib_rows + 48, rows);
  return DVSG_OK;
}

int dvsg_debug_plain_weights_f16(const dvsg_locnet_t *net, int unit, int kind, void *w16, size_t w16_bytes, int *dims) {
  DVSG_REQUIRE(net && dims, "dvsg_debug_plain_weights_f16: NULL pointer");
  net = base(net);
  DVSG_REQUIRE(unit >= 0 && unit < (int)net->units.size(), "dvsg_debug_plain_weights_f16: unit %d outside 0..%d", unit,
               (int)net->units.size() - 1);
  DVSG_REQUIRE(kind >= kKindC1 && kind <= kKindSc, "dvsg_debug_plain_weights_f16: kind %d outside 0..3", kind);
  const Unit &u = net->units[unit];
  DVSG_REQUIRE(kind != kKindSc || u.has_shortcut, "dvsg_debug_plain_weights_f16: unit %d has no shortcut convolution", unit);
  const ConvLayer &L = kind == kKindC1 ? u.c1 : kind == kKindC2 ? u.c2 : kind == kKindC3 ? u.c3 : u.shortcut;
  const int K = L.ksize * L.ksize * L.cin;
  dims[0] = L.cout; dims[1] = K; dims[2] = L.cin;
  if (!w16) return DVSG_OK;
  const size_t bytes = (size_t)L.cout * K * sizeof(_Float16);
  DVSG_REQUIRE(w16_bytes >= bytes, "dvsg_debug_plain_weights_f16: buffer %zu bytes < %zu", w16_bytes, bytes);
  DVSG_HIP(hipMemcpy(w16, L.wt16, bytes, hipMemcpyDeviceToHost));
  return DVSG_OK;
}

int dvsg_stabilize_f32(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B, int H, int W,
                       float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace, size_t workspace_bytes,
                       void *stream) {
  return stabilize(net, kF32, patches_t, u_t, nullptr, B, H, W, s_t_pred, F_t, x_s, y_s, workspace, workspace_bytes, stream);
}

int dvsg_stabilize_f32s(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B, int H, int W,
                        float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace, size_t workspace_bytes,
                        void *stream) {
  return stabilize(net, kF32S, patches_t, u_t, nullptr, B, H, W, s_t_pred, F_t, x_s, y_s, workspace, workspace_bytes, stream);
}

int dvsg_stabilize_f16(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B, int H, int W,
                       float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace, size_t workspace_bytes,
                       void *stream) {
  return stabilize(net, kF16, patches_t, u_t, nullptr, B, H, W, s_t_pred, F_t, x_s, y_s, workspace, workspace_bytes, stream);
}

int dvsg_stabilize_f32x3(const dvsg_locnet_t *net, const float *patches_t, const float *u_t, int B, int H, int W,
                         float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace, size_t workspace_bytes,
                         void *stream) {
  return stabilize(net, kF32X, patches_t, u_t, nullptr, B, H, W, s_t_pred, F_t, x_s, y_s, workspace, workspace_bytes, stream);
}

static int ring_precision(int precision) {
  return precision == DVSG_PRECISION_F32 ? kF32 : precision == DVSG_PRECISION_F16 ? kF16 : precision == DVSG_PRECISION_F32S ? kF32S
         : precision == DVSG_PRECISION_F32X3 ? kF32X : -1;
}

int dvsg_stabilize_ring_f32(const dvsg_locnet_t *net, int precision, const float *pool, int n_pool, const int32_t *table,
                            int B, int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace,
                            size_t workspace_bytes, void *stream) {
  return stabilize_ring(net, ring_precision(precision), pool, 0, n_pool, table, nullptr, B, H, W, s_t_pred, F_t, x_s, y_s,
                        workspace, workspace_bytes, stream);
}

int dvsg_stabilize_ring_u8(const dvsg_locnet_t *net, int precision, const uint8_t *pool, int n_pool, const int32_t *table,
                           int B, int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s, void *workspace,
                           size_t workspace_bytes, void *stream) {
  return stabilize_ring(net, ring_precision(precision), pool, 1, n_pool, table, nullptr, B, H, W, s_t_pred, F_t, x_s, y_s,
                        workspace, workspace_bytes, stream);
}

// dvsg_stabilize_ring_f32 with the result of window b written into pool frame out_slots[b]: the write-back of eval.py:116
// for streams whose history lives in the pool (coupe.dvsg_amd.online).  The contract of the header (distinct out slots,
// none of them read by `table`) is the caller's; it is not checked on the device.
int dvsg_stabilize_ring_inplace_f32(const dvsg_locnet_t *net, int precision, float *pool, int n_pool, const int32_t *table,
                                    const int32_t *out_slots, int B, int H, int W, float *F_t, float *x_s, float *y_s,
                                    void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(out_slots, "dvsg_stabilize_ring_inplace_f32: NULL out_slots");
  return stabilize_ring(net, ring_precision(precision), pool, 0, n_pool, table, nullptr, B, H, W, pool, F_t, x_s, y_s,
                        workspace, workspace_bytes, stream, out_slots);
}

// eval_train.py's evaluation graph (:25-51): F_t = localizationNet(patches_t * mask), the warp on the unmasked u_t.
int dvsg_stabilize_masked_f32(const dvsg_locnet_t *net, int precision, const float *patches_t, const float *u_t,
                              const float *mask, int B, int H, int W, float *s_t_pred, float *F_t, float *x_s, float *y_s,
                              void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(mask, "dvsg_stabilize_masked_f32: NULL mask");
  return stabilize(net, ring_precision(precision), patches_t, u_t, mask, B, H, W, s_t_pred, F_t, x_s, y_s, workspace,
                   workspace_bytes, stream);
}

int dvsg_stabilize_ring_masked_f32(const dvsg_locnet_t *net, int precision, const float *pool, int n_pool,
                                   const int32_t *table, const float *mask, int B, int H, int W, float *s_t_pred, float *F_t,
                                   float *x_s, float *y_s, void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(mask, "dvsg_stabilize_ring_masked_f32: NULL mask");
  return stabilize_ring(net, ring_precision(precision), pool, 0, n_pool, table, mask, B, H, W, s_t_pred, F_t, x_s, y_s,
                        workspace, workspace_bytes, stream);
}

int dvsg_stabilize_ring_masked_u8(const dvsg_locnet_t *net, int precision, const uint8_t *pool, int n_pool,
                                  const int32_t *table, const float *mask, int B, int H, int W, float *s_t_pred, float *F_t,
                                  float *x_s, float *y_s, void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(mask, "dvsg_stabilize_ring_masked_u8: NULL mask");
  return stabilize_ring(net, ring_precision(precision), pool, 1, n_pool, table, mask, B, H, W, s_t_pred, F_t, x_s, y_s,
                        workspace, workspace_bytes, stream);
}

// The CNN alone on a masked source -- F_t [B,25,2] into `out` (stage = -1) or the parity tap of `stage` (0..18).
// src_kind 0: `src` is a window tensor [B,H,W,c_in] (n_pool, table unused); 1 / 2: a float32 / uint8 frame pool + table [B,c_in/3].
int dvsg_locnet_forward_masked(const dvsg_locnet_t *net, int precision, const void *src_ptr, int src_kind, int n_pool,
                               const int32_t *table, const float *mask, int B, int H, int W, int stage, float *out,
                               size_t out_bytes, int *act_dims_host, void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(net && src_ptr && mask && out, "dvsg_locnet_forward_masked: NULL pointer");
  DVSG_REQUIRE(src_kind >= 0 && src_kind <= 2 && (src_kind == 0 || (table && n_pool > 0)),
               "dvsg_locnet_forward_masked: bad source (kind %d)", src_kind);
  DVSG_REQUIRE(stage >= -1 && stage <= 18 && (stage < 0 || act_dims_host), "dvsg_locnet_forward_masked: stage %d outside [-1,18]", stage);
  DVSG_REQUIRE(stage >= 0 || out_bytes >= (size_t)B * 50 * sizeof(float), "dvsg_locnet_forward_masked: F_t needs B*50 floats");
  const int prec = ring_precision(precision);
  DVSG_REQUIRE(prec >= 0, "dvsg_locnet_forward_masked: unknown precision %d", precision);
  Conv1Src src{src_ptr, src_kind ? table : nullptr, src_kind ? n_pool : 0};
  src.mask = mask;
  return forward(net, prec, src, src_kind, B, H, W, stage < 0 ? out : nullptr, stage, stage < 0 ? nullptr : out, out_bytes,
                 act_dims_host, workspace, workspace_bytes, as_stream(stream), nullptr);
}

int dvsg_locnet_forward_ring(const dvsg_locnet_t *net, int precision, const void *pool, int pool_is_u8, int n_pool,
                             const int32_t *table, int B, int H, int W, int stage, float *out, size_t out_bytes,
                             int *act_dims_host, void *workspace, size_t workspace_bytes, void *stream) {
  DVSG_REQUIRE(pool && table && out && n_pool > 0, "dvsg_locnet_forward_ring: bad arguments");
  DVSG_REQUIRE(stage >= -1 && stage <= 18 && (stage < 0 || act_dims_host), "dvsg_locnet_forward_ring: stage %d outside [-1,18]", stage);
  DVSG_REQUIRE(stage >= 0 || out_bytes >= (size_t)B * 50 * sizeof(float), "dvsg_locnet_forward_ring: F_t needs B*50 floats");
  const int prec = ring_precision(precision);
  DVSG_REQUIRE(prec >= 0, "dvsg_locnet_forward_ring: unknown precision %d", precision);
  const Conv1Src src{pool, table, n_pool};
  return forward(net, prec, src, pool_is_u8 ? kSrcRingU8 : kSrcRingF32, B, H, W, stage < 0 ? out : nullptr, stage,
                 stage < 0 ? nullptr : out, out_bytes, act_dims_host, workspace, workspace_bytes, as_stream(stream), nullptr);
}

}  // extern "C"
