// NSF_AR.forward (torch_mnf/flows/spline_flow.py:199-216: z -> x, the direction sampling runs through and the density
// pass of an NSF_AR used the IAF way round) on the f16 matrix pipe (mnf_rt.h), weights read from the plain `flat` vector in
// mnf_nsf_ar's own layout (mnf_nsf_ar_rt.h ArLayout).  Element e's conditioner reads the layer's already decoded OUTPUT:
// x_e, ld_e = RQS_inverse(z_e; net_e(x[:, :e])), element 0 from init_param, log_det = sum_e ld_e.  The total matrix work
// equals the one-pass direction's (mnf_nsf_ar_rt.hip); only the order is forced, so the four-nets-side-by-side net of that
// kernel is not available here: ONE net of at most 16 units per step, i.e. one unit tile (Hidden<1, NTL>).
//
// A wave owns kArSeqTiles 16-row tiles (two: 32 rows).  Two lane layouts alternate:
//   * matrix phases: lane (j, q) is row j of EVERY tile of the wave (the B operand's column j), as in every mnf_rt.h kernel;
//   * spline phase: lane (j, q) owns row j of tile q (lanes q >= kArSeqTiles idle: with four tiles all 64 lanes work, and the
//     kernel measures slower, profiles/r19/README.md), so the spline (mnf_nsf_spline.h, INV) runs once per element and wave.  The output layer is staged with block row 4 q' + r' of valid parameter tile t' = position 4 t' + r' for
//     EVERY q': after the tile's products each of the four lanes of row j holds the same four parameters, and a lane keeps
//     those of the row tile t == q (a select).
// The waves of a workgroup walk the elements together: net e (its first layer's K-steps over columns < e, its hidden
// layers, its valid output tiles: steps32(e) + n_hidden - 1 + TV blocks of 2 KB) is ONE chunk of Source<false>'s two LDS
// buffers, one barrier per element.  Element 0 stages nothing.  The decoded values sit in a per-wave LDS slab, float4
// (column group g, row R = 16 t + j of the wave) at slab[16 NTL g + R]; only the wave's own lanes read and write it, a wave's
// LDS accesses execute in order, so the dim steps need no barrier beyond the staging one.  "Columns >= e are 0" is a
// select on the value read: the slab is never cleared.  Every x_e goes to y as well (four columns per store); y is not
// read back.  Rows past the end compute on the last row (clamped) and store nothing.
//
// A row holding a NaN in z[:, i]: the spline hands a NaN through (outside the tail bound: identity), x[:, :i] was decoded
// before and is untouched, every later net of the row reads the NaN and x[:, i:] is NaN; the row is one COLUMN of the
// matrix products, so the other rows of its tile do not notice (the rescue path of the first layer re-splits them at the
// scale they had).
#include <hip/hip_runtime.h>

#include <cstring>

#include "mnf_nsf_ar_rt.h"
#include "mnf_nsf_spline.h"

#ifndef MNF_NSF_AR_SEQ_TILES
#define MNF_NSF_AR_SEQ_TILES 2  // row tiles per wave (1 / 2 / 4: the spline phase uses 16 lanes per tile; profiles/r19/README.md)
#endif

namespace mnf {

constexpr int kArSeqTiles = MNF_NSF_AR_SEQ_TILES;
constexpr int kArSeqMaxWaves = 8;
constexpr int kArSeqMaxDim = 128;  // (slab: 64 B per column, tile and wave; first layer: steps32(dim - 1) blocks per buffer)
static_assert(kArSeqTiles == 1 || kArSeqTiles == 2 || kArSeqTiles == 4, "a lane's spline row is tile q");

// the K that ship (a uniform switch in the kernel; the reference's default and its tests' K first)
__host__ __device__ constexpr bool ar_seq_has_k(int K) { return K == 5 || K == 8; }
__host__ __device__ inline int ar_seq_out_tiles(int K) { return 2 * ((K + 3) >> 2) + ((K + 2) >> 2); }

struct NsfArSeqRtArgs {
  const float* x;
  float* y;
  float* log_det;
  const float* flat;
  int64_t rows;
  int accumulate, vec;  // vec: the rows of y are 16-byte aligned (dwordx4 stores)
  float T;
  int cb, bt;  // blocks / bias tiles per streaming buffer: one whole net
  int block_words, bias_words, slab_words;  // slab_words: per wave
  ArLayout L;
};

// Net e as one chunk: block b = K-step b of the first layer (b < KS0), then hidden layer b - KS0 + 1, then valid output
// tile b - KS0 - (n_hidden - 1).  A wave converts whole blocks: every branch on b is uniform.
struct ArSeqNetFetch {
  const float* flat;
  const ArLayout* L;
  int e, KS0;
  static constexpr int R0 = 1 << 30, R1 = 1 << 30;  // (the block index is the first digit)
  __device__ __forceinline__ void load(int b, int, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int nh = L->n_hidden;
    if (b < KS0) {  // row i of net e against the columns 32 b .. of x[:, :e]
      const bool ok = i < L->hid[0];
      rt::load_row8(flat + L->n.base(e) + (ok ? i : 0) * e, ok, 32 * b, e, false, q, va, vb);
    } else if (b < KS0 + nh - 1) {
      const int l = b - KS0 + 1, hin = L->hid[l - 1];
      const bool ok = i < L->hid[l];
      rt::load_row8(flat + L->n.rest(e) + L->cw[l] + (ok ? i : 0) * hin, ok, 0, hin, false, q, va, vb);
    } else {  // block row i = 4 q' + r': the weight row of position 4 t' + r', whatever q'
      const int K = L->K, hin = L->hid[nh - 1];
      const int pos = 4 * ar_tile_of(b - KS0 - (nh - 1), K) + (i & 3), c = pos >> 4, kk = pos & 15;
      const bool ok = kk < (c < 2 ? K : K - 1);
      rt::load_row8(flat + L->n.rest(e) + L->cw[nh] + (ok ? c * K + kk : 0) * hin, ok, 0, hin, false, q, va, vb);
    }
  }
};
struct ArSeqNetBias {  // tile t < n_hidden: layer t's bias; then the valid output tiles', arranged as their blocks
  const float* flat;
  const ArLayout* L;
  int e;
  __device__ __forceinline__ float operator()(int t, int u) const {
    const int nh = L->n_hidden, K = L->K;
    int at;
    bool ok;
    if (t < nh) {
      ok = u < L->hid[t];
      at = L->cb[t] + u;
    } else {
      const int pos = 4 * ar_tile_of(t - nh, K) + (u & 3), c = pos >> 4, kk = pos & 15;
      ok = kk < (c < 2 ? K : K - 1);
      at = L->cb[nh] + c * K + kk;
    }
    const float v = flat[L->n.rest(e) + (ok ? at : 0)];
    return ok ? v : 0.f;
  }
};

// Net e up to its last hidden vector for the wave's NTL tiles, lane (j, q) = row j of every tile; the input is read from
// the slab (columns < e).
template <int NTL>
__device__ __forceinline__ void ar_seq_hidden(const NsfArSeqRtArgs& a, const rt::Chunk& c, int e, int KS0, float wup, int lane,
                                              int j, int q, const f32x4* slab4, rt::Hidden<1, NTL>& h) {
  using namespace rt;
  const ArLayout& L = a.L;
  const int G = (L.n.dim + 3) >> 2;
  Acc<1, NTL> acc;
  acc.zero();
  float down[NTL];  // the rows' running scale (a power of two <= 1)
#pragma unroll
  for (int t = 0; t < NTL; ++t) down[t] = 1.f;
  for (int ks = 0; ks < KS0; ++ks) {
    const int ga = 8 * ks + q, gb = ga + 4;
    f16x8 bh[NTL], bl[NTL];
    f32x4 xa[NTL], xb[NTL];
    float mx = 0.f;
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      const f32x4 va = slab4[16 * NTL * (ga < G ? ga : 0) + 16 * t + j], vb = slab4[16 * NTL * (gb < G ? gb : 0) + 16 * t + j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xa[t][r] = 4 * ga + r < e ? va[r] : 0.f;  // not yet decoded: 0
        xb[t][r] = 4 * gb + r < e ? vb[r] : 0.f;
      }
      split_kstep(xa[t], xb[t], down[t], bh[t], bl[t], mx);
    }
    if (__builtin_expect(wave_any(!(mx < kSplitLimit)), 0)) {
      // rare: a row at or beyond the split range (or non-finite): its accumulators and every later K-step of it move to
      // a smaller power-of-two scale (exact); finish_layer multiplies the layer's result back (mnf_rt.h first_layer)
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        float fm = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) fm = __builtin_fmaxf(fm, __builtin_fmaxf(finite_abs(xa[t][r]), finite_abs(xb[t][r])));
        const float want = pow2f(-down_exponent(max_over_q(fm), 13));
        if (want < down[t]) {
          const float f = want / down[t];
          acc.main[t][0] *= f;
          acc.corr[t][0] *= f;
          down[t] = want;
        }
        float unused = 0.f;
        split_kstep(xa[t], xb[t], down[t], bh[t], bl[t], unused);
      }
    }
    mac_kstep<1, NTL>(c.A, ks, 1, lane, bh, bl, acc.main, acc.corr);
  }
  float scale[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t) scale[t] = wup / down[t];
  finish_layer<1, NTL>(acc, c.bias, 1, q, scale, true, h);
  for (int l = 1; l < L.n_hidden; ++l) {
    acc.zero();
    f16x8 bh[NTL], bl[NTL];
    hidden_operand<1, NTL>(h, 0, bh, bl);
    mac_kstep<1, NTL>(c.A, KS0 + l - 1, 1, lane, bh, bl, acc.main, acc.corr);
#pragma unroll
    for (int t = 0; t < NTL; ++t) scale[t] = wup * h.up[t];
    finish_layer<1, NTL>(acc, c.bias + 16 * l, 1, q, scale, true, h);
  }
}

// The element's output layer and spline for a compile-time K.  has_net (uniform): the raw parameters are the output
// tiles of the staged net (blocks b0 .., bias tiles bias ..), kept by the lane whose row tile is q; else init_param.
template <int NTL, int K>
__device__ __forceinline__ void ar_seq_out(const NsfArSeqRtArgs& a, bool has_net, const uint32_t* A, int b0, const float* bias,
                                           float wup, int lane, int q, const rt::Hidden<1, NTL>& h, float v, float& out,
                                           float& ld) {
  using namespace rt;
  constexpr int NW_ = (K + 3) / 4, ND_ = (K - 1 + 3) / 4, TV = 2 * NW_ + ND_;  // tiles of widths / heights, derivatives
  float p[3 * K - 1];
  if (has_net) {
    f16x8 bh[NTL], bl[NTL];
    hidden_operand<1, NTL>(h, 0, bh, bl);
    // is[t]: this lane's row tile is t.  The rows' scales go through an empty asm so that the selects below stay selects of
    // registers: left alone they become ONE load at a selected address, which moves the hidden vector into scratch memory
    bool is[NTL];
    float up = 0.f;
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      float ut = h.up[t];
      asm volatile("" : "+v"(ut));
      is[t] = q == t;
      up = t == 0 || is[t] ? ut : up;
    }
    const float scale = wup * up;
#pragma unroll
    for (int tv = 0; tv < TV; ++tv) {
      f16x8 ah, al;
      read_block(A, b0 + tv, lane, ah, al);
      const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 mn = zero4, cr = zero4;
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        f32x4 m = mfma_h(ah, bh[t], zero4), k = mfma_h(ah, bl[t], zero4);
        k = mfma_h(al, bh[t], k);
        const bool mine = t == 0 || is[t];  // (t = 0 first: the later tiles overwrite it where they are the lane's)
        mn = mine ? m : mn;
        cr = mine ? k : cr;
      }
      const f32x4 o = (cr * kSplitInvScale + mn) * scale + *reinterpret_cast<const f32x4*>(bias + 16 * tv + 4 * q);
      const int cgrp = tv < NW_ ? 0 : tv < 2 * NW_ ? 1 : 2, k0 = 4 * (tv - cgrp * NW_);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k0 + i < (cgrp < 2 ? K : K - 1)) p[cgrp * K + k0 + i] = o[i];
      __builtin_amdgcn_sched_barrier(0);  // one tile's products at a time: hoisted together they cost ~30 registers per tile
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3 * K - 1; ++i) p[i] = a.flat[i];
  }
  rqs_regs<K, true, 3 * K - 1>(v, a.T, p, out, ld);
}

template <int NTL>
__device__ __forceinline__ void nsf_ar_seq_rt_block(const NsfArSeqRtArgs& a, rt::Source<false>& src, float wup, int64_t row0,
                                                    float* slab) {
  using namespace rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const ArLayout& L = a.L;
  const int d = L.n.dim, nh = L.n_hidden, K = L.K;
  const bool VEC = a.vec != 0;  // (uniform)
  // the spline phase's row: row j of tile q (lanes q >= NTL have none)
  const int64_t r = row0 + (int64_t)wave * NTL * 16 + 16 * q + j;
  const bool live = q < NTL && r < a.rows;
  const int64_t rc = live ? r : a.rows - 1;
  const float* zrow = a.x + rc * d;
  float* yrow = a.y + rc * d;
  const f32x4* slab4 = reinterpret_cast<const f32x4*>(slab);
  const int own = (16 * (q < NTL ? q : 0) + j) * 4;  // this lane's row in a column group of the slab
  const int TV = ar_seq_out_tiles(K);
  float lad = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  float nz = zrow[0];
#pragma unroll 1
  for (int e = 0; e < d; ++e) {
    const float z = nz;
    nz = zrow[e + 1 < d ? e + 1 : e];  // one element ahead of its use
    const int KS0 = steps32(e);
    Chunk c{nullptr, nullptr};
    Hidden<1, NTL> h;
    if (e > 0) {  // (uniform)
      c = src.template chunk<false>(KS0 + nh - 1 + TV, ArSeqNetFetch{a.flat, &L, e, KS0}, nh + TV, ArSeqNetBias{a.flat, &L, e});
      ar_seq_hidden<NTL>(a, c, e, KS0, wup, lane, j, q, slab4, h);
    } else {
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        h.hi[t][0] = h.lo[t][0] = u32x2{0u, 0u};
        h.up[t] = 1.f;
      }
    }
    float out = 0.f, ld = 0.f;
    switch (K) {  // (uniform)
#define MNF_NSF_AR_SEQ_RT_CASE(KK) \
  case KK: ar_seq_out<NTL, KK>(a, e > 0, c.A, KS0 + nh - 1, c.bias + 16 * nh, wup, lane, q, h, z, out, ld); break;
      MNF_NSF_AR_SEQ_RT_CASE(5) MNF_NSF_AR_SEQ_RT_CASE(8)
#undef MNF_NSF_AR_SEQ_RT_CASE
      default: break;
    }
    lad += ld;
    if (q < NTL) slab[64 * NTL * (e >> 2) + own + (e & 3)] = out;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) o[c4] = c4 == (e & 3) ? out : o[c4];
    if ((e & 3) == 3 || e == d - 1) store4(yrow, e & ~3, d, VEC, live, o);
  }
  if (live && a.log_det) a.log_det[r] = a.accumulate ? a.log_det[r] + lad : lad;
}

template <int NTL>
__global__ void __launch_bounds__(kArSeqMaxWaves * 64) nsf_ar_seq_rt_kernel(NsfArSeqRtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + 16;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  float* slab = bias + a.bias_words + (threadIdx.x >> 6) * a.slab_words;  // this wave's 16 NTL x dim floats
  // one staging exponent per launch: the largest finite WEIGHT of all nets (biases and init_param are not looked at)
  float mx = 0.f;
  for (int e = 1; e < a.L.n.dim; ++e)
    for (int l = 0; l <= a.L.n_hidden; ++l) mx = rt::range_abs_max(a.flat + a.L.w(e, l), a.L.n_in(e, l) * a.L.n_out(l), mx);
  const int ex = rt::weight_exponent(rt::block_weight_max(mx, scratch));
  const float wup = rt::pow2f(ex);
  rt::Source<false> src{blocks, bias, a.cb, a.bt, 0, 0, 0, rt::pow2f(-ex), 0};
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * NTL * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) nsf_ar_seq_rt_block<NTL>(a, src, wup, b * rows_per_block, slab);
}

// The launch of a shape, or false: the VALU kernel takes it.  Fills the kernel arguments' shape part.  One streaming buffer
// holds the largest net (element dim - 1) whole; the largest of 8 / 4 / 2 / 1 waves whose slabs fit next to the two buffers.
static bool nsf_ar_seq_rt_plan(int dim, int K, int n_hidden, const int* hidden, NsfArSeqRtArgs& a, RtPlan& p) {
  ArLayout& L = a.L;
  if (dim > kArSeqMaxDim || !ar_seq_has_k(K) || !ar_layout_plan(dim, K, n_hidden, hidden, L)) return false;
  p.mt_max = 1;
  set_staging(a, p, /*resident=*/false, (dim - 1 + 31) / 32 + n_hidden - 1 + ar_seq_out_tiles(K), n_hidden + ar_seq_out_tiles(K));
  a.slab_words = 64 * kArSeqTiles * ((dim + 3) / 4);
  const size_t slab = (size_t)a.slab_words * 4;
  const int nw = fit_slab_waves(kArSeqMaxWaves, p.lds, slab);
  if (nw < 1) return false;
  p.nw = nw;
  p.lds += nw * slab;
  return true;
}

// the plan's kernel, its dynamic-LDS attribute set
static void (*nsf_ar_seq_rt_kernel_of(const RtPlan&))(NsfArSeqRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, nsf_ar_seq_rt_kernel<kArSeqTiles>);
  return nsf_ar_seq_rt_kernel<kArSeqTiles>;
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_nsf_ar_seq_rt_supported(int dim, int K, int n_hidden, const int* hidden) {
  return rt_has_plan<NsfArSeqRtArgs>(
      [&](NsfArSeqRtArgs& a, RtPlan& p) { return nsf_ar_seq_rt_plan(dim, K, n_hidden, hidden, a, p); });
}

// workgroups of the launch (each walks the row blocks of 16 x tiles x waves rows blockIdx.x, + grid, ...); 0: no launch, or
// no device
extern "C" int64_t mnf_nsf_ar_seq_rt_grid(int64_t rows, int dim, int K, int n_hidden, const int* hidden) {
  return rt_grid_query<NsfArSeqRtArgs>(
      rows, kArSeqTiles, [&](NsfArSeqRtArgs& a, RtPlan& p) { return nsf_ar_seq_rt_plan(dim, K, n_hidden, hidden, a, p); },
      nsf_ar_seq_rt_kernel_of);
}

extern "C" int mnf_nsf_ar_seq_rt(const float* x, float* y, float* log_det, int accumulate, const float* flat, int64_t rows,
                                 int dim, int K, float tail_bound, int n_hidden, const int* hidden, void* stream) {
  if (!x || !y || x == y || !flat || rows < 0 || dim < 1 || K < 1 || !(tail_bound > 0.f) || !hidden_ok(n_hidden, hidden))
    return MNF_ERR_INVALID_ARG;
  if (1e-3 * K > 1.0) return MNF_ERR_DOMAIN;  // spline_flow.py:90-93
  if (rows == 0) return MNF_OK;
  if (rows * dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  NsfArSeqRtArgs a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  if (!nsf_ar_seq_rt_plan(dim, K, n_hidden, hidden, a, p)) return MNF_ERR_UNSUPPORTED;
  a.x = x; a.y = y; a.log_det = log_det; a.flat = flat; a.rows = rows; a.T = tail_bound;
  a.accumulate = accumulate != 0;
  a.vec = dim % 4 == 0 && aligned16(y);
  return launch_plan(nsf_ar_seq_rt_kernel_of(p), a, p, kArSeqTiles, rows, "nsf_ar_seq_rt", (hipStream_t)stream);
}
