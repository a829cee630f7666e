// What the two NSF_AR one-pass kernels share (mnf_nsf_ar_rt.hip: the density direction; mnf_nsf_ar_bwd_rt.hip: its
// gradients): mnf_nsf_ar's layout of `flat`, the staging functors of the block-diagonal "four nets side by side" net of a
// group of four elements, and the group's first and hidden layers.
#pragma once
#include <hip/hip_runtime.h>

#include "mnf_rt_host.h"

namespace mnf {

constexpr int kArStream = 24;  // blocks and bias tiles per streaming buffer (K = 16: 12 output tiles x 2 K-steps)
constexpr int kArMaxHidden = 4;

// mnf_nsf_ar's layout of `flat` (mnf_generic.hip nsf_ar_net): init_param (P = 3K-1 floats), then for e = 1 .. dim-1 the
// state_dict tensors of MLP(e, hidden..., P).  Net e has e * h0 + C floats: its offsets are closed forms in e.
struct ArNets {  // (the part the staging functors carry, by value)
  int dim, P, h0, C;
  __host__ __device__ int base(int e) const { return P + h0 * ((e - 1) * e / 2) + C * (e - 1); }  // layer 0's weights
  __host__ __device__ int rest(int e) const { return base(e) + e * h0; }                          // layer 0's bias
};
struct ArLayout {
  ArNets n;
  int K, n_hidden;
  int hid[kArMaxHidden];
  int cw[kArMaxHidden + 1], cb[kArMaxHidden + 1];  // layer l's weights / bias behind rest(e) (cb[0] = 0)
  __host__ __device__ int w(int e, int l) const { return l ? n.rest(e) + cw[l] : n.base(e); }
  __host__ __device__ int n_in(int e, int l) const { return l ? hid[l - 1] : e; }
  __host__ __device__ int n_out(int l) const { return l < n_hidden ? hid[l] : n.P; }
};

struct NsfArRtArgs {
  const float* x;
  float* y;
  float* log_det;
  const float* flat;
  int64_t rows;
  int accumulate, vec;  // vec: rows are 16-byte aligned (dwordx4 reads of x)
  float T;
  int cb, bt;  // LDS plan (mnf_rt.h Source)
  int block_words, bias_words;
  ArLayout L;
};

// the net (0 .. 3 of the group; 4: padding) that unit / K index o of a side-by-side layer of 4 x w units belongs to
__device__ __forceinline__ int ar_net_of(int o, int w) { return (o >= w) + (o >= 2 * w) + (o >= 3 * w) + (o >= 4 * w); }
// the K index of a lane's e-th weight in K-step ks (convert_block's order)
__device__ __forceinline__ int ar_k_of(int ks, int q, int e) { return 32 * ks + 4 * q + (e < 4 ? e : 12 + e); }

// First layer of group g, walked [K-step][tile]: digits (tile, K-step - ks0).  Block row o = (net q', unit u).
struct ArFirstFetch {
  const float* flat;
  ArNets N;
  int g, hw, R0, ks0;  // hw = hidden[0], R0 = MT
  static constexpr int R1 = 1 << 30;
  __device__ __forceinline__ void load(int m, int ksl, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int o = 16 * m + i, qn = ar_net_of(o, hw), e = 4 * g + qn;
    const bool ok = qn < 4 && e >= 1 && e < N.dim;
    const int ec = ok ? e : 1, u = ok ? o - qn * hw : 0;
    rt::load_row8(flat + N.base(ec) + u * ec, ok, 32 * (ks0 + ksl), ec, false, q, va, vb);  // columns >= e: 0
  }
};
// Layer l >= 1 (hidden -> hidden when l < n_hidden) of group g, the same walk: the diagonal blocks of the four nets.
struct ArHiddenFetch {
  const float* flat;
  ArNets N;
  int g, hin, hout, cw, R0, ks0;  // cw = the layer's ArLayout::cw, R0 = MT
  static constexpr int R1 = 1 << 30;
  __device__ __forceinline__ void load(int m, int ksl, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int o = 16 * m + i, qn = ar_net_of(o, hout), e = 4 * g + qn;
    const bool ok = qn < 4 && e >= 1 && e < N.dim;
    const int ec = ok ? e : 1, u = ok ? o - qn * hout : 0;
    const float* W = flat + N.rest(ec) + cw + u * hin;
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int k = ar_k_of(ks0 + ksl, q, e8), ku = k - qn * hin;
      const bool okk = ok && ku >= 0 && ku < hin;  // the K index is a unit of the same net
      const float v = W[okk ? ku : 0];
      if (e8 < 4) va[e8 & 3] = okk ? v : 0.f;
      else vb[e8 & 3] = okk ? v : 0.f;
    }
  }
};
struct ArHiddenBias {  // layer l (0: the first layer), tile t
  const float* flat;
  ArNets N;
  int g, hout, cb;  // cb = the layer's ArLayout::cb
  __device__ __forceinline__ float operator()(int t, int u) const {
    const int o = 16 * t + u, qn = ar_net_of(o, hout), e = 4 * g + qn;
    const bool ok = qn < 4 && e >= 1 && e < N.dim;
    const float v = flat[ok ? N.rest(e) + cb + (o - qn * hout) : 0];
    return ok ? v : 0.f;
  }
};

// valid parameter tiles of an element: tile t' holds the positions 4 t' .. 4 t' + 3 of 16 c + k (c = widths / heights /
// derivatives), as in mnf_nsf_rt.hip; the tv-th valid one
__device__ __forceinline__ int ar_tile_of(int tv, int K) {
  const int nw = (K + 3) >> 2;
  return tv < nw ? tv : tv < 2 * nw ? 4 + (tv - nw) : 8 + (tv - 2 * nw);
}
// Output layer of group g, walked [valid tile][K-step]: digits (K-step, valid tile).  Block row i = 4 q' + r' is the
// weight row of (element 4 g + q', position 4 t' + r').
struct ArOutFetch {
  const float* flat;
  ArNets N;
  int g, K, hin, cw, R0, R1;  // hin = the last hidden width, cw = the output layer's ArLayout::cw, R0 = KS, R1 = TV
  __device__ __forceinline__ void load(int ks, int tv, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int qn = i >> 2, e = 4 * g + qn, pos = 4 * ar_tile_of(tv, K) + (i & 3), c = pos >> 4, kk = pos & 15;
    const bool ok = e >= 1 && e < N.dim && kk < (c < 2 ? K : K - 1);
    const int ec = ok ? e : 1;
    const float* W = flat + N.rest(ec) + cw + (ok ? c * K + kk : 0) * hin;
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int k = ar_k_of(ks, q, e8), ku = k - qn * hin;
      const bool okk = ok && ku >= 0 && ku < hin;
      const float v = W[okk ? ku : 0];
      if (e8 < 4) va[e8 & 3] = okk ? v : 0.f;
      else vb[e8 & 3] = okk ? v : 0.f;
    }
  }
};
struct ArOutBias {  // tile t = valid tile tv; element 0: init_param
  const float* flat;
  ArNets N;
  int g, K, cb;  // cb = the output layer's ArLayout::cb
  __device__ __forceinline__ float operator()(int tv, int u) const {
    const int qn = u >> 2, e = 4 * g + qn, pos = 4 * ar_tile_of(tv, K) + (u & 3), c = pos >> 4, kk = pos & 15;
    const bool ok = e < N.dim && kk < (c < 2 ? K : K - 1);
    const int at = (e >= 1 ? N.rest(ok ? e : 1) + cb : 0) + c * K + kk;
    const float v = flat[ok ? at : 0];
    return ok ? v : 0.f;
  }
};

// The group's first layer: x[:, :4 g + 3] (what the widest net of the group reads) streamed K-step by K-step.
template <int NTL, typename Src>
__device__ __forceinline__ void ar_first_layer(const NsfArRtArgs& a, Src& src, int g, float wup, int lane, int q,
                                               const float* (&xrow)[NTL], rt::Hidden<4, NTL>& h) {
  using namespace rt;
  const ArLayout& L = a.L;
  const int n_cols = 4 * g + 3 < L.n.dim - 1 ? 4 * g + 3 : L.n.dim - 1;  // >= 1
  const bool VEC = a.vec != 0;                                      // (uniform; dim % 4 == 0 then)
  const int limit = VEC ? (n_cols + 3) & ~3 : n_cols;  // columns >= n_cols meet zero weights
  const int KS = steps32(n_cols), MT = tiles16(4 * L.hid[0]);
  const int KC = src.cb / MT;  // K-steps per chunk (>= 6)
  Acc<4, NTL> acc;
  acc.zero();
  float down[NTL];  // the rows' running scale (a power of two <= 1)
#pragma unroll
  for (int t = 0; t < NTL; ++t) down[t] = 1.f;
  ArFirstFetch fetch{a.flat, L.n, g, L.hid[0], MT, 0};
  const ArHiddenBias bias_fn{a.flat, L.n, g, L.hid[0], 0};
  Chunk c{nullptr, nullptr};
  int next_start = 0, chunk_start = 0;
  for (int ks = 0; ks < KS; ++ks) {
    if (ks == next_start) {  // (uniform) a new chunk of A blocks starts at this K-step
      const int kc = KS - ks < KC ? KS - ks : KC;
      fetch.ks0 = ks;
      c = src.template chunk<false>(kc * MT, fetch, ks + kc == KS ? MT : 0, bias_fn);
      chunk_start = ks;
      next_start = ks + kc;
    }
    f16x8 bh[NTL], bl[NTL];
    f32x4 xa[NTL], xb[NTL];
    float mx = 0.f;
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
      xa[t] = load4(xrow[t], 32 * ks + 4 * q, limit, VEC);
      xb[t] = load4(xrow[t], 32 * ks + 16 + 4 * q, limit, VEC);
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
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            acc.main[t][m] *= f;
            acc.corr[t][m] *= f;
          }
          down[t] = want;
        }
        float unused = 0.f;
        split_kstep(xa[t], xb[t], down[t], bh[t], bl[t], unused);
      }
    }
    mac_kstep<4, NTL>(c.A, (ks - chunk_start) * MT, MT, lane, bh, bl, acc.main, acc.corr);
  }
  float scale[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t) scale[t] = wup / down[t];
  finish_layer<4, NTL>(acc, c.bias, MT, q, scale, true, h);
}

// The hidden -> hidden layers 1 .. n_hidden - 1 of the group in registers (at most 2 K-steps x 4 tiles: one chunk each).
// hook(i, h): called with every finished hidden vector H_i, i = 2 .. n_hidden (the gradient kernel keeps them).
template <int NTL, typename Src, typename Hook = rt::NoLayerHook>
__device__ __forceinline__ void ar_hidden_layers(const NsfArRtArgs& a, Src& src, int g, float wup, int lane, int q,
                                                 rt::Hidden<4, NTL>& h, const Hook& hook = Hook()) {
  using namespace rt;
  const ArLayout& L = a.L;
  Acc<4, NTL> acc;
  for (int l = 1; l < L.n_hidden; ++l) {
    const int KS = steps32(16 * tiles16(4 * L.hid[l - 1])), MT = tiles16(4 * L.hid[l]);
    acc.zero();
    const Chunk c = src.template chunk<false>(KS * MT, ArHiddenFetch{a.flat, L.n, g, L.hid[l - 1], L.hid[l], L.cw[l], MT, 0}, MT,
                                              ArHiddenBias{a.flat, L.n, g, L.hid[l], L.cb[l]});
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      if (ks < KS) {
        f16x8 bh[NTL], bl[NTL];
        hidden_operand<4, NTL>(h, ks, bh, bl);
        mac_kstep<4, NTL>(c.A, ks * MT, MT, lane, bh, bl, acc.main, acc.corr);
      }
    float scale[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) scale[t] = wup * h.up[t];
    finish_layer<4, NTL>(acc, c.bias, MT, q, scale, true, h);
    hook(l + 1, h);
  }
}

// The shape envelope of both kernels and the layout of a shape's `flat` (false: outside)
inline bool ar_layout_plan(int dim, int K, int n_hidden, const int* hidden, ArLayout& L) {
  if (dim < 2 || dim > 32768 || K < 2 || K > 16 || n_hidden < 1 || n_hidden > kArMaxHidden || !hidden_ok(n_hidden, hidden))
    return false;
  for (int l = 0; l < n_hidden; ++l)
    if (hidden[l] < 4 || hidden[l] > 16) return false;  // four nets side by side: <= 64 units = 4 tiles
  if (mnf_nsf_ar_flat_floats(dim, K, n_hidden, hidden) >= (1ll << 31)) return false;
  L.n.dim = dim; L.K = K; L.n.P = 3 * K - 1; L.n.h0 = hidden[0]; L.n_hidden = n_hidden;
  for (int l = 0; l < kArMaxHidden; ++l) L.hid[l] = l < n_hidden ? hidden[l] : 0;
  int off = hidden[0];  // behind the e * h0 first-layer weights: the first layer's bias, then the other layers
  L.cw[0] = 0;
  L.cb[0] = 0;
  for (int l = 1; l <= n_hidden; ++l) {
    const int n_in = hidden[l - 1], n_out = l < n_hidden ? hidden[l] : L.n.P;
    L.cw[l] = off;
    off += n_in * n_out;
    L.cb[l] = off;
    off += n_out;
  }
  L.n.C = off;
  return true;
}

}  // namespace mnf
