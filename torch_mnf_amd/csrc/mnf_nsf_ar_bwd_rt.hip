// Gradients of NSF_AR.inverse (torch_mnf/flows/spline_flow.py:218-235 under loss.backward(): x -> z, the direction log_prob
// and training run through) on the f16 matrix pipe, for the shapes of mnf_nsf_ar_rt.hip and K from MNF_NSF_AR_BWD_KS:
//   z_i, ld_i = RQS_forward(x_i; net_{i-1}(x[:, :i])),  log_det = sum_i ld_i;  given grad_y, grad_ld, x and flat.
// Nothing is saved by the forward pass: like mnf_nsf_ar_bwd the kernel recomputes from x.
//
// A workgroup of nw waves owns a block of 16 nw rows, a wave one 16-row tile of it (lane (row j, q)).  The elements are
// walked in the forward kernel's GROUPS of four, 4 g .. 4 g + 3, lane q owning element 4 g + q, the four nets of a group as
// ONE block-diagonal net (mnf_nsf_ar_rt.h).  Per row block and group:
//   * the net forwards, every hidden vector kept (its sign bits; its values turned into the LDS exchange area);
//   * the output tiles give the lane's 3K-1 raw parameters, nsfgrad::rqs_grad<K, false> the direct term of grad_x[:, e] and the
//     parameter cotangents g_p, which go back into the tile layout (times the launch's cotangent scale): dW / db of the four
//     output layers through the exchange area (element 0: its bias only = init_param) and the chain start W_out^T g_p against
//     TURNED blocks;
//   * the hidden layers backwards and the first layer, diagonal blocks only: the turned blocks stage an off-diagonal weight as
//     exactly 0 (a select), and a weight-gradient product that lands on one is DROPPED (dw_phase_at: a negative offset), not
//     added as a computed 0;
//   * grad_x: lane (j, q') owns the columns 16 mi + 4 q' .. + 3 of its row, i.e. the group 4 mi + q' -- the group's own columns
//     are WRITTEN in its pass (direct term + what the later elements of the group send back), the columns of earlier groups
//     are read, added to and written back by the same lane (as nsf_bwd_rt parks cotangents in grad_x).
// Padding elements (e >= dim) and padding rows contribute nothing: their cotangents, hidden vectors and inputs enter the
// exchange area as selected zeros.  One staging exponent per launch (the largest finite weight); one cotangent scale per
// launch, a power of two from a sample of grad_y / grad_ld that every workgroup takes for itself (the rule of
// mnf_affine_half_grad_scale: at most 512 rows spread over the batch), so that a mean() loss over 10^6 rows stays in the
// split-f16 range of the weight-gradient products; the rows of the delta chain are scaled up as well as down on top of it
// (rt::split_rows_both), so that a row's grad_x does not depend on which batch it is in.  Loop order: row block outer, group inner -- a group's weights are staged again for every row block and
// its dW added once per row block.  The parameter sums are float atomics, each entry of a workgroup's from
// one lane in program order: with a slot per workgroup (mnf_nsf_ar_bwd_rt_det, mnf_rt_host.h launch_rt_bwd) they repeat bit
// for bit.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mnf_nsf_ar_rt.h"
#include "mnf_nsf_spline_grad.h"
#include "mnf_rt_bwd.h"

// the K values with an instantiation (each costs 10-20 KB of the library's size budget, tests/test_build_gate.py)
#ifndef MNF_NSF_AR_BWD_KS
#define MNF_NSF_AR_BWD_KS(X) X(5) X(8)
#endif

namespace mnf {

struct NsfArBwdRtArgs {
  NsfArRtArgs f;  // x, flat, rows, vec (of x), T, the streaming plan and the layout; y / log_det unused
  const float* grad_y;
  const float* grad_ld;
  float* grad_x;
  float* grad_flat;
  int gvec;                // grad_x's rows are 16-byte aligned
  int ht_tiles, ct_tiles;  // exchange tiles: the hidden vectors | a phase's cotangent / input tiles
  int64_t sample, stride;  // the cotangent scale's sample: rows 0, stride, 2 stride, ...
  int64_t slot_floats;     // 0; mnf_nsf_ar_bwd_rt_det: workgroup b adds into grad_flat + b * slot_floats (mnf_rt_host.h)
};

// first exchange tile of hidden vector H_i (i >= 1) of the side-by-side net
__host__ __device__ inline int ar_h_tile(const ArLayout& L, int i) {
  int t = 0;
  for (int k = 1; k < i; ++k) t += (4 * L.hid[k - 1] + 15) >> 4;
  return t;
}

// ---- turned blocks (the transposed layers of the delta chain); an entry off the diagonal blocks is staged as exactly 0
// Output layer: block row i = unit 16 mh + i of the last hidden vector, K index (K-step kp) = (valid tile 2 kp + (k >> 4),
// unit k & 15 = 4 q' + r'): digits (mh, kp).  A lane's eight K indices lie in ITS q' = q (ar_k_of).
struct ArOutTFetch {
  const float* flat;
  ArNets N;
  int g, K, hin, cw, R0, TV;  // R0 = hidden tiles
  static constexpr int R1 = 1 << 30;
  __device__ __forceinline__ void load(int mh, int kp, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int hu = 16 * mh + i, qn = ar_net_of(hu, hin), ku = hu - qn * hin, e = 4 * g + q;
    const bool ok = qn == q && e >= 1 && e < N.dim;
    const float* W = flat + N.rest(ok ? e : 1) + cw + (ok ? ku : 0);
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int tv = 2 * kp + (e8 >> 2), pos = 4 * ar_tile_of(tv < TV ? tv : 0, K) + (e8 & 3), c = pos >> 4, kk = pos & 15;
      const bool okk = ok && tv < TV && kk < (c < 2 ? K : K - 1);
      const float v = W[okk ? (c * K + kk) * hin : 0];
      if (e8 < 4) va[e8 & 3] = okk ? v : 0.f;
      else vb[e8 & 3] = okk ? v : 0.f;
    }
  }
};
// Layer l (1 .. n_hidden - 1: hin -> hout units per net): block row i = unit 16 mi + i of H_l, K index = unit of H_{l+1}: digits
// (mi, K-step)
struct ArHiddenTFetch {
  const float* flat;
  ArNets N;
  int g, hin, hout, cw, R0;  // R0 = tiles of H_l
  static constexpr int R1 = 1 << 30;
  __device__ __forceinline__ void load(int mi, int ks, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int hu = 16 * mi + i, qn = ar_net_of(hu, hin), ku = hu - qn * hin, e = 4 * g + qn;
    const bool ok = qn < 4 && e >= 1 && e < N.dim;
    const float* W = flat + N.rest(ok ? e : 1) + cw + (ok ? ku : 0);
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int ko = ar_k_of(ks, q, e8), uo = ko - qn * hout;
      const bool okk = ok && uo >= 0 && uo < hout;  // the K index is a unit of the same net
      const float v = W[okk ? uo * hin : 0];
      if (e8 < 4) va[e8 & 3] = okk ? v : 0.f;
      else vb[e8 & 3] = okk ? v : 0.f;
    }
  }
};
// First layer: block row i = input column 16 (m0 + ml) + i, K index = unit (net q', u) of H_1; net e reads the columns < e:
// digits (K-step, ml)
struct ArFirstTFetch {
  const float* flat;
  ArNets N;
  int g, hw, R0, m0;  // hw = hidden[0], R0 = KS over H_1
  static constexpr int R1 = 1 << 30;
  __device__ __forceinline__ void load(int ks, int ml, int, int i, int q, f32x4& va, f32x4& vb) const {
    const int col = 16 * (m0 + ml) + i;
#pragma unroll
    for (int e8 = 0; e8 < 8; ++e8) {
      const int ko = ar_k_of(ks, q, e8), qn = ar_net_of(ko, hw), e = 4 * g + qn;
      const bool ok = qn < 4 && e >= 1 && e < N.dim && col < e;
      const float v = flat[ok ? N.base(e) + (ko - qn * hw) * e + col : 0];
      if (e8 < 4) va[e8 & 3] = ok ? v : 0.f;
      else vb[e8 & 3] = ok ? v : 0.f;
    }
  }
};

// ---- where a weight-gradient product goes (rt::dw_phase_at): the float offset in `flat`, or -1: no add
struct ArOutAt {  // delta tile m = valid tile, unit u = 4 q' + r'; k = unit of the last hidden vector
  ArNets N;
  int g, K, hin, cw, cb;
  __device__ __forceinline__ int param(int m, int u) const {  // c K + kk of the element's 3K-1, or -1
    const int pos = 4 * ar_tile_of(m, K) + (u & 3), c = pos >> 4, kk = pos & 15;
    return kk < (c < 2 ? K : K - 1) ? c * K + kk : -1;
  }
  __device__ __forceinline__ int w(int m, int u, int k) const {
    const int qn = u >> 2, e = 4 * g + qn, pr = param(m, u), ku = k - qn * hin;
    return pr >= 0 && e >= 1 && e < N.dim && ku >= 0 && ku < hin ? N.rest(e) + cw + pr * hin + ku : -1;
  }
  __device__ __forceinline__ int b(int m, int u) const {  // element 0: init_param
    const int e = 4 * g + (u >> 2), pr = param(m, u);
    return pr >= 0 && e < N.dim ? (e >= 1 ? N.rest(e) + cb : 0) + pr : -1;
  }
};
struct ArHiddenAt {  // layer l: delta unit o = 16 m + u of H_{l+1}, k = unit of H_l
  ArNets N;
  int g, hin, hout, cw, cb;
  __device__ __forceinline__ int w(int m, int u, int k) const {
    const int o = 16 * m + u, qn = ar_net_of(o, hout), e = 4 * g + qn, ku = k - qn * hin;
    return qn < 4 && e >= 1 && e < N.dim && ku >= 0 && ku < hin ? N.rest(e) + cw + (o - qn * hout) * hin + ku : -1;
  }
  __device__ __forceinline__ int b(int m, int u) const {
    const int o = 16 * m + u, qn = ar_net_of(o, hout), e = 4 * g + qn;
    return qn < 4 && e >= 1 && e < N.dim ? N.rest(e) + cb + (o - qn * hout) : -1;
  }
};
struct ArFirstAt {  // delta unit o = 16 m + u of H_1, k = input column (< e)
  ArNets N;
  int g, hw;
  __device__ __forceinline__ int w(int m, int u, int k) const {
    const int o = 16 * m + u, qn = ar_net_of(o, hw), e = 4 * g + qn;
    return qn < 4 && e >= 1 && e < N.dim && k < e ? N.base(e) + (o - qn * hw) * e + k : -1;
  }
  __device__ __forceinline__ int b(int m, int u) const {
    const int o = 16 * m + u, qn = ar_net_of(o, hw), e = 4 * g + qn;
    return qn < 4 && e >= 1 && e < N.dim ? N.rest(e) + (o - qn * hw) : -1;
  }
};

template <int MT>
__device__ __forceinline__ void ar_zero_unless(bool keep, f32x4 (&v)[MT]) {  // (a select: padding rows hold a copy of the last row)
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[m][r] = keep ? v[m][r] : 0.f;
}

// The group's output layer for a compile-time K: parameters, spline derivative, dW_out / db_out, chain start.  dv: the
// cotangent of H_n's pre-activation (in units of the cotangent scale), g_v: the direct term of grad_x[:, 4 g + q].
template <int K, typename Src>
__device__ __forceinline__ void ar_bwd_out(const NsfArBwdRtArgs& a, Src& src, const rt::BwdLds& lds, int g, float wup, float gs,
                                           float inv_gs, const rt::Hidden<4, 1>& h, float v, float g_out, float gl, bool on,
                                           bool live, float* gflat, f32x4 (&dv)[4], float& g_v) {
  using namespace rt;
  constexpr int NW_ = (K + 3) / 4, ND_ = (K - 1 + 3) / 4, TV = 2 * NW_ + ND_, KSO = (TV + 1) / 2;
  const ArLayout& L = a.f.L;
  const int lane = lds.lane, q = lds.q, nh = L.n_hidden, hin = L.hid[nh - 1];
  const int MTh = tiles16(4 * hin), KS = steps32(16 * MTh);
  float p[3 * K - 1], g_p[3 * K - 1];
  {
    const Chunk c = src.template chunk<false>(TV * KS, ArOutFetch{a.f.flat, L.n, g, K, hin, L.cw[nh], KS, TV}, TV,
                                              ArOutBias{a.f.flat, L.n, g, K, L.cb[nh]});
#pragma unroll
    for (int tv = 0; tv < TV; ++tv) {
      f32x4 o[1];
      out_tile<4, 1>(c.A, tv * KS, KS, c.bias + tv * 16, lane, q, h, wup, o);
      const int cgrp = tv < NW_ ? 0 : tv < 2 * NW_ ? 1 : 2, k0 = 4 * (tv - cgrp * NW_);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k0 + i < (cgrp < 2 ? K : K - 1)) p[cgrp * K + k0 + i] = o[0][i];
    }
  }
  nsfgrad::rqs_grad<K, false>(v, a.f.T, p, g_out, gl, g_v, g_p);
  // the parameter cotangents back in the tile layout, times the cotangent scale; padding elements and rows: selected zeros
  f32x4 gt[TV];
  float fm = 0.f;
#pragma unroll
  for (int tv = 0; tv < TV; ++tv) {
    const int cgrp = tv < NW_ ? 0 : tv < 2 * NW_ ? 1 : 2, k0 = 4 * (tv - cgrp * NW_);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool valid = k0 + i < (cgrp < 2 ? K : K - 1);
      gt[tv][i] = valid && on ? g_p[valid ? cgrp * K + k0 + i : 0] * gs : 0.f;
      fm = __builtin_fmaxf(fm, finite_abs(gt[tv][i]));
    }
  }
  // chain start: (turned blocks of the group's output layers) x [tile 2 kp | tile 2 kp + 1], the row at one power-of-two scale
  {
    const Chunk ct = src.template chunk<false>(KSO * MTh, ArOutTFetch{a.f.flat, L.n, g, K, hin, L.cw[nh], MTh, TV}, 0, NoBias{});
    const int ed = both_exponent(max_over_q(fm));  // (up as well as down: grad_x does not depend on the launch's cotangent scale)
    const float down = pow2f(-ed);
    Acc<4, 1> accd;
    accd.zero();
#pragma unroll
    for (int kp = 0; kp < KSO; ++kp) {
      const f32x4 g0 = gt[2 * kp], g1 = 2 * kp + 1 < TV ? gt[2 * kp + 1 < TV ? 2 * kp + 1 : 0] : f32x4{0.f, 0.f, 0.f, 0.f};
      f16x8 bh[1], bl[1];
      float unused = 0.f;
      split_kstep(g0, g1, down, bh[0], bl[0], unused);
      mac_kstep<4, 1>(ct.A, kp * MTh, MTh, lane, bh, bl, accd.main, accd.corr);
    }
    chain_result<4>(accd, wup * pow2f(ed), lds.meta_bits[nh * 64 + lane], dv);
    ar_zero_unless<4>(live, dv);
  }
  if (gflat) {  // dW_out, db_out of the four elements
    const float sc = exchange_store<TV>(gt, TV, lds.exC, 0, 16 * lds.wave, lane, lds.ident);
    if (lane == 0) lds.sC[lds.wave] = sc;
    lds_barrier();
    dw_phase_at(lds.exC, 0, TV, lds.exH, ar_h_tile(L, nh), MTh, lds.sC, lds.sH + nh * 8, lds.nw, inv_gs, gflat,
                ArOutAt{L.n, g, K, hin, L.cw[nh], L.cb[nh]}, true, 0);
  }
}

// One group of one row block.
template <typename Src>
__device__ __forceinline__ void nsf_ar_bwd_group(const NsfArBwdRtArgs& a, Src& src, const rt::BwdLds& lds, int g, float wup,
                                                 float gs, float inv_gs, const float* xrow, const float* gyrow, float* gxrow,
                                                 float gl, bool live, float* gflat) {
  using namespace rt;
  const ArLayout& L = a.f.L;
  const int lane = lds.lane, wave = lds.wave, q = lds.q, nw = lds.nw, j = lane & 15;
  const int dim = L.n.dim, nh = L.n_hidden;
  const bool VEC = a.f.vec != 0, GVEC = a.gvec != 0;  // (uniform)
  // ---- forward, keeping every hidden vector: sign bits; true values (padding rows: zeros) in the exchange area
  Hidden<4, 1> h;
  auto hook = [&](int i, const Hidden<4, 1>& hh) {
    lds.meta_bits[i * 64 + lane] = pack_signs<4>(hh);
    if (gflat) {  // (uniform)
      f32x4 hv[4];
      unsplit<4>(hh, hv);
      ar_zero_unless<4>(live, hv);
      const float sc = exchange_store<4>(hv, tiles16(4 * L.hid[i - 1]), lds.exH, ar_h_tile(L, i), 16 * wave, lane, lds.ident);
      if (lane == 0) lds.sH[i * 8 + wave] = sc;
    }
  };
  {
    const float* xr[1] = {xrow};
    ar_first_layer<1>(a.f, src, g, wup, lane, q, xr, h);
    hook(1, h);
    ar_hidden_layers<1>(a.f, src, g, wup, lane, q, h, hook);
  }
  // ---- the lane's element, its spline derivative, the output layers' gradients and the chain start
  const int e = 4 * g + q;
  const bool real = e < dim;
  const float v = xrow[real ? e : 0], gyv = gyrow ? gyrow[real ? e : 0] : 0.f;
  f32x4 dv[4] = {};
  float g_v = 0.f;
  switch (L.K) {  // (uniform)
#define MNF_NSF_AR_BWD_CASE(KK) \
  case KK: ar_bwd_out<KK>(a, src, lds, g, wup, gs, inv_gs, h, v, gyv, gl, real && live, live, gflat, dv, g_v); break;
    MNF_NSF_AR_BWD_KS(MNF_NSF_AR_BWD_CASE)
#undef MNF_NSF_AR_BWD_CASE
    default: break;
  }
  // ---- the hidden layers backwards: delta_{i-1} = (W_{i-1}^T delta_i) * act'(H_{i-1}), diagonal blocks only
#pragma unroll 1
  for (int i = nh; i >= 2; --i) {
    const int hout = L.hid[i - 1], hin = L.hid[i - 2], MTi = tiles16(4 * hout), MTp = tiles16(4 * hin);
    if (gflat) {
      // delta_i goes into the exchange tiles of H_i, whose last reader (the phase before) every wave has left behind this barrier
      lds_barrier();
      const Exchange exD{lds.exH.tile(ar_h_tile(L, i)), lds.exH.R};
      const float sc = exchange_store<4>(dv, MTi, exD, 0, 16 * wave, lane, lds.ident);
      if (lane == 0) lds.sA[wave] = sc;
      lds_barrier();
      dw_phase_at(exD, 0, MTi, lds.exH, ar_h_tile(L, i - 1), MTp, lds.sA, lds.sH + (i - 1) * 8, nw, inv_gs, gflat,
                  ArHiddenAt{L.n, g, hin, hout, L.cw[i - 1], L.cb[i - 1]}, true, 0);
    }
    Hidden<4, 1> hd;
    split_rows_both<4>(dv, hd);
    const int KSi = steps32(16 * MTi);
    const Chunk c = src.template chunk<false>(KSi * MTp, ArHiddenTFetch{a.f.flat, L.n, g, hin, hout, L.cw[i - 1], MTp}, 0, NoBias{});
    Acc<4, 1> acc;
    acc.zero();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      if (ks < KSi) {
        f16x8 bh[1], bl[1];
        hidden_operand<4, 1>(hd, ks, bh, bl);
        mac_kstep<4, 1>(c.A, ks * MTp, MTp, lane, bh, bl, acc.main, acc.corr);
      }
    chain_result<4>(acc, wup * hd.up[0], lds.meta_bits[(i - 1) * 64 + lane], dv);
    ar_zero_unless<4>(live, dv);
  }
  // ---- the first layer: grad_x of the columns < 4 g + 4 and dW_0 / db_0, input tile by input tile
  const int h0 = L.hid[0], MT1 = tiles16(4 * h0), KS1 = steps32(16 * MT1);
  const int n_cols = 4 * g + 4 < dim ? 4 * g + 4 : dim, MI = tiles16(n_cols);  // (the tile of the group's own columns included)
  const Exchange exD1{lds.exH.tile(0), lds.exH.R};  // (delta_1 in H_1's tiles, as above)
  if (gflat) {
    lds_barrier();
    const float sc = exchange_store<4>(dv, MT1, exD1, 0, 16 * wave, lane, lds.ident);
    if (lane == 0) lds.sA[wave] = sc;
  }
  Hidden<4, 1> hd;
  split_rows_both<4>(dv, hd);
  // the direct terms of the group's four columns, on every lane of the row (element 4 g + r from lane (j, r))
  f32x4 direct;
#pragma unroll
  for (int r = 0; r < 4; ++r) direct[r] = __shfl(g_v, j + 16 * r, 64);
  int CI = src.cb / KS1;
  if (CI > lds.ct_tiles) CI = lds.ct_tiles;
  if (CI > 4) CI = 4;
#pragma unroll 1
  for (int mi0 = 0; mi0 < MI; mi0 += CI) {
    const int ci = MI - mi0 < CI ? MI - mi0 : CI;
    uint32_t* buf = src.cur_blocks();
    float* bbuf = src.cur_bias();
    stage_blocks(buf, ci * KS1, ArFirstTFetch{a.f.flat, L.n, g, h0, KS1, mi0}, src.wdown);
    stage_bias(bbuf, 1, NoBias{});
    src.commit();
    f32x4 xv[4];
#pragma unroll
    for (int ml = 0; ml < 4; ++ml) {
      xv[ml] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ml < ci) {
        f32x4 gx[1];
        out_tile<4, 1>(buf, ml * KS1, KS1, bbuf, lane, q, hd, wup, gx);
        const int col = 16 * (mi0 + ml) + 4 * q, gp = 4 * (mi0 + ml) + q;  // the lane's group of four columns
        const f32x4 before = load4(gxrow, col, dim, GVEC);  // (of a later group: not written yet, and not used)
        const f32x4 sent = gx[0] * inv_gs;
        f32x4 now;
#pragma unroll
        for (int r = 0; r < 4; ++r) now[r] = gp < g ? before[r] + sent[r] : direct[r] + sent[r];
        store4(gxrow, col, dim, GVEC, live && gp <= g, now);
        xv[ml] = load4(xrow, col, dim, VEC);
      }
    }
    if (gflat) {
      ar_zero_unless<4>(live, xv);
      const float sc = exchange_store<4>(xv, ci, lds.exC, 0, 16 * wave, lane, lds.ident);
      if (lane == 0) lds.sC[wave] = sc;
      lds_barrier();
      dw_phase_at(exD1, 0, MT1, lds.exC, 0, ci, lds.sA, lds.sC, nw, inv_gs, gflat, ArFirstAt{L.n, g, h0}, mi0 == 0, mi0);
    }
  }
}

__global__ void __launch_bounds__(512) nsf_ar_bwd_rt_kernel(NsfArBwdRtArgs a) {
  using namespace rt;
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, nw = blockDim.x >> 6;
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + kBwdHeadWords;
  float* bias = reinterpret_cast<float*>(blocks + a.f.block_words);
  const BwdLds lds = bwd_lds(rt_lds, bias + a.f.bias_words, a.ht_tiles, 0, a.ct_tiles);
  const ArLayout& L = a.f.L;
  const int dim = L.n.dim;
  // one staging exponent per launch: the largest finite WEIGHT of all nets (biases and init_param are not looked at)
  float mx = 0.f;
  for (int e = 1; e < dim; ++e)
    for (int l = 0; l <= L.n_hidden; ++l) mx = range_abs_max(a.f.flat + L.w(e, l), L.n_in(e, l) * L.n_out(l), mx);
  const int ex = weight_exponent(block_weight_max(mx, scratch));
  const float wup = pow2f(ex);
  Source<false> src{blocks, bias, a.f.cb, a.f.bt, 0, 0, 0, pow2f(-ex), 0};
  // one cotangent scale per launch: the power of two that brings the sample's largest finite |cotangent| into [1, 2)
  float gm = 0.f;
  if (a.grad_y)
    for (int64_t i = threadIdx.x; i < a.sample * dim; i += blockDim.x) {
      const int64_t r = i / dim, c = i - r * dim;
      gm = __builtin_fmaxf(gm, finite_abs(a.grad_y[r * a.stride * dim + c]));
    }
  if (a.grad_ld)
    for (int64_t i = threadIdx.x; i < a.sample; i += blockDim.x) gm = __builtin_fmaxf(gm, finite_abs(a.grad_ld[i * a.stride]));
  gm = block_weight_max(gm, scratch);
  int ge = 127 - (int)((__builtin_bit_cast(uint32_t, gm) >> 23) & 0xffu);
  ge = gm > 0.f ? (ge > 120 ? 120 : ge < -120 ? -120 : ge) : 0;
  const float gs = pow2f(ge), inv_gs = pow2f(-ge);
  const int G = (dim + 3) >> 2;
  const int64_t n_blocks = (a.f.rows + 16 * nw - 1) / (16 * nw);
  float* const gflat = a.grad_flat + blockIdx.x * a.slot_floats;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t r = blk * (16 * nw) + 16 * wave + j;
    const bool live = r < a.f.rows;
    const int64_t rc = live ? r : a.f.rows - 1;
    const float* xrow = a.f.x + rc * dim;
    const float* gyrow = a.grad_y ? a.grad_y + rc * dim : nullptr;
    float* gxrow = a.grad_x + rc * dim;
    const float glv = a.grad_ld ? a.grad_ld[rc] : 0.f;
    const float gl = live ? glv : 0.f;
#pragma unroll 1
    for (int g = 0; g < G; ++g) nsf_ar_bwd_group(a, src, lds, g, wup, gs, inv_gs, xrow, gyrow, gxrow, gl, live, gflat);
  }
}

// The launch of a shape, or false: mnf_nsf_ar_bwd takes it.  Fills the kernel arguments' shape part.
static bool nsf_ar_bwd_rt_plan(int dim, int K, int n_hidden, const int* hidden, NsfArBwdRtArgs& a, RtPlan& p) {
  bool shipped = false;
#define MNF_NSF_AR_BWD_HAS(KK) shipped = shipped || K == KK;
  MNF_NSF_AR_BWD_KS(MNF_NSF_AR_BWD_HAS)
#undef MNF_NSF_AR_BWD_HAS
  if (!shipped || !ar_layout_plan(dim, K, n_hidden, hidden, a.f.L)) return false;
  auto t16 = [](int n) { return (n + 15) / 16; };
  const int TV = 2 * ((K + 3) / 4) + (K + 2) / 4, MTh = t16(4 * hidden[n_hidden - 1]), KS = (16 * MTh + 31) / 32;
  const int KSO = (TV + 1) / 2;
  // a streaming buffer: the group's output blocks, their turned counterparts, a hidden layer, a chunk of the first layer
  a.f.cb = TV * KS > KSO * MTh ? TV * KS : KSO * MTh;
  if (a.f.cb < 12) a.f.cb = 12;
  if (a.f.cb > kArStream) return false;
  a.f.bt = TV > 8 ? TV : 8;
  a.ht_tiles = 0;
  for (int l = 0; l < n_hidden; ++l) a.ht_tiles += t16(4 * hidden[l]);
  p.mt_max = 4;
  p.resident = false;
  // (one chunk size; any wave count: fewer rows per block where the exchange area of 8 waves does not fit)
  const int ct = TV > 4 ? TV : 4;
  return rt::fit_bwd_lds(a.f, a, p, {/*nw_max=*/8, a.f.cb, a.f.cb, 1, /*ks1=*/1, /*ct_min=*/ct, /*ct_max=*/ct});
}

// the plan's kernel, its dynamic-LDS attribute set
static void (*nsf_ar_bwd_rt_kernel_of(const RtPlan&))(NsfArBwdRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, nsf_ar_bwd_rt_kernel);
  return nsf_ar_bwd_rt_kernel;
}

// the plan with the shape bound; a slot holds all of `flat`
struct nsf_ar_bwd_rt_slots {
  int dim, K, n_hidden;
  const int* hidden;
  int64_t operator()(NsfArBwdRtArgs& a, RtPlan& p) const {
    return nsf_ar_bwd_rt_plan(dim, K, n_hidden, hidden, a, p) ? mnf_nsf_ar_flat_floats(dim, K, n_hidden, hidden) : 0;
  }
};

// det: fixed-order parameter sums through `workspace` (mnf_rt_host.h run_rt_bwd)
static int nsf_ar_bwd_rt_run(const float* x, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                             const float* flat, int64_t rows, int dim, int K, float tail_bound, int n_hidden, const int* hidden,
                             bool det, float* workspace, int64_t workspace_floats, void* stream) {
  if (!x || !grad_x || x == grad_x || !flat || rows < 0 || dim < 1 || K < 1 || !(tail_bound > 0.f) || !hidden_ok(n_hidden, hidden) ||
      (grad_y && grad_y == grad_x) || (grad_flat && grad_flat == flat))
    return MNF_ERR_INVALID_ARG;
  auto fill = [&](NsfArBwdRtArgs& a) {
    a.f.x = x; a.f.flat = flat; a.f.rows = rows; a.f.T = tail_bound;
    a.grad_y = grad_y; a.grad_ld = grad_ld; a.grad_x = grad_x; a.grad_flat = grad_flat;
    a.f.vec = dim % 4 == 0 && aligned16(x);
    a.gvec = dim % 4 == 0 && aligned16(grad_x);
    a.sample = rows < 512 ? rows : 512;  // (mnf_affine_half_grad_scale's sample, at most 65,536 values)
    if (a.sample * dim > 65536) a.sample = 65536 / dim;
    a.stride = rows / a.sample;
  };
  return run_rt_bwd<NsfArBwdRtArgs>(
      {rows, dim, grad_flat, det, workspace, workspace_floats, "nsf_ar_bwd_rt", stream},
      /*in_domain=*/1e-3 * K <= 1.0 /* spline_flow.py:90-93 */, /*unsupported=*/false, nsf_ar_bwd_rt_slots{dim, K, n_hidden, hidden},
      fill, nsf_ar_bwd_rt_kernel_of);
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_nsf_ar_bwd_rt_supported(int dim, int K, int n_hidden, const int* hidden) {
  return rt_has_plan<NsfArBwdRtArgs>(nsf_ar_bwd_rt_slots{dim, K, n_hidden, hidden});
}

extern "C" int64_t mnf_nsf_ar_bwd_rt_det_workspace(int64_t rows, int dim, int K, int n_hidden, const int* hidden) {
  return rt_det_workspace<NsfArBwdRtArgs>(rows, dim, nsf_ar_bwd_rt_slots{dim, K, n_hidden, hidden}, nsf_ar_bwd_rt_kernel_of);
}

extern "C" int mnf_nsf_ar_bwd_rt(const float* x, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                                 const float* flat, int64_t rows, int dim, int K, float tail_bound, int n_hidden,
                                 const int* hidden, void* stream) {
  return nsf_ar_bwd_rt_run(x, grad_y, grad_ld, grad_x, grad_flat, flat, rows, dim, K, tail_bound, n_hidden, hidden, false, nullptr,
                           0, stream);
}

extern "C" int mnf_nsf_ar_bwd_rt_det(const float* x, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                                     const float* flat, int64_t rows, int dim, int K, float tail_bound, int n_hidden,
                                     const int* hidden, float* workspace, int64_t workspace_floats, void* stream) {
  return nsf_ar_bwd_rt_run(x, grad_y, grad_ld, grad_x, grad_flat, flat, rows, dim, K, tail_bound, n_hidden, hidden, true, workspace,
                           workspace_floats, stream);
}
