// AffineHalfFlow.forward / .inverse (torch_mnf/flows/affine_half_flow.py:44-66) for ANY conditioner shape on the f16
// matrix pipe: run-time layer count and widths (mnf_rt.h), weights read from the plain `flat` parameter vector.  Takes
// every call the per-shape kernels (mnf_ahf_split.hip, mnf_ahf_mfma.hip) have no instantiation for -- h_sizes of any
// length >= 1, hidden widths 4 .. 256, any even dim -- and the VALU kernel of mnf_generic.hip keeps the rest (few rows,
// hidden layers narrower than 4 units, no hidden layer at all).
//
// A wave owns NTL 16-row tiles: the s-net and the t-net run one after the other up to their last hidden vectors (the
// conditioning half streamed from memory K-step by K-step, copied to y on the way), then the output layer is walked
// tile by tile: s and t of 16 columns, the affine transform of those columns, the row's log|det J| in registers.
//
// A RUN of n_layers layers of one shape (mnf_affine_half_rt_stack) is the same kernel with a layer loop: one layer's
// weights are resident (or streamed) at a time, and the workgroup sweeps ITS OWN row blocks once per layer.  Lane (j, q)
// of a wave stores exactly the elements of row j that it loads -- conditioning half columns 32 ks + 4 q + r and
// 32 ks + 16 + 4 q + r, transformed half columns 16 m + 4 q + r: in both the lane is (col mod 16) / 4 -- and the row block
// -> wave -> tile mapping is the same in every layer, so everything layer l + 1 loads was stored by the same lane in
// layer l: the hand-over through memory needs no barrier, no fence and no grid-wide synchronisation (lanes of rows past
// the end and out-of-range column pieces read clamped addresses that other lanes write; selects drop those values).
// Without an intermediates buffer the layers after the first run in place in y by the same ownership.
//
// SAMPLE (ahf_rt_sample_kernel: mnf_affine_half_rt_stack_sample / _logq, forward, no intermediates): a compile-time noise
// source.  The first applied layer is the only one that reads a.x, so there every row piece -- the conditioning half's
// K-steps and the transformed half's ring -- is not loaded but generated: element k of the piece at column c of the half
// at offset `off` is z0_normal(seed, row0 + r, off + c + k) for c + k < H, else 0 (mnf_device.h; mnf_normal_rows writes the
// same numbers), r the lane's clamped row; no x pointer is dereferenced.  Box-Muller pairs are (2 p, 2 p + 1) in the row's
// GLOBAL column: an even piece start takes two pairs, an odd one (odd half, the half at offset H: dim = 6, 10, ...)
// three, of which it keeps the inner four numbers.  Where the conditioning half is walked once per net (the one-net-at-
// a-time branch) its noise is simply generated once per net: nothing is cached.  The layers after the first are the
// ordinary in-place layers.  y is the only row tensor written: no log_det, no ysq.
// With a log_q pointer (a run-time pointer of the same instantiations: NULL = the x-only form, whose y is the same bits)
// the lane that owns a row (q == 0) also keeps the sample's own log-density, in this fp32 order: each lane sums the
// squares of its noise pieces -- the conditioning half's in K-step order (columns 32 ks + 4 q .., then 32 ks + 16 + 4 q ..),
// then the transformed half's x1 pieces (not y1) in tile order -- and its s values in tile order; both sums go over the
// four lanes of the row by sum_over_q (xor 16, then xor 32); layer 0 stores
//   log_q[r] = (-0.5 |z_r|^2 - dim * kHalfLog2Pi) - ld_0,
// and every later layer l does log_q[r] -= ld_l, read and written by the same lane in layer order (log_det's
// `accumulate` pattern with the sign turned).  Nothing in it depends on the batch: a pure function of (seed, absolute
// row, parameters).
#include <hip/hip_runtime.h>

#include <cstring>

#include "mnf_rt_host.h"

namespace mnf {

struct AhfRtArgs {
  const float* x;
  float* y;
  float* mid;                // (n_layers - 1, rows, dim): every layer's output but the last, or NULL (in place in y)
  float* log_det;
  float* ysq;
  float* log_prob;           // the standard-normal epilogue on the last applied layer: log_prob[r] and / or ...
  double* lp_sum;            // ... its sum over rows, ADDED (one atomic per wave)
  const float* flat;         // n_layers parameter vectors of n_params floats back to back, model order
  int64_t rows;
  uint32_t parity;           // bit l: layer l's parity
  int n_layers;
  int dim, inverse, accumulate, has_scale, has_shift;
  int n_params;
  int vec;                   // rows and halves are 16-byte aligned: dwordx4 row accesses
  int cb, bt;                // LDS plan (mnf_rt.h Source)
  int block_words, bias_words;
  NetDesc s_net, t_net;
};

// what changes from layer to layer of a run (the by-value AhfRtArgs stays constant: it lives in scalar registers)
struct AhfRtLayer {
  const float* x;
  float* y;
  const float* flat;
  float* ysq;
  float* log_prob;
  int parity, accumulate, lp;  // lp: this layer ends with the log-prob epilogue (log_prob and / or the sum)
};

// the noise source of the sampling instantiations (NOISE = 1), by value next to AhfRtArgs
struct AhfRtNoise {
  uint64_t seed;
  int64_t row0;   // the stream's row of y's row 0
  float* log_q;   // (rows,) or NULL
};

constexpr float kLog2e = 1.4426950408889634f;

// A wave's running fp64 log-prob sum: the 16 floats in front of the blocks, which block_weight_max is done with once it
// has returned (8 waves x 8 bytes)
extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
__device__ __forceinline__ double* lp_slot(int wave) { return reinterpret_cast<double*>(rt_lds) + wave; }

// load4's piece of the noise row with hash `rh`: columns off + c .. off + c + 3 of the row, zeros from column `limit` of the
// half on (a piece wholly past the end generates nothing)
__device__ __forceinline__ f32x4 noise4(uint32_t rh, uint32_t seed_lo, int off, int c, int limit) {
  f32x4 v{0.f, 0.f, 0.f, 0.f};
  if (c >= limit) return v;
  const int g = off + c, p = g >> 1;
  float n[6];
  if (g & 1) {  // (uniform: odd half, the half at offset H) three pairs, the inner four numbers
    z0_normal_pair(rh, seed_lo, p, n[4], n[0]);
    z0_normal_pair(rh, seed_lo, p + 1, n[1], n[2]);
    z0_normal_pair(rh, seed_lo, p + 2, n[3], n[5]);
  } else {
    z0_normal_pair(rh, seed_lo, p, n[0], n[1]);
    z0_normal_pair(rh, seed_lo, p + 1, n[2], n[3]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = c + r < limit ? n[r] : 0.f;
  return v;
}

// NOISE (0 / 1): the sampling form -- `first` (the first applied layer) generates its rows from nz, every layer keeps nz.log_q
template <int MT_MAX, int NTL, int VEC, bool PREFILL, int NOISE = 0, typename Src>  // VEC: 0 / 1, or 2 = a.vec
__device__ __forceinline__ void ahf_rt_block(const AhfRtArgs& a, const AhfRtLayer& ly, Src& src, float wup, int64_t row0,
                                             const AhfRtNoise& nz = AhfRtNoise{}, bool first = false) {
  using namespace rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int H = a.dim / 2;
  const int cond_off = ly.parity ? H : 0, act_off = ly.parity ? 0 : H;
  const bool vec = VEC == 2 ? a.vec != 0 : VEC == 1;
  const float* xrow[NTL];
  float* yrow[NTL];
  bool live[NTL];
  uint32_t rh[NOISE ? NTL : 1];  // NOISE: the rows' hashes
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
    const int64_t r = row0 + (int64_t)(wave * NTL + t) * 16 + j;
    live[t] = !PREFILL && r < a.rows;
    const int64_t rc = r < a.rows ? r : a.rows - 1;
    xrow[t] = ly.x + rc * a.dim;
    yrow[t] = ly.y + rc * a.dim;
    if constexpr (NOISE != 0) rh[t] = z0_row_hash(nz.seed, nz.row0 + rc);
  }
  // NOISE: a piece of row tile t's input, columns c .. c + 3 of the half at offset `off` (`first`: uniform)
  [[maybe_unused]] auto in4 = [&](int t, int off, int c) {
    return first ? noise4(rh[t], (uint32_t)nz.seed, off, c, H) : load4(xrow[t] + off, c, H, vec);
  };
  float sq[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t) sq[t] = 0.f;

  const NetDesc& any_net = a.has_scale ? a.s_net : a.t_net;
  const int n_hid = any_net.n_lin - 1;  // hidden vectors per net
  Hidden<MT_MAX, NTL> hs, ht;
  // the conditioning half: B operands of the first layer; the first net's pass also copies it to y (:50, :60-61)
  const int n_nets = (a.has_scale ? 1 : 0) + (a.has_shift ? 1 : 0);
  auto load_x = [&](int t, int ks, f32x4& xa, f32x4& xb) {
    const int c0 = 32 * ks + 4 * q;
    if constexpr (NOISE != 0) {
      xa = in4(t, cond_off, c0);
      xb = in4(t, cond_off, c0 + 16);
    } else {
      xa = load4(xrow[t] + cond_off, c0, H, vec);
      xb = load4(xrow[t] + cond_off, c0 + 16, H, vec);
    }
  };
  if (MT_MAX == 4 && n_nets == 2) {
    // both nets' first layers in ONE pass over the conditioning half (it is loaded, copied to y and split once; at wide
    // dims the input side is most of the layer), then each net's hidden layers
    auto use_x = [&](int t, int ks, const f32x4& xa, const f32x4& xb) {
      const int c0 = 32 * ks + 4 * q;
      store4(yrow[t] + cond_off, c0, H, vec, live[t], xa);
      store4(yrow[t] + cond_off, c0 + 16, H, vec, live[t], xb);
      sq[t] += xa[0] * xa[0] + xa[1] * xa[1] + xa[2] * xa[2] + xa[3] * xa[3] + xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2] +
               xb[3] * xb[3];
    };
    const NetDesc* const nds[2] = {&a.s_net, &a.t_net};
    Hidden<MT_MAX, NTL> h2[2];
    first_layer<MT_MAX, NTL, PREFILL, 2>(src, ly.flat, nds, n_hid != 0, wup, lane, q, load_x, use_x, h2);
    hs = h2[0];
    ht = h2[1];
    hidden_layers<MT_MAX, NTL, PREFILL>(src, ly.flat, a.s_net, n_hid, -1, wup, lane, q, hs);
    hidden_layers<MT_MAX, NTL, PREFILL>(src, ly.flat, a.t_net, n_hid, -1, wup, lane, q, ht);
  } else {
#pragma unroll 1
    for (int net = 0; net < n_nets; ++net) {
      const bool copy = net == 0;
      auto use_x = [&](int t, int ks, const f32x4& xa, const f32x4& xb) {
        const int c0 = 32 * ks + 4 * q;
        store4(yrow[t] + cond_off, c0, H, vec, live[t] && copy, xa);
        store4(yrow[t] + cond_off, c0 + 16, H, vec, live[t] && copy, xb);
        const float ss = xa[0] * xa[0] + xa[1] * xa[1] + xa[2] * xa[2] + xa[3] * xa[3] + xb[0] * xb[0] + xb[1] * xb[1] +
                         xb[2] * xb[2] + xb[3] * xb[3];
        sq[t] += copy ? ss : 0.f;
      };
      // (s_net, t_net are both filled: an absent net is a copy of the other one; net 0 = the first PRESENT net)
      if (net == 1) hs = ht;  // (both nets present: the s-net's vector moves over, the t-net's takes its place)
      net_to_hidden<MT_MAX, NTL, PREFILL>(src, ly.flat, net == 0 && a.has_scale ? a.s_net : a.t_net, n_hid, -1, wup, lane, q,
                                          load_x, use_x, ht);
    }
  }
  const bool both = n_nets == 2;  // else the one present net's vector is in ht

  // ---- output layer, tile by tile: blocks [tile][head][K-step]
  const int L = any_net.n_lin - 1;
  const int KS = steps32(16 * tiles16(any_net.sizes[L])), M = tiles16(H);
  const int heads = (a.has_scale ? 1 : 0) + (a.has_shift ? 1 : 0);
  int MO = Src::resident ? M : src.cb / (heads * KS);
  if (MO > src.bt / heads && !Src::resident) MO = src.bt / heads;
  if (MO < 1) MO = 1;
  const float* W0 = ly.flat + any_net.w_off[L];
  const float* B0 = ly.flat + any_net.b_off[L];
  const int64_t w_stride = (int64_t)a.t_net.w_off[L] - a.s_net.w_off[L], b_stride = (int64_t)a.t_net.b_off[L] - a.s_net.b_off[L];
  float ld[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t) ld[t] = 0.f;
  // the transformed half runs kRing output tiles ahead in a register ring (see net_to_hidden)
  f32x4 r1[kRing][NTL];
  if (!PREFILL) {
#pragma unroll
    for (int u = 0; u < kRing; ++u)
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        if constexpr (NOISE != 0) r1[u][t] = in4(t, act_off, 16 * (u < M ? u : M - 1) + 4 * q);
        else r1[u][t] = load4(xrow[t] + act_off, 16 * (u < M ? u : M - 1) + 4 * q, H, vec);
      }
  }
  Chunk c{nullptr, nullptr};
  int next_start = 0, chunk_start = 0;
  for (int m_base = 0; m_base < M; m_base += kRing) {
#pragma unroll
    for (int u = 0; u < kRing; ++u) {
      const int m = m_base + u;
      if (m >= M) continue;
      if (m == next_start) {  // (uniform) a new chunk of output tiles starts here
        const int mo = M - m < MO ? M - m : MO;
        c = src.template chunk<PREFILL>(mo * heads * KS, DenseMMajor{W0, any_net.sizes[L], H, KS, m, heads, w_stride}, mo * heads,
                                        DenseBiasHeads{B0, H, m, heads, b_stride});
        chunk_start = m;
        next_start = m + mo;
      }
      if (PREFILL) continue;
      const int ml = m - chunk_start;
      const int col = 16 * m + 4 * q;
      f32x4 x1[NTL], s[NTL], tt[NTL];
      const int m_ahead = m + kRing < M ? m + kRing : M - 1;
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        x1[t] = r1[u][t];
        if constexpr (NOISE != 0) r1[u][t] = in4(t, act_off, 16 * m_ahead + 4 * q);
        else r1[u][t] = load4(xrow[t] + act_off, 16 * m_ahead + 4 * q, H, vec);
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        tt[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (both) {
        out_tile<MT_MAX, NTL>(c.A, (ml * 2) * KS, KS, c.bias + (ml * 2) * 16, lane, q, hs, wup, s);
        out_tile<MT_MAX, NTL>(c.A, (ml * 2 + 1) * KS, KS, c.bias + (ml * 2 + 1) * 16, lane, q, ht, wup, tt);
      } else {
        f32x4 o[NTL];
        out_tile<MT_MAX, NTL>(c.A, ml * KS, KS, c.bias + ml * 16, lane, q, ht, wup, o);
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
          if (a.has_scale) s[t] = o[t];
          else tt[t] = o[t];
        }
      }
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
        f32x4 y1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // forward: exp(s) z1 + t (:57); inverse: (z1 - t) / exp(s) (:53)
          y1[r] = NOISE == 0 && a.inverse ? (x1[t][r] - tt[t][r]) * __builtin_amdgcn_exp2f(-s[t][r] * kLog2e)
                            : __builtin_amdgcn_exp2f(s[t][r] * kLog2e) * x1[t][r] + tt[t][r];
          ld[t] += s[t][r];  // (padded columns: zero weights and bias, s = 0)
          if constexpr (NOISE != 0) sq[t] += col + r < H ? x1[t][r] * x1[t][r] : 0.f;  // (|z|^2 of the generated row, for log_q)
          else sq[t] += col + r < H ? y1[r] * y1[r] : 0.f;
        }
        store4(yrow[t] + act_off, col, H, vec, live[t], y1);
      }
    }
  }
  if (PREFILL) return;
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
    const int64_t r = row0 + (int64_t)(wave * NTL + t) * 16 + j;
    const float total = sum_over_q(NOISE == 0 && a.inverse ? -ld[t] : ld[t]);  // log_det = s.sum(1), sign flipped on the way back (:55, :62)
    const float sqt = sum_over_q(sq[t]);
    if constexpr (NOISE != 0) {
      if (q == 0 && live[t] && nz.log_q)
        nz.log_q[r] = first ? (-0.5f * sqt - (float)a.dim * kHalfLog2Pi) - total : nz.log_q[r] - total;
    } else if (q == 0 && live[t]) {
      float ld_row = total;
      if (a.log_det) {
        if (ly.accumulate) ld_row = a.log_det[r] + total;
        a.log_det[r] = ld_row;
      }
      if (ly.ysq) ly.ysq[r] = sqt;
      if (ly.lp) {  // log N(y_r; 0, I) + log_det, as gauss_logprob_sq_kernel (mnf_generic.hip) forms it
        const float lp = ld_row + (-0.5f * sqt - (float)a.dim * kHalfLog2Pi);
        if (ly.log_prob) ly.log_prob[r] = lp;
        if (a.lp_sum) atomicAdd(lp_slot(wave), (double)lp);  // the wave's fp64 slot in LDS
      }
    }
  }
}

template <int MT_MAX, int NTL, int NW, bool RESIDENT, int VEC>
__global__ void __launch_bounds__(NW * 64) ahf_rt_kernel(AhfRtArgs a) {
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + 16;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  rt::Source<RESIDENT> src{blocks, bias, a.cb, a.bt, 0, 0, 0, 1.f, 0};
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * NTL * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  const int64_t plane = a.rows * a.dim;
  // layers outermost: one layer's weights in LDS at a time; the workgroup keeps its row blocks through all layers
#pragma unroll 1
  for (int i = 0; i < a.n_layers; ++i) {
    const int l = a.inverse ? a.n_layers - 1 - i : i;
    const bool last = i == a.n_layers - 1;
    AhfRtLayer ly;
    ly.x = i == 0 ? a.x : a.mid ? a.mid + (i - 1) * plane : a.y;
    ly.y = last || !a.mid ? a.y : a.mid + i * plane;
    ly.flat = a.flat + (int64_t)l * a.n_params;
    ly.ysq = last ? a.ysq : nullptr;
    ly.log_prob = last ? a.log_prob : nullptr;
    ly.lp = last && (a.log_prob || a.lp_sum);
    ly.parity = (a.parity >> l) & 1u;
    ly.accumulate = i > 0 || a.accumulate;
    // (the two barriers in here also keep this layer's staging behind the other waves' last reads of the previous one's)
    float wmx = rt::net_weight_max(ly.flat, a.s_net, 0.f);  // (one net only: s_net and t_net are the same descriptor)
    if (a.has_scale && a.has_shift) wmx = rt::net_weight_max(ly.flat, a.t_net, wmx);
    const float wmax = rt::block_weight_max(wmx, scratch);
    const int e = rt::weight_exponent(wmax);  // weights are staged as w 2^-e: the largest one just below 2^15
    const float wup = rt::pow2f(e);
    src.wdown = rt::pow2f(-e);
    if (ly.lp && a.lp_sum && (threadIdx.x & 63) == 0) lp_slot(threadIdx.x >> 6)[0] = 0.0;
    if (RESIDENT) {
      src.slot = 0;
      src.btile = 0;
      ahf_rt_block<MT_MAX, NTL, VEC, true>(a, ly, src, wup, 0);
      __syncthreads();
    }
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
      src.slot = 0;
      src.btile = 0;
      ahf_rt_block<MT_MAX, NTL, VEC, false>(a, ly, src, wup, b * rows_per_block);
    }
  }
  if (a.lp_sum && (threadIdx.x & 63) == 0) atomicAdd(a.lp_sum, lp_slot(threadIdx.x >> 6)[0]);
}

// SAMPLE (see the head of this file): of `a` the output y, the parameters and the shape are used; a.inverse is 0
struct AhfRtSampleArgs {
  AhfRtArgs a;
  AhfRtNoise nz;
};
template <int MT_MAX, int NTL, int NW, bool RESIDENT, int VEC>
__global__ void __launch_bounds__(NW * 64) ahf_rt_sample_kernel(AhfRtSampleArgs s) {
  const AhfRtArgs& a = s.a;
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + 16;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  rt::Source<RESIDENT> src{blocks, bias, a.cb, a.bt, 0, 0, 0, 1.f, 0};
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * NTL * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  // ahf_rt_kernel's layer loop, forward and in place: layer 0 generates its rows, the later ones read y
#pragma unroll 1
  for (int l = 0; l < a.n_layers; ++l) {
    AhfRtLayer ly;
    ly.x = a.y;  // (layer 0: not read)
    ly.y = a.y;
    ly.flat = a.flat + (int64_t)l * a.n_params;
    ly.ysq = nullptr;
    ly.log_prob = nullptr;
    ly.lp = 0;
    ly.parity = (a.parity >> l) & 1u;
    ly.accumulate = 0;
    float wmx = rt::net_weight_max(ly.flat, a.s_net, 0.f);
    if (a.has_scale && a.has_shift) wmx = rt::net_weight_max(ly.flat, a.t_net, wmx);
    const float wmax = rt::block_weight_max(wmx, scratch);
    const int e = rt::weight_exponent(wmax);
    const float wup = rt::pow2f(e);
    src.wdown = rt::pow2f(-e);
    if (RESIDENT) {
      src.slot = 0;
      src.btile = 0;
      ahf_rt_block<MT_MAX, NTL, VEC, true, 1>(a, ly, src, wup, 0, s.nz, false);
      __syncthreads();
    }
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
      src.slot = 0;
      src.btile = 0;
      ahf_rt_block<MT_MAX, NTL, VEC, false, 1>(a, ly, src, wup, b * rows_per_block, s.nz, l == 0);
    }
  }
}

// The launch of a shape (`aligned`: x and y 16-byte aligned), or false: the VALU kernel takes it.  Fills the kernel
// arguments' shape part.
static bool ahf_rt_plan(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift, bool aligned, AhfRtArgs& a,
                        RtPlan& p) {
  if (dim < 2 || (dim & 1) || n_hidden < 1 || !hidden_ok(n_hidden, hidden) || (!has_scale && !has_shift)) return false;
  const int H = dim / 2;
  int sizes[MNF_MAX_LINEAR + 1];
  sizes[0] = H;
  const HiddenWidths w = scan_hidden(n_hidden, hidden, sizes);
  sizes[n_hidden + 1] = H;
  // (widths < 4: a sum of one or two split products is not a 1e-5 sum, flows.py _MIN_SPLIT_HIDDEN)
  if (w.min < 4 || w.max > 256) return false;
  const int64_t n_params = ahf_layout(n_hidden, sizes, has_scale, has_shift, a);
  if (!n_params) return false;
  a.n_params = (int)n_params;
  a.vec = dim % 8 == 0 && aligned;
  // blocks and bias tiles of the whole conditioner (the resident image): every layer of each net there is
  const int heads = (has_scale ? 1 : 0) + (has_shift ? 1 : 0);
  StagedTiles image = mlp_tiles(sizes, n_hidden + 1, H);
  image.blocks *= heads;
  image.bias *= heads;
  // Rows that are not 16-byte aligned (dim not a multiple of 8, a view at an odd offset) have the resident variant only,
  // except in the widest class, whose streaming kernel takes the alignment at run time (a branch around every row access:
  // 15-20 % on the memory-bound shapes) and serves every width: such a call goes there.
  plan_staging(a, p, image, /*resident_bytes=*/158 * 1024, /*stream=*/16);
  p.mt_max = !p.resident && !a.vec ? 16 : rt_size_class(w.max);
  p.nw = rt_fwd_waves(p);
  return true;
}

// the plan's kernel (vec: the arguments' a.vec), its dynamic-LDS attribute set
template <int MT_MAX, int NW>
static void (*ahf_rt_kernel_class(const RtPlan& p, bool vec))(AhfRtArgs) {
  constexpr int kStreamVec = MT_MAX == 16 ? 2 : 1;
  static DeviceMemo attr;
  allow_big_lds(attr, ahf_rt_kernel<MT_MAX, 1, NW, true, 1>, ahf_rt_kernel<MT_MAX, 1, NW, false, kStreamVec>,
                ahf_rt_kernel<MT_MAX, 1, NW, true, 0>);
  return !p.resident ? ahf_rt_kernel<MT_MAX, 1, NW, false, kStreamVec>
                     : vec ? ahf_rt_kernel<MT_MAX, 1, NW, true, 1> : ahf_rt_kernel<MT_MAX, 1, NW, true, 0>;
}
static void (*ahf_rt_kernel_of(const RtPlan& p, bool vec))(AhfRtArgs) {
  return p.mt_max == 4 ? ahf_rt_kernel_class<4, 8>(p, vec)
                       : p.mt_max == 8 ? ahf_rt_kernel_class<8, 8>(p, vec) : ahf_rt_kernel_class<16, 4>(p, vec);
}

// ... and its sampling twin
template <int MT_MAX, int NW>
static void (*ahf_rt_sample_kernel_class(const RtPlan& p, bool vec))(AhfRtSampleArgs) {
  constexpr int kStreamVec = MT_MAX == 16 ? 2 : 1;
  static DeviceMemo attr;
  allow_big_lds(attr, ahf_rt_sample_kernel<MT_MAX, 1, NW, true, 1>, ahf_rt_sample_kernel<MT_MAX, 1, NW, false, kStreamVec>,
                ahf_rt_sample_kernel<MT_MAX, 1, NW, true, 0>);
  return !p.resident ? ahf_rt_sample_kernel<MT_MAX, 1, NW, false, kStreamVec>
                     : vec ? ahf_rt_sample_kernel<MT_MAX, 1, NW, true, 1> : ahf_rt_sample_kernel<MT_MAX, 1, NW, true, 0>;
}
static void (*ahf_rt_sample_kernel_of(const RtPlan& p, bool vec))(AhfRtSampleArgs) {
  return p.mt_max == 4 ? ahf_rt_sample_kernel_class<4, 8>(p, vec)
                       : p.mt_max == 8 ? ahf_rt_sample_kernel_class<8, 8>(p, vec) : ahf_rt_sample_kernel_class<16, 4>(p, vec);
}

// Which runs go out as one launch: 1 .. 32 layers of a shape the kernel has.  Measured out: runs of the widest class's
// STREAMING shapes (hidden widths 129 .. 256 whose conditioner does not fit LDS: every row block re-stages the weights, the
// pass is bound by that staging, and nine layers in one launch were 4 % slower than nine launches -- 9.17 against 8.80 ns
// per row and layer at dim = 256, (200, 130, 40, 7), 262,144 rows); one layer of them is today's call.
static bool ahf_rt_stack_ok(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift, int n_layers) {
  AhfRtArgs a;
  RtPlan p;
  if (n_layers < 1 || n_layers > 32 || !ahf_rt_plan(dim, n_hidden, hidden, has_scale, has_shift, true, a, p)) return false;
  return n_layers == 1 || p.resident || p.mt_max != 16;
}

// A run of n_layers layers (see the head of this file; n_layers = 1: mid, log_prob, lp_sum NULL and `flats` the layer's
// vector).  MNF_ERR_UNSUPPORTED: the shape is outside the run-time-shaped kernel too.
int ahf_rt_stack_launch(const float* x, float* y, float* mid, float* log_det, float* ysq, float* log_prob, double* lp_sum,
                        int accumulate, const float* flats, uint32_t parity_bits, int n_layers, int64_t rows, int dim,
                        int inverse, int n_hidden, const int* hidden, int has_scale, int has_shift, hipStream_t stream) {
  if (!flats || rows * dim >= (1ll << 40) || (n_layers > 1 && rows * dim * (n_layers - 1) >= (1ll << 42)))
    return MNF_ERR_UNSUPPORTED;
  AhfRtArgs a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  if (!ahf_rt_plan(dim, n_hidden, hidden, has_scale, has_shift, aligned16(x, y, mid), a, p)) return MNF_ERR_UNSUPPORTED;
  a.x = x; a.y = y; a.mid = n_layers > 1 ? mid : nullptr; a.log_det = log_det; a.ysq = ysq; a.log_prob = log_prob;
  a.lp_sum = lp_sum; a.flat = flats; a.rows = rows; a.dim = dim; a.parity = parity_bits; a.n_layers = n_layers;
  a.inverse = inverse != 0; a.accumulate = accumulate != 0;
  a.has_scale = has_scale != 0; a.has_shift = has_shift != 0;
  return launch_plan(ahf_rt_kernel_of(p, a.vec != 0), a, p, 1, rows, n_layers > 1 ? "ahf_stack_rt" : "ahf_rt", stream);
}

// The seeded sample of a run (log_q NULL: x only): the forward launch without intermediates whose first layer generates
// its rows.  The plan is the forward launch's for the same y (an x that is not there constrains nothing).
int ahf_rt_sample_launch(uint64_t seed, int64_t row0, float* y, float* log_q, const float* flats, uint32_t parity_bits,
                                int n_layers, int64_t rows, int dim, int n_hidden, const int* hidden, int has_scale,
                                int has_shift, hipStream_t stream) {
  if (rows * dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  AhfRtSampleArgs s;
  memset(&s, 0, sizeof(s));
  RtPlan p;
  if (!ahf_rt_plan(dim, n_hidden, hidden, has_scale, has_shift, aligned16(y), s.a, p)) return MNF_ERR_UNSUPPORTED;
  s.a.y = y; s.a.flat = flats; s.a.rows = rows; s.a.dim = dim; s.a.parity = parity_bits; s.a.n_layers = n_layers;
  s.a.has_scale = has_scale != 0; s.a.has_shift = has_shift != 0;
  s.nz.seed = seed; s.nz.row0 = row0; s.nz.log_q = log_q;
  const char* tag = n_layers > 1 ? (log_q ? "ahf_stack_rt_sample_lq" : "ahf_stack_rt_sample")
                                 : (log_q ? "ahf_rt_sample_lq" : "ahf_rt_sample");
  return launch_plan(ahf_rt_sample_kernel_of(p, s.a.vec != 0), s, p, 1, rows, tag, stream);
}

// one layer; MNF_ERR_UNSUPPORTED: the shape is outside the run-time-shaped kernel too (the caller runs the VALU kernel)
int ahf_rt_launch(const float* x, float* y, float* log_det, float* ysq, int accumulate, const float* flat, int64_t rows,
                  int dim, int parity, int inverse, int n_hidden, const int* hidden, int has_scale, int has_shift,
                  hipStream_t stream) {
  return ahf_rt_stack_launch(x, y, nullptr, log_det, ysq, nullptr, nullptr, accumulate, flat, parity ? 1u : 0u, 1, rows, dim,
                             inverse, n_hidden, hidden, has_scale, has_shift, stream);
}

}  // namespace mnf

extern "C" int mnf_affine_half_rt_supported(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift) {
  return mnf::rt_has_plan<mnf::AhfRtArgs>([&](mnf::AhfRtArgs& a, mnf::RtPlan& p) {
    return mnf::ahf_rt_plan(dim, n_hidden, hidden, has_scale, has_shift, true, a, p);
  });
}

extern "C" int mnf_affine_half_rt_stack_supported(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift,
                                                  int n_layers) {
  return mnf::ahf_rt_stack_ok(dim, n_hidden, hidden, has_scale, has_shift, n_layers) ? 1 : 0;
}

extern "C" int mnf_affine_half_rt_stack(const float* x, float* y, float* intermediates, float* log_det, float* y_sqnorm,
                                        float* log_prob, double* log_prob_sum, int accumulate, const float* flats,
                                        const int* parity_host, int n_layers, int64_t rows, int dim, int inverse,
                                        int n_hidden, const int* hidden, int has_scale, int has_shift, void* stream) {
  if (!x || !y || x == y || !flats || !parity_host || n_layers < 1 || n_layers > 32 || rows < 0 || dim < 2 || (dim & 1) ||
      !mnf::hidden_ok(n_hidden, hidden) || (!has_scale && !has_shift) || ((log_prob || log_prob_sum) && !log_det) ||
      (intermediates && (intermediates == x || intermediates == y)) ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(intermediates) |
        reinterpret_cast<uintptr_t>(flats) | reinterpret_cast<uintptr_t>(log_det) | reinterpret_cast<uintptr_t>(y_sqnorm) |
        reinterpret_cast<uintptr_t>(log_prob)) & 3) ||
      (reinterpret_cast<uintptr_t>(log_prob_sum) & 7))
    return MNF_ERR_INVALID_ARG;
  if (rows == 0) return MNF_OK;
  if (!mnf_affine_half_rt_stack_supported(dim, n_hidden, hidden, has_scale, has_shift, n_layers)) return MNF_ERR_UNSUPPORTED;
  uint32_t bits = 0;
  for (int l = 0; l < n_layers; ++l) bits |= (parity_host[l] ? 1u : 0u) << l;
  return mnf::ahf_rt_stack_launch(x, y, intermediates, log_det, y_sqnorm, log_prob, log_prob_sum, accumulate, flats, bits,
                                  n_layers, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, (hipStream_t)stream);
}

extern "C" int mnf_affine_half_rt_stack_sample_supported(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift,
                                                         int n_layers) {
  return mnf_affine_half_rt_stack_supported(dim, n_hidden, hidden, has_scale, has_shift, n_layers);
}

// both sampling entries behind their argument checks (with_logq: log_q is required)
static int rt_stack_sample(uint64_t seed, int64_t row0, float* y, float* log_q, bool with_logq, const float* flats,
                           const int* parity_host, int n_layers, int64_t rows, int dim, int n_hidden, const int* hidden,
                           int has_scale, int has_shift, void* stream) {
  if (!y || !flats || !parity_host || (with_logq && !log_q) || n_layers < 1 || n_layers > 32 || rows < 0 || row0 < 0 || dim < 2 ||
      (dim & 1) || !mnf::hidden_ok(n_hidden, hidden) || (!has_scale && !has_shift) ||
      ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(flats) | reinterpret_cast<uintptr_t>(log_q)) & 3))
    return MNF_ERR_INVALID_ARG;
  if (rows == 0) return MNF_OK;
  if (!mnf_affine_half_rt_stack_sample_supported(dim, n_hidden, hidden, has_scale, has_shift, n_layers)) return MNF_ERR_UNSUPPORTED;
  uint32_t bits = 0;
  for (int l = 0; l < n_layers; ++l) bits |= (parity_host[l] ? 1u : 0u) << l;
  return mnf::ahf_rt_sample_launch(seed, row0, y, log_q, flats, bits, n_layers, rows, dim, n_hidden, hidden, has_scale, has_shift,
                                   (hipStream_t)stream);
}

extern "C" int mnf_affine_half_rt_stack_sample(uint64_t seed, int64_t row0, float* y, const float* flats, const int* parity_host,
                                               int n_layers, int64_t rows, int dim, int n_hidden, const int* hidden,
                                               int has_scale, int has_shift, void* stream) {
  return rt_stack_sample(seed, row0, y, nullptr, false, flats, parity_host, n_layers, rows, dim, n_hidden, hidden, has_scale,
                         has_shift, stream);
}

extern "C" int mnf_affine_half_rt_stack_sample_logq(uint64_t seed, int64_t row0, float* y, float* log_q, const float* flats,
                                                    const int* parity_host, int n_layers, int64_t rows, int dim, int n_hidden,
                                                    const int* hidden, int has_scale, int has_shift, void* stream) {
  return rt_stack_sample(seed, row0, y, log_q, true, flats, parity_host, n_layers, rows, dim, n_hidden, hidden, has_scale,
                         has_shift, stream);
}
