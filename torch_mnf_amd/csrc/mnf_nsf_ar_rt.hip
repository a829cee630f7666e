// NSF_AR.inverse (torch_mnf/flows/spline_flow.py:218-235: x -> z, the direction log_prob and training run through) for any
// dim >= 2, K <= 16 and 1 .. 4 hidden layers of 4 .. 16 units on the f16 matrix pipe (mnf_rt.h), weights read from the
// plain `flat` vector in mnf_nsf_ar's own layout.  Every conditioner reads the layer's INPUT, so the dim elements are
// independent: z_i, ld_i = RQS_forward(x_i; net_{i-1}(x[:, :i])), element 0 from init_param, log_det = sum_i ld_i.
//
// A wave owns kArTiles 16-row tiles, lane (row j, q).  The elements are walked in GROUPS of four, 4 g .. 4 g + 3, lane q
// handling element 4 g + q; the four nets of a group run as ONE block-diagonal net of width 4 n_h (unit u of net q' is
// unit q' n_h + u of the side-by-side layer):
//   * first layer: block row (q', u) holds the weights of net 4 g + q' against the columns < 4 g + q' of x, every other
//     column staged as exactly 0 (a select, never a multiply);
//   * hidden layers: the off-diagonal blocks are exactly 0;
//   * output layer: arranged as mnf_nsf_rt.hip's slots are, so that after its tiles lane (j, q) holds the 3K-1 raw spline
//     parameters of ITS element at compile-time positions; the spline then runs on 64 lanes (mnf_nsf_spline.h, one
//     direction only, chosen by a uniform switch over K);
//   * element 0 has no net: zero weights, the output bias = init_param; elements >= dim are padding (zero weights and
//     biases: finite parameters), they store nothing and add nothing to the log-det (selects).
// The weights do not stay resident (dim 64, n_h 8, K 5 is ~200 blocks of 2 KB): a group's blocks are streamed through the
// two LDS buffers of Source<false>, and every wave carries its kArTiles tiles through each staged group -- only the
// per-tile running log-det lives in registers across groups.  Rows holding non-finite values give NaN from the element
// after the first non-finite one on, as the reference does, and -- the four nets of a group share their input K-steps --
// possibly in the up to three elements before it that share its group.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mnf_nsf_ar_rt.h"
#include "mnf_nsf_spline.h"

#ifndef MNF_NSF_AR_TILES
#define MNF_NSF_AR_TILES 2  // row tiles per wave (profiles/r17/README.md)
#endif

namespace mnf {

constexpr int kArWaves = 8;
constexpr int kArTiles = MNF_NSF_AR_TILES;

// The group's output layer and spline for a compile-time K (the tiles of an element and the positions of its parameters
// are then static).  The wave's tiles take turns through ONE copy of the code: the tile's hidden vector is picked by
// uniform selects.  c: the staged output layer (TV tiles of KS blocks); row_first: the row of this lane in the wave's tile 0.
template <int NTL, int K>
__device__ __forceinline__ void ar_out(const NsfArRtArgs& a, const rt::Chunk& c, int KS, int g, float wup, int lane, int q,
                                       const rt::Hidden<4, NTL>& h, int64_t row_first, float (&lad)[NTL]) {
  using namespace rt;
  const ArLayout& L = a.L;
  constexpr int NW_ = (K + 3) / 4, ND_ = (K - 1 + 3) / 4, TV = 2 * NW_ + ND_;  // tiles of widths / heights, derivatives
  const int e = 4 * g + q;
  const bool real = e < L.n.dim;
#pragma unroll 1
  for (int t = 0; t < NTL; ++t) {
    const int64_t r = row_first + 16 * t;
    const bool live = r < a.rows;
    const int64_t at = (live ? r : a.rows - 1) * L.n.dim + (real ? e : 0);
    const float v = a.x[at];
    Hidden<4, 1> ht;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      ht.hi[0][m] = h.hi[0][m];
      ht.lo[0][m] = h.lo[0][m];
    }
    ht.up[0] = h.up[0];
#pragma unroll
    for (int tt = 1; tt < NTL; ++tt) {
      const bool pick = tt == t;  // (uniform)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        ht.hi[0][m] = pick ? h.hi[tt][m] : ht.hi[0][m];
        ht.lo[0][m] = pick ? h.lo[tt][m] : ht.lo[0][m];
      }
      ht.up[0] = pick ? h.up[tt] : ht.up[0];
    }
    // the element's parameter tiles -> the lane's 3K-1 raw parameters
    float p[3 * K - 1];
#pragma unroll
    for (int tv = 0; tv < TV; ++tv) {
      f32x4 o[1];
      out_tile<4, 1>(c.A, tv * KS, KS, c.bias + tv * 16, lane, q, ht, wup, o);
      const int cgrp = tv < NW_ ? 0 : tv < 2 * NW_ ? 1 : 2, k0 = 4 * (tv - cgrp * NW_);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k0 + i < (cgrp < 2 ? K : K - 1)) p[cgrp * K + k0 + i] = o[0][i];
    }
    float out, ld;
    rqs_regs<K, false, 3 * K - 1>(v, a.T, p, out, ld);
    if (real && live) a.y[at] = out;
#pragma unroll
    for (int tt = 0; tt < NTL; ++tt) lad[tt] += (tt == t && real) ? ld : 0.f;  // padding: a select, not a product
  }
}

template <int NTL, typename Src>
__device__ __forceinline__ void nsf_ar_rt_block(const NsfArRtArgs& a, Src& src, float wup, int64_t row0) {
  using namespace rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int64_t row_first = row0 + (int64_t)wave * NTL * 16 + j;
  const float* xrow[NTL];
  float lad[NTL];
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
    const int64_t r = row_first + 16 * t;
    xrow[t] = a.x + (r < a.rows ? r : a.rows - 1) * a.L.n.dim;
    lad[t] = 0.f;
  }
  const ArLayout& L = a.L;
  const int G = (L.n.dim + 3) >> 2, K = L.K, nh = L.n_hidden;
  const int KS = steps32(16 * tiles16(4 * L.hid[nh - 1])), TV = 2 * ((K + 3) >> 2) + ((K + 2) >> 2);  // the output layer
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    Hidden<4, NTL> h;
    ar_first_layer<NTL>(a, src, g, wup, lane, q, xrow, h);
    ar_hidden_layers<NTL>(a, src, g, wup, lane, q, h);
    const Chunk c = src.template chunk<false>(TV * KS, ArOutFetch{a.flat, L.n, g, K, L.hid[nh - 1], L.cw[nh], KS, TV}, TV,
                                              ArOutBias{a.flat, L.n, g, K, L.cb[nh]});
    switch (K) {  // (uniform)
#define MNF_NSF_AR_RT_CASE(KK) \
  case KK: ar_out<NTL, KK>(a, c, KS, g, wup, lane, q, h, row_first, lad); break;
      MNF_NSF_AR_RT_CASE(2) MNF_NSF_AR_RT_CASE(3) MNF_NSF_AR_RT_CASE(4) MNF_NSF_AR_RT_CASE(5) MNF_NSF_AR_RT_CASE(6)
      MNF_NSF_AR_RT_CASE(7) MNF_NSF_AR_RT_CASE(8) MNF_NSF_AR_RT_CASE(9) MNF_NSF_AR_RT_CASE(10) MNF_NSF_AR_RT_CASE(11)
      MNF_NSF_AR_RT_CASE(12) MNF_NSF_AR_RT_CASE(13) MNF_NSF_AR_RT_CASE(14) MNF_NSF_AR_RT_CASE(15) MNF_NSF_AR_RT_CASE(16)
#undef MNF_NSF_AR_RT_CASE
      default: break;
    }
  }
#pragma unroll
  for (int t = 0; t < NTL; ++t) {
    const int64_t r = row_first + 16 * t;
    const float total = sum_over_q(lad[t]);
    if (q == 0 && r < a.rows && a.log_det) a.log_det[r] = a.accumulate ? a.log_det[r] + total : total;
  }
}

template <int NW, int NTL>
__global__ void __launch_bounds__(NW * 64) nsf_ar_rt_kernel(NsfArRtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + 16;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  // one staging exponent per launch: the largest finite WEIGHT of all nets (biases and init_param are not looked at)
  float mx = 0.f;
  for (int e = 1; e < a.L.n.dim; ++e)
    for (int l = 0; l <= a.L.n_hidden; ++l) mx = rt::range_abs_max(a.flat + a.L.w(e, l), a.L.n_in(e, l) * a.L.n_out(l), mx);
  const int ex = rt::weight_exponent(rt::block_weight_max(mx, scratch));
  const float wup = rt::pow2f(ex);
  rt::Source<false> src{blocks, bias, a.cb, a.bt, 0, 0, 0, rt::pow2f(-ex), 0};
  const int64_t rows_per_block = (int64_t)NW * NTL * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) nsf_ar_rt_block<NTL>(a, src, wup, b * rows_per_block);
}

// The launch of a shape, or false: the VALU kernel takes it.  Fills the kernel arguments' shape part.
static bool nsf_ar_rt_plan(int dim, int K, int n_hidden, const int* hidden, NsfArRtArgs& a, RtPlan& p) {
  ArLayout& L = a.L;
  if (!ar_layout_plan(dim, K, n_hidden, hidden, L)) return false;
  p.mt_max = 4;
  set_staging(a, p, /*resident=*/false, kArStream, kArStream);
  p.nw = kArWaves;
  return true;
}

// the plan's kernel, its dynamic-LDS attribute set
static void (*nsf_ar_rt_kernel_of(const RtPlan&))(NsfArRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, nsf_ar_rt_kernel<kArWaves, kArTiles>);
  return nsf_ar_rt_kernel<kArWaves, kArTiles>;
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_nsf_ar_rt_supported(int dim, int K, int n_hidden, const int* hidden) {
  return rt_has_plan<NsfArRtArgs>([&](NsfArRtArgs& a, RtPlan& p) { return nsf_ar_rt_plan(dim, K, n_hidden, hidden, a, p); });
}

// workgroups of the launch (each walks the row blocks of 16 x tiles x waves rows blockIdx.x, + grid, ...); 0: no launch, or
// no device
extern "C" int64_t mnf_nsf_ar_rt_grid(int64_t rows, int dim, int K, int n_hidden, const int* hidden) {
  return rt_grid_query<NsfArRtArgs>(
      rows, kArTiles, [&](NsfArRtArgs& a, RtPlan& p) { return nsf_ar_rt_plan(dim, K, n_hidden, hidden, a, p); },
      nsf_ar_rt_kernel_of);
}

extern "C" int mnf_nsf_ar_rt(const float* x, float* y, float* log_det, int accumulate, const float* flat, int64_t rows, int dim,
                             int K, float tail_bound, int n_hidden, const int* hidden, void* stream) {
  if (!x || !y || x == y || !flat || rows < 0 || dim < 1 || K < 1 || !(tail_bound > 0.f) || !hidden_ok(n_hidden, hidden))
    return MNF_ERR_INVALID_ARG;
  if (1e-3 * K > 1.0) return MNF_ERR_DOMAIN;  // spline_flow.py:90-93
  if (rows == 0) return MNF_OK;
  if (rows * dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  NsfArRtArgs a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  if (!nsf_ar_rt_plan(dim, K, n_hidden, hidden, a, p)) return MNF_ERR_UNSUPPORTED;
  a.x = x; a.y = y; a.log_det = log_det; a.flat = flat; a.rows = rows; a.T = tail_bound;
  a.accumulate = accumulate != 0;
  a.vec = dim % 4 == 0 && aligned16(x);
  return launch_plan(nsf_ar_rt_kernel_of(p), a, p, kArTiles, rows, "nsf_ar_rt", (hipStream_t)stream);
}
