// Gradients of the one-pass direction of MAF / IAF (MAF.inverse, IAF.forward: torch_mnf/flows/maf.py:53-62 under
// loss.backward()) for MADE nets of 1 .. 4 hidden layers of widths 4 .. 64, any dim, on the f16 matrix pipe: run-time
// shapes (mnf_rt.h, mnf_rt_bwd.h), weights read from the plain `flat` parameter vector, masks from mnf_maf's byte buffer.
//
// A workgroup owns a block of 16 NW rows, a wave one tile of it: forward recompute of the masked net keeping every hidden
// vector; then the last MaskedLinear two 16-dim output tiles at a time as two heads (s = rows 0 .. dim-1, t = the next
// dim) -- s and t of the tiles, the cotangents
//   d s_j = G_j x_j e^{s_j} + g_ld      d t_j = G_j      grad_x_j = G_j e^{s_j}      (G_j = grad_y at column j, dim-1-j when parity)
// the first step of the delta chain  W_s^T d s + W_t^T d t  and the tiles' dW products through the LDS exchange area --,
// then the hidden layers backwards through the ReLU derivative (0 at 0) and the first layer input tile by input tile
// (grad_x += W_0^T delta_1, dW_0 += delta_1 (x) x): mnf_rt_bwd.h backward_tail.  Every weight is staged under its mask (a
// select), and a masked-out weight's gradient entry receives no add at all (MaskKeep).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mnf_hip.h"
#include "mnf_rnvp_common.h"
#include "mnf_rt_bwd.h"

namespace mnf {

struct MafBwdRtArgs {
  const float* x;
  const float* grad_y;
  const float* grad_ld;
  float* grad_x;
  float* grad_flat;
  const float* flat;
  const uint8_t* masks;
  const float* gscale_dev;
  int64_t rows;
  int dim, parity, n_params, vec;
  int s_w, s_b;  // float offsets of the last MaskedLinear (s = its first dim rows, t = the next dim)
  int cb, bt, block_words, bias_words;
  int ht_tiles, dt_tiles, ct_tiles;
  int m_off[MNF_MAX_LINEAR];  // byte offset of layer l's mask
  NetDesc net;                // dim -> h_1 .. h_n
  int64_t slot_floats;        // 0; mnf_maf_bwd_rt_det: workgroup b adds into grad_flat + b * slot_floats (mnf_rt_host.h)
};

// columns col .. col + 3 of a row seen flipped (column c <-> d-1-c): zeros beyond d; vec: one dwordx4 (d % 4 == 0).  No load
// under a divergent branch.
__device__ __forceinline__ f32x4 load4_flipped(const float* __restrict__ row, int col, int d, bool vec) {
  if (vec) {
    const bool ok = col < d;
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + (ok ? d - 4 - col : 0));
    return ok ? f32x4{v[3], v[2], v[1], v[0]} : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = col + r < d;
    const float g = row[ok ? d - 1 - col - r : 0];
    v[r] = ok ? g : 0.f;
  }
  return v;
}

template <int MT_MAX>
__global__ void __launch_bounds__(512) maf_bwd_rt_kernel(MafBwdRtArgs a) {
  using namespace rt;
  const bool VEC = a.vec != 0;  // (uniform) rows are 16-byte aligned: dwordx4 row accesses
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4, nw = blockDim.x >> 6;
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + kBwdHeadWords;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  const BwdLds lds = bwd_lds(rt_lds, bias + a.bias_words, a.ht_tiles, a.dt_tiles, a.ct_tiles);
  const NetDesc& nd = a.net;
  const int n_hid = nd.n_lin;  // every layer of `net` ends in a hidden vector, each with its ReLU
  const int d = a.dim;
  const uint8_t* M0 = a.masks + a.m_off[n_hid];  // the last MaskedLinear's mask: (h_n, 2 dim)
  float wmx = net_weight_max(a.flat, nd, a.masks, a.m_off, 0.f);
  wmx = masked_abs_max(a.flat + a.s_w, M0, nd.sizes[n_hid], 2 * d, wmx);
  const float wmax = block_weight_max(wmx, scratch);
  const int we = weight_exponent(wmax);
  const float wup = pow2f(we);
  Source<false> src{blocks, bias, a.cb, a.bt, 0, 0, 0, pow2f(-we), 0};
  const float gs = *a.gscale_dev, inv_gs = 1.f / gs;
  const MaskedLayersBwd layers{{a.masks, a.m_off, nd.sizes}};
  const int hl = nd.sizes[n_hid], MTh = tiles16(hl), KSh = steps32(16 * MTh), M = tiles16(d);
  const int t_w = a.s_w + d * hl, t_b = a.s_b + d;
  const int ht_last = exH_tile_of(nd, n_hid);
  const int64_t n_blocks = (a.rows + 16 * nw - 1) / (16 * nw);
  float* const gflat = a.grad_flat + blockIdx.x * a.slot_floats;
  float* const sC2 = lds.sH + (kMaxBwdLayers + 1) * 8;  // (the head's spare 8 floats) scales of the t cotangent tiles

  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t r = blk * (16 * nw) + 16 * wave + j;
    const bool live = r < a.rows;
    const int64_t rc = live ? r : a.rows - 1;
    const float* xrow = a.x + rc * d;
    const float* gyrow = a.grad_y ? a.grad_y + rc * d : xrow;
    float* gxrow = a.grad_x + rc * d;
    const float gl = a.grad_ld && live ? a.grad_ld[rc] : 0.f;
    const float rowmask = live ? 1.f : 0.f;
    // ---- forward recompute, every hidden vector kept
    Hidden<MT_MAX, 1> h;
    {
      auto load_x = [&](int, int ks, f32x4& xa, f32x4& xb) {
        const int c0 = 32 * ks + 4 * q;
        xa = load4(xrow, c0, d, VEC);
        xb = load4(xrow, c0 + 16, d, VEC);
      };
      forward_keep<MT_MAX>(src, a.flat, nd, n_hid, -1, wup, lds, load_x, h, layers);
    }
    // ---- the last layer, two 16-dim tiles per round: [s | t blocks] -> cotangents -> [W_s^T | W_t^T blocks] -> chain
    Acc<MT_MAX, 1> accd;
    accd.zero();
    float downd = 1.f;
    for (int m0 = 0; m0 < M; m0 += 2) {
      const int mo = M - m0 < 2 ? M - m0 : 2;
      uint32_t* buf = src.cur_blocks();
      float* bbuf = src.cur_bias();
      stage_blocks(buf, mo * 2 * KSh, MaskedMMajor{a.flat + a.s_w, hl, d, KSh, m0, 2, (int64_t)d * hl, M0, 2 * d, d}, src.wdown);
      stage_bias(bbuf, mo * 2, DenseBiasHeads{a.flat + a.s_b, d, m0, 2, d});
      src.commit();
      f32x4 gs2[2], gt2[2];
#pragma unroll
      for (int ml = 0; ml < 2; ++ml) {
        gs2[ml] = f32x4{0.f, 0.f, 0.f, 0.f};
        gt2[ml] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ml < mo) {
          const int col = 16 * (m0 + ml) + 4 * q;
          f32x4 s4[1], t4[1];
          out_tile<MT_MAX, 1>(buf, (ml * 2) * KSh, KSh, bbuf + (ml * 2) * 16, lane, q, h, wup, s4);
          out_tile<MT_MAX, 1>(buf, (ml * 2 + 1) * KSh, KSh, bbuf + (ml * 2 + 1) * 16, lane, q, h, wup, t4);
          const f32x4 xx = load4(xrow, col, d, VEC);
          const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
          const f32x4 G = !a.grad_y ? zero4 : a.parity ? load4_flipped(gyrow, col, d, VEC) : load4(gyrow, col, d, VEC);
          f32x4 gx;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float es = exp6r(s4[0][e]);
            gx[e] = G[e] * es;  // the direct term of y_j = x_j e^{s_j} + t_j
            const bool real = col + e < d;
            gs2[ml][e] = real ? __builtin_fmaf(G[e] * xx[e], es, gl) * gs * rowmask : 0.f;
            gt2[ml][e] = real ? G[e] * gs * rowmask : 0.f;
          }
          store4(gxrow, col, d, VEC, live, gx);
        }
      }
      // dW, db of the two tiles: cotangent tiles [s0 s1 t0 t1] x last hidden vector, an exchange scale per head (d s
      // carries the factor x e^s, which must not push d t down to f16's subnormals)
      if (gflat) {
        f32x4 cs[MT_MAX], ct[MT_MAX];
#pragma unroll
        for (int m = 0; m < MT_MAX; ++m) {
          cs[m] = m < 2 ? gs2[m & 1] : f32x4{0.f, 0.f, 0.f, 0.f};
          ct[m] = m < 2 ? gt2[m & 1] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float scs = exchange_store<MT_MAX>(cs, 2, lds.exC, 0, 16 * wave, lane, lds.ident);
        const float sct = exchange_store<MT_MAX>(ct, 2, lds.exC, 2, 16 * wave, lane, lds.ident);
        if (lane == 0) {
          lds.sC[wave] = scs;
          sC2[wave] = sct;
        }
      }
      // the chain's first step: accd += W_s^T-blocks x [d s tiles] + W_t^T-blocks x [d t tiles]
      uint32_t* bufT = src.cur_blocks();
      stage_blocks(bufT, MTh, MaskedTKMajor{a.flat + a.s_w, hl, d, MTh, m0 >> 1, M0, 2 * d}, src.wdown);
      stage_blocks(bufT + MTh * kBlockWords, MTh, MaskedTKMajor{a.flat + t_w, hl, d, MTh, m0 >> 1, M0 + d, 2 * d}, src.wdown);
      src.commit();  // (also: the cotangent tiles are in the exchange area)
#pragma unroll
      for (int head = 0; head < 2; ++head) {
        const f32x4& g0 = head == 0 ? gs2[0] : gt2[0];
        const f32x4& g1 = head == 0 ? gs2[1] : gt2[1];
        f16x8 bh[1], bl[1];
        float mx = 0.f;
        split_kstep(g0, g1, downd, bh[0], bl[0], mx);
        if (__builtin_expect(wave_any(!(mx < kSplitLimit)), 0)) {
          float fm = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) fm = __builtin_fmaxf(fm, __builtin_fmaxf(finite_abs(g0[e]), finite_abs(g1[e])));
          const float want = pow2f(-down_exponent(max_over_q(fm), 13));
          if (want < downd) {
            const float f = want / downd;
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) {
              accd.main[0][m] *= f;
              accd.corr[0][m] *= f;
            }
            downd = want;
          }
          float unused = 0.f;
          split_kstep(g0, g1, downd, bh[0], bl[0], unused);
        }
        mac_kstep<MT_MAX, 1>(bufT, head * MTh, MTh, lane, bh, bl, accd.main, accd.corr);
      }
      if (gflat) {
        dw_phase(lds.exC, 0, mo, lds.exH, ht_last, MTh, lds.sC, lds.sH + n_hid * 8, nw, inv_gs, gflat + a.s_w, gflat + a.s_b, d, hl,
                 m0, 0, MaskKeep{M0, 2 * d});
        dw_phase(lds.exC, 2, mo, lds.exH, ht_last, MTh, sC2, lds.sH + n_hid * 8, nw, inv_gs, gflat + t_w, gflat + t_b, d, hl, m0, 0,
                 MaskKeep{M0 + d, 2 * d});
      }
    }
    // ---- through the last hidden vector's ReLU, the hidden layers backwards, then the first layer: grad_x += W_0^T delta_1
    f32x4 dv[MT_MAX];
    chain_result<MT_MAX, true>(accd, wup / downd, lds.meta_bits[n_hid * 64 + lane], dv);
    auto load_in = [&](int mi) { return load4(xrow, 16 * mi + 4 * q, d, VEC); };
    auto add_in = [&](int mi, const f32x4& g) {
      const int col = 16 * mi + 4 * q;
      const f32x4 base = load4(gxrow, col, d, VEC);
      store4(gxrow, col, d, VEC, live, base + g);
    };
    backward_tail<MT_MAX>(src, a.flat, gflat, nd, n_hid, -1, dv, lds, wup, inv_gs, d, load_in, add_in, layers);
  }
}

// The launch of a shape, or false: the VALU kernel takes it.  Fills the kernel arguments' shape part.
static bool maf_bwd_rt_plan(int dim, int n_hidden, const int* hidden, MafBwdRtArgs& a, RtPlan& p) {
  if (dim < 1 || n_hidden < 1 || n_hidden > rt::kMaxBwdLayers || !hidden_ok(n_hidden, hidden)) return false;
  int sizes[MNF_MAX_LINEAR + 1];
  sizes[0] = dim;
  const HiddenWidths w = scan_hidden(n_hidden, hidden, sizes);
  if (w.min < 4 || w.max > 64) return false;  // the one size class built (4 hidden tiles)
  const int64_t n_params = maf_layout(dim, n_hidden, sizes, a);
  if (!n_params) return false;
  a.n_params = (int)n_params;
  p.mt_max = 4;
  p.resident = false;
  a.cb = rt::bwd_head_round_blocks(hidden[n_hidden - 1], hidden[0]);  // (the heads: the last MaskedLinear's s and t)
  a.bt = 4;
  a.ht_tiles = w.tiles;
  a.dt_tiles = 0;  // (the deltas reuse the hidden vectors' tiles: mnf_rt_bwd.h backward_tail)
  // (the output-layer chunks need four tiles: [s0 s1 t0 t1])
  const int KS1 = (16 * ((hidden[0] + 15) / 16) + 31) / 32;
  return rt::fit_bwd_lds(a, a, p, {/*nw_max=*/8, a.cb, a.cb, 1, KS1, /*ct_min=*/4, /*ct_max=*/p.mt_max});
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_maf_bwd_rt_supported(int dim, int n_hidden, const int* hidden) {
  return rt_has_plan<MafBwdRtArgs>([&](MafBwdRtArgs& a, RtPlan& p) { return maf_bwd_rt_plan(dim, n_hidden, hidden, a, p); });
}

// the plan's kernel, its dynamic-LDS attribute set
static void (*maf_bwd_rt_kernel_of(const RtPlan&))(MafBwdRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, maf_bwd_rt_kernel<4>);
  return maf_bwd_rt_kernel<4>;
}

extern "C" int64_t mnf_maf_bwd_rt_det_workspace(int64_t rows, int dim, int n_hidden, const int* hidden) {
  return rt_det_workspace<MafBwdRtArgs>(
      rows, dim, [&](MafBwdRtArgs& a, RtPlan& p) { return maf_bwd_rt_plan(dim, n_hidden, hidden, a, p) ? a.n_params : 0; },
      maf_bwd_rt_kernel_of);
}

// det: fixed-order parameter sums through `workspace` (mnf_rt_host.h run_rt_bwd)
static int maf_bwd_rt_run(const float* x, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                          const float* flat, const uint8_t* masks, const float* grad_scale_dev, int64_t rows, int dim, int parity,
                          int n_hidden, const int* hidden, bool det, float* workspace, int64_t workspace_floats, void* stream) {
  if (!x || !grad_x || x == grad_x || !flat || !masks || !grad_scale_dev || rows < 0 || dim < 1 || n_hidden < 1 ||
      !hidden_ok(n_hidden, hidden) || (grad_y && grad_y == grad_x) || (grad_flat && grad_flat == flat))
    return MNF_ERR_INVALID_ARG;
  auto fill = [&](MafBwdRtArgs& a) {
    a.x = x; a.grad_y = grad_y; a.grad_ld = grad_ld; a.grad_x = grad_x; a.grad_flat = grad_flat; a.flat = flat; a.masks = masks;
    a.gscale_dev = grad_scale_dev; a.rows = rows; a.dim = dim; a.parity = parity != 0;
    a.vec = dim % 4 == 0 && aligned16(x, grad_x, grad_y);
  };
  return run_rt_bwd<MafBwdRtArgs>(
      {rows, dim, grad_flat, det, workspace, workspace_floats, "maf_bwd_rt", stream}, /*in_domain=*/true, /*unsupported=*/false,
      [&](MafBwdRtArgs& a, RtPlan& p) { return maf_bwd_rt_plan(dim, n_hidden, hidden, a, p) ? a.n_params : 0; }, fill,
      maf_bwd_rt_kernel_of);
}

extern "C" int mnf_maf_bwd_rt(const float* x, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                              const float* flat, const uint8_t* masks, const float* grad_scale_dev, int64_t rows, int dim,
                              int parity, int n_hidden, const int* hidden, void* stream) {
  return maf_bwd_rt_run(x, grad_y, grad_ld, grad_x, grad_flat, flat, masks, grad_scale_dev, rows, dim, parity, n_hidden, hidden,
                        false, nullptr, 0, stream);
}

extern "C" int mnf_maf_bwd_rt_det(const float* x, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                                  const float* flat, const uint8_t* masks, const float* grad_scale_dev, int64_t rows, int dim,
                                  int parity, int n_hidden, const int* hidden, float* workspace, int64_t workspace_floats,
                                  void* stream) {
  return maf_bwd_rt_run(x, grad_y, grad_ld, grad_x, grad_flat, flat, masks, grad_scale_dev, rows, dim, parity, n_hidden, hidden,
                        true, workspace, workspace_floats, stream);
}
