// Gradients of AffineHalfFlow.forward / .inverse (torch_mnf/flows/affine_half_flow.py:44-66 under loss.backward(); the
// reference trains through these layers: tests/test_flows.py:14-31) for ANY conditioner shape on the f16 matrix pipe:
// run-time layer count and widths (mnf_rt.h, mnf_rt_bwd.h), weights read from the plain `flat` parameter vector.  Takes
// the calls the per-shape gradient kernels (mnf_ahf_bwd_split.hip, mnf_ahf_bwd_mfma.hip: three hidden layers of at most
// 32 units) have no instantiation for: 1 .. 4 hidden layers of widths 4 .. 64, any even dim (MT_MAX = 4: four 16-unit tiles
// per hidden vector), and -- the *_wide entry points -- the same with the widest layer at 65 .. 128 units (MT_MAX = 8).
//
// A workgroup owns a block of 16 NW rows, a wave one tile of it.  Per net (s, then t): the forward recompute keeps every
// hidden vector (turned, in the LDS exchange area) and the row scales; the output layer is walked two 16-column tiles at
// a time -- s or t of the tiles, the cotangents g_s / g_t from grad_y, grad_ld (and y: the inverse direction's g_s = -g y
// - g_ld needs no second net), grad_x of the transformed half, the first step of the delta chain W_out^T g and the
// tiles' dW_out products --, then the hidden layers backwards (delta chain in registers, dW per layer through the
// exchange area), then grad_x of the conditioning half and dW of the first layer input tile by input tile.
//
// A RUN of n_layers layers of one shape (mnf_affine_half_bwd_rt_stack) is the same kernel with a layer loop outermost,
// applied layers n - 1 .. 0: one layer's weights are staged at a time and the workgroup sweeps ITS OWN row blocks once per
// layer.  Lane (j, q) of a wave loads the grad_y elements of row j at within-half columns 16 m + 4 q + r and stores grad_x
// at exactly those positions (gx1 at act_off, add_gx at cond_off), and the row block -> wave -> tile mapping is the same
// in every layer: the grad_x a lane stores for applied layer i is the grad_y the same lane loads for layer i - 1, so the
// hand-over through memory needs no grid-wide synchronisation.  NOT in place in one buffer: in the forward direction the
// t pass reads grad_y of the transformed half after pass 0 has stored grad_x there.  The cotangent alternates between
// the caller's `work` plane and grad_x itself (layers of even index write grad_x, so layer 0 -- processed last -- leaves
// the result there; what layer i + 2 left in the plane layer i writes has been consumed by layer i + 1, same lanes).
#include <hip/hip_runtime.h>

#include <cstring>

#include "mnf_rt_bwd.h"

namespace mnf {

struct AhfBwdRtArgs {
  const float* x;
  const float* y;  // the layer's output for the same x (inverse direction only)
  const float* grad_y;
  const float* grad_ld;
  float* grad_x;
  float* grad_flat;
  const float* flat;
  const float* gscale_dev;  // per applied layer: the power of two that brings its cotangents near 1
  int64_t rows;
  int dim, inverse, has_scale, has_shift;
  int n_params, vec;
  int cb, bt, block_words, bias_words;  // weight stream (mnf_rt.h Source<false>)
  int ht_tiles, dt_tiles, ct_tiles;     // exchange tiles: hidden vectors of one net | one layer's deltas | a chunk
  NetDesc s_net, t_net;
  int64_t slot_floats;  // 0; mnf_affine_half_bwd_rt_det: workgroup b adds into grad_flat + b * slot_floats (mnf_rt_host.h)
  // a run of layers (n_layers = 1, outs = work = NULL: the one layer above)
  const float* outs;  // (n_layers, rows, dim): every applied layer's output; layer i reads x or outs[i - 1], and y = outs[i]
  float* work;        // (rows, dim): the cotangent plane that alternates with grad_x
  uint32_t parity;    // bit l: MODEL layer l's parity
  int n_layers;
  int lp;             // grad_ld is d loss / d log p: the last applied layer's grad_y is -y grad_ld, formed at the loads
};

// what changes from layer to layer of a run (the by-value AhfBwdRtArgs stays constant: it lives in scalar registers)
struct AhfBwdRtLayer {
  const float* x;
  const float* y;
  const float* grad_y;
  float* grad_x;
  const float* flat;
  float* gflat;
  int parity, lp;
};

constexpr float kLog2eB = 1.4426950408889634f;

// Threads the wide instantiation is compiled for; its plan takes at most that many waves.  256 (shipped): one wave per
// SIMD, 302 registers, no spills, at most 64 rows per workgroup; 512: two waves per SIMD at 256 registers each, 44 of them
// spilled (180 bytes of scratch per lane), up to 128 rows.  Measured (tools/time_ahf_bwd_rt_wide.py --lib, profiles/r20/):
// 256 is 5-19 % faster at h_sizes = (128, 128, 128) with the builds timed in either order; the other shapes are level to
// within what the order of the two builds in a run moves them by.
#ifndef MNF_AHF_BWD_RT_WIDE_THREADS
#define MNF_AHF_BWD_RT_WIDE_THREADS 256
#endif
static_assert(MNF_AHF_BWD_RT_WIDE_THREADS == 512 || MNF_AHF_BWD_RT_WIDE_THREADS == 256, "8 or 4 waves");

template <int MT_MAX>
__global__ void __launch_bounds__(MT_MAX > 4 ? MNF_AHF_BWD_RT_WIDE_THREADS : 512) ahf_bwd_rt_kernel(AhfBwdRtArgs a) {
  using namespace rt;
  const bool VEC = a.vec != 0;  // (uniform) rows are 16-byte aligned: dwordx4 row accesses
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4, nw = blockDim.x >> 6;
  // LDS: [scratch 16][scales: sA 8, sC 8, sH (layers + 1) x 8][weights][bias][exchange: HT | DT | CT][meta: per wave sign bits]
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + kBwdHeadWords;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  const BwdLds lds = bwd_lds(rt_lds, bias + a.bias_words, a.ht_tiles, a.dt_tiles, a.ct_tiles);
  float* const sC = lds.sC;
  float* const sH = lds.sH;
  const Exchange& exH = lds.exH;
  const Exchange& exC = lds.exC;
  const f16x4& ident = lds.ident;

  Source<false> src{blocks, bias, a.cb, a.bt, 0, 0, 0, 1.f, 0};
  const int H = a.dim / 2;
  const int n_nets = (a.has_scale ? 1 : 0) + (a.has_shift ? 1 : 0);
  const int64_t n_blocks = (a.rows + 16 * nw - 1) / (16 * nw);
  const int64_t plane = a.rows * a.dim;

  // layers outermost, last applied first: one layer's weights staged at a time; the workgroup keeps its row blocks
#pragma unroll 1
  for (int i = a.n_layers - 1; i >= 0; --i) {
    const int l = a.inverse ? a.n_layers - 1 - i : i;  // model index
    AhfBwdRtLayer ly;
    ly.x = i == 0 ? a.x : a.outs + (i - 1) * plane;
    ly.y = a.outs ? a.outs + i * plane : a.y;
    ly.grad_y = i == a.n_layers - 1 ? a.grad_y : (i & 1) ? a.grad_x : a.work;
    ly.grad_x = (i & 1) ? a.work : a.grad_x;
    ly.flat = a.flat + (int64_t)l * a.n_params;
    ly.gflat = a.grad_flat ? a.grad_flat + blockIdx.x * a.slot_floats + (int64_t)l * a.n_params : nullptr;
    ly.parity = (a.parity >> l) & 1u;
    ly.lp = a.lp && i == a.n_layers - 1;
    const float gs = a.gscale_dev[i], inv_gs = 1.f / gs;  // one scale per applied layer (one layer: its one float)
    // Layer boundary: every wave's stores of the previous layer are behind this barrier (rows past the end read the last
    // row's addresses, which another wave of this workgroup writes), and so are its last reads of the exchange area and
    // the weight stream; block_weight_max's two barriers then keep this layer's staging behind them as well.
    if (i != a.n_layers - 1) __syncthreads();
    float wmx = net_weight_max(ly.flat, a.s_net, 0.f);  // (one net only: s_net and t_net are the same descriptor)
    if (a.has_scale && a.has_shift) wmx = net_weight_max(ly.flat, a.t_net, wmx);
    const float wmax = block_weight_max(wmx, scratch);
    const int we = weight_exponent(wmax);
    const float wup = pow2f(we);
    src.wdown = pow2f(-we);
    const int cond_off = ly.parity ? H : 0, act_off = ly.parity ? 0 : H;
    float* const gflat = ly.gflat;

    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
      const int64_t r = blk * (16 * nw) + 16 * wave + j;
      const bool live = r < a.rows;
      const int64_t rc = live ? r : a.rows - 1;
      const float* xrow = ly.x + rc * a.dim;
      const float* yrow = ly.y ? ly.y + rc * a.dim : xrow;
      const float* gyrow = ly.grad_y ? ly.grad_y + rc * a.dim : xrow;
      float* gxrow = ly.grad_x + rc * a.dim;
      const float gl = a.grad_ld && live ? a.grad_ld[rc] : 0.f;
      // grad_y of 4 columns of a half: the tensor, or (lp) -y d loss / d log p -- the product is kept a product (no
      // contraction into the sums it feeds), so that it has the bits of a materialised grad_y
      auto load_gy = [&](int off, int col) {
        if (ly.lp) {
          f32x4 v = load4(yrow + off, col, H, VEC);
#pragma unroll
          for (int e4 = 0; e4 < 4; ++e4) {
            float p = v[e4] * -gl;
            asm volatile("" : "+v"(p));
            v[e4] = p;
          }
          return v;
        }
        return ly.grad_y ? load4(gyrow + off, col, H, VEC) : f32x4{0.f, 0.f, 0.f, 0.f};
      };
      const float rowmask = live ? 1.f : 0.f;  // rows past the end add nothing to the parameter sums

#pragma unroll 1
      for (int pass = 0; pass < n_nets; ++pass) {
        const bool is_s = a.has_scale && pass == 0;
        const NetDesc& nd = is_s ? a.s_net : a.t_net;
        const int n_hid = nd.n_lin - 1, L = n_hid;
        // ---- forward recompute: every hidden vector goes, turned, into the exchange area; its sign bits into LDS
        Hidden<MT_MAX, 1> h;
        {
          auto load_x = [&](int, int ks, f32x4& xa, f32x4& xb) {
            const int c0 = 32 * ks + 4 * q;
            xa = load4(xrow + cond_off, c0, H, VEC);
            xb = load4(xrow + cond_off, c0 + 16, H, VEC);
          };
          forward_keep<MT_MAX>(src, ly.flat, nd, n_hid, -1, wup, lds, load_x, h);
        }
        // ---- output layer, two 16-column tiles (one K-step of the chain) per chunk
        const int MTh = tiles16(nd.sizes[L]), KSh = steps32(16 * MTh), M = tiles16(H);
        // (the t pass behind an s pass needs e^{-s} in the inverse direction only, and only as g e^{-s}: that is the
        //  value-half cotangent the s pass stored in grad_x -- read back by the lane that wrote it, program order)
        const bool after_s = !is_s && a.has_scale;
        const int ht_last = exH_tile_of(nd, L);
        Acc<MT_MAX, 1> accd;
        accd.zero();
        float downd = 1.f;  // the row's running scale of the chain's first product (as in net_to_hidden)
        for (int m0 = 0; m0 < M; m0 += 2) {
          const int mo = M - m0 < 2 ? M - m0 : 2;
          uint32_t* buf = src.cur_blocks();
          float* bbuf = src.cur_bias();
          stage_blocks(buf, mo * KSh, DenseMMajor{ly.flat + nd.w_off[L], nd.sizes[L], H, KSh, m0, 1, 0}, src.wdown);
          stage_bias(bbuf, mo, DenseBias{ly.flat + nd.b_off[L], H, m0});
          const uint32_t* bufT = buf + mo * KSh * kBlockWords;
          stage_blocks(const_cast<uint32_t*>(bufT), MTh, DenseTKMajor{ly.flat + nd.w_off[L], nd.sizes[L], H, MTh, m0 >> 1},
                       src.wdown);
          src.commit();
          f32x4 g2[2];
#pragma unroll
          for (int ml = 0; ml < 2; ++ml) {
            g2[ml] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ml < mo) {
              const int col = 16 * (m0 + ml) + 4 * q;
              f32x4 o[1], sv[1];
              out_tile<MT_MAX, 1>(buf, ml * KSh, KSh, bbuf + 16 * ml, lane, q, h, wup, o);
              sv[0] = is_s ? o[0] : f32x4{0.f, 0.f, 0.f, 0.f};
              const f32x4 x1 = load4(xrow + act_off, col, H, VEC);
              const f32x4 gy1 = load_gy(act_off, col);
              const f32x4 y1 = a.inverse && is_s ? load4(yrow + act_off, col, H, VEC) : f32x4{0.f, 0.f, 0.f, 0.f};
              const f32x4 gxs = a.inverse && after_s ? load4(gxrow + act_off, col, H, VEC) : f32x4{0.f, 0.f, 0.f, 0.f};
              f32x4 gx1;
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4) {
                // forward: y = e^s v + t      g_v = g e^s     g_s = g e^s v + g_ld     g_t = g
                // inverse: y = (v - t) e^-s   g_v = g e^-s    g_s = -g y - g_ld        g_t = -g e^-s
                const float ex = __builtin_amdgcn_exp2f((a.inverse ? -sv[0][e4] : sv[0][e4]) * kLog2eB);
                gx1[e4] = gy1[e4] * ex;
                float g;
                if (is_s) g = a.inverse ? -gy1[e4] * y1[e4] - gl : gy1[e4] * ex * x1[e4] + gl;
                else if (after_s) g = a.inverse ? -gxs[e4] : gy1[e4];
                else g = a.inverse ? -gy1[e4] * ex : gy1[e4];  // (no scale net: ex = 1)
                // (wide: a select -- 0 * NaN from a clamped read-back would poison a whole dW block; the narrow
                //  instantiation keeps the product it shipped with, bit for bit and instruction for instruction)
                if constexpr (MT_MAX > 4) g2[ml][e4] = col + e4 < H && live ? g * gs : 0.f;
                else g2[ml][e4] = col + e4 < H ? g * gs * rowmask : 0.f;
              }
              if (pass == 0) store4(gxrow + act_off, col, H, VEC, live, gx1);
            }
          }
          // the chain's first step: accd += W_out^T-blocks x [g tile 0 | g tile 1]
          {
            f16x8 bh[1], bl[1];
            float mx = 0.f;
            split_kstep(g2[0], g2[1], downd, bh[0], bl[0], mx);
            if (__builtin_expect(wave_any(!(mx < kSplitLimit)), 0)) {
              float fm = 0.f;
#pragma unroll
              for (int e4 = 0; e4 < 4; ++e4) fm = __builtin_fmaxf(fm, __builtin_fmaxf(finite_abs(g2[0][e4]), finite_abs(g2[1][e4])));
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
              split_kstep(g2[0], g2[1], downd, bh[0], bl[0], unused);
            }
            mac_kstep<MT_MAX, 1>(bufT, 0, MTh, lane, bh, bl, accd.main, accd.corr);
          }
          // dW_out, db_out of the two tiles: cotangents (times the hidden vector's row scale) x last hidden vector
          if (gflat) {
            f32x4 cv[MT_MAX];
#pragma unroll
            for (int m = 0; m < MT_MAX; ++m) cv[m] = m < 2 ? g2[m < 2 ? m : 0] : f32x4{0.f, 0.f, 0.f, 0.f};
            const float sc = exchange_store<MT_MAX>(cv, mo, exC, 0, 16 * wave, lane, ident);
            if (lane == 0) sC[wave] = sc;
            lds_barrier();
            dw_phase(exC, 0, mo, exH, ht_last, MTh, sC, sH + L * 8, nw, inv_gs, gflat + nd.w_off[L], gflat + nd.b_off[L], H,
                     nd.sizes[L], m0, 0);
          }
        }
        // ---- hidden layers backwards, then grad_x of the conditioning half and dW_0 (mnf_rt_bwd.h)
        f32x4 dv[MT_MAX];
        chain_result<MT_MAX>(accd, wup / downd, lds.meta_bits[n_hid * 64 + lane], dv);
        auto load_in = [&](int mi) { return load4(xrow + cond_off, 16 * mi + 4 * q, H, VEC); };
        auto add_gx = [&](int mi, const f32x4& g) {
          const int col = 16 * mi + 4 * q;
          const f32x4 base = pass == 0 ? load_gy(cond_off, col) : load4(gxrow + cond_off, col, H, VEC);
          store4(gxrow + cond_off, col, H, VEC, live, base + g);
        };
        backward_tail<MT_MAX>(src, ly.flat, gflat, nd, n_hid, -1, dv, lds, wup, inv_gs, H, load_in, add_gx);
      }
    }
  }
}

// The launch of a shape, or false: the VALU kernel takes it.  Fills the kernel arguments' shape part.  wide: the shapes
// whose widest hidden layer has 65 .. 128 units (the MT_MAX = 8 instantiation); else those up to 64 (MT_MAX = 4).
static bool ahf_bwd_rt_plan(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift, bool wide,
                            AhfBwdRtArgs& a, RtPlan& p) {
  if (dim < 2 || (dim & 1) || n_hidden < 1 || n_hidden > rt::kMaxBwdLayers || !hidden_ok(n_hidden, hidden) ||
      (!has_scale && !has_shift))
    return false;
  const int H = dim / 2;
  int sizes[MNF_MAX_LINEAR + 1];
  sizes[0] = H;
  const HiddenWidths w = scan_hidden(n_hidden, hidden, sizes);
  sizes[n_hidden + 1] = H;
  if (w.min < 4 || w.max > (wide ? 128 : 64) || (wide && w.max <= 64)) return false;
  const int64_t n_params = ahf_layout(n_hidden, sizes, has_scale, has_shift, a);
  if (!n_params) return false;
  a.n_params = (int)n_params;
  p.mt_max = wide ? 8 : 4;
  a.bt = 8;  // (a layer's bias tiles: at most 8 at 128 units)
  a.ht_tiles = w.tiles;
  a.dt_tiles = 0;  // (the deltas reuse the hidden vectors' tiles: mnf_rt_bwd.h backward_tail)
  const int KS1 = (16 * ((hidden[0] + 15) / 16) + 31) / 32;
  // The LDS plan.  Rows per workgroup first (16 per wave, any wave count: the per-row-block cost is what this kernel is
  // bound by), then the roomier of two weight-stream sizes (12 blocks per buffer: fewer chunks; 8: the largest chunk
  // there is -- two output tiles' forward blocks and the transposed blocks of their K-step at 64 hidden units), then as
  // many first-layer input tiles per chunk as fit (the output-layer chunks need two).  Wide: that largest chunk is 2 x 4 +
  // 8 = 16 blocks at 128 hidden units (and a K-step of a 128-unit layer 8), so 24 or 16 blocks per buffer; four layers
  // of 128 units are 32 exchange tiles, which leave room for 32 rows (nw = 2) beside the 64 KB of weight stream.
  const int cb_lo = wide ? 16 : 8, cb_step = wide ? 8 : 4;
  return rt::fit_bwd_lds(a, a, p, {/*nw_max=*/wide ? MNF_AHF_BWD_RT_WIDE_THREADS / 64 : 8, cb_lo + cb_step, cb_lo, cb_step, KS1,
                                   /*ct_min=*/2, /*ct_max=*/p.mt_max});
}

// the plan with the shape bound; a slot holds the parameters of all n_layers layers (the frame: mnf_rt_host.h)
struct ahf_bwd_rt_slots {
  int dim, n_hidden;
  const int* hidden;
  int has_scale, has_shift;
  bool wide;
  int n_layers;
  int64_t operator()(AhfBwdRtArgs& a, RtPlan& p) const {
    if (n_layers < 1 || n_layers > 32 || !ahf_bwd_rt_plan(dim, n_hidden, hidden, has_scale, has_shift, wide, a, p)) return 0;
    return (int64_t)n_layers * a.n_params;
  }
};

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_affine_half_bwd_rt_supported(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift) {
  return rt_has_plan<AhfBwdRtArgs>(ahf_bwd_rt_slots{dim, n_hidden, hidden, has_scale, has_shift, false, 1});
}

// ... and the shapes of the wide instantiation: 1 exactly where the widest hidden layer has 65 .. 128 units and a plan
// exists -- never where the query above answers 1
extern "C" int mnf_affine_half_bwd_rt_wide_supported(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift) {
  return rt_has_plan<AhfBwdRtArgs>(ahf_bwd_rt_slots{dim, n_hidden, hidden, has_scale, has_shift, true, 1});
}

// Which runs go out as one launch: 1 .. 32 layers of a shape the kernel has (every shape class of the plan: the layer
// loop adds one weight-maximum pass and three barriers per layer to what n launches do, and takes n - 1 launches away).
extern "C" int mnf_affine_half_bwd_rt_stack_supported(int dim, int n_hidden, const int* hidden, int has_scale, int has_shift,
                                                      int n_layers) {
  return rt_has_plan<AhfBwdRtArgs>(ahf_bwd_rt_slots{dim, n_hidden, hidden, has_scale, has_shift, false, n_layers});
}

extern "C" int mnf_affine_half_bwd_rt_wide_stack_supported(int dim, int n_hidden, const int* hidden, int has_scale,
                                                           int has_shift, int n_layers) {
  return rt_has_plan<AhfBwdRtArgs>(ahf_bwd_rt_slots{dim, n_hidden, hidden, has_scale, has_shift, true, n_layers});
}

// the plan's kernel, its dynamic-LDS attribute set
static void (*ahf_bwd_rt_kernel_of(const RtPlan& p))(AhfBwdRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, ahf_bwd_rt_kernel<4>, ahf_bwd_rt_kernel<8>);
  return p.mt_max == 4 ? ahf_bwd_rt_kernel<4> : ahf_bwd_rt_kernel<8>;
}

static int64_t ahf_bwd_rt_workspace(int64_t rows, int dim, int n_hidden, const int* hidden, int has_scale, int has_shift,
                                    int n_layers, bool wide) {
  return rt_det_workspace<AhfBwdRtArgs>(rows, dim, ahf_bwd_rt_slots{dim, n_hidden, hidden, has_scale, has_shift, wide, n_layers},
                                        ahf_bwd_rt_kernel_of);
}

extern "C" int64_t mnf_affine_half_bwd_rt_det_workspace(int64_t rows, int dim, int n_hidden, const int* hidden, int has_scale,
                                                        int has_shift) {
  return ahf_bwd_rt_workspace(rows, dim, n_hidden, hidden, has_scale, has_shift, 1, false);
}

extern "C" int64_t mnf_affine_half_bwd_rt_wide_det_workspace(int64_t rows, int dim, int n_hidden, const int* hidden,
                                                             int has_scale, int has_shift) {
  return ahf_bwd_rt_workspace(rows, dim, n_hidden, hidden, has_scale, has_shift, 1, true);
}

extern "C" int64_t mnf_affine_half_bwd_rt_stack_det_workspace(int64_t rows, int dim, int n_hidden, const int* hidden,
                                                              int has_scale, int has_shift, int n_layers) {
  return ahf_bwd_rt_workspace(rows, dim, n_hidden, hidden, has_scale, has_shift, n_layers, false);
}

extern "C" int64_t mnf_affine_half_bwd_rt_wide_stack_det_workspace(int64_t rows, int dim, int n_hidden, const int* hidden,
                                                                   int has_scale, int has_shift, int n_layers) {
  return ahf_bwd_rt_workspace(rows, dim, n_hidden, hidden, has_scale, has_shift, n_layers, true);
}

// One layer (outs = work = NULL, n_layers = 1, y its output) or a run (y = NULL); lp: grad_ld is d loss / d log p.
// det: fixed-order parameter sums through `workspace` (mnf_rt_host.h run_rt_bwd); wide: the *_wide entries' shapes
static int ahf_bwd_rt_run(const float* x, const float* y, const float* outs, const float* grad_y, const float* grad_ld, int lp,
                          float* grad_x, float* work, float* grad_flat, const float* flat, const float* grad_scale_dev,
                          uint32_t parity_bits, int n_layers, int64_t rows, int dim, int inverse, int n_hidden,
                          const int* hidden, int has_scale, int has_shift, bool wide, bool det, float* workspace,
                          int64_t workspace_floats, void* stream) {
  if (!x || !grad_x || !flat || !grad_scale_dev || rows < 0 || dim < 2 || (dim & 1) || !hidden_ok(n_hidden, hidden))
    return MNF_ERR_INVALID_ARG;
  auto fill = [&](AhfBwdRtArgs& a) {
    a.x = x; a.y = y; a.grad_y = grad_y; a.grad_ld = grad_ld; a.grad_x = grad_x; a.grad_flat = grad_flat; a.flat = flat;
    a.gscale_dev = grad_scale_dev; a.rows = rows; a.dim = dim; a.parity = parity_bits; a.inverse = inverse != 0;
    a.has_scale = has_scale != 0; a.has_shift = has_shift != 0;
    a.outs = outs; a.work = work; a.n_layers = n_layers; a.lp = lp;
    // (the planes of outs are rows * dim floats apart: dim % 8 == 0 keeps them aligned with the base)
    a.vec = dim % 8 == 0 && aligned16(x, grad_x, y, grad_y, outs, work);
  };
  // (the inverse's scale gradient needs the layer's output; a run's planes stay below 2^42 elements)
  const bool unsupported = (inverse && has_scale && !y && !outs) || rows * dim * n_layers >= (1ll << 42);
  return run_rt_bwd<AhfBwdRtArgs>(
      {rows, dim, grad_flat, det, workspace, workspace_floats, n_layers > 1 ? "ahf_bwd_stack_rt" : "ahf_bwd_rt", stream},
      /*in_domain=*/true, unsupported, ahf_bwd_rt_slots{dim, n_hidden, hidden, has_scale, has_shift, wide, n_layers}, fill,
      ahf_bwd_rt_kernel_of);
}

extern "C" int mnf_affine_half_bwd_rt(const float* x, const float* y, const float* grad_y, const float* grad_ld, float* grad_x,
                                      float* grad_flat, const float* flat, const float* grad_scale_dev, int64_t rows, int dim,
                                      int parity, int inverse, int n_hidden, const int* hidden, int has_scale, int has_shift,
                                      void* stream) {
  return ahf_bwd_rt_run(x, y, nullptr, grad_y, grad_ld, 0, grad_x, nullptr, grad_flat, flat, grad_scale_dev, parity ? 1u : 0u,
                        1, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, false, false, nullptr, 0, stream);
}

extern "C" int mnf_affine_half_bwd_rt_wide(const float* x, const float* y, const float* grad_y, const float* grad_ld,
                                           float* grad_x, float* grad_flat, const float* flat, const float* grad_scale_dev,
                                           int64_t rows, int dim, int parity, int inverse, int n_hidden, const int* hidden,
                                           int has_scale, int has_shift, void* stream) {
  return ahf_bwd_rt_run(x, y, nullptr, grad_y, grad_ld, 0, grad_x, nullptr, grad_flat, flat, grad_scale_dev, parity ? 1u : 0u,
                        1, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, true, false, nullptr, 0, stream);
}

extern "C" int mnf_affine_half_bwd_rt_det(const float* x, const float* y, const float* grad_y, const float* grad_ld,
                                          float* grad_x, float* grad_flat, const float* flat, const float* grad_scale_dev,
                                          int64_t rows, int dim, int parity, int inverse, int n_hidden, const int* hidden,
                                          int has_scale, int has_shift, float* workspace, int64_t workspace_floats,
                                          void* stream) {
  return ahf_bwd_rt_run(x, y, nullptr, grad_y, grad_ld, 0, grad_x, nullptr, grad_flat, flat, grad_scale_dev, parity ? 1u : 0u,
                        1, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, false, true, workspace, workspace_floats,
                        stream);
}

extern "C" int mnf_affine_half_bwd_rt_wide_det(const float* x, const float* y, const float* grad_y, const float* grad_ld,
                                               float* grad_x, float* grad_flat, const float* flat, const float* grad_scale_dev,
                                               int64_t rows, int dim, int parity, int inverse, int n_hidden,
                                               const int* hidden, int has_scale, int has_shift, float* workspace,
                                               int64_t workspace_floats, void* stream) {
  return ahf_bwd_rt_run(x, y, nullptr, grad_y, grad_ld, 0, grad_x, nullptr, grad_flat, flat, grad_scale_dev, parity ? 1u : 0u,
                        1, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, true, true, workspace, workspace_floats,
                        stream);
}

// the run's own argument checks (before any launch), then ahf_bwd_rt_run
static int ahf_bwd_rt_stack(const float* x, const float* outs, const float* grad_y_last, const float* lp_grad,
                            const float* grad_ld, float* grad_x, float* grad_work, float* grad_flats, const float* flats,
                            const float* grad_scale_dev, const int* parity_host, int n_layers, int64_t rows, int dim,
                            int inverse, int n_hidden, const int* hidden, int has_scale, int has_shift, bool wide, bool det,
                            float* workspace, int64_t workspace_floats, void* stream) {
  if (!x || !outs || !grad_x || !flats || !grad_scale_dev || !parity_host || n_layers < 1 || n_layers > 32 || rows < 0 ||
      (lp_grad && (grad_y_last || grad_ld)) || (n_layers > 1 && !grad_work) || grad_work == grad_x || x == outs ||
      (!has_scale && !has_shift) ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(outs) | reinterpret_cast<uintptr_t>(grad_y_last) |
        reinterpret_cast<uintptr_t>(lp_grad) | reinterpret_cast<uintptr_t>(grad_ld) | reinterpret_cast<uintptr_t>(grad_x) |
        reinterpret_cast<uintptr_t>(grad_work) | reinterpret_cast<uintptr_t>(grad_flats) | reinterpret_cast<uintptr_t>(flats)) & 3))
    return MNF_ERR_INVALID_ARG;
  uint32_t bits = 0;
  for (int l = 0; l < n_layers; ++l) bits |= (parity_host[l] ? 1u : 0u) << l;
  return ahf_bwd_rt_run(x, nullptr, outs, grad_y_last, lp_grad ? lp_grad : grad_ld, lp_grad ? 1 : 0, grad_x,
                        n_layers > 1 ? grad_work : nullptr, grad_flats, flats, grad_scale_dev, bits, n_layers, rows, dim,
                        inverse, n_hidden, hidden, has_scale, has_shift, wide, det, workspace, workspace_floats, stream);
}

extern "C" int mnf_affine_half_bwd_rt_stack(const float* x, const float* outs, const float* grad_y_last, const float* lp_grad,
                                            const float* grad_ld, float* grad_x, float* grad_work, float* grad_flats,
                                            const float* flats, const float* grad_scale_dev, const int* parity_host,
                                            int n_layers, int64_t rows, int dim, int inverse, int n_hidden, const int* hidden,
                                            int has_scale, int has_shift, void* stream) {
  return ahf_bwd_rt_stack(x, outs, grad_y_last, lp_grad, grad_ld, grad_x, grad_work, grad_flats, flats, grad_scale_dev,
                          parity_host, n_layers, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, false, false,
                          nullptr, 0, stream);
}

extern "C" int mnf_affine_half_bwd_rt_wide_stack(const float* x, const float* outs, const float* grad_y_last,
                                                 const float* lp_grad, const float* grad_ld, float* grad_x, float* grad_work,
                                                 float* grad_flats, const float* flats, const float* grad_scale_dev,
                                                 const int* parity_host, int n_layers, int64_t rows, int dim, int inverse,
                                                 int n_hidden, const int* hidden, int has_scale, int has_shift, void* stream) {
  return ahf_bwd_rt_stack(x, outs, grad_y_last, lp_grad, grad_ld, grad_x, grad_work, grad_flats, flats, grad_scale_dev,
                          parity_host, n_layers, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, true, false,
                          nullptr, 0, stream);
}

extern "C" int mnf_affine_half_bwd_rt_stack_det(const float* x, const float* outs, const float* grad_y_last,
                                                const float* lp_grad, const float* grad_ld, float* grad_x, float* grad_work,
                                                float* grad_flats, const float* flats, const float* grad_scale_dev,
                                                const int* parity_host, int n_layers, int64_t rows, int dim, int inverse,
                                                int n_hidden, const int* hidden, int has_scale, int has_shift,
                                                float* workspace, int64_t workspace_floats, void* stream) {
  return ahf_bwd_rt_stack(x, outs, grad_y_last, lp_grad, grad_ld, grad_x, grad_work, grad_flats, flats, grad_scale_dev,
                          parity_host, n_layers, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, false, true,
                          workspace, workspace_floats, stream);
}

extern "C" int mnf_affine_half_bwd_rt_wide_stack_det(const float* x, const float* outs, const float* grad_y_last,
                                                     const float* lp_grad, const float* grad_ld, float* grad_x,
                                                     float* grad_work, float* grad_flats, const float* flats,
                                                     const float* grad_scale_dev, const int* parity_host, int n_layers,
                                                     int64_t rows, int dim, int inverse, int n_hidden, const int* hidden,
                                                     int has_scale, int has_shift, float* workspace, int64_t workspace_floats,
                                                     void* stream) {
  return ahf_bwd_rt_stack(x, outs, grad_y_last, lp_grad, grad_ld, grad_x, grad_work, grad_flats, flats, grad_scale_dev,
                          parity_host, n_layers, rows, dim, inverse, n_hidden, hidden, has_scale, has_shift, true, true,
                          workspace, workspace_floats, stream);
}
