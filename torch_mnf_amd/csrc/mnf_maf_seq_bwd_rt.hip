// Gradients of the element-by-element direction of MAF / IAF (MAF.forward, IAF.inverse: torch_mnf/flows/maf.py:39-51 under
// loss.backward()) for MADE nets of 1 .. 4 hidden layers of widths 4 .. 64 on the f16 matrix pipe, for masks that are
// autoregressive in index order (what mnf_maf_bwd asks for too).  DESIGN.md 3.8g: the reverse pass has two parts.
//
//   1. maf_seq_bwd_rt_kernel (this file): the triangular solve for the total cotangents G.  The activations at the decoded
//      output y serve every step, so the net is evaluated ONCE per 16-row tile (only its ReLU sign bits and e^{-s} are
//      kept); then for i = dim-1 .. 0, with G_i final,
//        c_s = -(G_i y_i) - grad_ld     c_t = -G_i e^{-s_i}     grad_z[i'] = G_i e^{-s_i}  (i' = dim-1-i when parity)
//      and the one-hot pair (c_s at output i, c_t at output dim + i) goes back through the masked net: the last
//      MaskedLinear as two fp32 rows on the VALU, the hidden layers and the first layer as split MFMA products against
//      TRANSPOSED blocks, the input cotangent added to G_j, j < i.  No parameter sums.
//   2. The parameter gradients are those of the ONE-PASS direction at x := y with grad_y := C, C_i = -G_i e^{-s_i},
//      grad_ld := -grad_ld, parity := 0: a launch of mnf_maf_bwd_rt (mnf_maf_bwd_rt_det: fixed-order sums), untouched.
//
// Like maf_seq_rt (mnf_maf_rt.hip) the solve stages everything once per workgroup and its waves never meet again: a wave
// owns a 16-row tile, G and e^{-s} live in two per-wave LDS slabs, float4 (column group g, row j) at slab[16 g + j].  All
// four lanes (j, q) of a row read G_i; lane (j, q) adds to the groups 4 m + q it holds in the accumulator layout.  The
// wave's LDS accesses are in program order, so no barrier sits inside the dim loop.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mnf_hip.h"
#include "mnf_rnvp_common.h"
#include "mnf_rt_bwd.h"

namespace mnf {

constexpr int kSeqBwdClass = 4;      // hidden tiles of a vector: widths up to 64 (mnf_maf_bwd_rt's class)
constexpr int kSeqBwdHeadWords = 32;  // scratch 16 | a bias tile of zeros 16

// One run of A blocks of a MaskedLinear W (n_out x n_in, the byte of W[o][k] at M[k * ldm + o]): block (A, B) holds rows
// a = 16 A + i against K indices b = 32 B + ...; forward: (o, k) = (a, b), turned: (o, k) = (b, a) -- the transposed matrix.
// Block index = d0 + R0 * d1 with (d0, d1) = (A, B) when a_first, else (B, A).
struct SeqBwdSeg {
  int w_off, m_off, n_in, n_out, ldm, turned, R0, a_first, n_blocks, dst;
};

struct MafSeqBwdArgs {
  const float* y;
  const float* grad_y;
  const float* grad_ld;
  float* grad_x;
  float* cot;
  float* neg_ld;
  const float* flat;
  const uint8_t* masks;
  const float* gscale_dev;
  int64_t rows;
  int dim, parity, vec;
  int s_w, s_b;                 // float offsets of the last MaskedLinear (s = its first dim rows, t = the next dim)
  int fwd_blocks, bias_tiles;   // the forward image: layers 0 .. n-1 and the s head of the last one
  int n_seg;
  SeqBwdSeg seg[2 * rt::kMaxBwdLayers + 1];  // what the workgroup stages as split-f16 blocks
  int t_off[MNF_MAX_LINEAR];    // first turned block of layer l (behind the forward image)
  int turned_blocks;
  int hp;                       // padded width of the last hidden vector: the row pitch of the fp32 last-layer rows
  int m_off[MNF_MAX_LINEAR];    // byte offset of layer l's mask
  NetDesc net;                  // dim -> h_1 .. h_n
};

// The workgroup's images: every segment's blocks dealt out over the waves, one block per trip (masked by a select, scaled by
// wdown, element-by-element loads at clamped indices: once per workgroup), and the forward layers' bias tiles as plain fp32.
__device__ __forceinline__ void maf_seq_bwd_stage(const MafSeqBwdArgs& a, uint32_t* blocks, float* bias, float wdown) {
  using namespace rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, i = lane & 15, q = lane >> 4;
#pragma unroll 1
  for (int s = 0; s < a.n_seg; ++s) {
    const SeqBwdSeg& g = a.seg[s];
    const float* W = a.flat + g.w_off;
    const uint8_t* Mk = a.masks + g.m_off;
#pragma unroll 1
    for (int b = wave; b < g.n_blocks; b += nw) {
      const int d1 = b / g.R0, d0 = b - d1 * g.R0;
      const int aa = 16 * (g.a_first ? d0 : d1) + i, b0 = 32 * (g.a_first ? d1 : d0) + 4 * q;
      f32x4 va, vb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int bb = b0 + (e & 3) + (e >> 2) * 16;
        const int o = g.turned ? bb : aa, k = g.turned ? aa : bb;
        const bool ok = o < g.n_out && k < g.n_in;
        const float w = W[ok ? (int64_t)o * g.n_in + k : 0];
        const uint8_t mb = Mk[ok ? (int64_t)k * g.ldm + o : 0];
        const float v = ok && mb ? w : 0.f;
        if (e < 4) va[e & 3] = v;
        else vb[e & 3] = v;
      }
      convert_block(blocks + (size_t)(g.dst + b) * kBlockWords, lane, va, vb, wdown);
    }
  }
  const NetDesc& nd = a.net;
  for (int u = threadIdx.x; u < a.bias_tiles * 16; u += blockDim.x) {
    int t = u >> 4, n_out = a.dim, off = a.s_b;  // (past the hidden layers: the s head)
    bool found = false;
    for (int l = 0; l < nd.n_lin; ++l) {
      const int nt = tiles16(nd.sizes[l + 1]);
      if (!found && t < nt) {
        found = true;
        n_out = nd.sizes[l + 1];
        off = nd.b_off[l];
      }
      t -= found ? 0 : nt;
    }
    const int o = 16 * t + (u & 15);
    const float v = a.flat[off + (o < n_out ? o : 0)];
    bias[u] = o < n_out ? v : 0.f;
  }
}

// One 16-row tile per wave.
__device__ __forceinline__ void maf_seq_bwd_block(const MafSeqBwdArgs& a, rt::Source<true>& src, float wup, float gs, int64_t row0,
                                                  const float* zero16, const float* lastW, float* slabG, float* slabE) {
  using namespace rt;
  constexpr int MT_MAX = kSeqBwdClass;
  const bool VEC = a.vec != 0;  // (uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int d = a.dim;
  const NetDesc& nd = a.net;
  const int n_hid = nd.n_lin;
  const MaskedLayers layers{a.masks, a.m_off, nd.sizes};
  const int hl = nd.sizes[n_hid], MTh = tiles16(hl), KS = steps32(16 * MTh), M = tiles16(d);
  const int MT1 = tiles16(nd.sizes[1]), KS1 = steps32(16 * MT1);
  const uint8_t* M0 = a.masks + a.m_off[n_hid];
  // the s head of the last MaskedLinear, every output tile: blocks [tile][K-step] (staged by maf_seq_bwd_stage)
  const MaskedMMajor s_fetch{a.flat + a.s_w, hl, d, KS, 0, 1, 0, M0, 2 * d, 0};
  const DenseBias s_bias{a.flat + a.s_b, d, 0};
  auto use_x = [&](int, int, const f32x4&, const f32x4&) {};
  Hidden<MT_MAX, 1> h;
  src.slot = 0;
  src.btile = 0;
  const int64_t r = row0 + (int64_t)wave * 16 + j;
  const bool live = r < a.rows;
  const int64_t rc = live ? r : a.rows - 1;
  const float* yrow = a.y + rc * d;
  const float* gyrow = a.grad_y ? a.grad_y + rc * d : yrow;
  float* gxrow = a.grad_x + rc * d;
  float* crow = a.cot + rc * d;
  const float gl = a.grad_ld ? a.grad_ld[rc] : 0.f;
  if (a.neg_ld && live && q == 0) a.neg_ld[r] = -gl;
  const float gls = gl * gs, inv_gs = 1.f / gs;
  f32x4* tileG = reinterpret_cast<f32x4*>(slabG) + j;  // group g of this lane's row at tile[16 g]
  f32x4* tileE = reinterpret_cast<f32x4*>(slabE) + j;

  // ---- the one evaluation of the net, on y: the ReLU sign bits of every hidden vector (16 per vector), e^{-s}, G := grad_y.
  // The y tile goes through the G slab (lane (j, q) writes and reads its own groups 4 m + q), as in maf_seq_rt.
  uint64_t bits = 0;
  {
#pragma unroll 1
    for (int m = 0; m < M; ++m) tileG[16 * (4 * m + q)] = load4(yrow, 16 * m + 4 * q, d, VEC);
    auto load_x = [&](int, int ks, f32x4& xa, f32x4& xb) {
      const int ga = 8 * ks + q, gb = ga + 4;
      const f32x4 va = tileG[16 * (ga < 4 * M ? ga : 0)], vb = tileG[16 * (gb < 4 * M ? gb : 0)];
      xa = ga < 4 * M ? va : f32x4{0.f, 0.f, 0.f, 0.f};
      xb = gb < 4 * M ? vb : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto hook = [&](int i, const Hidden<MT_MAX, 1>& hh) { bits |= (uint64_t)pack_signs<MT_MAX>(hh) << (16 * (i - 1)); };
    net_to_hidden<MT_MAX, 1, false>(src, a.flat, nd, n_hid, -1, wup, lane, q, load_x, use_x, h, hook, layers);
    const Chunk c = src.template chunk<false>(M * KS, s_fetch, M, s_bias);
#pragma unroll 1
    for (int m = 0; m < M; ++m) {
      f32x4 s4[1], es;
      out_tile<MT_MAX, 1>(c.A, m * KS, KS, c.bias + m * 16, lane, q, h, wup, s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) es[e] = exp6r(-s4[0][e]);
      f32x4 g = load4(gyrow, 16 * m + 4 * q, d, VEC) * gs;
      if (!a.grad_y) g = f32x4{0.f, 0.f, 0.f, 0.f};  // (uniform)
      tileE[16 * (4 * m + q)] = es;
      tileG[16 * (4 * m + q)] = g;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's slab writes, before its other lanes read them

  // ---- i = d-1 .. 0
  f32x4 ogx = f32x4{0.f, 0.f, 0.f, 0.f}, oc = ogx;
  float yn = yrow[d - 1];  // y_i, requested one step ahead
  const uint32_t* buf0 = src.blocks + a.t_off[0] * kBlockWords;
  for (int i = d - 1; i >= 0; --i) {
    const int e = i & 3;
    const float yi = yn;
    yn = yrow[i > 0 ? i - 1 : 0];
    const int slot = (16 * (i >> 2) + j) * 4 + e;
    const float G = slabG[slot], es = slabE[slot];
    const float ge = G * es;
    const float c_s = -(G * yi) - gls, c_t = -ge;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      ogx[c4] = c4 == e ? ge * inv_gs : ogx[c4];
      oc[c4] = c4 == e ? c_t * inv_gs : oc[c4];
    }
    if (e == 0 && live && q == ((i & 15) >> 2)) {
      // the group's four columns i .. i + 3 are final: one lane of the row's four stores them; grad_x flipped when parity
      if (VEC) {
        *reinterpret_cast<f32x4*>(crow + i) = oc;
        *reinterpret_cast<f32x4*>(gxrow + (a.parity ? d - 4 - i : i)) = a.parity ? f32x4{ogx[3], ogx[2], ogx[1], ogx[0]} : ogx;
      } else {
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4)
          if (i + c4 < d) {
            crow[i + c4] = oc[c4];
            gxrow[a.parity ? d - 1 - i - c4 : i + c4] = ogx[c4];
          }
      }
    }
    if (i == 0) break;  // nothing left to add to
    // delta_n = (c_s W_s[i, :] + c_t W_t[i, :]) * relu'(H_n)
    f32x4 dv[MT_MAX];
    const float* ws = lastW + (size_t)i * a.hp + 4 * q;
    const float* wt = lastW + (size_t)(d + i) * a.hp + 4 * q;
    const uint32_t bn = (uint32_t)(bits >> (16 * (n_hid - 1)));
#pragma unroll
    for (int m = 0; m < MT_MAX; ++m) {
      dv[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < MTh) {
        const f32x4 vs = *reinterpret_cast<const f32x4*>(ws + 16 * m), vt = *reinterpret_cast<const f32x4*>(wt + 16 * m);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) dv[m][rr] = (bn >> (4 * m + rr)) & 1u ? __builtin_fmaf(c_s, vs[rr], c_t * vt[rr]) : 0.f;
      }
    }
    // l = n-1 .. 1, the hidden layers backwards: delta_l = (W_l^T delta_{l+1}) * relu'(H_l); l = 0, the first layer:
    // G_j += (W_0^T delta_1)_j for the input tiles that hold a column j < i
    const int mi_end = (i + 15) >> 4;
#pragma unroll 1
    for (int l = n_hid - 1; l >= 0; --l) {
      Hidden<MT_MAX, 1> hd;
      split_rows_both<MT_MAX>(dv, hd);
      if (l == 0) {  // (uniform)
#pragma unroll 1
        for (int mi = 0; mi < mi_end; ++mi) {
          f32x4 gx[1];
          out_tile<MT_MAX, 1>(buf0, mi * KS1, KS1, zero16, lane, q, hd, wup, gx);
          f32x4* p = tileG + 16 * (4 * mi + q);
          *p = *p + gx[0];
        }
        break;
      }
      const int MTp = tiles16(nd.sizes[l]), KSl = steps32(16 * tiles16(nd.sizes[l + 1]));
      Acc<MT_MAX, 1> acc;
      acc.zero();
      const uint32_t* bufT = src.blocks + a.t_off[l] * kBlockWords;
#pragma unroll
      for (int ks = 0; ks < MT_MAX / 2; ++ks)
        if (ks < KSl) {
          f16x8 bh[1], bl[1];
          hidden_operand<MT_MAX, 1>(hd, ks, bh, bl);
          mac_kstep<MT_MAX, 1>(bufT, ks * MTp, MTp, lane, bh, bl, acc.main, acc.corr);
        }
      chain_result<MT_MAX, true>(acc, wup * hd.up[0], (uint32_t)(bits >> (16 * (l - 1))), dv);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

__global__ void __launch_bounds__(512) maf_seq_bwd_rt_kernel(MafSeqBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  float* scratch = reinterpret_cast<float*>(rt_lds);
  float* zero16 = scratch + 16;
  uint32_t* blocks = rt_lds + kSeqBwdHeadWords;
  float* bias = reinterpret_cast<float*>(blocks + (size_t)(a.fwd_blocks + a.turned_blocks) * rt::kBlockWords);
  float* lastW = bias + a.bias_tiles * 16;
  const int d = a.dim, n_hid = a.net.n_lin, hl = a.net.sizes[n_hid];
  const int slab_floats = 256 * ((d + 15) >> 4);  // 16 rows x the columns padded to whole 16-column tiles
  float* slabG = lastW + (size_t)2 * d * a.hp + (size_t)(threadIdx.x >> 6) * 2 * slab_floats;
  float* slabE = slabG + slab_floats;
  const uint8_t* M0 = a.masks + a.m_off[n_hid];
  float wmx = rt::net_weight_max(a.flat, a.net, a.masks, a.m_off, 0.f);
  wmx = rt::masked_abs_max(a.flat + a.s_w, M0, hl, 2 * d, wmx);
  const float wmax = rt::block_weight_max(wmx, scratch);
  const int e = rt::weight_exponent(wmax);
  const float wup = rt::pow2f(e);
  rt::Source<true> src{blocks, bias, 0, 0, 0, 0, 0, rt::pow2f(-e), 0};
  const float gs = *a.gscale_dev;
  if (threadIdx.x < 16) zero16[threadIdx.x] = 0.f;
  // the last MaskedLinear under its mask as plain fp32 rows of pitch hp (row o: s_o for o < d, t_{o-d} beyond), zero padded
  for (int idx = threadIdx.x; idx < 2 * d * a.hp; idx += blockDim.x) {
    const int o = idx / a.hp, k = idx - o * a.hp;
    const bool ok = k < hl;
    const float w = a.flat[a.s_w + (ok ? (int64_t)o * hl + k : 0)];
    const uint8_t mb = M0[ok ? (int64_t)k * 2 * d + o : 0];
    lastW[idx] = ok && mb ? w : 0.f;
  }
  maf_seq_bwd_stage(a, blocks, bias, src.wdown);
  __syncthreads();
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x)
    maf_seq_bwd_block(a, src, wup, gs, b * rows_per_block, zero16, lastW, slabG, slabE);
}

// The launch of a shape, or false: mnf_maf_bwd takes it.  Fills the kernel arguments' shape part.  mnf_maf_bwd_rt's shapes
// whose images fit 160 KB of LDS next to the slabs of 8 / 4 / 2 / 1 waves.
static bool maf_seq_bwd_rt_plan(int dim, int n_hidden, const int* hidden, MafSeqBwdArgs& a, RtPlan& p) {
  // The envelope is the weight pass's own -- mnf_maf_bwd_rt's: its query checks dim, the layer count, the widths (4 .. 64,
  // kSeqBwdClass tiles) and the layout's 31-bit guards, so nothing here repeats them
  static_assert(kSeqBwdClass == 4, "mnf_maf_bwd_rt's size class");
  if (!mnf_maf_bwd_rt_supported(dim, n_hidden, hidden)) return false;
  int sizes[MNF_MAX_LINEAR + 1];
  sizes[0] = dim;
  scan_hidden(n_hidden, hidden, sizes);
  maf_layout(dim, n_hidden, sizes, a);
  const int hl = hidden[n_hidden - 1];
  auto t16 = [](int n) { return (n + 15) / 16; };
  auto s32 = [](int n) { return (n + 31) / 32; };
  const int M = t16(dim), MTh = t16(hl);
  const StagedTiles net = mlp_tiles(sizes, n_hidden, dim);
  const int64_t fwd = net.blocks + (int64_t)M * s32(16 * MTh), tiles = net.bias + M;
  a.t_off[0] = (int)fwd;
  int64_t turned = (int64_t)M * s32(16 * t16(sizes[1]));
  for (int l = 1; l < n_hidden; ++l) {
    a.t_off[l] = (int)(fwd + turned);
    turned += (int64_t)s32(16 * t16(sizes[l + 1])) * t16(sizes[l]);
  }
  // the segment table, in the order the kernel walks the forward image: layers 0 .. n-1 K-step major, the s head tile major;
  // then the turned blocks: the first layer input-tile major, hidden layer l K-step major
  a.n_seg = 0;
  int dst = 0;
  for (int l = 0; l < n_hidden; ++l) {
    const int in_cols = l == 0 ? dim : 16 * t16(sizes[l]);
    const int MT = t16(sizes[l + 1]), nb = s32(in_cols) * MT;
    a.seg[a.n_seg++] = SeqBwdSeg{a.net.w_off[l], a.m_off[l], sizes[l], sizes[l + 1], sizes[l + 1], 0, MT, 1, nb, dst};
    dst += nb;
  }
  {
    const int KS = s32(16 * MTh);
    a.seg[a.n_seg++] = SeqBwdSeg{a.s_w, a.m_off[n_hidden], hl, dim, 2 * dim, 0, KS, 0, M * KS, dst};
  }
  {
    const int KS1 = s32(16 * t16(sizes[1]));
    a.seg[a.n_seg++] = SeqBwdSeg{a.net.w_off[0], a.m_off[0], dim, sizes[1], sizes[1], 1, KS1, 0, M * KS1, a.t_off[0]};
  }
  for (int l = 1; l < n_hidden; ++l) {
    const int MTp = t16(sizes[l]);
    a.seg[a.n_seg++] = SeqBwdSeg{a.net.w_off[l], a.m_off[l], sizes[l], sizes[l + 1], sizes[l + 1], 1, MTp, 1,
                                 s32(16 * t16(sizes[l + 1])) * MTp, a.t_off[l]};
  }
  a.hp = 16 * MTh;
  const int64_t fixed = 4ll * kSeqBwdHeadWords + (fwd + turned) * rt::kBlockWords * 4 + tiles * 64 + 2ll * dim * a.hp * 4;
  const int64_t slab = 2ll * 1024 * M;  // G and e^{-s}: 16 rows x 16 M columns of floats each
  if (fixed > (int64_t)kRtLdsBytes) return false;
  a.fwd_blocks = (int)fwd;
  a.turned_blocks = (int)turned;
  a.bias_tiles = (int)tiles;
  const int nw = fit_slab_waves(8, (size_t)fixed, (size_t)slab);
  if (nw < 1) return false;
  p.mt_max = kSeqBwdClass;
  p.resident = true;
  p.nw = nw;
  p.lds = (size_t)(fixed + nw * slab);
  return true;
}

// floats, each part a whole number of 16-byte groups: cot | the weight pass's discarded grad_x | neg_ld | one scale
static int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }
static int64_t seq_bwd_workspace(int64_t rows, int dim) {
  if (rows < 1 || dim < 1 || rows * dim >= (1ll << 40)) return 0;
  return 2 * round4(rows * dim) + round4(rows) + 4;
}

// the plan's kernel, its dynamic-LDS attribute set
static void (*maf_seq_bwd_rt_kernel_of(const RtPlan&))(MafSeqBwdArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, maf_seq_bwd_rt_kernel);
  return maf_seq_bwd_rt_kernel;
}

static int maf_seq_bwd_rt_run(const float* y, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                              const float* flat, const uint8_t* masks, const float* grad_scale_dev, int64_t rows, int dim,
                              int parity, int n_hidden, const int* hidden, bool det, float* workspace, int64_t workspace_floats,
                              void* stream) {
  if (!y || !grad_x || y == grad_x || !flat || !masks || !grad_scale_dev || !workspace || rows < 0 || dim < 1 || n_hidden < 1 ||
      !hidden_ok(n_hidden, hidden) || (grad_y && grad_y == grad_x) || (grad_flat && grad_flat == flat))
    return MNF_ERR_INVALID_ARG;
  if (rows == 0) return MNF_OK;
  if ((!det && deterministic()) || rows * dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  const int64_t own = seq_bwd_workspace(rows, dim);
  if (workspace_floats < own) return MNF_ERR_INVALID_ARG;
  MafSeqBwdArgs a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  if (!maf_seq_bwd_rt_plan(dim, n_hidden, hidden, a, p)) return MNF_ERR_UNSUPPORTED;
  const int64_t slots = det && grad_flat ? mnf_maf_bwd_rt_det_workspace(rows, dim, n_hidden, hidden) : 0;
  if (workspace_floats < own + slots) return MNF_ERR_INVALID_ARG;
  float* cot = workspace;
  float* gx2 = cot + round4(rows * dim);
  float* neg_ld = gx2 + round4(rows * dim);
  float* scale2 = neg_ld + round4(rows);
  a.y = y; a.grad_y = grad_y; a.grad_ld = grad_ld; a.grad_x = grad_x; a.cot = cot; a.neg_ld = grad_ld ? neg_ld : nullptr;
  a.flat = flat; a.masks = masks; a.gscale_dev = grad_scale_dev; a.rows = rows; a.dim = dim; a.parity = parity != 0;
  a.vec = dim % 4 == 0 && aligned16(y, grad_x, grad_y, cot);
  int rc = launch_plan(maf_seq_bwd_rt_kernel_of(p), a, p, 1, rows, "maf_seq_bwd_rt", (hipStream_t)stream);
  if (rc != MNF_OK || !grad_flat) return rc;
  // the parameter gradients: the one-pass direction's at x := y, grad_y := cot, grad_ld := -grad_ld, parity := 0
  rc = mnf_affine_half_grad_scale(cot, a.neg_ld, rows, dim, scale2, stream);
  if (rc != MNF_OK) return rc;
  rc = det ? mnf_maf_bwd_rt_det(y, cot, a.neg_ld, gx2, grad_flat, flat, masks, scale2, rows, dim, 0, n_hidden, hidden,
                                scale2 + 4, workspace_floats - own, stream)
           : mnf_maf_bwd_rt(y, cot, a.neg_ld, gx2, grad_flat, flat, masks, scale2, rows, dim, 0, n_hidden, hidden, stream);
  tag_kernel("maf_seq_bwd_rt");
  return rc;
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_maf_seq_bwd_rt_supported(int dim, int n_hidden, const int* hidden) {
  return rt_has_plan<MafSeqBwdArgs>([&](MafSeqBwdArgs& a, RtPlan& p) { return maf_seq_bwd_rt_plan(dim, n_hidden, hidden, a, p); });
}

extern "C" int64_t mnf_maf_seq_bwd_rt_workspace(int64_t rows, int dim) { return seq_bwd_workspace(rows, dim); }

extern "C" int64_t mnf_maf_seq_bwd_rt_det_workspace(int64_t rows, int dim, int n_hidden, const int* hidden) {
  const int64_t own = seq_bwd_workspace(rows, dim);
  return own > 0 ? own + mnf_maf_bwd_rt_det_workspace(rows, dim, n_hidden, hidden) : 0;
}

extern "C" int mnf_maf_seq_bwd_rt(const float* y, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                                  const float* flat, const uint8_t* masks, const float* grad_scale_dev, int64_t rows, int dim,
                                  int parity, int n_hidden, const int* hidden, float* workspace, int64_t workspace_floats,
                                  void* stream) {
  return maf_seq_bwd_rt_run(y, grad_y, grad_ld, grad_x, grad_flat, flat, masks, grad_scale_dev, rows, dim, parity, n_hidden,
                            hidden, false, workspace, workspace_floats, stream);
}

extern "C" int mnf_maf_seq_bwd_rt_det(const float* y, const float* grad_y, const float* grad_ld, float* grad_x, float* grad_flat,
                                      const float* flat, const uint8_t* masks, const float* grad_scale_dev, int64_t rows,
                                      int dim, int parity, int n_hidden, const int* hidden, float* workspace,
                                      int64_t workspace_floats, void* stream) {
  return maf_seq_bwd_rt_run(y, grad_y, grad_ld, grad_x, grad_flat, flat, masks, grad_scale_dev, rows, dim, parity, n_hidden,
                            hidden, true, workspace, workspace_floats, stream);
}
