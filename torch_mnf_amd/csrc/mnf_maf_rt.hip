// The one-pass direction of MAF / IAF (MAF.inverse, IAF.forward: torch_mnf/flows/maf.py:53-62) for ANY MADE shape on the
// f16 matrix pipe: net = MADE(dim, h_1 .. h_n, 2 dim) (layers/made.py: MaskedLinear + ReLU) with any number of hidden
// layers of widths 4 .. 128, any dim; run-time shapes (mnf_rt.h), weights read from the plain `flat` parameter vector,
// masks from the byte buffer mnf_maf takes.  That direction is one pass of a masked MLP followed by z = x e^s + t --
// nothing about it is sequential.  The element-by-element direction (MAF.forward, IAF.inverse: maf.py:39-51) is the second
// kernel family of this file, maf_seq_rt (below maf_rt_plan).
//
// A wave owns one 16-row tile: the last hidden vector with the row streamed from memory K-step by K-step (every input
// column: the masks do the autoregressive part), then the last MaskedLinear walked 16 output dims at a time as two heads,
// s = rows 0 .. dim-1 and t = rows dim .. 2 dim-1: y_j = x_j e^{s_j} + t_j, stored at column dim-1-j when `parity`, and the
// row's log|det J| = sum_j s_j in registers.  A masked-out weight is staged as exactly 0 (a select), and the scan for the
// launch's staging exponent leaves it out.  One size class (8 hidden tiles), resident and streaming, the rows' alignment
// taken at run time: the library's size budget holds no more.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mnf_hip.h"
#include "mnf_rnvp_common.h"
#include "mnf_rt_host.h"

namespace mnf {

struct MafRtArgs {
  const float* x;
  float* y;
  float* log_det;
  const float* flat;
  const uint8_t* masks;
  int64_t rows;
  int dim, parity, accumulate;
  int n_params, vec;  // vec: rows are 16-byte aligned and dim % 4 == 0 (dwordx4 row accesses)
  int s_w, s_b;       // float offsets of the last MaskedLinear (s = its first dim rows, t = the next dim)
  int cb, bt;
  int block_words, bias_words;
  int m_off[MNF_MAX_LINEAR];  // byte offset of layer l's mask
  NetDesc net;                // dim -> h_1 .. h_n: the layers that end in a hidden vector
};

template <int MT_MAX, bool PREFILL, typename Src>
__device__ __forceinline__ void maf_rt_block(const MafRtArgs& a, Src& src, float wup, int64_t row0) {
  using namespace rt;
  const bool VEC = a.vec != 0;  // (uniform)
  constexpr int NTL = 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int d = a.dim;
  const int64_t r = row0 + (int64_t)wave * 16 + j;
  const bool live = !PREFILL && r < a.rows;
  const int64_t rc = r < a.rows ? r : a.rows - 1;
  const float* xrow = a.x + rc * d;
  float* yrow = a.y + rc * d;

  Hidden<MT_MAX, NTL> h;
  auto load_x = [&](int, int ks, f32x4& xa, f32x4& xb) {
    const int c0 = 32 * ks + 4 * q;
    xa = load4(xrow, c0, d, VEC);
    xb = load4(xrow, c0 + 16, d, VEC);
  };
  auto use_x = [&](int, int, const f32x4&, const f32x4&) {};
  const int n_hid = a.net.n_lin;  // every layer of `net` ends in a hidden vector, each with its ReLU
  const MaskedLayers layers{a.masks, a.m_off, a.net.sizes};
  net_to_hidden<MT_MAX, NTL, PREFILL>(src, a.flat, a.net, n_hid, -1, wup, lane, q, load_x, use_x, h, NoLayerHook(), layers);

  // ---- the last MaskedLinear, 16 output dims at a time: blocks [tile][s | t][K-step]
  const int hl = a.net.sizes[n_hid];
  const int KS = steps32(16 * tiles16(hl)), M = tiles16(d);
  int MO = Src::resident ? M : src.cb / (2 * KS);
  if (!Src::resident && MO > src.bt / 2) MO = src.bt / 2;
  if (MO < 1) MO = 1;
  const float* W0 = a.flat + a.s_w;
  const float* B0 = a.flat + a.s_b;
  const uint8_t* M0 = a.masks + a.m_off[n_hid];
  float ld = 0.f;
  f32x4 nx;  // the next tile's columns (requested one tile ahead)
  if (!PREFILL) nx = load4(xrow, 4 * q, d, VEC);
  for (int m0 = 0; m0 < M; m0 += MO) {
    const int mo = M - m0 < MO ? M - m0 : MO;
    const Chunk c = src.template chunk<PREFILL>(mo * 2 * KS, MaskedMMajor{W0, hl, d, KS, m0, 2, (int64_t)d * hl, M0, 2 * d, d},
                                                mo * 2, DenseBiasHeads{B0, d, m0, 2, d});
    if (PREFILL) continue;
    for (int ml = 0; ml < mo; ++ml) {
      const int m = m0 + ml, col = 16 * m + 4 * q;
      const f32x4 xx = nx;
      const int m_next = m + 1 < M ? m + 1 : M - 1;
      nx = load4(xrow, 16 * m_next + 4 * q, d, VEC);
      f32x4 s4[NTL], t4[NTL];
      out_tile<MT_MAX, NTL>(c.A, (ml * 2) * KS, KS, c.bias + (ml * 2) * 16, lane, q, h, wup, s4);
      out_tile<MT_MAX, NTL>(c.A, (ml * 2 + 1) * KS, KS, c.bias + (ml * 2 + 1) * 16, lane, q, h, wup, t4);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = __builtin_fmaf(xx[e], exp6r(s4[0][e]), t4[0][e]);  // (:57)
        ld += col + e < d ? s4[0][e] : 0.f;                       // padding columns: s = 0
      }
      if (!a.parity) {  // (uniform)
        store4(yrow, col, d, VEC, live, o);
      } else if (VEC) {  // z.flip(dims=(1,)) (:58): columns col .. col + 3 land on d-1-col .. d-4-col, one dwordx4 (d % 4 == 0)
        if (live && col < d) *reinterpret_cast<f32x4*>(yrow + (d - 4 - col)) = f32x4{o[3], o[2], o[1], o[0]};
      } else if (live) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e < d) yrow[d - 1 - col - e] = o[e];
      }
    }
  }
  if (PREFILL) return;
  const float total = sum_over_q(ld);
  if (q == 0 && live && a.log_det) a.log_det[r] = a.accumulate ? a.log_det[r] + total : total;
}

template <int MT_MAX, int NW, bool RESIDENT>
__global__ void __launch_bounds__(NW * 64) maf_rt_kernel(MafRtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + 16;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  const int n_hid = a.net.n_lin;
  float wmx = rt::net_weight_max(a.flat, a.net, a.masks, a.m_off, 0.f);
  wmx = rt::masked_abs_max(a.flat + a.s_w, a.masks + a.m_off[n_hid], a.net.sizes[n_hid], 2 * a.dim, wmx);
  const float wmax = rt::block_weight_max(wmx, scratch);
  const int e = rt::weight_exponent(wmax);
  const float wup = rt::pow2f(e);
  rt::Source<RESIDENT> src{blocks, bias, a.cb, a.bt, 0, 0, 0, rt::pow2f(-e), 0};
  if (RESIDENT) {
    maf_rt_block<MT_MAX, true>(a, src, wup, 0);
    __syncthreads();
  }
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    src.slot = 0;
    src.btile = 0;
    maf_rt_block<MT_MAX, false>(a, src, wup, b * rows_per_block);
  }
}

constexpr int kMafRtClass = 8, kMafRtWaves = 8;  // the one size class built: hidden widths up to 128

// The launch of a shape, or false: the VALU kernel takes it.  Fills the kernel arguments' shape part.
static bool maf_rt_plan(int dim, int n_hidden, const int* hidden, MafRtArgs& a, RtPlan& p) {
  if (dim < 1 || n_hidden < 1 || !hidden_ok(n_hidden, hidden)) return false;
  int sizes[MNF_MAX_LINEAR + 1];
  sizes[0] = dim;
  const HiddenWidths w = scan_hidden(n_hidden, hidden, sizes);
  if (w.min < 4 || w.max > 16 * kMafRtClass) return false;
  const int64_t n_params = maf_layout(dim, n_hidden, sizes, a);
  if (!n_params) return false;
  a.n_params = (int)n_params;
  // the resident image: the net, then the last MaskedLinear's s and t tiles
  StagedTiles image = mlp_tiles(sizes, n_hidden, dim);
  const int KS = (16 * ((hidden[n_hidden - 1] + 15) / 16) + 31) / 32, M = (dim + 15) / 16;
  image.blocks += 2ll * KS * M;
  image.bias += 2ll * M;
  plan_staging(a, p, image, /*resident_bytes=*/150 * 1024, /*stream=*/16);
  p.mt_max = kMafRtClass;
  p.nw = kMafRtWaves;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// The element-by-element direction (MAF.forward, IAF.inverse: flows/maf.py:39-51), family maf_seq_rt: per 16-row tile, for
// i = 0 .. dim-1, the masked net on the partially decoded row (columns < i decoded, columns >= i exactly 0: maf.py:43-50,
// right for any MADE), of the last MaskedLinear only output tile i >> 4, and in the lane that holds column i
// v = (z_i - t_i) e^{-s_i}, z_i = x[parity ? dim-1-i : i] (the input is flipped, the output is not).
//
// Resident plans only: the converted net is staged once per workgroup, and after the barrier behind that the waves never
// meet again -- a streaming plan would re-stage every chunk dim times per row block with a barrier each.  The decoded tile
// sits in a per-wave LDS slab, float4 (column group g, row j) at slab[16 g + j]: first_layer asks lane (j, q) for columns
// 32 ks + 4 q + (0..3) and + 16, out_tile hands lane (j, q) columns 16 m + 4 q + (0..3), so the lane that decodes column c
// of row j -- q = (c % 16) / 4 -- is the only lane that ever reads it: no barrier, no cross-lane traffic between steps, and
// the slab's reads and writes are one lane's own LDS accesses in program order.  "Columns >= i are 0" is a select on the
// value read (the slab is never cleared; what a tile's predecessor left there is not looked at).  Step i walks only the
// K-steps of the first layer that hold a column < i (the others multiply zeros): its NetDesc says n_in = max(i, 1).
// Rows past the end read the last row (clamped) and never store.
// ---------------------------------------------------------------------------------------------------------------------
template <int MT_MAX, bool PREFILL, typename Src>
__device__ __forceinline__ void maf_seq_rt_block(const MafRtArgs& a, Src& src, float wup, int64_t row0, float* slab) {
  using namespace rt;
  const bool VEC = a.vec != 0;  // (uniform)
  constexpr int NTL = 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int d = a.dim;
  const int n_hid = a.net.n_lin;
  const MaskedLayers layers{a.masks, a.m_off, a.net.sizes};
  const int hl = a.net.sizes[n_hid];
  const int KS = steps32(16 * tiles16(hl)), M = tiles16(d);
  // the last MaskedLinear, every output tile: blocks [tile][s | t][K-step], as maf_rt_block's resident chunk
  const MaskedMMajor out_fetch{a.flat + a.s_w, hl, d, KS, 0, 2, (int64_t)d * hl, a.masks + a.m_off[n_hid], 2 * d, d};
  const DenseBiasHeads out_bias{a.flat + a.s_b, d, 0, 2, d};
  auto use_x = [&](int, int, const f32x4&, const f32x4&) {};
  Hidden<MT_MAX, NTL> h;
  if (PREFILL) {
    auto no_x = [&](int, int, f32x4&, f32x4&) {};
    net_to_hidden<MT_MAX, NTL, true>(src, a.flat, a.net, n_hid, -1, wup, lane, q, no_x, use_x, h, NoLayerHook(), layers);
    src.template chunk<true>(M * 2 * KS, out_fetch, M * 2, out_bias);
    return;
  }
  const int64_t r = row0 + (int64_t)wave * 16 + j;
  const bool live = r < a.rows;
  const int64_t rc = live ? r : a.rows - 1;
  const float* xrow = a.x + rc * d;
  float* yrow = a.y + rc * d;
  const int G = (d + 3) >> 2;                           // the slab's column groups
  f32x4* tile = reinterpret_cast<f32x4*>(slab) + j;     // group g of this lane's row at tile[16 g]
  const int first_blocks = steps32(d) * tiles16(a.net.sizes[1]), first_bias = tiles16(a.net.sizes[1]);
  NetDesc first;  // layer 0 over columns < i (first_layer reads these four fields)
  first.sizes[1] = a.net.sizes[1];
  first.w_off[0] = a.net.w_off[0];
  first.b_off[0] = a.net.b_off[0];
  const NetDesc* const nds[1] = {&first};
  // z_i four at a time (columns i0 .. i0 + 3 of the flipped input), requested one group ahead
  auto load_z4 = [&](int i0) -> f32x4 {
    if (!a.parity) return load4(xrow, i0, d, VEC);  // (uniform)
    if (VEC) {  // d % 4 == 0: columns d-1-i0 .. d-4-i0, one dwordx4
      const f32x4 v = *reinterpret_cast<const f32x4*>(xrow + (d - 4 - i0));
      return f32x4{v[3], v[2], v[1], v[0]};
    }
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = i0 + e < d;
      const float x = xrow[ok ? d - 1 - i0 - e : 0];
      v[e] = ok ? x : 0.f;
    }
    return v;
  };
  float ld = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f}, z4 = o;
  f32x4 nz = load_z4(0);
  for (int i = 0; i < d; ++i) {
    const int e = i & 3;
    if (e == 0) {  // (uniform)
      z4 = nz;
      nz = load_z4(i + 4 < d ? i + 4 : i);
    }
    auto load_x = [&](int, int ks, f32x4& xa, f32x4& xb) {
      const int ga = 8 * ks + q, gb = ga + 4;
      const f32x4 va = tile[16 * (ga < G ? ga : 0)], vb = tile[16 * (gb < G ? gb : 0)];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        xa[c] = 4 * ga + c < i ? va[c] : 0.f;  // not yet decoded: 0 (maf.py:43)
        xb[c] = 4 * gb + c < i ? vb[c] : 0.f;
      }
    };
    first.sizes[0] = i > 0 ? i : 1;
    src.slot = 0;
    src.btile = 0;
    Hidden<MT_MAX, NTL> h1[1];
    first_layer<MT_MAX, NTL, false, 1>(src, a.flat, nds, true, wup, lane, q, load_x, use_x, h1, NoLayerHook(), layers);
    src.slot = first_blocks;  // (the resident image holds every K-step of layer 0)
    src.btile = first_bias;
    h = h1[0];
    hidden_layers<MT_MAX, NTL, false>(src, a.flat, a.net, n_hid, -1, wup, lane, q, h, NoLayerHook(), layers);
    const Chunk c = src.template chunk<false>(M * 2 * KS, out_fetch, M * 2, out_bias);
    const int m = i >> 4;
    f32x4 s4[NTL], t4[NTL];
    out_tile<MT_MAX, NTL>(c.A, (m * 2) * KS, KS, c.bias + (m * 2) * 16, lane, q, h, wup, s4);
    out_tile<MT_MAX, NTL>(c.A, (m * 2 + 1) * KS, KS, c.bias + (m * 2 + 1) * 16, lane, q, h, wup, t4);
    auto pick = [&](const f32x4& v) { return e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3]; };  // (uniform)
    const float s = pick(s4[0]), t = pick(t4[0]);
    const float v = (pick(z4) - t) * exp6r(-s);  // (:49)
    const bool own = q == ((i & 15) >> 2);       // the lane (j, q) that holds column i
    if (own) slab[(16 * (i >> 2) + j) * 4 + e] = v;
    ld -= own ? s : 0.f;  // (:50)
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) o[c4] = c4 == e ? v : o[c4];
    if (e == 3 || i == d - 1) store4(yrow, i & ~3, d, VEC, live && own, o);
  }
  const float total = sum_over_q(ld);
  if (q == 0 && live && a.log_det) a.log_det[r] = a.accumulate ? a.log_det[r] + total : total;
}

__global__ void __launch_bounds__(kMafRtWaves * 64) maf_seq_rt_kernel(MafRtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t rt_lds[];
  float* scratch = reinterpret_cast<float*>(rt_lds);
  uint32_t* blocks = rt_lds + 16;
  float* bias = reinterpret_cast<float*>(blocks + a.block_words);
  float* slab = bias + a.bias_words + (threadIdx.x >> 6) * (64 * ((a.dim + 3) >> 2));  // this wave's 16 x dim floats
  const int n_hid = a.net.n_lin;
  float wmx = rt::net_weight_max(a.flat, a.net, a.masks, a.m_off, 0.f);
  wmx = rt::masked_abs_max(a.flat + a.s_w, a.masks + a.m_off[n_hid], a.net.sizes[n_hid], 2 * a.dim, wmx);
  const float wmax = rt::block_weight_max(wmx, scratch);
  const int e = rt::weight_exponent(wmax);
  const float wup = rt::pow2f(e);
  rt::Source<true> src{blocks, bias, a.cb, a.bt, 0, 0, 0, rt::pow2f(-e), 0};
  maf_seq_rt_block<kMafRtClass, true>(a, src, wup, 0, slab);
  __syncthreads();
  const int64_t rows_per_block = (int64_t)(blockDim.x >> 6) * 16;
  const int64_t n_blocks = (a.rows + rows_per_block - 1) / rows_per_block;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) maf_seq_rt_block<kMafRtClass, false>(a, src, wup, b * rows_per_block, slab);
}

// The launch of a shape on maf_seq_rt, or false: maf_rt_plan's resident plans, with a slab of 16 x dim floats per wave
// behind the net and as many waves per workgroup (8 / 4 / 2 / 1) as the 160 KB of LDS then hold.
static bool maf_seq_rt_plan(int dim, int n_hidden, const int* hidden, MafRtArgs& a, RtPlan& p) {
  if (!maf_rt_plan(dim, n_hidden, hidden, a, p) || !p.resident) return false;
  const size_t slab = (size_t)256 * ((dim + 3) / 4);
  const int nw = fit_slab_waves(kMafRtWaves, p.lds, slab);
  if (nw < 1) return false;
  p.nw = nw;
  p.lds += nw * slab;
  return true;
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_maf_rt_supported(int dim, int n_hidden, const int* hidden) {
  return rt_has_plan<MafRtArgs>([&](MafRtArgs& a, RtPlan& p) { return maf_rt_plan(dim, n_hidden, hidden, a, p); });
}

static void (*maf_rt_kernel_of(const RtPlan& p))(MafRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, maf_rt_kernel<kMafRtClass, kMafRtWaves, true>, maf_rt_kernel<kMafRtClass, kMafRtWaves, false>);
  return p.resident ? maf_rt_kernel<kMafRtClass, kMafRtWaves, true> : maf_rt_kernel<kMafRtClass, kMafRtWaves, false>;
}

// workgroups of the launch (each walks the row blocks of 16 x 8 rows blockIdx.x, + grid, ...); 0: no launch, or no device
extern "C" int64_t mnf_maf_rt_grid(int64_t rows, int dim, int n_hidden, const int* hidden) {
  return rt_grid_query<MafRtArgs>(
      rows, 1, [&](MafRtArgs& a, RtPlan& p) { return maf_rt_plan(dim, n_hidden, hidden, a, p); }, maf_rt_kernel_of);
}

extern "C" int mnf_maf_rt(const float* x, float* y, float* log_det, int accumulate, const float* flat, const uint8_t* masks,
                          int64_t rows, int dim, int parity, int n_hidden, const int* hidden, void* stream) {
  if (!x || !y || x == y || !flat || !masks || rows < 0 || dim < 1 || n_hidden < 1 || !hidden_ok(n_hidden, hidden))
    return MNF_ERR_INVALID_ARG;
  if (rows == 0) return MNF_OK;
  if (rows * dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  MafRtArgs a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  if (!maf_rt_plan(dim, n_hidden, hidden, a, p)) return MNF_ERR_UNSUPPORTED;
  a.x = x; a.y = y; a.log_det = log_det; a.flat = flat; a.masks = masks; a.rows = rows; a.dim = dim;
  a.parity = parity != 0;
  a.accumulate = accumulate != 0;
  a.vec = dim % 4 == 0 && aligned16(x, y);
  return launch_plan(maf_rt_kernel_of(p), a, p, 1, rows, "maf_rt", (hipStream_t)stream);
}

static void (*maf_seq_rt_kernel_of(const RtPlan&))(MafRtArgs) {
  static DeviceMemo attr;
  allow_big_lds(attr, maf_seq_rt_kernel);
  return maf_seq_rt_kernel;
}

extern "C" int mnf_maf_seq_rt_supported(int dim, int n_hidden, const int* hidden) {
  return rt_has_plan<MafRtArgs>([&](MafRtArgs& a, RtPlan& p) { return maf_seq_rt_plan(dim, n_hidden, hidden, a, p); });
}

// workgroups of the launch (each walks the row blocks of 16 x waves rows blockIdx.x, + grid, ...); 0: no launch, or no device
extern "C" int64_t mnf_maf_seq_rt_grid(int64_t rows, int dim, int n_hidden, const int* hidden) {
  return rt_grid_query<MafRtArgs>(
      rows, 1, [&](MafRtArgs& a, RtPlan& p) { return maf_seq_rt_plan(dim, n_hidden, hidden, a, p); }, maf_seq_rt_kernel_of);
}

extern "C" int mnf_maf_seq_rt(const float* x, float* y, float* log_det, int accumulate, const float* flat, const uint8_t* masks,
                              int64_t rows, int dim, int parity, int n_hidden, const int* hidden, void* stream) {
  if (!x || !y || x == y || !flat || !masks || rows < 0 || dim < 1 || n_hidden < 1 || !hidden_ok(n_hidden, hidden))
    return MNF_ERR_INVALID_ARG;
  if (rows == 0) return MNF_OK;
  if (rows * dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  MafRtArgs a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  if (!maf_seq_rt_plan(dim, n_hidden, hidden, a, p)) return MNF_ERR_UNSUPPORTED;
  a.x = x; a.y = y; a.log_det = log_det; a.flat = flat; a.masks = masks; a.rows = rows; a.dim = dim;
  a.parity = parity != 0;
  a.accumulate = accumulate != 0;
  a.vec = dim % 4 == 0 && aligned16(x, y);
  return launch_plan(maf_seq_rt_kernel_of(p), a, p, 1, rows, "maf_seq_rt", (hipStream_t)stream);
}
