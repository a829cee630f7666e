// y = x @ W for Glow's d x d matrix on the fp32 matrix cores: per-shape kernels (d in {16, 32, 64, 128}) and, below
// them, the run-time-shaped pair for any d up to 1024 (forward / grad_x and the weight gradient) and, built on those
// two, Glow.inverse + ActNormFlow.inverse as one launch each way at any such d (glow_actnorm_inv_rt, _bwd_rt).
//
// Same transposed scheme as the coupling kernels: one wave owns 16 rows; lane (j, q) loads the
// row as float4s (element 16 g + 4 q + e is the k = q operand of K-step 4 g + e); output tile m
// leaves dims 16 m + 4 q + r in register r of lane (j, q), i.e. a float4 of the output row.
// W is pre-arranged into A-operand order (image) and copied to LDS once per workgroup.
// HBM-bound: 8 d bytes per row, 2 d^2 flops per row (d = 32: 8 flop/B).
#include <hip/hip_runtime.h>

#include "mnf_device.h"
#include "mnf_rt_host.h"  // (the Glow kernels at any dim launch like the run-time-shaped ones)

namespace mnf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kLinWaves = 4;

template <int D>
__global__ void __launch_bounds__(kLinWaves * 64)
linear_rows_mfma_kernel(const float* __restrict__ x, const float* __restrict__ image, float* __restrict__ y,
                        int64_t rows) {
  constexpr int G = D / 16, NK = D / 4;
  __shared__ __attribute__((aligned(16))) float lds[D * D];
  {
    const float4* src = reinterpret_cast<const float4*>(image);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < D * D / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int n_tiles = (int)((rows + 15) >> 4);
  for (int tile = (int)blockIdx.x * kLinWaves + wave; tile < n_tiles; tile += (int)gridDim.x * kLinWaves) {
    const int64_t row = (int64_t)tile * 16 + j;
    const bool live = row < rows;
    const int64_t rowc = live ? row : rows - 1;
    const float* xr = x + rowc * D + 4 * q;
    f32x4 xv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) xv[g] = *reinterpret_cast<const f32x4*>(xr + 16 * g);
    int a_off = lane * 4;
    asm volatile("" : "+v"(a_off));  // keep the operand reads in the loop (see mnf_ahf_mfma.hip)
    const f32x4* A4 = reinterpret_cast<const f32x4*>(lds + a_off);
    f32x4 acc[G];
#pragma unroll
    for (int m = 0; m < G; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    int n = 0;
    f32x4 a4;
#pragma unroll
    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
      for (int m = 0; m < G; ++m) {
        if ((n & 3) == 0) a4 = A4[64 * (n >> 2)];
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[n & 3], xv[kk >> 2][kk & 3], acc[m], 0, 0, 0);
        ++n;
      }
    if (live) {
      float* yr = y + rowc * D + 4 * q;
#pragma unroll
      for (int m = 0; m < G; ++m) *reinterpret_cast<f32x4*>(yr + 16 * m) = acc[m];
    }
  }
}

template <int D>
static void build_index(int32_t* idx) {
  constexpr int G = D / 16, NK = D / 4;
  int n = 0;
  for (int kk = 0; kk < NK; ++kk) {
    const int g = kk >> 2, e = kk & 3;
    for (int m = 0; m < G; ++m, ++n)
      for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 15, kq = lane >> 4;
        idx[(n >> 2) * 256 + lane * 4 + (n & 3)] = (16 * g + 4 * kq + e) * D + 16 * m + i;  // W[k][out]
      }
  }
}

template <int D>
static int launch(const float* x, const float* image, float* y, int64_t rows, hipStream_t stream) {
  const int64_t n_tiles = (rows + 15) / 16;
  int64_t blocks = (n_tiles + kLinWaves - 1) / kLinWaves;
  if (blocks > 256 * 8) blocks = 256 * 8;
  tag_kernel("linear_rows_mfma");
  hipLaunchKernelGGL((linear_rows_mfma_kernel<D>), dim3((unsigned)blocks), dim3(kLinWaves * 64), 0, stream, x,
                     image, y, rows);
  return check_launch();
}

// ------------------------------------------------------------------------------------------------------------------
// The run-time-shaped pair (any 2 <= dim <= 1024, no template parameter): y = x @ M and grad_W += x^T g.
//
// linear_rows_rt_kernel.  The same transposed scheme -- a wave owns 16 rows, M^T tiles are the A operand, the rows the B
// operand, so lane (j, q) leaves with columns 16 t + 4 q .. + 3 of row j (a dwordx4 store when dim % 4 == 0 and the
// pointers are aligned: `vec`) -- but with k ASCENDING: K-step s multiplies k = 4 s + q, lane (j, q) loads the one float
// x[row j][4 s + q] for it, and every output element is ONE accumulator that starts at 0 and walks k = 0 .. dim - 1
// through all K-chunks.  v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, so y is bit for bit linear_rows_kernel's
// (up to the sign of a zero: the zero-padded k-steps add fma(0, 0, acc)).  M -- read transposed when `trans`, which is
// grad_x = grad_y @ W^T without a copy -- is staged into LDS as Ml[k][column], zero past dim on both axes, rows of ldw
// = 16 mod 64 floats (the four k of a K-step on distinct banks).  A dim whose whole M fits stays resident for the
// persistent workgroup; above that a workgroup streams [64 k][128 columns] chunks through two buffers, one LDS-only
// barrier per chunk.  Column tiles go in groups of 8 (32 accumulator registers), the row tile is re-read per group;
// the independent accumulators that hide the MFMA's dependent latency are the group's tiles.  Past `rows` the
// addresses are clamped and the stores skipped.  8 dim bytes per row; 2 dim^2 flop per row.
struct LinRtArgs {
  const float* x;
  const float* M;
  float* y;
  int64_t rows;
  int dim, trans, vec, resident, krows, ldw, ncols, ngroups, nw, grid;  // (nw, grid: the launch's own, as arguments)
};
constexpr int kLinRtChunkK = 64, kLinRtGroupCols = 128;

__device__ __forceinline__ void lin_rt_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// chunk `s` of a row round (column group s / nkc, k rows (s % nkc) * krows ..) -> buf; lanes run along M's rows
__device__ __forceinline__ void lin_rt_stage(const LinRtArgs& a, int s, int nkc, float* buf, int lane, int wave, int nw) {
  const int g = s / nkc, k0 = (s - g * nkc) * a.krows, c0 = a.resident ? 0 : g * kLinRtGroupCols, dim = a.dim;
  const int n_fast = a.trans ? a.krows : a.ncols, n_slow = a.trans ? a.ncols : a.krows;
  for (int sl = wave; sl < n_slow; sl += nw)
    for (int f = lane; f < n_fast; f += 64) {
      const int kk = a.trans ? f : sl, c = a.trans ? sl : f;
      const int k = k0 + kk, col = c0 + c;
      const bool ok = k < dim && col < dim;
      const float v = a.M[ok ? (a.trans ? col * dim + k : k * dim + col) : 0];
      buf[kk * a.ldw + c] = ok ? v : 0.f;
    }
}

__global__ void __launch_bounds__(512) linear_rows_rt_kernel(LinRtArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lin_rt_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = a.nw;
  const int j = lane & 15, q = lane >> 4, dim = a.dim, ldw = a.ldw;
  const int ntile = (dim + 15) >> 4;
  const int nkc = a.resident ? 1 : (dim + a.krows - 1) / a.krows, steps = a.ngroups * nkc;
  const int buf_floats = a.krows * ldw;
  const int64_t n_tiles = (a.rows + 15) >> 4;
  f32x4 acc[8];
  bool staged = false;
  for (int64_t base = (int64_t)blockIdx.x * nw; base < n_tiles; base += (int64_t)a.grid * nw) {
    const int64_t row = (base + wave) * 16 + j;
    const bool live = row < a.rows;
    const int64_t roff = (live ? row : a.rows - 1) * dim;
    const float* xr = a.x + roff;
    float* yr = a.y + roff;
    // step s = (column group g, K-chunk c); step -1 only stages.  Streaming: chunk s + 1 goes into the other buffer
    // while chunk s is multiplied, one barrier per step (the buffer written next is free once every wave is past it).
    for (int s = -1, g = 0, c = 0; s < steps; ++s) {
      if (a.resident ? !staged : s + 1 < steps) {
        lin_rt_stage(a, s + 1, nkc, lin_rt_lds + (a.resident ? 0 : ((s + 1) & 1) * buf_floats), lane, wave, nw);
        staged = true;
        if (a.resident) lin_rt_barrier();
      }
      if (s >= 0) {
        const int nt = min(8, ntile - 8 * g);
        if (c == 0) {
#pragma unroll
          for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* buf = lin_rt_lds + (a.resident ? g * kLinRtGroupCols : (s & 1) * buf_floats) + j;
        const int k0 = c * a.krows, kend = min(a.krows, dim - k0);
        for (int kb = 0; kb < kend; kb += 16) {  // 4 K-steps: their 4 row loads in flight together
          float xv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + kb + 4 * u + q;
            const float v = xr[min(k, dim - 1)];
            xv[u] = k < dim ? v : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (kb + 4 * u >= kend) break;
            const float* ap = buf + (kb + 4 * u + q) * ldw;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              if (t >= nt) break;
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[16 * t], xv[u], acc[t], 0, 0, 0);
            }
          }
        }
        if (++c == nkc) {
          const int lim = live ? dim : 0;  // (nothing of a row past `rows` is stored)
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            if (t >= nt) break;
            const int col = g * kLinRtGroupCols + 16 * t + 4 * q;
            if (a.vec) {
              if (col < lim) *reinterpret_cast<f32x4*>(yr + col) = acc[t];
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (col + r < lim) yr[col + r] = acc[t][r];
            }
          }
          c = 0, ++g;
        }
      }
      if (!a.resident) lin_rt_barrier();
    }
  }
}

struct LinRtPlan {
  int resident, krows, ldw, ncols, ngroups, nw;
  size_t lds;
};
static bool lin_rt_plan(int dim, LinRtPlan& p) {
  if (dim < 2 || dim > 1024) return false;
  const int dimp = (dim + 15) / 16 * 16, kr = (dim + 3) / 4 * 4;
  const int ldw = (dimp + 47) / 64 * 64 + 16;  // the smallest width >= dimp that is 16 mod 64
  p.ngroups = (dimp + kLinRtGroupCols - 1) / kLinRtGroupCols;
  p.resident = (size_t)kr * ldw * 4 <= 160 * 1024;  // dim <= 192
  if (p.resident) {
    p.krows = kr, p.ldw = ldw, p.ncols = dimp;
    p.lds = (size_t)kr * ldw * 4;
  } else {
    p.krows = kLinRtChunkK, p.ldw = kLinRtGroupCols + 16, p.ncols = kLinRtGroupCols;
    p.lds = (size_t)2 * p.krows * p.ldw * 4;
  }
  // a streamed chunk serves 16 nw rows: 8 waves halve the staging traffic per row; a resident M beyond half the LDS
  // leaves one workgroup per CU, which then needs the 8 waves too
  p.nw = p.resident && p.lds <= 80 * 1024 ? 4 : 8;
  return true;
}

// xtg_rt_kernel.  Rows on the K axis, four per instruction, as xtg32_mfma_kernel: lane (c, k) loads x[row k][i0 + 16 ti
// + c] and g[row k][j0 + 16 tj + c].  A wave owns ONE (64 x 64 output block, row slice) pair -- up to 4 x 4 tiles in 64
// registers, 8 rows of loads in flight -- and writes its sums with plain stores into part[slice][dim * dim] (a slice is
// xtg_rt_slice_floats long): every (slice, element) has exactly one writer, det_reduce_async adds the slices in order,
// and the result has the same bits every run in every mode.  Columns past dim and rows past the slice load a clamped
// address and select 0.
struct XtgRtArgs {
  const float* x;
  const float* g;
  float* part;
  int64_t rows, per;
  int dim, slices;
};
constexpr int64_t kXtgRtMaxFloats = (int64_t)8 << 20;  // the workspace's cap: 32 MB
__host__ __device__ inline int64_t xtg_rt_slice_floats(int dim) { return (int64_t)((dim + 15) / 16 * 16) * dim; }

__global__ void __launch_bounds__(256) xtg_rt_kernel(XtgRtArgs a) {
  const int lane = threadIdx.x & 63, c = lane & 15, k = lane >> 4, dim = a.dim;
  // (block = (blockIdx.y, blockIdx.x), the workgroup's waves take four slices of it: all of it scalars)
  const int slice = (int)blockIdx.z * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slice >= a.slices) return;
  const int i0 = (int)blockIdx.y * 64, j0 = (int)blockIdx.x * 64;
  const int nti = min(4, (dim - i0 + 15) >> 4), ntj = min(4, (dim - j0 + 15) >> 4);
  int xo[4], go[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    xo[t] = i0 + 16 * t + c < dim ? i0 + 16 * t + c : -1;
    go[t] = j0 + 16 * t + c < dim ? j0 + 16 * t + c : -1;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t r0 = (int64_t)slice * a.per, r1 = min(a.rows, r0 + a.per);
  constexpr int U = 2;  // 4-row groups in flight per trip
  for (int64_t rb = r0; rb < r1; rb += 4 * U) {
    float xa[U][4], ga[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = rb + 4 * u + k;
      const bool live = row < r1;
      const int64_t off = (live ? row : r0) * dim;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        xa[u][t] = ga[u][t] = 0.f;
        if (t < nti) {
          const float v = a.x[off + max(xo[t], 0)];
          xa[u][t] = live && xo[t] >= 0 ? v : 0.f;
        }
        if (t < ntj) {
          const float v = a.g[off + max(go[t], 0)];
          ga[u][t] = live && go[t] >= 0 ? v : 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        if (ti >= nti) break;
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
          if (tj >= ntj) break;
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u][ti], ga[u][tj], acc[ti][tj], 0, 0, 0);
        }
      }
  }
  // (a slice holds whole 16-row tiles, xtg_rt_slice_floats: the rows past dim receive the zeros of the padded columns)
  float* out = a.part + (int64_t)slice * xtg_rt_slice_floats(dim);
  const uint32_t o0 = (uint32_t)((i0 + 4 * k) * dim + j0 + c);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    if (tj >= ntj) break;
    if (j0 + 16 * tj + c < dim) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        if (ti >= nti) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[o0 + (uint32_t)((16 * ti + r) * dim + 16 * tj)] = acc[ti][tj][r];
      }
    }
  }
}

// Row slices of the launch: enough (block, slice) waves for 8 per CU at small dim (dim <= 64 is ONE block), at least 64
// rows each, at most 1024 and within the workspace cap; whole 16-row trips.  det_reduce_async walks its rows one by one,
// so more than kXtgRtGroup slices are added up in two steps, both in a fixed order: slices s, s + 32, s + 64, ... into
// partial sum s % 32 (32 more slice-sized blocks behind the slices), then the 32 partial sums into grad_W
// (dim = 1024: 8 slices, one step; dim = 48: up to 1024 slices, two).
constexpr int kXtgRtGroup = 32;
struct XtgRtPlan {
  int slices, groups;  // groups: 0 = one step, else kXtgRtGroup partial sums
  int64_t per, floats;
};
static XtgRtPlan xtg_rt_plan(int64_t rows, int dim, int cus) {
  const int nbj = (dim + 63) / 64, nb = nbj * nbj;
  const int64_t sf = xtg_rt_slice_floats(dim);
  int64_t s = ((int64_t)8 * cus + nb - 1) / nb;
  s = min(s, (int64_t)1024);
  int64_t cap = kXtgRtMaxFloats / sf;  // slice-sized blocks the workspace may hold, the partial sums among them
  cap = cap > 2 * kXtgRtGroup ? cap - kXtgRtGroup : min(cap, (int64_t)kXtgRtGroup);
  s = max(min(min(s, cap), (rows + 63) / 64), (int64_t)1);
  XtgRtPlan p;
  p.groups = s > kXtgRtGroup ? kXtgRtGroup : 0;
  if (p.groups) s = s / kXtgRtGroup * kXtgRtGroup;
  p.slices = (int)s;
  p.per = ((rows + s - 1) / s + 15) / 16 * 16;
  p.floats = (s + p.groups) * sf;
  return p;
}

// ------------------------------------------------------------------------------------------------------------------
// Glow.inverse followed by ActNormFlow.inverse at any 2 <= dim <= 1024 (the run-time-shaped form of mnf_glow_actnorm.hip's
// pair): z = (u @ M - t) e^-s forward, grad_u = (grad_z e^-s) @ M^T and the sums backward.
//
// glow_actnorm_inv_rt_kernel / glow_actnorm_inv_bwd_rt_kernel are linear_rows_rt_kernel's loop (same staging, same
// k-ascending chain with one accumulator per output element: u @ M has mnf_linear_rows_rt's bits) with
//   * forward: an epilogue on the lane's own columns, (acc - t[c]) * expf(-s[c]) -- affine_const_kernel's expression, so z
//     is the layer-by-layer route's bit for bit -- and, in the log-prob form, |z|^2 carried in a register across the
//     column groups of a row tile, added over the four q lanes in a fixed order, and
//     log p = log_det_rows[row] + ((ld_glow - sum s) - dim log(2 pi) / 2 - |z|^2 / 2);
//   * backward: a prologue on the row loads, grad_z[k] * expf(-s[k]) (log-prob form: (-z[k] * grad_log_prob[row]) *
//     expf(-s[k]), the product kept a product), M read transposed.
// t and e^-s are staged once per workgroup into the first 2 x 1024 floats of LDS, zero past dim (a padded column leaves
// z = 0 and adds nothing to |z|^2); M's buffers follow.  The per-row scalar is loaded from a selected pointer, never
// under a branch.
struct GaRtArgs {
  LinRtArgs l;           // x: u (forward), grad_z or z (backward: the log-prob form forms grad_z from z); y: z or grad_u
  const float* s;
  const float* t;
  const float* ld_glow;  // forward
  const float* row_in;   // log-prob form: log_det_rows (forward) / grad_log_prob (backward); else NULL
  float* ld_out;         // forward
  float* lp_out;         // forward, log-prob form
};
constexpr int kGaRtPostFloats = 2 * 1024;

template <bool BWD>
__device__ __forceinline__ void ga_rt_rows(const GaRtArgs& ga, float* lds) {
  const LinRtArgs& a = ga.l;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = a.nw;
  const int j = lane & 15, q = lane >> 4, dim = a.dim, ldw = a.ldw;
  const int ntile = (dim + 15) >> 4;
  const int nkc = a.resident ? 1 : (dim + a.krows - 1) / a.krows, steps = a.ngroups * nkc;
  const int buf_floats = a.krows * ldw;
  const int64_t n_tiles = (a.rows + 15) >> 4;
  const bool lp = ga.row_in != nullptr;
  float* tl = lds;
  float* el = lds + 1024;
  float* mbuf = lds + kGaRtPostFloats;
  for (int i = threadIdx.x; i < 1024; i += nw * 64) {  // (the first barrier of the row loop publishes them)
    const float sv = ga.s[min(i, dim - 1)], tv = ga.t[min(i, dim - 1)];
    el[i] = i < dim ? expf(-sv) : 0.f;
    if (!BWD) tl[i] = i < dim ? tv : 0.f;
  }
  float ldc = 0.f;
  if (!BWD) {  // the pair's log|det J| = Glow's - sum s, in sum_vec_kernel's order; every wave forms the same value
    float acc = 0.f;
    for (int c0 = 0; c0 < dim; c0 += 64) {  // (uniform trip count, clamped load and select: a dead lane adds +0)
      const float v = ga.s[min(c0 + lane, dim - 1)];
      acc += c0 + lane < dim ? v : 0.f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    const float ldg = *(ga.ld_glow ? ga.ld_glow : ga.s);  // (a selected pointer, not a load under a branch)
    const float ld = (ga.ld_glow ? ldg : 0.f) + -__shfl(acc, 0, 64);
    if (blockIdx.x == 0 && threadIdx.x == 0) ga.ld_out[0] = ld;
    ldc = ld - (float)dim * kHalfLog2Pi;
  }
  f32x4 acc[8];
  bool staged = false;
  for (int64_t base = (int64_t)blockIdx.x * nw; base < n_tiles; base += (int64_t)a.grid * nw) {
    const int64_t row = (base + wave) * 16 + j;
    const bool live = row < a.rows;
    const int64_t rowc = live ? row : a.rows - 1;
    const int64_t roff = rowc * dim;
    const float* xr = a.x + roff;
    float* yr = a.y + roff;
    const float rin = *(lp ? ga.row_in + rowc : ga.s);
    float sq = 0.f;
    for (int s = -1, g = 0, c = 0; s < steps; ++s) {
      if (a.resident ? !staged : s + 1 < steps) {
        lin_rt_stage(a, s + 1, nkc, mbuf + (a.resident ? 0 : ((s + 1) & 1) * buf_floats), lane, wave, nw);
        staged = true;
        if (a.resident) lin_rt_barrier();
      }
      if (s >= 0) {
        const int nt = min(8, ntile - 8 * g);
        if (c == 0) {
#pragma unroll
          for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* buf = mbuf + (a.resident ? g * kLinRtGroupCols : (s & 1) * buf_floats) + j;
        const int k0 = c * a.krows, kend = min(a.krows, dim - k0);
        for (int kb = 0; kb < kend; kb += 16) {
          float xv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + kb + 4 * u + q, kc = min(k, dim - 1);
            float v = xr[kc];
            if (BWD) v = (lp ? -v * rin : v) * el[kc];
            xv[u] = k < dim ? v : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (kb + 4 * u >= kend) break;
            const float* ap = buf + (kb + 4 * u + q) * ldw;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              if (t >= nt) break;
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[16 * t], xv[u], acc[t], 0, 0, 0);
            }
          }
        }
        if (++c == nkc) {
          const int lim = live && a.y ? dim : 0;  // (nothing of a row past `rows` is stored)
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            if (t >= nt) break;
            const int col = g * kLinRtGroupCols + 16 * t + 4 * q;
            f32x4 o = acc[t];
            if (!BWD) {
              const f32x4 tv = *reinterpret_cast<const f32x4*>(tl + col), ev = *reinterpret_cast<const f32x4*>(el + col);
#pragma unroll
              for (int r = 0; r < 4; ++r) o[r] = (o[r] - tv[r]) * ev[r];
              sq += (o[0] * o[0] + o[1] * o[1]) + (o[2] * o[2] + o[3] * o[3]);
            }
            if (a.vec) {
              if (col < lim) *reinterpret_cast<f32x4*>(yr + col) = o;
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (col + r < lim) yr[col + r] = o[r];
            }
          }
          c = 0, ++g;
        }
      }
      if (!a.resident) lin_rt_barrier();
    }
    if (!BWD && lp) {
      sq = sum_over_q(sq);
      if (live && q == 0) ga.lp_out[row] = rin + (ldc - 0.5f * sq);
    }
  }
}

__global__ void __launch_bounds__(512) glow_actnorm_inv_rt_kernel(GaRtArgs ga) {
  extern __shared__ __attribute__((aligned(16))) float ga_rt_lds[];
  ga_rt_rows<false>(ga, ga_rt_lds);
}

__global__ void __launch_bounds__(512) glow_actnorm_inv_bwd_rt_kernel(GaRtArgs ga) {
  extern __shared__ __attribute__((aligned(16))) float ga_rt_lds[];
  ga_rt_rows<true>(ga, ga_rt_lds);
}

// lin_rt_plan with the 2 x 1024 staged floats in front of M: resident up to dim 184, streamed above
static bool ga_rt_plan(int dim, LinRtPlan& p) {
  if (!lin_rt_plan(dim, p)) return false;
  const size_t post = (size_t)kGaRtPostFloats * 4;
  if (p.resident && p.lds + post > 160 * 1024) {
    p.resident = 0, p.krows = kLinRtChunkK, p.ldw = kLinRtGroupCols + 16, p.ncols = kLinRtGroupCols;
    p.lds = (size_t)2 * p.krows * p.ldw * 4;
  }
  p.lds += post;
  p.nw = p.resident && p.lds <= 80 * 1024 ? 4 : 8;
  return true;
}

// glow_actnorm_sums_rt_kernel.  xtg_rt_kernel's scheme -- a wave owns one (64 x 64 block of grad_m, row slice) pair and is
// the only writer of its sums -- with the backward prologue on the g operand, grad_m = u^T (grad_z e^-s).  The waves of
// the first block row (blockIdx.y == 0: together they see every column once per slice) also keep the column sums -- lane
// (c, k) adds rows k, k + 4, ... in order, the four k lanes are added in a fixed order -- and store
//   grad_s part = -sum_r grad_z z - [slice 0: grad_ld] - [log-prob form: sum_r grad_log_prob over the slice's rows]
//   grad_t part = -sum_r grad_z e^-s          grad_ld_glow part = sum_r grad_log_prob (log-prob form)
// behind the slice's dim x dim block: a slice is [grad_m | grad_s | grad_t | grad_ld_glow], ga_rt_slice_floats long, and
// det_reduce_async adds the slices in order.  The second load of a row (z for grad_s) goes to the address of the first
// where the wave has no use for it: issued by every wave, a cache hit there.
struct GaRtSumArgs {
  const float* u;
  const float* g;   // grad_z, or z in the log-prob form
  const float* z;
  const float* glp;  // grad_log_prob (log-prob form), else NULL
  const float* s;
  const float* grad_ld;
  float* part;
  int64_t rows, per, slice_floats;
  int dim, slices;
};
// (a slice's 0..3 padding floats are never written: the first step of a two-step reduction adds them into the partial
// sums' own padding, which nothing reads)
__host__ __device__ inline int64_t ga_rt_slice_floats(int dim) { return ((int64_t)dim * dim + 2 * dim + 1 + 3) / 4 * 4; }

__global__ void __launch_bounds__(256) glow_actnorm_sums_rt_kernel(GaRtSumArgs a) {
  const int lane = threadIdx.x & 63, c = lane & 15, k = lane >> 4, dim = a.dim;
  const int slice = (int)blockIdx.z * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slice >= a.slices) return;
  const int i0 = (int)blockIdx.y * 64, j0 = (int)blockIdx.x * 64;
  const int nti = min(4, (dim - i0 + 15) >> 4), ntj = min(4, (dim - j0 + 15) >> 4);
  const bool lp = a.glp != nullptr, sums = blockIdx.y == 0;
  const float* zsrc = sums ? a.z : a.g;
  int xo[4], go[4];
  float es[4], cs[4], ct[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    xo[t] = i0 + 16 * t + c < dim ? i0 + 16 * t + c : -1;
    go[t] = j0 + 16 * t + c < dim ? j0 + 16 * t + c : -1;
    es[t] = expf(-a.s[max(go[t], 0)]);
    cs[t] = ct[t] = 0.f;
  }
  float gsum = 0.f;
  f32x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t r0 = (int64_t)slice * a.per, r1 = min(a.rows, r0 + a.per);
  constexpr int U = 2;  // 4-row groups in flight per trip
  for (int64_t rb = r0; rb < r1; rb += 4 * U) {
    float xa[U][4], ga[U][4], gz[U][4], za[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = rb + 4 * u + k;
      const bool live = row < r1;
      const int64_t rowc = live ? row : r0, off = rowc * dim;
      const float rg = *(lp ? a.glp + rowc : a.s);
      gsum += live ? rg : 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        xa[u][t] = ga[u][t] = gz[u][t] = za[u][t] = 0.f;
        if (t < nti) {
          const float v = a.u[off + max(xo[t], 0)];
          xa[u][t] = live && xo[t] >= 0 ? v : 0.f;
        }
        if (t < ntj) {
          const float v = a.g[off + max(go[t], 0)], zv = zsrc[off + max(go[t], 0)];
          const bool ok = live && go[t] >= 0;
          gz[u][t] = ok ? (lp ? -v * rg : v) : 0.f;
          za[u][t] = ok ? zv : 0.f;
          ga[u][t] = gz[u][t] * es[t];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        cs[t] -= gz[u][t] * za[u][t];
        ct[t] -= ga[u][t];
      }
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        if (ti >= nti) break;
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
          if (tj >= ntj) break;
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u][ti], ga[u][tj], acc[ti][tj], 0, 0, 0);
        }
      }
    }
  }
  // (only grad_m's dim rows are stored: the column sums sit right behind them)
  float* out = a.part + (int64_t)slice * a.slice_floats;
  const uint32_t o0 = (uint32_t)((i0 + 4 * k) * dim + j0 + c);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    if (tj >= ntj) break;
    if (j0 + 16 * tj + c < dim) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        if (ti >= nti) break;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (i0 + 4 * k + 16 * ti + r < dim) out[o0 + (uint32_t)((16 * ti + r) * dim + 16 * tj)] = acc[ti][tj][r];
      }
    }
  }
  if (!sums) return;
  gsum = sum_over_q(gsum);
  const float gld = *(a.grad_ld ? a.grad_ld : a.s);  // (a selected pointer, not a load under a branch)
  const float off_s = (slice == 0 && a.grad_ld ? gld : 0.f) + (lp ? gsum : 0.f);
  float* out_s = out + (int64_t)dim * dim;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float vs = sum_over_q(cs[t]), vt = sum_over_q(ct[t]);
    if (k == 0 && go[t] >= 0) {
      out_s[go[t]] = vs - off_s;
      out_s[dim + go[t]] = vt;
    }
  }
  if (blockIdx.x == 0 && lane == 0) out_s[2 * dim] = lp ? gsum : 0.f;
}

}  // namespace mnf

extern "C" {

int64_t mnf_linear_rows_image_floats(int dim) {
  return (dim == 16 || dim == 32 || dim == 64 || dim == 128) ? (int64_t)dim * dim : 0;
}

int mnf_linear_rows_image_index(int dim, int32_t* idx_host) {
  if (!idx_host) return MNF_ERR_INVALID_ARG;
  switch (dim) {
    case 16: mnf::build_index<16>(idx_host); return MNF_OK;
    case 32: mnf::build_index<32>(idx_host); return MNF_OK;
    case 64: mnf::build_index<64>(idx_host); return MNF_OK;
    case 128: mnf::build_index<128>(idx_host); return MNF_OK;
  }
  return MNF_ERR_UNSUPPORTED;
}

int mnf_linear_rows_img(const float* x, const float* image, float* y, int64_t rows, int dim, void* stream) {
  if (!x || !image || !y || x == y || rows < 0) return MNF_ERR_INVALID_ARG;
  if (rows == 0) return MNF_OK;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(image)) & 15)
    return MNF_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  switch (dim) {
    case 16: return mnf::launch<16>(x, image, y, rows, st);
    case 32: return mnf::launch<32>(x, image, y, rows, st);
    case 64: return mnf::launch<64>(x, image, y, rows, st);
    case 128: return mnf::launch<128>(x, image, y, rows, st);
  }
  return MNF_ERR_UNSUPPORTED;
}

int mnf_linear_rows_rt_supported(int dim) {
  mnf::LinRtPlan p;
  return mnf::lin_rt_plan(dim, p) ? 1 : 0;
}

int mnf_linear_rows_rt(const float* x, const float* M, float* y, int64_t rows, int dim, int trans, void* stream) {
  if (!x || !M || !y || x == y || rows < 0) return MNF_ERR_INVALID_ARG;
  mnf::LinRtPlan p;
  if (!mnf::lin_rt_plan(dim, p)) return MNF_ERR_UNSUPPORTED;
  if (rows == 0) return MNF_OK;
  static mnf::DeviceMemo big_lds;
  mnf::allow_big_lds(big_lds, mnf::linear_rows_rt_kernel);
  const int vec = dim % 4 == 0 && mnf::aligned16(x, y);
  const int grid = (int)mnf::persistent_grid(mnf::linear_rows_rt_kernel, p.nw, p.lds, 16 * p.nw, rows);
  const mnf::LinRtArgs a{x, M, y, rows, dim, trans != 0, vec, p.resident, p.krows, p.ldw, p.ncols, p.ngroups, p.nw, grid};
  mnf::tag_kernel("linear_rows_rt");
  hipLaunchKernelGGL(mnf::linear_rows_rt_kernel, dim3((unsigned)grid), dim3(p.nw * 64), p.lds, (hipStream_t)stream, a);
  return mnf::check_launch();
}

int64_t mnf_linear_rows_bwd_weight_rt_workspace(int64_t rows, int dim) {
  if (rows < 1 || !mnf_linear_rows_rt_supported(dim) || !mnf::gfx950_visible()) return 0;
  return mnf::xtg_rt_plan(rows, dim, mnf::device_cus(mnf::current_device())).floats;
}

int mnf_linear_rows_bwd_weight_rt(const float* x, const float* grad_y, float* grad_W, int64_t rows, int dim,
                                  float* workspace, int64_t workspace_floats, void* stream) {
  if (!x || !grad_y || !grad_W || rows < 0 || (rows > 0 && !workspace)) return MNF_ERR_INVALID_ARG;
  if (!mnf_linear_rows_rt_supported(dim)) return MNF_ERR_UNSUPPORTED;
  if (rows == 0) return MNF_OK;
  const mnf::XtgRtPlan p = mnf::xtg_rt_plan(rows, dim, mnf::device_cus(mnf::current_device()));
  if (workspace_floats < p.floats) return MNF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nbj = (unsigned)(dim + 63) / 64;
  const int64_t sf = mnf::xtg_rt_slice_floats(dim), n = (int64_t)dim * dim;
  const mnf::XtgRtArgs a{x, grad_y, workspace, rows, p.per, dim, p.slices};
  mnf::tag_kernel("linear_rows_bwd_weight_rt");
  hipLaunchKernelGGL(mnf::xtg_rt_kernel, dim3(nbj, nbj, (unsigned)(p.slices + 3) / 4), dim3(256), 0, st, a);
  if (int rc = mnf::check_launch()) return rc;
  if (!p.groups) return mnf::det_reduce_async(workspace, p.slices, sf, n, grad_W, st);
  float* sums = workspace + p.slices * sf;
  if (int rc = mnf::zero_floats_async(sums, p.groups * sf, st)) return rc;
  if (int rc = mnf::det_reduce_async(workspace, p.slices / p.groups, p.groups * sf, p.groups * sf, sums, st)) return rc;
  return mnf::det_reduce_async(sums, p.groups, sf, n, grad_W, st);
}

int mnf_glow_actnorm_inv_rt_supported(int dim) {
  mnf::LinRtPlan p;
  return mnf::ga_rt_plan(dim, p) ? 1 : 0;
}

int mnf_glow_actnorm_inv_rt(const float* u, const float* M, const float* s, const float* t, float* z, const float* ld_glow,
                            float* ld_out, const float* log_det_rows, float* log_prob, int64_t rows, int dim,
                            void* stream) {
  const bool lp = log_prob != nullptr;
  if (!u || !M || !s || !t || !ld_out || (log_det_rows != nullptr) != lp || (!z && !lp) || u == z || rows < 0)
    return MNF_ERR_INVALID_ARG;
  mnf::LinRtPlan p;
  if (!mnf::ga_rt_plan(dim, p)) return MNF_ERR_UNSUPPORTED;
  if (rows == 0) return MNF_OK;
  static mnf::DeviceMemo big_lds;
  mnf::allow_big_lds(big_lds, mnf::glow_actnorm_inv_rt_kernel);
  const int vec = dim % 4 == 0 && mnf::aligned16(u, z);
  const int grid = (int)mnf::persistent_grid(mnf::glow_actnorm_inv_rt_kernel, p.nw, p.lds, 16 * p.nw, rows);
  const mnf::GaRtArgs a{{u, M, z, rows, dim, 0, vec, p.resident, p.krows, p.ldw, p.ncols, p.ngroups, p.nw, grid},
                        s, t, ld_glow, log_det_rows, ld_out, log_prob};
  mnf::tag_kernel("glow_actnorm_inv_rt");
  hipLaunchKernelGGL(mnf::glow_actnorm_inv_rt_kernel, dim3((unsigned)grid), dim3(p.nw * 64), p.lds, (hipStream_t)stream, a);
  return mnf::check_launch();
}

int64_t mnf_glow_actnorm_inv_bwd_rt_workspace(int64_t rows, int dim) {
  if (rows < 1 || !mnf_glow_actnorm_inv_rt_supported(dim) || !mnf::gfx950_visible()) return 0;
  // (xtg_rt_plan caps the slice count by ITS slice size; where dim is a multiple of 16 a slice here is 2 dim + 4 floats
  //  longer, so the workspace may pass the plan's 32 MB by that much per slice: 8 x 2,052 floats at dim 1024)
  const mnf::XtgRtPlan p = mnf::xtg_rt_plan(rows, dim, mnf::device_cus(mnf::current_device()));
  return (int64_t)(p.slices + p.groups) * mnf::ga_rt_slice_floats(dim);
}

int mnf_glow_actnorm_inv_bwd_rt(const float* u, const float* z, const float* grad_z, const float* grad_log_prob,
                                const float* M, const float* s, const float* t, float* grad_u, float* grad_m, float* grad_s,
                                float* grad_t, const float* grad_ld, float* grad_ld_glow, int64_t rows, int dim,
                                float* workspace, int64_t workspace_floats, void* stream) {
  const bool lp = grad_log_prob != nullptr;
  if (!u || !z || !M || !s || !t || !grad_u || !grad_m || (grad_z != nullptr) == lp || u == grad_u || z == grad_u ||
      grad_z == grad_u || rows < 0 || (rows > 0 && !workspace))
    return MNF_ERR_INVALID_ARG;
  mnf::LinRtPlan lin;
  if (!mnf::ga_rt_plan(dim, lin)) return MNF_ERR_UNSUPPORTED;
  if (rows == 0) return MNF_OK;
  const mnf::XtgRtPlan p = mnf::xtg_rt_plan(rows, dim, mnf::device_cus(mnf::current_device()));
  const int64_t sf = mnf::ga_rt_slice_floats(dim), n = (int64_t)dim * dim;
  if (workspace_floats < (p.slices + p.groups) * sf) return MNF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  // grad_u = (grad_z e^-s) @ M^T
  static mnf::DeviceMemo big_lds;
  mnf::allow_big_lds(big_lds, mnf::glow_actnorm_inv_bwd_rt_kernel);
  const float* g = lp ? z : grad_z;
  const int vec = dim % 4 == 0 && mnf::aligned16(g, grad_u);
  const int grid = (int)mnf::persistent_grid(mnf::glow_actnorm_inv_bwd_rt_kernel, lin.nw, lin.lds, 16 * lin.nw, rows);
  const mnf::GaRtArgs a{{g, M, grad_u, rows, dim, 1, vec, lin.resident, lin.krows, lin.ldw, lin.ncols, lin.ngroups, lin.nw, grid},
                        s, t, nullptr, grad_log_prob, nullptr, nullptr};
  mnf::tag_kernel("glow_actnorm_inv_bwd_rt");
  hipLaunchKernelGGL(mnf::glow_actnorm_inv_bwd_rt_kernel, dim3((unsigned)grid), dim3(lin.nw * 64), lin.lds, st, a);
  if (int rc = mnf::check_launch()) return rc;
  // the sums: one writer per (slice, entry), then the slices in order
  const unsigned nbj = (unsigned)(dim + 63) / 64;
  const mnf::GaRtSumArgs sa{u, g, z, grad_log_prob, s, grad_ld, workspace, rows, p.per, sf, dim, p.slices};
  hipLaunchKernelGGL(mnf::glow_actnorm_sums_rt_kernel, dim3(nbj, nbj, (unsigned)(p.slices + 3) / 4), dim3(256), 0, st, sa);
  if (int rc = mnf::check_launch()) return rc;
  const float* part = workspace;
  int n_part = p.slices;
  if (p.groups) {
    float* sums = workspace + p.slices * sf;
    if (int rc = mnf::zero_floats_async(sums, p.groups * sf, st)) return rc;
    if (int rc = mnf::det_reduce_async(workspace, p.slices / p.groups, p.groups * sf, p.groups * sf, sums, st)) return rc;
    part = sums, n_part = p.groups;
  }
  float* gl = lp ? grad_ld_glow : nullptr;
  // (a caller that keeps [grad_m | grad_s | grad_t | grad_ld_glow] back to back, as a slice does, gets them in one launch)
  if (grad_s == grad_m + n && grad_t == grad_s + dim && (!lp || gl == grad_t + dim))
    return mnf::det_reduce_async(part, n_part, sf, n + 2 * dim + (lp ? 1 : 0), grad_m, st);
  if (int rc = mnf::det_reduce_async(part, n_part, sf, n, grad_m, st)) return rc;
  if (grad_s)
    if (int rc = mnf::det_reduce_async(part + n, n_part, sf, dim, grad_s, st)) return rc;
  if (grad_t)
    if (int rc = mnf::det_reduce_async(part + n + dim, n_part, sf, dim, grad_t, st)) return rc;
  return gl ? mnf::det_reduce_async(part + n + 2 * dim, n_part, sf, 1, gl, st) : MNF_OK;
}

}  // extern "C"
