// y = x @ W for Glow's d x d matrix on the fp32 matrix cores: per-shape kernels (d in {16, 32, 64, 128}) and, below
// them, the run-time-shaped pair for any d up to 1024 (forward / grad_x and the weight gradient).
//
// Same transposed scheme as the coupling kernels: one wave owns 16 rows; lane (j, q) loads the
// row as float4s (element 16 g + 4 q + e is the k = q operand of K-step 4 g + e); output tile m
// leaves dims 16 m + 4 q + r in register r of lane (j, q), i.e. a float4 of the output row.
// W is pre-arranged into A-operand order (image) and copied to LDS once per workgroup.
// HBM-bound: 8 d bytes per row, 2 d^2 flops per row (d = 32: 8 flop/B).
#include <hip/hip_runtime.h>

#include "mnf_device.h"
#include "mnf_host.h"

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

}  // extern "C"
