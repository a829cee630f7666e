// The two gradients of MNFConv2d.forward's fused node (mnf_mnf_conv_fwd.hip; layers._MnfConvFwdFn.backward) on the exact-fp32
// matrix instruction (v_mfma_f32_16x16x4_f32), for contiguous NCHW float32, stride 1, no padding, one group.  g is the output
// cotangent (B, n_out, OH, OW), gv the variance's (mnf_mnf_noise_bwd's result), K = n_in k^2, K' = n_out k^2.
//
// mnf_mnf_conv_bwd_weight -- one pass over x for both weight matrices and the bias:
//   grad_Wz[co, j]    = sum_p g [p, co] x[patch(p, j)]          j = (ci, ky, kx), p over all B OH OW output pixels
//   grad_W_var[co, j] = sum_p gv[p, co] x[patch(p, j)]^2        (the square is taken in registers)
//   grad_b_var[co]    = sum_p gv[p, co]                         (column K of the second product: x := 1)
//   An implicit GEMM that reduces over pixels: output channels are the instruction's rows, 16 weight positions its columns,
//   4 pixels go per step.  A workgroup is ONE wave: it owns CT = 4 column tiles (64 weight positions, every channel tile,
//   both products: 128 accumulator registers; tiles past column K are skipped) and one slice of the pixels, which it adds in pixel order.  A lane's columns
//   never change, so its CT patch offsets are computed once and stay in registers (no LDS table: there is nothing to share).
//   The loads of the next 16 pixels are issued before the products of the current 16.  A pixel past the slice's end reads the
//   last pixel's (legal) addresses and its operands are SELECTED to zero.  The partial block goes to the slice's slot of the
//   caller's workspace with plain stores -- laid out [grad_Wz | grad_W_var | grad_b_var] like the outputs -- and
//   det_reduce_async adds the slots in slice order (more than 32 slices: in two steps, every `groups`-th slice first): no
//   atomics, a call repeats bit for bit.  An empty slice stores zeros.  The slice count depends on the shape alone
//   (conv_bwd_weight_plan).
//
// mnf_mnf_conv_bwd_input -- the forward kernel with the roles swapped:
//   grad_x[n, ci, y, x] = sum_{co,ky,kx} g [n, co, y - ky, x - kx] Wz[co, ci, ky, kx]
//                       + 2 x[n, ci, y, x] sum_{co,ky,kx} gv[n, co, y - ky, x - kx] W_var[co, ci, ky, kx]
//   Input channels are the rows (n_in <= 64), 16 consecutive input pixels of the flattened (n, y, x) index the columns, the
//   reduction index is k' = (co, ky, kx).  The LDS table holds (offset, ky | kx << 8) per k'; a term whose (y - ky, x - kx)
//   falls outside the output image -- and every padding k' -- reads element 0 and is SELECTED to zero (never multiplied by a
//   mask: 0 * NaN).  Both transposed weight matrices go through LDS interleaved, in chunks, exactly as the forward's; the
//   gathers run four K-steps ahead of the products; the epilogue acc1 + 2 x acc2 is in the kernel.  No workspace, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mnf_hip.h"
#include "mnf_host.h"

namespace mnf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace convb {
constexpr int MT = 4;        // channel tiles (rows <= 64)
constexpr int U = 4;         // K-steps whose loads are issued together
constexpr int KMAX = 4096;   // n_in k^2 and n_out k^2
// weight gradients
constexpr int CT = 4;                                   // column tiles per wave
constexpr int64_t WS_MAX_FLOATS = (int64_t)8 << 20;     // the workspace's cap: 32 MB (mnf_linear_mfma.hip's)
constexpr int TARGET_WAVES = 2048;                      // column blocks x slices aims here (two waves per SIMD of 256 CUs)
constexpr int TWO_STAGE_SLICES = 32;                    // more slices than this are added up in two steps
constexpr int MIN_SLICE_PIXELS = 256;                   // a slice shorter than this is not worth its slot
// input gradient
constexpr int P = 2;         // pixel tiles per wave
constexpr int KC = 64;       // k' per weight chunk
constexpr int WAVES = 4;     // per workgroup
constexpr int GROUP = 16 * P * WAVES;
}  // namespace convb

// n / d for 0 <= n < 2^31 as a multiply and a shift (the divisor is a launch constant): the pixel index is taken apart
// eight times per 16 pixels in the weight kernel, next to 64 matrix instructions
struct FastDiv {
  unsigned d, mul, shr;
  __device__ __forceinline__ int div(int n) const { return d == 1 ? n : (int)(__umulhi((unsigned)n, mul) >> shr); }
};
static FastDiv fast_div(int d) {
  FastDiv f{(unsigned)d, 0u, 0u};
  if (d > 1) {
    int l = 0;  // ceil(log2(d))
    while (((int64_t)1 << l) < d) ++l;
    f.mul = (unsigned)((((uint64_t)1 << (31 + l)) + (unsigned)d - 1) / (unsigned)d);
    f.shr = (unsigned)(l - 1);
  }
  return f;
}

// ---------------------------------------------------------------------------------------------------- weight gradients
struct ConvBwdWArgs {
  const float* x;
  const float* g;
  const float* gv;
  float* ws;
  int n_in, height, width, n_out, ksize;
  int K;           // n_in k^2
  int ohw, ow;     // output pixels per image, per row
  FastDiv by_ohw, by_ow;
  int n_pixels;    // batch * ohw
  int per_slice;   // pixels per slice, a multiple of 16
  int64_t slot;    // floats per slice: 2 n_out K + n_out
};

__global__ void __launch_bounds__(64) conv_bwd_weight_kernel(const ConvBwdWArgs a) {
  using namespace convb;
  const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
  const int mt = (a.n_out + 15) >> 4;
  const int hw = a.height * a.width, kk2 = a.ksize * a.ksize;
  int off[CT];
  bool one[CT];  // the bias column
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int col = (blockIdx.x * CT + t) * 16 + c;
    int o = 0;
    if (col < a.K) {
      const int ci = col / kk2, r = col - ci * kk2, ky = r / a.ksize;
      o = ci * hw + ky * a.width + (r - ky * a.ksize);
    }
    off[t] = o, one[t] = col == a.K;
  }
  const int tiles_left = (a.K + 16) / 16 - blockIdx.x * CT;  // of the K + 1 columns
  const int nt = tiles_left < CT ? tiles_left : CT;
  int coff[MT];   // this lane's channel of each tile, inside an output image (clamped), and whether it exists
  bool has[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int co = 16 * m + c;
    has[m] = co < a.n_out, coff[m] = (has[m] ? co : a.n_out - 1) * a.ohw;  // < 64 * ohw: 32-bit
  }
  int begin = blockIdx.y * a.per_slice;  // (n_slices * per_slice < 2^31: the entry checks)
  begin = begin < a.n_pixels ? begin : a.n_pixels;
  const int end = a.n_pixels - begin < a.per_slice ? a.n_pixels : begin + a.per_slice;

  // 16 pixels' operands: g / gv at (pixel p0 + 4 u + q, channel 16 m + c), x at (that pixel, this lane's columns)
  auto load = [&](int p0, float (&ag)[U][MT], float (&av)[U][MT], float (&xv)[U][CT]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + 4 * u + q;
      const bool ok = p < end;
      const int pc = ok ? p : a.n_pixels - 1;
      const int n = a.by_ohw.div(pc), rem = pc - n * a.ohw, oy = a.by_ow.div(rem);
      const float* xp = a.x + ((int64_t)n * a.n_in * hw + oy * a.width + (rem - oy * a.ow));
      const int64_t gb = (int64_t)n * a.n_out * a.ohw + rem;
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
          const int64_t at = gb + coff[m];
          const float v1 = a.g[at], v2 = a.gv[at];
          const bool use = ok && has[m];
          ag[u][m] = use ? v1 : 0.f, av[u][m] = use ? v2 : 0.f;
        }
#pragma unroll
      for (int t = 0; t < CT; ++t)
        if (t < nt) {
          const float v = xp[off[t]];
          xv[u][t] = ok ? (one[t] ? 1.f : v) : 0.f;
        }
    }
  };

  f32x4 sg[MT][CT], sv[MT][CT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < CT; ++t) sg[m][t] = f32x4{0.f, 0.f, 0.f, 0.f}, sv[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  float ng[U][MT] = {}, nv[U][MT] = {}, nx[U][CT] = {};
  if (begin < end) load(begin, ng, nv, nx);
#pragma unroll 1
  for (int p0 = begin; p0 < end; p0 += 16) {
    float cg[U][MT], cv[U][MT], cx[U][CT], cs[U][CT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int m = 0; m < MT; ++m) cg[u][m] = ng[u][m], cv[u][m] = nv[u][m];
#pragma unroll
      for (int t = 0; t < CT; ++t) cx[u][t] = nx[u][t], cs[u][t] = nx[u][t] * nx[u][t];
    }
    load(p0 + 16, ng, nv, nx);  // (past the end: the last pixel's addresses, unused)
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int t = 0; t < CT; ++t)
            if (t < nt) {
              sg[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cg[u][m], cx[u][t], sg[m][t], 0, 0, 0);
              sv[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv[u][m], cs[u][t], sv[m][t], 0, 0, 0);
            }
        }
  }

  float* slot = a.ws + (int64_t)blockIdx.y * a.slot;
  const int64_t nk = (int64_t)a.n_out * a.K;
#pragma unroll
  for (int m = 0; m < MT; ++m)
    if (m < mt) {
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const int col = (blockIdx.x * CT + t) * 16 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = 16 * m + 4 * q + r;
          if (co >= a.n_out) continue;
          if (col < a.K) {
            slot[(int64_t)co * a.K + col] = sg[m][t][r];
            slot[nk + (int64_t)co * a.K + col] = sv[m][t][r];
          } else if (col == a.K) {
            slot[2 * nk + co] = sv[m][t][r];
          }
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------------- input gradient
struct ConvBwdIArgs {
  const float* x;
  const float* g;
  const float* gv;
  const float* Wz;
  const float* W_var;
  float* grad_x;
  int n_in, height, width, n_out, ksize;
  int K;           // n_in k^2: a weight row
  int Kr, Krp;     // n_out k^2, and padded to a multiple of 4 U
  int oh, ow, ohw;
  int n_pixels;    // batch * height * width
  int pt;          // pixel tiles per wave in this launch: P, or 1 for few pixels
  int n_groups;
};

__global__ void __launch_bounds__(64 * convb::WAVES) conv_bwd_input_kernel(const ConvBwdIArgs a) {
  using namespace convb;
  __shared__ int2 s_tab[KMAX];  // (offset of g[co, -ky, -kx] from the pixel's own, ky | kx << 8; bit 16: padding)
  __shared__ float2 s_w[(KC / 4) * MT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int mt = (a.n_in + 15) >> 4;
  const int hw = a.height * a.width, kk2 = a.ksize * a.ksize;

  for (int k = tid; k < a.Krp; k += 64 * WAVES) {
    int2 e = make_int2(0, 1 << 16);
    if (k < a.Kr) {
      const int co = k / kk2, r = k - co * kk2, ky = r / a.ksize, kx = r - ky * a.ksize;
      e = make_int2(co * a.ohw - ky * a.ow - kx, ky | kx << 8);
    }
    s_tab[k] = e;
  }
  const int n_chunks = (a.Krp + KC - 1) / KC;

  // One chunk of both TRANSPOSED weight matrices, the forward kernel's staging: this thread's k' = k0 + (tid & 63) of the
  // input channels wave, wave + 4, ... (rows >= n_in and k' >= K': zeros), in A-operand order in LDS.
  constexpr int PRE = 16 * MT * KC / (64 * WAVES);
  float2 pre[PRE];
  const int kk = tid & (KC - 1);
  auto fetch = [&](int k0) {
    const int k = k0 + kk;
    const int co = k / kk2, r = k - co * kk2;
    int w0 = wave;  // opaque: the 16 addresses are formed here, not kept in registers across the persistent loop
    asm volatile("" : "+v"(w0));
#pragma unroll
    for (int j = 0; j < PRE; ++j)
      if (j < 4 * mt) {
        const int ci = w0 + WAVES * j;
        pre[j] = make_float2(0.f, 0.f);
        if (ci < a.n_in && k < a.Kr) {
          const int at = co * a.K + ci * kk2 + r;  // < 64 * 4096
          pre[j] = make_float2(a.Wz[at], a.W_var[at]);
        }
      }
  };
  auto put = [&]() {
#pragma unroll
    for (int j = 0; j < PRE; ++j)
      if (j < 4 * mt) {
        const int ci = wave + WAVES * j;
        s_w[((kk >> 2) * MT + (ci >> 4)) * 64 + (kk & 3) * 16 + (ci & 15)] = pre[j];
      }
  };
  fetch(0);
  if (n_chunks == 1) put();  // the only chunk stays resident
  __syncthreads();

  const int pt = a.pt;
  for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
    int q4 = 4 * q;  // opaque per pass, as in the forward kernel
    asm volatile("" : "+v"(q4));
    int64_t gb[P];   // of g[n, 0, y, x] (a virtual element where (y, x) is outside the output image)
    int64_t at0[P];  // of x[n, 0, y, x]
    int py[P], px[P];
    bool live[P];
#pragma unroll
    for (int t = 0; t < P; ++t) {
      int p = ((grp * WAVES + wave) * pt + t) * 16 + c;
      live[t] = t < pt && p < a.n_pixels;
      p = live[t] ? p : a.n_pixels - 1;
      const int n = p / hw, rem = p - n * hw;
      py[t] = rem / a.width, px[t] = rem - py[t] * a.width;
      gb[t] = (int64_t)n * a.n_out * a.ohw + py[t] * a.ow + px[t];
      at0[t] = (int64_t)n * a.n_in * hw + rem;
    }
    f32x4 a1[P][MT], a2[P][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < P; ++t) a1[t][m] = f32x4{0.f, 0.f, 0.f, 0.f}, a2[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};

    // The gathers of both cotangents run one group of U K-steps ahead of the products.  Every address is legal (an absent
    // term reads element 0), so no load is guarded; the value is selected where it is used.
    float gn[U][P] = {}, vn[U][P] = {};
    bool okn[U][P] = {};
    auto gather = [&](int kb) {
      int2 e[U];
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = s_tab[kb + 4 * u + q];
#pragma unroll
      for (int t = 0; t < P; ++t) {
        if (t >= pt) continue;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ky = e[u].y & 255, kx = (e[u].y >> 8) & 255;
          const bool ok = e[u].y < (1 << 16) && (unsigned)(py[t] - ky) < (unsigned)a.oh && (unsigned)(px[t] - kx) < (unsigned)a.ow;
          const int64_t at = ok ? gb[t] + e[u].x : 0;
          gn[u][t] = a.g[at], vn[u][t] = a.gv[at], okn[u][t] = ok;
        }
      }
    };
    gather(0);
    auto products = [&](auto nt, int g0, const float (&v1)[U][P], const float (&v2)[U][P]) {
      constexpr int NT = decltype(nt)::value;
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float2 w = s_w[((g0 + u) * MT + m) * 64 + lane];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              a1[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, v1[u][t], a1[t][m], 0, 0, 0);
              a2[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, v2[u][t], a2[t][m], 0, 0, 0);
            }
          }
        }
    };

    for (int ch = 0; ch < n_chunks; ++ch) {
      const int k0 = ch * KC;
      if (n_chunks > 1) {
        __syncthreads();  // the previous chunk's readers are done
        put();
        __syncthreads();
        fetch(ch + 1 == n_chunks ? 0 : k0 + KC);  // (the last chunk fetches the next pass's first)
      }
      const int steps = ((a.Krp - k0 < KC ? a.Krp - k0 : KC)) >> 2;  // a multiple of U
#pragma unroll 1
      for (int g0 = 0; g0 < steps; g0 += U) {
        float v1[U][P], v2[U][P];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int t = 0; t < P; ++t) v1[u][t] = okn[u][t] ? gn[u][t] : 0.f, v2[u][t] = okn[u][t] ? vn[u][t] : 0.f;
        const int kb = k0 + 4 * (g0 + U);
        gather(kb < a.Krp ? kb : a.Krp - 4 * U);  // (past the end: the last group again, unused)
        if (pt > 1)
          products(std::integral_constant<int, P>{}, g0, v1, v2);
        else
          products(std::integral_constant<int, 1>{}, g0, v1, v2);
      }
    }

#pragma unroll
    for (int t = 0; t < P; ++t) {
      if (t >= pt) continue;
      // x at the tile's elements first, all loads in flight at once, from clamped addresses; the stores are per-lane selects
      float xi[MT][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ci = 16 * m + q4 + r;
            xi[m][r] = a.x[at0[t] + (int64_t)(ci < a.n_in ? ci : a.n_in - 1) * hw];
          }
        }
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ci = 16 * m + q4 + r;
            const float o = fmaf(2.f * xi[m][r], a2[t][m][r], a1[t][m][r]);
            if (live[t] && ci < a.n_in) a.grad_x[at0[t] + (int64_t)ci * hw] = o;
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host
// the forward's envelope (mnf_mnf_conv_fwd_supported)
static bool conv_bwd_shape_ok(int n_in, int n_out, int ksize, int height, int width) {
  if (n_in < 1 || n_out < 1 || n_out > 64 || ksize < 1 || height < ksize || width < ksize) return false;
  if ((int64_t)n_in * ksize * ksize > convb::KMAX) return false;
  return (int64_t)(n_in > 64 ? n_in : 64) * height * width < ((int64_t)1 << 31);
}
static bool conv_bwd_input_shape_ok(int n_in, int n_out, int ksize, int height, int width) {
  return conv_bwd_shape_ok(n_in, n_out, ksize, height, width) && n_in <= 64 &&
         (int64_t)n_out * ksize * ksize <= convb::KMAX;
}
// batch * per_image as a 32-bit pixel count with room for the kernels' look-ahead, or 0 (compared by division: the product
// itself may not fit 64 bits)
static int64_t conv_bwd_pixels(int64_t batch, int64_t per_image) {
  const int64_t max_pixels = ((int64_t)1 << 31) - (1 << 16);
  return batch < 1 || batch > max_pixels / per_image ? 0 : batch * per_image;
}

// The weight launch's split, from the shape alone: column blocks of CT tiles over the K + 1 columns, and as many pixel
// slices as bring the grid to TARGET_WAVES waves -- at least 2, none shorter than MIN_SLICE_PIXELS pixels unless that
// leaves fewer than 2, and no more than the workspace cap holds.
struct ConvBwdWPlan {
  int col_blocks, slices, per_slice;
  int groups;      // 0: the slots are added in one step; else slices = groups * (slices / groups), added in two
  int64_t slot;
  int64_t floats() const { return (slices + groups) * slot; }
};
static ConvBwdWPlan conv_bwd_weight_plan(int64_t n_pixels, int n_in, int n_out, int ksize) {
  using namespace convb;
  ConvBwdWPlan p;
  const int K = n_in * ksize * ksize;
  p.col_blocks = ((K + 1 + 15) / 16 + CT - 1) / CT;
  p.slot = 2 * (int64_t)n_out * K + n_out;
  int64_t s = TARGET_WAVES / p.col_blocks;
  const int64_t by_pixels = (n_pixels + MIN_SLICE_PIXELS - 1) / MIN_SLICE_PIXELS;
  s = s < by_pixels ? s : by_pixels;
  s = s < 2 ? 2 : s;
  const int64_t cap = WS_MAX_FLOATS / p.slot;  // >= 15: a slot is at most 2 * 64 * 4096 + 64 floats
  s = s < cap ? s : cap;
  // det_reduce_async walks its rows one by one: many slices are added as `groups` interleaved sums of r slices each (slice
  // j, j + groups, ... in order), which are then added in order -- r ~ sqrt(slices), the sums behind the slots
  p.groups = 0;
  if (s > TWO_STAGE_SLICES) {
    int64_t r = 1;
    while (r * r < s) ++r;
    int64_t g = s / r;
    while (g * r + g > cap) --g;
    p.groups = (int)g, s = g * r;
  }
  p.slices = (int)s;
  p.per_slice = (int)(((n_pixels + s - 1) / s + 15) / 16 * 16);
  return p;
}

}  // namespace mnf

using namespace mnf;

extern "C" {

int mnf_mnf_conv_bwd_weight_supported(int n_in, int n_out, int kernel_size, int height, int width) {
  return conv_bwd_shape_ok(n_in, n_out, kernel_size, height, width) ? 1 : 0;
}

int mnf_mnf_conv_bwd_input_supported(int n_in, int n_out, int kernel_size, int height, int width) {
  return conv_bwd_input_shape_ok(n_in, n_out, kernel_size, height, width) ? 1 : 0;
}

int64_t mnf_mnf_conv_bwd_weight_workspace(int64_t batch, int n_in, int n_out, int kernel_size, int height, int width) {
  if (!conv_bwd_shape_ok(n_in, n_out, kernel_size, height, width)) return 0;
  const int64_t n_pixels = conv_bwd_pixels(batch, (int64_t)(height - kernel_size + 1) * (width - kernel_size + 1));
  if (!n_pixels) return 0;
  return conv_bwd_weight_plan(n_pixels, n_in, n_out, kernel_size).floats();
}

int mnf_mnf_conv_bwd_weight(const float* x, const float* grad_out, const float* grad_var, float* grad_Wz, float* grad_W_var,
                            float* grad_b_var, float* workspace, int64_t workspace_floats, int64_t batch, int n_in,
                            int height, int width, int n_out, int kernel_size, void* stream) {
  if (!x || !grad_out || !grad_var || !grad_Wz || !grad_W_var || !grad_b_var || !workspace || batch < 1 || n_in < 1 ||
      height < 1 || width < 1 || n_out < 1 || kernel_size < 1)
    return MNF_ERR_INVALID_ARG;
  if (!conv_bwd_shape_ok(n_in, n_out, kernel_size, height, width)) return MNF_ERR_UNSUPPORTED;
  const int oh = height - kernel_size + 1, ow = width - kernel_size + 1;
  const int64_t n_pixels = conv_bwd_pixels(batch, (int64_t)oh * ow);
  if (!n_pixels) return MNF_ERR_UNSUPPORTED;
  const ConvBwdWPlan p = conv_bwd_weight_plan(n_pixels, n_in, n_out, kernel_size);
  if (workspace_floats < p.floats()) return MNF_ERR_INVALID_ARG;
  const hipStream_t st = (hipStream_t)stream;
  ConvBwdWArgs a;
  a.x = x, a.g = grad_out, a.gv = grad_var, a.ws = workspace;
  a.n_in = n_in, a.height = height, a.width = width, a.n_out = n_out, a.ksize = kernel_size;
  a.K = n_in * kernel_size * kernel_size;
  a.ohw = oh * ow, a.ow = ow, a.by_ohw = fast_div(a.ohw), a.by_ow = fast_div(ow);
  a.n_pixels = (int)n_pixels, a.per_slice = p.per_slice, a.slot = p.slot;
  const int64_t nk = (int64_t)n_out * a.K;
  // the outputs are overwritten: zeroed (a kernel node), then the slots are added in slice order.  Outputs that lie one
  // behind the other like a slot take one launch each instead of three
  const bool packed = grad_W_var == grad_Wz + nk && grad_b_var == grad_W_var + nk;
  if (packed) {
    if (int rc = zero_floats_async(grad_Wz, p.slot, st)) return rc;
  } else {
    if (int rc = zero_floats_async(grad_Wz, nk, st)) return rc;
    if (int rc = zero_floats_async(grad_W_var, nk, st)) return rc;
    if (int rc = zero_floats_async(grad_b_var, n_out, st)) return rc;
  }
  tag_kernel("mnf_conv_bwd_weight");
  hipLaunchKernelGGL(conv_bwd_weight_kernel, dim3((unsigned)p.col_blocks, (unsigned)p.slices), dim3(64), 0, st, a);
  if (int rc = check_launch()) return rc;
  const float* part = workspace;
  int rows = p.slices;
  if (p.groups) {  // sums[j] = slot j + slot (j + groups) + ...
    float* sums = workspace + p.slices * p.slot;
    if (int rc = zero_floats_async(sums, p.groups * p.slot, st)) return rc;
    if (int rc = det_reduce_async(workspace, p.slices / p.groups, p.groups * p.slot, p.groups * p.slot, sums, st)) return rc;
    part = sums, rows = p.groups;
  }
  if (packed) return det_reduce_async(part, rows, p.slot, p.slot, grad_Wz, st);
  if (int rc = det_reduce_async(part, rows, p.slot, nk, grad_Wz, st)) return rc;
  if (int rc = det_reduce_async(part + nk, rows, p.slot, nk, grad_W_var, st)) return rc;
  return det_reduce_async(part + 2 * nk, rows, p.slot, n_out, grad_b_var, st);
}

int mnf_mnf_conv_bwd_input(const float* x, const float* grad_out, const float* grad_var, const float* Wz,
                           const float* W_var, float* grad_x, int64_t batch, int n_in, int height, int width, int n_out,
                           int kernel_size, void* stream) {
  if (!x || !grad_out || !grad_var || !Wz || !W_var || !grad_x || batch < 1 || n_in < 1 || height < 1 || width < 1 ||
      n_out < 1 || kernel_size < 1)
    return MNF_ERR_INVALID_ARG;
  if (!conv_bwd_input_shape_ok(n_in, n_out, kernel_size, height, width)) return MNF_ERR_UNSUPPORTED;
  const int64_t n_pixels = conv_bwd_pixels(batch, (int64_t)height * width);
  if (!n_pixels) return MNF_ERR_UNSUPPORTED;
  ConvBwdIArgs a;
  a.x = x, a.g = grad_out, a.gv = grad_var, a.Wz = Wz, a.W_var = W_var, a.grad_x = grad_x;
  a.n_in = n_in, a.height = height, a.width = width, a.n_out = n_out, a.ksize = kernel_size;
  a.K = n_in * kernel_size * kernel_size;
  a.Kr = n_out * kernel_size * kernel_size, a.Krp = (a.Kr + 4 * convb::U - 1) / (4 * convb::U) * (4 * convb::U);
  a.oh = height - kernel_size + 1, a.ow = width - kernel_size + 1, a.ohw = a.oh * a.ow;
  a.n_pixels = (int)n_pixels;
  static DeviceMemo resident;
  const int blocks =
      resident.get([](int dev) { return resident_by_occupancy(conv_bwd_input_kernel, 64 * convb::WAVES, dev, 2); });
  // as the forward: two pixel tiles per wave share every weight read; a call too small to fill the resident workgroups that
  // way runs one tile per wave (same results: a pixel's sums do not depend on its tile's owner)
  a.pt = (n_pixels + convb::GROUP - 1) / convb::GROUP < blocks ? 1 : convb::P;
  const int64_t group = 16 * a.pt * convb::WAVES;
  a.n_groups = (int)((n_pixels + group - 1) / group);
  const int grid = a.n_groups < blocks ? a.n_groups : blocks;
  tag_kernel("mnf_conv_bwd_input");
  hipLaunchKernelGGL(conv_bwd_input_kernel, dim3((unsigned)grid), dim3(64 * convb::WAVES), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // extern "C"
