// MNFConv2d.forward (torch_mnf/layers/mnf_conv.py:67-88, algorithm 2 of the MNF paper) behind its operands as ONE launch:
//   out[n, co, oy, ox] = fma(sqrt(v), eps[n, co, oy, ox], m)
//   m = b_mean[co] + sum_k x[n, ci, oy + ky, ox + kx]   * Wz[co, k]         k = (ci, ky, kx)
//   v = b_var[co]  + sum_k x[n, ci, oy + ky, ox + kx]^2 * W_var[co, k]
// for contiguous NCHW float32 x, stride 1, no padding, no dilation, one group.  Both convolutions read the same input
// patch, one needs its square, the epilogue is elementwise: an implicit GEMM on the exact-fp32 matrix instruction
// (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, bit for bit), the output channels as its rows and 16 consecutive
// output pixels (of the flattened (n, oy, ox) index) as its columns -- lanes 0..15 of a result register hold 16
// consecutive pixels of one channel, 64-byte runs of out / eps / var_out wherever a tile does not cross a row's end.
//
//   offsets   ci H W + ky W + kx for every k, in LDS; K = n_in k^2 is padded to a multiple of 16 (four matrix
//             instructions' worth, whose gathers are issued together) with offset 0 and zero weights: the padded steps
//             re-read the patch's first element and multiply it by zero
//   weights   through LDS in chunks of KC = 64 k, both convolutions' interleaved, already in A-operand order: the
//             float2 (Wz, W_var)[co = 16 m + (lane & 15)][k = 4 g + (lane >> 4)] of step g and channel tile m sits
//             at word-pair (4 g + m) * 64 + lane -- one conflict-free ds_read_b64 feeds 2 P matrix instructions.  A
//             chunk is read into registers while the previous one is multiplied, and written to LDS between two
//             barriers; a K of one chunk is staged once per workgroup.  Only the READ side is conflict-free: a wave
//             fetches 64 consecutive k of one channel (coalesced global reads), so its 64 LDS stores of a chunk row sit
//             16 or 64 word-pairs apart and serialise on a few banks -- 16 such stores per thread and chunk, against
//             256 matrix instructions per wave and chunk; turning the assignment round would un-coalesce the global side
//   gathers   x at 16 consecutive pixels and one k per quarter wave; they run four K-steps ahead of the products
//   waves     each owns P = 2 pixel tiles x 4 channel tiles x {mean, var} accumulators (64 registers); a workgroup
//             of 4 waves = 128 pixels per pass of a persistent loop.  A call too small to fill the resident
//             workgroups that way runs one tile per wave (64 pixels per pass, twice the workgroups)
//   edges     pixels past the end compute on the last pixel's (clamped) addresses, rows >= n_out on zero weights;
//             neither is stored.  Channel tiles past ceil(n_out / 16) are skipped (a uniform branch).
// No atomics, no scratch, no host synchronisation: the launch is capturable in a hipGraph, and it repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mnf_hip.h"
#include "mnf_host.h"

namespace mnf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace convf {
constexpr int P = 2;         // pixel tiles per wave
constexpr int MT = 4;        // channel tiles (n_out <= 64)
constexpr int KC = 64;       // k per weight chunk
constexpr int U = 4;         // K-steps (of 4 k) whose gathers are issued together: K is padded to 4 U
constexpr int WAVES = 4;     // per workgroup
constexpr int KMAX = 4096;   // n_in k^2, padded
constexpr int GROUP = 16 * P * WAVES;  // pixels per workgroup pass
}  // namespace convf

struct ConvFwdArgs {
  const float* x;
  const float* Wz;
  const float* W_var;
  const float* b_mean;
  const float* b_var;
  const float* eps;
  float* out;
  float* var_out;  // may be null
  int n_in, height, width, n_out, ksize;
  int K, Kp;       // n_in k^2, and padded to a multiple of 4 U
  int ohw, ow;     // output pixels per image, per row
  int n_pixels;    // batch * ohw
  int pt;          // pixel tiles per wave in this launch: P, or 1 for few pixels
  int n_groups;    // ceil(n_pixels / (16 pt WAVES))
};

__global__ void __launch_bounds__(64 * convf::WAVES) conv_fwd_kernel(const ConvFwdArgs a) {
  using namespace convf;
  __shared__ int s_off[KMAX];
  __shared__ float2 s_w[(KC / 4) * MT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int mt = (a.n_out + 15) >> 4;
  const int hw = a.height * a.width, kk2 = a.ksize * a.ksize;

  for (int k = tid; k < a.Kp; k += 64 * WAVES) {
    int o = 0;
    if (k < a.K) {
      const int ci = k / kk2, r = k - ci * kk2, ky = r / a.ksize;
      o = ci * hw + ky * a.width + (r - ky * a.ksize);
    }
    s_off[k] = o;
  }
  const int n_chunks = (a.Kp + KC - 1) / KC;

  // One chunk of both weight matrices: `fetch` reads this thread's share -- k = k0 + (tid & 63) of the channels wave,
  // wave + 4, ... (rows >= n_out and k >= K: zeros) -- into registers, `put` writes it to LDS in A-operand order.  The
  // fetch of the next chunk is issued before the products of the current one, so its latency hides behind them.
  constexpr int PRE = 16 * MT * KC / (64 * WAVES);
  float2 pre[PRE];
  const int kk = tid & (KC - 1);
  auto fetch = [&](int k0) {
    const int k = k0 + kk;
    int w0 = wave;  // opaque: the 16 addresses are formed here, not kept in registers across the persistent loop
    asm volatile("" : "+v"(w0));
#pragma unroll
    for (int j = 0; j < PRE; ++j)
      if (j < 4 * mt) {
        const int co = w0 + WAVES * j;
        pre[j] = make_float2(0.f, 0.f);
        if (co < a.n_out && k < a.K) {
          const int at = co * a.K + k;  // < 64 * 4096
          pre[j] = make_float2(a.Wz[at], a.W_var[at]);
        }
      }
  };
  auto put = [&]() {
#pragma unroll
    for (int j = 0; j < PRE; ++j)
      if (j < 4 * mt) {
        const int co = wave + WAVES * j;
        s_w[((kk >> 2) * MT + (co >> 4)) * 64 + (kk & 3) * 16 + (co & 15)] = pre[j];
      }
  };
  fetch(0);
  if (n_chunks == 1) put();  // the only chunk stays resident
  __syncthreads();

  const int pt = a.pt;
  for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
    int q4 = 4 * q;  // opaque per pass: what depends on it below (32 bias values, 32 channel offsets) is recomputed each
    asm volatile("" : "+v"(q4));  // pass, not kept in registers across the whole persistent loop (the Makefile's
                                  // check_agpr.py run fails the build if another compiler spills after all)
    const float* xb[P];
    int64_t at0[P];  // of (n, channel 0, oy, ox) in out / eps / var_out
    bool live[P];
#pragma unroll
    for (int t = 0; t < P; ++t) {
      int p = ((grp * WAVES + wave) * pt + t) * 16 + c;
      live[t] = t < pt && p < a.n_pixels;
      p = live[t] ? p : a.n_pixels - 1;
      const int n = p / a.ohw, rem = p - n * a.ohw, oy = rem / a.ow;
      xb[t] = a.x + ((int64_t)n * a.n_in * hw + oy * a.width + (rem - oy * a.ow));
      at0[t] = (int64_t)n * a.n_out * a.ohw + rem;
    }
    f32x4 am[P][MT], av[P][MT];  // the sums start at the biases
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = 16 * m + q4 + r;
        const int cc = co < a.n_out ? co : a.n_out - 1;
        const float b1 = a.b_mean[cc], b2 = a.b_var[cc];
#pragma unroll
        for (int t = 0; t < P; ++t) am[t][m][r] = b1, av[t][m][r] = b2;
      }

    // The patch gathers run one group of U K-steps ahead of the products (the offset table holds every k, so they do
    // not stop at a weight chunk's end): xn = x at the pixels of this wave's tiles and the k of the NEXT group.
    float xn[U][P] = {};
    auto gather = [&](int kb) {
      int o[U];
#pragma unroll
      for (int u = 0; u < U; ++u) o[u] = s_off[kb + 4 * u + q];
#pragma unroll
      for (int u = 0; u < U; ++u) xn[u][0] = xb[0][o[u]];
      if (pt > 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) xn[u][1] = xb[1][o[u]];
      }
    };
    gather(0);
    // U K-steps of NT pixel tiles: 2 NT independent accumulator chains per channel tile, each in k order
    auto products = [&](auto nt, int g0, const float (&xv)[U][P], const float (&xs)[U][P]) {
      constexpr int NT = decltype(nt)::value;
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float2 w = s_w[((g0 + u) * MT + m) * 64 + lane];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              am[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, xv[u][t], am[t][m], 0, 0, 0);
              av[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, xs[u][t], av[t][m], 0, 0, 0);
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
      const int steps = ((a.Kp - k0 < KC ? a.Kp - k0 : KC)) >> 2;  // a multiple of U
#pragma unroll 1
      for (int g0 = 0; g0 < steps; g0 += U) {
        float xv[U][P], xs[U][P];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int t = 0; t < P; ++t) xv[u][t] = xn[u][t], xs[u][t] = xn[u][t] * xn[u][t];
        const int kb = k0 + 4 * (g0 + U);
        gather(kb < a.Kp ? kb : a.Kp - 4 * U);  // (past the end: the last group again, unused)
        if (pt > 1)
          products(std::integral_constant<int, P>{}, g0, xv, xs);
        else
          products(std::integral_constant<int, 1>{}, g0, xv, xs);
      }
    }

#pragma unroll
    for (int t = 0; t < P; ++t) {
      if (t >= pt) continue;
      // the tile's noise first, all loads in flight at once, from clamped addresses (a pixel past the end reads the last
      // pixel's, a channel past the end the last channel's); the stores are per-lane selects
      float e[MT][4];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = 16 * m + q4 + r;
            e[m][r] = a.eps[at0[t] + (co < a.n_out ? co : a.n_out - 1) * a.ohw];
          }
        }
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m < mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = 16 * m + q4 + r;
            const int64_t at = at0[t] + co * a.ohw;
            const float v = av[t][m][r];
            const float o = fmaf(sqrtf(v), e[m][r], am[t][m][r]);
            if (live[t] && co < a.n_out) {
              a.out[at] = o;
              if (a.var_out) a.var_out[at] = v;
            }
          }
        }
    }
  }
}

static bool conv_fwd_shape_ok(int n_in, int n_out, int ksize, int height, int width) {
  if (n_in < 1 || n_out < 1 || n_out > 64 || ksize < 1 || height < ksize || width < ksize) return false;
  if ((int64_t)n_in * ksize * ksize > convf::KMAX) return false;
  // the patch offsets (< n_in H W) and the channel offsets inside an output image (< 64 H W) are 32-bit
  return (int64_t)(n_in > 64 ? n_in : 64) * height * width < ((int64_t)1 << 31);
}

}  // namespace mnf

using namespace mnf;

extern "C" {

int mnf_mnf_conv_fwd_supported(int n_in, int n_out, int kernel_size, int height, int width) {
  return conv_fwd_shape_ok(n_in, n_out, kernel_size, height, width) ? 1 : 0;
}

int mnf_mnf_conv_fwd(const float* x, const float* Wz, const float* W_var, const float* b_mean, const float* b_var,
                     const float* eps, float* out, float* var_out, int64_t batch, int n_in, int height, int width,
                     int n_out, int kernel_size, void* stream) {
  if (!x || !Wz || !W_var || !b_mean || !b_var || !eps || !out || batch < 1 || n_in < 1 || height < 1 || width < 1 ||
      n_out < 1 || kernel_size < 1)
    return MNF_ERR_INVALID_ARG;
  if (!conv_fwd_shape_ok(n_in, n_out, kernel_size, height, width)) return MNF_ERR_UNSUPPORTED;
  const int oh = height - kernel_size + 1, ow = width - kernel_size + 1;
  // the pixel index is 32-bit (compared by division: batch * oh * ow itself may not fit 64 bits)
  const int64_t max_pixels = ((int64_t)1 << 31) - 2 * convf::GROUP;
  if (batch > max_pixels / ((int64_t)oh * ow)) return MNF_ERR_UNSUPPORTED;
  const int64_t n_pixels = batch * oh * ow;
  ConvFwdArgs a;
  a.x = x, a.Wz = Wz, a.W_var = W_var, a.b_mean = b_mean, a.b_var = b_var, a.eps = eps, a.out = out, a.var_out = var_out;
  a.n_in = n_in, a.height = height, a.width = width, a.n_out = n_out, a.ksize = kernel_size;
  a.K = n_in * kernel_size * kernel_size, a.Kp = (a.K + 4 * convf::U - 1) / (4 * convf::U) * (4 * convf::U);
  a.ohw = oh * ow, a.ow = ow;
  a.n_pixels = (int)n_pixels;
  static DeviceMemo resident;
  const int blocks = resident.get([](int dev) { return resident_by_occupancy(conv_fwd_kernel, 64 * convf::WAVES, dev, 2); });
  // two pixel tiles per wave share every weight read; a call that would not fill the resident workgroups that way
  // spreads over twice as many with one tile per wave (same results: a pixel's sums do not depend on its tile's owner)
  a.pt = (n_pixels + convf::GROUP - 1) / convf::GROUP < blocks ? 1 : convf::P;
  const int64_t group = 16 * a.pt * convf::WAVES;
  a.n_groups = (int)((n_pixels + group - 1) / group);
  const int grid = a.n_groups < blocks ? a.n_groups : blocks;
  tag_kernel("mnf_conv_fwd");
  hipLaunchKernelGGL(conv_fwd_kernel, dim3((unsigned)grid), dim3(64 * convf::WAVES), 0, (hipStream_t)stream, a);
  return check_launch();
}

}  // extern "C"
