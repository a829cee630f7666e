// The shape plans of the run-time-shaped launchers (torch_mnf_amd/csrc/mnf_*_rt.hip), dumped over a grid of shapes: one
// line per cell with the plan function's answer and the bytes of its Args and RtPlan (both zeroed before the call) in hex.
// For comparing two trees: build it against each with the same PLAN, run both, and `cmp` the outputs.
//
// Host code only: the unit's source is compiled into this program for its static plan function, nothing looks a kernel up
// or launches one, and it runs on a machine without a GPU.  PLAN picks the plan function (the table below); TREE is the
// tree's root, whose mnf_generic.o (built by the Makefile) supplies fill_net, hidden_ok and mnf_nsf_ar_flat_floats:
//
//   for n in 1 2 3 4 5 6 7 8 9 10 11 12 13; do
//     hipcc -std=c++17 -O1 --offload-arch=gfx950 --cuda-host-only -DPLAN=$n -I$TREE/torch_mnf_amd/csrc -I$TREE/include \
//       tools/rt_plan_dump.hip -Wl,$TREE/torch_mnf_amd/csrc/mnf_generic.o -Wl,--unresolved-symbols=ignore-all \
//       -o /tmp/rt_plan_dump_$n && /tmp/rt_plan_dump_$n > plans_$n.txt
//   done
//
// (--unresolved-symbols=ignore-all: the launch half of the unit refers to the rest of the library, and is never called.)
// The counts of the grid -- cells, cells with a plan, resident / streaming plans, plans with fewer than 8 waves -- go to
// stderr.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if PLAN == 1
#include "mnf_ahf_rt.hip"
#define PLAN_NAME "ahf_rt_plan"
#define PLAN_ARGS mnf::AhfRtArgs
#define PLAN_CALL mnf::ahf_rt_plan(dim, n, h, hs, ht, flag, a, p)
#define USES_HEADS 1
#define USES_FLAG 1
#elif PLAN == 2
#include "mnf_rnvp_rt.hip"
#define PLAN_NAME "rnvp_rt_plan"
#define PLAN_ARGS mnf::RnvpRtArgs
#define PLAN_CALL mnf::rnvp_rt_plan(dim, n, h, flag, a, p)
#define USES_FLAG 1
#elif PLAN == 3
#include "mnf_nsf_rt.hip"
#define PLAN_NAME "nsf_rt_plan"
#define PLAN_ARGS mnf::NsfRtArgs
#define PLAN_CALL mnf::nsf_rt_plan(dim, K, n, h, flag, a, p)
#define USES_K 1
#define USES_FLAG 1
#elif PLAN == 4
#include "mnf_maf_rt.hip"
#define PLAN_NAME "maf_rt_plan"
#define PLAN_ARGS mnf::MafRtArgs
#define PLAN_CALL mnf::maf_rt_plan(dim, n, h, a, p)
#elif PLAN == 5
#include "mnf_maf_rt.hip"
#define PLAN_NAME "maf_seq_rt_plan"
#define PLAN_ARGS mnf::MafRtArgs
#define PLAN_CALL mnf::maf_seq_rt_plan(dim, n, h, a, p)
#elif PLAN == 6
#include "mnf_ahf_bwd_rt.hip"
#define PLAN_NAME "ahf_bwd_rt_plan"
#define PLAN_ARGS mnf::AhfBwdRtArgs
#define PLAN_CALL mnf::ahf_bwd_rt_plan(dim, n, h, hs, ht, flag, a, p)
#define USES_HEADS 1
#define USES_FLAG 1
#elif PLAN == 7
#include "mnf_rnvp_bwd_rt.hip"
#define PLAN_NAME "rnvp_bwd_rt_plan"
#define PLAN_ARGS mnf::RnvpBwdRtArgs
#define PLAN_CALL mnf::rnvp_bwd_rt_plan(dim, n, h, a, p)
#elif PLAN == 8
#include "mnf_nsf_bwd_rt.hip"
#define PLAN_NAME "nsf_bwd_rt_plan"
#define PLAN_ARGS mnf::NsfBwdRtArgs
#define PLAN_CALL mnf::nsf_bwd_rt_plan(dim, K, n, h, a, p)
#define USES_K 1
#elif PLAN == 9
#include "mnf_maf_bwd_rt.hip"
#define PLAN_NAME "maf_bwd_rt_plan"
#define PLAN_ARGS mnf::MafBwdRtArgs
#define PLAN_CALL mnf::maf_bwd_rt_plan(dim, n, h, a, p)
#elif PLAN == 10
#include "mnf_maf_bwd_rt.hip"  // (mnf_maf_bwd_rt_supported, which the plan below asks)
#include "mnf_maf_seq_bwd_rt.hip"
#define PLAN_NAME "maf_seq_bwd_rt_plan"
#define PLAN_ARGS mnf::MafSeqBwdArgs
#define PLAN_CALL mnf::maf_seq_bwd_rt_plan(dim, n, h, a, p)
#elif PLAN == 11
#include "mnf_nsf_ar_rt.hip"
#define PLAN_NAME "nsf_ar_rt_plan"
#define PLAN_ARGS mnf::NsfArRtArgs
#define PLAN_CALL mnf::nsf_ar_rt_plan(dim, K, n, h, a, p)
#define USES_K 1
#elif PLAN == 12
#include "mnf_nsf_ar_bwd_rt.hip"
#define PLAN_NAME "nsf_ar_bwd_rt_plan"
#define PLAN_ARGS mnf::NsfArBwdRtArgs
#define PLAN_CALL mnf::nsf_ar_bwd_rt_plan(dim, K, n, h, a, p)
#define USES_K 1
#elif PLAN == 13
#include "mnf_nsf_ar_seq_rt.hip"
#define PLAN_NAME "nsf_ar_seq_rt_plan"
#define PLAN_ARGS mnf::NsfArSeqRtArgs
#define PLAN_CALL mnf::nsf_ar_seq_rt_plan(dim, K, n, h, a, p)
#define USES_K 1
#else
#error "PLAN = 1 .. 13"
#endif
#ifndef USES_K
#define USES_K 0
#endif
#ifndef USES_HEADS
#define USES_HEADS 0
#endif
#ifndef USES_FLAG
#define USES_FLAG 0
#endif

static long g_cells = 0, g_plans = 0, g_resident = 0, g_streaming = 0, g_few_waves = 0;

static void hex(const void* v, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(v);
  for (size_t i = 0; i < n; ++i) printf("%02x", b[i]);
}

// one cell: flag is `aligned` (forward plans) or `wide` (ahf_bwd_rt_plan)
static void cell(int dim, int K, int n, const int* h, int hs, int ht, bool flag) {
  PLAN_ARGS a;
  mnf::RtPlan p;
  memset(&a, 0, sizeof(a));
  memset(&p, 0, sizeof(p));
  const bool ok = PLAN_CALL;
  ++g_cells;
  if (ok) {
    ++g_plans;
    ++(p.resident ? g_resident : g_streaming);
    if (p.nw < 8) ++g_few_waves;
  }
  printf("%d %d %d [", dim, K, n);
  for (int i = 0; h && i < n; ++i) printf(i ? " %d" : "%d", h[i]);
  printf(h ? "] %d %d %d : %d" : "null] %d %d %d : %d", hs, ht, (int)flag, (int)ok);
  printf(" ");
  hex(&a, sizeof(a));
  printf(" ");
  hex(&p, sizeof(p));
  printf("\n");
}

// every axis the plan function has, around one (dim, hidden) pair
static void cells(int dim, int n, const int* h) {
  static const int Ks[] = {1, 2, 5, 8, 10, 16, 17};
  for (int ki = 0; ki < (USES_K ? 7 : 1); ++ki)
    for (int heads = USES_HEADS ? 0 : 3; heads < 4; ++heads)
      for (int flag = 0; flag < (USES_FLAG ? 2 : 1); ++flag) cell(dim, USES_K ? Ks[ki] : 0, n, h, heads & 1, heads >> 1, flag != 0);
}

int main() {
  static const int dims[] = {1, 2, 3, 4, 6, 8, 16, 17, 32, 37, 64, 100, 128, 130, 256, 512, 784, 4096};
  static const int widths[] = {3, 4, 7, 16, 17, 24, 33, 64, 65, 100, 128, 129, 200, 256, 257};
  constexpr int kMixed = 24;  // mixed-width tuples per layer count, next to the 15 uniform ones
  uint32_t lcg = 12345u;
  auto next = [&](uint32_t m) {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 8) % m;
  };
  for (int n = 0; n <= 6; ++n) {
    const int n_tuples = n == 0 ? 1 : n == 1 ? 15 : 15 + kMixed;
    for (int t = 0; t < n_tuples; ++t) {
      int h[8] = {0};
      // mixed tuples: every second one from the widths up to 64 (the gradient kernels' envelope), every fourth from those
      // up to 16 (the NSF_AR kernels')
      const uint32_t pool = t % 4 == 1 ? 4 : t % 2 == 0 ? 8 : 15;
      for (int i = 0; i < n; ++i) h[i] = t < 15 ? widths[t] : widths[1 + next(pool - 1)];
      for (int dim : dims) cells(dim, n, h);
    }
  }
  // null and non-positive hidden
  const int zero[3] = {16, 0, 16}, negative[2] = {-4, 16};
  for (int dim : {2, 16, 64}) {
    cells(dim, 2, nullptr);
    cells(dim, 3, zero);
    cells(dim, 2, negative);
    cells(dim, -1, zero);
  }
  fprintf(stderr, "%s: %ld cells, %ld with a plan: %ld resident, %ld streaming, %ld with nw < 8\n", PLAN_NAME, g_cells, g_plans,
          g_resident, g_streaming, g_few_waves);
  return 0;
}
