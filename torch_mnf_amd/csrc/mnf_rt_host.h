// Host side of the run-time-shaped matrix-core launchers (mnf_*_rt.hip; mnf_rt.h: any layer count and widths, weights from
// `flat`).  Each unit has a plan function of the shape alone -- false where the kernel has no launch for the shape, else
// the kernel arguments' shape part and an RtPlan -- which its queries (mnf_*_rt_supported, _grid, _det_workspace) and its
// launch answer from.  Here: what those plans are made of, and the frame around them.  (The LDS fit of the gradient
// kernels is built on mnf_rt_bwd.h's exchange area and lives there: rt::fit_bwd_lds.)
#pragma once
#include <cstring>

#include "mnf_host.h"
#include "mnf_rt.h"

namespace mnf {

// dynamic LDS a workgroup may ask for (allow_big_lds sets the attribute, every plan fits its launch under it)
constexpr size_t kRtLdsBytes = 160 * 1024;

struct RtPlan {
  int mt_max;     // size class: hidden tiles of a vector (4 / 8 / 16: widths up to 64 / 128 / 256)
  bool resident;  // forward kernels: the whole conditioner staged into LDS once (else chunk by chunk)
  int nw;         // waves per workgroup
  size_t lds;     // dynamic LDS bytes
};
// rows a workgroup takes per step: 16 per wave and row tile
inline int64_t rt_rows_per_block(const RtPlan& p, int tiles_per_wave = 1) { return (int64_t)16 * tiles_per_wave * p.nw; }

// sizes[1 .. n_hidden] := hidden[]; the smallest and largest width and the 16-unit tiles of all of them
struct HiddenWidths {
  int min, max, tiles;
};
inline HiddenWidths scan_hidden(int n_hidden, const int* hidden, int* sizes) {
  HiddenWidths w{1 << 30, 0, 0};
  for (int i = 0; i < n_hidden; ++i) {
    sizes[1 + i] = hidden[i];
    w.min = hidden[i] < w.min ? hidden[i] : w.min;
    w.max = hidden[i] > w.max ? hidden[i] : w.max;
    w.tiles += (hidden[i] + 15) / 16;
  }
  return w;
}
// the size class of a widest hidden layer of up to 256 units
inline int rt_size_class(int max_width) { return max_width <= 64 ? 4 : max_width <= 128 ? 8 : 16; }

// ---- where a family's parameters sit in `flat`: one function per family, shared by its directions.  sizes[]: the widths
// of the conditioner (scan_hidden).  Each fills the layout part of the kernel arguments and returns the parameter count;
// 0: an offset would leave 31 bits.
// AffineHalfFlow: the s net, then the t net (half -> hidden -> half each); an absent net aliases the other
template <typename Args>
inline int64_t ahf_layout(int n_hidden, const int* sizes, int has_scale, int has_shift, Args& a) {
  int64_t off = 0;
  if (has_scale) off += fill_net(a.s_net, n_hidden + 2, sizes, off);
  if (has_shift) off += fill_net(a.t_net, n_hidden + 2, sizes, off);
  if (!has_scale) a.s_net = a.t_net;
  if (!has_shift) a.t_net = a.s_net;
  return off >= (1ll << 31) ? 0 : off;
}
// NSF_CL: f1, then f2 (half -> hidden -> P * half each, sizes[n_hidden + 1] = P * half); the output layer's weights alone
// stay below 2^30
template <typename Args>
inline int64_t nsf_cl_layout(int n_hidden, const int* sizes, int max_width, Args& a) {
  if ((int64_t)sizes[n_hidden + 1] * max_width >= (1ll << 30)) return 0;
  const int64_t off = fill_net(a.f1, n_hidden + 2, sizes, 0);
  return off + fill_net(a.f2, n_hidden + 2, sizes, off);
}
// RNVP: the net dim -> h_1 .. h_n, then the heads Linear(h_n, dim): t, then s
template <typename Args>
inline int64_t rnvp_layout(int dim, int n_hidden, const int* sizes, Args& a) {
  int64_t off = fill_net(a.net, n_hidden + 1, sizes, 0);
  const int hl = sizes[n_hidden];
  a.t_w = (int)off; off += (int64_t)hl * dim;
  a.t_b = (int)off; off += dim;
  a.s_w = (int)off; off += (int64_t)hl * dim;
  a.s_b = (int)off; off += dim;
  return off >= (1ll << 31) ? 0 : off;
}
// MAF / IAF: the masked net dim -> h_1 .. h_n, then the last MaskedLinear(h_n, 2 dim) [s | t]; m_off[l]: layer l's mask in
// `masks`, a byte per weight
template <typename Args>
inline int64_t maf_layout(int dim, int n_hidden, const int* sizes, Args& a) {
  int64_t off = fill_net(a.net, n_hidden + 1, sizes, 0), moff = 0;
  const int hl = sizes[n_hidden];
  for (int l = 0; l < n_hidden; ++l) {
    a.m_off[l] = (int)moff;
    moff += (int64_t)sizes[l] * sizes[l + 1];
  }
  a.m_off[n_hidden] = (int)moff;
  moff += 2ll * dim * hl;
  a.s_w = (int)off; off += 2ll * dim * hl;
  a.s_b = (int)off; off += 2ll * dim;
  return off >= (1ll << 31) || moff >= (1ll << 31) ? 0 : off;
}

// ---- forward plans: what is staged, and where
// The staged image of Linear layers 0 .. n_layers - 1 of an MLP of widths sizes[]: A blocks of 32 input columns x 16 units
// and 16-unit bias tiles.  Layer 0 reads in_cols0 columns, a later one its predecessor's whole tiles.
struct StagedTiles {
  int64_t blocks, bias;
};
inline StagedTiles mlp_tiles(const int* sizes, int n_layers, int in_cols0) {
  StagedTiles t{0, 0};
  for (int l = 0; l < n_layers; ++l) {
    const int in_cols = l == 0 ? in_cols0 : 16 * ((sizes[l] + 15) / 16);
    t.blocks += (int64_t)((in_cols + 31) / 32) * ((sizes[l + 1] + 15) / 16);
    t.bias += (sizes[l + 1] + 15) / 16;
  }
  return t;
}
// LDS of a forward kernel: 64 bytes of scratch, then one resident image or two streaming buffers of cb blocks and bt bias tiles
template <typename Args>
inline void set_staging(Args& a, RtPlan& p, bool resident, int cb, int bt) {
  p.resident = resident;
  a.cb = cb;
  a.bt = bt;
  a.block_words = (resident ? 1 : 2) * cb * rt::kBlockWords;
  a.bias_words = (resident ? 1 : 2) * bt * 16;
  p.lds = 64 + (size_t)a.block_words * 4 + (size_t)a.bias_words * 4;
}
// ... the resident image where it fits `resident_bytes`, else buffers of `stream` blocks and bias tiles
template <typename Args>
inline void plan_staging(Args& a, RtPlan& p, StagedTiles image, int64_t resident_bytes, int stream) {
  const bool resident = image.blocks * 2048 + image.bias * 64 <= resident_bytes;
  set_staging(a, p, resident, resident ? (int)image.blocks : stream, resident ? (int)image.bias : stream);
}
// Workgroups of 8 waves (4 in the widest class) -- of 4 when the LDS footprint of a resident plan lets a CU hold two or
// more of them (they overlap each other's barriers, staging and memory waits; streaming: every wave of the CU shares one
// conversion of the weights)
inline int rt_fwd_waves(const RtPlan& p) { return p.mt_max == 16 || (p.resident && p.lds <= 79 * 1024) ? 4 : 8; }
// the largest of nw_max, nw_max / 2, .. 1 waves whose per-wave slabs fit next to `fixed` bytes (0: not even one)
inline int fit_slab_waves(int nw_max, size_t fixed, size_t slab) {
  int nw = nw_max;
  while (nw >= 1 && fixed + nw * slab > kRtLdsBytes) nw >>= 1;
  return nw;
}

// ---- launches
// up to kRtLdsBytes of dynamic LDS for each of `kernels`, set once per device (`memo`: the call site's own)
template <typename... K>
inline void allow_big_lds(DeviceMemo& memo, K... kernels) {
  memo.get([&](int) {
    ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernels), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRtLdsBytes),
     ...);
    return 1;
  });
}
// The launches themselves exist once in the library, whatever the kernel's argument struct: RtKernel is a kernel of one
// by-value struct argument with its type dropped (hipLaunchKernel is what the <<< >>> stub of such a kernel calls).
#define MNF_RT_ONCE inline __attribute__((noinline))
struct RtKernel {
  const void* fn;
  template <typename Args>
  RtKernel(void (*kernel)(Args)) : fn(reinterpret_cast<const void*>(kernel)) {}
};
// persistent grid: as many workgroups of nw waves as the occupancy query says are resident (one per CU if it fails), at
// most one per `rows_per_block` rows
MNF_RT_ONCE int64_t persistent_grid(RtKernel kernel, int nw, size_t lds, int64_t rows_per_block, int64_t rows) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel.fn, nw * 64, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  const int64_t need = (rows + rows_per_block - 1) / rows_per_block;
  const int64_t grid = (int64_t)per_cu * device_cus(current_device());
  return grid > need ? need : grid;
}
MNF_RT_ONCE int launch_grid(RtKernel kernel, void* args, int64_t grid, int nw, size_t lds, const char* tag, hipStream_t stream) {
  tag_kernel(tag);
  (void)hipLaunchKernel(kernel.fn, dim3((unsigned)grid), dim3(nw * 64), &args, lds, stream);
  return check_launch();
}
// ... launched; tags the launch with the kernel family `tag`
template <typename Args>
inline int launch_persistent(void (*kernel)(Args), const Args& a, int nw, size_t lds, int64_t rows_per_block, int64_t rows,
                             const char* tag, hipStream_t stream) {
  return launch_grid(kernel, const_cast<Args*>(&a), persistent_grid(kernel, nw, lds, rows_per_block, rows), nw, lds, tag, stream);
}
// ... of a plan
template <typename Args>
inline int launch_plan(void (*kernel)(Args), const Args& a, const RtPlan& p, int tiles_per_wave, int64_t rows, const char* tag,
                       hipStream_t stream) {
  return launch_persistent(kernel, a, p.nw, p.lds, rt_rows_per_block(p, tiles_per_wave), rows, tag, stream);
}

// The fixed-order form of the run-time-shaped gradient launches (mnf_*_bwd_rt_det): every workgroup of the persistent
// grid adds into a slot of its own (grad_flat + blockIdx.x * slot_floats), and det_reduce_async adds the slots up in
// order.  A parameter's entry in a slot receives its adds from ONE lane, in program order (the weight-gradient products
// go to the waves by shape alone, mnf_rt_bwd.h dw_phase_rows), so that every slot -- and the sum -- is the same every
// run.  The grid is persistent_grid's, capped so that the slots stay within kRtDetMaxBytes.
constexpr int64_t kRtDetMaxBytes = (int64_t)512 << 20;
inline int64_t rt_det_slot_floats(int64_t n_params) { return (n_params + 63) / 64 * 64; }  // whole 256-byte lines
inline int64_t rt_det_slots(int64_t grid, int64_t n_params) {
  int64_t cap = kRtDetMaxBytes / (4 * rt_det_slot_floats(n_params));
  if (cap < 1) cap = 1;
  return grid < cap ? grid : cap;
}
// det: the slots in `workspace` (at least slots x slot_floats floats, else MNF_ERR_INVALID_ARG before any launch), zeroed,
// filled, added to a.grad_flat; grad_flat == NULL or !det: launch_persistent
// (args: the caller's own copy of the arguments, whose grad_flat and slot_floats members this sets)
MNF_RT_ONCE int launch_rt_bwd(RtKernel kernel, void* args, float** grad_flat, int64_t* slot_floats, int nw, size_t lds,
                              int64_t rows_per_block, int64_t rows, int64_t n_params, bool det, float* workspace,
                              int64_t workspace_floats, const char* tag, hipStream_t stream) {
  *slot_floats = 0;
  const int64_t grid = persistent_grid(kernel, nw, lds, rows_per_block, rows);
  if (!det || !*grad_flat) return launch_grid(kernel, args, grid, nw, lds, tag, stream);
  const int64_t slots = rt_det_slots(grid, n_params);
  const int64_t slot = rt_det_slot_floats(n_params);
  if (!workspace || workspace_floats < slots * slot) return MNF_ERR_INVALID_ARG;
  float* const dst = *grad_flat;
  *grad_flat = workspace;
  *slot_floats = slot;
  int rc = zero_floats_async(workspace, slots * slot, stream);
  if (rc != MNF_OK) return rc;
  rc = launch_grid(kernel, args, slots, nw, lds, tag, stream);
  return rc != MNF_OK ? rc : det_reduce_async(workspace, (int)slots, slot, n_params, dst, stream);
}

// ---- the entry frame.  `plan` is the unit's plan function with the shape bound, called as plan(Args&, RtPlan&): 0 or false
// where the shape has none; for the gradient entries, the number of parameters a workgroup's slot holds where it has one.
// `kernel_of` is the unit's X_kernel_of(const RtPlan&): the plan's kernel with its dynamic-LDS attribute set.  It touches
// HIP, so the queries call it only once a gfx950 device is known to be visible: without one they answer 0 from the shape alone.
// mnf_*_rt_supported
template <typename Args, typename Plan>
inline int rt_has_plan(Plan plan) {
  Args a;
  RtPlan p;
  return plan(a, p) ? 1 : 0;
}
// mnf_*_rt_grid: workgroups of the launch (each walks the row blocks blockIdx.x, + grid, ...); 0: no launch, or no device
template <typename Args, typename Plan, typename KernelOf>
inline int64_t rt_grid_query(int64_t rows, int tiles_per_wave, Plan plan, KernelOf kernel_of) {
  Args a;
  RtPlan p;
  if (rows < 1 || !plan(a, p) || !gfx950_visible()) return 0;
  return persistent_grid(kernel_of(p), p.nw, p.lds, rt_rows_per_block(p, tiles_per_wave), rows);
}
// mnf_*_bwd_rt_det_workspace: floats of workspace launch_rt_bwd's det form needs (0: no launch, or no device)
template <typename Args, typename Plan, typename KernelOf>
inline int64_t rt_det_workspace(int64_t rows, int dim, Plan plan, KernelOf kernel_of) {
  Args a;
  RtPlan p;
  int64_t n_params = 0;
  if (rows < 1 || rows * dim >= (1ll << 40) || !(n_params = plan(a, p)) || !gfx950_visible()) return 0;
  const int64_t grid = persistent_grid(kernel_of(p), p.nw, p.lds, rt_rows_per_block(p), rows);
  return rt_det_slots(grid, n_params) * rt_det_slot_floats(n_params);
}
// The gradient entries behind their own argument checks.  In this order: MNF_ERR_INVALID_ARG for a det call without a
// workspace, MNF_ERR_DOMAIN unless in_domain, MNF_OK for no rows, MNF_ERR_UNSUPPORTED if `unsupported` (the unit's own
// reasons), for a call that is not det under MNF_DETERMINISTIC=1, beyond 2^40 elements and where the shape has no plan; then
// fill(a) sets the call's part of the arguments and the plan's kernel is launched (det: fixed-order sums through `workspace`).
struct RtBwdCall {
  int64_t rows;
  int dim;
  const float* grad_flat;
  bool det;
  float* workspace;
  int64_t workspace_floats;
  const char* tag;
  void* stream;
};
template <typename Args, typename Plan, typename Fill, typename KernelOf>
inline int run_rt_bwd(const RtBwdCall& c, bool in_domain, bool unsupported, Plan plan, Fill fill, KernelOf kernel_of) {
  if (c.det && c.grad_flat && c.rows > 0 && (!c.workspace || c.workspace_floats < 1)) return MNF_ERR_INVALID_ARG;
  if (!in_domain) return MNF_ERR_DOMAIN;
  if (c.rows == 0) return MNF_OK;
  if (unsupported || (!c.det && deterministic()) || c.rows * c.dim >= (1ll << 40)) return MNF_ERR_UNSUPPORTED;
  Args a;
  memset(&a, 0, sizeof(a));
  RtPlan p;
  const int64_t n_params = plan(a, p);
  if (!n_params) return MNF_ERR_UNSUPPORTED;
  fill(a);
  return launch_rt_bwd(kernel_of(p), &a, &a.grad_flat, &a.slot_floats, p.nw, p.lds, rt_rows_per_block(p), c.rows, n_params, c.det,
                       c.workspace, c.workspace_floats, c.tag, (hipStream_t)c.stream);
}

}  // namespace mnf
