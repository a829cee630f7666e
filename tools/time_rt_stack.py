"""A 9-layer AffineHalfFlow model on the run-time-shaped kernels: one launch for the run (fuse_affine_runs on:
ahf_stack_rt) against one per layer (off: ahf_rt), alternating in one process -- ns per row and layer of model.inverse()
and of log_prob(return_sum=True).
usage: python3 tools/time_rt_stack.py [only the cases whose name contains this] [repetitions]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import torch_mnf_amd as amd

ONLY = sys.argv[1] if len(sys.argv) > 1 else ""
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
DEV, LAYERS = "cuda", 9

# (dim, h_sizes, rows)
CASES = [
    (64, (24, 24), 262144), (64, (24, 24), 4096), (64, (64, 64, 64), 262144), (512, (24, 24, 24), 262144),
    (512, (64, 64, 64), 262144), (256, (200, 130, 40, 7), 262144), (128, (100,), 262144),
]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps):
    """best and median of `reps` timings of each of `fns`, taken in turns (ms)"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(once(fn))
    return [(min(t), sorted(t)[len(t) // 2]) for t in times]


for dim, hs, rows in CASES:
    name = f"d={dim} {hs} rows={rows}"
    if ONLY not in name:
        continue
    torch.manual_seed(dim + len(hs))
    models = []
    for fused in (True, False):
        torch.manual_seed(dim + len(hs))
        flows = [amd.AffineHalfFlow(dim, parity=bool(i % 2), h_sizes=hs) for i in range(LAYERS)]
        if flows[0]._image_index_host() is not None:  # a shape with per-shape kernels: forced onto this tier
            for f in flows:
                f.force_generic = 2
        m = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)
        m.fuse_affine_runs = fused
        models.append(m)
    x = torch.randn(rows, dim, device=DEV)
    per = 1e6 / (rows * LAYERS)  # ms -> ns per row and layer
    with torch.no_grad():
        names = []
        for m in models:
            m.inverse(x)
            names.append(amd.last_kernel())
        inv = alternate([lambda m=m: m.inverse(x) for m in models], REPS)
        lp = alternate([lambda m=m: m.log_prob(x, return_sum=True) for m in models], REPS)
    print(f"{name:40s} inverse  fused {inv[0][0] * per:7.4f} (median {inv[0][1] * per:7.4f})  unfused {inv[1][0] * per:7.4f} "
          f"(median {inv[1][1] * per:7.4f}) ns/row/layer  [{names[0]} / {names[1]}]")
    print(f"{'':40s} log_prob fused {lp[0][0] * per:7.4f} (median {lp[0][1] * per:7.4f})  unfused {lp[1][0] * per:7.4f} "
          f"(median {lp[1][1] * per:7.4f}) ns/row/layer  [epilogue fused: {models[0]._logprob_done} / {models[1]._logprob_done}]",
          flush=True)
