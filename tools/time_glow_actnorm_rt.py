#!/usr/bin/env python3
"""The training pass of one [ActNormFlow, Glow] pair closing a log-prob, fused (glow_actnorm_inv_rt / _bwd_rt: one
autograd node, one launch each way plus the fixed-order reduction) against layer by layer (MNF_NO_PAIR_FUSION: Glow on
linear_rows_rt, ActNorm's affine_const kernels, gauss_logprob), through the Python layer with HIP events.

The routes ALTERNATE inside one process (fused, layers, layers again, fused, ...), each call timed by its own event pair;
reported is the median over --reps timed calls (at least 15) after --warmup untimed rounds, in ns per row, forward
(log_prob) and forward + backward separately.  The layer-by-layer route is timed TWICE per round ("layers", "layers'"):
the difference of the two medians is the run-to-run spread the verdict allows the fused route.  Next to each line: the
GPU kernels of one call (torch.profiler, counted once outside the timing; n/a where the profiler is not available) and the
HBM bytes per row by arithmetic.

usage: time_glow_actnorm_rt.py [--dims 48,100,256,512] [--rows 65536,262144] [--reps 15] [--warmup 3] [--no-launch-count]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch, flows  # noqa: E402


def make_pair(dim, dev):
    torch.manual_seed(dim)
    return amd.NormalizingFlowModel(amd.StandardNormal(dim), [amd.ActNormFlow(dim), amd.Glow(dim)]).to(dev)


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception:  # noqa: BLE001 (no profiler in this build: the timing does not depend on it)
        return None


def alternate(calls, reps, warmup):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="48,100,256,512")
    ap.add_argument("--rows", default="65536,262144")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    reps = max(args.reps, 15)
    dev = "cuda"
    _dispatch.GLOW_ACTNORM_RT = True  # the route under test is opt-in
    print(f"# median of {reps} alternating calls after {args.warmup} warm-up rounds; ns per row; [GPU kernels per call]")
    print("# bytes per row (rows through HBM, d = dim, b = ceil(d / 64) block rows of the weight-gradient pass):")
    print("#   forward   fused  8 d (u in, z out)            layers 20 d (Glow 8 d, ActNorm 8 d, log-prob 4 d)")
    print("#   backward  fused  8 d + 8 d b (grad_u pass: z in, grad_u out; sums pass: u and z per block row)")
    print("#             layers 36 d + 8 d b (log-prob 8 d, ActNorm 8 d + column sums 12 d, grad_x 8 d, grad_W 8 d b)")
    for dim in (int(v) for v in args.dims.split(",")):
        for rows in (int(v) for v in args.rows.split(",")):
            model = make_pair(dim, dev)
            x = torch.randn(rows, dim, device=dev, generator=torch.Generator(device=dev).manual_seed(rows + dim))
            with torch.no_grad():
                model.log_prob(x)  # ActNorm's data-dependent initialisation
            x.requires_grad_(True)
            routed = flows._pair_fusable(model.flows[1], model.flows[0], x) and flows._pair_route(model.flows[1], rows) == "rt"

            def run(fused, backward):
                def fn():
                    flows._NO_PAIR_FUSION_ENV = not fused
                    try:
                        lp = model.log_prob(x)
                        if backward:
                            (-lp.mean()).backward()
                    finally:
                        flows._NO_PAIR_FUSION_ENV = False
                return fn

            b = (dim + 63) // 64
            hbm = {("fused", False): 8 * dim, ("layers", False): 20 * dim, ("fused", True): 16 * dim + 8 * dim * b,
                   ("layers", True): 56 * dim + 8 * dim * b}
            for backward in (False, True):
                calls = {"fused": run(True, backward), "layers": run(False, backward), "layers'": run(False, backward)}
                ms = alternate(calls, reps, args.warmup)
                n_k = {k: None if args.no_launch_count else count_kernels(calls[k]) for k in ("fused", "layers")}
                ns = {k: v * 1e6 / rows for k, v in ms.items()}
                spread = abs(ns["layers"] - ns["layers'"])
                ref = min(ns["layers"], ns["layers'"])
                verdict = "fused wins" if ns["fused"] <= ref else "level" if ns["fused"] <= ref + spread else "fused LOSES"
                cells = " | ".join(f"{k} {ns[k]:8.3f}" for k in ("fused", "layers", "layers'"))
                kern = " ".join(f"{k} {'n/a' if n_k[k] is None else n_k[k]}" for k in ("fused", "layers"))
                print(f"dim {dim:5d} rows {rows:8d} {'fwd+bwd' if backward else 'fwd    '}: {cells} | spread {spread:6.3f}"
                      f" | kernels [{kern}] | bytes/row fused {hbm[('fused', backward)]} layers {hbm[('layers', backward)]}"
                      f" | {verdict}{'' if routed else '  (NOT routed to the fused pair)'}", flush=True)
            del model, x


if __name__ == "__main__":
    main()
