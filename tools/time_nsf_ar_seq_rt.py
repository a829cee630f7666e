#!/usr/bin/env python3
"""NSF_AR's element-by-element direction (NSF_AR.forward: z -> x, what sampling runs through) per kernel route, through the
layer with HIP events under no_grad: the VALU kernel (force_generic = 1: nsf_ar_generic, a block-wide MLP per element and
a spline per row) against the matrix-core kernel nsf_ar_seq_rt (_dispatch.NSF_AR_SEQ_RT_MIN_ROWS set for the run,
force_generic = 2).  The method is tools/time_nsf_ar_rt.py's: the routes ALTERNATE inside one process (valu, rt, valu,
...), each call timed by its own event pair; reported per route are the median, the minimum and the maximum over --reps
timed calls (at least 15) after --warmup untimed rounds, in ns per row, and whether the new route wins by more than the
VALU kernel's own min-max spread.  A shape outside the kernel's plan shows the VALU kernel on both sides, marked.

usage: time_nsf_ar_seq_rt.py [--shapes "2:8:16;6:5:8;16:8:8;64:5:8;64:8:16"] [--rows 2048,8192,65536,262144] [--reps 15]
                             [--warmup 3] [--no-header]        (a shape is dim:K:n_h)

The tiles-per-wave choice is a compile-time constant of the kernel (csrc/mnf_nsf_ar_seq_rt.hip MNF_NSF_AR_SEQ_TILES): time a
library built with another value by pointing MNF_LIB_PATH at it.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402
from torch_mnf_amd import synthetic as recipes  # noqa: E402

DEV = "cuda"


def layers_for(dim, K, n_h):
    """{"valu": layer, "rt": layer}: the same parameters under force_generic = 1 / 2"""
    sd = recipes.nsf_ar_params(3100 + dim + K, dim, K, n_h)
    layers = {}
    for route, force in (("valu", 1), ("rt", 2)):
        f = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
        f.load_state_dict(sd)
        f.force_generic = force
        layers[route] = f.to(DEV)
    return layers


def alternate(layers, z, reps, warmup):
    """({route: [ms, ...]}, {route: kernel family}): the routes take turns, one timed call each per round"""
    kernels, times = {}, {route: [] for route in layers}
    with torch.no_grad():
        for _ in range(warmup):
            for route, f in layers.items():
                f.forward(z)
                torch.cuda.synchronize()
                kernels[route] = amd.last_kernel()
        for _ in range(reps):
            for route, f in layers.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f.forward(z)
                b.record()
                b.synchronize()
                times[route].append(a.elapsed_time(b))
    return times, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:8:16;6:5:8;16:8:8;64:5:8;64:8:16")
    ap.add_argument("--rows", default="2048,8192,65536,262144")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-header", action="store_true")
    args = ap.parse_args()
    reps = max(args.reps, 15)
    _dispatch.NSF_AR_SEQ_RT_MIN_ROWS = 1  # the route is opt-in as shipped
    if not args.no_header:
        print(f"# NSF_AR.forward (element by element), force_generic = 1 (valu) against NSF_AR_SEQ_RT_MIN_ROWS set + force_generic = 2 "
              f"(rt); median [min .. max] of {reps} alternating calls after {args.warmup} warm-up rounds; ns per row", flush=True)
    for spec in args.shapes.split(";"):
        dim, K, n_h = (int(v) for v in spec.split(":"))
        layers = layers_for(dim, K, n_h)
        for rows in (int(v) for v in args.rows.split(",")):
            g = torch.Generator(device=DEV).manual_seed(rows + dim)
            z = 1.4 * torch.randn(rows, dim, device=DEV, generator=g)
            times, kernels = alternate(layers, z, reps, max(args.warmup, 1))
            ns = {k: [t * 1e6 / rows for t in v] for k, v in times.items()}
            med = {k: statistics.median(v) for k, v in ns.items()}
            cell = {k: f"{med[k]:9.3f} [{min(ns[k]):9.3f} .. {max(ns[k]):9.3f}]" for k in ns}
            spread = max(ns["valu"]) - min(ns["valu"])
            if not kernels["rt"].endswith("_rt"):
                verdict = f"no rt kernel for the shape ({kernels['rt']})"
            elif med["valu"] - med["rt"] > spread:
                verdict = "rt wins by more than the valu spread"
            else:
                verdict = "rt wins inside the valu spread" if med["rt"] <= med["valu"] else "rt LOSES"
            print(f"dim {dim:4d} K {K:2d} n_h {n_h:2d} rows {rows:7d} fwd: valu {cell['valu']} | rt {cell['rt']} | "
                  f"valu/rt {med['valu'] / med['rt']:7.2f}  {verdict}  [{kernels['valu']} | {kernels['rt']}]", flush=True)


if __name__ == "__main__":
    main()
