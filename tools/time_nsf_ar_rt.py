#!/usr/bin/env python3
"""NSF_AR's one-pass direction (NSF_AR.inverse: x -> z, the density pass) per kernel route, through the layer with HIP
events, forward pass only (no gradients wanted): the VALU kernel (force_generic = 1: nsf_ar_generic, a block-wide MLP per
element and a spline per row) against the matrix-core kernel (force_generic = 2: nsf_ar_rt).  The method is
tools/time_maf_rt.py's: the routes ALTERNATE inside one process (valu, rt, valu, ...), each call timed by its own event
pair; reported is the median over --reps timed calls (at least 15) after --warmup untimed rounds, in ns per row, and which
route wins.  A shape outside the kernel's plan shows the VALU kernel on both sides, marked.

usage: time_nsf_ar_rt.py [--shapes "2:8:16;6:5:8;16:8:8;64:5:8;64:8:16"] [--rows 2048,8192,65536,262144] [--reps 15]
                         [--warmup 3]        (a shape is dim:K:n_h)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from time_maf_rt import DEV, alternate  # noqa: E402
from torch_mnf_amd import synthetic as recipes  # noqa: E402


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


def inverse_calls(layers, rows, dim):
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    x = 1.4 * torch.randn(rows, dim, device=DEV, generator=g)

    def inv(f):
        def timed(_):
            with torch.no_grad():
                f.inverse(x)
        return (lambda: None), timed

    return {route: inv(f) for route, f in layers.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:8:16;6:5:8;16:8:8;64:5:8;64:8:16")
    ap.add_argument("--rows", default="2048,8192,65536,262144")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-header", action="store_true")
    args = ap.parse_args()
    reps = max(args.reps, 15)
    if not args.no_header:
        print(f"# NSF_AR.inverse (one pass), force_generic = 1 (valu) against 2 (rt); median of {reps} alternating calls after "
              f"{args.warmup} warm-up rounds; ns per row", flush=True)
    for spec in args.shapes.split(";"):
        dim, K, n_h = (int(v) for v in spec.split(":"))
        layers = layers_for(dim, K, n_h)
        for rows in (int(v) for v in args.rows.split(",")):
            kernels = {}
            ms = alternate(inverse_calls(layers, rows, dim), reps, max(args.warmup, 1), kernels, "inv")
            ns = {k: f"{ms[k] * 1e6 / rows:10.3f}" for k in ("valu", "rt")}
            if not kernels[("inv", "rt")].endswith("_rt"):
                verdict = f"no rt kernel for the shape ({kernels[('inv', 'rt')]})"
            else:
                verdict = "rt wins" if ms["rt"] <= ms["valu"] else "rt LOSES"
            print(f"dim {dim:4d} K {K:2d} n_h {n_h:2d} rows {rows:7d} inv: valu {ns['valu']} | rt {ns['rt']} | "
                  f"valu/rt {ms['valu'] / ms['rt']:7.2f}  {verdict}  [{kernels[('inv', 'valu')]} | {kernels[('inv', 'rt')]}]", flush=True)


if __name__ == "__main__":
    main()
