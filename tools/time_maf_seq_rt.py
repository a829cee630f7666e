#!/usr/bin/env python3
"""MAF's element-by-element direction (MAF.forward: sampling) per kernel route, through the layer with HIP events, forward
pass only (no gradients wanted): the VALU kernel (force_generic = 1: maf_generic, a thread per row, dim net evaluations
each) against the matrix-core kernel (force_generic = 2: maf_seq_rt).  The method is tools/time_maf_rt.py's: the routes
ALTERNATE inside one process (valu, rt, valu, ...), each call timed by its own event pair; reported is the median over
--reps timed calls (at least 15) after --warmup untimed rounds, in ns per row, and which route wins.  A shape outside
the kernel's plan (a net that does not stay resident in LDS) shows the VALU kernel on both sides, marked.

usage: time_maf_seq_rt.py [--shapes "2:24,24,24;6:16,16;64:24,24,24;64:64,64"] [--rows 2048,8192,65536] [--reps 15]
                          [--warmup 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from time_maf_rt import DEV, alternate, layers_for  # noqa: E402


def forward_calls(layers, rows, dim):
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    z = torch.randn(rows, dim, device=DEV, generator=g)

    def fwd(f):
        def timed(_):
            with torch.no_grad():
                f.forward(z)
        return (lambda: None), timed

    return {route: fwd(f) for route, f in layers.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:24,24,24;6:16,16;64:24,24,24;64:64,64")
    ap.add_argument("--rows", default="2048,8192,65536")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    reps = max(args.reps, 15)
    print(f"# MAF.forward (element by element), force_generic = 1 (valu) against 2 (rt); median of {reps} alternating calls "
          f"after {args.warmup} warm-up rounds; ns per row", flush=True)
    for spec in args.shapes.split(";"):
        dim, hs = spec.split(":")
        dim, h_sizes = int(dim), tuple(int(v) for v in hs.split(","))
        layers = layers_for(dim, h_sizes)
        for rows in (int(v) for v in args.rows.split(",")):
            kernels = {}
            ms = alternate(forward_calls(layers, rows, dim), reps, max(args.warmup, 1), kernels, "fwd")
            ns = {k: f"{ms[k] * 1e6 / rows:10.3f}" if k in ms else "       n/a" for k in ("valu", "rt")}
            ratio = f"{ms['valu'] / ms['rt']:7.2f}" if len(ms) == 2 else "    n/a"
            if "valu" not in ms:
                verdict = "no VALU kernel for the shape: rt is the only route"
            elif not kernels[("fwd", "rt")].endswith("_rt"):
                verdict = f"no rt kernel for the shape ({kernels[('fwd', 'rt')]})"
            else:
                verdict = "rt wins" if ms["rt"] <= ms["valu"] else "rt LOSES"
            print(f"dim {dim:4d} h {str(h_sizes):14s} rows {rows:7d} fwd: valu {ns['valu']} | rt {ns['rt']} | "
                  f"valu/rt {ratio}  {verdict}  [{kernels[('fwd', 'valu')]} | {kernels[('fwd', 'rt')]}]", flush=True)


if __name__ == "__main__":
    main()
