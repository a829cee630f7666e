#!/usr/bin/env python3
"""A training step's share of one MAF layer in its element-by-element direction (MAF.forward -- what IAF.inverse, the density
pass of an IAF, runs): forward + backward through the layer with HIP events, the forward pass on maf_seq_rt both times
(force_generic = 2), the backward pass on the parent's route (_dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = None: maf_bwd_generic)
against the matrix-core route (the constant 0: maf_seq_bwd_rt -- gradient scale, solve, second gradient scale, weight pass).
The method is tools/time_maf_rt.py's: the routes ALTERNATE inside one process (valu, rt, valu, ...), each call timed by its
own event pair; reported is the median over --reps timed calls (at least 15) after --warmup untimed rounds, in ns per row,
and which route wins.  Cotangents are those of a mean loss (~1 / rows).

--det ROWS adds the fixed-order form (mnf_maf_seq_bwd_rt_det) at that row count: MNF_DETERMINISTIC is read once per process,
so those cells run in a child process started with the switch set.

usage: time_maf_seq_bwd_rt.py [--shapes "2:24,24,24;6:16,16;64:24,24,24;64:64,64"] [--rows 2048,8192,65536] [--det 65536]
                              [--reps 15] [--warmup 3]
"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from time_maf_rt import DEV, alternate  # noqa: E402

import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402

ROUTES = (("valu", None), ("rt", 0))  # route -> _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS during its calls


def step_calls(layer, rows, dim):
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    z = torch.randn(rows, dim, device=DEV, generator=g)
    w_y = torch.randn(rows, dim, device=DEV, generator=g) / rows
    w_l = torch.randn(rows, device=DEV, generator=g) / rows

    def step(floor):
        def timed(_):
            _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = floor
            try:
                layer.zero_grad(set_to_none=True)
                y, ld = layer.forward(z.detach().requires_grad_(True))
                torch.autograd.backward([y, ld], [w_y, w_l])
            finally:
                _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = None
        return (lambda: None), timed

    return {route: step(floor) for route, floor in ROUTES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:24,24,24;6:16,16;64:24,24,24;64:64,64")
    ap.add_argument("--rows", default="2048,8192,65536")
    ap.add_argument("--det", default="65536", help="row counts of the fixed-order cells (a child process); '' for none")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    reps = max(args.reps, 15)
    det = amd.deterministic()
    if not det:
        print(f"# MAF.forward + backward, force_generic = 2, _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = None (valu) against 0 (rt); "
              f"median of {reps} alternating calls after {args.warmup} warm-up rounds; ns per row", flush=True)
    for spec in args.shapes.split(";"):
        dim, hs = spec.split(":")
        dim, h_sizes = int(dim), tuple(int(v) for v in hs.split(","))
        torch.manual_seed(dim + len(h_sizes))
        layer = amd.MAF(dim, parity=True, h_sizes=h_sizes).to(DEV)
        layer.force_generic = 2
        for rows in (int(v) for v in args.rows.split(",") if v):
            kernels = {}
            ms = alternate(step_calls(layer, rows, dim), reps, max(args.warmup, 1), kernels, "fwd+bwd")
            ns = {k: f"{ms[k] * 1e6 / rows:10.3f}" for k in ms}
            if not kernels[("fwd+bwd", "rt")].endswith("_rt"):
                verdict = f"no rt kernel for the shape ({kernels[('fwd+bwd', 'rt')]})"
            else:
                verdict = "rt wins" if ms["rt"] <= ms["valu"] else "rt LOSES"
            print(f"dim {dim:4d} h {str(h_sizes):14s} rows {rows:7d} fwd+bwd{' det' if det else '    '}: valu {ns['valu']} | "
                  f"rt {ns['rt']} | valu/rt {ms['valu'] / ms['rt']:7.2f}  {verdict}  "
                  f"[{kernels[('fwd+bwd', 'valu')]} | {kernels[('fwd+bwd', 'rt')]}]", flush=True)
    if not det and args.det:
        print("# the same under MNF_DETERMINISTIC=1 (rt: mnf_maf_seq_bwd_rt_det, fixed-order sums; valu: atomic sums, warns)",
              flush=True)
        env = dict(os.environ, MNF_DETERMINISTIC="1", PYTHONWARNINGS="ignore")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--shapes", args.shapes, "--rows", args.det, "--det", "",
                        "--reps", str(reps), "--warmup", str(args.warmup)], env=env, check=True)


if __name__ == "__main__":
    main()
