#!/usr/bin/env python3
"""A training step's share of one NSF_AR layer in its one-pass direction (NSF_AR.inverse: x -> z, the density pass): forward +
backward through the layer with HIP events, the forward pass on nsf_ar_rt both times (force_generic = 2), the backward pass
on the parent's route (_dispatch.NSF_AR_BWD_RT_MIN_ROWS = None: nsf_ar_bwd_generic) against the matrix-core route (the
constant 0: nsf_ar_bwd_rt), in the same build.  The method is tools/time_maf_rt.py's: the routes ALTERNATE inside one
process (valu, rt, valu, ...), each call timed by its own event pair; reported is the median over --reps timed calls (at
least 15) after --warmup untimed rounds, in ns per row, and which route wins.  Cotangents are those of a mean loss
(~1 / rows).  One process per shape (a child each), so that no shape inherits another's allocator or clock state.

--det ROWS adds the fixed-order form (mnf_nsf_ar_bwd_rt_det) at that row count: MNF_DETERMINISTIC is read once per process,
so those cells run in child processes started with the switch set.

usage: time_nsf_ar_bwd_rt.py [--shapes "2:8:16;6:5:8;16:8:8;64:5:8;64:8:16"] [--rows 2048,8192,65536,262144] [--det 65536]
                             [--reps 15] [--warmup 3]        (a shape is dim:K:n_h)
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
from torch_mnf_amd import synthetic as recipes  # noqa: E402

ROUTES = (("valu", None), ("rt", 0))  # route -> _dispatch.NSF_AR_BWD_RT_MIN_ROWS during its calls


def step_calls(layer, rows, dim):
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    x = 1.4 * torch.randn(rows, dim, device=DEV, generator=g)
    w_y = torch.randn(rows, dim, device=DEV, generator=g) / rows
    w_l = torch.randn(rows, device=DEV, generator=g) / rows

    def step(floor):
        def timed(_):
            _dispatch.NSF_AR_BWD_RT_MIN_ROWS = floor
            try:
                layer.zero_grad(set_to_none=True)
                z, ld = layer.inverse(x.detach().requires_grad_(True))
                torch.autograd.backward([z, ld], [w_y, w_l])
            finally:
                _dispatch.NSF_AR_BWD_RT_MIN_ROWS = None
        return (lambda: None), timed

    return {route: step(floor) for route, floor in ROUTES}


def one_shape(spec, rows_list, reps, warmup):
    det = amd.deterministic()
    dim, K, n_h = (int(v) for v in spec.split(":"))
    layer = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
    layer.load_state_dict(recipes.nsf_ar_params(3100 + dim + K, dim, K, n_h))
    layer.force_generic = 2
    layer.to(DEV)
    for rows in rows_list:
        kernels = {}
        ms = alternate(step_calls(layer, rows, dim), reps, max(warmup, 1), kernels, "fwd+bwd")
        ns = {k: f"{ms[k] * 1e6 / rows:10.3f}" for k in ms}
        if not kernels[("fwd+bwd", "rt")].endswith("_rt"):
            verdict = f"no rt kernel for the shape ({kernels[('fwd+bwd', 'rt')]})"
        else:
            verdict = "rt wins" if ms["rt"] <= ms["valu"] else "rt LOSES"
        print(f"dim {dim:4d} K {K:2d} n_h {n_h:2d} rows {rows:7d} fwd+bwd{' det' if det else '    '}: valu {ns['valu']} | "
              f"rt {ns['rt']} | valu/rt {ms['valu'] / ms['rt']:7.2f}  {verdict}  "
              f"[{kernels[('fwd+bwd', 'valu')]} | {kernels[('fwd+bwd', 'rt')]}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:8:16;6:5:8;16:8:8;64:5:8;64:8:16")
    ap.add_argument("--rows", default="2048,8192,65536,262144")
    ap.add_argument("--det", default="65536", help="row counts of the fixed-order cells (child processes); '' for none")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one-shape", default="", help="(internal) time this shape in this process")
    args = ap.parse_args()
    reps = max(args.reps, 15)
    if args.one_shape:
        one_shape(args.one_shape, [int(v) for v in args.rows.split(",") if v], reps, args.warmup)
        return

    def children(rows, env):
        for spec in args.shapes.split(";"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one-shape", spec, "--rows", rows, "--reps", str(reps),
                            "--warmup", str(args.warmup)], env=env, check=True)

    print(f"# NSF_AR.inverse + backward, force_generic = 2, _dispatch.NSF_AR_BWD_RT_MIN_ROWS = None (valu) against 0 (rt); "
          f"median of {reps} alternating calls after {args.warmup} warm-up rounds; ns per row", flush=True)
    children(args.rows, dict(os.environ))
    if args.det:
        print("# the same under MNF_DETERMINISTIC=1 (rt: mnf_nsf_ar_bwd_rt_det, fixed-order sums; valu: atomic sums, warns)",
              flush=True)
        children(args.det, dict(os.environ, MNF_DETERMINISTIC="1", PYTHONWARNINGS="ignore"))


if __name__ == "__main__":
    main()
