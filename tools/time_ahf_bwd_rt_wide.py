#!/usr/bin/env python3
"""A training step's share of one AffineHalfFlow layer whose widest hidden layer has 65 .. 128 units: forward + backward
through the layer with HIP events, the forward pass on ahf_rt both times (default dispatch: no per-shape kernel, >= 2,048
rows), the backward pass on the parent's route (_dispatch.AHF_BWD_RT_WIDE_MIN_ROWS = None: ahf_bwd_generic) against the
matrix-core route (the constant 0: ahf_bwd_rt's wide instantiation), in the same build and the same process.  The method is
tools/time_nsf_ar_seq_rt.py's: the routes ALTERNATE (valu, rt, valu, ...), each call timed by its own event pair; reported
are the median, minimum and maximum over --reps timed calls (at least 15) after --warmup untimed rounds, in ns per row, and
whether the route wins by more than the min-max spread of the VALU side's timings.  Cotangents are those of a mean loss
(~1 / rows).  One process per shape (a child each), so that no shape inherits another's allocator or clock state.

--det ROWS adds the fixed-order form (mnf_affine_half_bwd_rt_wide_det) at that row count: MNF_DETERMINISTIC is read once per
process, so those cells run in child processes started with the switch set.

--lib LABEL=PATH[;LABEL=PATH] repeats the whole table for other builds of the library, loaded through MNF_LIB_PATH: the wide
instantiation's launch bounds are a compile-time choice (-DMNF_AHF_BWD_RT_WIDE_THREADS=512 / 256 on mnf_ahf_bwd_rt.hip),
and one library holds one of them.  An empty PATH is the tree's own library.

usage: time_ahf_bwd_rt_wide.py [--shapes "64:128;64:96,96;64:128,128,128;512:128,128"] [--rows 2048,8192,65536,262144]
                               [--det 65536] [--reps 15] [--warmup 3] [--lib "512=;256=/path/libmnf_hip.so"]
"""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402
from torch_mnf_amd import synthetic as recipes  # noqa: E402

DEV = "cuda"
ROUTES = (("valu", None), ("rt", 0))  # route -> _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS during its calls


def alternate(layer, rows, dim, reps, warmup):
    """({route: [ms, ...]}, {route: the gradient kernel's family})"""
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    x = torch.randn(rows, dim, device=DEV, generator=g)
    w_y = torch.randn(rows, dim, device=DEV, generator=g) / rows
    w_l = torch.randn(rows, device=DEV, generator=g) / rows

    def step(floor):
        _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS = floor
        try:
            layer.zero_grad(set_to_none=True)
            z, ld = layer.forward(x.detach().requires_grad_(True), inverse=True)
            torch.autograd.backward([z, ld], [w_y, w_l])
        finally:
            _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS = None

    kernels, times = {}, {route: [] for route, _ in ROUTES}
    for _ in range(warmup):
        for route, floor in ROUTES:
            step(floor)
            torch.cuda.synchronize()
            kernels[route] = amd.last_kernel()
    for _ in range(reps):
        for route, floor in ROUTES:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(floor)
            b.record()
            b.synchronize()
            times[route].append(a.elapsed_time(b))
    return times, kernels


def one_shape(spec, rows_list, reps, warmup):
    det = amd.deterministic()
    dim, hs = spec.split(":")
    dim, h_sizes = int(dim), tuple(int(v) for v in hs.split(","))
    layer = amd.AffineHalfFlow(dim, parity=False, h_sizes=h_sizes)
    layer.load_state_dict(recipes.affine_half_params(3100 + dim, dim, h_sizes=h_sizes))
    layer.to(DEV)
    for rows in rows_list:
        times, kernels = alternate(layer, rows, dim, reps, max(warmup, 1))
        ns = {k: [t * 1e6 / rows for t in v] for k, v in times.items()}
        med = {k: statistics.median(v) for k, v in ns.items()}
        cell = {k: f"{med[k]:9.3f} [{min(ns[k]):9.3f} .. {max(ns[k]):9.3f}]" for k in ns}
        spread = max(ns["valu"]) - min(ns["valu"])
        if kernels["rt"] != "ahf_bwd_rt":
            verdict = f"no rt kernel for the shape ({kernels['rt']})"
        elif med["valu"] - med["rt"] > spread:
            verdict = "rt wins by more than the valu spread"
        else:
            verdict = "rt wins inside the valu spread" if med["rt"] <= med["valu"] else "rt LOSES"
        print(f"dim {dim:4d} h {hs:12s} rows {rows:7d} fwd+bwd{' det' if det else '    '}: valu {cell['valu']} | rt {cell['rt']} | "
              f"valu/rt {med['valu'] / med['rt']:7.2f}  {verdict}  [{kernels['valu']} | {kernels['rt']}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64:128;64:96,96;64:128,128,128;512:128,128")
    ap.add_argument("--rows", default="2048,8192,65536,262144")
    ap.add_argument("--det", default="65536", help="row counts of the fixed-order cells (child processes); '' for none")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default="", help="LABEL=PATH;... : other builds of the library (MNF_LIB_PATH); '' = this tree's")
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

    print(f"# AffineHalfFlow.forward(inverse=True) + backward, _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS = None (valu) against 0 (rt); "
          f"median [min .. max] of {reps} alternating calls after {args.warmup} warm-up rounds; ns per row", flush=True)
    for build in (args.lib.split(";") if args.lib else ["="]):
        label, _, path = build.partition("=")
        env = dict(os.environ)
        if path:
            env["MNF_LIB_PATH"] = path
        if label:
            print(f"## build {label}: {path or 'the tree library'}", flush=True)
        children(args.rows, env)
        if args.det:
            print("# the same under MNF_DETERMINISTIC=1 (rt: mnf_affine_half_bwd_rt_wide_det, fixed-order sums; valu: atomic sums, "
                  "warns)", flush=True)
            children(args.det, dict(env, MNF_DETERMINISTIC="1", PYTHONWARNINGS="ignore"))


if __name__ == "__main__":
    main()
