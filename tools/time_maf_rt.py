#!/usr/bin/env python3
"""MAF's one-pass direction (MAF.inverse) per kernel route, through the layer with HIP events: the forward pass alone (no
gradients wanted), the backward pass alone and forward + backward (a training step's share of this layer: grad_x and the
parameter sums, with the gradient-scale launch the rt route needs) on the VALU kernel (force_generic = 1: maf_generic /
maf_bwd_generic) and on the run-time-shaped matrix-core kernels (force_generic = 2: maf_rt / maf_bwd_rt).

The routes ALTERNATE inside one process (valu, rt, valu, ...), each call timed by its own event pair; reported is the
median over --reps timed calls (at least 15) after --warmup untimed rounds, in ns per row, and which route wins.  A shape
outside the rt kernels' plan (the gradient kernel: widths up to 64, four layers) shows the VALU kernel on both sides,
marked; a shape the VALU kernel refuses (its masked weights must fit 144 KB of LDS) shows the rt route alone.

usage: time_maf_rt.py [--shapes "2:24,24,24;6:16,16;64:24,24,24;64:64,64;256:64"] [--rows 2048,8192,65536,262144]
                      [--reps 15] [--warmup 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torch_mnf_amd as amd  # noqa: E402

DEV = "cuda"


def layers_for(dim, h_sizes):
    """{route: layer}: one set of weights, two routes"""
    torch.manual_seed(dim + len(h_sizes))
    base = amd.MAF(dim, parity=True, h_sizes=h_sizes).to(DEV)
    out = {}
    for route, force in (("valu", 1), ("rt", 2)):
        f = amd.MAF(dim, parity=True, h_sizes=h_sizes).to(DEV)
        f.load_state_dict(base.state_dict())
        f.force_generic = force
        out[route] = f
    return out


def passes_for(layers, rows, dim):
    """{pass: {route: (prepare, timed)}} on fixed inputs; `kernels` collects the family each pass ran"""
    g = torch.Generator(device=DEV).manual_seed(rows + dim)
    x = torch.randn(rows, dim, device=DEV, generator=g)
    w_y = torch.randn(rows, dim, device=DEV, generator=g) / rows
    w_l = torch.randn(rows, device=DEV, generator=g) / rows
    kernels = {}

    def fwd(f):
        def timed(_):
            with torch.no_grad():
                f.inverse(x)
        return (lambda: None), timed

    def graph(f):
        f.zero_grad(set_to_none=True)
        y, ld = f.inverse(x.detach().requires_grad_(True))
        return y, ld

    def bwd(f):
        return (lambda: graph(f)), (lambda out: torch.autograd.backward(list(out), [w_y, w_l]))

    def both(f):
        return (lambda: None), (lambda _: torch.autograd.backward(list(graph(f)), [w_y, w_l]))

    out = {}
    for name, make in (("fwd", fwd), ("bwd", bwd), ("fwd+bwd", both)):
        out[name] = {route: make(f) for route, f in layers.items()}
    return out, kernels


def alternate(calls, reps, warmup, kernels, name):
    """{route: median ms}: the routes take turns, one timed call each per round"""
    calls = dict(calls)
    for _ in range(warmup):
        for route, (prepare, timed) in list(calls.items()):
            try:
                timed(prepare())
            except amd._lib.MnfHipError as err:  # (raised before any launch: the route has no kernel for the shape)
                assert err.code == amd._lib.MNF_ERR_UNSUPPORTED, err
                kernels[(name, route)] = "unsupported"
                del calls[route]
                continue
            torch.cuda.synchronize()
            kernels[(name, route)] = amd.last_kernel()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for route, (prepare, timed) in calls.items():
            state = prepare()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            timed(state)
            b.record()
            b.synchronize()
            times[route].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:24,24,24;6:16,16;64:24,24,24;64:64,64;256:64")
    ap.add_argument("--rows", default="2048,8192,65536,262144")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    reps = max(args.reps, 15)
    print(f"# MAF.inverse, force_generic = 1 (valu) against 2 (rt); median of {reps} alternating calls after {args.warmup} "
          f"warm-up rounds; ns per row", flush=True)
    for spec in args.shapes.split(";"):
        dim, hs = spec.split(":")
        dim, h_sizes = int(dim), tuple(int(v) for v in hs.split(","))
        layers = layers_for(dim, h_sizes)
        for rows in (int(v) for v in args.rows.split(",")):
            passes, kernels = passes_for(layers, rows, dim)
            for name, calls in passes.items():
                ms = alternate(calls, reps, max(args.warmup, 1), kernels, name)
                ns = {k: f"{ms[k] * 1e6 / rows:9.3f}" if k in ms else "      n/a" for k in ("valu", "rt")}
                ratio = f"{ms['valu'] / ms['rt']:6.2f}" if len(ms) == 2 else "   n/a"
                if "valu" not in ms:
                    verdict = "no VALU kernel for the shape: rt is the only route"
                elif not kernels[(name, "rt")].endswith("_rt"):
                    verdict = f"no rt kernel for the shape ({kernels[(name, 'rt')]})"
                else:
                    verdict = "rt wins" if ms["rt"] <= ms["valu"] else "rt LOSES"
                print(f"dim {dim:4d} h {str(h_sizes):14s} rows {rows:7d} {name:8s}: valu {ns['valu']} | rt {ns['rt']} | "
                      f"valu/rt {ratio}  {verdict}  [{kernels[(name, 'valu')]} | {kernels[(name, 'rt')]}]", flush=True)


if __name__ == "__main__":
    main()
