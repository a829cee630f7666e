#!/usr/bin/env python3
"""Glow's three row passes per kernel route, through the C ABI with HIP events: forward y = x @ W, grad_x = g @ W^T and
grad_W += x^T g on the per-shape kernel (where the dim has one), the run-time-shaped kernel (rt) and the VALU kernel.

The routes ALTERNATE inside one process (route A, route B, route C, route A, ...), each call timed by its own event pair;
reported is the median over --reps timed calls (at least 15) after --warmup untimed rounds, in ns per row, and for the rt
kernel its share of the bound: 8 dim bytes per row against 8 TB/s up to dim 64, 2 dim^2 flop per row against the fp32
matrix rate (155 TF) above.  The per-shape and VALU grad_x routes include the W^T copy (and the operand-image gather)
they need per call; the rt route reads W transposed itself.

usage: time_glow_rt.py [--dims 6,48,100,256] [--rows 512,2048,8192,65536] [--reps 15] [--warmup 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torch_mnf_amd import _lib  # noqa: E402
from torch_mnf_amd.flows import _linear_rows_image, _linear_rows_table  # noqa: E402

HBM_BYTES_PER_S, FP32_MATRIX_FLOPS = 8.0e12, 155.0e12


def bound_ns_per_row(dim):
    return 1e9 * (8.0 * dim / HBM_BYTES_PER_S if dim <= 64 else 2.0 * dim * dim / FP32_MATRIX_FLOPS)


def routes_for(lib, rows, dim, dev):
    """{pass: {route: callable}} on fixed buffers"""
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(dim)
    x = torch.randn(rows, dim, device=dev, generator=g)
    gy = torch.randn(rows, dim, device=dev, generator=g)
    W = torch.randn(dim, dim, device=dev, generator=g) / dim ** 0.5
    y, gW = torch.empty_like(x), torch.zeros_like(W)
    table = _linear_rows_table(lib, dim, x.device)
    n_ws = lib.mnf_linear_rows_bwd_weight_rt_workspace(rows, dim)
    work = torch.empty(max(n_ws, 1), device=dev)

    def ok(rc):
        assert rc == 0, rc

    def img(src, M):
        ok(lib.mnf_linear_rows_img(src.data_ptr(), _linear_rows_image(lib, M, table).data_ptr(), y.data_ptr(), rows, dim, st))

    out = {"fwd": {}, "grad_x": {}, "grad_W": {}}
    if table is not None:
        out["fwd"]["per-shape"] = lambda: img(x, W)
        out["grad_x"]["per-shape"] = lambda: img(gy, W.t().contiguous())
    if lib.mnf_linear_rows_rt_supported(dim):
        out["fwd"]["rt"] = lambda: ok(lib.mnf_linear_rows_rt(x.data_ptr(), W.data_ptr(), y.data_ptr(), rows, dim, 0, st))
        out["grad_x"]["rt"] = lambda: ok(lib.mnf_linear_rows_rt(gy.data_ptr(), W.data_ptr(), y.data_ptr(), rows, dim, 1, st))
        out["grad_W"]["rt"] = lambda: ok(lib.mnf_linear_rows_bwd_weight_rt(x.data_ptr(), gy.data_ptr(), gW.data_ptr(), rows,
                                                                           dim, work.data_ptr(), n_ws, st))
    out["fwd"]["valu"] = lambda: ok(lib.mnf_linear_rows(x.data_ptr(), W.data_ptr(), y.data_ptr(), rows, dim, st))
    out["grad_x"]["valu"] = lambda: ok(lib.mnf_linear_rows(gy.data_ptr(), W.t().contiguous().data_ptr(), y.data_ptr(), rows,
                                                           dim, st))
    # the entry the rt kernel stands beside: xtg32_mfma_kernel at dim = 32 ("per-shape"), the VALU kernel elsewhere
    out["grad_W"]["per-shape" if dim == 32 else "valu"] = lambda: ok(lib.mnf_linear_rows_bwd_weight(
        x.data_ptr(), gy.data_ptr(), gW.data_ptr(), rows, dim, st))
    return out


def alternate(calls, reps, warmup):
    """{route: median ms}: the routes take turns, one timed call each per round"""
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
    ap.add_argument("--dims", default="6,48,100,256")
    ap.add_argument("--rows", default="512,2048,8192,65536")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    reps = max(args.reps, 15)
    lib = _lib.load()
    print(f"# median of {reps} alternating calls after {args.warmup} warm-up rounds; ns per row (share of the rt bound)")
    for dim in (int(v) for v in args.dims.split(",")):
        for rows in (int(v) for v in args.rows.split(",")):
            for name, calls in routes_for(lib, rows, dim, "cuda").items():
                ms = alternate(calls, reps, args.warmup)
                cells = []
                for route in ("per-shape", "rt", "valu"):
                    if route in ms:
                        ns = ms[route] * 1e6 / rows
                        share = f" ({100 * bound_ns_per_row(dim) / ns:.0f} % of bound)" if route == "rt" else ""
                        cells.append(f"{route} {ns:9.3f}{share}")
                verdict = ""
                if "rt" in ms:  # against the kernel the parent dispatch runs for the shape
                    verdict = "  rt wins" if ms["rt"] <= ms.get("per-shape", ms.get("valu")) else "  rt LOSES"
                print(f"dim {dim:5d} rows {rows:8d} {name:7s}: " + " | ".join(cells) + verdict, flush=True)


if __name__ == "__main__":
    main()
