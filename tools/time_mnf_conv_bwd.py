#!/usr/bin/env python3
"""MNFConv2d forward + backward with the gradient convolutions on the library's own kernels (_dispatch.MNF_CONV_BWD_FUSED:
mnf_conv_bwd_weight and mnf_conv_bwd_input) against the parent route (the fused forward of _dispatch.MNF_CONV_FUSED with
aten's convolution_backward twice), through the Python layer with HIP events: MNF-LeNet's two convolutions at the
reference's batch size and at larger ones, and a whole MNFLeNet forward + backward.

tools/time_mnf_conv_fwd.py's protocol: the routes ALTERNATE inside one process (new, parent, parent again, new, ...), each
call timed by its own event pair; reported is the median over --reps timed calls (at least 15) after --warmup untimed
rounds, in microseconds per call.  The parent route is timed TWICE per round ("parent", "parent'"): the difference of the
two medians is the run-to-run spread, and a cell counts as won only if the new route beats BOTH parent medians by more than
it.  Next to each line: the GPU kernels of one call (torch.profiler, counted once outside the timing; n/a where the
profiler is not available).  Under each layer line a "parts" line times the backward piece by piece outside autograd: each
new entry alone against the aten launches it replaces.  MNF_CONV_FUSED is on for every timed call; both switches are the shipped ones (off) afterwards.

usage: time_mnf_conv_bwd.py [--batches 128,1024,8192] [--lenet-rows 128,4096] [--reps 15] [--warmup 3] [--no-launch-count]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from time_mnf_conv_fwd import LAYERS, alternate, count_kernels  # noqa: E402

import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402


def routed(bwd_fused, fn):
    """fn on the fused forward, its backward under the switch; both switches are the shipped ones (off) again afterwards."""
    def call():
        _dispatch.MNF_CONV_FUSED, _dispatch.MNF_CONV_BWD_FUSED = True, bwd_fused
        try:
            return fn()
        finally:
            _dispatch.MNF_CONV_FUSED = _dispatch.MNF_CONV_BWD_FUSED = False
    return call


def report(label, fn, reps, warmup, count):
    calls = {"new": routed(True, fn), "parent": routed(False, fn), "parent'": routed(False, fn)}
    us = {k: 1e3 * v for k, v in alternate(calls, reps, warmup).items()}
    n_k = {k: count_kernels(calls[k]) if count else None for k in ("new", "parent")}
    spread = abs(us["parent"] - us["parent'"])
    lo, hi = min(us["parent"], us["parent'"]), max(us["parent"], us["parent'"])
    verdict = "new wins" if us["new"] < lo - spread else "new LOSES" if us["new"] > hi + spread else "level"
    cells = " | ".join(f"{k} {us[k]:9.1f}" for k in ("new", "parent", "parent'"))
    kern = " ".join(f"{k} {'n/a' if n_k[k] is None else n_k[k]}" for k in ("new", "parent"))
    print(f"{label}: {cells} | spread {spread:7.1f} | kernels [{kern}] | {lo / us['new']:5.2f} x | {verdict}", flush=True)


def parts(n_in, n_out, k, size, batch, reps, warmup):
    """The backward of one layer call piece by piece, outside autograd: the two new entries against the launches they
    replace (aten's convolution_backward on (g, x, Wz); x * x and convolution_backward on (gv, x * x, W_var); the
    gx + 2 x gx2 epilogue), same protocol."""
    dev, lib = "cuda", amd._lib.load()
    torch.manual_seed(batch + n_out)
    x = torch.randn(batch, n_in, size, size, device=dev)
    wz, wv = 0.1 * torch.randn(n_out, n_in, k, k, device=dev), 1e-4 * torch.rand(n_out, n_in, k, k, device=dev)
    g = torch.randn(batch, n_out, size - k + 1, size - k + 1, device=dev)
    gv = 30 * torch.randn_like(g)
    need_x = n_in > 1
    n = wz.numel()
    n_ws = lib.mnf_mnf_conv_bwd_weight_workspace(batch, n_in, n_out, k, size, size)
    work, buf, gx = torch.empty(max(n_ws, 1), device=dev), torch.empty(2 * n + n_out, device=dev), torch.empty_like(x)
    stream = torch.cuda.current_stream().cuda_stream
    geometry = ([n_out], [1, 1], [0, 0], [1, 1], False, [0, 0], 1)
    conv_bwd = torch.ops.aten.convolution_backward
    gx12 = conv_bwd(g, x, wz, *geometry, [True, False, False])[0], conv_bwd(gv, x * x, wv, *geometry, [True, False, False])[0]
    calls = {
        "new weight": lambda: lib.mnf_mnf_conv_bwd_weight(
            x.data_ptr(), g.data_ptr(), gv.data_ptr(), buf.data_ptr(), buf.data_ptr() + 4 * n, buf.data_ptr() + 8 * n,
            work.data_ptr(), n_ws, batch, n_in, size, size, n_out, k, stream),
        "aten weight": lambda: (conv_bwd(g, x, wz, *geometry, [False, True, False]),
                                conv_bwd(gv, x * x, wv, *geometry, [False, True, True])),
    }
    if need_x and lib.mnf_mnf_conv_bwd_input_supported(n_in, n_out, k, size, size):
        calls["new input"] = lambda: lib.mnf_mnf_conv_bwd_input(
            x.data_ptr(), g.data_ptr(), gv.data_ptr(), wz.data_ptr(), wv.data_ptr(), gx.data_ptr(), batch, n_in, size, size,
            n_out, k, stream)
        calls["aten input"] = lambda: (conv_bwd(g, x, wz, *geometry, [True, False, False]),
                                       conv_bwd(gv, x * x, wv, *geometry, [True, False, False]),
                                       gx12[0] + 2 * x * gx12[1])
        calls["aten both"] = lambda: (conv_bwd(g, x, wz, *geometry, [True, True, False]),
                                      conv_bwd(gv, x * x, wv, *geometry, [True, True, True]), gx12[0] + 2 * x * gx12[1])
    us = {k_: 1e3 * v for k_, v in alternate(calls, reps, warmup).items()}
    print(f"  parts, MNFConv2d({n_in}, {n_out}, {k}) {size}x{size} batch {batch:5d}: "
          + " | ".join(f"{k_} {v:8.1f}" for k_, v in us.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,1024,8192")
    ap.add_argument("--lenet-rows", default="128,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    reps, dev = max(args.reps, 15), "cuda"
    count = not args.no_launch_count
    print(f"# forward + backward; median of {reps} alternating calls after {args.warmup} warm-up rounds; microseconds per "
          "call; [GPU kernels per call]; 'wins' = ahead of both parent medians by more than their difference", flush=True)
    lib = amd._lib.load()
    for (n_in, n_out, k), size in LAYERS:
        for batch in (int(v) for v in args.batches.split(",")):
            torch.manual_seed(n_out + batch)
            layer = amd.MNFConv2d(n_in, n_out, k).to(dev)
            x = torch.randn(batch, n_in, size, size, device=dev)
            x.requires_grad_(n_in > 1)  # the first convolution's input is data
            which = [name for name, q in (("weight", lib.mnf_mnf_conv_bwd_weight_supported),
                                          ("input", lib.mnf_mnf_conv_bwd_input_supported))
                     if q(n_in, n_out, k, size, size) and (name == "weight" or x.requires_grad)]

            def both():
                layer.zero_grad(set_to_none=True)
                x.grad = None
                layer.forward(x).sum().backward()

            report(f"MNFConv2d({n_in}, {n_out}, {k}) {size}x{size} batch {batch:5d} [{' + '.join(which) or 'none'}]", both, reps,
                   args.warmup, count)
            del layer, x
            parts(n_in, n_out, k, size, batch, reps, args.warmup)
    for rows in (int(v) for v in args.lenet_rows.split(",")):
        torch.manual_seed(rows)
        model = amd.MNFLeNet().to(dev)
        x = torch.randn(rows, 1, 28, 28, device=dev)

        def lenet():
            model.zero_grad(set_to_none=True)
            model(x).sum().backward()

        report(f"MNFLeNet forward + backward rows {rows:5d}              ", lenet, reps, args.warmup, count)
        del model, x


if __name__ == "__main__":
    main()
