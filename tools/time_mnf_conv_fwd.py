#!/usr/bin/env python3
"""MNFConv2d.forward on the fused route (_dispatch.MNF_CONV_FUSED: one mnf_conv_fwd launch behind sample_z and the operand
launch) against the route of today (two MIOpen convolutions, the x * x launch, the noise launch), through the Python layer
with HIP events: MNF-LeNet's two convolutions at the reference's batch size and at prediction batch sizes, forward under
no_grad and forward + backward, and a whole MNFLeNet forward.

The routes ALTERNATE inside one process (fused, miopen, miopen again, fused, ...), each call timed by its own event pair;
reported is the median over --reps timed calls (at least 15) after --warmup untimed rounds, in microseconds per call.  The
current route is timed TWICE per round ("miopen", "miopen'"): the difference of the two medians is the run-to-run spread
the verdict allows the fused route.  Next to each line: the GPU kernels of one call (torch.profiler, counted once outside
the timing; n/a where the profiler is not available).

usage: time_mnf_conv_fwd.py [--batches 128,1024,8192] [--lenet-rows 128,4096] [--reps 15] [--warmup 3] [--no-launch-count]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402

LAYERS = (((1, 20, 5), 28), ((20, 50, 5), 12))  # MNF-LeNet's convolutions and their input sizes


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


def routed(fused, fn):
    """fn under the switch; the switch is the shipped one (off) again afterwards."""
    def call():
        _dispatch.MNF_CONV_FUSED = fused
        try:
            return fn()
        finally:
            _dispatch.MNF_CONV_FUSED = False
    return call


def report(label, calls, reps, warmup, count):
    us = {k: 1e3 * v for k, v in alternate(calls, reps, warmup).items()}
    n_k = {k: count_kernels(calls[k]) if count else None for k in ("fused", "miopen")}
    spread = abs(us["miopen"] - us["miopen'"])
    ref = min(us["miopen"], us["miopen'"])
    verdict = "fused wins" if us["fused"] < ref - spread else "level" if us["fused"] <= ref + spread else "fused LOSES"
    cells = " | ".join(f"{k} {us[k]:9.1f}" for k in ("fused", "miopen", "miopen'"))
    kern = " ".join(f"{k} {'n/a' if n_k[k] is None else n_k[k]}" for k in ("fused", "miopen"))
    print(f"{label}: {cells} | spread {spread:7.1f} | kernels [{kern}] | {ref / us['fused']:5.2f} x | {verdict}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,1024,8192")
    ap.add_argument("--lenet-rows", default="128,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    reps, dev = max(args.reps, 15), "cuda"
    print(f"# median of {reps} alternating calls after {args.warmup} warm-up rounds; microseconds per call; "
          "[GPU kernels per call]; 'wins' = ahead of the faster miopen median by more than the spread", flush=True)
    for (n_in, n_out, k), size in LAYERS:
        for batch in (int(v) for v in args.batches.split(",")):
            torch.manual_seed(n_out + batch)
            layer = amd.MNFConv2d(n_in, n_out, k).to(dev)
            x = torch.randn(batch, n_in, size, size, device=dev)
            x.requires_grad_(n_in > 1)  # the first convolution's input is data
            lib = amd._lib.load()
            note = "" if lib.mnf_mnf_conv_fwd_supported(n_in, n_out, k, size, size) else "  (NOT routed to the fused kernel)"

            def forward():
                with torch.no_grad():
                    return layer.forward(x)

            def both():
                layer.zero_grad(set_to_none=True)
                x.grad = None
                layer.forward(x).sum().backward()

            for name, fn in (("fwd    ", forward), ("fwd+bwd", both)):
                calls = {"fused": routed(True, fn), "miopen": routed(False, fn), "miopen'": routed(False, fn)}
                report(f"MNFConv2d({n_in}, {n_out}, {k}) {size}x{size} batch {batch:5d} {name}{note}", calls, reps,
                       args.warmup, not args.no_launch_count)
            del layer, x
    for rows in (int(v) for v in args.lenet_rows.split(",")):
        torch.manual_seed(rows)
        model = amd.MNFLeNet().to(dev)
        x = torch.randn(rows, 1, 28, 28, device=dev)

        def lenet():
            with torch.no_grad():
                return model(x)

        calls = {"fused": routed(True, lenet), "miopen": routed(False, lenet), "miopen'": routed(False, lenet)}
        report(f"MNFLeNet forward (no_grad) rows {rows:5d}        ", calls, reps, args.warmup, not args.no_launch_count)
        del model, x


if __name__ == "__main__":
    main()
