"""A 9-layer AffineHalfFlow model on the run-time-shaped kernels: one launch for the run (fuse_affine_runs on:
ahf_stack_rt) against one per layer (off: ahf_rt), alternating in one process -- ns per row and layer of model.inverse()
and of log_prob(return_sum=True).
usage: python3 tools/time_rt_stack.py [only the cases whose name contains this] [repetitions]

Training mode: forward + backward + FusedAdam step of -log_prob(x).mean() with the parameters in a FlatParameters buffer,
``fuse_rt_training`` on (one ahf_stack_rt + one ahf_bwd_stack_rt launch) against off (the layer-by-layer route, launch for
launch what it was before the switch existed), alternating in one process on one build: median, best and the spread
(10th .. 90th percentile) of the step time over the repetitions, after warm-up steps.
usage: python3 tools/time_rt_stack.py --train [filter] [repetitions]
       python3 tools/time_rt_stack.py --steps on|off [filter] [steps]   (that many steps one way, nothing else: for a
                                                                         kernel trace's launch counts)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import torch_mnf_amd as amd

MODE = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("--train", "--steps") else ""
ARGS = sys.argv[2:] if MODE else sys.argv[1:]
ROUTE = ARGS.pop(0) if MODE == "--steps" else ""
ONLY = ARGS[0] if ARGS else ""
REPS = int(ARGS[1]) if len(ARGS) > 1 else (15 if MODE == "--train" else 10 if MODE else 7)
DEV, LAYERS = "cuda", 9

# (dim, h_sizes, rows)
CASES = [
    (64, (24, 24), 262144), (64, (24, 24), 4096), (64, (64, 64, 64), 262144), (512, (24, 24, 24), 262144),
    (512, (64, 64, 64), 262144), (256, (200, 130, 40, 7), 262144), (128, (100,), 262144),
]


# training mode: (layers, dim, h_sizes, rows)
TRAIN_CASES = [
    (9, 64, (24, 24), 262144), (9, 64, (24, 24), 65536), (9, 64, (64, 64, 64), 262144), (9, 64, (64, 64, 64), 65536),
    (9, 512, (24, 24, 24), 262144), (3, 10, (16, 40), 262144),
]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps):
    """best and median of `reps` timings of each of `fns`, taken in turns (ms)"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(once(fn))
    return [(min(t), sorted(t)[len(t) // 2]) for t in times]


def training_model(layers, dim, hs, switch):
    torch.manual_seed(dim + len(hs))
    flows = [amd.AffineHalfFlow(dim, parity=bool(i % 2), h_sizes=hs) for i in range(layers)]
    if flows[0]._image_index_host() is not None:  # a shape with per-shape kernels: forced onto this tier
        for f in flows:
            f.force_generic = 2
    m = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)
    m.fuse_rt_training = switch
    opt = amd.FusedAdam(amd.FlatParameters(m), lr=1e-4)

    def step(x):
        opt.zero_grad()
        loss = -m.log_prob(x).mean()
        loss.backward()
        opt.step()

    return m, step


def train_mode():
    for layers, dim, hs, rows in TRAIN_CASES:
        name = f"{layers} x d={dim} {hs} rows={rows}"
        if ONLY not in name:
            continue
        x = torch.randn(rows, dim, device=DEV) * 0.5
        routes = [("on", True), ("off", False)] if MODE == "--train" else [(ROUTE, ROUTE == "on")]
        steps, kernels = [], []
        for _, switch in routes:
            m, step = training_model(layers, dim, hs, switch)
            steps.append(lambda step=step: step(x))
            if MODE == "--steps":
                continue
            lp = m.log_prob(x)
            k_fwd = amd.last_kernel()
            (-lp.mean()).backward()
            kernels.append(f"{k_fwd} / {amd.last_kernel()}")
            del lp
        if MODE == "--steps":
            for _ in range(REPS):
                steps[0]()
            torch.cuda.synchronize()
            print(f"{name}: {REPS} steps, fuse_rt_training {ROUTE}")
            continue
        for _ in range(3):  # warm-up: caches, allocator, clocks
            for fn in steps:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in steps]
        for _ in range(REPS):
            for k, fn in enumerate(steps):
                times[k].append(once(fn))
        cells = []
        for (label, _), t, kn in zip(routes, times, kernels):
            t = sorted(t)
            cells.append(f"{label:3s} median {t[len(t) // 2]:8.3f} best {t[0]:8.3f} p10..p90 {t[len(t) // 10]:8.3f}..{t[(9 * len(t)) // 10]:8.3f} ms"
                         f"  [{kn}]")
        med = [sorted(t)[len(t) // 2] for t in times]
        print(f"{name:44s} {cells[0]}\n{'':44s} {cells[1]}\n{'':44s} on / off = {med[0] / med[1]:.3f}  ({REPS} steps each, in turns)",
              flush=True)


if MODE:
    train_mode()
    sys.exit(0)

for dim, hs, rows in CASES:
    name = f"d={dim} {hs} rows={rows}"
    if ONLY not in name:
        continue
    torch.manual_seed(dim + len(hs))
    models = []
    for fused in (True, False):
        torch.manual_seed(dim + len(hs))
        flows = [amd.AffineHalfFlow(dim, parity=bool(i % 2), h_sizes=hs) for i in range(LAYERS)]
        if flows[0]._image_index_host() is not None:  # a shape with per-shape kernels: forced onto this tier
            for f in flows:
                f.force_generic = 2
        m = amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)
        m.fuse_affine_runs = fused
        models.append(m)
    x = torch.randn(rows, dim, device=DEV)
    per = 1e6 / (rows * LAYERS)  # ms -> ns per row and layer
    with torch.no_grad():
        names = []
        for m in models:
            m.inverse(x)
            names.append(amd.last_kernel())
        inv = alternate([lambda m=m: m.inverse(x) for m in models], REPS)
        lp = alternate([lambda m=m: m.log_prob(x, return_sum=True) for m in models], REPS)
    print(f"{name:40s} inverse  fused {inv[0][0] * per:7.4f} (median {inv[0][1] * per:7.4f})  unfused {inv[1][0] * per:7.4f} "
          f"(median {inv[1][1] * per:7.4f}) ns/row/layer  [{names[0]} / {names[1]}]")
    print(f"{'':40s} log_prob fused {lp[0][0] * per:7.4f} (median {lp[0][1] * per:7.4f})  unfused {lp[1][0] * per:7.4f} "
          f"(median {lp[1][1] * per:7.4f}) ns/row/layer  [epilogue fused: {models[0]._logprob_done} / {models[1]._logprob_done}]",
          flush=True)
