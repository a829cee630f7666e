"""Sampling, three routes in turns in one process, microseconds per call (median of 15 alternating calls):

  parent      ``model.sample(n)``: torch.randn, then forward with every intermediate kept (what sample() has always done)
  general     the seeded general route: ``mnf_normal_rows`` writes the noise, then the pass without intermediates
  one-launch  the seeded one-launch route (``ahf_split_stack_sample``: the noise is generated inside the stack kernel)

Cells: c1's shape (9 x AffineHalfFlow(2)) at 4,096 rows, c2's (9 x AffineHalfFlow(64)) at 2^16, 2^18 and 2^20 rows, c4's
(9 x AffineHalfFlow(256)) at its 2^19 rows, and one run-time-shaped model (h_sizes = (24, 24), dim 64, 2^18 rows).  A model
without a sample launch (c1: halves narrower than a tile; the run-time-shaped one) has no one-launch cell.

usage: python3 tools/time_sample.py [output file, default profiles/r28/sample_ab.txt]
       python3 tools/time_sample.py --forward   (only: model.forward(z) of the c2 model at 2^20 rows -- the forward
                                                 instantiations fed a row tensor; runs on any build, for a parent / new A/B)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import torch_mnf_amd as amd
from torch_mnf_amd import synthetic

DEV, REPS, SEED = "cuda", 15, 0x9E3779B97F4A7C15
# (name, dim, h_sizes, rows)
CELLS = [("c1", 2, (24, 24, 24), 4096), ("c2", 64, (24, 24, 24), 1 << 16), ("c2", 64, (24, 24, 24), 1 << 18),
         ("c2", 64, (24, 24, 24), 1 << 20), ("c4", 256, (24, 24, 24), 1 << 19), ("rt (24, 24)", 64, (24, 24), 1 << 18)]


def model_for(dim, hs):
    flows = []
    for i in range(9):
        f = amd.AffineHalfFlow(dim, parity=bool(i % 2), h_sizes=hs)
        f.load_state_dict(synthetic.affine_half_params(1000 + i, dim, h_sizes=hs, s_last_gain=2.0))
        flows.append(f)
    return amd.NormalizingFlowModel(amd.StandardNormal(dim, DEV), flows).to(DEV)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b)


def alternate(fns, reps=REPS):
    """(median, best) in us of `reps` timings of each of `fns`, taken in turns after three warm-up rounds"""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(once(fn))
    return [(sorted(t)[len(t) // 2], min(t)) for t in times]


def forward_only():
    model = model_for(64, (24, 24, 24))
    z = torch.randn(1 << 20, 64, device=DEV)
    with torch.no_grad():
        (med, best), = alternate([lambda: model.forward(z)])
    print(f"c2 model.forward(z) at 2^20 rows [{amd.last_kernel()}]: median {med:9.1f} us  best {best:9.1f} us  ({REPS} calls)")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r28", "sample_ab.txt")
    lines = [f"sample(): us per call, median (best) of {REPS} calls per route, the routes taken in turns",
             f"{'cell':28s} {'parent sample(n)':>24s} {'seeded, general':>24s} {'seeded, one launch':>24s}   one launch / parent"]
    with torch.no_grad():
        for name, dim, hs, rows in CELLS:
            model = model_for(dim, hs)

            def general():
                z = model.base.sample((rows,), seed=SEED)
                return model._pass(z, False, last_only=True)[0][-1]

            fns = [lambda: model.sample(rows), general]
            model.sample(rows, seed=SEED)
            one = amd.last_kernel() == "ahf_split_stack_sample"
            if one:
                fns.append(lambda: model.sample(rows, seed=SEED))
                assert torch.equal(model.sample(rows, seed=SEED), general())
            res = alternate(fns)
            cells = [f"{m:12.1f} ({b:9.1f})" for m, b in res] + ([] if one else [f"{'-':>24s}"])
            ratio = f"{res[2][0] / res[0][0]:.3f}" if one else f"(general / parent {res[1][0] / res[0][0]:.3f})"
            lines.append(f"{name + f' d={dim} rows={rows}':28s} " + " ".join(cells) + f"   {ratio}")
            print(lines[-1], flush=True)
            del model
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    forward_only() if "--forward" in sys.argv[1:] else main()
