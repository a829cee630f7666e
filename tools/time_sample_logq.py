"""sample(n, seed=s, return_log_prob=True): the sample and its log-density, three routes in turns in one process,
microseconds per call (median and min / max of 15 alternating calls):

  (a) parent      what a user had to do before: ``x = model.sample(n, seed=s); lp = model.log_prob(x)`` -- a forward pass,
                  then every layer again in the inverse direction.  Timed twice per round (a, a'), for its own spread.
  (b) general     the new general route: ``mnf_normal_rows_sq`` (noise and its |z|^2), the forward pass without
                  intermediates, ``mnf_gauss_logq_sq``.  On a model with a one-launch route it is reached by switching that
                  launch off for the call (the code the model itself falls back to).
  (c) one launch  ``ahf_split_stack_sample_lq``: x and log_q out of the stack kernel, where the model has it.

Cells: c2's model (9 x AffineHalfFlow(64)) at 2^16 / 2^18 / 2^20 rows, c4's (9 x AffineHalfFlow(256)) at 2^19, the
run-time-shaped (64, (24, 24)) x 3 model at 2^18, c1's (9 x AffineHalfFlow(2)) at 4,096.

usage: python3 tools/time_sample_logq.py [output file, default profiles/r30/sample_logq_ab.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import torch_mnf_amd as amd
from torch_mnf_amd import synthetic

DEV, REPS, SEED = "cuda", 15, 0x9E3779B97F4A7C15
# (name, dim, h_sizes, layers, rows)
CELLS = [("c2", 64, (24, 24, 24), 9, 1 << 16), ("c2", 64, (24, 24, 24), 9, 1 << 18), ("c2", 64, (24, 24, 24), 9, 1 << 20),
         ("c4", 256, (24, 24, 24), 9, 1 << 19), ("rt (24, 24) x 3", 64, (24, 24), 3, 1 << 18), ("c1", 2, (24, 24, 24), 9, 4096)]


def model_for(dim, hs, n_layers):
    flows = []
    for i in range(n_layers):
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
    """(median, min, max) in us of `reps` timings of each of `fns`, taken in turns after three warm-up rounds"""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(once(fn))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r30", "sample_logq_ab.txt")
    cell = lambda r: f"{r[0]:9.1f} ({r[1]:8.1f} ..{r[2]:9.1f})"
    lines = [f"sample + log-density: us per call, median (min .. max) of {REPS} calls per route, the routes taken in turns",
             f"{'cell':30s} {'(a) sample; log_prob':>31s} {'(a) again':>31s} {'(b) general':>31s} {'(c) one launch':>31s}   b / a   c / a"]
    with torch.no_grad():
        for name, dim, hs, n_layers, rows in CELLS:
            model = model_for(dim, hs, n_layers)

            def parent():
                return model.log_prob(model.sample(rows, seed=SEED))

            def new():
                return model.sample(rows, seed=SEED, return_log_prob=True)

            x, lq = new()
            one = amd.last_kernel() == "ahf_split_stack_sample_lq"
            run = model._sample_run()

            def general():
                if not one:
                    return new()
                run.launch_sample_logq = lambda *a: None  # (the instance attribute shadows the method for this call)
                try:
                    return new()
                finally:
                    del run.launch_sample_logq

            xg, lqg = general()
            assert amd.last_kernel() not in ("ahf_split_stack_sample_lq", "ahf_split_stack_sample")
            assert torch.equal(xg, x)
            worst = float((lqg - lq).abs().max() / lq.abs().max())
            res = alternate([parent, parent, general] + ([new] if one else []))
            a = min(res[0][0], res[1][0])
            cells = [cell(r) for r in res] + ([] if one else [f"{'-':>31s}"])
            lines.append(f"{name + f' d={dim} rows={rows}':30s} " + " ".join(cells) + f"   {res[2][0] / a:5.3f}   "
                         + (f"{res[3][0] / a:5.3f}" if one else "    -") + f"   (log_q, b against c: {worst:.1e})")
            print(lines[-1], flush=True)
            del model
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
