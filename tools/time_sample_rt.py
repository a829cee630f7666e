"""Seeded sampling of a model on the run-time-shaped tier: the general route (``mnf_normal_rows(_sq)`` writes the noise,
``ahf_stack_rt`` reads it back; with log-q also ``mnf_gauss_logq_sq``) against the one launch whose first layer generates
its rows (``ahf_stack_rt_sample`` / ``ahf_stack_rt_sample_lq``), microseconds per call.

Every figure comes from a FRESH process that holds one model and one setting of ``_dispatch.RT_SAMPLE_MIN_ROWS``: per
model the processes run off, on, off, on -- the general route (what the parent commit runs: the switch off) is so timed
twice, for its own spread, with the new route in between -- and each times every row count of the model, x-only and with
log-q: the median of 15 calls after three warm-up calls.

Cells (every row count is one the tier takes by itself, from RT_MIN_ROWS):
  (64, (24, 24)) x 3 and x 9 layers at 4,096 / 2^16 / 2^18 / 2^20 rows; c6's model (dim 512, 9 layers) at 2^16 / 2^18;
  (6, (8,)) x 3 (odd half, the narrowest plan) at 4,096 / 2^16.

usage: python3 tools/time_sample_rt.py [output file, default profiles/r31/sample_rt_ab.txt]
       python3 tools/time_sample_rt.py --child MODEL on|off      (one process of the above; prints one JSON line)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, SEED = 15, 0x9E3779B97F4A7C15
# name: (dim, h_sizes, layers, row counts)
MODELS = {
    "(64, (24, 24)) x 3": (64, (24, 24), 3, (4096, 1 << 16, 1 << 18, 1 << 20)),
    "(64, (24, 24)) x 9": (64, (24, 24), 9, (4096, 1 << 16, 1 << 18, 1 << 20)),
    "c6 (512, (24, 24, 24)) x 9": (512, (24, 24, 24), 9, (1 << 16, 1 << 18)),
    "(6, (8,)) x 3": (6, (8,), 3, (4096, 1 << 16)),
}
NEW = ("ahf_stack_rt_sample", "ahf_stack_rt_sample_lq")


def child(name, switch):
    import torch

    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch, synthetic

    dim, hs, n_layers, row_counts = MODELS[name]
    _dispatch.RT_SAMPLE_MIN_ROWS = _dispatch.RT_MIN_ROWS if switch == "on" else None
    flows = []
    for i in range(n_layers):
        f = amd.AffineHalfFlow(dim, parity=bool(i % 2), h_sizes=hs)
        f.load_state_dict(synthetic.affine_half_params(1000 + i, dim, h_sizes=hs, s_last_gain=2.0))
        flows.append(f)
    model = amd.NormalizingFlowModel(amd.StandardNormal(dim, "cuda"), flows).to("cuda")
    out = {}
    with torch.no_grad():
        for rows in row_counts:
            for form, fn in (("x", lambda: model.sample(rows, seed=SEED)),
                             ("lq", lambda: model.sample(rows, seed=SEED, return_log_prob=True))):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                assert (amd.last_kernel() in NEW) == (switch == "on"), amd.last_kernel()
                times = []
                for _ in range(REPS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    times.append(1e3 * a.elapsed_time(b))
                out[f"{rows} {form}"] = sorted(times)[REPS // 2]
    print(json.dumps(out), flush=True)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r31", "sample_rt_ab.txt")
    lines = [f"seeded sample on the run-time-shaped tier: us per call, median of {REPS} calls, one fresh process per column",
             "general = RT_SAMPLE_MIN_ROWS None (the parent commit's route), one launch = ahf_stack_rt_sample(_lq); verdict against",
             "the two general columns: won (below both), level (between them or within their spread of the nearer), LOST",
             f"{'cell':44s} {'general':>10s} {'one launch':>10s} {'general':>10s} {'one launch':>10s}   new / old  verdict"]
    for name, (dim, hs, n_layers, row_counts) in MODELS.items():
        cols = []
        for switch in ("off", "on", "off", "on"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, switch], capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:  # (a process that failed ends the measurement: nothing more is started on the device)
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"{name} {switch}: exit status {p.returncode}")
            cols.append(json.loads(p.stdout.strip().splitlines()[-1]))
        for rows in row_counts:
            for form in ("x", "lq"):
                g0, n0, g1, n1 = (c[f"{rows} {form}"] for c in cols)
                spread, new, old = abs(g0 - g1), 0.5 * (n0 + n1), 0.5 * (g0 + g1)
                verdict = "won" if max(n0, n1) < min(g0, g1) else "level" if new <= max(g0, g1) + spread else "LOST"
                lines.append(f"{name + f' rows={rows} ' + ('x only' if form == 'x' else 'x, log_q'):44s} {g0:10.1f} {n0:10.1f} "
                             f"{g1:10.1f} {n1:10.1f}   {new / old:9.3f}  {verdict}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        main()
