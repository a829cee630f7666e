"""The measured table of the run-time-shaped gradient kernels' operating-range cases (tests/rt_bwd_range_cases.py): runs
every case and the one-node run on the GPU, figures before verdicts, and writes one line per case -- its worst comparison:
error against the float64 oracle, budget, fp64 head-room, share used -- to OUT (default profiles/r9/rt_bwd_range.txt's
section for this sum mode is pasted from it).  MNF_DETERMINISTIC=1 in the environment measures the fixed-order forms.

    python tools/rt_bwd_range_table.py [OUT] [--force-generic 1]     # 1: the VALU kernels on the same inputs
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rt_bwd_range_cases as R  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from helpers import GRAD_LOG  # noqa: E402


def main(argv):
    force = int(argv[argv.index("--force-generic") + 1]) if "--force-generic" in argv else 2
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--force-generic")]
    out = paths[0] if paths else None
    worst, failed, slowest, t_all = [], [], 0.0, time.time()

    def measure(cid, fn):
        nonlocal slowest
        i0, t0 = len(GRAD_LOG), time.time()
        try:
            fn()
        except AssertionError as e:  # (anything else -- a HIP error -- ends the run)
            failed.append(f"FAILED {cid}: {str(e).splitlines()[0][:240]}")
        slowest = max(slowest, time.time() - t0)
        recs = GRAD_LOG[i0:]
        if recs:
            w = max(recs, key=lambda r: r["err"] / r["budget"])
            worst.append(dict(w, what=f"{cid:32s} {len(recs):3d} comparisons, worst: {w['what'][len(cid):].strip()}"))

    for case in R.CASES:
        measure(case.id, lambda: R.run_case(amd, case, force_generic=force))
    if force == 2:
        measure(R.RUN_ID, lambda: R.run_the_run(amd))
    mode = "MNF_DETERMINISTIC=1 (fixed-order sums)" if amd.deterministic() else "default mode (atomic sums)"
    text = "\n".join([f"{mode}, force_generic = {force}", R.table(worst), *failed,
                      f"{len(GRAD_LOG)} comparisons, {len(failed)} cases failed; slowest case {slowest:.2f} s, "
                      f"all of them {time.time() - t_all:.1f} s (oracle runs included)"])
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
