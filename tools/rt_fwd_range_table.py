"""The measured table of the run-time-shaped forward kernels' operating-range cases (tests/rt_fwd_range_cases.py): runs
every case and the stack on the GPU, figures before verdicts, and writes one line per case -- its worst comparison: error
against the float64 oracle, budget, fp64 head-room, share used -- to OUT (profiles/r10/rt_fwd_range.txt holds both settings).

    python tools/rt_fwd_range_table.py [OUT] [--force-generic 1]     # 1: the fp32 VALU kernels on the same inputs
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rt_fwd_range_cases as F  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from helpers import PARITY_LOG  # noqa: E402


def main(argv):
    force = int(argv[argv.index("--force-generic") + 1]) if "--force-generic" in argv else 2
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--force-generic")]
    out = paths[0] if paths else None
    worst, failed, slowest, t_all = [], [], (0.0, ""), time.time()
    by_kernel = {}

    def measure(cid, kernel, fn):
        nonlocal slowest
        i0, t0 = len(PARITY_LOG), time.time()
        try:
            fn()
        except AssertionError as e:  # (anything else -- a HIP error -- ends the run)
            failed.append(f"FAILED {cid}: {str(e).splitlines()[0][:240]}")
        slowest = max(slowest, (time.time() - t0, cid))
        recs = PARITY_LOG[i0:]
        if recs:
            w = max(recs, key=lambda r: r["err"] / r["budget"])
            worst.append(dict(w, what=f"{cid:32s} {len(recs):3d} comparisons, worst: {w['what'][len(cid):].strip()}"))
            if not w["stress"] and w["err"] / w["budget"] > by_kernel.get(kernel, (0.0, ""))[0]:
                by_kernel[kernel] = (w["err"] / w["budget"], cid)

    for case in F.CASES:
        measure(case.id, F.kernel_of(case.layer, force), lambda: F.run_case(amd, case, force_generic=force))
    if force == 2:
        measure(F.STACK_ID, "ahf_stack_rt", lambda: F.run_stack(amd))
    text = "\n".join([f"force_generic = {force}", F.table(worst), *failed,
                      *[f"worst non-stress share of budget, {k}: {100 * v[0]:.0f} % ({v[1]})" for k, v in sorted(by_kernel.items())],
                      f"{len(PARITY_LOG)} comparisons, {len(failed)} cases failed; slowest case {slowest[0]:.2f} s "
                      f"({slowest[1]}), all of them {time.time() - t_all:.1f} s (oracle runs included)"])
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
