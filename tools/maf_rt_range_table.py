"""The measured table of the MAF / IAF matrix-core kernels' operating- and parameter-range cases
(tests/maf_rt_range_cases.py): runs every forward, gradient and parameter case on the GPU, figures before verdicts, and
writes one line per case -- its worst comparison: error against the float64 oracle, budget, fp64 head-room, share used -- to
OUT (profiles/r24/maf_rt_range.txt holds the sections).  MNF_DETERMINISTIC=1 in the environment measures the fixed-order
gradient forms; MNF_LIB_PATH another build.

    python tools/maf_rt_range_table.py [OUT] [--force-generic 1]     # 1: the fp32 VALU kernels (maf_generic / maf_bwd_generic)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import maf_rt_range_cases as M  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from helpers import GRAD_LOG, PARITY_LOG  # noqa: E402


def main(argv):
    force = int(argv[argv.index("--force-generic") + 1]) if "--force-generic" in argv else 2
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--force-generic")]
    out = paths[0] if paths else None
    worst, failed, no_valu, slowest, t_all = [], [], [], (0.0, ""), time.time()
    by_kernel = {}
    mode = "MNF_DETERMINISTIC=1 (fixed-order sums)" if amd.deterministic() else "default mode (atomic sums)"
    head = f"{os.path.basename(amd.library_path())}, {mode}, force_generic = {force}"

    def family_of(case, gradient):
        kernel = M.kernel_of(case, gradient, force)
        if force != 2:  # one VALU kernel serves both directions: keep their worst shares apart
            kernel += " (one-pass)" if case.inverse else " (element by element)"
        return kernel

    def measure(cid, kernel, log, fn):
        nonlocal slowest
        i0, t0 = len(log), time.time()
        try:
            fn()
        except AssertionError as e:  # (anything else -- a HIP error -- ends the run)
            failed.append(f"FAILED {cid}: {str(e).splitlines()[0][:240]}")
        except amd._lib.MnfHipError as e:  # the VALU kernels have no launch for some shapes (refused before any launch)
            if force == 2 or e.code != amd._lib.MNF_ERR_UNSUPPORTED:
                raise
            no_valu.append(f"no VALU kernel for this shape: {cid}")
        slowest = max(slowest, (time.time() - t0, cid))
        recs = log[i0:]
        if recs:
            w = max(recs, key=lambda r: r["err"] / r["budget"])
            label = w["what"].split(cid, 1)[-1].strip()
            worst.append(dict(w, what=f"{cid:44s} {len(recs):3d} comparisons, worst: {label}"))
            if not w["stress"] and w["err"] / w["budget"] > by_kernel.get(kernel, (0.0, ""))[0]:
                by_kernel[kernel] = (w["err"] / w["budget"], cid)

    for name, cases in (("fwd", M.FWD_CASES), ("param-fwd", M.PARAM_FWD_CASES)):
        for case in cases:
            measure(f"{name} {case.id}", family_of(case, False), PARITY_LOG, lambda: M.run_forward(amd, case, force_generic=force))
    for name, cases in (("grad", M.GRAD_CASES), ("param-grad", M.PARAM_GRAD_CASES)):
        for case in cases:
            kernel = family_of(case, True)
            measure(f"{name} {case.id}", kernel, GRAD_LOG, lambda: M.run_gradients(amd, case, force_generic=force))
    text = "\n".join([head, M.table(worst), *failed, *no_valu,
                      *[f"worst non-stress share of budget, {k}: {100 * v[0]:.0f} % ({v[1]})" for k, v in sorted(by_kernel.items())],
                      f"{len(PARITY_LOG) + len(GRAD_LOG)} comparisons, {len(failed)} cases failed; slowest case "
                      f"{slowest[0]:.2f} s ({slowest[1]}), all of them {time.time() - t_all:.1f} s (oracle runs included)"])
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
