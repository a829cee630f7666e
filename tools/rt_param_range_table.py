"""The measured table of the run-time-shaped kernels' parameter-range cases (tests/rt_param_range_cases.py): runs every
forward and every gradient case on the GPU, figures before verdicts, and writes one line per case -- its worst comparison:
error against the float64 oracle, budget, fp64 head-room, share used -- to OUT (profiles/r11/rt_param_range.txt holds the
sections).  MNF_DETERMINISTIC=1 in the environment measures the fixed-order gradient forms; MNF_LIB_PATH another build.

    python tools/rt_param_range_table.py [OUT] [--force-generic 1] [--beyond]
        --force-generic 1   the fp32 VALU kernels on the same inputs
        --beyond            instead of the table: UNASSERTED rows beyond the envelope (layer_spread at 2^28, 2^34, 2^40
                            between the Linears; hidden_outlier at 2^30 and 2^36), forward kernels, errors only
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import rt_fwd_range_cases as F  # noqa: E402
import rt_param_range_cases as P  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from helpers import GRAD_LOG, PARITY_LOG, normwise_err, rowwise_err  # noqa: E402


def beyond(force: int) -> list[str]:
    """layer_spread with per-Linear maxima 2^28, 2^34, 2^40 apart (first Linear x 2^9, second / (2^9 g), third x g: the
    hidden vectors stay below 2^13; layers with one hidden layer cannot get there and are left out) and hidden_outlier with
    A = 2^30, 2^36: the same fixtures at magnitudes past the documented envelope, nothing asserted."""
    lines = [f"{'y row-wise':>11s} {'ld':>10s} {'fp32 oracle y':>13s}  what (errors against the float64 oracle)"]
    keep = (P.SPREAD_F, P.SPREAD_G, P.OUTLIER)
    settings = [("layer_spread", lg, (2.0 ** 9, 2.0 ** (lg - 18), P.OUTLIER)) for lg in (28, 34, 40)] + \
               [("hidden_outlier", lg, (P.SPREAD_F, P.SPREAD_G, 2.0 ** lg)) for lg in (30, 36)]
    try:
        for fam, lg, (f, g, a) in settings:
            P.SPREAD_F, P.SPREAD_G, P.OUTLIER = f, g, a
            P.fixture.cache_clear()
            P.oracle.cache_clear()
            for case in (c for c in P.FWD_CASES if c.family == fam):
                if fam == "layer_spread" and case.layer.tag in ("rnvp50", "ahf40w", "rnvp800"):
                    continue
                fx, ref = P.fixture(case), P.oracle(case)
                f = P.module_of(amd, fx)
                f.force_generic = force
                y, ld = P.call(amd, f, fx, fx.x, F.kernel_of(case.layer, force))
                ok = bool(torch.isfinite(y).all())
                e_y = rowwise_err(y.numpy(), ref.y64.numpy()) if ok else float("nan")
                e_l = normwise_err(ld.numpy(), ref.ld64.numpy()) if bool(torch.isfinite(ld).all()) else float("nan")
                lines.append(f"{e_y:11.2e} {e_l:10.2e} {rowwise_err(ref.y32.numpy(), ref.y64.numpy()):13.2e}  "
                             f"{case.id} at 2^{lg}")
    finally:
        P.SPREAD_F, P.SPREAD_G, P.OUTLIER = keep
        P.fixture.cache_clear()
        P.oracle.cache_clear()
    return lines


def main(argv):
    force = int(argv[argv.index("--force-generic") + 1]) if "--force-generic" in argv else 2
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--force-generic")]
    out = paths[0] if paths else None
    worst, failed, slowest, t_all = [], [], (0.0, ""), time.time()
    by_kernel = {}
    mode = "MNF_DETERMINISTIC=1 (fixed-order sums)" if amd.deterministic() else "default mode (atomic sums)"
    head = f"{os.path.basename(amd.library_path())}, {mode}, force_generic = {force}"

    def measure(cid, kernel, log, fn):
        nonlocal slowest
        i0, t0 = len(log), time.time()
        try:
            fn()
        except AssertionError as e:  # (anything else -- a HIP error -- ends the run)
            failed.append(f"FAILED {cid}: {str(e).splitlines()[0][:240]}")
        slowest = max(slowest, (time.time() - t0, cid))
        recs = log[i0:]
        if recs:
            w = max(recs, key=lambda r: r["err"] / r["budget"])
            worst.append(dict(w, what=f"{cid:40s} {len(recs):3d} comparisons, worst: {w['what'][len(cid) - 5:].strip()}"))
            if not w["stress"] and w["err"] / w["budget"] > by_kernel.get(kernel, (0.0, ""))[0]:
                by_kernel[kernel] = (w["err"] / w["budget"], cid)

    if "--beyond" in argv:
        text = "\n".join([head + ", beyond the envelope (unasserted)", *beyond(force)])
    else:
        for case in P.FWD_CASES:
            measure("fwd  " + case.id, F.kernel_of(case.layer, force), PARITY_LOG,
                    lambda: P.run_forward(amd, case, force_generic=force))
        for case in P.GRAD_CASES:
            kernel = case.layer.kernel if force == 2 else case.layer.kernel.replace("_rt", "_generic")
            measure("grad " + case.id, kernel, GRAD_LOG, lambda: P.run_gradients(amd, case, force_generic=force))
        text = "\n".join([head, P.table(worst), *failed,
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
