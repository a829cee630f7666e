"""Forward + backward of one layer per shape of tools/soak_determinism_rt.py, ns per row (HIP events, best of 5), and the
gradient kernel family that ran.  Run it with and without MNF_DETERMINISTIC=1 to compare the atomic and the fixed-order
gradient sums (profiles/r7/rt_deterministic.md).

usage: python3 tools/time_rt_deterministic.py [rows]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch_mnf_amd as amd

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
dev = torch.device("cuda")


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


torch.manual_seed(5)
LAYERS = [("AffineHalfFlow(64, (24, 24))", amd.AffineHalfFlow(64, parity=False, h_sizes=(24, 24)), lambda f, x: f.forward(x)),
          ("NSF_CL(128, K=8, n_h=32)", amd.NSF_CL(128, K=8, B=3, n_h=32), lambda f, x: f.forward(x)),
          ("RNVP(100, (100,))", amd.RNVP(100, h_sizes=(100,)), lambda f, x: f.forward(x, seed=9))]
for name, f, call in LAYERS:
    f = f.to(dev)
    dim = f.dim
    x = torch.randn(ROWS, dim, device=dev).requires_grad_(True)
    w = torch.randn(ROWS, dim, device=dev) / ROWS

    def step():
        y, ld = call(f, x)
        ((y * w).sum() + ld.mean()).backward()

    t = timed(step)
    print(f"{name}: forward + backward {t * 1e6 / ROWS:.2f} ns/row at {ROWS} rows; gradient kernel {amd.last_kernel()}; "
          f"MNF_DETERMINISTIC={os.environ.get('MNF_DETERMINISTIC', '0')}")
