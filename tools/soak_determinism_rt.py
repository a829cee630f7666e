"""Are training steps on the run-time-shaped gradient kernels reproducible bit for bit?  Three models none of whose
layers has a per-shape gradient kernel -- 9 x AffineHalfFlow(64, h_sizes=(24, 24)) with FusedAdam + FlatParameters,
3 x NSF_CL(128, K=8, n_h=32) with torch.optim.Adam, RNVP(100, h_sizes=(100,)) with FusedAdam + FlatParameters -- each run
the same N Adam steps twice from identical parameters, inputs and seeds; the parameters after each run must be identical
(torch.equal).  Under MNF_DETERMINISTIC=1 the gradient launches are the fixed-order forms mnf_*_bwd_rt_det; without it,
the atomic ones (sums that may differ in their last bits).  The gradient kernel family each model ran is printed too.

usage: python3 tools/soak_determinism_rt.py [steps] [rows]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch_mnf_amd as amd

dev = torch.device("cuda")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 65536


def data(seed, dim):
    return torch.randn(rows, dim, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def run_ahf():
    torch.manual_seed(71)
    flows = [amd.AffineHalfFlow(64, parity=bool(i % 2), h_sizes=(24, 24)) for i in range(9)]
    model = amd.NormalizingFlowModel(amd.StandardNormal(64), flows).to(dev)
    opt = amd.FusedAdam(amd.FlatParameters(model), lr=1e-3)
    x = data(1, 64)
    return model, opt, (lambda: -model.log_prob(x).mean())


def run_nsf():
    torch.manual_seed(72)
    flows = [amd.NSF_CL(128, K=8, B=3, n_h=32) for _ in range(3)]
    model = amd.NormalizingFlowModel(amd.StandardNormal(128), flows).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    x = data(2, 128)
    return model, opt, (lambda: -model.log_prob(x).mean())


def run_rnvp():
    torch.manual_seed(73)
    model = amd.RNVP(100, h_sizes=(100,)).to(dev)
    opt = amd.FusedAdam(amd.FlatParameters(model), lr=1e-3)
    z = data(3, 100)

    def loss():
        x, ld = model.forward(z, seed=9)
        return x.pow(2).mean() - ld.mean()
    return model, opt, loss


def trajectory(build):
    torch.manual_seed(0)
    model, opt, loss_fn = build()
    kernels = set()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        kernels.add(amd.last_kernel())  # (the last launch of a backward pass: the first layer's gradient kernel)
        opt.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps * 1e3
    return [p.detach().clone() for p in model.parameters()], float(loss), dt, kernels


bad_total = 0
for name, build in (("ahf_rt", run_ahf), ("nsf_rt", run_nsf), ("rnvp_rt", run_rnvp)):
    a, la, ta, ka = trajectory(build)
    b, lb, tb, kb = trajectory(build)
    bad = sum(int(not torch.equal(p, q)) for p, q in zip(a, b))
    worst = max(float((p - q).abs().max() / (p.abs().max() + 1e-30)) for p, q in zip(a, b))
    print(f"{name}: {steps} Adam steps twice at {rows} rows: {bad} of {len(a)} parameter tensors differ (worst relative "
          f"difference {worst:.2e}); final loss {la:.6f} / {lb:.6f}; {min(ta, tb):.3f} ms per step; gradient kernels "
          f"{','.join(sorted(ka | kb))}; MNF_DETERMINISTIC={os.environ.get('MNF_DETERMINISTIC', '0')}")
    bad_total += bad
sys.exit(1 if bad_total else 0)
