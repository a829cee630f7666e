"""Run by tests/test_hip_glow_rt.py in a child process under MNF_DETERMINISTIC=1 (the switch is read once per process):
a [ActNormFlow, Glow, NSF_CL] x 2 model at dim = 48 whose Glow layers run on the run-time-shaped kernels -- one
GraphedStep of -log_prob.mean() captured and replayed for 3 steps, done twice from the same state: the same losses and
the same parameters bit for bit.  Prints "glow rt model child ok" at the end."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import recipes  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402

DEV = "cuda"
DIM, ROWS, K, N_H = 48, 4096, 8, 8


def build_layers():
    """(modules, oracle layer specs) of [ActNormFlow, Glow, NSF_CL(K = 8, n_h = 8)] x 2"""
    flows, specs = [], []
    for i in range(2):
        ap, gp = recipes.actnorm_params(940 + i, DIM), recipes.glow_params(950 + i, DIM)
        sp = recipes.nsf_cl_params(960 + i, DIM, K, N_H)
        an, gl, nsf = amd.ActNormFlow(DIM), amd.Glow(DIM), amd.NSF_CL(DIM, K=K, B=3, n_h=N_H)
        an.load_state_dict(ap)
        an.data_dep_init_done = True
        gl.P = gp["P"]
        gl.load_state_dict({k: gp[k] for k in "LSU"})
        nsf.load_state_dict(sp)
        flows += [an, gl, nsf]
        specs += [{"kind": "affine_const", "params": ap}, {"kind": "glow", "params": gp},
                  {"kind": "nsf_cl", "K": K, "B": 3.0, "params": sp}]
    return flows, specs


def actnorm_sums_repeat():
    """ActNormFlow's own gradient launch in this mode: grad_s and grad_t as blocks added in order -- the same bits twice,
    and the float64 sums to fp32 accuracy"""
    rows = 30001
    ap = recipes.actnorm_params(980, DIM)
    x_cpu, w = recipes.gaussian(981, rows, DIM), recipes.gaussian(982, rows, DIM)
    for inverse in (False, True):
        runs = []
        for _ in range(2):
            an = amd.ActNormFlow(DIM)
            an.load_state_dict(ap)
            an.data_dep_init_done = True
            an.to(DEV)
            x = x_cpu.to(DEV).requires_grad_(True)
            y, _ = (an.inverse if inverse else an.forward)(x)
            (y * w.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            runs.append((an.s.grad.clone(), an.t.grad.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), inverse
        s64, t64 = ap["s"].double().requires_grad_(True), ap["t"].double().requires_grad_(True)
        y64 = (x_cpu.double() - t64) * torch.exp(-s64) if inverse else x_cpu.double() * torch.exp(s64) + t64
        (y64 * w.double()).sum().backward()
        for got, ref in zip(runs[0], (s64.grad, t64.grad)):
            err = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
            assert err <= 1e-5, (inverse, err)
    print("actnorm: fixed-order column sums repeat bit for bit")


def main():
    assert amd.deterministic(), "run under MNF_DETERMINISTIC=1"
    actnorm_sums_repeat()
    _dispatch.GLOW_RT_MIN_ROWS = 0
    assert _dispatch.glow_route(ROWS, DIM) == "rt" and _dispatch.glow_route(ROWS, DIM, weight=True) == "rt"
    batches = [recipes.gaussian(970 + i, ROWS, DIM).to(DEV) for i in range(4)]

    def build():
        model = amd.NormalizingFlowModel(amd.StandardNormal(DIM), build_layers()[0]).to(DEV)
        return model, amd.FusedAdam(amd.FlatParameters(model), lr=1e-3, capturable=True)

    def replay():
        model, opt = build()
        step = amd.GraphedStep(opt, lambda x: -model.log_prob(x).mean(), batches[0])
        losses = [float(step(x)) for x in batches[1:]]
        torch.cuda.synchronize()
        return losses, opt.flat.data.clone()

    (la, pa), (lb, pb) = replay(), replay()
    assert len(la) == 3 and all(v == v and abs(v) != float("inf") for v in la), la
    assert la == lb, (la, lb)
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), float((pa - pb).abs().max())
    print(f"graph: two replays of {len(la)} steps, identical parameters; losses {la}")
    print("glow rt model child ok")


if __name__ == "__main__":
    main()
