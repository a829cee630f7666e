"""Run by tests/test_rt_deterministic.py in a child process under MNF_DETERMINISTIC=1 (the switch is read once per process):
the run-time-shaped gradient shapes of tests/test_hip_round6.py land on the *_bwd_rt kernels -- their fixed-order forms --
and match the float64 oracle; a graphed training step on those kernels replays bit for bit; a gradient pass on the VALU
kernel (atomic sums) warns once per layer and shape, an rt one does not; the operating-range table of
tests/rt_bwd_range_cases.py holds in this mode too, and its `!same` cases repeat bit for bit; so does the gradient half of the
parameter-range table (tests/rt_param_range_cases.py); the reference's own gradients (fixture G17) of the AffineHalfFlow d = 64
case and of the 4-layer run hold on the fixed-order kernels with the same budget.  Prints "rt deterministic child ok" at the end."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import numpy as np  # noqa: E402

import recipes  # noqa: E402
import rt_bwd_range_cases as R  # noqa: E402
import rt_golden_cases as G  # noqa: E402
import rt_param_range_cases as P  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from oracle import flow_oracle as O  # noqa: E402
from test_hip_autograd import OracleGrads, cot_loss  # noqa: E402
from recipes import rnvp_params_layers as _rnvp_sd  # noqa: E402
from test_hip_round6 import AHF_BWD_SHAPES, NSF_BWD_SHAPES, RNVP_BWD_SHAPES, _backward  # noqa: E402

DEV = "cuda"
assert amd.deterministic(), "run under MNF_DETERMINISTIC=1"


def rt(f):
    f.force_generic = 2
    return f.to(DEV)


def layers_on_the_rt_kernels():
    # (round 6's row counts: the fixtures' rows there are clear of spline knots and LeakyReLU kinks -- at 4,133 rows the
    #  NSF_CL (50, 10, 12) inverse fixture has a row whose float64 and kernel derivatives take different one-sided slopes,
    #  in either mode: grad_x does not go through the slots.  Larger batches: tests/test_rt_deterministic.py in process)
    for dim, hs, kw in AHF_BWD_SHAPES:
        for inverse in (False, True):
            for rows, parity in ((300, True), (2100, False)):
                sd = recipes.affine_half_params(31 + dim, dim, h_sizes=hs, s_last_gain=2.0, **kw)
                x_cpu = recipes.gaussian(232 + dim, rows, dim)
                w_y, w_l = recipes.gaussian(33, rows, dim), recipes.gaussian(34, rows, 1)[:, 0]
                ref = OracleGrads(cot_loss(lambda x, p: O.affine_half(x, p, parity, inverse, **kw), w_y, w_l), x_cpu, sd)
                f = amd.AffineHalfFlow(dim, parity, h_sizes=hs, **kw)
                f.load_state_dict(sd)
                got = _backward(rt(f), x_cpu, lambda m, x: m.forward(x, inverse=inverse), w_y, w_l)
                assert amd.last_kernel() == "ahf_bwd_rt", (dim, hs, kw, amd.last_kernel())
                ref.check_all(got, f"deterministic ahf_bwd_rt d={dim} h={hs} {kw} rows={rows} inv={inverse}")
    for dim, K, n_h in NSF_BWD_SHAPES:
        for inverse in (False, True):
            rows = 700
            sd = recipes.nsf_cl_params(51 + dim + K, dim, K, n_h)
            x_cpu = recipes.gaussian(52 + dim, rows, dim, scale=1.4)
            w_y, w_l = recipes.gaussian(53, rows, dim), recipes.gaussian(54, rows, 1)[:, 0]
            ref = OracleGrads(cot_loss(lambda x, p: O.nsf_cl(x, p, K, 3.0, inverse), w_y, w_l), x_cpu, sd)
            f = amd.NSF_CL(dim, K=K, B=3, n_h=n_h)
            f.load_state_dict(sd)
            got = _backward(rt(f), x_cpu, lambda m, x: (m.inverse if inverse else m.forward)(x), w_y, w_l)
            assert amd.last_kernel() == "nsf_bwd_rt", (dim, K, n_h, amd.last_kernel())
            ref.check_all(got, f"deterministic nsf_bwd_rt ({dim},{K},{n_h}) inv={inverse}")
    for dim, hs in RNVP_BWD_SHAPES:
        for seeded in (False, True):
            rows = 700
            sd = _rnvp_sd(41 + dim, dim, hs)
            z_cpu = recipes.gaussian(42 + dim, rows, dim)
            w_y, w_l = recipes.gaussian(43, rows, dim), recipes.gaussian(44, rows, 1)[:, 0]
            f = amd.RNVP(dim, h_sizes=hs)
            f.load_state_dict(sd)
            rt(f)
            mask = f.mask_for(77, rows).cpu() if seeded else recipes.bernoulli_mask(97, rows, dim)
            ref = OracleGrads(cot_loss(lambda x, p: O.rnvp(x, p, mask.to(x.dtype)), w_y, w_l), z_cpu, sd)
            call = (lambda m, z: m.forward(z, seed=77)) if seeded else (lambda m, z: m.forward(z, mask=mask.to(DEV)))
            got = _backward(f, z_cpu, call, w_y, w_l)
            assert amd.last_kernel() == "rnvp_bwd_rt", (dim, hs, amd.last_kernel())
            ref.check_all(got, f"deterministic rnvp_bwd_rt d={dim} h={hs} seeded={seeded}")
    print("layers: every run-time-shaped gradient shape on its *_bwd_rt kernel, within the oracle budget")


def graphed_step_replays_identically():
    """tests/test_hip_round6.py's graphed model on the run-time-shaped kernels, built and replayed twice from the same state"""
    dim, rows = 16, 4096
    batches = [recipes.gaussian(400 + i, rows, dim).to(DEV) for i in range(6)]

    def build():
        torch.manual_seed(31)
        layers = [amd.AffineHalfFlow(dim, parity=False, h_sizes=(20, 20)), amd.NSF_CL(dim, K=6, B=3, n_h=24),
                  amd.AffineHalfFlow(dim, parity=True, h_sizes=(40,)), amd.AffineHalfFlow(dim, parity=False, h_sizes=(12, 16, 12, 8))]
        model = amd.NormalizingFlowModel(amd.StandardNormal(dim), layers).to(DEV)
        return model, amd.FusedAdam(amd.FlatParameters(model), lr=1e-3, capturable=True)

    # eagerly first: which gradient kernels the step runs
    model, opt = build()
    kernels = set()
    loss = -model.log_prob(batches[0]).mean()
    loss.backward()
    torch.cuda.synchronize()
    kernels.add(amd.last_kernel())
    assert kernels <= {"ahf_bwd_rt", "nsf_bwd_rt"}, kernels
    del loss, model, opt

    def replay():
        model, opt = build()
        step = amd.GraphedStep(opt, lambda x: -model.log_prob(x).mean(), batches[0])
        losses = [float(step(x)) for x in batches[1:]]
        torch.cuda.synchronize()
        return losses, opt.flat.data.clone()

    (la, pa), (lb, pb) = replay(), replay()
    assert la == lb, (la, lb)
    assert torch.equal(pa, pb), float((pa - pb).abs().max())
    assert la[-1] < la[0], la
    print(f"graph: two replays of {len(la)} steps, identical parameters; kernels {sorted(kernels)}")


def warns_once_where_the_sums_are_atomic():
    def backward_twice(f, rows):
        x = torch.randn(rows, f.dim, device=DEV)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for _ in range(2):
                xg = x.clone().requires_grad_(True)
                y, ld = f.forward(xg)
                (y.sum() + ld.sum()).backward()
            torch.cuda.synchronize()
        return [m for m in w if issubclass(m.category, RuntimeWarning) and "MNF_DETERMINISTIC" in str(m.message)]

    torch.manual_seed(3)
    valu = amd.AffineHalfFlow(64, parity=False, h_sizes=(128,)).to(DEV)
    w = backward_twice(valu, 4096)
    assert amd.last_kernel() == "ahf_bwd_generic", amd.last_kernel()
    assert len(w) == 1, [str(m.message) for m in w]
    text = str(w[0].message)
    assert "AffineHalfFlow" in text and "128" in text and "failed" not in text.lower(), text
    w = backward_twice(amd.AffineHalfFlow(64, parity=False, h_sizes=(24, 24)).to(DEV), 4096)
    assert amd.last_kernel() == "ahf_bwd_rt", amd.last_kernel()
    assert not w, [str(m.message) for m in w]
    print("warnings: one for the VALU gradient kernel, none for the rt one")


def range_cases_hold_and_repeat():
    """The table the default mode's test runs (kernel name + oracle budget per case); the cases whose row blocks mix
    exchange scales (dw_phase_rows' second branch) twice: the same parameter gradients, bit for bit."""
    twice = 0
    for case in R.CASES:
        got = R.run_case(amd, case, prefix="deterministic ")
        if case.family in ("cot_outlier", "big_hidden"):
            again, kernel = R.gpu_grads(amd, R.fixture(case))
            assert kernel == case.layer.kernel, (case.id, kernel)
            for k in got:
                if k != "x":
                    assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (case.id, k)
            twice += 1
    R.run_the_run(amd, prefix="deterministic ")
    print(f"range: {len(R.CASES)} cases and the one-node run within the oracle budget; {twice} of them twice, bit for bit")


def parameter_range_cases_hold():
    """The gradient half of tests/rt_param_range_cases.py on the fixed-order kernels: kernel name + oracle budget per case."""
    for case in P.GRAD_CASES:
        P.run_gradients(amd, case, prefix="deterministic ")
    print(f"parameter range: {len(P.GRAD_CASES)} gradient cases within the oracle budget")


def reference_gradients_hold():
    """Fixture G17 (tests/golden/g17_cases.py) in this mode: the AffineHalfFlow d = 64 case on ahf_bwd_rt, the 4-layer run
    layer by layer and as one node (ahf_bwd_stack_rt) -- tests/test_hip_rt_golden.py's checks, the same budget."""
    cache = {}

    def golden(name):
        if name not in cache:
            cache[name] = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        return cache[name]

    G.layer_case(amd, golden, "ahf_d64_h24x24_inv", 2, prefix="deterministic ")
    for fused in (False, True):
        G.run_case(amd, golden, fused, prefix="deterministic ")
    print("reference gradients: the d = 64 layer and the 4-layer run (both routes) within the fixture's budget")


if __name__ == "__main__":
    warns_once_where_the_sums_are_atomic()
    graphed_step_replays_identically()
    layers_on_the_rt_kernels()
    range_cases_hold_and_repeat()
    parameter_range_cases_hold()
    reference_gradients_hold()
    print("rt deterministic child ok")
