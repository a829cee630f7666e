"""Run by tests/test_hip_nsf_ar_bwd_rt.py in a child process under MNF_DETERMINISTIC=1 (the switch is read once per
process): with the route opted in, the gradients of NSF_AR.inverse land on nsf_ar_bwd_rt in its fixed-order form
(mnf_nsf_ar_bwd_rt_det: a slot per workgroup, added up in order) -- two backward passes of one shape give bit-identical
gradients, within the float64 oracle's budget, and no atomic-sums warning.  Prints "nsf ar bwd rt deterministic child ok"."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import recipes  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from oracle import flow_oracle as O  # noqa: E402
from test_hip_autograd import OracleGrads, cot_loss  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402

DEV = "cuda"
assert amd.deterministic(), "run under MNF_DETERMINISTIC=1"


def main():
    _dispatch.NSF_AR_BWD_RT_MIN_ROWS = 0
    dim, K, n_h, rows = 37, 5, 8, 4099  # two K-steps of input, dim % 4 = 1, 33 row blocks, a ragged last tile
    sd = recipes.nsf_ar_params(5000 + dim, dim, K, n_h)
    layer = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
    layer.load_state_dict(sd)
    layer.force_generic = 2
    layer.to(DEV)
    x = recipes.gaussian(5001, rows, dim, scale=1.4)
    w, v = recipes.gaussian(5002, rows, dim), recipes.gaussian(5003, rows, 1)[:, 0]
    runs = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            layer.zero_grad()
            xg = x.to(DEV).requires_grad_(True)
            z, ld = layer.inverse(xg)
            ((z * w.to(DEV)).sum() + (ld * v.to(DEV)).sum()).backward()
            torch.cuda.synchronize()
            assert amd.last_kernel() == "nsf_ar_bwd_rt", amd.last_kernel()
            runs.append({"x": xg.grad.clone(), **{n: p.grad.clone() for n, p in layer.named_parameters()}})
    noted = [m for m in caught if issubclass(m.category, RuntimeWarning) and "MNF_DETERMINISTIC" in str(m.message)]
    assert not noted, [str(m.message) for m in noted]
    for k, g in runs[0].items():
        assert torch.equal(g.view(torch.int32), runs[1][k].view(torch.int32)), k
    ref = OracleGrads(cot_loss(lambda xx, p: O.nsf_ar(xx, p, K, 3.0, True), w, v), x, sd)
    ref.check_all(runs[0], f"deterministic nsf_ar_bwd_rt d={dim} K={K} n_h={n_h} rows={rows}")
    print("nsf ar bwd rt deterministic child ok")


if __name__ == "__main__":
    main()
