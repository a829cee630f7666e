"""Run by tests/test_hip_ahf_bwd_rt_wide.py in a child process under MNF_DETERMINISTIC=1 (the switch is read once per
process): with the route opted in, the gradients of an AffineHalfFlow whose hidden layers are 128 units wide land on
ahf_bwd_rt in its fixed-order form (mnf_affine_half_bwd_rt_wide_det: a slot per workgroup, added up in order) -- two backward
passes of one shape give bit-identical gradients, within the float64 oracle's budget, and no atomic-sums warning.  Prints
"ahf bwd rt wide deterministic child ok"."""
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
    _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS = 2048
    dim, hs, rows, inverse = 64, (128, 128), 4099, True  # 33+ row blocks, a ragged last tile, rows that are 16-byte aligned
    sd = recipes.affine_half_params(31 + dim, dim, h_sizes=hs, s_last_gain=2.0)
    layer = amd.AffineHalfFlow(dim, False, h_sizes=hs)
    layer.load_state_dict(sd)
    layer.to(DEV)
    x = recipes.gaussian(232 + dim, rows, dim)
    w, v = recipes.gaussian(33, rows, dim), recipes.gaussian(34, rows, 1)[:, 0]
    runs = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            layer.zero_grad()
            xg = x.to(DEV).requires_grad_(True)
            z, ld = layer.forward(xg, inverse=inverse)
            ((z * w.to(DEV)).sum() + (ld * v.to(DEV)).sum()).backward()
            torch.cuda.synchronize()
            assert amd.last_kernel() == "ahf_bwd_rt", amd.last_kernel()
            runs.append({"x": xg.grad.clone(), **{n: p.grad.clone() for n, p in layer.named_parameters()}})
    noted = [m for m in caught if issubclass(m.category, RuntimeWarning) and "MNF_DETERMINISTIC" in str(m.message)]
    assert not noted, [str(m.message) for m in noted]
    for k, g in runs[0].items():
        assert torch.equal(g.view(torch.int32), runs[1][k].view(torch.int32)), k
    ref = OracleGrads(cot_loss(lambda xx, p: O.affine_half(xx, p, False, inverse), w, v), x, sd)
    ref.check_all(runs[0], f"deterministic ahf_bwd_rt wide d={dim} h={hs} rows={rows}")
    print("ahf bwd rt wide deterministic child ok")


if __name__ == "__main__":
    main()
