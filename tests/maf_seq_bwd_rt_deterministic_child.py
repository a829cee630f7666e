"""Run by tests/test_hip_maf_seq_bwd_rt.py in a child process under MNF_DETERMINISTIC=1 (the switch is read once per
process): with the route opted in, the gradients of the element-by-element direction of MAF land on maf_seq_bwd_rt in its
fixed-order form (mnf_maf_seq_bwd_rt_det: the solve has no sums, the weight pass is mnf_maf_bwd_rt_det) -- two backward
passes of one shape give bit-identical gradients, within the float64 oracle's budget, and no atomic-sums warning; the
cot_small, cot_outlier and big_rows gradient cases of one layer of tests/maf_rt_range_cases.py hold in this mode with the same
budget, two passes bit-identical.  Prints "maf seq bwd rt deterministic child ok"."""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import maf_rt_range_cases as M  # noqa: E402
import recipes  # noqa: E402
import torch_mnf_amd as amd  # noqa: E402
from oracle import flow_oracle as O  # noqa: E402
from test_hip_autograd import OracleGrads, cot_loss  # noqa: E402
from torch_mnf_amd import _dispatch  # noqa: E402

DEV = "cuda"
assert amd.deterministic(), "run under MNF_DETERMINISTIC=1"


def main():
    _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS = 0
    # odd widths, three layers, one workgroup's worth of slots | a persistent grid smaller than the row blocks
    for dim, h_sizes, rows in ((37, (20, 7, 33), 257), (6, (8,), 70003)):
        parity = True
        sd = recipes.maf_params(2100 + dim + len(h_sizes), dim, h_sizes, gain=1.2, last_gain=0.5)
        masks = O.made_masks(dim, h_sizes, 2 * dim)
        layer = amd.MAF(dim, parity=parity, h_sizes=h_sizes)
        layer.load_state_dict(sd, strict=False)
        layer.force_generic = 2
        layer.to(DEV)
        z = recipes.gaussian(2600 + dim, rows, dim)
        w_y, w_l = recipes.gaussian(2700 + dim, rows, dim), recipes.gaussian(2701 + dim, rows, 1)[:, 0]
        runs = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2):
                layer.zero_grad()
                zg = z.to(DEV).requires_grad_(True)
                y, ld = layer.forward(zg)
                ((y * w_y.to(DEV)).sum() + (ld * w_l.to(DEV)).sum()).backward()
                torch.cuda.synchronize()
                assert amd.last_kernel() == "maf_seq_bwd_rt", amd.last_kernel()
                runs.append({"x": zg.grad.clone(), **{n: p.grad.clone() for n, p in layer.named_parameters()}})
        noted = [m for m in caught if issubclass(m.category, RuntimeWarning) and "MNF_DETERMINISTIC" in str(m.message)]
        assert not noted, [str(m.message) for m in noted]
        for k, v in runs[0].items():
            assert torch.equal(v.view(torch.int32), runs[1][k].view(torch.int32)), (rows, k)
        ref = OracleGrads(cot_loss(lambda xx, p: O.maf(xx, p, masks, parity, False), w_y, w_l), z, sd)
        ref.check_all(runs[0], f"deterministic maf_seq_bwd_rt d={dim} h={h_sizes} rows={rows}")
        for m in layer._masked():
            assert float((m.weight.grad * (m.mask.T == 0)).abs().max()) == 0.0
    # the range table's gradient cases of one layer on the fixed-order route
    n = M.run_deterministic(amd, M.DETERMINISTIC_LAYER, inverse=False)
    assert n == 3, n
    print(f"range: {n} gradient cases of {M.DETERMINISTIC_LAYER} on maf_seq_bwd_rt within the oracle budget, twice, bit for bit")
    print("maf seq bwd rt deterministic child ok")


if __name__ == "__main__":
    main()
