"""Run by tests/test_hip_maf_rt.py in a child process under MNF_DETERMINISTIC=1 (the switch is read once per process): the
one-pass direction of MAF lands on maf_bwd_rt in its fixed-order form -- two backward passes of one shape give bit-identical
parameter gradients, no atomic-sums warning, the gradients within the float64 oracle's budget --, the atomic entry refuses,
the element-by-element direction (VALU kernel, atomic sums) still warns, and the cot_small, cot_outlier and big_rows gradient
cases of one layer of tests/maf_rt_range_cases.py hold in this mode with the same budget, two passes bit-identical.  Prints
"maf rt deterministic child ok"."""
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
from torch_mnf_amd import _lib  # noqa: E402
from torch_mnf_amd.flows import _grad_scale  # noqa: E402

DEV = "cuda"
assert amd.deterministic(), "run under MNF_DETERMINISTIC=1"


def main():
    dim, h_sizes, parity = 37, (20, 7, 33), True
    sd = recipes.maf_params(2600, dim, h_sizes, gain=1.2, last_gain=0.5)
    masks = O.made_masks(dim, h_sizes, 2 * dim)
    layer = amd.MAF(dim, parity=parity, h_sizes=h_sizes)
    layer.load_state_dict(sd, strict=False)
    layer.force_generic = 2
    layer.to(DEV)
    for rows in (257, 4133):  # one workgroup's worth of slots | several row blocks per slot
        x = recipes.gaussian(2601, rows, dim)
        w_y, w_l = recipes.gaussian(2602, rows, dim), recipes.gaussian(2603, rows, 1)[:, 0]
        runs = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2):
                layer.zero_grad()
                xg = x.to(DEV).requires_grad_(True)
                y, ld = layer.inverse(xg)
                ((y * w_y.to(DEV)).sum() + (ld * w_l.to(DEV)).sum()).backward()
                torch.cuda.synchronize()
                assert amd.last_kernel() == "maf_bwd_rt", amd.last_kernel()
                runs.append({"x": xg.grad.clone(), **{n: p.grad.clone() for n, p in layer.named_parameters()}})
        noted = [m for m in caught if issubclass(m.category, RuntimeWarning) and "MNF_DETERMINISTIC" in str(m.message)]
        assert not noted, [str(m.message) for m in noted]
        for k, v in runs[0].items():
            assert torch.equal(v.view(torch.int32), runs[1][k].view(torch.int32)), (rows, k)
        ref = OracleGrads(cot_loss(lambda xx, p: O.maf(xx, p, masks, parity, True), w_y, w_l), x, sd)
        ref.check_all(runs[0], f"deterministic maf_bwd_rt d={dim} h={h_sizes} rows={rows}")
        for m in layer._masked():
            assert float((m.weight.grad * (m.mask.T == 0)).abs().max()) == 0.0
    # the atomic entry refuses under the switch, before any launch
    lib = _lib.load()
    flat, _ = layer._packed(torch.device(DEV))
    mb = layer._mask_bytes(torch.device(DEV))
    xd = x.to(DEV)
    gx, gf = torch.empty_like(xd), torch.zeros_like(flat)
    gy = w_y.to(DEV)
    sc = _grad_scale(gy, None, rows, dim, xd.device)
    rc = lib.mnf_maf_bwd_rt(xd.data_ptr(), gy.data_ptr(), None, gx.data_ptr(), gf.data_ptr(), flat.data_ptr(), mb.data_ptr(),
                            sc.data_ptr(), rows, dim, 1, len(h_sizes), layer._hid, None)
    assert rc == _lib.MNF_ERR_UNSUPPORTED, rc
    # the element-by-element direction stays on the VALU kernel: atomic sums, one warning
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        xg = x[:64].to(DEV).requires_grad_(True)
        y, ld = layer.forward(xg)
        (y.sum() + ld.sum()).backward()
        torch.cuda.synchronize()
    assert amd.last_kernel() == "maf_bwd_generic", amd.last_kernel()
    assert any("MNF_DETERMINISTIC" in str(m.message) for m in caught)
    # the range table's gradient cases of one layer on the fixed-order kernel
    n = M.run_deterministic(amd, M.DETERMINISTIC_LAYER, inverse=True)
    assert n == 3, n
    print(f"range: {n} gradient cases of {M.DETERMINISTIC_LAYER} on maf_bwd_rt within the oracle budget, twice, bit for bit")
    print("maf rt deterministic child ok")


if __name__ == "__main__":
    main()
