"""The run-time-shaped gradient kernels outside the split range (tests/rt_bwd_range_cases.py has the table and says which
kernel path each family is for; tests/test_rt_bwd_range_host.py shows in float64 that every case gets there): outlier
and tiny cotangents, cotangents far off the sampled gradient scale, rows, activations and hidden vectors beyond 2^13,
weights of a wide dynamic range, a non-finite row, absent cotangents -- the counterparts of test_hip_autograd.py's
test_split_gradient_kernel_* for kernels that have no fp32 fix-up pass to hand such tiles to.

Every comparison is against the float64 oracle at the audited budget (GBASE + twice the fp32 oracle's own distance), is
recorded in helpers.GRAD_LOG (tests/test_zz_audit.py: 80 % rule), and grad_x is held a second time on the ordinary rows
alone, normalised by THEIR maximum.  profiles/r9/rt_bwd_range.txt: the measured table.  Cost: the shapes are round 6's
smallest; the slowest case measured 0.6 s (the one that loads the library), all 84 together 2 s -- reported there, not
asserted (a time limit in a test fails for reasons that are not the code's)."""
import pytest
import torch

import rt_bwd_range_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_rt_gradient_kernels_outside_the_split_range(amd, case):
    R.run_case(amd, case)


def test_one_node_training_run_outside_the_split_range(amd):
    """Three layers as one autograd node (fuse_rt_training: ahf_bwd_rt with its layer loop) and layer by layer, on a
    weighted NLL with an unsampled outlier weight and rows beyond 2^13: each route against the float64 oracle chain, and
    x.grad of the two bit for bit."""
    R.run_the_run(amd)
