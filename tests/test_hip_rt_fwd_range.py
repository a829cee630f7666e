"""The run-time-shaped forward kernels (ahf_rt, ahf_stack_rt, nsf_rt, rnvp_rt) outside the split range
(tests/rt_fwd_range_cases.py has the table and says which code in csrc/mnf_rt.h each family is for;
tests/test_rt_fwd_range_host.py shows in float64 that every case gets there): rows and hidden vectors beyond 2^13 in
some 16-row tiles and not in others, conditioner outputs far beyond scale 1, a non-finite row -- in every size class
(MT_MAX 4 / 8 / 16), with resident and with streamed weights, forward and inverse.

Every comparison is against the float64 oracle at RTOL + twice the fp32 oracle's own distance, y row by row, and is
recorded in helpers.PARITY_LOG (tests/test_zz_audit.py: 80 % rule); the conditioning half / the elements beyond the tail
bound pass through bit for bit; rows beyond the range leave every other row's bits alone.
profiles/r10/rt_fwd_range.txt (written by tools/rt_fwd_range_table.py): the measured table, the fp32 VALU kernels on the
same inputs, three scratch builds that show the cases bite, and the cost -- slowest case 0.5 s (the one that loads the
library), all 117 together 1.4 s; reported there, not asserted (a time limit in a test fails for reasons that are not
the code's)."""
import pytest

import rt_fwd_range_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


@pytest.mark.parametrize("case", F.CASES, ids=F.CASE_IDS)
def test_rt_forward_kernels_outside_the_split_range(amd, case):
    F.run_case(amd, case)


def test_stack_outside_the_split_range(amd):
    """Three (64, (24, 24)) layers as one ahf_stack_rt launch on rows beyond 2^13: every intermediate, log_det and the
    fused log-prob against the float64 chain; the layer-by-layer route and the rows' independence bit for bit."""
    F.run_stack(amd)
