"""The run-time-shaped kernels across the PARAMETER range (tests/rt_param_range_cases.py has the table and says which code
in csrc/mnf_rt.h each family is for; tests/test_rt_param_range_host.py shows in float64 that every case gets there): a bias
2^36 times the largest weight, Linears whose maxima lie 2^24 apart, one hidden unit 2^24 times its neighbours, all-zero
weights, a +inf weight -- through the forward kernels (ahf_rt, nsf_rt, rnvp_rt; resident and streamed weights, MT_MAX 4 /
8 / 16) and through the gradient kernels (ahf_bwd_rt, nsf_bwd_rt, rnvp_bwd_rt), both directions where a layer has them.

Every comparison is against the float64 oracle -- outputs at RTOL + twice the fp32 oracle's own distance, y row by row and a
column of another magnitude on its own maximum; gradients at GBASE + the same -- and is recorded in helpers.PARITY_LOG /
GRAD_LOG (tests/test_zz_audit.py: 80 % rule).  profiles/r11/rt_param_range.txt (written by tools/rt_param_range_table.py):
the measured table, the fp32 VALU kernels on the same inputs, the rows beyond the envelope, and the builds that show the
cases bite.  tests/rt_deterministic_child.py runs the gradient half under MNF_DETERMINISTIC=1.

Measured (MI355X, profiles/r11/rt_param_range.txt): all 96 forward and 50 gradient cases hold, worst share of budget
ahf_rt 7 %, nsf_rt 45 %, rnvp_rt 4 %, ahf_bwd_rt 7 %, nsf_bwd_rt 60 %, rnvp_bwd_rt 50 %; the fp32 VALU kernels on the same
inputs: 70 % at most.  Before their fixes the gradient cases found two bugs in the *_bwd_rt kernels:
  pack_signs() took the LeakyReLU sign from the f16 head alone: a small positive unit whose head rounds to +0 (its row
      scaled down next to a 2^24 unit, or a hidden vector divided by 2^8) got slope 0.2 -- grad x 3.4e-2 / 6.8e-2 on
      ahf64 hidden_outlier, 9.6e-4 on nsf50-inv, 9.8e-5 .. 1.0e-3 on ahf10 / nsf50-fwd layer_spread (budget 1e-5)
  rnvp_bwd_rt gave the shift and the scale cotangent tiles ONE exchange scale per wave: a scale cotangent of 2^36 left the
      shift cotangents at 2^-24 -- grad t.weight 9.6e-5 / 8.9e-5 on rnvp50 / rnvp64 big_bias_head_2p36 (budget 1.1e-5)"""
import pytest

import rt_param_range_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


@pytest.mark.parametrize("case", P.FWD_CASES, ids=P.FWD_IDS)
def test_rt_forward_kernels_across_the_parameter_range(amd, case):
    P.run_forward(amd, case)


@pytest.mark.parametrize("case", P.GRAD_CASES, ids=P.GRAD_IDS)
def test_rt_gradient_kernels_across_the_parameter_range(amd, case):
    P.run_gradients(amd, case)
