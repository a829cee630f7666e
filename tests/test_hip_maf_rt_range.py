"""The MAF / IAF matrix-core kernels across the operating and the parameter range (tests/maf_rt_range_cases.py has the layer
table and the three case tables and says which code each family is for; tests/test_maf_rt_range_host.py shows in float64 that
every case gets there and that every layer has the plan the table claims): rows and late-decoded elements beyond 2^13,
hidden vectors beyond 2^13, large output heads, a non-finite input, cotangents of a mean loss, of 40 and with unsampled
outliers at 2^17, a bias 2^36 times the largest weight, MaskedLinears whose maxima lie 2^24 apart, one hidden unit 2^24 times
its neighbours, all-zero weights, a +inf weight, 2^40 parked in every masked-out weight -- through maf_rt (resident and
streamed weights) and maf_seq_rt, and through maf_bwd_rt and maf_seq_bwd_rt (the solve route is opted in as
tests/test_hip_maf_seq_bwd_rt.py does).  Every case names the kernel it ran.

Every comparison is against the float64 oracle (O.maf with O.made_masks) -- outputs at RTOL + twice the fp32 oracle's own
distance, capped by MAX_WIDENING, y row by row, a column of another magnitude on its own maximum, log_det of the special and
of the ordinary rows as tensors of their own; gradients at GBASE + the same, grad_x of the ordinary rows on its own norm,
masked-out entries exactly zero -- and is recorded in helpers.PARITY_LOG / GRAD_LOG (tests/test_zz_audit.py: 80 % rule).
profiles/r24/maf_rt_range.txt (written by tools/maf_rt_range_table.py): the measured tables of both kernel tiers.  The
children tests/maf_rt_deterministic_child.py and tests/maf_seq_bwd_rt_deterministic_child.py run one layer's cot_small,
cot_outlier and big_rows gradient cases under MNF_DETERMINISTIC=1.

Measured (MI355X, profiles/r24/maf_rt_range.txt): all 66 + 58 + 63 + 48 cases hold; worst share of budget maf_rt 14 %,
maf_seq_rt 8 %, maf_seq_bwd_rt 48 %, maf_bwd_rt 8 %; the fp32 VALU kernels on the same inputs: 11 % at most.  STRESS and
LEFT_OUT_* are empty.  Before its fix the forward table found one bug: finish_layer's ReLU was a v_max_f32 under
-fno-honor-nans, which answers 0 for a NaN -- the row with the inf came out finite in every column but one (all 11
nonfinite_row cases).  The element-by-element direction's big_bias_head cases take 2^24 (forward) and 2^21 (gradients) in
place of 2^36: the decoded y_j enters the row the net reads, and one scale per row is the split format's stated limit (2^36:
y 1.2e-5 .. 4.7e-5, gradients 1.6e-2 .. 1.7e-1; 2^24: gradients 2.5e-5 .. 6.0e-5; the table in tests/maf_rt_range_cases.py).

The gradient table found a second one: big_hidden (first MaskedLinear x 4500, second / 4500) hands the first layer deltas of
2^-14 and less in units of the gradient scale, and backward_tail's exchange_store / split_rows only ever scaled DOWN -- the
deltas were f16 subnormals throughout, carried to 2^-36 absolute: grad net.0.weight 9.25e-6 of a budget of 1.05e-5 on
(37, (20, 7, 33)) (88 %; (64, 24x3) 65 %; maf_bwd_generic 3 %), above tests/test_zz_audit.py's 80 %.  Fixed in
csrc/mnf_rt_bwd.h (delta_exponent: a masked chain's delta whose maximum is below 2^-6 is scaled up as well): 7 % / 2 %."""
import pytest

import maf_rt_range_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    import torch_mnf_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch_mnf_amd


@pytest.fixture(autouse=True)
def opted_in(monkeypatch):
    from torch_mnf_amd import _dispatch

    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 0)


@pytest.mark.parametrize("case", M.FWD_CASES, ids=M.FWD_IDS)
def test_maf_forward_kernels_across_the_operating_range(amd, case):
    got = M.run_forward(amd, case, force_generic=2)
    assert got["kernel"] == ("maf_rt" if case.inverse else "maf_seq_rt") == amd.last_kernel()


@pytest.mark.parametrize("case", M.GRAD_CASES, ids=M.GRAD_IDS)
def test_maf_gradient_kernels_across_the_operating_range(amd, case):
    M.run_gradients(amd, case, force_generic=2)
    assert amd.last_kernel() == ("maf_bwd_rt" if case.inverse else "maf_seq_bwd_rt")


@pytest.mark.parametrize("case", M.PARAM_FWD_CASES, ids=M.PARAM_FWD_IDS)
def test_maf_forward_kernels_across_the_parameter_range(amd, case):
    got = M.run_forward(amd, case, force_generic=2)
    assert got["kernel"] == ("maf_rt" if case.inverse else "maf_seq_rt") == amd.last_kernel()


@pytest.mark.parametrize("case", M.PARAM_GRAD_CASES, ids=M.PARAM_GRAD_IDS)
def test_maf_gradient_kernels_across_the_parameter_range(amd, case):
    M.run_gradients(amd, case, force_generic=2)
    assert amd.last_kernel() == ("maf_bwd_rt" if case.inverse else "maf_seq_bwd_rt")
