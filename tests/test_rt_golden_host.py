"""Host side of the reference fixtures on the run-time-shaped tier (tests/test_hip_parity.py's "rt" parametrisations,
tests/test_hip_rt_golden.py): for every shape those tests force onto the tier, the library's own query says it has the
shape -- a layer with ``force_generic = 2`` whose shape the tier lacks is served by the VALU kernels, and a GPU case must
not be quietly served by another tier.  No GPU."""
import pytest

import rt_golden_cases as RG
from torch_mnf_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("what,dim,hs,scale,shift,run,grads", RG.ahf_shapes(), ids=[s[0] for s in RG.ahf_shapes()])
def test_affine_half_shapes_are_on_the_tier(lib, what, dim, hs, scale, shift, run, grads):
    hid, n = _lib.int_array(list(hs)), len(hs)
    assert lib.mnf_affine_half_rt_supported(dim, n, hid, int(scale), int(shift)) == 1
    if run:
        assert lib.mnf_affine_half_rt_stack_supported(dim, n, hid, int(scale), int(shift), run) == 1
    if grads:
        assert lib.mnf_affine_half_bwd_rt_supported(dim, n, hid, int(scale), int(shift)) == 1
        if run:
            assert lib.mnf_affine_half_bwd_rt_stack_supported(dim, n, hid, int(scale), int(shift), run) == 1


@pytest.mark.parametrize("what,dim,K,n_h,grads", RG.nsf_shapes(), ids=[s[0] for s in RG.nsf_shapes()])
def test_nsf_cl_shapes_are_on_the_tier(lib, what, dim, K, n_h, grads):
    hid = _lib.int_array([n_h] * 3)
    assert lib.mnf_nsf_cl_rt_supported(dim, K, 3, hid) == 1
    if grads:
        assert lib.mnf_nsf_cl_bwd_rt_supported(dim, K, 3, hid) == 1


@pytest.mark.parametrize("what,dim,hs,grads", RG.rnvp_shapes(), ids=[s[0] for s in RG.rnvp_shapes()])
def test_rnvp_shapes_are_on_the_tier(lib, what, dim, hs, grads):
    hid = _lib.int_array(list(hs))
    assert lib.mnf_rnvp_rt_supported(dim, len(hs), hid) == 1
    if grads:
        assert lib.mnf_rnvp_bwd_rt_supported(dim, len(hs), hid) == 1


@pytest.mark.parametrize("what,dim", RG.glow_dims(), ids=[s[0] for s in RG.glow_dims()])
def test_glow_dims_are_on_the_tier(lib, what, dim):
    assert lib.mnf_linear_rows_rt_supported(dim) == 1
    if what.startswith("block"):
        assert lib.mnf_glow_actnorm_inv_rt_supported(dim) == 1
