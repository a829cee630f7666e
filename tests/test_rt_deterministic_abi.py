"""The fixed-order forms of the run-time-shaped gradient launches (include/mnf_hip.h mnf_*_bwd_rt_det and their
*_det_workspace queries): declared, bound, and checking their arguments before any launch -- no GPU needed."""
import ctypes

import pytest

DET = ["mnf_affine_half_bwd_rt_det", "mnf_nsf_cl_bwd_rt_det", "mnf_rnvp_bwd_rt_det"]
QUERIES = [n + "_workspace" for n in DET]


@pytest.fixture(scope="module")
def lib():
    from torch_mnf_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def _lib():
    from torch_mnf_amd import _lib

    return _lib


def test_the_six_entries_are_declared_and_bound(lib, _lib):
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mnf_hip.h")).read()
    for name in DET + QUERIES:
        assert name in _lib.SIGNATURES, name
        assert f" {name}(" in header, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name


def _buf(n=4096):
    return (ctypes.c_float * n)()


def _addr(b):
    return ctypes.addressof(b)


def test_argument_checks_come_before_any_launch(lib, _lib):
    """A NULL pointer or a non-empty batch without a workspace: MNF_ERR_INVALID_ARG, whatever the mode and without a GPU
    (host buffers: nothing may be launched on them)."""
    x, y, g, gx, gf, flat, sc, ws = (_addr(_buf()) for _ in range(8))
    hid = _lib.int_array([24, 24])
    bad = _lib.MNF_ERR_INVALID_ARG
    # AffineHalfFlow(64, (24, 24))
    ahf = lambda x_, gf_, ws_, n: lib.mnf_affine_half_bwd_rt_det(x_, None, g, None, gx, gf_, flat, sc, 100, 64, 0, 0, 2, hid,
                                                                 1, 1, ws_, n, None)
    assert ahf(None, gf, ws, 1 << 20) == bad
    assert ahf(x, gf, None, 1 << 20) == bad
    assert ahf(x, gf, ws, 0) == bad
    assert lib.mnf_affine_half_bwd_rt_det(x, None, g, None, None, gf, flat, sc, 100, 64, 0, 0, 2, hid, 1, 1, ws, 1 << 20,
                                          None) == bad  # grad_x
    assert lib.mnf_affine_half_bwd_rt_det(x, None, g, None, gx, gf, None, sc, 100, 64, 0, 0, 2, hid, 1, 1, ws, 1 << 20,
                                          None) == bad  # flat
    # NSF_CL(128, K=8, n_h=32)
    h3 = _lib.int_array([32, 32, 32])
    nsf = lambda x_, y_, ws_, n: lib.mnf_nsf_cl_bwd_rt_det(x_, y_, g, None, gx, gf, flat, sc, 100, 128, 8, 3.0, 0, 3, h3,
                                                           ws_, n, None)
    assert nsf(None, y, ws, 1 << 20) == bad
    assert nsf(x, None, ws, 1 << 20) == bad
    assert nsf(x, y, None, 1 << 20) == bad
    assert nsf(x, y, ws, 0) == bad
    # RNVP(800, (100,))
    h1 = _lib.int_array([100])
    rnvp = lambda z_, gz_, ws_, n: lib.mnf_rnvp_bwd_rt_det(z_, None, 7, g, None, gz_, gf, flat, sc, 100, 800, 1, h1, ws_, n,
                                                           None)
    assert rnvp(None, gx, ws, 1 << 20) == bad
    assert rnvp(x, None, ws, 1 << 20) == bad
    assert rnvp(x, gx, None, 1 << 20) == bad
    assert rnvp(x, gx, ws, 0) == bad
    # an empty batch needs no workspace
    assert lib.mnf_rnvp_bwd_rt_det(x, None, 7, g, None, gx, gf, flat, sc, 0, 800, 1, h1, None, 0, None) == _lib.MNF_OK


@pytest.mark.parametrize("kind,dim,hidden,K", [("ahf", 64, (300,), None), ("ahf", 64, (64,) * 5, None), ("ahf", 63, (24, 24), None),
                                               ("nsf", 128, (64, 64, 64), 16), ("nsf", 16, (3, 3, 3), 8),
                                               ("rnvp", 100, (200,), None), ("rnvp", 100, (128,) * 5, None)])
def test_workspace_queries_refuse_what_the_kernels_refuse(lib, _lib, kind, dim, hidden, K):
    hid, n = _lib.int_array(hidden), len(hidden)
    if kind == "ahf":
        assert lib.mnf_affine_half_bwd_rt_supported(dim, n, hid, 1, 1) == 0
        assert lib.mnf_affine_half_bwd_rt_det_workspace(65536, dim, n, hid, 1, 1) == 0
    elif kind == "nsf":
        assert lib.mnf_nsf_cl_bwd_rt_supported(dim, K, n, hid) == 0
        assert lib.mnf_nsf_cl_bwd_rt_det_workspace(65536, dim, K, n, hid) == 0
    else:
        assert lib.mnf_rnvp_bwd_rt_supported(dim, n, hid) == 0
        assert lib.mnf_rnvp_bwd_rt_det_workspace(65536, dim, n, hid) == 0


def test_workspace_queries_of_an_empty_batch_are_zero(lib, _lib):
    hid = _lib.int_array([24, 24])
    assert lib.mnf_affine_half_bwd_rt_supported(64, 2, hid, 1, 1) == 1
    assert lib.mnf_affine_half_bwd_rt_det_workspace(0, 64, 2, hid, 1, 1) == 0
    assert lib.mnf_nsf_cl_bwd_rt_det_workspace(0, 128, 8, 2, hid) == 0
    assert lib.mnf_rnvp_bwd_rt_det_workspace(0, 800, 2, hid) == 0


def test_the_deterministic_mode_warning_names_layer_shape_and_switch_once(_lib):
    """The warning a deterministic-mode gradient pass on an atomic kernel raises names the layer, its shape and the
    switch, and never says 'failed' (tests/test_hip_round5.py greps a deterministic-mode child's output for it)."""
    import warnings

    from torch_mnf_amd import _lib as L

    saved = L.deterministic, L.last_kernel
    L.deterministic = lambda: True
    L.last_kernel = lambda: "ahf_bwd_generic"
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            L.note_atomic_sums("AffineHalfFlow.backward", "dim=64, hidden=(128,) [abi test]")
            L.note_atomic_sums("AffineHalfFlow.backward", "dim=64, hidden=(128,) [abi test]")
        L.last_kernel = lambda: "ahf_bwd_rt"
        with warnings.catch_warnings(record=True) as w2:
            warnings.simplefilter("always")
            L.note_atomic_sums("AffineHalfFlow.backward", "dim=64, hidden=(24, 24) [abi test]")
    finally:
        L.deterministic, L.last_kernel = saved
    assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning), w
    text = str(w[0].message)
    assert "AffineHalfFlow" in text and "hidden=(128,)" in text and "MNF_DETERMINISTIC" in text
    assert "failed" not in text.lower()
    assert not w2
