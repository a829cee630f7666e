"""Host side of the run-time-shaped AffineHalfFlow run's gradient launch (mnf_affine_half_bwd_rt_stack and its
fixed-order form): symbols, the shape query, the argument checks and the Python switch -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_affine_half_bwd_rt_stack_supported", "mnf_affine_half_bwd_rt_stack",
       "mnf_affine_half_bwd_rt_stack_det_workspace", "mnf_affine_half_bwd_rt_stack_det")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    import torch_mnf_amd

    if not os.path.exists(torch_mnf_amd.library_path()):
        entry.build()
    return torch_mnf_amd._lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    import torch_mnf_amd

    raw = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", raw).group(1))
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 18


SHAPES = [(64, (24, 24), 1, 1), (64, (64, 64, 64), 1, 1), (10, (16, 40), 1, 1), (2, (24, 24), 1, 1), (512, (24, 24, 24), 1, 1),
          (64, (24, 24), 0, 1), (64, (24, 24), 1, 0), (64, (24, 24), 0, 0), (64, (20, 30, 40, 50), 1, 1), (64, (24,) * 5, 1, 1),
          (64, (65,), 1, 1), (64, (2, 24), 1, 1), (63, (24, 24), 1, 1), (64, (), 1, 1), (256, (64, 64, 64), 1, 1)]


@pytest.mark.parametrize("dim,hs,scale,shift", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_supported_query_follows_the_single_layer_query(lib, dim, hs, scale, shift):
    """One plan: n_layers = 1 answers what mnf_affine_half_bwd_rt_supported answers, and (no shape class was measured
    out) so do 2 .. 32 layers; 0 and 33 layers are refused."""
    from torch_mnf_amd._lib import int_array

    hid = int_array(list(hs)) if hs else None
    one = lib.mnf_affine_half_bwd_rt_supported(dim, len(hs), hid, scale, shift)
    for n in (1, 2, 9, 32):
        assert lib.mnf_affine_half_bwd_rt_stack_supported(dim, len(hs), hid, scale, shift, n) == one
    for n in (0, 33, -1):
        assert lib.mnf_affine_half_bwd_rt_stack_supported(dim, len(hs), hid, scale, shift, n) == 0


def test_supported_query_refuses_what_the_issue_names(lib):
    from torch_mnf_amd._lib import int_array

    q = lib.mnf_affine_half_bwd_rt_stack_supported
    assert q(64, 2, int_array([24, 24]), 1, 1, 9) == 1
    assert q(64, 2, int_array([24, 24]), 1, 1, 0) == 0 and q(64, 2, int_array([24, 24]), 1, 1, 33) == 0
    assert q(63, 2, int_array([24, 24]), 1, 1, 9) == 0   # odd dim
    assert q(64, 1, int_array([65]), 1, 1, 9) == 0       # a hidden width of 65
    # no device is visible here or the query refuses: no workspace either way
    assert lib.mnf_affine_half_bwd_rt_stack_det_workspace(4096, 64, 1, int_array([65]), 1, 1, 3) == 0
    assert lib.mnf_affine_half_bwd_rt_stack_det_workspace(4096, 64, 2, int_array([24, 24]), 1, 1, 33) == 0
    assert lib.mnf_affine_half_bwd_rt_stack_det_workspace(0, 64, 2, int_array([24, 24]), 1, 1, 3) == 0


def test_argument_checking_without_a_gpu(lib):
    """Every refusal below comes back before any launch (host memory stands in for the device pointers)."""
    from torch_mnf_amd import _lib
    from torch_mnf_amd._lib import int_array

    hid, par = int_array([24, 24]), int_array([0, 1, 0])
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    ok = dict(x=p, outs=p + 1024, gy=p + 2048, lp=None, gl=p + 3072, gx=p + 4096, work=p + 5120, gf=p + 6144, flats=p + 7168,
              sc=p + 8192, par=par, n=3, rows=4, dim=64, inv=0, nh=2, hid=hid, s=1, t=1)

    def go(det=False, ws=None, ws_n=0, **kw):
        a = {**ok, **kw}
        args = (a["x"], a["outs"], a["gy"], a["lp"], a["gl"], a["gx"], a["work"], a["gf"], a["flats"], a["sc"], a["par"], a["n"],
                a["rows"], a["dim"], a["inv"], a["nh"], a["hid"], a["s"], a["t"])
        if det:
            return lib.mnf_affine_half_bwd_rt_stack_det(*args, ws, ws_n, None)
        return lib.mnf_affine_half_bwd_rt_stack(*args, None)

    bad = _lib.MNF_ERR_INVALID_ARG
    for det in (False, True):
        kw = dict(det=det, ws=p + 9216, ws_n=1 << 20)
        assert go(lp=p + 3072, **kw) == bad                              # both cotangent forms
        assert go(lp=p + 3072, gy=None, **kw) == bad and go(lp=p + 3072, gl=None, **kw) == bad
        assert go(x=None, **kw) == bad and go(outs=None, **kw) == bad and go(gx=None, **kw) == bad
        assert go(flats=None, **kw) == bad and go(sc=None, **kw) == bad and go(par=None, **kw) == bad
        assert go(work=None, **kw) == bad and go(work=ok["gx"], **kw) == bad   # a run needs the second cotangent plane
        assert go(n=0, **kw) == bad and go(n=33, **kw) == bad
        assert go(dim=63, **kw) == bad and go(rows=-1, **kw) == bad and go(s=0, t=0, **kw) == bad
        assert go(x=p + 2, **kw) == bad                                  # not even float-aligned
        assert go(rows=0, **kw) == _lib.MNF_OK                           # empty batch: no launch, no device needed
        assert go(rows=0, lp=p + 3072, gy=None, gl=None, **kw) == _lib.MNF_OK
        assert go(rows=0, n=1, work=None, **kw) == _lib.MNF_OK
    assert go(det=True, ws=None, ws_n=0) == bad                          # parameter sums wanted, nowhere to put the slots
    assert go(det=True, ws=p + 9216, ws_n=0) == bad
    assert go(det=True, ws=None, ws_n=0, rows=0) == _lib.MNF_OK


def test_kernel_family_name_is_in_the_rt_tier():
    from torch_mnf_amd import _dispatch

    assert _dispatch.tier_of_kernel("ahf_bwd_stack_rt") == "rt"
    assert _dispatch.tier_of_kernel("ahf_bwd_rt") == "rt"
    assert "fuse_rt_training" in _dispatch.__doc__


def test_the_switch_is_off_by_default():
    import torch_mnf_amd as amd

    assert amd.NormalizingFlow([]).fuse_rt_training is False
    layers = [amd.AffineHalfFlow(8, parity=bool(i % 2), h_sizes=(12,)) for i in range(2)]
    assert amd.FusedAffineStack(layers).fuse_rt_training is False
    assert amd.NormalizingFlowModel(None, layers).fuse_rt_training is False
