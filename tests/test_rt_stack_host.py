"""Host side of the run-time-shaped AffineHalfFlow run (mnf_affine_half_rt_stack): symbols, the shape query and the
argument checks -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_affine_half_rt_stack", "mnf_affine_half_rt_stack_supported")


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

    header = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 17
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mnf_affine_half_rt_stack" in table


SHAPES = [(64, (24, 24), 1, 1), (512, (24, 24, 24), 1, 1), (256, (200, 130, 40, 7), 1, 1), (6, (5, 9), 1, 1),
          (64, (24, 24), 0, 1), (64, (24, 24), 1, 0), (64, (24, 24), 0, 0), (64, (2, 24), 1, 1), (64, (300,), 1, 1),
          (63, (24, 24), 1, 1), (64, (), 1, 1), (40, (256,), 1, 1)]


@pytest.mark.parametrize("dim,hs,scale,shift", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_supported_query_follows_the_single_layer_query(lib, dim, hs, scale, shift):
    from torch_mnf_amd._lib import int_array

    hid = int_array(list(hs)) if hs else None
    one = lib.mnf_affine_half_rt_supported(dim, len(hs), hid, scale, shift)
    assert lib.mnf_affine_half_rt_stack_supported(dim, len(hs), hid, scale, shift, 1) == one
    # measured out (csrc/mnf_ahf_rt.hip ahf_rt_stack_ok): runs of the widest class's streaming shapes -- hidden widths
    # beyond 128 whose conditioner does not fit LDS -- are no faster in one launch; one layer is today's call
    excluded = (dim, hs) == (256, (200, 130, 40, 7))
    for n in (2, 9, 32):
        assert lib.mnf_affine_half_rt_stack_supported(dim, len(hs), hid, scale, shift, n) == (0 if excluded else one)
    for n in (0, 33, -1):
        assert lib.mnf_affine_half_rt_stack_supported(dim, len(hs), hid, scale, shift, n) == 0


def test_supported_query_refuses_what_the_issue_names(lib):
    from torch_mnf_amd._lib import int_array

    q = lib.mnf_affine_half_rt_stack_supported
    assert q(64, 2, int_array([24, 24]), 1, 1, 9) == 1
    assert q(64, 2, int_array([2, 24]), 1, 1, 9) == 0    # a hidden width of 2
    assert q(64, 1, int_array([300]), 1, 1, 9) == 0      # ... of 300
    assert q(63, 2, int_array([24, 24]), 1, 1, 9) == 0   # odd dim
    assert q(64, 2, int_array([24, 24]), 1, 1, 0) == 0 and q(64, 2, int_array([24, 24]), 1, 1, 33) == 0


def test_argument_checking_without_a_gpu(lib):
    from torch_mnf_amd import _lib
    from torch_mnf_amd._lib import int_array

    hid, par = int_array([24, 24]), int_array([0, 1, 0])
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf)
    call = lib.mnf_affine_half_rt_stack
    ok = dict(x=p, y=p + 1024, mid=None, ld=None, sq=None, lp=None, total=None, acc=0, flats=p + 2048, par=par, n=3, rows=4,
              dim=64, inv=0, nh=2, hid=hid, s=1, t=1, stream=None)

    def go(**kw):
        a = {**ok, **kw}
        return call(a["x"], a["y"], a["mid"], a["ld"], a["sq"], a["lp"], a["total"], a["acc"], a["flats"], a["par"], a["n"],
                    a["rows"], a["dim"], a["inv"], a["nh"], a["hid"], a["s"], a["t"], a["stream"])

    bad = _lib.MNF_ERR_INVALID_ARG
    assert go(flats=None) == bad
    assert go(x=None) == bad and go(y=None) == bad and go(y=p) == bad and go(par=None) == bad
    assert go(n=0) == bad and go(n=33) == bad
    assert go(dim=63) == bad and go(rows=-1) == bad
    assert go(x=p + 2) == bad and go(flats=p + 2049) == bad            # not even float-aligned
    assert go(lp=p + 512) == bad                                       # the epilogue needs log_det
    assert go(total=p + 516, ld=p + 512) == bad                        # a misaligned double
    assert go(s=0, t=0) == bad
    assert go(rows=0) == 0                                             # empty batch: no launch, no device needed
    assert go(rows=0, n=32, par=int_array([0] * 32)) == 0
    assert go(rows=0, hid=int_array([2, 24])) == 0


def test_kernel_family_name_is_in_the_rt_tier():
    from torch_mnf_amd import _dispatch

    assert _dispatch.tier_of_kernel("ahf_stack_rt") == "rt"
    assert _dispatch.tier_of_kernel("ahf_rt") == "rt"
