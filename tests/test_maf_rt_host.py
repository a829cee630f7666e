"""Host side of the MAF / IAF one-pass kernels on the matrix cores (mnf_maf_rt, mnf_maf_bwd_rt and its fixed-order form):
symbols, the shape queries at the envelope's edges, the argument checks, the empty batch, the dispatch tier and the
layer's own route -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_maf_rt_supported", "mnf_maf_bwd_rt_supported", "mnf_maf_rt", "mnf_maf_rt_grid", "mnf_maf_bwd_rt",
       "mnf_maf_bwd_rt_det_workspace", "mnf_maf_bwd_rt_det")
FWD_MAX, BWD_MAX = 128, 64  # widest hidden layer of the forward / the gradient kernel (include/mnf_hip.h)


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    import torch_mnf_amd

    if not os.path.exists(torch_mnf_amd.library_path()):
        entry.build()
    return torch_mnf_amd._lib.load()


def arr(*h):
    from torch_mnf_amd._lib import int_array

    return int_array(list(h))


def test_new_symbols_are_declared_exported_and_bound(lib):
    import torch_mnf_amd

    header = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 21
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mnf_maf_rt", "mnf_maf_bwd_rt", "maf_rt", "maf_bwd_rt"):
        assert name in table


def test_supported_queries_at_the_envelope_edges(lib):
    fwd, bwd = lib.mnf_maf_rt_supported, lib.mnf_maf_bwd_rt_supported
    for q, widest in ((fwd, FWD_MAX), (bwd, BWD_MAX)):
        assert q(6, 1, arr(3)) == 0 and q(6, 1, arr(4)) == 1
        assert q(6, 1, arr(widest)) == 1 and q(6, 1, arr(widest + 1)) == 0
        assert q(6, 3, arr(24, 3, 24)) == 0 and q(6, 3, arr(24, widest + 1, 24)) == 0  # every layer counts
        assert q(1, 1, arr(8)) == 1 and q(0, 1, arr(8)) == 0 and q(-2, 1, arr(8)) == 0  # dim = 1 is a shape
        assert q(6, 1, None) == 0 and q(6, 1, arr(0)) == 0 and q(6, 1, arr(-4)) == 0
        assert q(6, 0, None) == 0 and q(6, 0, arr(8)) == 0
        assert q(2, 3, arr(24, 24, 24)) == 1 and q(37, 3, arr(20, 7, 33)) == 1 and q(100, 4, arr(16, 16, 16, 16)) == 1
    # the forward kernel has no layer limit but the library's own (MNF_MAX_LINEAR); the gradient kernel keeps four vectors
    assert fwd(6, 5, arr(8, 8, 8, 8, 8)) == 1 and bwd(6, 5, arr(8, 8, 8, 8, 8)) == 0
    assert bwd(6, 4, arr(8, 8, 8, 8)) == 1
    assert fwd(130, 2, arr(128, 128)) == 1 and fwd(4096, 1, arr(64)) == 1  # streaming: any dim
    assert fwd(40, 1, arr(128)) == 1 and bwd(40, 1, arr(128)) == 0


def test_argument_errors_come_before_any_launch(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 8192)()
    p = ctypes.addressof(buf)
    x, y, ld, flat, masks, gx, gf, sc, ws = (p + 4096 * i for i in range(9))
    bad, unsupported, hid = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, arr(8)
    fwd = lib.mnf_maf_rt
    assert fwd(None, y, ld, 0, flat, masks, 4, 6, 0, 1, hid, None) == bad
    assert fwd(x, None, ld, 0, flat, masks, 4, 6, 0, 1, hid, None) == bad
    assert fwd(x, x, ld, 0, flat, masks, 4, 6, 0, 1, hid, None) == bad          # x and y alias
    assert fwd(x, y, ld, 0, None, masks, 4, 6, 0, 1, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, None, 4, 6, 0, 1, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, masks, -1, 6, 0, 1, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, masks, 4, 0, 0, 1, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, masks, 4, 6, 0, 0, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, masks, 4, 6, 0, 1, None, None) == bad         # malformed hidden
    assert fwd(x, y, ld, 0, flat, masks, 4, 6, 0, 1, arr(0), None) == bad
    assert fwd(x, y, ld, 0, flat, masks, 4, 6, 0, 1, arr(3), None) == unsupported
    assert fwd(x, y, ld, 0, flat, masks, 4, 6, 0, 1, arr(FWD_MAX + 1), None) == unsupported
    assert fwd(x, y, ld, 0, flat, masks, 0, 6, 1, 1, hid, None) == _lib.MNF_OK  # empty batch: no launch, no device needed
    assert fwd(x, y, None, 0, flat, masks, 0, 6, 1, 1, hid, None) == _lib.MNF_OK
    for det in (False, True):
        call = lib.mnf_maf_bwd_rt_det if det else lib.mnf_maf_bwd_rt
        tail = (ws, 1024, None) if det else (None,)

        def bwd(*a):
            return call(*a, *tail)

        assert bwd(None, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 1, hid) == bad
        assert bwd(x, y, ld, None, gf, flat, masks, sc, 4, 6, 0, 1, hid) == bad
        assert bwd(x, y, ld, x, gf, flat, masks, sc, 4, 6, 0, 1, hid) == bad     # grad_x aliases x
        assert bwd(x, y, ld, y, gf, flat, masks, sc, 4, 6, 0, 1, hid) == bad     # grad_x aliases grad_y
        assert bwd(x, y, ld, gx, flat, flat, masks, sc, 4, 6, 0, 1, hid) == bad  # grad_flat aliases flat
        assert bwd(x, y, ld, gx, gf, None, masks, sc, 4, 6, 0, 1, hid) == bad
        assert bwd(x, y, ld, gx, gf, flat, None, sc, 4, 6, 0, 1, hid) == bad
        assert bwd(x, y, ld, gx, gf, flat, masks, None, 4, 6, 0, 1, hid) == bad
        assert bwd(x, y, ld, gx, gf, flat, masks, sc, -1, 6, 0, 1, hid) == bad
        assert bwd(x, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 1, None) == bad
        assert bwd(x, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 0, hid) == bad
        assert bwd(x, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 1, arr(BWD_MAX + 1)) == unsupported
        assert bwd(x, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 5, arr(8, 8, 8, 8, 8)) == unsupported
        assert bwd(x, y, ld, gx, gf, flat, masks, sc, 0, 6, 0, 1, hid) == _lib.MNF_OK
        assert bwd(x, None, None, gx, None, flat, masks, sc, 0, 6, 1, 1, hid) == _lib.MNF_OK
    # the fixed-order form: parameter sums wanted, rows to run, no workspace
    assert lib.mnf_maf_bwd_rt_det(x, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 1, hid, None, 0, None) == bad
    assert lib.mnf_maf_bwd_rt_det(x, y, ld, gx, gf, flat, masks, sc, 4, 6, 0, 1, hid, ws, 0, None) == bad


def test_queries_that_need_a_device_are_zero_without_one(lib):
    import torch

    ws, grid = lib.mnf_maf_bwd_rt_det_workspace, lib.mnf_maf_rt_grid
    assert ws(0, 6, 1, arr(8)) == 0 and ws(-5, 6, 1, arr(8)) == 0 and ws(4096, 6, 1, arr(3)) == 0
    assert ws(4096, 6, 5, arr(8, 8, 8, 8, 8)) == 0 and ws(4096, 6, 1, None) == 0
    assert grid(0, 6, 1, arr(8)) == 0 and grid(4096, 6, 1, arr(3)) == 0
    n, g = ws(4096, 6, 2, arr(16, 16)), grid(4096, 6, 2, arr(16, 16))
    if torch.cuda.is_available():
        assert n > 0 and n % 64 == 0 and 1 <= g <= 32
    else:
        assert n == 0 and g == 0


def test_tier_of_a_maf_call(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    default = _dispatch.MAF_RT_MIN_ROWS
    assert default is None or default >= _dispatch.RT_MIN_ROWS >= 2048
    assert default is None or default > 257  # every MAF test of the earlier rounds stays on the kernels it ran
    if default is None:  # opt-in: no row count reaches the kernels by itself
        assert tier("maf", "fwd", 1 << 20, 6, (16, 16)) == "valu" and tier("maf", "bwd", 1 << 20, 6, (16, 16)) == "valu"
    monkeypatch.setattr(_dispatch, "MAF_RT_MIN_ROWS", 8192)
    for direction in ("fwd", "bwd"):
        assert tier("maf", direction, 8191, 6, (16, 16)) == "valu"
        assert tier("maf", direction, 8192, 6, (16, 16)) == "rt"
        assert tier("maf", direction, 1 << 20, 2, (24, 24, 24)) == "rt"
        assert tier("maf", direction, 1 << 20, 6, (3,)) == "valu"
        assert tier("maf", direction, 1 << 20, 6, (FWD_MAX + 1,)) == "valu"
    assert tier("maf", "fwd", 1 << 20, 40, (128,)) == "rt" and tier("maf", "bwd", 1 << 20, 40, (128,)) == "valu"
    assert tier("maf", "fwd", 1 << 20, 6, (8,) * 5) == "rt" and tier("maf", "bwd", 1 << 20, 6, (8,) * 5) == "valu"
    monkeypatch.setattr(_dispatch, "MAF_RT_MIN_ROWS", 16)  # never below wants_rt's own number
    assert tier("maf", "fwd", _dispatch.RT_MIN_ROWS - 1, 6, (16, 16)) == "valu"
    assert tier("maf", "fwd", _dispatch.RT_MIN_ROWS, 6, (16, 16)) == "rt"
    assert _dispatch.tier_of_kernel("maf_rt") == "rt" and _dispatch.tier_of_kernel("maf_bwd_rt") == "rt"
    assert _dispatch.tier_of_kernel("maf_generic") == "valu" and _dispatch.tier_of_kernel("maf_bwd_generic") == "valu"
    # the other kinds answer as before
    assert tier("ahf", "fwd", 4096, 64, (24, 24, 24)) == "per-shape"


def test_the_layers_route(lib, monkeypatch):
    """flows.MAF._rt: the one-pass direction only; force_generic = 1 / 2 as elsewhere; an fp32 request stays off the
    split-f16 kernels; below MAF_RT_MIN_ROWS (or with None) the route is the VALU kernel's."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    maf = amd.MAF(6, parity=True, h_sizes=(16, 16))
    monkeypatch.setattr(_dispatch, "MAF_RT_MIN_ROWS", None)
    assert not maf._rt(1 << 20, False) and not maf._rt(1 << 20, False, bwd=True)
    maf.force_generic = 2
    assert maf._rt(5, False) and maf._rt(5, False, bwd=True) and not maf._rt(5, True) and not maf._rt(1 << 20, True, bwd=True)
    maf.force_generic = 0
    monkeypatch.setattr(_dispatch, "MAF_RT_MIN_ROWS", 4096)
    assert maf._rt(4096, False) and maf._rt(4096, False, bwd=True) and not maf._rt(4095, False) and not maf._rt(4096, True)
    maf.force_fp32_mfma = True
    assert not maf._rt(1 << 20, False) and not maf._rt(1 << 20, False, bwd=True)
    maf.force_fp32_mfma = False
    maf.force_generic = 1
    assert not maf._rt(1 << 20, False)
    wide = amd.MAF(40, parity=False, h_sizes=(128,))
    assert wide._rt(4096, False) and not wide._rt(4096, False, bwd=True)
    narrow = amd.IAF(6, parity=False, h_sizes=(3,))
    narrow.force_generic = 2
    assert not narrow._rt(4096, False)
