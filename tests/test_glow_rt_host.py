"""Host side of Glow's run-time-shaped kernels (mnf_linear_rows_rt, mnf_linear_rows_bwd_weight_rt): symbols, the shape
query, the workspace query, the dispatch tier and the argument checks -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_linear_rows_rt_supported", "mnf_linear_rows_rt", "mnf_linear_rows_bwd_weight_rt_workspace",
       "mnf_linear_rows_bwd_weight_rt", "mnf_affine_const_bwd_det_workspace", "mnf_affine_const_bwd_det")


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
    assert torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 19
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mnf_linear_rows_rt", "mnf_linear_rows_bwd_weight_rt"):
        assert name in table


def test_supported_query_is_the_range_two_to_1024(lib):
    for dim in (2, 6, 48, 100, 1024):
        assert lib.mnf_linear_rows_rt_supported(dim) == 1, dim
    for dim in (0, 1, 1025, -4):
        assert lib.mnf_linear_rows_rt_supported(dim) == 0, dim


def test_workspace_query_is_zero_where_there_is_nothing_to_launch(lib):
    q = lib.mnf_linear_rows_bwd_weight_rt_workspace
    assert q(0, 48) == 0
    assert q(4096, 1025) == 0 and q(4096, 1) == 0
    n = q(4096, 48)  # 0 without a gfx950 device; with one, whole slices of 16 * ceil(dim / 16) * dim floats, <= 32 MB
    assert n >= 0 and n % (48 * 48) == 0 and n * 4 <= 32 << 20
    n = q(1 << 20, 1024)
    assert n >= 0 and n % (1024 * 1024) == 0 and n * 4 <= 32 << 20


def test_tier_of_a_glow_call(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    assert tier("glow", "fwd", 262144, 64, ()) == "per-shape"
    assert tier("glow", "fwd", 5, 16, ()) == "per-shape" and tier("glow", "fwd", 5, 128, ()) == "per-shape"
    assert tier("glow", "fwd", 262144, 100, ()) == "rt" and tier("glow", "bwd", 262144, 100, ()) == "rt"
    assert tier("glow", "fwd", _dispatch.GLOW_RT_MIN_ROWS, 100, ()) == "rt"
    assert tier("glow", "fwd", _dispatch.GLOW_RT_MIN_ROWS - 1, 100, ()) == "valu"
    assert tier("glow", "bwd", _dispatch.GLOW_RT_MIN_ROWS - 1, 100, ()) == "valu"
    assert tier("glow", "fwd", 262144, 1025, ()) == "valu" and tier("glow", "bwd", 262144, 1025, ()) == "valu"
    # the weight gradient: only dim = 32 has a per-shape kernel; 64 and 128 go to the run-time-shaped one
    assert tier("glow", "bwd", 262144, 32, ()) == "per-shape"
    assert tier("glow", "bwd", 262144, 64, ()) == "rt" and tier("glow", "bwd", 262144, 128, ()) == "rt"
    assert tier("glow", "bwd", 100, 64, ()) == "valu"
    # force_generic on the layer: 1 = VALU, 2 = run-time-shaped wherever the library has the dim
    assert _dispatch.glow_route(5, 64, 2) == "rt" and _dispatch.glow_route(1 << 20, 100, 1) == "valu"
    assert _dispatch.glow_route(5, 1025, 2) == "valu" and _dispatch.glow_route(5, 32, 2, weight=True) == "rt"
    monkeypatch.setattr(_dispatch, "GLOW_RT_MIN_ROWS", 0)
    assert tier("glow", "fwd", 1, 48, ()) == "rt"
    # the other kinds answer as before
    assert tier("ahf", "fwd", 4096, 64, (24, 24, 24)) == "per-shape"


def test_kernel_family_names_are_in_the_rt_tier():
    from torch_mnf_amd import _dispatch

    assert _dispatch.tier_of_kernel("linear_rows_rt") == "rt"
    assert _dispatch.tier_of_kernel("linear_rows_bwd_weight_rt") == "rt"
    assert _dispatch.tier_of_kernel("linear_rows_generic") == "valu"


def test_argument_checking_without_a_gpu(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    bad, unsupported = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED
    fwd = lib.mnf_linear_rows_rt
    assert fwd(None, p, p + 4096, 4, 6, 0, None) == bad
    assert fwd(p, None, p + 4096, 4, 6, 0, None) == bad
    assert fwd(p, p + 4096, None, 4, 6, 0, None) == bad
    assert fwd(p, p + 4096, p, 4, 6, 0, None) == bad              # x and y alias
    assert fwd(p, p + 4096, p + 8192, -1, 6, 0, None) == bad
    assert fwd(p, p + 4096, p + 8192, 4, 1025, 0, None) == unsupported
    assert fwd(p, p + 4096, p + 8192, 4, 1, 1, None) == unsupported
    assert fwd(p, p + 4096, p + 8192, 0, 6, 1, None) == 0          # empty batch: no launch, no device needed
    bwd = lib.mnf_linear_rows_bwd_weight_rt
    assert bwd(None, p, p + 4096, 4, 6, p + 8192, 1024, None) == bad
    assert bwd(p, None, p + 4096, 4, 6, p + 8192, 1024, None) == bad
    assert bwd(p, p + 4096, None, 4, 6, p + 8192, 1024, None) == bad
    assert bwd(p, p + 4096, p + 8192, 4, 6, None, 0, None) == bad  # rows without a workspace
    assert bwd(p, p + 4096, p + 8192, -1, 6, p + 12288, 1024, None) == bad
    assert bwd(p, p + 4096, p + 8192, 4, 1025, p + 12288, 1024, None) == unsupported
    assert bwd(p, p + 4096, p + 8192, 0, 6, None, 0, None) == 0


def test_actnorm_fixed_order_sums_host_side(lib):
    """The graphed [ActNormFlow, Glow, NSF_CL] step replays bit for bit under MNF_DETERMINISTIC=1 only if ActNorm's column
    sums have a fixed order too: mnf_affine_const_bwd_det, a block of sums per workgroup."""
    from torch_mnf_amd import _lib

    q = lib.mnf_affine_const_bwd_det_workspace
    assert q(0, 48) == 0 and q(4096, 257) == 0 and q(4096, 0) == 0
    assert q(5, 48) == 2 * 48                      # one workgroup of 5 x 48 threads
    assert q(1 << 20, 48) == 2048 * 2 * 48         # the grid's cap
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    call = lib.mnf_affine_const_bwd_det
    bad = _lib.MNF_ERR_INVALID_ARG
    assert call(None, p, p, p, p + 4096, p + 8192, p + 8448, 4, 48, 0, p + 12288, 96, None) == bad
    assert call(p, p, p, p, p + 4096, None, p + 8448, 4, 48, 0, p + 12288, 96, None) == bad
    assert call(p, p, p, p, p + 4096, p + 8192, p + 8448, -1, 48, 0, p + 12288, 96, None) == bad
    assert call(p, p, p, p, p + 4096, p + 8192, p + 8448, 4, 48, 0, p + 12288, 95, None) == bad   # workspace too small
    assert call(p, p, p, p, p + 4096, p + 8192, p + 8448, 4, 48, 0, None, 0, None) == bad
    assert call(p, p, p, p, p + 4096, p + 8192, p + 8448, 4, 257, 0, p + 12288, 96, None) == _lib.MNF_ERR_UNSUPPORTED
    assert call(p, p, p, p, p + 4096, p + 8192, p + 8448, 0, 48, 0, None, 0, None) == 0
