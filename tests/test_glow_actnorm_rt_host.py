"""Host side of the run-time-shaped [Glow.inverse, ActNormFlow.inverse] pair (mnf_glow_actnorm_inv_rt, _bwd_rt): symbols,
the shape query, the workspace query, the dispatch tier and the argument checks -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_glow_actnorm_inv_rt_supported", "mnf_glow_actnorm_inv_rt", "mnf_glow_actnorm_inv_bwd_rt_workspace",
       "mnf_glow_actnorm_inv_bwd_rt")


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
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", header).group(1))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 20
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mnf_glow_actnorm_inv_rt", "mnf_glow_actnorm_inv_bwd_rt"):
        assert name in table


def test_supported_query_is_the_range_two_to_1024(lib):
    for dim in (2, 3, 48, 192, 193, 1024):
        assert lib.mnf_glow_actnorm_inv_rt_supported(dim) == 1, dim
    for dim in (1, 0, -4, 1025):
        assert lib.mnf_glow_actnorm_inv_rt_supported(dim) == 0, dim


def test_workspace_query_is_zero_where_there_is_nothing_to_launch(lib):
    q = lib.mnf_glow_actnorm_inv_bwd_rt_workspace
    assert q(0, 48) == 0
    assert q(4096, 1025) == 0 and q(4096, 1) == 0
    n = q(4096, 48)  # 0 without a gfx950 device; with one, whole slices [grad_m | grad_s | grad_t | grad_ld_glow]
    slice_floats = (48 * 48 + 2 * 48 + 1 + 3) // 4 * 4
    assert n >= 0 and n % slice_floats == 0


def test_kernel_family_names_are_in_the_rt_tier_and_in_the_table():
    from torch_mnf_amd import _dispatch

    assert _dispatch.tier_of_kernel("glow_actnorm_inv_rt") == "rt"
    assert _dispatch.tier_of_kernel("glow_actnorm_inv_bwd_rt") == "rt"
    assert _dispatch.tier_of_kernel("glow_actnorm_inv") == "per-shape"
    for name in ("glow_actnorm_inv_rt", "glow_actnorm_inv_bwd_rt"):
        assert re.search(r"\|\s*" + name + r"\s", _dispatch.__doc__), f"{name} has no row in _dispatch's table"


def test_argument_checking_without_a_gpu(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 16384)()
    p = ctypes.addressof(buf)
    u, M, s, t, z, ldg, ldo, ldr, lp = (p + 4096 * i for i in range(9))
    s, t = s + 4, t + 4  # 4-byte aligned only
    bad, unsupported = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED
    fwd = lib.mnf_glow_actnorm_inv_rt
    assert fwd(None, M, s, t, z, ldg, ldo, None, None, 4, 6, None) == bad
    assert fwd(u, None, s, t, z, ldg, ldo, None, None, 4, 6, None) == bad
    assert fwd(u, M, None, t, z, ldg, ldo, None, None, 4, 6, None) == bad
    assert fwd(u, M, s, None, z, ldg, ldo, None, None, 4, 6, None) == bad
    assert fwd(u, M, s, t, None, ldg, ldo, None, None, 4, 6, None) == bad   # z may be NULL in the log-prob form only
    assert fwd(u, M, s, t, z, ldg, None, None, None, 4, 6, None) == bad     # ld_out is always written
    assert fwd(u, M, s, t, u, ldg, ldo, None, None, 4, 6, None) == bad      # in place
    assert fwd(u, M, s, t, z, ldg, ldo, ldr, None, 4, 6, None) == bad       # log_det_rows and log_prob: both or neither
    assert fwd(u, M, s, t, z, ldg, ldo, None, lp, 4, 6, None) == bad
    assert fwd(u, M, s, t, z, ldg, ldo, None, None, -1, 6, None) == bad
    for dim in (1, 0, 1025):
        assert fwd(u, M, s, t, z, ldg, ldo, None, None, 4, dim, None) == unsupported
        assert fwd(u, M, s, t, None, ldg, ldo, ldr, lp, 4, dim, None) == unsupported
    assert fwd(u, M, s, t, z, ldg, ldo, None, None, 0, 6, None) == 0        # empty batch: no launch, no device needed
    assert fwd(u, M, s, t, None, ldg, ldo, ldr, lp, 0, 48, None) == 0

    bwd = lib.mnf_glow_actnorm_inv_bwd_rt
    gz, glp, gu, gm, gs, gt, work = (p + 4096 * i for i in range(9, 16))

    def call(**kw):
        a = dict(u=u, z=z, grad_z=gz, grad_log_prob=None, M=M, s=s, t=t, grad_u=gu, grad_m=gm, grad_s=gs, grad_t=gt,
                 grad_ld=None, grad_ld_glow=None, rows=4, dim=6, workspace=work, workspace_floats=1024, stream=None)
        a.update(kw)
        return bwd(*a.values())

    for name in ("u", "z", "M", "s", "t", "grad_u", "grad_m"):
        assert call(**{name: None}) == bad, name
    assert call(grad_u=u) == bad                                   # in place
    assert call(grad_log_prob=glp) == bad                          # both cotangents
    assert call(grad_z=None) == bad                                # neither
    assert call(rows=-1) == bad
    assert call(workspace=None, workspace_floats=0) == bad         # rows without a workspace
    assert call(workspace_floats=0) == bad                         # a workspace that is too small
    assert call(workspace_floats=6 * 6 + 2 * 6) == bad             # (less than one slice)
    for dim in (1, 1025):
        assert call(dim=dim) == unsupported
        assert call(dim=dim, grad_z=None, grad_log_prob=glp) == unsupported
    assert call(rows=0, workspace=None, workspace_floats=0) == 0
    assert call(rows=0, grad_z=None, grad_log_prob=glp, grad_s=None, grad_t=None) == 0


def test_the_per_shape_entry_still_refuses_dim_48(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 8192)()
    p = ctypes.addressof(buf)
    assert lib.mnf_glow_actnorm_inv(p, p + 4096, p + 8192, p + 8192, p + 16384, None, None, 4, 48, None) \
        == _lib.MNF_ERR_UNSUPPORTED
