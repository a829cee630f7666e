"""Host side of the gradients of NSF_AR's one-pass direction on the matrix cores (mnf_nsf_ar_bwd_rt, kernel family
nsf_ar_bwd_rt): the oracle's autograd against the reference's own gradients (fixture G18), symbols, the shape query at every
edge of the envelope, the argument checks, the empty batch, the workspace query, the dispatch tier and the layer's own
route -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import g18_cases as G18
from helpers import assert_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_nsf_ar_bwd_rt_supported", "mnf_nsf_ar_bwd_rt", "mnf_nsf_ar_bwd_rt_det", "mnf_nsf_ar_bwd_rt_det_workspace")
SHIPPED_KS, NOT_SHIPPED_K = (5, 8), 10  # csrc/mnf_nsf_ar_bwd_rt.hip MNF_NSF_AR_BWD_KS


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


# ---------------------------------------------------------------------------------------------------------------------
# the referee, pinned to the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(G18.CASES))
def test_g18_oracle_gradients_are_the_references(golden, tag):
    """The GPU tests of this kernel are refereed by torch.autograd through the oracle's NSF_AR.inverse: here that referee
    meets the reference's own autograd (fixture G18), in fp32 against its fp32 gradients and in float64 against its
    .double() run, for x and every parameter."""
    from oracle import flow_oracle as O

    fx = golden("g18_nsf_ar_grads")
    dim, K, n_h, rows = G18.CASES[tag]
    sd, x, w, v = G18.inputs(tag)
    assert 0.005 < float((x.abs() > G18.B).float().mean()) < 0.08  # some elements on the identity tails
    for dt, key, loss_key in ((torch.float32, "g32", "loss"), (torch.float64, "g64", "loss64")):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        p = {k: t.to(dt).clone().requires_grad_(True) for k, t in sd.items()}
        z, ld = O.nsf_ar(xx, p, K, G18.B, True)
        loss = (z * w.to(dt)).sum() + (ld * v.to(dt)).sum()
        loss.backward()
        assert abs(float(loss.detach()) - float(fx[f"{tag}.{loss_key}"])) <= 1e-5 * abs(float(fx[f"{tag}.{loss_key}"]))
        got = {"x": xx.grad, **{k: t.grad for k, t in p.items()}}
        ref, ref64 = G18.split(tag, fx[f"{tag}.{key}"]), G18.split(tag, fx[f"{tag}.g64"])
        for k in G18.grad_names(tag):
            assert float(np.abs(ref64[k]).max()) > 0, f"{tag}: the fixture's gradient {k} is all zero"
            err = assert_parity(got[k], ref[k], ref64[k] if dt == torch.float32 else None, f"g18 {tag} {dt} oracle grad {k}",
                                rtol=1e-5 if dt == torch.float32 else 1e-12)
            print(f"g18 {tag} grad {k}: {dt} oracle vs the reference {err:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    import torch_mnf_amd

    header = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", header).group(1))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 25
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("nsf_ar_bwd_rt", "NSF_AR_BWD_RT_MIN_ROWS"):
        assert name in table


def test_supported_query_at_the_envelope_edges(lib):
    q = lib.mnf_nsf_ar_bwd_rt_supported
    h3 = lambda n: arr(n, n, n)  # noqa: E731
    for K in SHIPPED_KS:
        assert q(6, K, 3, h3(3)) == 0 and q(6, K, 3, h3(4)) == 1  # four nets side by side: 4 .. 16 units each
        assert q(6, K, 3, h3(16)) == 1 and q(6, K, 3, h3(17)) == 0
        for pos in range(3):  # every layer position
            for width, ok in ((3, 0), (4, 1), (16, 1), (17, 0)):
                h = [8, 8, 8]
                h[pos] = width
                assert q(6, K, 3, arr(*h)) == ok, (K, h)
        assert q(6, K, 3, arr(4, 16, 9)) == 1
        assert q(6, K, 0, None) == 0 and q(6, K, 0, h3(8)) == 0
        assert q(6, K, 1, arr(8)) == 1 and q(6, K, 4, arr(8, 8, 8, 8)) == 1 and q(6, K, 5, arr(8, 8, 8, 8, 8)) == 0
        assert q(6, K, 4, arr(16, 16, 16, 16)) == 1  # the largest exchange area: fewer waves per workgroup, still a plan
        assert q(0, K, 3, h3(8)) == 0 and q(-3, K, 3, h3(8)) == 0
        assert q(1, K, 3, h3(8)) == 0  # dim = 1 has no net: the parent kernel
        assert q(2, K, 3, h3(8)) == 1
        assert q(6, K, 3, None) == 0 and q(6, K, 3, arr(8, 0, 8)) == 0 and q(6, K, 3, arr(8, -8, 8)) == 0
        # flat below 2^31 floats: dim^2 / 2 first-layer rows of 16 floats pass it near dim = 16,384
        assert q(8192, K, 1, arr(16)) == 1 and q(20000, K, 1, arr(16)) == 0 and q(1 << 30, K, 1, arr(16)) == 0
    for K in range(0, 20):  # the compile-time list and nothing else (the forward kernel takes 2 .. 16)
        assert q(6, K, 3, h3(8)) == (1 if K in SHIPPED_KS else 0), K
        assert lib.mnf_nsf_ar_rt_supported(6, K, 3, h3(8)) == (1 if 2 <= K <= 16 else 0)
    assert q(6, NOT_SHIPPED_K, 3, h3(8)) == 0


def test_argument_errors_come_before_any_launch(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * (6 * 4096))()
    p = ctypes.addressof(buf)
    x, gy, gl, gx, gf, flat = (p + 4 * 4096 * i for i in range(6))
    bad, unsupported, hid = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, arr(8, 8, 8)
    for det in (False, True):
        entry = lib.mnf_nsf_ar_bwd_rt_det if det else lib.mnf_nsf_ar_bwd_rt
        tail = (gf, 1 << 20, None) if det else (None,)  # (_det: a stand-in workspace; nothing below reaches a launch)
        call = lambda *a: entry(*a, *tail)  # noqa: E731
        assert call(None, gy, gl, gx, gf, flat, 4, 6, 5, 3.0, 3, hid) == bad
        assert call(x, gy, gl, None, gf, flat, 4, 6, 5, 3.0, 3, hid) == bad
        assert call(x, gy, gl, x, gf, flat, 4, 6, 5, 3.0, 3, hid) == bad       # x and grad_x alias
        assert call(x, gx, gl, gx, gf, flat, 4, 6, 5, 3.0, 3, hid) == bad      # grad_y and grad_x alias
        assert call(x, gy, gl, gx, flat, flat, 4, 6, 5, 3.0, 3, hid) == bad    # grad_flat and flat alias
        assert call(x, gy, gl, gx, gf, None, 4, 6, 5, 3.0, 3, hid) == bad
        assert call(x, gy, gl, gx, gf, flat, -1, 6, 5, 3.0, 3, hid) == bad
        assert call(x, gy, gl, gx, gf, flat, 4, 0, 5, 3.0, 3, hid) == bad
        assert call(x, gy, gl, gx, gf, flat, 4, 6, 0, 3.0, 3, hid) == bad
        assert call(x, gy, gl, gx, gf, flat, 4, 6, 5, 0.0, 3, hid) == bad
        assert call(x, gy, gl, gx, gf, flat, 4, 6, 5, 3.0, 3, None) == bad      # malformed hidden
        assert call(x, gy, gl, gx, gf, flat, 4, 6, 5, 3.0, 3, arr(8, 0, 8)) == bad
        assert call(x, gy, gl, gx, gf, flat, 4, 6, 5, 3.0, -1, hid) == bad
        for outside in ((6, 5, 3, arr(3, 3, 3)), (6, 5, 3, arr(17, 17, 17)), (1, 5, 3, hid), (6, NOT_SHIPPED_K, 3, hid), (6, 17, 3, hid),
                        (6, 5, 0, None), (6, 5, 5, arr(8, 8, 8, 8, 8))):
            dim, K, n, h = outside
            assert call(x, gy, gl, gx, gf, flat, 4, dim, K, 3.0, n, h) == unsupported, outside[:3]
        # the empty batch: no launch, no device needed -- with and without cotangents and parameter sums
        assert call(x, gy, gl, gx, gf, flat, 0, 6, 5, 3.0, 3, hid) == _lib.MNF_OK
        assert call(x, None, None, gx, None, flat, 0, 6, 5, 3.0, 3, hid) == _lib.MNF_OK
    det = lib.mnf_nsf_ar_bwd_rt_det
    assert det(x, gy, gl, gx, gf, flat, 4, 6, 5, 3.0, 3, hid, None, 1 << 20, None) == bad   # parameter sums without a workspace
    assert det(x, gy, gl, gx, gf, flat, 4, 6, 5, 3.0, 3, hid, gf, 0, None) == bad
    assert det(x, gy, gl, gx, gf, flat, 0, 6, 5, 3.0, 3, hid, None, 0, None) == _lib.MNF_OK


def test_the_workspace_query_is_zero_without_a_launch_or_a_device(lib):
    ws = lib.mnf_nsf_ar_bwd_rt_det_workspace
    hid = arr(8, 8, 8)
    assert ws(0, 6, 5, 3, hid) == 0 and ws(-3, 6, 5, 3, hid) == 0
    assert ws(4096, 6, 5, 3, arr(3, 3, 3)) == 0 and ws(4096, 1, 5, 3, hid) == 0 and ws(4096, 6, 5, 3, None) == 0
    assert ws(4096, 6, NOT_SHIPPED_K, 3, hid) == 0
    n = ws(4096, 6, 5, 3, hid)
    if torch.cuda.is_available():
        slot = (lib.mnf_nsf_ar_flat_floats(6, 5, 3, hid) + 63) // 64 * 64
        assert n % slot == 0 and 1 <= n // slot <= 4096 // 16  # at most one slot per 16-row tile
    else:
        assert n == 0


# ---------------------------------------------------------------------------------------------------------------------
# the Python route
# ---------------------------------------------------------------------------------------------------------------------
def test_tier_of_the_gradient_pass(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    assert _dispatch.NSF_AR_BWD_RT_MIN_ROWS is None  # shipped: opt-in
    hid = (8, 8, 8)
    for rows in (64, 2048, 1 << 20):  # no row count reaches the kernel by itself
        assert tier("nsf_ar", "bwd", rows, 6, hid, K=5) == "valu"
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 2048)  # the forward kernel's constant does not move the gradients
    assert tier("nsf_ar", "fwd", 1 << 20, 6, hid, K=5) == "rt" and tier("nsf_ar", "bwd", 1 << 20, 6, hid, K=5) == "valu"
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", None)
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 8192)
    assert tier("nsf_ar", "bwd", 8191, 6, hid, K=5) == "valu"
    assert tier("nsf_ar", "bwd", 8192, 6, hid, K=5) == "rt"
    assert tier("nsf_ar", "fwd", 8192, 6, hid, K=5) == "valu"  # ... and the other way round
    assert tier("nsf_ar", "bwd", 1 << 20, 70, (16, 16, 16), K=8) == "rt"
    for dim, K, hidden in ((6, 5, (3, 3, 3)), (6, 5, (20, 20, 20)), (1, 5, hid), (6, NOT_SHIPPED_K, hid), (6, 16, hid)):
        assert tier("nsf_ar", "bwd", 1 << 20, dim, hidden, K=K) == "valu"  # no plan: the parent kernel
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 16)  # never below wants_rt's own number
    assert tier("nsf_ar", "bwd", _dispatch.RT_MIN_ROWS - 1, 6, hid, K=5) == "valu"
    assert tier("nsf_ar", "bwd", _dispatch.RT_MIN_ROWS, 6, hid, K=5) == "rt"
    assert _dispatch.tier_of_kernel("nsf_ar_bwd_rt") == "rt" and _dispatch.tier_of_kernel("nsf_ar_bwd_generic") == "valu"


def test_the_layers_route(lib, monkeypatch):
    """flows.NSF_AR._rt_bwd: NSF_AR_BWD_RT_MIN_ROWS first (None: never), then wants_rt and the fp32 request, then the
    library's plan."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    assert _dispatch.NSF_AR_BWD_RT_MIN_ROWS is None
    big = 1 << 20
    layer = amd.NSF_AR(6, K=5, B=3, n_h=8)
    assert not layer._rt_bwd(big) and not layer._rt_bwd(5)  # shipped: opt-in ...
    layer.force_generic = 2
    assert not layer._rt_bwd(big) and not layer._rt_bwd(5)  # ... which force_generic = 2 alone does not lift
    assert layer._rt(big)                                    # (the forward kernel's own switch is not touched)
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 16)  # only the forward constant set: the gradients stay
    layer.force_generic = 0
    assert layer._rt(big) and not layer._rt_bwd(big)
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", None)
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 4096)
    assert layer._rt_bwd(4096) and not layer._rt_bwd(4095) and not layer._rt(big)
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 16)
    assert layer._rt_bwd(_dispatch.RT_MIN_ROWS) and not layer._rt_bwd(_dispatch.RT_MIN_ROWS - 1)  # below RT_MIN_ROWS: never ...
    layer.force_generic = 2
    assert layer._rt_bwd(16) and not layer._rt_bwd(15)  # ... unless force_generic = 2 lifts that floor
    layer.force_fp32_mfma = True  # an fp32 request never takes the split-f16 kernel
    assert not layer._rt_bwd(big)
    layer.force_generic = 0
    assert not layer._rt_bwd(big)
    layer.force_fp32_mfma = False
    layer.force_generic = 1
    assert not layer._rt_bwd(big)
    monkeypatch.setattr(_dispatch, "NSF_AR_BWD_RT_MIN_ROWS", 0)
    for dim, K, n_h in ((6, 5, 3), (6, 5, 20), (1, 5, 8), (6, NOT_SHIPPED_K, 8)):  # no plan for the shape
        other = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
        assert not other._rt_bwd(big)
        other.force_generic = 2
        assert not other._rt_bwd(big)
    for K in SHIPPED_KS:
        other = amd.NSF_AR(9, K=K, B=3, n_h=6)
        other.force_generic = 2
        assert other._rt_bwd(1)
