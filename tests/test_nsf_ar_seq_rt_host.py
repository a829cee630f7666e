"""Host side of NSF_AR's element-by-element direction on the matrix cores (mnf_nsf_ar_seq_rt, kernel family nsf_ar_seq_rt):
symbols, the shape query at every edge of the envelope, the argument checks, the empty batch, the grid query, the dispatch
tier and the layer's own route -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_nsf_ar_seq_rt_supported", "mnf_nsf_ar_seq_rt_grid", "mnf_nsf_ar_seq_rt")
SHIPPED_KS, NOT_SHIPPED_K = (5, 8), 10  # csrc/mnf_nsf_ar_seq_rt.hip ar_seq_has_k
MAX_DIM = 128                           # csrc/mnf_nsf_ar_seq_rt.hip kArSeqMaxDim


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
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", header).group(1))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 26
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("nsf_ar_seq_rt", "NSF_AR_SEQ_RT_MIN_ROWS"):
        assert name in table


def test_supported_query_at_the_envelope_edges(lib):
    q = lib.mnf_nsf_ar_seq_rt_supported
    h3 = lambda n: arr(n, n, n)  # noqa: E731
    for K in SHIPPED_KS:
        # dim: 1 has no net; the slab bounds it above
        assert q(0, K, 3, h3(8)) == 0 and q(-3, K, 3, h3(8)) == 0 and q(1, K, 3, h3(8)) == 0
        assert q(2, K, 3, h3(8)) == 1 and q(64, K, 3, h3(16)) == 1
        assert q(MAX_DIM, K, 3, h3(8)) == 1 and q(MAX_DIM + 1, K, 3, h3(8)) == 0 and q(1 << 30, K, 1, arr(16)) == 0
        assert q(MAX_DIM, K, 4, arr(16, 16, 16, 16)) == 1  # the largest net at the largest dim: fewer waves, still a plan
        largest = max(d for d in range(1, 300) if q(d, K, 3, h3(8)))
        assert largest == MAX_DIM and all(q(d, K, 3, h3(8)) for d in range(2, largest + 1))
        # widths: one unit tile, 4 .. 16 units, at every layer position
        assert q(6, K, 3, h3(3)) == 0 and q(6, K, 3, h3(4)) == 1 and q(6, K, 3, h3(16)) == 1 and q(6, K, 3, h3(17)) == 0
        for pos in range(3):
            for width, ok in ((3, 0), (4, 1), (16, 1), (17, 0)):
                h = [8, 8, 8]
                h[pos] = width
                assert q(6, K, 3, arr(*h)) == ok, (K, h)
        assert q(6, K, 3, arr(4, 16, 9)) == 1
        # hidden layers: 1 .. 4
        assert q(6, K, 0, None) == 0 and q(6, K, 0, h3(8)) == 0
        assert q(6, K, 1, arr(8)) == 1 and q(6, K, 4, arr(8, 8, 8, 8)) == 1 and q(6, K, 5, arr(8, 8, 8, 8, 8)) == 0
        assert q(6, K, 3, None) == 0 and q(6, K, 3, arr(8, 0, 8)) == 0 and q(6, K, 3, arr(8, -8, 8)) == 0
    for K in range(0, 20):  # the compile-time list and nothing else
        assert q(6, K, 3, h3(8)) == (1 if K in SHIPPED_KS else 0), K
    assert q(6, NOT_SHIPPED_K, 3, h3(8)) == 0


def test_argument_errors_come_before_any_launch(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * (4 * 4096))()
    p = ctypes.addressof(buf)
    x, y, ld, flat = (p + 4 * 4096 * i for i in range(4))
    bad, unsupported, hid = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, arr(8, 8, 8)
    call = lambda *a: lib.mnf_nsf_ar_seq_rt(*a, None)  # noqa: E731
    assert call(None, y, ld, 0, flat, 4, 6, 5, 3.0, 3, hid) == bad
    assert call(x, None, ld, 0, flat, 4, 6, 5, 3.0, 3, hid) == bad
    assert call(x, x, ld, 0, flat, 4, 6, 5, 3.0, 3, hid) == bad  # in place: the nets read the output while it is written
    assert call(x, y, ld, 0, None, 4, 6, 5, 3.0, 3, hid) == bad
    assert call(x, y, ld, 0, flat, -1, 6, 5, 3.0, 3, hid) == bad
    assert call(x, y, ld, 0, flat, 4, 0, 5, 3.0, 3, hid) == bad
    assert call(x, y, ld, 0, flat, 4, 6, 0, 3.0, 3, hid) == bad
    assert call(x, y, ld, 0, flat, 4, 6, 5, 0.0, 3, hid) == bad
    assert call(x, y, ld, 0, flat, 4, 6, 5, 3.0, 3, None) == bad
    assert call(x, y, ld, 0, flat, 4, 6, 5, 3.0, 3, arr(8, 0, 8)) == bad
    assert call(x, y, ld, 0, flat, 4, 6, 5, 3.0, -1, hid) == bad
    assert call(x, y, ld, 0, flat, 4, 6, 1001, 3.0, 3, hid) == _lib.MNF_ERR_DOMAIN
    for outside in ((6, 5, 3, arr(3, 3, 3)), (6, 5, 3, arr(17, 17, 17)), (1, 5, 3, hid), (6, NOT_SHIPPED_K, 3, hid), (6, 17, 3, hid),
                    (MAX_DIM + 1, 5, 3, hid), (6, 5, 0, None), (6, 5, 5, arr(8, 8, 8, 8, 8))):
        dim, K, n, h = outside
        assert call(x, y, ld, 0, flat, 4, dim, K, 3.0, n, h) == unsupported, outside[:3]
    assert call(x, y, ld, 0, flat, 0, 6, 5, 3.0, 3, hid) == _lib.MNF_OK  # the empty batch: no launch, no device needed
    assert call(x, y, None, 1, flat, 0, 6, 5, 3.0, 3, hid) == _lib.MNF_OK


def test_the_grid_query_is_zero_without_a_launch_or_a_device(lib):
    grid = lib.mnf_nsf_ar_seq_rt_grid
    hid = arr(8, 8, 8)
    assert grid(0, 6, 5, 3, hid) == 0 and grid(-3, 6, 5, 3, hid) == 0
    assert grid(4096, 6, 5, 3, arr(3, 3, 3)) == 0 and grid(4096, 1, 5, 3, hid) == 0 and grid(4096, 6, 5, 3, None) == 0
    assert grid(4096, 6, NOT_SHIPPED_K, 3, hid) == 0 and grid(4096, MAX_DIM + 1, 5, 3, hid) == 0
    n = grid(4096, 6, 5, 3, hid)
    if torch.cuda.is_available():
        assert 1 <= n <= 4096 // 32  # at most one workgroup per wave's worth of rows
    else:
        assert n == 0


def test_tier_of_the_element_by_element_direction(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    assert _dispatch.NSF_AR_SEQ_RT_MIN_ROWS is None  # shipped: opt-in
    hid = (8, 8, 8)
    before = {(kind, d): tier(kind, d, 1 << 20, 6, hid, K=5) for kind in ("nsf_ar", "maf", "maf_seq", "nsf", "ahf", "rnvp")
              for d in ("fwd", "bwd")}
    for rows in (64, 2048, 1 << 20):  # no row count reaches the kernel by itself
        assert tier("nsf_ar_seq", "fwd", rows, 6, hid, K=5) == "valu" and tier("nsf_ar_seq", "bwd", rows, 6, hid, K=5) == "valu"
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 2048)  # the one-pass direction's constant does not move this one
    assert tier("nsf_ar", "fwd", 1 << 20, 6, hid, K=5) == "rt" and tier("nsf_ar_seq", "fwd", 1 << 20, 6, hid, K=5) == "valu"
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", None)
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 8192)
    assert tier("nsf_ar_seq", "fwd", 8191, 6, hid, K=5) == "valu"
    assert tier("nsf_ar_seq", "fwd", 8192, 6, hid, K=5) == "rt"
    assert tier("nsf_ar_seq", "fwd", 1 << 20, 64, (16, 16, 16), K=8) == "rt"
    assert tier("nsf_ar_seq", "bwd", 1 << 20, 6, hid, K=5) == "valu"  # its gradients: always the VALU kernel
    for dim, K, hidden in ((6, 5, (3, 3, 3)), (6, 5, (20, 20, 20)), (1, 5, hid), (6, NOT_SHIPPED_K, hid), (MAX_DIM + 1, 5, hid)):
        assert tier("nsf_ar_seq", "fwd", 1 << 20, dim, hidden, K=K) == "valu"  # no plan: the parent kernel
    for key, was in before.items():  # the other kinds answer as before
        assert tier(key[0], key[1], 1 << 20, 6, hid, K=5) == was, key
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 16)  # never below wants_rt's own number
    assert tier("nsf_ar_seq", "fwd", _dispatch.RT_MIN_ROWS - 1, 6, hid, K=5) == "valu"
    assert tier("nsf_ar_seq", "fwd", _dispatch.RT_MIN_ROWS, 6, hid, K=5) == "rt"
    assert _dispatch.tier_of_kernel("nsf_ar_seq_rt") == "rt" and _dispatch.tier_of_kernel("nsf_ar_generic") == "valu"


def test_the_layers_route(lib, monkeypatch):
    """flows.NSF_AR._rt_seq: NSF_AR_SEQ_RT_MIN_ROWS first (None: never), then wants_rt and the fp32 request, then the
    library's plan."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    big = 1 << 20
    layer = amd.NSF_AR(6, K=5, B=3, n_h=8)
    assert not layer._rt_seq(big) and not layer._rt_seq(5)  # shipped: opt-in ...
    layer.force_generic = 2
    assert not layer._rt_seq(big) and not layer._rt_seq(5)  # ... which force_generic = 2 alone does not lift
    assert layer._rt(big)                                    # (the one-pass kernel's own switch is not touched)
    layer.force_generic = 0
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 4096)
    assert layer._rt_seq(4096) and not layer._rt_seq(4095) and not layer._rt(big) and not layer._rt_bwd(big)
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 16)
    assert layer._rt_seq(_dispatch.RT_MIN_ROWS) and not layer._rt_seq(_dispatch.RT_MIN_ROWS - 1)  # below RT_MIN_ROWS: never ...
    layer.force_generic = 2
    assert layer._rt_seq(16) and not layer._rt_seq(15)  # ... unless force_generic = 2 lifts that floor
    layer.force_fp32_mfma = True  # an fp32 request never takes the split-f16 kernel
    assert not layer._rt_seq(big)
    layer.force_generic = 0
    assert not layer._rt_seq(big)
    layer.force_fp32_mfma = False
    layer.force_generic = 1
    assert not layer._rt_seq(big)
    monkeypatch.setattr(_dispatch, "NSF_AR_SEQ_RT_MIN_ROWS", 0)
    for dim, K, n_h in ((6, 5, 3), (6, 5, 20), (1, 5, 8), (6, NOT_SHIPPED_K, 8), (MAX_DIM + 1, 5, 4)):  # no plan for the shape
        other = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
        assert not other._rt_seq(big)
        other.force_generic = 2
        assert not other._rt_seq(big)
    for K in SHIPPED_KS:
        other = amd.NSF_AR(9, K=K, B=3, n_h=6)
        other.force_generic = 2
        assert other._rt_seq(1)
