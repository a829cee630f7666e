"""Host side of the MAF / IAF element-by-element direction on the matrix cores (mnf_maf_seq_rt, kernel family maf_seq_rt):
symbols, the shape query at the envelope's edges and at the resident / streaming border, the argument checks, the empty
batch, the dispatch tier and the layer's own route -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_maf_seq_rt_supported", "mnf_maf_seq_rt_grid", "mnf_maf_seq_rt")
WIDEST = 128  # widest hidden layer (include/mnf_hip.h)


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
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 22
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("maf_seq_rt", "MAF_SEQ_RT_MIN_ROWS"):
        assert name in table


def test_supported_query_at_the_envelope_edges(lib):
    q, one_pass = lib.mnf_maf_seq_rt_supported, lib.mnf_maf_rt_supported
    assert q(6, 1, arr(3)) == 0 and q(6, 1, arr(4)) == 1
    assert q(6, 1, arr(WIDEST)) == 1 and q(6, 1, arr(WIDEST + 1)) == 0
    assert q(6, 3, arr(24, 3, 24)) == 0 and q(6, 3, arr(24, WIDEST + 1, 24)) == 0  # every layer counts
    assert q(1, 1, arr(8)) == 1 and q(0, 1, arr(8)) == 0 and q(-2, 1, arr(8)) == 0  # dim = 1 is a shape
    assert q(6, 1, None) == 0 and q(6, 1, arr(0)) == 0 and q(6, 1, arr(-4)) == 0
    assert q(6, 0, None) == 0 and q(6, 0, arr(8)) == 0
    assert q(6, 5, arr(8, 8, 8, 8, 8)) == 1  # no layer limit but the library's own
    for dim, hidden, _ in SEQ_SHAPES:
        assert q(dim, len(hidden), arr(*hidden)) == 1, (dim, hidden)
    # resident plans only: the one-pass kernel streams these two nets (144 and 512 blocks of 2 KB), this one has no launch
    for dim, hidden in ((130, (128, 128)), (4096, (64,))):
        assert one_pass(dim, len(hidden), arr(*hidden)) == 1 and q(dim, len(hidden), arr(*hidden)) == 0
    # near the LDS limit: 72 blocks + 22 bias tiles = 148,864 bytes of net, and four waves' slabs of 16 x 36 floats behind it
    assert q(33, 2, arr(128, 128)) == 1
    # one 32-column K-step more (8 blocks) and the net alone is past 150 KB
    assert one_pass(65, 2, arr(128, 128)) == 1 and q(65, 2, arr(128, 128)) == 0


SEQ_SHAPES = [(2, (24, 24, 24), 17), (3, (5,), 130), (37, (20, 7, 33), 257), (40, (64,), 129), (64, (24, 24, 24), 145),
              (100, (16,) * 4, 33), (33, (128, 128), 145), (130, (64, 64), 33), (6, (8,), 70003)]


def test_argument_errors_come_before_any_launch(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 8192)()
    p = ctypes.addressof(buf)
    x, y, ld, flat, masks = (p + 4096 * i for i in range(5))
    bad, unsupported, hid = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, arr(8)
    fwd = lib.mnf_maf_seq_rt
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
    assert fwd(x, y, ld, 0, flat, masks, 4, 6, 0, 1, arr(WIDEST + 1), None) == unsupported
    assert fwd(x, y, ld, 0, flat, masks, 4, 130, 0, 2, arr(128, 128), None) == unsupported  # a streaming plan
    assert fwd(x, y, ld, 0, flat, masks, 0, 6, 1, 1, hid, None) == _lib.MNF_OK  # empty batch: no launch, no device needed
    assert fwd(x, y, None, 0, flat, masks, 0, 6, 1, 1, hid, None) == _lib.MNF_OK


def test_the_grid_query_is_zero_without_a_launch_or_a_device(lib):
    import torch

    grid = lib.mnf_maf_seq_rt_grid
    assert grid(0, 6, 1, arr(8)) == 0 and grid(-3, 6, 1, arr(8)) == 0
    assert grid(4096, 6, 1, arr(3)) == 0 and grid(4096, 130, 2, arr(128, 128)) == 0 and grid(4096, 6, 1, None) == 0
    g = grid(4096, 6, 2, arr(16, 16))
    if torch.cuda.is_available():
        assert 1 <= g <= 32  # 4,096 rows are 32 blocks of 8 waves x 16 rows
    else:
        assert g == 0


def test_tier_of_an_element_by_element_call(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    default = _dispatch.MAF_SEQ_RT_MIN_ROWS
    assert default is None or default >= _dispatch.RT_MIN_ROWS >= 2048
    before = [tier("maf", d, r, 6, (16, 16)) for d in ("fwd", "bwd") for r in (64, 2047, 2048, 1 << 20)]
    monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", None)  # opt-in: no row count reaches the kernel by itself
    for rows in (64, 2048, 1 << 20):
        assert tier("maf_seq", "fwd", rows, 6, (16, 16)) == "valu" and tier("maf_seq", "bwd", rows, 6, (16, 16)) == "valu"
    monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", 8192)
    assert tier("maf_seq", "fwd", 8191, 6, (16, 16)) == "valu"
    assert tier("maf_seq", "fwd", 8192, 6, (16, 16)) == "rt"
    assert tier("maf_seq", "fwd", 1 << 20, 2, (24, 24, 24)) == "rt"
    assert tier("maf_seq", "fwd", 1 << 20, 33, (128, 128)) == "rt"
    for dim, hidden in ((6, (3,)), (6, (WIDEST + 1,)), (130, (128, 128)), (4096, (64,))):  # no plan: the VALU kernel
        assert tier("maf_seq", "fwd", 1 << 20, dim, hidden) == "valu"
    for rows in (64, 8192, 1 << 20):  # the gradients of this direction have no matrix-core kernel
        assert tier("maf_seq", "bwd", rows, 6, (16, 16)) == "valu"
    monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", 16)  # never below wants_rt's own number
    assert tier("maf_seq", "fwd", _dispatch.RT_MIN_ROWS - 1, 6, (16, 16)) == "valu"
    assert tier("maf_seq", "fwd", _dispatch.RT_MIN_ROWS, 6, (16, 16)) == "rt"
    assert tier("maf_seq", "bwd", _dispatch.RT_MIN_ROWS, 6, (16, 16)) == "valu"
    # the one-pass direction answers as before, whatever this direction's constant says
    assert [tier("maf", d, r, 6, (16, 16)) for d in ("fwd", "bwd") for r in (64, 2047, 2048, 1 << 20)] == before
    assert _dispatch.tier_of_kernel("maf_seq_rt") == "rt"
    assert _dispatch.tier_of_kernel("maf_generic") == "valu" and _dispatch.tier_of_kernel("maf_bwd_generic") == "valu"


def test_the_layers_route(lib, monkeypatch):
    """flows.MAF._rt_seq: wants_rt, then force_generic = 2 or MAF_SEQ_RT_MIN_ROWS, then the library's plan; MAF._rt keeps
    answering False for a sequential call in every one of these states."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    shipped = _dispatch.MAF_SEQ_RT_MIN_ROWS
    assert shipped is None or shipped >= _dispatch.RT_MIN_ROWS
    big = 1 << 20

    def never_rt(layer):
        return not any(layer._rt(rows, True, bwd=bwd) for rows in (5, 4096, big) for bwd in (False, True))

    for cls in (amd.MAF, amd.IAF):
        layer = cls(6, parity=True, h_sizes=(16, 16))
        monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", None)
        assert not layer._rt_seq(big) and not layer._rt_seq(5) and never_rt(layer)
        layer.force_generic = 2
        assert layer._rt_seq(5) and layer._rt_seq(big) and never_rt(layer)
        layer.force_generic = 1
        assert not layer._rt_seq(big) and never_rt(layer)
        layer.force_generic = 0
        monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", 4096)
        assert layer._rt_seq(4096) and not layer._rt_seq(4095) and never_rt(layer)
        monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", 16)
        assert layer._rt_seq(_dispatch.RT_MIN_ROWS) and not layer._rt_seq(_dispatch.RT_MIN_ROWS - 1)
        layer.force_fp32_mfma = True  # an fp32 request stays off the split-f16 kernel
        assert not layer._rt_seq(big) and never_rt(layer)
        layer.force_fp32_mfma = False
        layer.force_generic = 1
        assert not layer._rt_seq(big)
    monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", 4096)
    for dim, hidden in ((6, (3,)), (130, (128, 128))):  # no plan for the shape
        layer = amd.IAF(dim, parity=False, h_sizes=hidden)
        assert not layer._rt_seq(big) and never_rt(layer)
        layer.force_generic = 2
        assert not layer._rt_seq(big) and never_rt(layer)
    wide = amd.MAF(33, parity=False, h_sizes=(128, 128))
    assert wide._rt_seq(4096) and never_rt(wide)
