"""Host side of the gradients of the MAF / IAF element-by-element direction on the matrix cores (mnf_maf_seq_bwd_rt, kernel
family maf_seq_bwd_rt): symbols, the shape query, the workspace queries, the argument checks, the empty batch, the refusal of
the atomic entry under MNF_DETERMINISTIC=1 (a child process), the dispatch tier and the layer's own opt-in route -- none of
it needs a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_maf_seq_bwd_rt_supported", "mnf_maf_seq_bwd_rt_workspace", "mnf_maf_seq_bwd_rt_det_workspace",
       "mnf_maf_seq_bwd_rt", "mnf_maf_seq_bwd_rt_det")
PLANNED = [(2, (24, 24, 24)), (3, (5,)), (6, (16, 16)), (37, (20, 7, 33)), (40, (64,)), (64, (24, 24, 24)), (64, (64, 64))]


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
    from torch_mnf_amd import _dispatch

    header = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", header).group(1))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 23
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("maf_seq_bwd_rt", "MAF_SEQ_BWD_RT_MIN_ROWS"):
        assert name in table, name
    for name in ("maf_seq_bwd_rt", "MAF_SEQ_BWD_RT_MIN_ROWS"):
        assert name in _dispatch.__doc__, name
    assert _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS is None  # opt-in


def test_supported_query(lib):
    q, one_pass = lib.mnf_maf_seq_bwd_rt_supported, lib.mnf_maf_bwd_rt_supported
    for dim, hidden in PLANNED:
        assert q(dim, len(hidden), arr(*hidden)) == 1, (dim, hidden)
    assert q(6, 1, arr(3)) == 0 and q(6, 1, arr(4)) == 1          # widths 4 .. 64
    assert q(6, 1, arr(64)) == 1 and q(6, 1, arr(65)) == 0
    assert q(6, 3, arr(24, 3, 24)) == 0 and q(6, 3, arr(24, 65, 24)) == 0  # every layer counts
    assert q(6, 4, arr(8, 8, 8, 8)) == 1 and q(6, 5, arr(8, 8, 8, 8, 8)) == 0  # 1 .. 4 hidden layers
    assert q(100, 4, arr(16, 16, 16, 16)) == 1 and q(200, 1, arr(8)) == 1    # dim is bounded by the LDS plan alone
    assert q(130, 2, arr(128, 128)) == 0
    assert q(4096, 1, arr(64)) == 0 and one_pass(4096, 1, arr(64)) == 1  # 8,192 fp32 rows of the last layer: no LDS plan
    assert q(6, 1, None) == 0 and q(6, 1, arr(0)) == 0 and q(6, 1, arr(-4)) == 0
    assert q(6, 0, None) == 0 and q(6, 0, arr(8)) == 0
    assert q(0, 1, arr(8)) == 0 and q(-2, 1, arr(8)) == 0 and q(1, 1, arr(8)) == 1
    # never a shape the weight pass does not have
    for dim in (1, 2, 6, 37, 64, 100, 130, 300, 1000, 4096):
        for hidden in ((3,), (4,), (8,), (64,), (65,), (128,), (16, 16), (64, 64), (128, 128), (20, 7, 33), (16,) * 4, (8,) * 5):
            if not one_pass(dim, len(hidden), arr(*hidden)):
                assert q(dim, len(hidden), arr(*hidden)) == 0, (dim, hidden)


def test_workspace_queries(lib):
    plain, det = lib.mnf_maf_seq_bwd_rt_workspace, lib.mnf_maf_seq_bwd_rt_det_workspace
    hid = arr(20, 7, 33)
    assert plain(0, 37) == 0 and plain(-5, 37) == 0 and det(0, 37, 3, hid) == 0 and det(-1, 37, 3, hid) == 0
    last = 0
    for rows in (1, 2, 16, 17, 257, 4096, 70003, 1 << 20):
        n = plain(rows, 37)
        assert n >= 2 * rows * 37 + rows + 1  # cot, the weight pass's discarded grad_x, -grad_ld, one scale
        assert n >= last
        last = n
        assert det(rows, 37, 3, hid) >= n


def test_argument_errors_come_before_any_launch(lib):
    """Host buffers: nothing may be launched on them."""
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * (8 * 4096))()
    p = ctypes.addressof(buf)
    y, gy, gl, gx, gf, flat, sc, ws = (p + 4 * 4096 * i for i in range(8))
    masks = gl + 2048
    bad, unsupported, hid = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, arr(8)
    rows, dim = 4, 6
    n_ws = lib.mnf_maf_seq_bwd_rt_workspace(rows, dim)
    assert 0 < n_ws <= 4096
    for entry in (lib.mnf_maf_seq_bwd_rt, lib.mnf_maf_seq_bwd_rt_det):
        def call(y=y, gy=gy, gl=gl, gx=gx, gf=gf, flat=flat, masks=masks, sc=sc, rows=rows, dim=dim, n=1, hid=hid, ws=ws,
                 n_ws=n_ws):
            return entry(y, gy, gl, gx, gf, flat, masks, sc, rows, dim, 1, n, hid, ws, n_ws, None)

        assert call(y=None) == bad and call(gx=None) == bad and call(flat=None) == bad and call(masks=None) == bad
        assert call(sc=None) == bad and call(ws=None) == bad
        assert call(n_ws=n_ws - 1) == bad and call(n_ws=0) == bad  # a workspace that is too small
        assert call(gx=y) == bad                                   # y == grad_x
        assert call(gy=gx) == bad                                  # grad_y == grad_x
        assert call(gf=flat) == bad                                # grad_flat == flat
        assert call(rows=-1) == bad and call(dim=0) == bad and call(n=0) == bad
        assert call(hid=None) == bad and call(hid=arr(0)) == bad and call(hid=arr(-3)) == bad
        assert call(hid=arr(3)) == unsupported and call(hid=arr(65)) == unsupported  # outside the plan
        assert call(n=5, hid=arr(8, 8, 8, 8, 8)) == unsupported
        # the empty batch: no launch, no device needed -- whatever the workspace
        assert call(rows=0) == _lib.MNF_OK and call(rows=0, gy=None, gl=None, n_ws=0) == _lib.MNF_OK


CHILD = """
import ctypes, sys
sys.path.insert(0, {root!r})
import torch_mnf_amd
from torch_mnf_amd import _lib
lib = _lib.load()
assert torch_mnf_amd.deterministic()
buf = (ctypes.c_float * (8 * 4096))()
p = ctypes.addressof(buf)
y, gy, gl, gx, gf, flat, sc, ws = (p + 4 * 4096 * i for i in range(8))
hid = _lib.int_array([8])
n = lib.mnf_maf_seq_bwd_rt_workspace(4, 6)
rc = lib.mnf_maf_seq_bwd_rt(y, gy, gl, gx, gf, flat, gl + 2048, sc, 4, 6, 1, 1, hid, ws, n, None)
assert rc == _lib.MNF_ERR_UNSUPPORTED, rc   # the atomic entry refuses, before any launch
assert lib.mnf_maf_seq_bwd_rt(y, gy, gl, gx, gf, flat, gl + 2048, sc, 0, 6, 1, 1, hid, ws, n, None) == _lib.MNF_OK
assert lib.mnf_maf_seq_bwd_rt_det(y, gy, gl, gx, gf, flat, gl + 2048, sc, 0, 6, 1, 1, hid, ws, n, None) == _lib.MNF_OK
assert lib.mnf_maf_seq_bwd_rt_det(None, gy, gl, gx, gf, flat, gl + 2048, sc, 4, 6, 1, 1, hid, ws, n, None) == _lib.MNF_ERR_INVALID_ARG
print("maf seq bwd rt refusal child ok")
"""


def test_the_atomic_entry_refuses_under_the_deterministic_switch(lib):
    """MNF_DETERMINISTIC is read once per process: a fresh child."""
    env = dict(os.environ, MNF_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    tail = "\n".join((p.stdout + p.stderr).splitlines()[-30:])
    assert p.returncode == 0, tail
    assert "maf seq bwd rt refusal child ok" in p.stdout, tail


def test_tier_of_the_gradients_of_an_element_by_element_call(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    floor = _dispatch.RT_MIN_ROWS
    probes = [(k, d, r) for k in ("maf", "maf_seq") for d in ("fwd", "bwd") for r in (64, 2047, 2048, 8192, 1 << 20)
              if (k, d) != ("maf_seq", "bwd")]
    before = [tier(k, d, r, 6, (16, 16)) for k, d, r in probes]
    assert _dispatch.MAF_SEQ_BWD_RT_MIN_ROWS is None
    for seq_fwd in (_dispatch.MAF_SEQ_RT_MIN_ROWS, 2048, 16):  # the forward constant does not move the gradients
        monkeypatch.setattr(_dispatch, "MAF_SEQ_RT_MIN_ROWS", seq_fwd)
        for rows in (1, 64, 2047, 2048, 8192, 1 << 20):
            assert tier("maf_seq", "bwd", rows, 6, (16, 16)) == "valu"
    monkeypatch.undo()
    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 8192)
    assert tier("maf_seq", "bwd", 8191, 6, (16, 16)) == "valu"
    assert tier("maf_seq", "bwd", 8192, 6, (16, 16)) == "rt"
    for dim, hidden in PLANNED:
        assert tier("maf_seq", "bwd", 1 << 20, dim, hidden) == "rt"
    for dim, hidden in ((6, (3,)), (6, (65,)), (6, (128,)), (130, (128, 128)), (4096, (64,)), (6, (8,) * 5)):  # no plan
        assert tier("maf_seq", "bwd", 1 << 20, dim, hidden) == "valu"
    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 0)  # never below wants_rt's own number
    assert tier("maf_seq", "bwd", floor - 1, 6, (16, 16)) == "valu"
    assert tier("maf_seq", "bwd", floor, 6, (16, 16)) == "rt"
    # every other answer is what it was, whatever this constant says
    assert [tier(k, d, r, 6, (16, 16)) for k, d, r in probes] == before
    assert _dispatch.tier_of_kernel("maf_seq_bwd_rt") == "rt"
    assert _dispatch.tier_of_kernel("maf_bwd_generic") == "valu" and _dispatch.tier_of_kernel("maf_seq_rt") == "rt"


def test_the_layers_route(lib, monkeypatch):
    """flows.MAF._rt_seq_bwd: opt-in through MAF_SEQ_BWD_RT_MIN_ROWS alone -- force_generic = 2 by itself does not select it --,
    then wants_rt, then the library's plan; MAF._rt keeps answering False for a sequential call."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    big = 1 << 20

    def never_rt(layer):
        return not any(layer._rt(rows, True, bwd=bwd) for rows in (5, 4096, big) for bwd in (False, True))

    for cls in (amd.MAF, amd.IAF):
        layer = cls(6, parity=True, h_sizes=(16, 16))
        monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", None)
        assert not layer._rt_seq_bwd(5) and not layer._rt_seq_bwd(big) and never_rt(layer)
        layer.force_generic = 2
        assert not layer._rt_seq_bwd(5) and not layer._rt_seq_bwd(big) and never_rt(layer)
        layer.force_generic = 1
        assert not layer._rt_seq_bwd(big)
        monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 0)
        assert not layer._rt_seq_bwd(big) and never_rt(layer)  # force_generic = 1 vetoes
        layer.force_generic = 2
        assert layer._rt_seq_bwd(5) and layer._rt_seq_bwd(big) and never_rt(layer)  # ... = 2 lifts the row floor
        layer.force_generic = 0
        assert layer._rt_seq_bwd(_dispatch.RT_MIN_ROWS) and not layer._rt_seq_bwd(_dispatch.RT_MIN_ROWS - 1)
        monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 8192)
        assert layer._rt_seq_bwd(8192) and not layer._rt_seq_bwd(8191) and never_rt(layer)
        layer.force_generic = 2
        assert layer._rt_seq_bwd(8192) and not layer._rt_seq_bwd(8191)
        layer.force_generic = 0
        layer.force_fp32_mfma = True  # an fp32 request stays off the split-f16 kernels
        assert not layer._rt_seq_bwd(big)
    monkeypatch.setattr(_dispatch, "MAF_SEQ_BWD_RT_MIN_ROWS", 0)
    for dim, hidden in ((6, (3,)), (6, (128,)), (130, (128, 128))):  # no plan for the shape
        layer = amd.IAF(dim, parity=False, h_sizes=hidden)
        layer.force_generic = 2
        assert not layer._rt_seq_bwd(big) and never_rt(layer)
