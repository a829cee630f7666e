"""Host side of NSF_AR's one-pass direction on the matrix cores (mnf_nsf_ar_rt, kernel family nsf_ar_rt): symbols, the shape
query at every edge of the envelope, the argument checks, the empty batch, the dispatch tier, the layer's own route and
the library's export list -- none of it needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_nsf_ar_rt_supported", "mnf_nsf_ar_rt_grid", "mnf_nsf_ar_rt")
K_TOP = 16  # largest K of the envelope (include/mnf_hip.h)


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
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 24
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("nsf_ar_rt", "NSF_AR_RT_MIN_ROWS"):
        assert name in table


def test_supported_query_at_the_envelope_edges(lib):
    q = lib.mnf_nsf_ar_rt_supported
    h3 = lambda n: arr(n, n, n)  # noqa: E731
    assert q(6, 5, 3, h3(3)) == 0 and q(6, 5, 3, h3(4)) == 1        # four nets side by side: 4 .. 16 units each
    assert q(6, 5, 3, h3(16)) == 1 and q(6, 5, 3, h3(17)) == 0
    assert q(6, 5, 3, arr(8, 3, 8)) == 0 and q(6, 5, 3, arr(8, 8, 17)) == 0 and q(6, 5, 3, arr(4, 16, 9)) == 1  # every layer
    assert q(6, 1, 3, h3(8)) == 0 and q(6, 2, 3, h3(8)) == 1
    assert q(6, K_TOP, 3, h3(8)) == 1 and q(6, K_TOP + 1, 3, h3(8)) == 0
    assert q(0, 5, 3, h3(8)) == 0 and q(-3, 5, 3, h3(8)) == 0
    assert q(1, 5, 3, h3(8)) == 0  # dim = 1 has no net: the VALU kernel
    assert q(2, 5, 3, h3(8)) == 1
    assert q(6, 5, 0, None) == 0 and q(6, 5, 0, h3(8)) == 0
    assert q(6, 5, 1, arr(8)) == 1 and q(6, 5, 4, arr(8, 8, 8, 8)) == 1 and q(6, 5, 5, arr(8, 8, 8, 8, 8)) == 0
    assert q(6, 5, 3, None) == 0 and q(6, 5, 3, arr(8, 0, 8)) == 0 and q(6, 5, 3, arr(8, -8, 8)) == 0
    for dim, K, n_h, _ in SHAPES:
        assert q(dim, K, 3, h3(n_h)) == 1, (dim, K, n_h)
    # flat below 2^31 floats: dim^2 / 2 first-layer rows of 16 floats pass it near dim = 16,384
    assert q(8192, 5, 1, arr(16)) == 1 and q(20000, 5, 1, arr(16)) == 0 and q(1 << 30, 5, 1, arr(16)) == 0


SHAPES = [(2, 8, 16, 17), (3, 5, 8, 130), (6, 3, 5, 257), (13, 16, 4, 145), (37, 5, 8, 145), (70, 8, 16, 33), (33, 10, 12, 129),
          (6, 8, 8, 70003)]


def test_argument_errors_come_before_any_launch(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 8192)()
    p = ctypes.addressof(buf)
    x, y, ld, flat = (p + 4096 * i for i in range(4))
    bad, unsupported, hid = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, arr(8, 8, 8)
    fwd = lib.mnf_nsf_ar_rt
    assert fwd(None, y, ld, 0, flat, 4, 6, 5, 3.0, 3, hid, None) == bad
    assert fwd(x, None, ld, 0, flat, 4, 6, 5, 3.0, 3, hid, None) == bad
    assert fwd(x, x, ld, 0, flat, 4, 6, 5, 3.0, 3, hid, None) == bad          # x and y alias
    assert fwd(x, y, ld, 0, None, 4, 6, 5, 3.0, 3, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, -1, 6, 5, 3.0, 3, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, 4, 0, 5, 3.0, 3, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, 4, 6, 0, 3.0, 3, hid, None) == bad
    assert fwd(x, y, ld, 0, flat, 4, 6, 5, 3.0, 3, None, None) == bad         # malformed hidden
    assert fwd(x, y, ld, 0, flat, 4, 6, 5, 3.0, 3, arr(8, 0, 8), None) == bad
    assert fwd(x, y, ld, 0, flat, 4, 6, 5, 3.0, -1, hid, None) == bad
    for outside in ((6, 5, 3, arr(3, 3, 3)), (6, 5, 3, arr(17, 17, 17)), (1, 5, 3, hid), (6, 1, 3, hid), (6, K_TOP + 1, 3, hid),
                    (6, 5, 0, None), (6, 5, 5, arr(8, 8, 8, 8, 8))):
        dim, K, n, h = outside
        assert fwd(x, y, ld, 0, flat, 4, dim, K, 3.0, n, h, None) == unsupported, outside[:3]
    assert fwd(x, y, ld, 0, flat, 0, 6, 5, 3.0, 3, hid, None) == _lib.MNF_OK  # empty batch: no launch, no device needed
    assert fwd(x, y, None, 1, flat, 0, 6, 5, 3.0, 3, hid, None) == _lib.MNF_OK


def test_the_grid_query_is_zero_without_a_launch_or_a_device(lib):
    import torch

    grid = lib.mnf_nsf_ar_rt_grid
    hid = arr(8, 8, 8)
    assert grid(0, 6, 5, 3, hid) == 0 and grid(-3, 6, 5, 3, hid) == 0
    assert grid(4096, 6, 5, 3, arr(3, 3, 3)) == 0 and grid(4096, 1, 5, 3, hid) == 0 and grid(4096, 6, 5, 3, None) == 0
    g = grid(4096, 6, 5, 3, hid)
    if torch.cuda.is_available():
        assert 1 <= g <= 32  # at most one workgroup per 128 rows (8 waves of one 16-row tile each would be the smallest block)
    else:
        assert g == 0


def test_tier_of_a_one_pass_call(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    assert _dispatch.NSF_AR_RT_MIN_ROWS is None  # shipped: opt-in
    hid = (8, 8, 8)
    for rows in (64, 2048, 1 << 20):  # no row count reaches the kernel by itself
        assert tier("nsf_ar", "fwd", rows, 6, hid, K=5) == "valu" and tier("nsf_ar", "bwd", rows, 6, hid, K=5) == "valu"
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 8192)
    assert tier("nsf_ar", "fwd", 8191, 6, hid, K=5) == "valu"
    assert tier("nsf_ar", "fwd", 8192, 6, hid, K=5) == "rt"
    assert tier("nsf_ar", "fwd", 1 << 20, 70, (16, 16, 16), K=K_TOP) == "rt"
    for dim, K, hidden in ((6, 5, (3, 3, 3)), (6, 5, (20, 20, 20)), (1, 5, hid), (6, K_TOP + 1, hid)):  # no plan: the VALU kernel
        assert tier("nsf_ar", "fwd", 1 << 20, dim, hidden, K=K) == "valu"
    for rows in (64, 8192, 1 << 20):  # no gradient kernel
        assert tier("nsf_ar", "bwd", rows, 6, hid, K=5) == "valu"
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 16)  # never below wants_rt's own number
    assert tier("nsf_ar", "fwd", _dispatch.RT_MIN_ROWS - 1, 6, hid, K=5) == "valu"
    assert tier("nsf_ar", "fwd", _dispatch.RT_MIN_ROWS, 6, hid, K=5) == "rt"
    assert tier("nsf_ar", "bwd", _dispatch.RT_MIN_ROWS, 6, hid, K=5) == "valu"
    assert _dispatch.tier_of_kernel("nsf_ar_rt") == "rt"
    assert _dispatch.tier_of_kernel("nsf_ar_generic") == "valu" and _dispatch.tier_of_kernel("nsf_ar_bwd_generic") == "valu"


def test_the_layers_route(lib, monkeypatch):
    """flows.NSF_AR._rt: wants_rt, then force_generic = 2 or NSF_AR_RT_MIN_ROWS, then the library's plan."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    assert _dispatch.NSF_AR_RT_MIN_ROWS is None
    big = 1 << 20
    layer = amd.NSF_AR(6, K=5, B=3, n_h=8)
    assert not layer._rt(big) and not layer._rt(5)  # shipped: opt-in
    layer.force_generic = 2
    assert layer._rt(5) and layer._rt(big)
    layer.force_fp32_mfma = True  # an fp32 request never takes the split-f16 kernel, not even asked for by name
    assert not layer._rt(5) and not layer._rt(big)
    layer.force_fp32_mfma = False
    layer.force_generic = 1
    assert not layer._rt(big)
    layer.force_generic = 0
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 4096)
    assert layer._rt(4096) and not layer._rt(4095)
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 16)
    assert layer._rt(_dispatch.RT_MIN_ROWS) and not layer._rt(_dispatch.RT_MIN_ROWS - 1)
    layer.force_fp32_mfma = True
    assert not layer._rt(big)
    layer.force_fp32_mfma = False
    layer.force_generic = 1
    assert not layer._rt(big)
    monkeypatch.setattr(_dispatch, "NSF_AR_RT_MIN_ROWS", 4096)
    for dim, K, n_h in ((6, 5, 3), (6, 5, 20), (1, 5, 8), (6, K_TOP + 1, 8)):  # no plan for the shape
        other = amd.NSF_AR(dim, K=K, B=3, n_h=n_h)
        assert not other._rt(big)
        other.force_generic = 2
        assert not other._rt(big)


def test_the_library_exports_the_c_abi_and_nothing_else(lib):
    """nm -D --defined-only: only mnf_* names (csrc/exports.map keeps the kernel templates' host stubs local), and exactly
    the functions include/mnf_hip.h declares."""
    import torch_mnf_amd

    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm to read the dynamic symbol table with"
    out = subprocess.run([nm, "-D", "--defined-only", torch_mnf_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert exported and all(name.startswith("mnf_") for name in exported), sorted(n for n in exported if not n.startswith("mnf_"))[:8]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mnf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mnf_\w+)\s*\(", header))
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
