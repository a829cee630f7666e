"""Host side of seeded sampling on the run-time-shaped tier: ``mnf_affine_half_rt_stack_sample``,
``mnf_affine_half_rt_stack_sample_logq`` and ``mnf_affine_half_rt_stack_sample_supported`` are declared, exported and bound
at ABI >= 32; the shape query answers as ``mnf_affine_half_rt_stack_supported`` does (every plan of the kernel has a
sampling instantiation: nothing was narrowed); both entries refuse a bad argument before any launch (no device is touched:
the checks come first); and ``_dispatch`` has the switch and names the kernel families -- none of it needs a GPU."""
import ctypes
import fnmatch
import itertools
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_affine_half_rt_stack_sample", "mnf_affine_half_rt_stack_sample_logq", "mnf_affine_half_rt_stack_sample_supported")
FAMILIES = ("ahf_stack_rt_sample", "ahf_stack_rt_sample_lq", "ahf_rt_sample", "ahf_rt_sample_lq")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    import torch_mnf_amd

    if not os.path.exists(torch_mnf_amd.library_path()):
        entry.build()
    return torch_mnf_amd._lib.load()


def test_new_symbols_are_declared_exported_and_bound_at_abi_32(lib):
    import torch_mnf_amd

    header = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", header).group(1))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exports = open(os.path.join(ROOT, "torch_mnf_amd", "csrc", "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:\s*([^}]*?)local:", exports, flags=re.S).group(1).split(";") if g.strip()]
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), f"{name} is not in exports.map's global list {globs}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared >= 32 and torch_mnf_amd._lib.ABI_VERSION >= 32 and lib.mnf_abi_version() >= 32
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version()


def test_supported_is_the_forward_run_query(lib):
    import torch_mnf_amd

    L = torch_mnf_amd._lib
    seen = set()
    for dim, h_sizes, n_layers, scale, shift in itertools.product(
            (2, 6, 12, 64, 512, 1024), ((8,), (24, 24), (96,), (200,), (256, 256)), (1, 3, 32, 33), (0, 1), (0, 1)):
        args = (dim, len(h_sizes), L.int_array(h_sizes), scale, shift, n_layers)
        got, want = lib.mnf_affine_half_rt_stack_sample_supported(*args), lib.mnf_affine_half_rt_stack_supported(*args)
        assert got == want, (dim, h_sizes, n_layers, scale, shift, got, want)
        seen.add(got)
        if n_layers == 33 or not (scale or shift):
            assert got == 0
    assert seen == {0, 1}
    # the cases the GPU tests rely on, by value
    for dim, h_sizes, n_layers in ((6, (8,), 3), (12, (8, 8), 2), (64, (24, 24), 3), (64, (96,), 2), (16, (200,), 2),
                                   (1024, (256, 256), 1), (8, (8,), 32)):
        assert lib.mnf_affine_half_rt_stack_sample_supported(dim, len(h_sizes), L.int_array(h_sizes), 1, 1, n_layers) == 1
    # a streaming plan of the widest class goes out one layer at a time, as the forward run does
    assert lib.mnf_affine_half_rt_stack_sample_supported(1024, 2, L.int_array((256, 256)), 1, 1, 2) == 0
    assert lib.mnf_affine_half_rt_stack_sample_supported(7, 1, L.int_array((8,)), 1, 1, 2) == 0
    assert lib.mnf_affine_half_rt_stack_sample_supported(8, 1, L.int_array((3,)), 1, 1, 2) == 0


# Host buffers stand in for device memory: every call below must return before a launch, so nothing reads them.
@pytest.mark.parametrize("with_logq", [False, True], ids=["x_only", "logq"])
def test_argument_checks(lib, with_logq):
    import torch_mnf_amd

    L = torch_mnf_amd._lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    hid, par = L.int_array((24, 24)), L.int_array((0, 1, 0))

    def call(seed=5, row0=0, y=p, log_q=p, flats=p, parity=par, n_layers=3, rows=8, dim=64, n_hidden=2, hidden=hid, scale=1,
             shift=1):
        if with_logq:
            return lib.mnf_affine_half_rt_stack_sample_logq(ctypes.c_uint64(seed), row0, y, log_q, flats, parity, n_layers, rows,
                                                            dim, n_hidden, hidden, scale, shift, None)
        return lib.mnf_affine_half_rt_stack_sample(ctypes.c_uint64(seed), row0, y, flats, parity, n_layers, rows, dim, n_hidden,
                                                   hidden, scale, shift, None)

    bad_args = [dict(y=None), dict(flats=None), dict(parity=None), dict(y=p + 2), dict(y=p + 1), dict(flats=p + 2),
                dict(n_layers=0), dict(n_layers=33), dict(rows=-1), dict(row0=-1), dict(dim=0), dict(dim=1), dict(dim=63),
                dict(dim=-2), dict(hidden=None), dict(n_hidden=-1), dict(n_hidden=8), dict(hidden=L.int_array((24, 0))),
                dict(scale=0, shift=0)]
    if with_logq:
        bad_args += [dict(log_q=None), dict(log_q=p + 2), dict(log_q=p + 1)]
    for bad in bad_args:
        assert call(**bad) == L.MNF_ERR_INVALID_ARG, bad
        assert call(**{"rows": 0, **bad}) == L.MNF_ERR_INVALID_ARG, bad  # (the checks come before the rows == 0 return)
    assert call(rows=0) == L.MNF_OK
    assert all(v == 0.0 for v in buf), "a rows == 0 call wrote something"
    # a shape the query refuses: UNSUPPORTED, still before any launch
    assert call(hidden=L.int_array((24, 3))) == L.MNF_ERR_UNSUPPORTED
    assert call(hidden=L.int_array((24, 300))) == L.MNF_ERR_UNSUPPORTED


def test_dispatch_switch_and_docstring_table(lib):
    from torch_mnf_amd import _dispatch, flows

    assert hasattr(_dispatch, "RT_SAMPLE_MIN_ROWS")
    floor = _dispatch.RT_SAMPLE_MIN_ROWS
    assert floor is None or (isinstance(floor, int) and not isinstance(floor, bool) and floor >= _dispatch.RT_MIN_ROWS)
    assert "RT_SAMPLE_MIN_ROWS" in _dispatch.__doc__
    for family in FAMILIES:
        assert family in _dispatch.__doc__, family
        assert _dispatch.tier_of_kernel(family) == "rt", family
    doc = flows.NormalizingFlowModel.sample.__doc__
    for family in ("ahf_stack_rt_sample", "ahf_rt_sample", "ahf_stack_rt_sample_lq", "ahf_rt_sample_lq"):
        assert family in doc, family


def test_route_is_off_with_the_switch_none(lib, monkeypatch):
    """``_launch_sample_rt`` answers None before it touches the library or the device when the switch is None or the call is
    below it."""
    import torch
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch

    run = amd.flows._AffineRun([amd.AffineHalfFlow(64, parity=bool(i % 2), h_sizes=(24, 24)) for i in range(3)])
    monkeypatch.setattr(_dispatch, "RT_SAMPLE_MIN_ROWS", None)
    assert run._launch_sample_rt(1, 0, 4096, torch.device("cpu"), None, False) is None
    monkeypatch.setattr(_dispatch, "RT_SAMPLE_MIN_ROWS", 8192)
    assert run.launch_sample(1, 0, 4096, torch.device("cpu"), ("rt", None)) is None
    assert run.launch_sample_logq(1, 0, 4096, torch.device("cpu"), ("rt", None)) is None
    assert run._rt_sample_ok is None  # (the shape query has not been asked)
