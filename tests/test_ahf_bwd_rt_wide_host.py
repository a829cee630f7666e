"""Host side of the AffineHalfFlow gradient kernel's second size class (conditioners whose widest hidden layer has 65 .. 128
units: the mnf_affine_half_bwd_rt_wide* entries, kernel families ahf_bwd_rt / ahf_bwd_stack_rt): symbols, the shape queries
at every edge of the envelope, the old queries' unchanged answers, the workspace queries, the argument checks and the
dispatch tier -- none of it needs a GPU, and no call here reaches a launch."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_affine_half_bwd_rt_wide_supported", "mnf_affine_half_bwd_rt_wide", "mnf_affine_half_bwd_rt_wide_det",
       "mnf_affine_half_bwd_rt_wide_det_workspace", "mnf_affine_half_bwd_rt_wide_stack_supported",
       "mnf_affine_half_bwd_rt_wide_stack", "mnf_affine_half_bwd_rt_wide_stack_det",
       "mnf_affine_half_bwd_rt_wide_stack_det_workspace")
# (dim, hidden, scale, shift)
WIDE = [(64, (65,), 1, 1), (64, (128,), 1, 1), (64, (128,) * 4, 1, 1), (2, (128,), 1, 1), (512, (96, 24), 1, 1),
        (64, (4, 128), 1, 1), (64, (128,), 0, 1), (64, (128,), 1, 0), (64, (128, 128, 128), 1, 1), (10, (100, 72), 1, 1)]
NARROW = [(64, (64,), 1, 1), (64, (24, 24), 1, 1), (64, (64, 64, 64), 1, 1), (2, (4,), 1, 1)]
NEITHER = [(64, (129,), 1, 1), (64, (128,) * 5, 1, 1), (64, (3, 128), 1, 1), (63, (128,), 1, 1), (64, (128,), 0, 0),
           (64, (), 1, 1), (64, (256,), 1, 1), (0, (128,), 1, 1), (64, (128, 3), 1, 1)]


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


def shape_args(dim, hidden, scale, shift):
    return dim, len(hidden), arr(*hidden), scale, shift


def test_new_symbols_are_declared_exported_and_bound(lib):
    import torch_mnf_amd
    from torch_mnf_amd import _dispatch

    header = open(os.path.join(ROOT, "include", "mnf_hip.h")).read()
    declared = int(re.search(r"#define MNF_ABI_VERSION (\d+)", header).group(1))
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sig = torch_mnf_amd._lib.SIGNATURES
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in sig, f"{name} is not in _lib.SIGNATURES"
        assert sig[name] == sig[name.replace("_wide", "")], f"{name}: not the signature of its narrow sibling"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 27
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW + ("AHF_BWD_RT_WIDE_MIN_ROWS",):
        assert name in table, name
    assert "AHF_BWD_RT_WIDE_MIN_ROWS" in _dispatch.__doc__
    assert _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS is None  # opt-in


def test_the_query_at_every_edge_of_the_envelope(lib):
    wide, stack = lib.mnf_affine_half_bwd_rt_wide_supported, lib.mnf_affine_half_bwd_rt_wide_stack_supported
    for s in WIDE:
        assert wide(*shape_args(*s)) == 1, s
        assert stack(*shape_args(*s), 1) == 1 and stack(*shape_args(*s), 32) == 1, s
        assert stack(*shape_args(*s), 0) == 0 and stack(*shape_args(*s), 33) == 0, s
    for s in NARROW + NEITHER:
        assert wide(*shape_args(*s)) == 0, s
        assert stack(*shape_args(*s), 3) == 0, s
    assert wide(64, 1, None, 1, 1) == 0 and wide(64, 0, None, 1, 1) == 0 and wide(64, 1, arr(-128), 1, 1) == 0
    # the widest layer decides, wherever it stands; every layer is at least 4 units wide
    assert wide(64, 3, arr(24, 65, 24), 1, 1) == 1 and wide(64, 3, arr(24, 64, 24), 1, 1) == 0
    assert wide(64, 2, arr(128, 129), 1, 1) == 0 and wide(64, 2, arr(128, 4), 1, 1) == 1
    # dim is bounded by the weight count alone (one row block of 16 rows always fits)
    assert wide(4096, 1, arr(128), 1, 1) == 1


def test_the_old_queries_answer_what_they_answered(lib):
    narrow, stack = lib.mnf_affine_half_bwd_rt_supported, lib.mnf_affine_half_bwd_rt_stack_supported
    ws, stack_ws = lib.mnf_affine_half_bwd_rt_det_workspace, lib.mnf_affine_half_bwd_rt_stack_det_workspace
    for s in NARROW:
        assert narrow(*shape_args(*s)) == 1 and stack(*shape_args(*s), 3) == 1, s
    for s in WIDE + NEITHER:
        assert narrow(*shape_args(*s)) == 0 and stack(*shape_args(*s), 3) == 0, s
        assert ws(4096, *shape_args(*s)) == 0 and stack_ws(4096, *shape_args(*s), 3) == 0, s
    # the two envelopes are disjoint and together what the issue's plan covers: 1 .. 4 layers of widths 4 .. 128
    for dim in (2, 10, 64, 512):
        for hidden in ((4,), (64,), (65,), (128,), (129,), (3,), (24, 128), (128, 24), (64,) * 4, (128,) * 4, (8,) * 5):
            a = shape_args(dim, hidden, 1, 1)
            n, w = narrow(*a), lib.mnf_affine_half_bwd_rt_wide_supported(*a)
            assert n + w == int(len(hidden) <= 4 and min(hidden) >= 4 and max(hidden) <= 128), (dim, hidden)
            assert w == int(n + w == 1 and max(hidden) > 64), (dim, hidden)


def test_workspace_queries(lib):
    """0 for a refused shape and for an empty batch (and, without a gfx950 device, for everything: the grid is the
    device's)."""
    one, run = lib.mnf_affine_half_bwd_rt_wide_det_workspace, lib.mnf_affine_half_bwd_rt_wide_stack_det_workspace
    for s in NARROW + NEITHER:
        assert one(4096, *shape_args(*s)) == 0 and run(4096, *shape_args(*s), 3) == 0, s
    for s in WIDE:
        for rows in (0, -1):
            assert one(rows, *shape_args(*s)) == 0 and run(rows, *shape_args(*s), 3) == 0, s
        assert run(4096, *shape_args(*s), 0) == 0 and run(4096, *shape_args(*s), 33) == 0, s
        n1, n3 = one(4096, *shape_args(*s)), run(4096, *shape_args(*s), 3)
        assert n1 >= 0 and n3 >= 0 and (n1 == 0) == (n3 == 0) and n3 >= n1, (s, n1, n3)
        assert n1 % 64 == 0 and n3 % 64 == 0, s  # whole slots of 256-byte lines


def test_argument_errors_come_before_any_launch(lib):
    """Host buffers: nothing may be launched on them, and nothing is -- every call below is refused or an empty batch."""
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * (12 * 4096))()
    p = ctypes.addressof(buf)
    x, y, gy, gl, gx, gf, flat, sc, ws, outs, work, lp = (p + 4 * 4096 * i for i in range(12))
    bad, unsupported, ok = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED, _lib.MNF_OK
    hid = arr(128)
    for det in (False, True):
        entry = lib.mnf_affine_half_bwd_rt_wide_det if det else lib.mnf_affine_half_bwd_rt_wide
        extra = (ws, 4096) if det else ()

        def call(x=x, gx=gx, flat=flat, sc=sc, rows=4, dim=64, n=1, hid=hid, scale=1, shift=1, extra=extra, gf=gf):
            return entry(x, y, gy, gl, gx, gf, flat, sc, rows, dim, 0, 0, n, hid, scale, shift, *extra, None)

        assert call(x=None) == bad and call(gx=None) == bad and call(flat=None) == bad and call(sc=None) == bad
        assert call(rows=-1) == bad and call(dim=0) == bad and call(dim=63) == bad
        assert call(hid=None) == bad and call(hid=arr(0)) == bad and call(n=0) == unsupported
        if det:
            assert call(extra=(None, 4096)) == bad and call(extra=(ws, 0)) == bad  # parameter sums wanted, no workspace
        assert call(hid=arr(64)) == unsupported and call(hid=arr(129)) == unsupported  # the narrow kernel's, nobody's
        assert call(hid=arr(3, 128), n=2) == unsupported and call(scale=0, shift=0) == unsupported
        assert call(n=5, hid=arr(128, 128, 128, 128, 128)) == unsupported
        assert call(rows=0) == ok  # the empty batch: no launch, no device needed
    par = arr(0, 1, 0)
    for det in (False, True):
        entry = lib.mnf_affine_half_bwd_rt_wide_stack_det if det else lib.mnf_affine_half_bwd_rt_wide_stack
        extra = (ws, 4096) if det else ()

        def run(x=x, outs=outs, gy=gy, lp=None, gl=gl, gx=gx, work=work, gf=gf, flat=flat, sc=sc, par=par, n=3, rows=4,
                hid=hid, scale=1, shift=1):
            return entry(x, outs, gy, lp, gl, gx, work, gf, flat, sc, par, n, rows, 64, 1, 1, hid, scale, shift, *extra, None)

        assert run(x=None) == bad and run(outs=None) == bad and run(gx=None) == bad and run(flat=None) == bad
        assert run(sc=None) == bad and run(par=None) == bad and run(n=0) == bad and run(n=33) == bad and run(rows=-1) == bad
        assert run(lp=lp) == bad and run(gy=None, lp=lp) == bad  # both cotangent forms at once
        assert run(work=None) == bad and run(work=gx) == bad and run(outs=x) == bad
        assert run(scale=0, shift=0) == bad
        for name in ("x", "outs", "gy", "gl", "gx", "work", "gf", "flat"):  # a pointer that is not 4-byte aligned
            assert run(**{name: locals()[name] + 2}) == bad, name
        assert run(gy=None, gl=None, lp=lp + 2) == bad
        assert run(hid=arr(64)) == unsupported and run(hid=arr(129)) == unsupported
        assert run(rows=0) == ok


def test_tier(lib, monkeypatch):
    from torch_mnf_amd import _dispatch

    tier = _dispatch.tier
    floor = _dispatch.RT_MIN_ROWS
    wide3, narrow3 = (128,) * 3, (64, 64, 64)
    probes = [("ahf", d, r, 64, h) for d in ("fwd", "bwd") for r in (64, floor - 1, floor, 8192, 262144)
              for h in (narrow3, (24, 24), (64,)) ] + [("ahf", "fwd", r, 64, wide3) for r in (64, floor, 262144)]
    before = [tier(*p) for p in probes]
    assert _dispatch.AHF_BWD_RT_WIDE_MIN_ROWS is None
    assert tier("ahf", "bwd", 262144, 64, wide3) == "valu"  # as shipped
    assert tier("ahf", "fwd", 262144, 64, wide3) == "rt"
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 2048)
    assert tier("ahf", "bwd", 262144, 64, wide3) == "rt"
    assert tier("ahf", "bwd", 2048, 64, wide3) == "rt" and tier("ahf", "bwd", 2047, 64, wide3) == "valu"
    for dim, hidden, scale, shift in WIDE:
        assert tier("ahf", "bwd", 262144, dim, hidden, scale=bool(scale), shift=bool(shift)) == "rt", (dim, hidden)
    for dim, hidden in ((64, (129,)), (64, (128,) * 5), (64, (3, 128)), (64, (256,))):
        assert tier("ahf", "bwd", 262144, dim, hidden) == "valu", (dim, hidden)
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 8192)
    assert tier("ahf", "bwd", 8191, 64, wide3) == "valu" and tier("ahf", "bwd", 8192, 64, wide3) == "rt"
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 0)  # never below wants_rt's own number
    assert tier("ahf", "bwd", floor - 1, 64, wide3) == "valu" and tier("ahf", "bwd", floor, 64, wide3) == "rt"
    # every other answer is what it was, whatever the constant says: (64, 64, 64) and the narrow shapes in particular
    for value in (0, 2048, 1 << 20):
        monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", value)
        assert [tier(*p) for p in probes] == before
    assert _dispatch.tier_of_kernel("ahf_bwd_rt") == "rt" and _dispatch.tier_of_kernel("ahf_bwd_stack_rt") == "rt"


def test_the_layers_route(lib, monkeypatch):
    """flows._ahf_bwd_rt_wide: opt-in through AHF_BWD_RT_WIDE_MIN_ROWS alone -- force_generic = 2 by itself does not select
    it --, then wants_rt, then the library's plan."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch
    from torch_mnf_amd.flows import _ahf_bwd_rt_wide

    big = 1 << 20
    f = amd.AffineHalfFlow(64, parity=False, h_sizes=(128, 128, 128))
    route = lambda rows: _ahf_bwd_rt_wide(lib, f, rows)
    assert not route(5) and not route(big)
    f.force_generic = 2
    assert not route(5) and not route(big)
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 0)
    assert route(5) and route(big)  # force_generic = 2 lifts wants_rt's row floor
    f.force_generic = 1
    assert not route(big)           # ... = 1 vetoes
    f.force_generic = 0
    assert route(_dispatch.RT_MIN_ROWS) and not route(_dispatch.RT_MIN_ROWS - 1)
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 8192)
    assert route(8192) and not route(8191)
    f.force_generic = 2
    assert route(8192) and not route(8191)  # the constant is a floor of its own
    f.force_generic = 0
    f.force_fp32_mfma = True  # an fp32 request stays off the split-f16 kernels
    assert not route(big)
    monkeypatch.setattr(_dispatch, "AHF_BWD_RT_WIDE_MIN_ROWS", 0)
    for hidden in ((64, 64, 64), (24, 24), (129,), (128,) * 5, (3, 128)):  # the narrow kernel's shapes, nobody's shapes
        g = amd.AffineHalfFlow(64, parity=False, h_sizes=hidden)
        g.force_generic = 2
        assert not _ahf_bwd_rt_wide(lib, g, big), hidden
