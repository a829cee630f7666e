"""The Python-decided routes onto the run-time-shaped kernels, as one table (_dispatch.RT_ROUTES / rt_route): the layers'
predicates and tier() give the same answer over constants x row counts x shapes, the table's two class columns hold row by
row, and the one gradient-launch helper (flows._bwd_rt_launch) follows the X / X_det / X_det_workspace protocol against a
recording stand-in for the library -- none of it needs a GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# route -> (reached by force_generic = 2 alone with the constant None, an fp32 request vetoes under force_generic = 2)
EXPECTED = {
    "maf": (True, False), "maf_bwd": (True, False), "maf_seq": (True, False), "maf_seq_bwd": (False, False),
    "nsf_ar": (True, True), "nsf_ar_bwd": (False, True), "nsf_ar_seq": (False, True), "ahf_bwd_wide": (False, True),
}
CONSTANT = {
    "maf": "MAF_RT_MIN_ROWS", "maf_bwd": "MAF_RT_MIN_ROWS", "maf_seq": "MAF_SEQ_RT_MIN_ROWS",
    "maf_seq_bwd": "MAF_SEQ_BWD_RT_MIN_ROWS", "nsf_ar": "NSF_AR_RT_MIN_ROWS", "nsf_ar_bwd": "NSF_AR_BWD_RT_MIN_ROWS",
    "nsf_ar_seq": "NSF_AR_SEQ_RT_MIN_ROWS", "ahf_bwd_wide": "AHF_BWD_RT_WIDE_MIN_ROWS",
}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    import torch_mnf_amd

    if not os.path.exists(torch_mnf_amd.library_path()):
        entry.build()
    return torch_mnf_amd._lib.load()


def _cases(lib, route):
    """[(layer, predicate(rows), tier(rows), the library has the shape)] of one route: its shape, one the query refuses (a
    hidden width of 3), and for the MAF family the IAF way round too."""
    import torch_mnf_amd as amd
    from torch_mnf_amd import _dispatch, flows

    def tier(kind, direction, layer, K=None):
        return lambda rows: _dispatch.tier(kind, direction, rows, layer.dim, layer.h_sizes, K)

    out = []
    if route.startswith("maf"):
        for layer, has in ((amd.MAF(6, False, h_sizes=(16, 16)), True), (amd.IAF(6, False, h_sizes=(16, 16)), True),
                           (amd.MAF(6, False, h_sizes=(3, 16)), False)):
            pred = {"maf": lambda r, m=layer: m._rt(r, False), "maf_bwd": lambda r, m=layer: m._rt(r, False, bwd=True),
                    "maf_seq": layer._rt_seq, "maf_seq_bwd": layer._rt_seq_bwd}[route]
            kind, direction = ("maf_seq" if "seq" in route else "maf"), ("bwd" if route.endswith("bwd") else "fwd")
            out.append((layer, pred, tier(kind, direction, layer), has))
    elif route.startswith("nsf_ar"):
        for layer, has in ((amd.NSF_AR(6, K=5, n_h=8), True), (amd.NSF_AR(6, K=5, n_h=3), False)):
            pred = {"nsf_ar": layer._rt, "nsf_ar_bwd": layer._rt_bwd, "nsf_ar_seq": layer._rt_seq}[route]
            kind, direction = ("nsf_ar_seq", "fwd") if route == "nsf_ar_seq" else ("nsf_ar", "bwd" if route.endswith("bwd") else "fwd")
            out.append((layer, pred, tier(kind, direction, layer, 5), has))
    else:
        for layer, has in ((amd.AffineHalfFlow(64, False, h_sizes=(128,)), True),
                           (amd.AffineHalfFlow(64, False, h_sizes=(3, 128)), False)):
            out.append((layer, lambda r, f=layer: flows._ahf_bwd_rt_wide(lib, f, r), tier("ahf", "bwd", layer), has))
    return out


@pytest.mark.parametrize("route", sorted(EXPECTED))
def test_tier_and_the_layers_agree_and_the_table_holds(lib, monkeypatch, route):
    """With force_generic = 0 and no fp32 request a layer's predicate is true exactly where tier() says "rt", at every
    constant and row count, for a shape the library has and one it refuses; and the table's class columns are what the
    predicates do under force_generic = 2."""
    from torch_mnf_amd import _dispatch

    RT = _dispatch.RT_MIN_ROWS
    by_name, vetoes = EXPECTED[route]
    entry = _dispatch.RT_ROUTES[route]
    assert (entry.floor, entry.by_name, entry.fp32_vetoes_by_name) == (CONSTANT[route], by_name, vetoes)
    assert set(_dispatch.RT_ROUTES) == set(EXPECTED)
    rows_grid = (5, RT - 1, RT, 4095, 4096, 65535, 65536, 1 << 20)
    for layer, pred, tier, has in _cases(lib, route):
        for value in (None, 0, 4096, 65536):
            monkeypatch.setattr(_dispatch, entry.floor, value)
            for rows in rows_grid:
                want = has and value is not None and rows >= value and rows >= RT
                assert pred(rows) == (tier(rows) == "rt") == want, (route, layer.h_sizes, value, rows)
        # the class column: force_generic = 2 alone, the constant None -- by name at any row count, opt-in never
        monkeypatch.setattr(_dispatch, entry.floor, None)
        layer.force_generic = 2
        assert [pred(r) for r in rows_grid] == [has and by_name] * len(rows_grid), (route, layer.h_sizes)
        # the fp32 column: an fp32 request under force_generic = 2 (the constant 0, so that an opt-in route is open)
        monkeypatch.setattr(_dispatch, entry.floor, 0)
        layer.force_fp32_mfma = True
        assert [pred(r) for r in rows_grid] == [has and not vetoes] * len(rows_grid), (route, layer.h_sizes)
        layer.force_generic = 0  # without force_generic = 2 the request vetoes on every route
        assert not any(pred(r) for r in rows_grid)
        layer.force_generic, layer.force_fp32_mfma = 1, False  # and force_generic = 1 never reaches one
        assert not any(pred(r) for r in rows_grid)
        layer.force_generic = 0


class _Recorder:
    """Stands in for the library: every attribute is an entry that records its arguments and returns a preset code."""

    def __init__(self, **codes):
        self.codes, self.calls = codes, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.codes.get(name, 0)
        return entry


def test_the_gradient_launch_helper(monkeypatch):
    from torch_mnf_amd import _lib, flows

    stream, args, shape = 0xABCD, (11, None, 3.5, 7), (4096, 6, 2)
    monkeypatch.setattr(flows, "_stream", lambda: stream)
    made = []
    real_empty = torch.empty

    def empty(*a, **kw):
        made.append(real_empty(*a, **kw))
        return made[-1]
    monkeypatch.setattr(flows.torch, "empty", empty)

    # atomic sums: the entry with the stream behind its arguments, no query, no workspace
    monkeypatch.setattr(_lib, "deterministic", lambda: False)
    lib = _Recorder(mnf_x_bwd_rt=-77)
    assert flows._bwd_rt_launch(lib, "mnf_x_bwd_rt", args, shape, "cpu") == -77
    assert lib.calls == [("mnf_x_bwd_rt", args + (stream,))] and not made

    # fixed order: the workspace query on the shape, then the _det entry with exactly that many floats behind its arguments
    monkeypatch.setattr(_lib, "deterministic", lambda: True)
    lib = _Recorder(mnf_x_bwd_rt_det_workspace=640, mnf_x_bwd_rt_det=-5)
    assert flows._bwd_rt_launch(lib, "mnf_x_bwd_rt", args, shape, "cpu") == -5
    assert len(made) == 1 and made[0].dtype == torch.float32 and made[0].numel() == 640
    assert lib.calls == [("mnf_x_bwd_rt_det_workspace", shape), ("mnf_x_bwd_rt_det", args + (made[0].data_ptr(), 640, stream))]

    # no workspace for the call: UNSUPPORTED, nothing launched, nothing allocated
    for n in (0, -1):
        lib, made[:] = _Recorder(mnf_x_bwd_rt_det_workspace=n), []
        assert flows._bwd_rt_launch(lib, "mnf_x_bwd_rt", args, shape, "cpu") == _lib.MNF_ERR_UNSUPPORTED
        assert lib.calls == [("mnf_x_bwd_rt_det_workspace", shape)] and not made

    # no parameter sums wanted: no slots -- the entry receives (None, 0)
    lib = _Recorder(mnf_x_bwd_rt_det_workspace=640)
    assert flows._bwd_rt_launch(lib, "mnf_x_bwd_rt", args, shape, "cpu", sums=False) == 0
    assert lib.calls == [("mnf_x_bwd_rt_det_workspace", shape), ("mnf_x_bwd_rt_det", args + (None, 0, stream))] and not made
