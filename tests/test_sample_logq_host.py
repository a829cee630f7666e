"""Host side of ``NormalizingFlowModel.sample(..., return_log_prob=True)``: the four C names
``mnf_affine_half_stack_sample_logq``, ``mnf_affine_half_stack_sample_logq_supported``, ``mnf_normal_rows_sq`` and
``mnf_gauss_logq_sq`` are declared, exported and bound at ABI 31; every entry refuses a bad argument before any launch (no
device is touched: the checks come first); the shape query answers on the host alone at the edges of the sample launch's
envelope; and the Python form keeps its signature default and its ``ValueError``s -- none of it needs a GPU."""
import ctypes
import fnmatch
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_affine_half_stack_sample_logq", "mnf_affine_half_stack_sample_logq_supported", "mnf_normal_rows_sq",
       "mnf_gauss_logq_sq")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    import torch_mnf_amd

    if not os.path.exists(torch_mnf_amd.library_path()):
        entry.build()
    return torch_mnf_amd._lib.load()


def test_new_symbols_are_declared_exported_and_bound_at_abi_31(lib):
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
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version()
    assert declared >= 31


# ------------------------------------------------------------------------------------------------- argument checks
# Host buffers stand in for device memory: every call below must return before a launch, so nothing reads them.
def test_stack_sample_logq_argument_checks(lib):
    import torch_mnf_amd

    L = torch_mnf_amd._lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    hid, par = L.int_array((24, 24, 24)), L.int_array((0, 1, 0))

    def call(seed=5, row0=0, y=p, log_q=p, images=p, splits=p, parity=par, n_layers=3, rows=8, dim=64, n_hidden=3, hidden=hid):
        return lib.mnf_affine_half_stack_sample_logq(ctypes.c_uint64(seed), row0, y, log_q, images, splits, parity, n_layers,
                                                     rows, dim, n_hidden, hidden, None)

    for bad in (dict(y=None), dict(log_q=None), dict(log_q=p + 2), dict(log_q=p + 1), dict(images=None), dict(splits=None),
                dict(parity=None), dict(n_layers=0), dict(n_layers=33), dict(rows=-1), dict(row0=-1), dict(dim=0),
                dict(dim=63), dict(hidden=None), dict(n_hidden=-1), dict(n_hidden=8)):
        assert call(**bad) == L.MNF_ERR_INVALID_ARG, bad
    assert call(rows=0) == L.MNF_OK
    assert call(rows=0, log_q=None) == L.MNF_ERR_INVALID_ARG  # (the checks come before the rows == 0 return)


def test_normal_rows_sq_argument_checks(lib):
    import torch_mnf_amd

    L = torch_mnf_amd._lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(row0=0, out=p, sq=p, rows=4, dim=8):
        return lib.mnf_normal_rows_sq(ctypes.c_uint64(7), row0, out, sq, rows, dim, None)

    for bad in (dict(out=None), dict(sq=None), dict(rows=-1), dict(row0=-1), dict(dim=0), dict(dim=-3)):
        assert call(**bad) == L.MNF_ERR_INVALID_ARG, bad
    assert call(rows=0) == L.MNF_OK
    assert all(v == 0.0 for v in buf), "a rows == 0 call wrote something"


def test_gauss_logq_sq_argument_checks(lib):
    import torch_mnf_amd

    L = torch_mnf_amd._lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(sq=p, ld=p, lq=p, rows=4, dim=8):
        return lib.mnf_gauss_logq_sq(sq, ld, lq, rows, dim, None)

    for bad in (dict(sq=None), dict(ld=None), dict(lq=None), dict(rows=-1), dict(dim=0)):
        assert call(**bad) == L.MNF_ERR_INVALID_ARG, bad
    assert call(rows=0) == L.MNF_OK


# ------------------------------------------------------------------------------------------------- shape query
def _supported(lib, dim, h_sizes, n_layers, name="mnf_affine_half_stack_sample_logq_supported"):
    import torch_mnf_amd

    return getattr(lib, name)(dim, len(h_sizes), torch_mnf_amd._lib.int_array(h_sizes), n_layers)


def test_logq_supported_query_at_the_edges_of_the_sample_envelope(lib):
    for dim in (32, 64, 128, 256):
        for hid in (16, 24, 32):
            for n_layers in (1, 2, 32):
                # the stack kernel's table: hidden 24 at every dim, 16 up to dim 64, 32 up to dim 128 -- and at dim <= 64
                # one layer only (the stack launcher's own rule)
                want = int(hid == 24 or (hid == 16 and dim <= 64) or (hid == 32 and (dim == 128 or (dim <= 64 and n_layers == 1))))
                assert _supported(lib, dim, (hid,) * 3, n_layers) == want, (dim, hid, n_layers)
                assert _supported(lib, dim, (hid,) * 3, n_layers, "mnf_affine_half_stack_sample_supported") == want
    assert _supported(lib, 64, (32,) * 3, 2) == 0 and _supported(lib, 32, (32,) * 3, 2) == 0
    for dim in (2, 30, 50, 100, 250):  # a half narrower than its tile: the ragged variant has no noise source
        assert _supported(lib, dim, (24,) * 3, 2) == 0, dim
    assert _supported(lib, 63, (24,) * 3, 2) == 0 and _supported(lib, 258, (24,) * 3, 2) == 0
    for n_layers in (0, 33, -1):
        assert _supported(lib, 64, (24,) * 3, n_layers) == 0, n_layers
    assert _supported(lib, 64, (24, 24), 3) == 0      # a run-time-shaped conditioner
    assert _supported(lib, 64, (64,) * 3, 1) == 0     # hidden width 64 has no stack kernel


# ------------------------------------------------------------------------------------------------- the Python form
def _cpu_model(base=None):
    import torch_mnf_amd as amd

    flows = [amd.AffineHalfFlow(64, parity=bool(i % 2)) for i in range(3)]
    return amd.NormalizingFlowModel(base if base is not None else amd.StandardNormal(64), flows)


def test_signature_has_return_log_prob_defaulting_to_false(lib):
    import torch_mnf_amd as amd

    sig = inspect.signature(amd.NormalizingFlowModel.sample)
    assert "return_log_prob" in sig.parameters
    assert sig.parameters["return_log_prob"].default is False
    assert sig.parameters["return_log_prob"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["seed"].default is None and sig.parameters["first_row"].default == 0


def test_value_errors_stay_with_the_flag(lib):
    class OtherBase:
        def sample(self, *shape):
            raise AssertionError("the base must not be asked")

    with pytest.raises(ValueError):
        _cpu_model().sample(5, first_row=3, return_log_prob=True)
    with pytest.raises(ValueError):
        _cpu_model(OtherBase()).sample(5, seed=1, return_log_prob=True)
    model = _cpu_model()
    for bad in ((), (3, 4), (2.5,), ((3,),), (True,), (-1,)):
        with pytest.raises(ValueError):
            model.sample(*bad, seed=1, return_log_prob=True)
    with pytest.raises(ValueError):
        model.sample(5, seed=1, first_row=-1, return_log_prob=True)
