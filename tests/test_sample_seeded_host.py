"""Host side of seeded sampling (``NormalizingFlowModel.sample(n, seed=, first_row=)``): the three C entries
``mnf_affine_half_stack_sample``, ``mnf_affine_half_stack_sample_supported`` and ``mnf_normal_rows`` are declared, exported
and bound, the shape query answers on the host alone, and the Python form refuses what the stream does not define -- none
of it needs a GPU."""
import fnmatch
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_affine_half_stack_sample", "mnf_affine_half_stack_sample_supported", "mnf_normal_rows")


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
    exports = open(os.path.join(ROOT, "torch_mnf_amd", "csrc", "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:\s*([^}]*?)local:", exports, flags=re.S).group(1).split(";") if g.strip()]
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), f"{name} is not in exports.map's global list {globs}"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 30


def _supported(lib, dim, h_sizes, n_layers):
    import torch_mnf_amd

    return lib.mnf_affine_half_stack_sample_supported(dim, len(h_sizes), torch_mnf_amd._lib.int_array(h_sizes), n_layers)


def test_supported_query(lib):
    for dim, h_sizes, n_layers in ((64, (24, 24, 24), 9), (32, (16,) * 3, 1), (256, (24,) * 3, 32)):
        assert _supported(lib, dim, h_sizes, n_layers) == 1, (dim, h_sizes, n_layers)
    for dim, h_sizes, n_layers in ((2, (24,) * 3, 9), (50, (24,) * 3, 9),      # halves narrower than their tile
                                   (64, (24, 24), 3),                          # a run-time-shaped conditioner
                                   (64, (24,) * 3, 0), (64, (24,) * 3, 33),    # layer count
                                   (64, (32,) * 3, 2)):                        # the stack kernel does not take this shape
        assert _supported(lib, dim, h_sizes, n_layers) == 0, (dim, h_sizes, n_layers)
    assert _supported(lib, 64, (32,) * 3, 1) == 1 and _supported(lib, 128, (32,) * 3, 2) == 1  # (where it does)


def _cpu_model(base=None):
    import torch_mnf_amd as amd

    flows = [amd.AffineHalfFlow(64, parity=bool(i % 2)) for i in range(3)]
    return amd.NormalizingFlowModel(base if base is not None else amd.StandardNormal(64), flows)


def test_first_row_without_a_seed_is_refused(lib):
    import torch_mnf_amd as amd

    with pytest.raises(ValueError):
        _cpu_model().sample(5, first_row=3)
    with pytest.raises(ValueError):
        amd.StandardNormal(64).sample((5,), first_row=3)


def test_seed_needs_a_standard_normal_base(lib):
    class OtherBase:
        def sample(self, *shape):
            raise AssertionError("the base must not be asked")

    with pytest.raises(ValueError):
        _cpu_model(OtherBase()).sample(5, seed=1)


def test_seed_takes_one_integer_row_count(lib):
    model = _cpu_model()
    for bad in ((), (3, 4), (2.5,), ((3,),)):
        with pytest.raises(ValueError):
            model.sample(*bad, seed=1)
    with pytest.raises(ValueError):
        model.sample(5, seed=1, first_row=-1)
