"""Host side of MNFConv2d's gradient kernels (mnf_mnf_conv_bwd_weight / _input, csrc/mnf_mnf_conv_bwd.hip): symbols, the
shape queries' envelopes, the workspace plan, the argument checks and the shipped state of the dispatch switch -- none of
it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_mnf_conv_bwd_weight_supported", "mnf_mnf_conv_bwd_input_supported", "mnf_mnf_conv_bwd_weight_workspace",
       "mnf_mnf_conv_bwd_weight", "mnf_mnf_conv_bwd_input")
CAP = 32 * 2 ** 20 // 4  # the workspace cap, in floats


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
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared >= 29 and torch_mnf_amd._lib.ABI_VERSION >= 29 and lib.mnf_abi_version() >= 29


def test_supported_queries_at_the_envelopes_edges(lib):
    qw, qi = lib.mnf_mnf_conv_bwd_weight_supported, lib.mnf_mnf_conv_bwd_input_supported  # (n_in, n_out, k, height, width)
    for shape in ((1, 20, 5, 28, 28), (20, 50, 5, 12, 12), (3, 1, 1, 1, 1), (1, 64, 3, 8, 8), (4096, 8, 1, 4, 4),
                  (83, 64, 7, 7, 8), (64, 64, 8, 8, 8)):
        assert qw(*shape) == 1, shape
    for shape in ((1, 65, 3, 8, 8),                      # n_out = 65
                  (4097, 8, 1, 4, 4), (84, 8, 7, 9, 9),  # K = 4,097 / 4,116
                  (1, 20, 5, 4, 28), (1, 20, 5, 28, 4),  # k > H, k > W
                  (0, 20, 5, 28, 28), (1, 0, 5, 28, 28), (1, 20, 0, 28, 28), (1, 20, 5, -28, 28)):
        assert qw(*shape) == 0 and qi(*shape) == 0, shape
    for shape in ((20, 50, 5, 12, 12), (64, 8, 5, 5, 6), (5, 64, 8, 8, 9), (64, 64, 8, 8, 8)):
        assert qi(*shape) == 1, shape                    # n_in = 64, K' = 4,096
    for shape in ((65, 8, 3, 5, 5), (83, 64, 7, 7, 8),   # n_in = 65 / 83
                  (1, 57, 9, 9, 9), (4, 4097, 1, 4, 4), (1, 65, 3, 8, 8)):  # K' = 4,617 / n_out > 64
        assert qi(*shape) == 0, shape
    assert qi(1, 51, 9, 9, 9) == 0 and qi(1, 50, 9, 9, 9) == 1  # K' = 4,131 / 4,050
    assert qi(4, 64, 8, 9, 9) == 1 and qw(4, 64, 8, 9, 9) == 1  # K' = 4,096


def test_workspace_query(lib):
    """Positive and at most 32 MB for every supported shape, a whole number of slots (2 n_out K + n_out floats: the outputs'
    layout), at least two of them; 0 where the entry would refuse the shape."""
    ws = lib.mnf_mnf_conv_bwd_weight_workspace  # (batch, n_in, n_out, k, height, width)
    for batch, n_in, n_out, k, H, W in ((1, 3, 1, 1, 1, 1), (128, 1, 20, 5, 28, 28), (2 ** 20, 1, 20, 5, 28, 28),
                                        (8192, 20, 50, 5, 12, 12), (1, 83, 64, 7, 7, 8), (2 ** 16, 64, 64, 8, 64, 64)):
        n, slot = ws(batch, n_in, n_out, k, H, W), 2 * n_out * n_in * k * k + n_out
        assert 0 < n <= CAP and n % slot == 0 and n // slot >= 2, (batch, n_in, n_out, k, H, W, n)
    assert ws(64, 1, 20, 5, 28, 28) == ws(64, 1, 20, 5, 28, 28)  # shape alone decides
    for bad in ((1, 1, 65, 3, 8, 8), (1, 84, 8, 7, 9, 9), (1, 1, 20, 5, 4, 28), (0, 1, 20, 5, 28, 28), (-1, 1, 20, 5, 28, 28),
                (2 ** 31, 1, 20, 1, 1, 1), (2 ** 62, 1, 20, 5, 6, 6)):
        assert ws(*bad) == 0, bad


def test_argument_checking_without_a_gpu(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 16384)()
    p = ctypes.addressof(buf)
    ptrs = [p + 4096 * i for i in range(8)]
    bad, unsupported = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED
    need = lib.mnf_mnf_conv_bwd_weight_workspace(1, 1, 4, 3, 6, 6)
    assert need > 0

    def weight(**kw):
        a = dict(x=ptrs[0], grad_out=ptrs[1], grad_var=ptrs[2], grad_Wz=ptrs[3], grad_W_var=ptrs[4], grad_b_var=ptrs[5],
                 workspace=ptrs[6], workspace_floats=need, batch=1, n_in=1, height=6, width=6, n_out=4, kernel_size=3,
                 stream=None)
        a.update(kw)
        return lib.mnf_mnf_conv_bwd_weight(*a.values())

    def inp(**kw):
        a = dict(x=ptrs[0], grad_out=ptrs[1], grad_var=ptrs[2], Wz=ptrs[3], W_var=ptrs[4], grad_x=ptrs[5], batch=1, n_in=1,
                 height=6, width=6, n_out=4, kernel_size=3, stream=None)
        a.update(kw)
        return lib.mnf_mnf_conv_bwd_input(*a.values())

    for name in ("x", "grad_out", "grad_var", "grad_Wz", "grad_W_var", "grad_b_var", "workspace"):
        assert weight(**{name: None}) == bad, name
    for name in ("x", "grad_out", "grad_var", "Wz", "W_var", "grad_x"):
        assert inp(**{name: None}) == bad, name
    for name in ("batch", "n_in", "height", "width", "n_out", "kernel_size"):
        for call in (weight, inp):
            assert call(**{name: 0}) == bad and call(**{name: -3}) == bad, name
    for small in (need - 1, 0, -1):
        assert weight(workspace_floats=small) == bad, small
    for call in (weight, inp):
        assert call(n_out=65) == unsupported
        assert call(n_in=84, kernel_size=7, height=9, width=9) == unsupported
        assert call(height=2) == unsupported                      # height < k
        assert call(batch=2 ** 31, kernel_size=1) == unsupported  # the pixel index is 32-bit
        assert call(batch=2 ** 62, kernel_size=5) == unsupported  # a pixel count beyond 64 bits is refused, not wrapped
    assert inp(n_in=65) == unsupported and inp(n_out=57, kernel_size=9, height=9, width=9) == unsupported
    assert weight(n_out=65, workspace_floats=0) == unsupported    # the envelope is asked before the workspace


def test_switch_ships_off_and_has_its_row():
    from torch_mnf_amd import _dispatch

    assert _dispatch.MNF_CONV_BWD_FUSED is False
    assert _dispatch.MNF_CONV_FUSED is False
    for family in ("mnf_conv_bwd_weight", "mnf_conv_bwd_input"):
        assert family in _dispatch.__doc__, f"{family} has no row in _dispatch's table"
    assert "MNF_CONV_BWD_FUSED" in _dispatch.__doc__
