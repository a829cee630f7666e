"""Host side of MNFConv2d.forward as one matrix-core launch (mnf_mnf_conv_fwd, mnf_conv.py:67-88): symbols, the shape
query's envelope, the argument checks and the shipped state of the dispatch switch -- none of it needs a GPU."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mnf_mnf_conv_fwd_supported", "mnf_mnf_conv_fwd")


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
    assert "mnf_conv.py:67-88" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mnf_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in torch_mnf_amd._lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert declared == torch_mnf_amd._lib.ABI_VERSION == lib.mnf_abi_version() >= 28


def test_supported_query_is_the_envelope(lib):
    q = lib.mnf_mnf_conv_fwd_supported  # (n_in, n_out, kernel_size, height, width)
    for shape in ((1, 20, 5, 28, 28), (20, 50, 5, 12, 12), (3, 1, 1, 1, 1), (64, 64, 7, 7, 7), (83, 64, 7, 9, 9),
                  (4096, 64, 1, 1, 1), (1, 64, 64, 64, 64)):
        assert q(*shape) == 1, shape
    for shape in ((1, 65, 3, 8, 8),                                 # n_out > 64
                  (84, 8, 7, 9, 9), (4097, 8, 1, 4, 4), (2, 8, 46, 50, 50),  # n_in k^2 = 4,116 / 4,097 / 4,232
                  (1, 20, 5, 4, 28), (1, 20, 5, 28, 4),             # height / width < k
                  (0, 20, 5, 28, 28), (1, 0, 5, 28, 28), (1, 20, 0, 28, 28), (1, 20, 5, 0, 28), (1, 20, 5, 28, 0),
                  (-1, 20, 5, 28, 28), (1, -20, 5, 28, 28), (1, 20, -5, 28, 28), (1, 20, 5, -28, 28), (1, 20, 5, 28, -28)):
        assert q(*shape) == 0, shape


def test_argument_checking_without_a_gpu(lib):
    from torch_mnf_amd import _lib

    buf = (ctypes.c_float * 8192)()
    p = ctypes.addressof(buf)
    x, wz, wv, bm, bv, eps, out, var = (p + 4096 * i for i in range(8))
    bad, unsupported = _lib.MNF_ERR_INVALID_ARG, _lib.MNF_ERR_UNSUPPORTED

    def call(**kw):
        a = dict(x=x, Wz=wz, W_var=wv, b_mean=bm, b_var=bv, eps=eps, out=out, var_out=var, batch=1, n_in=1, height=6,
                 width=6, n_out=4, kernel_size=3, stream=None)
        a.update(kw)
        return lib.mnf_mnf_conv_fwd(*a.values())

    assert call(x=None) == bad
    for name in ("Wz", "W_var", "b_mean", "b_var", "eps", "out"):
        assert call(**{name: None}) == bad, name
    for name in ("batch", "n_in", "height", "width", "n_out", "kernel_size"):
        assert call(**{name: 0}) == bad and call(**{name: -3}) == bad, name
    assert call(n_out=65) == unsupported
    assert call(n_in=84, kernel_size=7, height=9, width=9) == unsupported
    assert call(height=2) == unsupported                      # height < k
    assert call(batch=2 ** 31, kernel_size=1) == unsupported  # the output pixel index is 32-bit
    assert call(x=None, var_out=None) == bad                  # (var_out alone may be NULL: checked on the GPU)
    # a batch whose pixel count does not fit 64 bits is refused, not wrapped (6x6 input, k = 5: 4 pixels per image)
    for batch in (2 ** 62, 2 ** 62 + 1, 2 ** 63 - 1, 2 ** 29):
        assert call(batch=batch, kernel_size=5) == unsupported, batch


def test_cpu_or_float64_input_never_reaches_the_kernel(lib, monkeypatch):
    """With the switch on, an input that is not float32 on the layer's GPU gets the error of the shipped route: the
    predicate refuses it, the autograd node refuses it, and neither passes a pointer to mnf_mnf_conv_fwd."""
    import torch

    import torch_mnf_amd as amd
    from torch_mnf_amd import layers

    calls = []
    monkeypatch.setattr(lib, "mnf_mnf_conv_fwd", lambda *a: calls.append(a) or 0)
    monkeypatch.setattr(amd._dispatch, "MNF_CONV_FUSED", True)
    layer = amd.MNFConv2d(1, 4, 3)
    for x in (torch.zeros(2, 1, 6, 6), torch.zeros(2, 1, 6, 6, dtype=torch.float64), torch.zeros(2, 1, 6, 6, dtype=torch.float16)):
        assert layer._fused_forward_has(x) is False
        with pytest.raises(RuntimeError, match="GPU"):
            layer.forward(x)
        w = torch.zeros(4, 1, 3, 3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layers._MnfConvFwdFn.apply(x, w, w, torch.zeros(4), torch.zeros(4), None)
    assert calls == []


def test_switch_ships_off_and_has_its_row():
    from torch_mnf_amd import _dispatch

    assert _dispatch.MNF_CONV_FUSED is False
    assert re.search(r"\|\s*mnf_conv_fwd\s", _dispatch.__doc__), "mnf_conv_fwd has no row in _dispatch's table"
    assert "MNF_CONV_FUSED" in _dispatch.__doc__
