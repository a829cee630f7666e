"""The two host helpers every layer in flows.py / layers.py shares -- the split operand-image pack (flows._pack_split) and
the per-device table cache (flows._device_table) -- against a recording stand-in for the library: the buffer size with its
tail words, the library call's argument order, build once / rebuild on another device / remember "no kernel".  No GPU."""
import ctypes

import torch

from test_rt_routes_host import _Recorder


def test_the_split_image_pack(monkeypatch):
    from torch_mnf_amd import _lib, flows

    stream, n_split, n_plain = 0xABCD, 5, 3
    monkeypatch.setattr(flows, "_stream", lambda: stream)
    made = []
    real_empty = torch.empty

    def empty(*a, **kw):
        made.append(real_empty(*a, **kw))
        return made[-1]
    monkeypatch.setattr(flows.torch, "empty", empty)

    idx = torch.zeros(2 * n_split + n_plain, dtype=torch.int32)
    flat = torch.zeros(22)
    words = n_split + n_plain + _lib.MNF_SPLIT_TAIL_WORDS
    assert _lib.MNF_SPLIT_TAIL_WORDS > 0

    # one image: n_split + n_plain + the tail words, mnf_pack_gather_split(flat, index, image, n_split, n_plain, stream)
    lib = _Recorder()
    image = flows._pack_split(lib, flat, (idx, n_split, n_plain))
    assert len(made) == 1 and made[0] is image
    assert image.dtype == torch.int32 and image.numel() == words and image.device == idx.device
    assert lib.calls == [("mnf_pack_gather_split",
                          (flat.data_ptr(), idx.data_ptr(), image.data_ptr(), n_split, n_plain, stream))]

    # a batch of 2 at stride 11: exactly n * words in ONE buffer, mnf_pack_gather_split_batch(..., n, stride, stream)
    lib, made[:] = _Recorder(), []
    images = flows._pack_split(lib, flat, (idx, n_split, n_plain), 2, 11)
    assert len(made) == 1 and made[0] is images
    assert images.dtype == torch.int32 and images.numel() == 2 * words
    assert lib.calls == [("mnf_pack_gather_split_batch",
                          (flat.data_ptr(), idx.data_ptr(), images.data_ptr(), n_split, n_plain, 2, 11, stream))]

    # a failing pack raises, as every checked library call does
    lib = _Recorder(mnf_pack_gather_split=_lib.MNF_ERR_INVALID_ARG)
    try:
        flows._pack_split(lib, flat, (idx, n_split, n_plain))
    except _lib.MnfHipError as err:
        assert err.code == _lib.MNF_ERR_INVALID_ARG
    else:
        raise AssertionError("a failed pack must raise")


def test_the_device_table_cache():
    from torch_mnf_amd import flows

    asked = []

    def build():
        asked.append(1)
        return (ctypes.c_int32 * 4)(3, 1, 4, 1)

    cache = {}
    first = flows._device_table(cache, "t", "cpu", build)
    assert first.dtype == torch.int32 and first.tolist() == [3, 1, 4, 1] and first.device.type == "cpu"
    assert flows._device_table(cache, "t", torch.device("cpu"), build) is first and len(asked) == 1  # built once
    meta = flows._device_table(cache, "t", "meta", build)  # another device: rebuilt there
    assert meta.device.type == "meta" and meta.numel() == 4 and len(asked) == 2
    assert flows._device_table(cache, "t", "meta", build) is meta and len(asked) == 2
    assert flows._device_table(cache, "t", "cpu", build) is not first and len(asked) == 3

    # a layout's tuple: the host tables go to the device, the word counts ride along
    both = flows._device_table(cache, "layout", "cpu", lambda: ((ctypes.c_int32 * 2)(7, 8), (ctypes.c_int32 * 1)(9), 5, 3))
    assert [t.tolist() for t in both[:2]] == [[7, 8], [9]] and both[2:] == (5, 3)
    assert flows._device_table(cache, "layout", "cpu", build) is both  # (another slot, its own entry)

    # "no such kernel" is an answer too: remembered per device, the library is not asked again
    asked_none = []
    for _ in range(3):
        assert flows._device_table(cache, "none", "cpu", lambda: asked_none.append(1)) is None
    assert len(asked_none) == 1
    assert flows._device_table(cache, "none", "meta", lambda: asked_none.append(1)) is None and len(asked_none) == 2


def test_the_layers_use_the_one_cache():
    """A layer's table methods are views of its one ``_tables`` dict, with the return values their callers rely on:
    None / False where the shape has no kernel."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    import torch_mnf_amd as amd

    if not os.path.exists(amd.library_path()):
        entry.build()
    f = amd.AffineHalfFlow(6, False, h_sizes=(16, 16))  # no per-shape kernel at this shape
    assert f._device_index("cpu") is None and f._bwd_index("cpu") is None
    assert f._device_split_index("cpu") is False and f._bwd_split_index("cpu") is False
    assert set(f._tables) == {"image", "bwd", "split", "bwd_split"}
    g = amd.AffineHalfFlow(64, False)  # the flagship shape: every table exists
    idx = g._device_index("cpu")
    assert idx is g._device_index("cpu") and idx.dtype == torch.int32
    table = g._bwd_split_index("cpu")
    assert table is g._bwd_split_index("cpu") and table[0].numel() == 2 * table[1] + table[2]
    assert amd.RNVP(6, (5,))._bwd_index("cpu") is False
    assert amd.NSF_CL(6, K=5, n_h=8)._bwd_tile_tables("cpu") is False
