#!/usr/bin/env python3
"""One line per cell for every host-only shape query of the per-shape AffineHalfFlow and NSF_CL units: the return value, the
out-parameters and, for the *_index entries, a hash of the table written.  Needs no GPU (the workspace queries then use the
fallback CU count).  Two builds of the library answer the same when their dumps are equal byte for byte:

    MNF_LIB_PATH=/path/to/libmnf_hip.so python tools/shape_query_dump.py > dump.txt

The last lines ("# name: cells, with a shape") count the cells per query and those the library has a shape for."""
from __future__ import annotations

import ctypes
import hashlib
import itertools
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_mnf_amd import _lib  # noqa: E402

DIMS = [0, 1, 3] + list(range(2, 261, 2))
WIDTHS = [1, 3, 8, 16, 17, 24, 25, 32, 33, 64, 65]
MIXED = [(8, 16, 24), (24, 16, 8), (16, 32, 24), (1, 3, 8), (17, 24, 25), (32, 33, 8), (64, 65, 1), (64, 24, 16),
         (33, 8, 8), (25, 25, 32), (8, 8, 16), (16, 16, 17), (3, 8, 1), (64, 64, 33), (24, 24, 65)]
HIDDEN = [None, ()]  # a null `hidden` (with n_hidden = 3), then n_hidden = 0 .. 4
HIDDEN += [(w,) * n for n in (1, 2, 4) for w in (8, 24, 65)]
HIDDEN += [(w,) * 3 for w in WIDTHS] + MIXED + [(16, 24), (8, 16, 24, 8)]
HAS = [(1, 1), (1, 0), (0, 1), (0, 0)]
KS = [2, 4, 5, 8, 10, 11]
LAYERS = [1, 2, 32, 33]
ROWS = [0, 1, 16, 4096]

lib = _lib.load()
cells, shaped = Counter(), Counter()
out = []


def hidden_args(hidden):
    if hidden is None:
        return 3, None
    return len(hidden), _lib.int_array(hidden)


def emit(name, key, shape, *values):
    cells[name] += 1
    shaped[name] += bool(shape)
    out.append(f"{name} {key} -> {' '.join(str(v) for v in values)}\n")


def table_hash(buf, n):
    return hashlib.sha1(memoryview(buf).cast("B")[: 4 * n]).hexdigest()[:16] if n > 0 else "-"


def index_call(name, fn, args, n_ints, key):
    """fn(*args, table): with a table of n_ints entries where the size query has a shape, else a null one and a small one"""
    if n_ints > 0:
        buf = (ctypes.c_int32 * n_ints)()
        rc = fn(*args, buf)
        emit(name, key, rc == 0, rc, table_hash(buf, n_ints))
    else:
        buf = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
        emit(name, key, False, fn(*args, buf), list(buf))
    emit(name, key + " null", False, fn(*args, None))


def i64():
    return ctypes.c_int64(-7)


for dim, hidden in itertools.product(DIMS, HIDDEN):
    nh, hp = hidden_args(hidden)
    hk = f"dim={dim} hidden={hidden}"
    for hs, ht in HAS:
        key = f"{hk} s={hs} t={ht}"
        n = lib.mnf_affine_half_image_floats(dim, nh, hp, hs, ht)
        emit("mnf_affine_half_image_floats", key, n, n)
        index_call("mnf_affine_half_image_index", lib.mnf_affine_half_image_index, (dim, nh, hp, hs, ht), n, key)
        sw, pw = i64(), i64()
        rc = lib.mnf_affine_half_split_layout(dim, nh, hp, hs, ht, ctypes.byref(sw), ctypes.byref(pw))
        emit("mnf_affine_half_split_layout", key, rc == 0, rc, sw.value, pw.value)
        emit("mnf_affine_half_split_layout", key + " null", False,
             lib.mnf_affine_half_split_layout(dim, nh, hp, hs, ht, None, ctypes.byref(pw)))
        index_call("mnf_affine_half_split_index", lib.mnf_affine_half_split_index, (dim, nh, hp, hs, ht),
                   2 * sw.value + pw.value if rc == 0 else 0, key)
        n = lib.mnf_affine_half_bwd_index_ints(dim, nh, hp, hs, ht)
        emit("mnf_affine_half_bwd_index_ints", key, n, n)
        index_call("mnf_affine_half_bwd_index", lib.mnf_affine_half_bwd_index, (dim, nh, hp, hs, ht), n, key)
        sw, pw = i64(), i64()
        rc = lib.mnf_affine_half_bwd_split_layout(dim, nh, hp, hs, ht, ctypes.byref(sw), ctypes.byref(pw))
        emit("mnf_affine_half_bwd_split_layout", key, rc == 0, rc, sw.value, pw.value)
        index_call("mnf_affine_half_bwd_split_index", lib.mnf_affine_half_bwd_split_index, (dim, nh, hp, hs, ht),
                   2 * sw.value + pw.value if rc == 0 else 0, key)
    for n_layers in LAYERS:
        v = lib.mnf_affine_half_stack_sample_supported(dim, nh, hp, n_layers)
        emit("mnf_affine_half_stack_sample_supported", f"{hk} layers={n_layers}", v, v)
    for rows in ROWS:
        v = lib.mnf_affine_half_bwd_mfma_workspace(rows, dim, nh, hp)
        emit("mnf_affine_half_bwd_mfma_workspace", f"{hk} rows={rows}", v, v)
        v = lib.mnf_affine_half_bwd_split_workspace(rows, dim, nh, hp)
        emit("mnf_affine_half_bwd_split_workspace", f"{hk} rows={rows}", v, v)
    for K in KS:
        key = f"{hk} K={K}"
        n = lib.mnf_nsf_cl_image_floats(dim, K, nh, hp)
        emit("mnf_nsf_cl_image_floats", key, n, n)
        index_call("mnf_nsf_cl_image_index", lib.mnf_nsf_cl_image_index, (dim, K, nh, hp), n, key)
        sw, pw = i64(), i64()
        rc = lib.mnf_nsf_cl_split_layout(dim, K, nh, hp, ctypes.byref(sw), ctypes.byref(pw))
        emit("mnf_nsf_cl_split_layout", key, rc == 0, rc, sw.value, pw.value)
        index_call("mnf_nsf_cl_split_index", lib.mnf_nsf_cl_split_index, (dim, K, nh, hp),
                   2 * sw.value + pw.value if rc == 0 else 0, key)
        v = lib.mnf_nsf_cl_bwd_tile_supported(dim, K, nh, hp)
        emit("mnf_nsf_cl_bwd_tile_supported", key, v, v)
        sw, pw, np_ = i64(), i64(), i64()
        rc = lib.mnf_nsf_cl_bwd_tile_layout(dim, K, nh, hp, ctypes.byref(sw), ctypes.byref(pw), ctypes.byref(np_))
        emit("mnf_nsf_cl_bwd_tile_layout", key, rc == 0, rc, sw.value, pw.value, np_.value)
        if rc == 0:  # (image entries: two per split word, then the plain words; flush entries: one per parameter)
            idx = (ctypes.c_int32 * (2 * sw.value + pw.value))()
            flush = (ctypes.c_int32 * np_.value)()
            rc = lib.mnf_nsf_cl_bwd_tile_index(dim, K, nh, hp, idx, flush)
            emit("mnf_nsf_cl_bwd_tile_index", key, rc == 0, rc, table_hash(idx, len(idx)), table_hash(flush, len(flush)))
        else:
            idx = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
            emit("mnf_nsf_cl_bwd_tile_index", key, False, lib.mnf_nsf_cl_bwd_tile_index(dim, K, nh, hp, idx, idx), list(idx))
        emit("mnf_nsf_cl_bwd_tile_index", key + " null", False, lib.mnf_nsf_cl_bwd_tile_index(dim, K, nh, hp, None, None))
        for rows in ROWS:
            v = lib.mnf_nsf_cl_bwd_tile_workspace(rows, dim, K, nh, hp)
            emit("mnf_nsf_cl_bwd_tile_workspace", f"{key} rows={rows}", v, v)
    if len(out) > 100000:
        sys.stdout.writelines(out)
        out.clear()

sys.stdout.writelines(out)
for name in sorted(cells):
    print(f"# {name}: {cells[name]} cells, {shaped[name]} with a shape")
