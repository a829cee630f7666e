"""Host restatement of the three counter-based random streams of ``torch_mnf_amd/csrc/mnf_device.h`` (mix32,
rnvp_mask_word / rnvp_mask_bit, ml_normal, z0_normal_pair / z0_normal), in numpy.

The integer part (hashes, mask bits, the two 24-bit uniforms' integers) is bit-exact; the two uniforms are formed in
float32 exactly as the device forms them; everything after that (log, sqrt, cos, sin) is float64.  The streams are pure
functions of (seed, row, column), so whatever is computed here at a fixed seed is the same number on every run.

A plain helper module (like rt_golden_cases.py): only tests/ imports it.
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
# mnf_device.h: mix32's two multipliers, the row and the column multiplier, the h1 -> h2 constant, z0's seed constant
MIX_C1 = 0x85EBCA6B
MIX_C2 = 0xC2B2AE35
ROW_C = 0x9E3779B1
COL_C = 0x85EBCA77
H2_XOR = 0x68BC21EB
Z0_XOR = 0x5BD1E995
# MNFLinear._slab_seed: the seed of 64-output slab k
SLAB_STEP = 0x9E3779B97F4A7C15
# the largest magnitude either normal stream can produce: u1 = 0.5 * 2**-24, r = sqrt(50 ln 2)
R_MAX = float(np.sqrt(50.0 * np.log(2.0)))

_U32 = np.uint32


def mix32(h):
    """mnf_device.h mix32 on uint32 (scalar or array); returns the same kind."""
    scalar = np.isscalar(h) or np.ndim(h) == 0
    h = np.atleast_1d(np.asarray(h, dtype=np.uint64) & np.uint64(M32)).astype(_U32)
    h = h ^ (h >> _U32(16))
    h = h * _U32(MIX_C1)  # (uint32 arrays wrap)
    h = h ^ (h >> _U32(13))
    h = h * _U32(MIX_C2)
    h = h ^ (h >> _U32(16))
    return int(h[0]) if scalar else h


def unmix32(h: int) -> int:
    """The inverse of mix32 (each of its five steps is a bijection of uint32), on a Python int."""
    h = int(h) & M32
    h ^= h >> 16
    h = (h * pow(MIX_C2, -1, 1 << 32)) & M32
    h ^= h >> 13
    h ^= h >> 26
    h = (h * pow(MIX_C1, -1, 1 << 32)) & M32
    h ^= h >> 16
    return h


def row_hash(seed: int, rows, row0: int = 0):
    """a_row = mix32(lo32(row) * ROW_C + hi32(row) + hi32(seed)) for rows row0 .. row0 + rows - 1 -> uint32 (rows,).
    ``rows`` may also be an explicit int64 array of row numbers (the hi32(row) term is host-only: no device call
    materialises 2**32 rows)."""
    seed = int(seed) & M64
    r = (np.arange(rows, dtype=np.uint64) + np.uint64(row0)) if np.isscalar(rows) else np.asarray(rows).astype(np.uint64)
    lo = (r & np.uint64(M32)).astype(_U32)
    hi = (r >> np.uint64(32)).astype(_U32)
    return mix32(lo * _U32(ROW_C) + hi + _U32(seed >> 32))


def _h1(seed: int, rows, n_idx: int, seed_xor: int = 0, row0: int = 0):
    """mix32(a_row ^ (idx * COL_C + (lo32(seed) ^ seed_xor))) -> uint32 (rows, n_idx)."""
    seed_lo = ((int(seed) & M32) ^ seed_xor) & M32
    a = row_hash(seed, rows, row0)
    c = np.arange(n_idx, dtype=_U32) * _U32(COL_C) + _U32(seed_lo)
    return mix32(a[:, None] ^ c[None, :])


def mask_words(seed: int, rows, dim: int, row0: int = 0):
    """rnvp_mask_word for words 0 .. ceil(dim / 32) - 1 -> uint32 (rows, words)."""
    return _h1(seed, rows, (dim + 31) // 32, 0, row0)


def mask(seed: int, rows, dim: int, row0: int = 0):
    """rnvp_mask_bit: exact 0 / 1 values, float32 (rows, dim)."""
    w = mask_words(seed, rows, dim, row0)
    d = np.arange(dim)
    return ((w[:, d >> 5] >> (d & 31).astype(_U32)[None, :]) & _U32(1)).astype(np.float32)


def uniform24(h):
    """The device's uniform of a hash: ((float)(h >> 8) + 0.5f) * 2**-24, every step in float32.  For h >> 8 >= 2**23
    the sum rounds to even, and at h >> 8 == 2**24 - 1 the result is exactly 1.0."""
    k = (np.asarray(h, dtype=_U32) >> _U32(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(2.0 ** -24)


def radius(h1):
    """sqrt(-2 ln u1) in float64 on the device's float32 u1 (+0 at u1 == 1)."""
    return np.sqrt(np.maximum(-2.0 * np.log(uniform24(h1).astype(np.float64)), 0.0))


def ml_normal(seed: int, rows, cols: int, row0: int = 0):
    """ml_normal(seed, row, col) -> (float64 normals (rows, cols), h1, h2)."""
    h1 = _h1(seed, rows, cols, 0, row0)
    h2 = mix32(h1 ^ _U32(H2_XOR))
    x = radius(h1) * np.cos(2.0 * np.pi * uniform24(h2).astype(np.float64))
    return x, h1, h2


def z0_normal(seed: int, rows, cols: int, row0: int = 0):
    """z0_normal(seed, row, col) -> (float64 normals (rows, cols), h1, h2); h1 / h2 are per COLUMN (each pair's hash
    repeated for its two columns), so that they index like the normals."""
    pairs = (cols + 1) // 2
    h1 = _h1(seed, rows, pairs, Z0_XOR, row0)
    h2 = mix32(h1 ^ _U32(H2_XOR))
    r = radius(h1)
    ph = 2.0 * np.pi * uniform24(h2).astype(np.float64)
    x = np.empty((h1.shape[0], 2 * pairs), dtype=np.float64)
    x[:, 0::2] = r * np.cos(ph)
    x[:, 1::2] = r * np.sin(ph)
    return x[:, :cols], np.repeat(h1, 2, axis=1)[:, :cols], np.repeat(h2, 2, axis=1)[:, :cols]


_STREAMS = {"mask": (5, 0), "ml": (0, 0), "z0": (1, Z0_XOR)}  # column -> hash index shift, xor on lo32(seed)


def seed_for(target_h1: int, seed_hi: int, row: int, col: int, stream: str) -> int:
    """The seed (hi32 = seed_hi) under which element (row, col) of ``stream`` ("ml", "z0", "mask") gets the hash
    ``target_h1`` (for "mask": the word holding the column): a_row ^ (idx * COL_C + (seed_lo ^ k)) = unmix32(target)."""
    shift, k = _STREAMS[stream]
    seed_hi = int(seed_hi) & M32
    a = int(row_hash(seed_hi << 32, np.array([row], dtype=np.int64))[0])
    idx = int(col) >> shift
    seed_lo = (((unmix32(target_h1) ^ a) - idx * COL_C) & M32) ^ k
    return (seed_hi << 32) | seed_lo


def h1_for_h2(target_h2: int) -> int:
    """The h1 whose h2 = mix32(h1 ^ H2_XOR) is ``target_h2``."""
    return unmix32(target_h2) ^ H2_XOR


def slab_seed(seed: int, k: int) -> int:
    """MNFLinear._slab_seed restated: the seed of 64-output slab k."""
    return (int(seed) + k * SLAB_STEP) & M64


def mnf_linear_noise(seed: int, rows: int, n_out: int):
    """The (rows, n_out) noise of MNFLinear.forward under ``seed``: one ml_normal stream per 64-output slab, column
    indices restarting inside each slab -> (normals, h1, h2)."""
    if n_out <= 64:
        return ml_normal(seed, rows, n_out)
    parts = [ml_normal(slab_seed(seed, k), rows, min(64, n_out - lo)) for k, lo in enumerate(range(0, n_out, 64))]
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
