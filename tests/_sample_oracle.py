"""The sampling rule (csrc/include/common.h, 'Gumbel-max sampling') restated in numpy: uint32
arithmetic for the hash, float64 for everything else.  Independent of the package: the sampling
tests compare ``ops.reference.sample_gumbel`` and the HIP kernel against this file.

A helper module, not a conftest: tests import what they use.
"""
from __future__ import annotations

import numpy as np

SALT = 0x5A3B1E97
GOLDEN = 0x9E3779B1


def _u32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64).astype(np.uint32)  # the low 32 bits


def fmix32(h: np.ndarray) -> np.ndarray:
    h = np.array(h, dtype=np.uint32, ndmin=1)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)  # uint32 arrays wrap mod 2^32
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def gumbel(seed: int, draw: int, rows: np.ndarray, V: int) -> np.ndarray:
    """g[b, i] for batch rows ``rows`` and i < V, float64."""
    seed &= (1 << 64) - 1
    r0 = fmix32(_u32([(seed & 0xFFFFFFFF) ^ SALT]))
    r1 = fmix32(r0 + _u32([seed >> 32]))
    r2 = fmix32(r1 + _u32([draw & 0xFFFFFFFF]))
    r3 = fmix32(r2 ^ _u32(rows))                                        # [B]
    i = _u32(np.arange(V)) * np.uint32(GOLDEN)                          # [V]
    h = fmix32((r3[:, None] + i[None, :]).reshape(-1)).reshape(len(rows), V)
    u = ((h >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return -np.log(-np.log(u))


def sample(logits, temperature: float, top_k, seed: int, draw: int, row0: int = 0):
    """(tokens [B] int64, gaps [B] float64) for ``logits`` [B, V] (any float array; the values are
    taken as they are).  gap = best score - second best score (inf with one candidate)."""
    l = np.asarray(logits, dtype=np.float64)
    B, V = l.shape
    inv_t = float(np.float32(1.0 / temperature))
    g = gumbel(seed, draw, np.arange(B) + row0, V)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (l - l.max(axis=1, keepdims=True)) * inv_t + g
    if top_k is not None:
        kth = -np.sort(-l, axis=1)[:, min(top_k, V) - 1][:, None]
        s = np.where(l < kth, -np.inf, s)
    s = np.where(np.isneginf(l), -np.inf, s)
    tok = s.argmax(axis=1)  # the first index of the maximum
    if V == 1:
        return tok, np.full(B, np.inf)
    top2 = -np.partition(-s, 1, axis=1)[:, :2]
    with np.errstate(invalid="ignore"):
        gap = top2[:, 0] - top2[:, 1]
    return tok, gap
