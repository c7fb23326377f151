"""The nucleus (top-p) rule of csrc/include/common.h ('Gumbel-max sampling') restated in numpy
float64 on top of ``_sample_oracle``.  Independent of the package: the top-p tests compare
``ops.reference.sample_gumbel`` and the HIP kernel against this file.

For one row: K = what top-k keeps (ties at the k-th value all kept, -inf never), w_i = exp((l_i - m)
* inv_t) on K, Z their sum, A(v) the mass of the entries of K strictly above the value v; kept is
every i in K with A(l_i) < top_p * Z, top_p taken as a float32.  The masses are summed per distinct
value, so equal logits share one answer by construction.

A helper module, not a conftest: tests import what they use.
"""
from __future__ import annotations

import numpy as np

import _sample_oracle as O


def delta(V: int, top_p: float) -> float:
    """The relative half-width of the bracket the GPU tests put around top_p: four times the bound
    common.h derives for the kernel's integer masses (|A^/Z^ - A/Z| <= 8.8e-6 A/Z + V 2^-32, a
    relative shift of top_p by at most 8.8e-6 + V 2^-32 / top_p at the boundary), never above 1e-3."""
    return min(1e-3, 4.0 * (8.8e-6 + V * 2.0 ** -32 / top_p))


def bracket(l, temperature: float, top_k, top_p, seed: int, draw: int, row0: int = 0, margin: float = 1e-3):
    """(tokens [B], ok [B]) for the kernel's draw from bf16-valued logits ``l`` [B, V]: the rule's
    token under top_p (1 - delta), and whether the draw is decided -- the same token under
    top_p (1 + delta) and both top-two score gaps at least ``margin``."""
    l = np.asarray(l, dtype=np.float64)
    d = delta(l.shape[1], top_p)
    lo, hi = keep(l, temperature, top_k, top_p * (1 - d)), keep(l, temperature, top_k, top_p * (1 + d))
    ta, ga = sample(l, temperature, top_k, None, seed, draw, row0, kept=lo)
    tb, gb = (ta, ga) if np.array_equal(lo, hi) else sample(l, temperature, top_k, None, seed, draw, row0, kept=hi)
    return ta, (ta == tb) & (ga >= margin) & (gb >= margin)


def keep(l, temperature: float, top_k, top_p) -> np.ndarray:
    """Boolean [B, V]: the kept set of every row of ``l`` [B, V]."""
    l = np.asarray(l, dtype=np.float64)
    B, V = l.shape
    inv_t = float(np.float32(1.0 / temperature))
    out = np.isfinite(l) | np.isposinf(l)
    out &= ~np.isneginf(l)
    if top_k is not None:
        kth = -np.sort(-l, axis=1)[:, min(top_k, V) - 1][:, None]
        out &= l >= kth
    if top_p is None or float(np.float32(top_p)) >= 1.0:
        return out
    p = float(np.float32(top_p))
    for b in range(B):
        idx = np.nonzero(out[b])[0]
        if idx.size == 0:
            continue
        vals, inv = np.unique(l[b, idx], return_inverse=True)  # ascending distinct values
        with np.errstate(over="ignore", under="ignore"):
            w = np.exp((l[b, idx] - l[b, idx].max()) * inv_t)
        mass = np.bincount(inv.reshape(-1), weights=w, minlength=len(vals))[::-1]  # descending values
        above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])
        kept_val = (above < p * mass.sum())[::-1]  # per ascending distinct value
        out[b, idx] = kept_val[inv.reshape(-1)]
    return out


def threshold(l, temperature: float, top_k, top_p):
    """(lowest kept value [B] float64, kept count [B] int64) per row; -inf and 0 for an empty set."""
    l = np.asarray(l, dtype=np.float64)
    k = keep(l, temperature, top_k, top_p)
    low = np.where(k, l, np.inf).min(axis=1)
    return np.where(k.any(axis=1), low, -np.inf), k.sum(axis=1)


def sample(logits, temperature: float, top_k, top_p, seed: int, draw: int, row0: int = 0, kept=None):
    """(tokens [B], gaps [B]) as ``_sample_oracle.sample`` with the nucleus applied; ``kept``: a
    precomputed ``keep(...)`` of the same arguments."""
    l = np.asarray(logits, dtype=np.float64)
    if kept is None:
        kept = keep(l, temperature, top_k, top_p)
    # the row maximum is always kept, so the masked rows keep their maximum
    return O.sample(np.where(kept, l, -np.inf), temperature, None, seed, draw, row0)
