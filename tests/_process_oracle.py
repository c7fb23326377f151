"""The logits-processor rule (csrc/include/common.h, 'Logits processors') restated in numpy: float32
scalar operations for the penalties, an integer round-to-nearest-even for bf16 and a plain loop for
the no-repeat n-gram ban.  Independent of the package: the processor tests compare
``ops.reference.process_logits`` and the HIP kernel against this file.

Rows travel as bit patterns: uint16 for bf16, or float32 arrays as they are.

A helper module, not a conftest: tests import what they use.
"""
from __future__ import annotations

import numpy as np

NEG_INF_BF16 = 0xFF80
OFF = dict(rp=1.0, pp=0.0, fp=0.0, g=0)


def bf16_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(x) -> int:
    """Round-to-nearest-even on the float32 bit pattern (finite values and infinities)."""
    u = int(np.asarray(x, dtype=np.float32).view(np.uint32))
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def params(rp=1.0, pp=0.0, fp=0.0, g=0):
    """(rp, inv, pp, fp) as float32 scalars, and g."""
    return (np.float32(rp), np.float32(1.0 / rp), np.float32(pp), np.float32(fp)), int(g)


def penalty(x: np.float32, c: int, rp, inv, pp, fp) -> np.float32:
    """The fixed sequence: every step one correctly rounded float32 operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.float32(x * inv) if x > 0 else np.float32(x * rp)
        q = np.float32(fp * np.float32(c))
        q = np.float32(q + pp)
        return np.float32(a - q)


def process_row(row, hist, rp=1.0, pp=0.0, fp=0.0, g=0, V=None):
    """One row: ``row`` uint16 (bf16 bits) or float32, ``hist`` a sequence of n >= 1 token ids.  Only
    the first ``V`` entries (default: all) are in the vocabulary; the rest is returned untouched.
    Returns a new array of ``row``'s dtype."""
    row = np.asarray(row)
    out = row.copy()
    V = len(row) if V is None else V
    (rp, inv, pp, fp), g = params(rp, pp, fp, g)
    bf = row.dtype == np.uint16
    h = [int(t) for t in hist]
    n = len(h)
    real = lambda t: 0 <= t < V
    counts = {}
    for t in h:
        if real(t):
            counts[t] = counts.get(t, 0) + 1
    for t, c in counts.items():
        x = bf16_to_f32(row[t])[()] if bf else np.float32(row[t])
        if np.isneginf(x):
            continue
        y = penalty(x, c, rp, inv, pp, fp)
        out[t] = f32_to_bf16(y) if bf else y
    if g >= 1:
        for e in range(g - 2, n - 1):
            if all(real(h[e - j]) and h[e - j] == h[n - 1 - j] for j in range(g - 1)) and real(h[e + 1]):
                out[h[e + 1]] = NEG_INF_BF16 if bf else -np.inf
    return out


def process(rows, hists, rp=1.0, pp=0.0, fp=0.0, g=0, V=None):
    """``process_row`` over rows [R, ld] and one history per row."""
    rows = np.asarray(rows)
    return np.stack([process_row(rows[r], hists[r], rp, pp, fp, g, V) for r in range(rows.shape[0])])


def no_repeat_holds(seq, start, g, window=None) -> bool:
    """True if no g-gram whose last token sits at a column >= ``start`` of ``seq`` occurs earlier in
    that token's history -- the ``window`` tokens before it (None: all of them), the token included
    as the g-gram's end."""
    s = [int(t) for t in seq]
    for T in range(start, len(s)):
        lo = 0 if window is None else max(0, T - window)
        h = s[lo:T + 1]
        n = len(h)
        if n < g:
            continue
        tail = h[n - g:]
        for e in range(g - 1, n - 1):  # an earlier g-gram ending at slot e of h
            if h[e - g + 1:e + 1] == tail:
                return False
    return True
