"""The speculative-decoding rule (csrc/include/common.h, 'Speculative greedy decoding') restated in
plain numpy / Python integers, independent of ``ops/reference.py`` and of the kernels: the tests
compare both against this.

A helper module, not a conftest: tests import what they use.
"""
from __future__ import annotations

import numpy as np


def draft(s, p: int, K: int, ngram: int):
    """(rows [K], positions [K], has_draft) for committed tokens s[0 .. p]."""
    s = np.asarray(s, dtype=np.int64)
    assert 0 <= p < len(s)
    best_ml, best_e = 0, -1
    for e in range(p - 1, -1, -1):  # most recent first: a later e only wins with a longer match
        ml = 0
        for j in range(ngram):
            if e - j < 0 or s[e - j] != s[p - j]:
                break
            ml = j + 1
        if ml > best_ml:
            best_ml, best_e = ml, e
    pos = np.arange(p, p + K, dtype=np.int64)
    if best_ml == 0:
        return np.full(K, s[p], dtype=np.int64), pos, False
    x = np.zeros(p + K, dtype=np.int64)
    x[:p + 1] = s[:p + 1]
    for r in range(1, K):
        x[p + r] = x[best_e + r]
    return x[p:].copy(), pos, True


def accept(rows, g, has_draft: bool, p: int, end: int):
    """(a, count): count tokens g[0 .. count - 1] go to columns p + 1 ..; (0, 0) when p == end."""
    if p >= end:
        return 0, 0
    a = 0
    if has_draft:
        for r in range(1, len(rows)):
            if int(rows[r]) != int(g[r - 1]):
                break
            a = r
    return a, min(a + 1, end - p)


def simulate(greedy, T: int, K: int, ngram: int):
    """The rule run over a known greedy sequence ``greedy`` (columns 0 .. end; the first T + 1 are
    committed going in): the row argmax g_r is greedy[p + r + 1] while the rows before it were
    accepted.  Returns (steps, hist [K + 1])."""
    greedy = np.asarray(greedy, dtype=np.int64)
    end = len(greedy) - 1
    p, steps, hist = T, 0, np.zeros(K + 1, dtype=np.int64)
    while p < end:
        rows, _, has = draft(greedy, p, K, ngram)
        g = []
        for r in range(K):  # row r's argmax is the greedy token only while its inputs are greedy
            if p + r + 1 > end or (r >= 1 and rows[r] != greedy[p + r]):
                break
            g.append(greedy[p + r + 1])
        g += [-1] * (K - len(g))
        _, cnt = accept(rows, g, has, p, end)
        p += cnt
        steps += 1
        hist[cnt] += 1
    return steps, hist
