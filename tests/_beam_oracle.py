"""The beam-search rule of csrc/include/common.h ('Beam search') over the reals, in numpy float64,
and the band check the GPU tests run against it.  A helper module, not a conftest: tests import what
they use.

One prompt at a time: ``scores`` [W] (the device's own fp32 sums going into the step, exact in
fp64), ``fin`` [W] bool, ``logits`` [W, V] (the step's bf16 logits as floats).  A live beam w offers
every (w, i) with c* = s_w + lp*_i; a finished beam only (w, pad) with c* = s_w.

Tolerance (derived, not chosen): a device candidate differs from c* by at most
``d = L.tol(V, lp) + 2^-23 |c|`` -- the log-probability kernel's four-times-the-bound plus the one
fp32 add.  A finished beam's candidate and a -inf candidate are exact (d = 0)."""
import numpy as np

import _logprob_oracle as L


def candidates(scores, fin, logits, pad):
    """(c*, d, offered), each [W, V]: the fp64 candidates, their allowed device error and which
    (w, i) are offered at all."""
    l = np.asarray(logits, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float64)
    fin = np.asarray(fin, dtype=bool)
    W, V = l.shape
    m, lnz = L.lse(l)
    lp = (l - m[:, None]) - lnz[:, None]
    with np.errstate(invalid="ignore"):
        c = s[:, None] + lp
        d = L.tol(V, lp) + 2.0 ** -23 * np.abs(c)
    d = np.where(np.isfinite(c), d, 0.0)
    offered = np.ones((W, V), dtype=bool)
    for w in np.nonzero(fin)[0]:
        offered[w] = False
        offered[w, pad] = True
        c[w, pad], d[w, pad] = s[w], 0.0
    return c, d, offered


def step(scores, fin, logits, eos, pad):
    """The rule itself, by brute force over all W * V candidates: (parents, tokens, scores,
    finished), best first -- c* descending, then the lower beam, then the row's own order (logit
    descending, index ascending)."""
    c, _, offered = candidates(scores, fin, logits, pad)
    W, V = c.shape
    l = np.asarray(logits, dtype=np.float64)
    ws, toks = np.nonzero(offered)
    # np.lexsort: the last key is the most significant
    order = np.lexsort((toks, -l[ws, toks], ws, -c[ws, toks]))[:W]
    par, tok = ws[order], toks[order]
    done = np.asarray(fin, dtype=bool)[par] | ((tok == eos) if eos is not None else False)
    return par, tok, c[par, tok], done


def band_check(scores, fin, logits, pad, parents, tokens, new_scores, what=""):
    """The device's choice ``(parents, tokens, new_scores)`` [W] of one prompt and step against the
    fp64 candidates, with no exclusions:
      * every chosen x and unchosen y: c*_x >= c*_y - (d_x + d_y);
      * consecutive chosen candidates are non-increasing within d_r + d_{r+1};
      * each new score is within d of the c* of its own (parent, token).
    Returns ``sharp``: every oracle-chosen candidate clears every other one by more than the two
    tolerances -- then the chosen SET must be the oracle's exactly, which is asserted too."""
    c, d, offered = candidates(scores, fin, logits, pad)
    W, V = c.shape
    par, tok = np.asarray(parents, dtype=np.int64), np.asarray(tokens, dtype=np.int64)
    got = np.asarray(new_scores, dtype=np.float64)
    assert ((0 <= par) & (par < W) & (0 <= tok) & (tok < V)).all(), f"{what}: parent / token out of range"
    assert offered[par, tok].all(), f"{what}: a chosen (parent, token) is not a candidate: {par}, {tok}"
    flat = par * V + tok
    assert len(set(flat.tolist())) == W, f"{what}: a candidate was chosen twice: {par}, {tok}"
    cx, dx = c[par, tok], d[par, tok]
    same = (got == cx) | (np.abs(got - cx) <= dx)  # -inf == -inf
    assert same.all(), f"{what}: new scores {got} vs c* {cx}, allowed {dx}"
    chosen = np.zeros((W, V), dtype=bool)
    chosen[par, tok] = True
    rest = offered & ~chosen
    if rest.any():
        lo, hi = (cx + dx).min(), (c[rest] - d[rest]).max()
        assert lo >= hi, f"{what}: an unchosen candidate beats a chosen one by {hi - lo:.3g} beyond the band"
    with np.errstate(invalid="ignore"):
        mono = (cx[:-1] >= cx[1:] - (dx[:-1] + dx[1:])) | (cx[:-1] == cx[1:])
    assert mono.all(), f"{what}: chosen candidates not in descending order: {cx}"
    opar, otok, oc, _ = step(scores, fin, logits, None, pad)
    orest = offered.copy()
    orest[opar, otok] = False
    sharp = (not orest.any()) or bool((oc - d[opar, otok]).min() > (c[orest] + d[orest]).max())
    if sharp:
        assert set(flat.tolist()) == set((opar * V + otok).tolist()), \
            f"{what}: the cut is sharp but the chosen set differs: {par}, {tok} vs {opar}, {otok}"
    return sharp
