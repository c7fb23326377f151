"""The per-token log-probability rule of csrc/include/common.h ('Per-token log-probabilities') over
the reals, in numpy float64: the log-softmax of a row of logits at temperature 1, before any top-k or
top-p filter.  A helper module, not a conftest: tests import what they use.

``bound`` is the error the rule's fp32 / integer evaluation may have against this, as derived in
common.h; the tests allow ``FACTOR`` times it (the factor of the top-p tests)."""
import numpy as np

EPS_W = 4.4e-6  # common.h: relative error of one fp32 weight of the nucleus / log-probability rule
FACTOR = 4.0


def lse(l):
    """(m, ln Z) per row of ``l`` [..., V]: the row maximum and the log of sum exp(l - m); -inf
    entries weigh 0."""
    l = np.asarray(l, dtype=np.float64)
    m = l.max(axis=-1)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(l), 0.0, np.exp(l - m[..., None]))
    return m, np.log(w.sum(axis=-1))


def logprob(l, t):
    """lp of token ``t`` [...] under the rows of ``l`` [..., V]; -inf for a -inf logit."""
    l = np.asarray(l, dtype=np.float64)
    m, lnz = lse(l)
    lt = np.take_along_axis(l, np.asarray(t, dtype=np.int64)[..., None], axis=-1)[..., 0]
    return (lt - m) - lnz


def bound(V, lp):
    """|device lp - real lp| allowed by the derivation in common.h, for a vocabulary of V and a
    log-probability of ``lp``: eps_w + V 2^-32 (the integer masses), 2^-23 (ln V + 1) (the
    conversion and logf), 2^-23 |lp| (the two subtractions)."""
    lp = np.abs(np.asarray(lp, dtype=np.float64))
    return EPS_W + V * 2.0 ** -32 + 2.0 ** -23 * (np.log(V) + 1.0) + 2.0 ** -23 * lp


def tol(V, lp):
    return FACTOR * bound(V, lp)
