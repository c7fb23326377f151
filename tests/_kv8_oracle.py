"""The KV8 rule (csrc/include/common.h) in numpy, written from the rule's words and not from
``ops/quant.py``: the scale of a vector is the SMALLEST power of two s >= 2^-126 with a / s <= 127,
found by trying the three candidates around the exponent of a = max |u|; a NaN or inf anywhere in
the vector gives s = NaN and q = 0; a zero vector s = 1, q = 0.

A helper module, not a conftest: tests import what they use.  Inputs are float32 or float64 arrays
(a bf16 tensor goes in as its exact float32 values)."""
from __future__ import annotations

import numpy as np

S_MIN_EXP = -126


def scale_of(a):
    """The scale of one vector with a = max |u| (a Python float or numpy scalar)."""
    a = float(a)
    if not np.isfinite(a):
        return float("nan")
    if a == 0.0:
        return 1.0
    _, e = np.frexp(a)  # 2^(e-1) <= a < 2^e
    for k in (int(e) - 8, int(e) - 7, int(e) - 6):
        k = max(k, S_MIN_EXP)
        if a / 2.0 ** k <= 127.0:  # exact: a power of two, fp64 holds every fp32 quotient
            return 2.0 ** k
    raise AssertionError(f"no scale for a = {a!r}")


def snap(u):
    """(q int8 [..., n], s [...] float32 -- float64 for float64 input --, s * q in u's dtype) of the
    vectors along the last axis of ``u``."""
    u = np.asarray(u)
    assert u.dtype in (np.float32, np.float64) and u.ndim >= 1 and u.shape[-1] >= 1
    flat = u.reshape(-1, u.shape[-1]).astype(np.float64)
    q = np.zeros(flat.shape, dtype=np.int8)
    s = np.ones(flat.shape[0], dtype=np.float64)
    for i, vec in enumerate(flat):
        if not np.isfinite(vec).all():
            s[i] = np.nan
            continue
        s[i] = scale_of(np.abs(vec).max())
        q[i] = np.clip(np.rint(vec / s[i]), -127, 127).astype(np.int8)  # rint: halves to even
    deq = (q.astype(np.float64) * s[:, None]).astype(u.dtype)
    sd = np.float64 if u.dtype == np.float64 else np.float32
    return q.reshape(u.shape), s.astype(sd).reshape(u.shape[:-1]), deq.reshape(u.shape)
