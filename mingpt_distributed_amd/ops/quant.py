"""Weight-only int8 rows with power-of-two scales: the W8 rule of csrc/include/common.h in torch ops.

For W [N, K] and a_n = max_k |W[n, k]|: s_n = 1 and q = 0 for a zero row, else s_n is the smallest
power of two with a_n / s_n <= 127, taken from the exponent of a_n (frexp), and q[n, k] =
clamp(rne(W[n, k] / s_n), -127, 127).  Then |W - s q| <= s_n / 2 < a_n / 127, max_k |q[n, k]| >= 64
on a non-zero row, s q is exact in bf16 and ``quantize_rows(s q) == (q, s)``.  Works on CPU and GPU
tensors, bf16 and fp32.

``snap_vectors`` is the same rule per K / V vector of the int8 KV cache (the KV8 rule of common.h), with a
non-finite vector mapped to a NaN scale instead of an error."""
from __future__ import annotations

import torch

_MIN_EXP = -126  # s_n stays a normal fp32 (rows with a_n < 2^-119 lose the >= 64 consequence only)


def quantize_rows(w: torch.Tensor):
    """(q int8 [N, K], s float32 [N]) of ``w`` [N, K] (bf16 or fp32) by the W8 rule.  ValueError for a
    non-finite weight, another dtype or another rank."""
    if w.dim() != 2 or w.shape[1] < 1:
        raise ValueError(f"quantize_rows: a matrix [N, K] is needed, got {tuple(w.shape)}")
    if w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"quantize_rows: bf16 or fp32 weights, got {w.dtype}")
    f = w.detach().float()
    if not bool(torch.isfinite(f).all()):
        raise ValueError("quantize_rows: non-finite weight")
    a = f.abs().amax(dim=1)
    m, e = torch.frexp(a)  # a = m 2^e, m in [0.5, 1)
    ex = torch.where(m <= 127.0 / 128.0, e - 7, e - 6).clamp_(min=_MIN_EXP)
    one = torch.ones_like(a)
    s = torch.where(a > 0, torch.ldexp(one, ex), one)
    q = torch.round(f / s[:, None]).clamp_(-127, 127).to(torch.int8)  # exact division; halves to even
    return q, s


def snap_vectors(x: torch.Tensor):
    """The KV8 rule of csrc/include/common.h: ``(q, s, s * q)`` of ``x`` [..., n], the last dimension being
    the vector (the K, or the V, of one sequence, position, layer and head).  ``q`` int8 of ``x``'s shape,
    ``s`` [...] (float32; float64 for a float64 ``x``) and ``s * q`` in ``x``'s dtype.  With a = max |u|
    over a vector u: a not finite (a NaN or an inf anywhere in u) gives s = NaN and q = 0, so every
    dequantized element of that vector is NaN and no other vector is touched; a == 0 gives s = 1,
    q = 0; otherwise the W8 rule above, unchanged.  ``s * q`` is exact in bf16 and wider, and snapping
    it again returns the same ``(q, s)``.  Works on CPU and GPU tensors, bf16, fp32 and fp64."""
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"snap_vectors: a tensor [..., n] is needed, got {tuple(x.shape)}")
    if x.dtype not in (torch.bfloat16, torch.float32, torch.float64):
        raise ValueError(f"snap_vectors: bf16, fp32 or fp64 vectors, got {x.dtype}")
    f = x.detach().to(torch.float64 if x.dtype == torch.float64 else torch.float32)
    a = f.abs().amax(dim=-1)  # NaN if any element is
    ok = torch.isfinite(a)
    af = torch.where(ok, a, torch.zeros_like(a))
    m, e = torch.frexp(af)  # a = m 2^e, m in [0.5, 1)
    ex = torch.where(m <= 127.0 / 128.0, e - 7, e - 6).clamp_(min=_MIN_EXP)
    one = torch.ones_like(af)
    s = torch.where(af > 0, torch.ldexp(one, ex), one)
    fz = torch.where(ok.unsqueeze(-1), f, torch.zeros_like(f))
    q = torch.round(fz / s.unsqueeze(-1)).clamp_(-127, 127)  # exact division; halves to even
    s = torch.where(ok, s, torch.full_like(s, float("nan")))
    return q.to(torch.int8), s, (q * s.unsqueeze(-1)).to(x.dtype)


def dequantize_rows(q: torch.Tensor, s: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """s_n q[n, k] as ``dtype`` (exact in bf16 and wider)."""
    return (q.float() * s[:, None].float()).to(dtype)
