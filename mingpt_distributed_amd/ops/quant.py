"""Weight-only int8 rows with power-of-two scales: the W8 rule of csrc/include/common.h in torch ops.

For W [N, K] and a_n = max_k |W[n, k]|: s_n = 1 and q = 0 for a zero row, else s_n is the smallest
power of two with a_n / s_n <= 127, taken from the exponent of a_n (frexp), and q[n, k] =
clamp(rne(W[n, k] / s_n), -127, 127).  Then |W - s q| <= s_n / 2 < a_n / 127, max_k |q[n, k]| >= 64
on a non-zero row, s q is exact in bf16 and ``quantize_rows(s q) == (q, s)``.  Works on CPU and GPU
tensors, bf16 and fp32."""
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


def dequantize_rows(q: torch.Tensor, s: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """s_n q[n, k] as ``dtype`` (exact in bf16 and wider)."""
    return (q.float() * s[:, None].float()).to(dtype)
