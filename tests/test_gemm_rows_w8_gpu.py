"""The W8 rows GEMM (gemm_rows_w8, csrc/kernels/gemm_rows.hip) through the binding: bit-equal to gemm_rows on
the dequantized matrix and inside its fp64 bound; exact integers over all of -127..127 against fp64 rounded
once (a sign-extension, byte-order or lane-slot mistake is an O(1) error whatever the bf16 kernel does); guard
bands and a pad column; argument checks."""
import math

import numpy as np
import pytest
import torch

from _guard import BACK, FRONT, SENTINEL_BYTE, bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext
from mingpt_distributed_amd.ops.quant import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16


def _bf(*shape, scale=1.0, seed=0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)


# one partial step on wave 0, quarter 0, the last column tile 7 wide | 2 row tiles, a fifth partial step wraps to
# wave 0 | 3 row tiles, wave 0 takes a second load group | 4 row tiles, gpt2-xl's widest row | the longest row
@pytest.mark.parametrize("M,N,K", [(9, 23, 8), (17, 23, 136), (33, 40, 520), (64, 23, 6400), (49, 16, 8192)], ids=str)
def test_equals_gemm_rows_and_fp64(M, N, K):
    """Per epilogue: the bits of gemm_rows on s q, and |got - ref| <= 1.13 (2^-8 |ref| + 2 K 2^-24 S) against fp64
    with S = sum_k |x_k s q_k| + |bias| + |resid|, test_gemm_rows_gpu.py's bound."""
    C = ext()
    w = _bf(N, K, scale=0.05, seed=K + N + 1)
    w[N // 2] = 0  # a zero row: scale 1, q 0
    q, s = quantize_rows(w)
    assert float(s[N // 2]) == 1.0 and not q[N // 2].any()
    x, bias, resid = _bf(M, K, seed=K + M), _bf(N, seed=K + 2), _bf(M, N, seed=K + 3)
    x64, w64 = x.double().numpy(), dequantize_rows(q, s, torch.float64).numpy()
    b64, r64 = bias.double().numpy(), resid.double().numpy()
    x, q, s, w, bias, resid = (t.to(DEV) for t in (x, q, s, dequantize_rows(q, s), bias, resid))
    for epi in (0, 1, 2, 3):
        b, r = bias if epi else None, resid if epi == 3 else None
        y = C.gemm_rows_w8(x, q, s, epi, b, r, 0)
        assert y.shape == (M, N) and bit_equal(y, C.gemm_rows(x, w, epi, b, r, 0))
        ref, S = x64 @ w64.T + (b64 if epi else 0), np.abs(x64) @ np.abs(w64).T + (np.abs(b64) if epi else 0)
        if epi == 2:
            ref = 0.5 * ref * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (ref + 0.044715 * ref ** 3)))
        if epi == 3:
            ref, S = ref + r64, S + np.abs(r64)
        allow = 1.13 * (2.0 ** -8 * np.abs(ref) + 2 * K * 2.0 ** -24 * S)
        err = np.abs(y.double().cpu().numpy() - ref)
        print(f"({M}, {N}, {K}) epilogue {epi}: worst error / allowance {float((err[allow > 0] / allow[allow > 0]).max()):.3f}")
        assert (err <= allow).all(), f"epilogue {epi}: {int((err > allow).sum())} elements outside the allowance"


@pytest.mark.parametrize("M,N,K", [(64, 23, 520), (9, 23, 8)], ids=str)
def test_exact_integers(M, N, K):
    """q over all of -127..127, scales 2^-3 .. 2^2 by row, x integers of -4..4: every sum is below 2^24, exact
    in fp32, and the output is the fp64 result rounded once to bf16."""
    rng = np.random.default_rng(K)
    q, x, s = rng.integers(-127, 128, size=(N, K)), rng.integers(-4, 5, size=(M, K)), 2.0 ** (np.arange(N) % 6 - 3)
    q.flat[0], q.flat[-1] = -127, 127
    assert q.min() == -127 and q.max() == 127 and np.abs(x @ q.T).max() < 2 ** 24
    t = lambda a, dt: torch.from_numpy(a).to(dt).to(DEV)
    y = ext().gemm_rows_w8(t(x, BF), t(q, torch.int8), t(s, torch.float32), 0, None, None, 0)
    bad = y != t((x @ q.T) * s, BF)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} wrong, first at (row, column) {bad.nonzero()[0].tolist()}"


def test_guard_bands_and_padding():
    """(33, 23, 136), ldy = 24, epilogue 3: q inside an int8 buffer whose margins hold 127, x, scale, bias and
    resid between NaN margins: finite, equal to the plain run, no margin changed, the pad column untouched."""
    C = ext()
    M, N, K, ld = 33, 23, 136, 24
    x, b, r = _bf(M, K, seed=31).to(DEV), _bf(N, seed=33).to(DEV), _bf(M, ld, seed=34).to(DEV)
    q, s = (t.to(DEV) for t in quantize_rows(_bf(N, K, scale=0.05, seed=32)))
    qbuf = torch.full((FRONT + N * K + BACK,), 127, dtype=torch.int8, device=DEV)
    qv = qbuf[FRONT:FRONT + N * K].view(N, K).copy_(q)
    (got,), _ = guarded(lambda x, scale, bias, resid: C.gemm_rows_w8(x, qv, scale, 3, bias, resid, ld)[:, :N],
                        {"x": x, "scale": s, "bias": b, "resid": r}, name="gemm_rows_w8 epi 3")
    assert (qbuf[:FRONT] == 127).all() and (qbuf[FRONT + N * K:] == 127).all() and torch.equal(qv, q)
    want = C.gemm_rows_w8(x, q, s, 3, b, r, ld)[:, :N].clone()
    assert bit_equal(got, want) and bit_equal(want, C.gemm_rows(x, dequantize_rows(q, s), 3, b, r, ld)[:, :N])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    block = torch.empty(M, ld, dtype=BF, device=DEV)  # y lands on this block, filled with the sentinel and freed
    block.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    ptr = block.data_ptr()
    del block
    y = C.gemm_rows_w8(x, q, s, 3, b, r, ld)
    assert y.data_ptr() == ptr, "y did not land on the sentinel block: nothing was checked"
    assert bit_equal(y[:, :N], want) and (y[:, N:].contiguous().view(torch.uint8) == SENTINEL_BYTE).all()


def test_refusals():
    C = ext()
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=DEV)
    q, one = lambda *s: z(*s, dt=torch.int8), lambda n, dt=torch.float32: torch.ones(n, dtype=dt, device=DEV)
    assert C.gemm_rows_w8_supported(64, 8192) and not C.gemm_rows_w8_supported(65, 8)
    assert C.gemm_rows_w8(z(9, 16), q(16, 16), one(16), 0, None, None, 24).shape == (9, 24)
    for args in [(z(65, 8), q(16, 8), one(16)), (z(9, 8200), q(16, 8200), one(16)),  # M = 65; K = 8200
                 (z(9, 12), q(16, 12), one(16)), (z(9, 16), z(16, 16), one(16)),  # K % 8; Wq not int8
                 (z(9, 16), q(16, 16), one(15)), (z(9, 16), q(16, 16), one(16, BF)),  # scale: size; dtype
                 (z(9, 16), q(16 * 16 + 4)[4:].view(16, 16), one(16))]:  # Wq 4 bytes off 8-byte alignment
        with pytest.raises((ValueError, RuntimeError)):
            C.gemm_rows_w8(*args, 0, None, None, 0)
