"""The residual-stream dropout mask against an independent oracle.

The keep-rate tests (tests/test_dropout_rate_gpu.py) pass for any mask with the right density, and
the kernel-vs-kernel tests share csrc/include/common.h's helpers: a mask that repeated per tile or
per row block would pass both.  Here the documented rule is written out again in torch integer
arithmetic (int64 values masked to 32 bits), from the comment in common.h:

    word(m, n) = fmix32(m * ceil(N / 2) + (n >> 1) + key(seed))          (32-bit wrap-around)
    key(seed)  = fmix32(lo32(seed) ^ 0x0d0f0d0f) ^ (hi32(seed) * 0x9E3779B1)
    element (m, n) of a row-major [M, N] tensor takes half (n & 1) of its word (0: low 16 bits) and
    is kept iff that half >= thr = round(65536 p); kept values are scaled by 65536 / (65536 - thr)

and every kernel that applies the mask must reproduce the oracle's keep set exactly.  The embedding
forward (embedding.hip) uses the same rule with m = the token's row in [B * T] and N = n_embed.
"""
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
M32 = 0xFFFFFFFF
SEEDS = [7, (5 << 32) + 7, (1 << 63) - 12345]  # the second differs from the first in the high word only


def _mul32(h, c):
    """(h * c) mod 2^32 for int64 tensors / Python ints 0 <= h < 2^32, without leaving 63 bits."""
    return ((h & 0xFFFF) * c + ((((h >> 16) * c) & 0xFFFF) << 16)) & M32


def _fmix32(h):
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def _key(seed):
    lo, hi = seed & M32, (seed >> 32) & M32
    return _fmix32(lo ^ 0x0D0F0D0F) ^ _mul32(hi, 0x9E3779B1)


def threshold(p):
    return int(round(65536 * p))


def keep_scale(p):
    return 65536.0 / (65536 - threshold(p))


def oracle_keep(M, N, p, seed, device="cpu"):
    """bool [M, N]: the elements the documented rule keeps."""
    m = torch.arange(M, dtype=torch.int64, device=device)[:, None]
    n = torch.arange(N, dtype=torch.int64, device=device)[None, :]
    word = _fmix32((_mul32(m, (N + 1) // 2) + (n >> 1) + _key(seed)) & M32)
    half = torch.where((n & 1) == 1, word >> 16, word & 0xFFFF)
    return half >= threshold(p)


def test_oracle_self_check():
    """fmix32 is murmur3's finaliser (published vectors), the keep rate at p = 0.1 is within 1e-3
    over >= 1e7 draws, and seeds matter -- the low word and the high word."""
    assert _fmix32(0) == 0 and _fmix32(1) == 0x514E28B7 and _fmix32(0xFFFFFFFF) == 0x81F16F39
    t = torch.tensor([1, 0xFFFFFFFF], dtype=torch.int64)
    assert _fmix32(t).tolist() == [0x514E28B7, 0x81F16F39]
    assert _mul32(torch.tensor([0xFFFFFFFF]), 0xC2B2AE35).item() == (0xFFFFFFFF * 0xC2B2AE35) & M32
    M, N = 2500, 4001  # odd N: rows start on a fresh word
    keep = oracle_keep(M, N, 0.1, SEEDS[0])
    assert keep.numel() >= 10_000_000
    assert abs(keep.float().mean().item() - 0.9) < 1e-3
    assert (keep.float().mean(0) - 0.9).abs().max().item() < 0.03  # no dead or stuck columns
    for other in SEEDS[1:] + [8]:
        diff = (oracle_keep(64, N, 0.1, other) != keep[:64]).float().mean().item()
        assert 0.1 < diff < 0.26, (other, diff)  # two independent masks differ at 2 * 0.9 * 0.1 = 0.18
    assert threshold(0.1) == 6554 and threshold(0.3) == 19661 and abs(keep_scale(0.1) - 1 / 0.9) < 1e-4


def _ext():
    from mingpt_distributed_amd.ops._ext import ext

    return ext()


def _assert_mask(out, p, seed, what):
    """out = keep * scale (bf16) of an all-ones input."""
    M, N = out.shape
    want = oracle_keep(M, N, p, seed, device=out.device)
    got = out != 0
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {out.numel()} keep decisions differ from the documented "
                           f"rule, first at (m, n) = {tuple(bad.nonzero()[0].tolist())}")
    kept = out[got].float()
    assert torch.equal(kept, torch.full_like(kept, keep_scale(p)).to(BF).float()), f"{what}: keep scale"


@gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("M,N", [(5, 24), (130, 520), (37, 1600)])
def test_elementwise_and_layernorm_masks(M, N, p, seed):
    C = _ext()
    ones = torch.ones(M, N, device=DEV, dtype=BF)
    zeros = torch.zeros(M, N, device=DEV, dtype=BF)
    _assert_mask(C.bias_dropout_residual(ones, None, zeros, p, seed), p, seed, "bias_dropout_residual")
    _assert_mask(C.dropout_bwd(ones, p, seed), p, seed, "dropout_bwd")
    db = torch.zeros(N, device=DEV)
    dx = C.dropout_bias_grad(ones, db, p, seed)
    _assert_mask(dx, p, seed, "dropout_bias_grad")
    # the column sums are of the fp32 kept values (before dx's bf16 rounding): count * scale
    cols = oracle_keep(M, N, p, seed, device=DEV).float().sum(0) * keep_scale(p)
    torch.testing.assert_close(db, cols, atol=2e-2, rtol=1e-3)  # test_kernels_gpu.py:264
    # LayerNorm backward with the fused residual-dropout backward: dy = 0 makes dx = dres = 1 exactly
    x = torch.randn(M, N, device=DEV).to(BF)
    w = torch.ones(N, device=DEV, dtype=BF)
    _, mean, rstd = C.layernorm_fwd(x, w, torch.zeros_like(w), 1e-5)
    z = lambda: torch.zeros(N, device=DEV)  # noqa: E731
    dx, dz = C.layernorm_bwd_dropout(zeros, x, w, mean, rstd, z(), z(), ones, z(), p, seed)
    assert torch.equal(dx, ones)
    _assert_mask(dz, p, seed, "layernorm_bwd_dropout dz")


@gpu
@pytest.mark.parametrize("seed", SEEDS[:2])
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_embedding_mask(p, seed):
    """embedding.hip: rowdrop8(.., m = token row in [B * T], c = column, N = D): the same rule."""
    C = _ext()
    B, T, V, D = 3, 70, 11, 520
    idx = torch.randint(0, V, (B, T), device=DEV)
    wte = torch.ones(V, D, device=DEV, dtype=BF)
    wpe = torch.zeros(T, D, device=DEV, dtype=BF)
    out = C.embedding_fwd(idx, wte, wpe, p, seed)
    _assert_mask(out.view(B * T, D), p, seed, "embedding_fwd")
    # and the backward regenerates it: dwpe[t] = sum_b mask[b * T + t] * scale for dout = 1
    dwte, dwpe = torch.zeros(V, D, device=DEV), torch.zeros(T, D, device=DEV)
    C.embedding_bwd(idx, torch.ones(B, T, D, device=DEV, dtype=BF), dwte, dwpe, p, seed)
    keep = oracle_keep(B * T, D, p, seed, device=DEV).float() * keep_scale(p)
    torch.testing.assert_close(dwpe, keep.view(B, T, D).sum(0), atol=1e-3, rtol=1e-3)  # test_kernels_gpu.py:103
    ref = torch.zeros(V, D, device=DEV).index_add_(0, idx.flatten(), keep)
    torch.testing.assert_close(dwte, ref, atol=1e-3, rtol=1e-3)


@gpu
@pytest.mark.parametrize("variant", [0, 1, 5, 6], ids=["auto", "t128", "w4", "w4n192"])
@pytest.mark.parametrize("seed", SEEDS[:2])
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_gemm_resid_epilogue_mask(p, seed, variant):
    """out = resid + drop(A W^T + b) with A W^T = 0, b = 1, resid = 0 (test_residual_dropout_rate's
    construction) at 520 x 520: more than two 256-tiles in both directions, each partial."""
    from mingpt_distributed_amd.ops import gemm as G

    C = _ext()
    M = N = 520
    K = 64
    a = torch.zeros(M, K, device=DEV, dtype=BF)
    w = torch.zeros(N, K, device=DEV, dtype=BF)
    bias = torch.ones(N, device=DEV, dtype=BF)
    resid = torch.zeros(M, N, device=DEV, dtype=BF)
    C.gemm_set_variant(variant)
    try:
        out = G.gemm_nt(a, w, bias=bias, epi="resid", resid=resid, p=p, seed=seed)
    finally:
        C.gemm_set_variant(0)
    _assert_mask(out, p, seed, f"gemm resid epilogue (tile configuration {variant})")
