"""Seeded sampling on the CPU: ``ops.reference.sample_gumbel`` and ``generate(seed=...)`` against
the rule restated in numpy uint32 / float64 (tests/_sample_oracle.py, which imports nothing from the
package and is shared with the GPU sampling tests)."""
import numpy as np
import pytest
import torch

import _sample_oracle as O
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.ops.reference import sample_gumbel

CHI2_10DOF_P1E4 = 35.56  # chi-square, 10 degrees of freedom, p = 1e-4


def _bf16_logits(B, V, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16)


def _model():
    torch.manual_seed(0)
    return GPT(GPTConfig(n_layer=2, n_head=2, n_embed=32, vocab_size=50, block_size=16), verbose=False).eval()


def test_restatement_hash_vectors():
    """The restatement itself: murmur3's finaliser on known inputs, and u strictly inside (0, 1)."""
    assert O.fmix32([0])[0] == 0
    assert O.fmix32([1])[0] == 0x514E28B7 and O.fmix32([0xFFFFFFFF])[0] == 0x81F16F39
    g = O.gumbel(seed=(1 << 64) - 1, draw=(1 << 32) - 1, rows=np.arange(3), V=4096)
    assert np.isfinite(g).all()
    assert not np.array_equal(g[0], g[1])


@pytest.mark.parametrize("V,k,T", [(1, None, 1.0), (7, None, 1.0), (7, 3, 0.5), (1000, 10, 1.0),
                                   (1000, 2000, 0.7), (1000, 999, 1.3), (50257, 40, 0.8)])
def test_sample_gumbel_matches_restatement(V, k, T):
    """Draw for draw: the fp64 torch implementation and the numpy restatement pick the same token
    (both are fp64: they may only differ where the top-two score gap is at rounding level)."""
    B = 8 if V > 10000 else 64
    logits = _bf16_logits(B, V, 3.0, 1)
    logits[0, V // 2] = float("-inf")
    n = 0
    for seed, draw, row0 in [(0, 0, 0), (123456789012345678, 7, 5), ((1 << 64) - 1, (1 << 31) + 3, 1000)]:
        got = sample_gumbel(logits, T, k, seed, draw, row0).view(-1).numpy()
        want, gap = O.sample(logits.float().numpy(), T, k, seed, draw, row0)
        ok = gap > 1e-9
        assert ok.mean() > 0.99
        assert np.array_equal(got[ok], want[ok])
        n += ok.sum()
    assert n > 0


def test_sample_gumbel_fp32_logits_and_shape():
    logits = torch.randn(5, 33)
    out = sample_gumbel(logits, 0.9, 4, seed=3, draw=2)
    assert out.shape == (5, 1) and out.dtype == torch.long
    want, _ = O.sample(logits.numpy(), 0.9, 4, 3, 2)
    assert np.array_equal(out.view(-1).numpy(), want)


@pytest.mark.parametrize("use_cache", [True, False])
def test_generate_seed_determinism(use_cache):
    m = _model()
    idx = torch.randint(0, 50, (3, 4))
    a = m.generate(idx, 20, do_sample=True, top_k=8, temperature=0.9, seed=11, use_cache=use_cache)
    torch.manual_seed(999)  # the global generator plays no part
    b = m.generate(idx, 20, do_sample=True, top_k=8, temperature=0.9, seed=11, use_cache=use_cache)
    c = m.generate(idx, 20, do_sample=True, top_k=8, temperature=0.9, seed=12, use_cache=use_cache)
    assert a.shape == (3, 24) and torch.equal(a[:, :4], idx)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert not torch.equal(a[0, 4:], a[1, 4:])  # rows draw independently


def test_generate_seed_follows_the_rule():
    """Each generated token is the restatement's pick from the logits of its prefix, with the
    token's column as the draw counter (window slide included: block_size 16, 24 columns)."""
    m = _model()
    idx = torch.randint(0, 50, (2, 4))
    out = m.generate(idx, 20, do_sample=True, top_k=5, temperature=0.7, seed=5)
    checked = 0
    with torch.no_grad():
        for col in range(4, 24):
            logits, _ = m(out[:, max(0, col - 16):col])
            want, gap = O.sample(logits[:, -1].numpy(), 0.7, 5, 5, col)
            ok = gap > 1e-3  # the KV-cache path and the full forward differ in fp32 rounding
            assert np.array_equal(out[:, col].numpy()[ok], want[ok])
            checked += ok.sum()
    assert checked >= 36


def test_generate_unseeded_unchanged():
    """seed=None: torch's global generator decides, as before."""
    m = _model()
    idx = torch.randint(0, 50, (2, 4))
    torch.manual_seed(7)
    a = m.generate(idx, 15, do_sample=True, top_k=5)
    torch.manual_seed(7)
    b = m.generate(idx, 15, do_sample=True, top_k=5)
    torch.manual_seed(8)
    c = m.generate(idx, 15, do_sample=True, top_k=5)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # and it is the reference's recipe: softmax of the top-k-masked logits, torch.multinomial
    torch.manual_seed(7)
    x = idx
    with torch.no_grad():
        for _ in range(3):
            logits = m(x)[0][:, -1].float()
            v, _ = torch.topk(logits, 5)
            logits[logits < v[:, [-1]]] = -float("inf")
            x = torch.cat([x, torch.multinomial(torch.softmax(logits, -1), 1)], 1)
    assert torch.equal(m.generate(idx, 0, do_sample=True, top_k=5), idx)
    torch.manual_seed(7)
    assert torch.equal(m.generate(idx, 3, do_sample=True, top_k=5, use_cache=False), x)


@pytest.mark.parametrize("seed", [1, 20240607, (1 << 63) + 12345])
def test_distribution_chi_square(seed):
    """V = 11, 8192 draws (one per batch row), chi-square against the fp64 softmax."""
    V, N = 11, 8192
    logits = _bf16_logits(1, V, 1.5, 3)
    p = torch.softmax(logits.double(), -1).view(-1).numpy()
    assert (p * N).min() > 5  # the chi-square approximation holds
    tok = sample_gumbel(logits.expand(N, V), 1.0, None, seed, draw=0).view(-1).numpy()
    obs = np.bincount(tok, minlength=V)
    chi2 = float(((obs - p * N) ** 2 / (p * N)).sum())
    print(f"seed {seed}: chi2 {chi2:.2f}, smallest expected count {(p * N).min():.1f}")
    assert chi2 < CHI2_10DOF_P1E4


def test_distribution_with_temperature_and_draws():
    """The same through the draw counter (B = 64 rows x 128 draws) at T = 2."""
    V, B, D = 11, 64, 128
    logits = _bf16_logits(1, V, 1.5, 3)
    p = torch.softmax(logits.double() * float(np.float32(0.5)), -1).view(-1).numpy()
    tok = np.concatenate([sample_gumbel(logits.expand(B, V), 2.0, None, 77, draw=d).view(-1).numpy()
                          for d in range(D)])
    obs = np.bincount(tok, minlength=V)
    chi2 = float(((obs - p * B * D) ** 2 / (p * B * D)).sum())
    print(f"chi2 {chi2:.2f}")
    assert chi2 < CHI2_10DOF_P1E4


def test_top_k_threshold_ties():
    """top_k = 3 with the threshold value four times over (two above it): nothing below the
    threshold is ever drawn, every tied token is."""
    V = 16
    l = torch.full((V,), -1.0)
    l[2], l[9] = 3.0, 2.5          # the top two
    l[[0, 5, 11, 15]] = 2.0        # the 3rd largest, four times: all kept
    l[7] = 1.984375                # the next bf16 below 2.0: never kept
    logits = l.to(torch.bfloat16).view(1, V).expand(4096, V)
    tok = sample_gumbel(logits, 1.0, 3, seed=9, draw=1).view(-1).numpy()
    seen = set(np.unique(tok).tolist())
    assert seen == {0, 2, 5, 9, 11, 15}
    want, _ = O.sample(logits.float().numpy(), 1.0, 3, 9, 1)
    assert np.array_equal(tok, want)


def test_argument_checks():
    m = _model()
    idx = torch.randint(0, 50, (1, 4))
    with pytest.raises(ValueError):
        m.generate(idx, 2, do_sample=True, top_k=0, seed=1)
    with pytest.raises(ValueError):
        m.generate(idx, 2, do_sample=True, temperature=0.0, seed=1)
    with pytest.raises(ValueError):
        sample_gumbel(torch.zeros(1, 4), 1.0, 0, 1, 0)
    with pytest.raises(ValueError):
        sample_gumbel(torch.zeros(1, 4), -1.0, None, 1, 0)
    # greedy ignores the seed
    assert torch.equal(m.generate(idx, 5, do_sample=False, seed=1), m.generate(idx, 5, do_sample=False))
