"""``kv_cache="int8"`` on the CPU halves of ``generate_beam``, ``generate_speculative`` and ``score``: the
KV8 model (every K and V vector snapped before any attention reads it) as ``generate(kv_cache="int8")``
runs it, on a float32 model of 2 layers.  Comparisons between an incremental decode and a full forward
use the tolerance ``test_beam_cpu`` / ``test_logprobs_cpu`` use on the default path, rtol = atol = 1e-5."""
import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig, generate_beam, generate_speculative, score

V, BS, T, NEW = 96, 48, 6, 10
TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=32, vocab_size=V, block_size=BS, embed_drop=0.0, resid_drop=0.0,
                    attn_drop=0.0)
    m = GPT(cfg, verbose=False).eval()
    with torch.no_grad():  # the initialisation's near-uniform model hides the K/V rounding: sharpen it
        for p in m.parameters():
            if p.dim() >= 2:
                p.mul_(3.0)
    return m


@pytest.fixture(scope="module")
def idx():
    return torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(5))


def test_one_beam_is_kv8_greedy(model, idx):
    tokens, lengths, scores = generate_beam(model, idx, NEW, 1, kv_cache="int8")
    g, lp = model.generate(idx, NEW, return_logprobs=True, kv_cache="int8")
    assert torch.equal(tokens[:, 0], g) and (lengths == T + NEW).all()
    torch.testing.assert_close(scores[:, 0], lp[:, T:].sum(1), **TOL)


def test_three_beams_score_as_the_kv8_model(model, idx):
    B, W = idx.size(0), 3
    tokens, lengths, scores = generate_beam(model, idx, NEW, W, kv_cache="int8")
    assert (lengths == T + NEW).all()
    lp = score(model, tokens.view(B * W, T + NEW), kv_cache="int8")[:, T:].sum(1).view(B, W)
    torch.testing.assert_close(scores, lp, **TOL)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    # another model than the bf16-cache one: the beams or their scores differ for some prompt
    t16, _, s16 = generate_beam(model, idx, NEW, W)
    # (by more than ten times the tolerance above)
    assert not torch.equal(tokens, t16) or not torch.allclose(scores, s16, rtol=1e-4, atol=1e-4)
    # and the default model's score of the same beams is not the KV8 model's
    assert not torch.allclose(score(model, tokens.view(B * W, -1))[:, T:].sum(1).view(B, W), lp, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,draft_len", [(1, 3), (2, 3), (1, 7)])
def test_speculative_is_kv8_greedy(model, B, draft_len):
    g = torch.Generator().manual_seed(B + draft_len)
    prompts = torch.randint(0, V, (B, 5), generator=g).repeat(1, 3)[:, :12].contiguous()
    n = 20
    out, stats = generate_speculative(model, prompts, n, draft_len=draft_len, return_stats=True, kv_cache="int8")
    assert torch.equal(out, model.generate(prompts, n, kv_cache="int8"))
    hist, steps = stats["emitted_hist"], stats["steps"]
    K = draft_len + 1
    assert hist.shape == (B, K + 1) and torch.equal((hist * torch.arange(K + 1)).sum(1), torch.full((B,), n - 1))
    assert torch.equal(hist.sum(1), steps) and (hist[:, 0] == 0).all()


def test_score_matches_the_kv8_decode(model, idx):
    g, lp = model.generate(idx, NEW, return_logprobs=True, kv_cache="int8")
    got = score(model, g, kv_cache="int8")
    torch.testing.assert_close(got[:, T:], lp[:, T:], **TOL)
    assert (got[:, 0] == 0).all()
    assert not torch.allclose(got, score(model, g), rtol=1e-4, atol=1e-4), "the KV8 model scores as the default one"
    lengths = torch.tensor([T + NEW, 5, 9])
    padded = score(model, g, lengths, kv_cache="int8")
    for b, n in enumerate(lengths.tolist()):
        assert (padded[b, n:] == 0).all()
        torch.testing.assert_close(padded[b, 1:n], got[b, 1:n], **TOL)


def test_kv_cache_is_validated(model, idx):
    for call in (lambda kv: generate_beam(model, idx, 2, 2, kv_cache=kv),
                 lambda kv: generate_speculative(model, idx[:1], 2, kv_cache=kv),
                 lambda kv: score(model, idx, kv_cache=kv)):
        for kv in ("fp8", "INT8", None):
            with pytest.raises(ValueError, match="kv_cache"):
                call(kv)


def test_bf16_is_the_call_without_the_argument(model, idx):
    a, b = generate_beam(model, idx, NEW, 3, kv_cache="bf16"), generate_beam(model, idx, NEW, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    p = idx[:1].repeat(1, 2)
    assert torch.equal(generate_speculative(model, p, NEW, kv_cache="bf16"), generate_speculative(model, p, NEW))
    assert torch.equal(score(model, idx, kv_cache="bf16"), score(model, idx))
