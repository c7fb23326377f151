"""Nucleus (top-p) sampling on the CPU: ``ops.reference.sample_gumbel(top_p=)``, ``generate`` and
``generate_batch`` against the rule restated in numpy float64 (tests/_nucleus_oracle.py, which
imports nothing from the package and is shared with the GPU top-p tests)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _nucleus_oracle as N
import _sample_oracle as O
from mingpt_distributed_amd.models import GPT, GPTConfig, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops import reference as R
from mingpt_distributed_amd.ops.reference import sample_gumbel

MARGIN = 1e-3


def _bf16_logits(B, V, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=64, vocab_size=300, block_size=32, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).eval()


# ------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("V,k,T,p", [(7, None, 1.0, 0.5), (7, 3, 0.5, 0.9), (1000, None, 1.0, 0.9),
                                     (1000, 10, 1.0, 0.5), (1000, 2000, 0.7, 0.3), (50257, None, 1.0, 0.9),
                                     (50257, 40, 0.8, 0.9), (50257, None, 1.3, 0.95)])
def test_sample_gumbel_matches_oracle(V, k, T, p):
    B = 4 if V > 10000 else 64
    logits = _bf16_logits(B, V, 1.0 if V < 100 else 3.0, V + (k or 0))
    l = logits.float().numpy()
    kept = N.keep(l, T, k, p)
    assert (kept.sum(1) < (np.isfinite(l).sum(1) if k is None else min(k, V))).any(), "the case has no teeth"
    n = 0
    for seed, draw, row0 in [(0, 0, 0), (123456789012345678, 7, 5), ((1 << 64) - 1, (1 << 31) + 3, 1000)]:
        got = sample_gumbel(logits, T, k, seed, draw, row0, p).view(-1).numpy()
        want, gap = N.sample(l, T, k, p, seed, draw, row0, kept=kept)
        ok = gap >= MARGIN
        assert ok.mean() > 0.95
        assert np.array_equal(got[ok], want[ok])
        assert kept[np.arange(B), got].all()
        n += ok.sum()
    assert n > 0


def test_off_is_bit_for_bit_the_present_function():
    logits = _bf16_logits(64, 1000, 3.0, 2)
    for k, T in [(None, 1.0), (10, 0.7)]:
        for draw in range(4):
            base = sample_gumbel(logits, T, k, 99, draw, 3)
            assert torch.equal(sample_gumbel(logits, T, k, 99, draw, 3, None), base)
            assert torch.equal(sample_gumbel(logits, T, k, 99, draw, 3, top_p=1.0), base)
            want, _ = O.sample(logits.float().numpy(), T, k, 99, draw, 3)
            assert np.array_equal(base.view(-1).numpy(), want)


def test_ties_straddling_the_boundary_are_kept_together():
    """3.0 once, 2.0 four times, the next bf16 below 2.0 once, -1.0 ten times at T = 1: the mass
    above 2.0 is 0.33 of the total and above 1.984375 it is 0.82, so top_p = 0.5 is reached inside
    the tie group: all four are kept and nothing below is."""
    V = 16
    l = torch.full((V,), -1.0)
    l[2] = 3.0
    l[[0, 5, 11, 15]] = 2.0
    l[7] = 1.984375
    logits = l.to(torch.bfloat16).view(1, V).expand(4096, V)
    low, cnt = N.threshold(logits[:1].float().numpy(), 1.0, None, 0.5)
    assert low[0] == 2.0 and cnt[0] == 5
    tok = sample_gumbel(logits, 1.0, None, seed=9, draw=1, top_p=0.5).view(-1).numpy()
    assert set(np.unique(tok).tolist()) == {0, 2, 5, 11, 15}
    want, _ = N.sample(logits.float().numpy(), 1.0, None, 0.5, 9, 1)
    assert np.array_equal(tok, want)
    # with top-k 3 first (ties at the k-th kept: the same five), and a top_p that drops the group
    tok = sample_gumbel(logits, 1.0, 3, seed=9, draw=2, top_p=0.5).view(-1).numpy()
    assert set(np.unique(tok).tolist()) == {0, 2, 5, 11, 15}
    tok = sample_gumbel(logits, 1.0, None, seed=9, draw=3, top_p=0.3).view(-1).numpy()
    assert set(np.unique(tok).tolist()) == {2}


def test_one_hot_row_and_minus_inf_entries():
    V = 50
    l = torch.full((3, V), -30.0)
    l[0, 17] = 30.0                      # one-hot: the maximum holds all the mass
    l[1] = float("-inf")
    l[1, 4] = -7.0                       # a single finite entry
    l[2, :10] = float("-inf")            # -inf entries next to a flat rest: never kept, no NaN
    l[2, 10:] = 0.0
    logits = l.to(torch.bfloat16)
    low, cnt = N.threshold(logits.float().numpy(), 1.0, None, 0.9)
    assert low.tolist() == [30.0, -7.0, 0.0] and cnt.tolist() == [1, 1, 40]
    seen2 = set()
    for d in range(64):
        tok = sample_gumbel(logits, 1.0, None, 5, d, top_p=0.9).view(-1).tolist()
        assert tok[0] == 17 and tok[1] == 4 and tok[2] >= 10
        seen2.add(tok[2])
    assert len(seen2) > 10
    # a tiny top_p keeps the maxima only
    tok = sample_gumbel(logits, 1.0, None, 5, 0, top_p=1e-6).view(-1).tolist()
    assert tok[0] == 17 and tok[1] == 4 and tok[2] >= 10


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.5, float("nan"), float("inf")])
def test_argument_rejection(model, bad):
    idx = torch.randint(0, 300, (1, 4))
    with pytest.raises(ValueError):
        R.check_sample_args(1.0, None, bad)
    with pytest.raises(ValueError):
        sample_gumbel(torch.zeros(1, 4), 1.0, None, 1, 0, top_p=bad)
    with pytest.raises(ValueError):
        model.generate(idx, 2, do_sample=True, seed=1, top_p=bad)
    with pytest.raises(ValueError):
        model.generate(idx, 2, do_sample=True, top_p=bad)
    with pytest.raises(ValueError):
        model.generate_batch([idx[0]], 2, do_sample=True, seed=1, top_p=bad)


def test_accepted_arguments():
    R.check_sample_args(1.0, None)
    R.check_sample_args(1.0, 5, None)
    R.check_sample_args(1.0, 5, 1.0)
    R.check_sample_args(1.0, None, 1e-30)


# ------------------------------------------------------------------------------------ generate
def _single(model, prompt, b, n, kw):
    """A hand-rolled loop over the CPU cache path on one row, as batch row b, picking with the oracle."""
    gaps = []
    with torch.no_grad():
        cache = gen._CpuCache(model, prompt.view(1, -1))
        out, logits = prompt.clone(), cache.logits
        for _ in range(n):
            col = out.numel()
            tok, gap = N.sample(logits.numpy(), kw["temperature"], kw["top_k"], kw["top_p"], kw["seed"], col, row0=b)
            gaps.append(gap[0])
            nxt = torch.from_numpy(tok).view(1, 1)
            out = torch.cat([out, nxt.view(1)])
            logits = cache.step(nxt, col)
    assert min(gaps) > 1e-9  # both sides are fp64: only a rounding-level tie could differ
    return out


SAMPLED = dict(do_sample=True, top_k=50, temperature=0.9, seed=4321, top_p=0.6)
LENS = [1, 5, 9, 3]
NEW = 10


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 300, (n,), generator=g) for n in LENS]


def test_generate_follows_the_rule(model, prompts):
    for kw in (SAMPLED, dict(SAMPLED, top_k=None)):
        want = _single(model, prompts[2], 0, NEW, kw)
        got = model.generate(prompts[2].view(1, -1), NEW, **kw)
        assert torch.equal(got[0], want)
        assert not torch.equal(got, model.generate(prompts[2].view(1, -1), NEW, **dict(kw, top_p=None)))
        assert torch.equal(model.generate(prompts[2].view(1, -1), NEW, **dict(kw, top_p=1.0)),
                           model.generate(prompts[2].view(1, -1), NEW, **dict(kw, top_p=None)))


def test_generate_without_cache_follows_the_rule(model, prompts):
    idx = prompts[1].view(1, -1).repeat(3, 1)
    out = model.generate(idx, NEW, use_cache=False, **SAMPLED)
    checked = 0
    with torch.no_grad():
        for col in range(5, 5 + NEW):
            logits, _ = model(out[:, :col])
            want, gap = N.sample(logits[:, -1].numpy(), 0.9, 50, 0.6, 4321, col)
            ok = gap > 1e-9
            assert np.array_equal(out[:, col].numpy()[ok], want[ok])
            checked += ok.sum()
    assert checked >= 3 * NEW - 1


def test_generate_batch_follows_the_rule(model, prompts):
    tokens, lengths = generate_batch(model, prompts, NEW, pad_token=7, **SAMPLED)
    assert lengths.tolist() == [n + NEW for n in LENS]
    for b, p in enumerate(prompts):
        assert torch.equal(tokens[b, :lengths[b]], _single(model, p, b, NEW, SAMPLED)), f"row {b}"
        assert (tokens[b, lengths[b]:] == 7).all()
    m_tokens, m_lengths = model.generate_batch(prompts, NEW, pad_token=7, **SAMPLED)
    assert torch.equal(m_tokens, tokens) and torch.equal(m_lengths, lengths)
    off, _ = generate_batch(model, prompts, NEW, pad_token=7, **dict(SAMPLED, top_p=None))
    assert not torch.equal(off, tokens)


def test_unseeded_path(model, prompts):
    """seed=None: with top_p=None the reference's recipe on torch's generator, exactly as before;
    with top_p every drawn token lies inside the fp64 nucleus of the logits it was drawn from."""
    idx = prompts[1].view(1, -1).repeat(4, 1)
    torch.manual_seed(7)
    x = idx
    with torch.no_grad():
        for _ in range(6):
            logits = model(x)[0][:, -1].float()
            v, _ = torch.topk(logits, 20)
            logits[logits < v[:, [-1]]] = -float("inf")
            x = torch.cat([x, torch.multinomial(torch.softmax(logits, -1), 1)], 1)
    for p in (None, 1.0):
        torch.manual_seed(7)
        assert torch.equal(model.generate(idx, 6, do_sample=True, top_k=20, use_cache=False, top_p=p), x)
    torch.manual_seed(7)
    cached = model.generate(idx, 6, do_sample=True, top_k=20)
    torch.manual_seed(7)
    assert torch.equal(model.generate(idx, 6, do_sample=True, top_k=20, top_p=None), cached)

    inside = total = 0
    for k in (20, None):
        torch.manual_seed(3)
        out = model.generate(idx, 12, do_sample=True, top_k=k, use_cache=False, top_p=0.4)
        with torch.no_grad():
            for col in range(5, 17):
                logits = model(out[:, :col])[0][:, -1].float().numpy()
                kept = N.keep(logits, 1.0, k, 0.4)
                assert kept[np.arange(4), out[:, col].numpy()].all()
                wide = N.keep(logits, 1.0, k, None)
                inside += kept.sum()
                total += wide.sum()
    assert inside < total / 2  # the nucleus excluded tokens: the assertion above has teeth


def test_cli_flag_reaches_generate(monkeypatch):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "projects", "generate",
                        "generate.py")
    spec = importlib.util.spec_from_file_location("generate_project_top_p", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = []
    real, real_batch = GPT.generate, GPT.generate_batch

    def generate(self, *a, **kw):
        seen.append(("generate", kw.get("top_p")))
        return real(self, *a, **kw)

    def generate_many(self, *a, **kw):
        seen.append(("generate_batch", kw.get("top_p")))
        return real_batch(self, *a, **kw)

    monkeypatch.setattr(GPT, "generate", generate)
    monkeypatch.setattr(GPT, "generate_batch", generate_many)
    base = ["--random-init", "--model-type", "gpt-micro", "--num-samples", "1", "--steps", "2", "--device", "cpu"]
    mod.main(base + ["--top-p", "0.8"])
    mod.main(base)
    mod.main(base + ["--top-p", "0.25", "--prompt", "1 2 3", "--prompt", "4 5"])
    assert seen == [("generate", 0.8), ("generate", None), ("generate_batch", 0.25)]
