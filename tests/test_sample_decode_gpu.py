"""Seeded sampling through the decode path: the device-side token loop (``_GpuCache.sample``: LM
head, then the sample kernel, captured once and replayed) and ``generate(seed=...)`` on the GPU,
against the rule restated in numpy float64 (tests/_sample_oracle.py)."""
import numpy as np
import pytest
import torch

import _sample_oracle as O
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
BS = 64


def _model(vocab):
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=vocab, block_size=BS, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


@pytest.fixture(scope="module", params=[9000, 1000])
def setup(request):
    model = _model(request.param)
    idx = torch.randint(0, request.param, (2, 5), device="cuda")
    return model, idx, request.param


def test_teacher_forced_parity(setup):
    """30 device-loop tokens, then the same tokens fed one by one through the logits step of a
    second decode state (same kernels, so the same bf16 logits): the rule applied to each step's
    logits gives the device's token wherever the fp64 top-two gap is at least 1e-3; at most 2 of
    the 60 draws may fall under that margin."""
    model, idx, V = setup
    B, T0, n = 2, idx.size(1), 30
    seed, T, k = 1234567, 0.9, 50
    with torch.no_grad():
        dev = gen._GpuCache(model, idx, BS)
        first = dev.sample_prefill(gen._sample_words(seed, T0, T, k)).clone()
        seq = dev.sample(first.view(B, 1), T0, n, gen._sample_words(seed, T0 + 1, T, k)).clone()
        ref = gen._GpuCache(model, idx, BS)
        want0, gap0 = O.sample(ref.logits.float().cpu().numpy(), T, k, seed, T0)
        ok = gap0 >= MARGIN
        assert np.array_equal(first.cpu().numpy()[ok], want0[ok])
        toks = torch.cat([first.view(B, 1), seq], 1)
        skipped = 0
        for j in range(n):
            logits = ref.step(toks[:, j:j + 1].contiguous(), T0 + j)
            want, gap = O.sample(logits.float().cpu().numpy(), T, k, seed, T0 + 1 + j)
            ok = gap >= MARGIN
            skipped += int((~ok).sum())
            got = seq[:, j].cpu().numpy()
            assert np.array_equal(got[ok], want[ok]), f"step {j}: device {got}, rule {want}, gap {gap}"
    assert ((seq >= 0) & (seq < V)).all()
    print(f"skipped {skipped} of {B * n}")
    assert skipped <= 2


def test_graph_against_eager(setup, monkeypatch):
    model, idx, V = setup
    kw = dict(do_sample=True, top_k=20, temperature=0.8, seed=99)
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_decode_cache", None)
    a = model.generate(idx, 40, **kw)
    monkeypatch.setattr(gen, "_GRAPH_DECODE", True)
    b = model.generate(idx, 40, **kw)
    assert a.shape == (2, 45) and torch.equal(a, b)


def test_repeat_and_recapture(setup):
    """A second call replays the cached graph and repeats the tokens; another seed, top_k or
    temperature changes the tokens through the parameter block, on the same graph object."""
    model, idx, V = setup
    kw = dict(do_sample=True, top_k=20, temperature=0.8)
    a = model.generate(idx, 40, seed=7, **kw)
    graph = model._mg_decode_cache._loops["sample"].graph
    b = model.generate(idx, 40, seed=7, **kw)
    assert torch.equal(a, b)
    c = model.generate(idx, 40, seed=8, **kw)
    assert not torch.equal(a, c)
    d = model.generate(idx, 40, seed=7, do_sample=True, top_k=3, temperature=0.8)
    e = model.generate(idx, 40, seed=7, do_sample=True, top_k=20, temperature=3.0)
    f = model.generate(idx, 40, seed=7, do_sample=True, top_k=None, temperature=0.8)
    assert not torch.equal(a, d) and not torch.equal(a, e) and not torch.equal(a, f)
    assert model._mg_decode_cache._loops["sample"].graph is graph
    assert torch.equal(model.generate(idx, 40, seed=7, **kw), a)


def test_no_cache_path_follows_the_rule(setup):
    """use_cache=False with a seed: the full forward, then ops.reference.sample_gumbel on the
    device.  Each token is the restatement's pick from the logits of its prefix."""
    model, idx, V = setup
    a = model.generate(idx, 6, do_sample=True, top_k=5, seed=3, use_cache=False)
    assert a.shape == (2, 11) and torch.equal(a, model.generate(idx, 6, do_sample=True, top_k=5, seed=3,
                                                                use_cache=False))
    with torch.no_grad():
        for col in range(5, 11):
            logits = model(a[:, :col])[0][:, -1]
            want, gap = O.sample(logits.float().cpu().numpy(), 1.0, 5, 3, col)
            ok = gap >= MARGIN
            assert np.array_equal(a[:, col].cpu().numpy()[ok], want[ok])


def test_window_slide(setup):
    model, idx, V = setup
    a = model.generate(idx, 90, do_sample=True, top_k=10, seed=21)
    b = model.generate(idx, 90, do_sample=True, top_k=10, seed=21)
    assert a.shape == (2, 95) and torch.equal(a, b)
    assert torch.equal(a[:, :5], idx) and ((a >= 0) & (a < V)).all()


def test_greedy_intact(setup):
    """Greedy before and after a sampled call: the greedy graphs, their device buffers and the
    LM-head argmax keys are untouched by the sampled loop."""
    model, idx, V = setup
    g0 = model.generate(idx, 50, do_sample=False)
    ggraph = model._mg_decode_cache._loops["greedy"].graph
    model.generate(idx, 50, do_sample=True, top_k=10, seed=1)
    g1 = model.generate(idx, 50, do_sample=False)
    assert torch.equal(g0, g1)
    assert model._mg_decode_cache._loops["greedy"].graph is ggraph
    torch.manual_seed(3)
    u0 = model.generate(idx, 10, do_sample=True, top_k=10)  # the unseeded host loop still works
    torch.manual_seed(3)
    u1 = model.generate(idx, 10, do_sample=True, top_k=10)
    assert torch.equal(u0, u1) and u0.shape == (2, 15)
