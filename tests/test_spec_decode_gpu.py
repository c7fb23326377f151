"""Speculative greedy decoding through the decode path on the GPU (``generate_speculative``,
``_GpuCache.spec``): the tokens of ``generate`` bit for bit on three model shapes -- every row of a
verify step is computed from that row's inputs alone -- across the split change of the decode
attention, up to the last column of the window, on a replayed and on a re-captured graph; the
statistics add up, and over the cases the steps emit 1, between 2 and K - 1, and K tokens."""
import functools
import gc

import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig, generate_speculative
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

CONFIGS = {"w48-v512": dict(n_layer=3, n_head=3, n_embed=48, vocab_size=512, block_size=320),
           "w64-v50257": dict(n_layer=2, n_head=2, n_embed=64, vocab_size=50257, block_size=128),
           "w32-v97": dict(n_layer=2, n_head=2, n_embed=32, vocab_size=97, block_size=128)}
SHAPES = [(1, 1), (1, 3), (1, 7), (2, 3), (4, 1)]  # (B, draft_len)
T, NEW = 12, 44


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def _model(name):
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, **CONFIGS[name])
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


def _prompts(name, B, T, periodic, seed):
    """Random prompts, or a random 5-token pattern repeated (the n-gram draft matches at once)."""
    V = CONFIGS[name]["vocab_size"]
    g = torch.Generator().manual_seed(seed)
    if periodic:
        return torch.randint(0, V, (B, 5), generator=g).repeat(1, T // 5 + 1)[:, :T].contiguous().cuda()
    return torch.randint(0, V, (B, T), generator=g).cuda()


def _check_stats(stats, B, K, n):
    steps, hist = stats["steps"].cpu(), stats["emitted_hist"].cpu()
    assert steps.shape == (B,) and hist.shape == (B, K + 1) and steps.dtype == hist.dtype == torch.long
    e = torch.arange(K + 1)
    assert torch.equal((hist * e).sum(1), torch.full((B,), max(n - 1, 0))), hist.tolist()
    assert torch.equal(hist.sum(1), steps) and (hist[:, 0] == 0).all()
    return hist.sum(0)


@functools.lru_cache(maxsize=None)
def _run(name, B, draft_len, T, n, periodic, ngram=3):
    """One case: speculative against plain greedy, bit for bit, and the statistics; returns the
    histogram summed over the batch (kept, so the coverage test re-runs nothing)."""
    model = _model(name)
    idx = _prompts(name, B, T, periodic, seed=7 * B + draft_len)
    want = model.generate(idx, n)
    got, stats = model.generate_speculative(idx, n, draft_len=draft_len, ngram=ngram, return_stats=True)
    assert got.dtype == torch.long and got.shape == (B, T + n)
    assert torch.equal(got, want), f"first difference at column {int((got != want).any(0).nonzero()[0])} (T = {T})"
    return _check_stats(stats, B, draft_len + 1, n)


@pytest.mark.parametrize("periodic", [False, True], ids=["random", "periodic"])
@pytest.mark.parametrize("B,draft_len", SHAPES, ids=[f"B{b}-d{d}" for b, d in SHAPES])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_equals_generate(name, B, draft_len, periodic):
    _run(name, B, draft_len, T, NEW, periodic)


@pytest.mark.parametrize("B,draft_len", [(1, 7), (2, 3)], ids=lambda x: str(x))
def test_splits_change_mid_run(B, draft_len):
    """T = 250, n = 60: the decode attention goes from one split to two at position 256, inside a run
    and (K = 8) inside a group."""
    _run("w48-v512", B, draft_len, 250, 60, True)


@pytest.mark.parametrize("name,B,draft_len", [("w32-v97", 1, 7), ("w64-v50257", 2, 3), ("w48-v512", 1, 3)])
def test_fills_the_window(name, B, draft_len):
    """T + n == block_size: the last steps' rows run past the window and are skipped by the kernels."""
    bs = CONFIGS[name]["block_size"]
    _run(name, B, draft_len, bs - 40, 40, True)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_short_runs(n):
    model = _model("w32-v97")
    idx = _prompts("w32-v97", 2, T, True, seed=n)
    got, stats = model.generate_speculative(idx, n, draft_len=2, return_stats=True)
    assert torch.equal(got, model.generate(idx, n))
    assert stats["steps"].tolist() == [max(n - 1, 0)] * 2
    _check_stats(stats, 2, 3, n)


def test_replay_and_recapture():
    """A second call replays the captured graph and is equal; a call with another ngram or another
    length uses the same graph; a call after a weight change re-captures and follows the new weights."""
    name = "w64-v50257"
    model = _model(name)
    idx = _prompts(name, 1, T, True, seed=3)
    a, sa = model.generate_speculative(idx, NEW, draft_len=3, return_stats=True)
    loop = model._mg_spec_cache._loops[("spec", 4)]
    assert loop.graph is not None
    b, sb = model.generate_speculative(idx, NEW, draft_len=3, return_stats=True)
    assert torch.equal(a, b) and torch.equal(sa["emitted_hist"], sb["emitted_hist"])
    assert model._mg_spec_cache._loops[("spec", 4)] is loop
    c = model.generate_speculative(idx, NEW - 9, draft_len=3, ngram=1)
    assert torch.equal(c, a[:, :T + NEW - 9]) and model._mg_spec_cache._loops[("spec", 4)].graph is loop.graph
    w = model.transformer.h[0].mlp.c_fc.weight
    keep = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(-1.0)
        d = model.generate_speculative(idx, NEW, draft_len=3)
        assert model._mg_spec_cache._loops[("spec", 4)] is not loop
        assert torch.equal(d, model.generate(idx, NEW)) and not torch.equal(d, a)
    finally:
        with torch.no_grad():
            w.copy_(keep)
    assert torch.equal(model.generate_speculative(idx, NEW, draft_len=3), a)


def test_eager_steps_are_equal(monkeypatch):
    """The step launched eagerly (no graph) gives the same tokens and statistics."""
    name = "w48-v512"
    model = _model(name)
    idx = _prompts(name, 2, T, False, seed=5)
    a, sa = model.generate_speculative(idx, NEW, draft_len=3, return_stats=True)
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_spec_cache", None)
    b, sb = model.generate_speculative(idx, NEW, draft_len=3, return_stats=True)
    assert model._mg_spec_cache._loops[("spec", 4)].graph is None
    assert torch.equal(a, b) and torch.equal(sa["steps"], sb["steps"])
    model.__dict__.pop("_mg_spec_cache", None)  # an eager-built state has no graphs: start over


def test_plain_loops_left_alone():
    """Speculative calls keep a decode state of their own: ``generate`` replays the graph it had."""
    name = "w32-v97"
    model = _model(name)
    idx = _prompts(name, 2, T, True, seed=8)
    g0 = model.generate(idx, NEW)
    loops = model._mg_decode_cache._loops
    graph = loops["greedy"].graph
    model.generate_speculative(idx, NEW, draft_len=3)
    assert model._mg_decode_cache._loops is loops and loops["greedy"].graph is graph and graph is not None
    assert torch.equal(model.generate(idx, NEW), g0)


def test_argument_errors():
    model = _model("w32-v97")
    idx = _prompts("w32-v97", 1, T, True, seed=1)
    for kw, match in [(dict(draft_len=0), "draft_len"), (dict(draft_len=8), "draft_len"), (dict(ngram=0), "ngram"),
                      (dict(ngram=5), "ngram"), (dict(max_new_tokens=-1), "max_new_tokens"),
                      (dict(max_new_tokens=128 - T + 1), "block_size"),
                      (dict(idx=idx.repeat(3, 1), draft_len=3), "draft_len"),
                      (dict(idx=torch.tensor([[0, 97]]).cuda()), "outside"), (dict(idx=idx[0]), "idx")]:
        args = dict(idx=idx, max_new_tokens=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            generate_speculative(model, **args)


def test_every_kind_of_step_occurs():
    """Over the listed cases the histograms show a step emitting 1 token, one emitting between 2 and
    K - 1, and one emitting K -- rejections, partial acceptances and full acceptances all ran."""
    single = partial = full = 0
    for name in CONFIGS:
        for B, d in SHAPES:
            for periodic in (False, True):
                h = _run(name, B, d, T, NEW, periodic)
                K = d + 1
                single += int(h[1]) if K > 1 else 0
                partial += int(h[2:K].sum())
                full += int(h[K])
    print(f"steps emitting 1 token: {single}, 2 .. K - 1: {partial}, K: {full}")
    assert single > 0 and partial > 0 and full > 0
