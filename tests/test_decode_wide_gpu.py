"""The device decode loops on models whose MLP output projection is wider than 4096 columns
(n_embed 1280 and 1600: gpt2-large's and gpt2-xl's widths, K = 5120 and 6400 on the skinny GEMM's
two-segment path): speculative decoding equals greedy bit for bit, the decode step does go through
the skinny GEMM, the captured graph equals the eager step loop, greedy follows ``use_cache=False``
up to a near-tie of the reference's logits, and the sampled, log-probability and beam loops run,
repeat, and report the log-softmax of their own logits."""
import functools
import gc

import numpy as np
import pytest
import torch

import _logprob_oracle as L
from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops import reference as R
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

BS = 96
CONFIGS = {"w1280-v50257": dict(n_layer=2, n_head=20, n_embed=1280, vocab_size=50257, block_size=BS),  # fused argmax
           "w1280-v512": dict(n_layer=2, n_head=20, n_embed=1280, vocab_size=512, block_size=BS),      # torch argmax
           "w1600-v512": dict(n_layer=2, n_head=25, n_embed=1600, vocab_size=512, block_size=BS)}      # K = 6400
SHAPES = [(1, 1), (1, 7), (2, 3), (4, 1)]  # (B, draft_len)
T, NEW = 12, 40
SEEDED = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.9, seed=1234567)


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


@functools.lru_cache(maxsize=None)
def _greedy(name, B, seed, periodic=False):
    """(prompt, greedy tokens) on the captured graph: computed once, shared, left unchanged."""
    idx = _prompts(name, B, T, periodic, seed)
    return idx, _model(name).generate(idx, NEW)


# ------------------------------------------------------------------ 1. speculative equals greedy
@pytest.mark.parametrize("periodic", [False, True], ids=["random", "periodic"])
@pytest.mark.parametrize("B,draft_len", SHAPES, ids=[f"B{b}-d{d}" for b, d in SHAPES])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_speculative_equals_generate(name, B, draft_len, periodic):
    model = _model(name)
    idx, want = _greedy(name, B, 7 * B + draft_len, periodic)
    K = draft_len + 1
    got, stats = model.generate_speculative(idx, NEW, draft_len=draft_len, return_stats=True)
    assert got.dtype == torch.long and got.shape == (B, T + NEW)
    assert torch.equal(got, want), f"first difference at column {int((got != want).any(0).nonzero()[0])} (T = {T})"
    steps, hist = stats["steps"].cpu(), stats["emitted_hist"].cpu()
    assert steps.shape == (B,) and hist.shape == (B, K + 1) and steps.dtype == hist.dtype == torch.long
    assert torch.equal((hist * torch.arange(K + 1)).sum(1), torch.full((B,), NEW - 1)), hist.tolist()
    assert torch.equal(hist.sum(1), steps) and (hist[:, 0] == 0).all()


# ------------------------------------------------------------------ 2. the skinny path is taken
@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_goes_through_the_skinny_gemm(name, monkeypatch):
    """Without this, every other test's ``generate`` could pass on the MFMA fallback."""
    model, C = _model(name), ext()
    D = CONFIGS[name]["n_embed"]
    assert C.gemv_supported(8, 4 * D)
    widths = []
    real = C.gemv

    def counted(x, *args, **kw):
        widths.append(x.size(-1))
        return real(x, *args, **kw)

    idx, want = _greedy(name, 2, 3)
    model.__dict__.pop("_mg_decode_cache", None)  # a fresh state: the step is built (and called) again
    monkeypatch.setattr(C, "gemv", counted)
    got = model.generate(idx, NEW)
    monkeypatch.undo()
    model.__dict__.pop("_mg_decode_cache", None)
    assert widths.count(4 * D) >= 1, f"no skinny GEMM call on {4 * D} columns (widths seen: {sorted(set(widths))})"
    assert widths.count(D) >= 3 * widths.count(4 * D)  # qkv, attention projection, MLP in (and the LM head)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ 3. graph equals eager
@pytest.mark.parametrize("name", list(CONFIGS))
def test_graph_equals_eager_and_replays(name, monkeypatch):
    model = _model(name)
    idx, a = _greedy(name, 2, 5)
    b = model.generate(idx, NEW)  # captures, if another test's batch size came in between
    graph = model._mg_decode_cache._loops["greedy"].graph
    c = model.generate(idx, NEW)  # replays the captured graph
    assert graph is not None and model._mg_decode_cache._loops["greedy"].graph is graph
    assert torch.equal(a, b) and torch.equal(a, c)
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_decode_cache", None)
    c = model.generate(idx, NEW)
    assert model._mg_decode_cache._loops["greedy"].graph is None
    assert torch.equal(a, c)
    model.__dict__.pop("_mg_decode_cache", None)  # an eager-built state has no graphs: start over


# ------------------------------------------------------------------ 4. greedy against use_cache=False
@pytest.mark.parametrize("name", list(CONFIGS))
def test_greedy_follows_the_uncached_reference(name):
    """``use_cache=False`` re-runs the whole prefix on the MFMA GEMM; the decode step's logits
    differ from its in the last bf16 bits.  A row may leave the reference only at a column where the
    reference's two best logits are closer than 0.05 (bf16 logits of magnitude under about 8
    resolve 2^-5); a row is compared up to its first such column."""
    model = _model(name)
    idx, got = _greedy(name, 2, 11)
    with torch.no_grad():
        want = model.generate(idx, NEW, use_cache=False)
        agree = 0
        for b in range(idx.size(0)):
            diff = (got[b] != want[b]).nonzero()
            col = int(diff[0]) if diff.numel() else T + NEW
            agree += col - T
            if diff.numel():
                top = model(want[b:b + 1, :col])[0][0, -1].float().topk(2).values
                gap = float(top[0] - top[1])
                print(f"row {b} leaves the reference at column {col}: top-two gap {gap:.4f}")
                assert gap < 0.05, f"row {b} differs at column {col} where the reference's gap is {gap:.4f}"
    print(f"{name}: {agree} of {idx.size(0) * NEW} tokens compared, all equal")


# ------------------------------------------------------------------ 5. the other loops
def _teacher_forced(model, idx, tokens, n):
    """fp64 log-probabilities [rows, n] of ``tokens[:, T0:T0 + n]`` on the logits of a second decode
    state fed the same tokens one by one (the same kernels on the same rows: the same bf16 logits)."""
    T0 = idx.size(1)
    out = []
    with torch.no_grad():
        ref = gen._GpuCache(model, idx, BS)
        logits = ref.logits
        for j in range(n):
            col = T0 + j
            out.append(R.token_logprob(logits, tokens[:, col]).double().cpu().numpy())
            if j + 1 < n:
                logits = ref.step(tokens[:, col:col + 1].contiguous(), col)
    return np.stack(out, axis=1)


@pytest.mark.parametrize("mode", ["greedy", "seeded"])
def test_sampled_and_logprob_loops(mode):
    name = "w1280-v50257"
    model, V = _model(name), CONFIGS[name]["vocab_size"]
    kw = SEEDED if mode == "seeded" else {}
    idx = _prompts(name, 2, T, False, seed=13)
    plain = model.generate(idx, NEW, **kw)
    tokens, lp = model.generate(idx, NEW, return_logprobs=True, **kw)
    assert torch.equal(tokens, plain) and lp.dtype == torch.float32 and lp.shape == tokens.shape
    assert (lp[:, :T] == 0.0).all() and (lp[:, T:] < 0).all() and torch.isfinite(lp).all()
    again = model.generate(idx, NEW, return_logprobs=True, **kw)
    assert torch.equal(again[0], tokens) and bit_equal(again[1], lp) and torch.equal(model.generate(idx, NEW, **kw), plain)
    if mode == "greedy":
        assert torch.equal(plain, model.generate(idx, NEW))
    want = _teacher_forced(model, idx, tokens, NEW)
    err, tol = np.abs(lp[:, T:].double().cpu().numpy() - want), L.tol(V, want)
    print(f"worst error {float((err / tol).max()):.3f} of the allowed")
    assert (err <= tol).all()


def test_two_beams():
    name = "w1280-v50257"
    model, V = _model(name), CONFIGS[name]["vocab_size"]
    idx = _prompts(name, 1, T, False, seed=17)
    n, W = 24, 2
    tokens, lengths, scores = model.generate_beam(idx, n, W)
    assert tokens.shape == (1, W, T + n) and (lengths == T + n).all() and scores.dtype == torch.float32
    assert torch.isfinite(scores).all() and scores[0, 0] >= scores[0, 1]
    again = model.generate_beam(idx, n, W)
    assert torch.equal(again[0], tokens) and torch.equal(again[1], lengths) and bit_equal(again[2], scores)
    # every beam's score is the sum of its tokens' log-probabilities: teacher-forced as W rows
    want = _teacher_forced(model, idx.repeat(W, 1), tokens[0], n)
    tol = L.tol(V, want).sum(1) + n * 2.0 ** -23 * np.abs(want).sum(1)  # n lp errors + n fp32 adds
    err = np.abs(scores[0].double().cpu().numpy() - want.sum(1))
    print(f"beam scores {scores[0].tolist()}, |error| {err.tolist()}, allowed {tol.tolist()}")
    assert (err <= tol).all()
