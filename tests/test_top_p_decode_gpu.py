"""Nucleus (top-p) sampling through the decode paths on the GPU: ``generate(seed=, top_p=)`` (the
captured sampled loop), ``generate_batch(top_p=)`` (the ragged loop) and ``use_cache=False``, against
the rule restated in numpy float64 (tests/_nucleus_oracle.py).

Every token is checked teacher-forced: the generated sequence is fed one token at a time through
the logits step of a second decode state (same kernels, so the same bf16 logits) and the rule is
applied to each step's logits.  A draw counts where it is decided (``_nucleus_oracle.bracket``: the
same fp64 token at top_p (1 +- delta) and top-two score gaps of at least 1e-3)."""
import gc

import numpy as np
import pytest
import torch

import _nucleus_oracle as N
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

BS = 64
V = 1000
KW = dict(do_sample=True, top_k=None, temperature=0.8, seed=1234567, top_p=0.5)


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=V, block_size=BS, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def idx():
    g = torch.Generator().manual_seed(1)
    return torch.randint(0, V, (2, 5), generator=g).cuda()


def _check_row(model, ref, seq, T0, b, kw):
    """Row ``seq`` (1-D, a prompt of T0 tokens first) against the rule on the B = 1 decode path's
    logits, as batch row b; ``ref``: a B = 1 decode state to prefill again, or None.  No token may
    lie outside the nucleus at top_p (1 + delta).  Returns (ref, decided draws, undecided draws)."""
    decided = undecided = 0
    d = N.delta(V, kw["top_p"])
    with torch.no_grad():
        prompt = seq[None, :T0].contiguous()
        if ref is None:
            ref = gen._GpuCache(model, prompt, BS)
        else:
            ref.prefill(prompt)
        logits = ref.logits
        for col in range(T0, seq.numel()):
            l = logits.float().cpu().numpy()
            want, ok = N.bracket(l, kw["temperature"], kw["top_k"], kw["top_p"], kw["seed"], col, row0=b)
            got = int(seq[col])
            if ok[0]:
                assert got == int(want[0]), f"row {b} column {col}: device {got}, rule {int(want[0])}"
            decided += int(ok[0])
            undecided += int(not ok[0])
            assert N.keep(l, kw["temperature"], kw["top_k"], kw["top_p"] * (1 + d))[0, got], \
                f"row {b} column {col}: token {got} is outside the nucleus"
            if col + 1 < seq.numel():
                logits = ref.step(seq[col:col + 1].view(1, 1).contiguous(), col)
    return ref, decided, undecided


def _check(model, out, lens, kw, max_undecided):
    """Every row of ``out`` ((prompt length, total length) per row in ``lens``); returns the number
    of decided draws."""
    decided = undecided = 0
    ref = None
    for b in range(out.size(0)):
        ref, a, u = _check_row(model, ref, out[b, :int(lens[b][1])], int(lens[b][0]), b, kw)
        decided, undecided = decided + a, undecided + u
    print(f"decided {decided}, undecided {undecided}")
    assert undecided <= max_undecided
    return decided


@pytest.mark.parametrize("k", [None, 50])
def test_generate_follows_the_rule(model, idx, k):
    """30 tokens for 2 rows; the B = 2 loop's logits are the B = 1 path's on this model
    (tests/test_generate_batch_gpu.py, RECT_DIFF 'tiny').  At most 2 of the 60 draws may be
    undecided, as in the top-k decode test."""
    kw = dict(KW, top_k=k)
    out = model.generate(idx, 30, **kw)
    assert out.shape == (2, 35) and torch.equal(out[:, :5], idx)
    assert _check(model, out, [(5, 35)] * 2, kw, 2) >= 58
    off = model.generate(idx, 30, **dict(kw, top_p=None))
    assert not torch.equal(off, out)
    assert torch.equal(model.generate(idx, 30, **dict(kw, top_p=1.0)), off)


def test_another_top_p_on_the_same_graph(model, idx, monkeypatch):
    a = model.generate(idx, 30, **KW)
    graph = model._mg_decode_cache._loops["sample"].graph
    assert graph is not None
    kw = dict(KW, top_p=0.9)
    b = model.generate(idx, 30, **kw)
    assert model._mg_decode_cache._loops["sample"].graph is graph
    assert not torch.equal(a, b)
    _check(model, b, [(5, 35)] * 2, kw, 2)
    assert torch.equal(model.generate(idx, 30, **KW), a)
    assert model._mg_decode_cache._loops["sample"].graph is graph
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_decode_cache", None)
    assert torch.equal(model.generate(idx, 30, **kw), b), "the replayed loop differs from eager launches"
    model.__dict__.pop("_mg_decode_cache", None)


LENS = [1, 5, 17, 3]


def _prompts():
    g = torch.Generator().manual_seed(2)
    return [torch.randint(0, V, (n,), generator=g).cuda() for n in LENS]


def test_generate_batch_ragged(model):
    """Every row is the single-prompt rule on that row alone, with batch row b and the row's own
    columns as draw counters; the ragged loop serves another top_p without a new capture."""
    prompts = _prompts()
    kw = dict(KW, top_k=50)
    tokens, lengths = model.generate_batch(prompts, 20, pad_token=7, **kw)
    assert lengths.tolist() == [n + 20 for n in LENS]
    for b, n in enumerate(LENS):
        assert torch.equal(tokens[b, :n], prompts[b]) and (tokens[b, n + 20:] == 7).all()
    _check(model, tokens, [(n, n + 20) for n in LENS], kw, 3)
    graph = model._mg_decode_cache._loops[("ragged", False)].graph
    kw9 = dict(kw, top_p=0.9)
    t9, _ = model.generate_batch(prompts, 20, pad_token=7, **kw9)
    assert model._mg_decode_cache._loops[("ragged", False)].graph is graph
    assert not torch.equal(t9, tokens)
    _check(model, t9, [(n, n + 20) for n in LENS], kw9, 3)
    off, _ = model.generate_batch(prompts, 20, pad_token=7, **dict(kw, top_p=None))
    assert not torch.equal(off, tokens)


def test_generate_batch_equal_lengths_is_generate(model):
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, V, (3, 7), generator=g).cuda()
    want = model.generate(idx, 30, **KW)
    tokens, lengths = model.generate_batch(list(idx), 30, **KW)
    assert torch.equal(tokens, want) and lengths.tolist() == [37] * 3


def test_rows_finished_by_eos_are_left_alone(model):
    prompts = _prompts()
    full, _ = model.generate_batch(prompts, 20, **KW)
    eos = None
    for b, n in enumerate(LENS):  # a token some row produced at step >= 3, new to that row
        part = full[b, n:n + 20].tolist()
        for j in range(3, 20):
            if eos is None and part[j] not in part[:j]:
                eos = part[j]
    assert eos is not None
    tokens, lengths = model.generate_batch(prompts, 20, eos_token=eos, pad_token=3, **KW)
    stopped = 0
    for b, n in enumerate(LENS):
        part = full[b, n:n + 20].tolist()
        keep = part.index(eos) + 1 if eos in part else 20
        stopped += keep < 20
        assert int(lengths[b]) == n + keep
        assert torch.equal(tokens[b, :n + keep], full[b, :n + keep])
        assert (tokens[b, n + keep:] == 3).all()
    assert stopped >= 1


def test_no_cache_path_follows_the_rule(model, idx):
    """use_cache=False: the full forward, then ops.reference.sample_gumbel(top_p=) on the device; each
    token is the rule's pick from the logits of its prefix.  Its first token is the cached path's
    wherever the draw is decided on both paths' logits."""
    kw = dict(KW, top_k=50)
    a = model.generate(idx, 6, use_cache=False, **kw)
    assert a.shape == (2, 11) and torch.equal(a, model.generate(idx, 6, use_cache=False, **kw))
    decided = 0
    with torch.no_grad():
        for col in range(5, 11):
            logits = model(a[:, :col])[0][:, -1]
            want, ok = N.bracket(logits.float().cpu().numpy(), kw["temperature"], 50, kw["top_p"], kw["seed"], col)
            assert np.array_equal(a[:, col].cpu().numpy()[ok], want[ok])
            decided += ok.sum()
        assert decided >= 10
        cached = model.generate(idx, 6, **kw)
        l_full = model(idx)[0][:, -1].float().cpu().numpy()
        l_dec = gen._GpuCache(model, idx, BS).logits.float().cpu().numpy()
        w1, ok1 = N.bracket(l_full, kw["temperature"], 50, kw["top_p"], kw["seed"], 5)
        w2, ok2 = N.bracket(l_dec, kw["temperature"], 50, kw["top_p"], kw["seed"], 5)
        both = ok1 & ok2 & (w1 == w2)
        assert np.array_equal(a[:, 5].cpu().numpy()[both], cached[:, 5].cpu().numpy()[both])
