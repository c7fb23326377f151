"""Beam search through the decode path on the GPU (``generate_beam``, ``_GpuCache.beam``): one beam
against greedy decoding bit for bit, the device loop replayed teacher-forced through a second decode
state and checked step by step against the rule in numpy float64 (tests/_beam_oracle.py: the band
``d = L.tol(V, lp) + 2^-23 |c|``, no exclusions), scores against ``GPT.score``, the stop token, repeat
/ eager / early-exit bit-equality, and the plain loops left alone.  The model is that of
test_logprob_decode_gpu.py."""
import gc

import numpy as np
import pytest
import torch

import _beam_oracle as O
from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig, generate_beam
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

BS, T, NEW = 64, 5, 30


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


def _model(vocab):
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=vocab, block_size=BS, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


@pytest.fixture(scope="module", params=[9000, 1000], ids=["9000", "1000"])
def setup(request):
    """(model, prompts [3, 5], V)."""
    V = request.param
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(V)).cuda()
    return _model(V), idx, V


def _histories(model, W, cols):
    st = model._mg_beam_cache.beam_state(W)
    return [st[k][:, :, cols].cpu().numpy() for k in ("hparent", "htok", "hscore")]


def _backtrack(hparent, htok):
    B, W, n = htok.shape
    out = np.zeros((B, W, n), dtype=np.int64)
    for b in range(B):
        for w in range(W):
            r = w
            for j in range(n - 1, -1, -1):
                out[b, w, j] = htok[b, r, j]
                r = hparent[b, r, j]
    return out


def test_one_beam_is_greedy(setup):
    """W = 1: the tokens of ``generate`` bit for bit, and the score is the sequential fp32 sum of
    ``generate(return_logprobs=True)``'s numbers."""
    model, idx, V = setup
    tokens, lengths, scores = model.generate_beam(idx[:2], NEW, 1)
    assert tokens.shape == (2, 1, T + NEW) and (lengths == T + NEW).all() and scores.dtype == torch.float32
    g, lp = model.generate(idx[:2], NEW, return_logprobs=True)
    assert torch.equal(tokens[:, 0], g) and torch.equal(g, model.generate(idx[:2], NEW))
    lp = lp.cpu().numpy()
    for b in range(2):
        s = np.float32(0.0)
        for x in lp[b, T:]:
            s = np.float32(s + np.float32(x))
        assert np.float32(scores[b, 0].item()) == s, f"row {b}: {scores[b, 0].item()!r} vs {s!r}"


@pytest.mark.parametrize("B,W", [(1, 4), (2, 4), (1, 3), (1, 8), (3, 4)], ids=lambda x: str(x))
def test_teacher_forced_replay(setup, B, W):
    """The device loop's token and parent histories fed step by step through a second decode state
    of B * W rows (the same kernels on the same rows, so the loop's own logits; its caches
    re-gathered with ``index_select`` by the parents): the band check holds at every step with the
    device's own scores going in, and the returned sequences are the backtrack of the histories.
    (3, 4) is 12 rows: the MFMA path."""
    model, idx, V = setup
    idx = idx[:B].contiguous()
    R = B * W
    tokens, lengths, scores = model.generate_beam(idx, NEW, W, pad_token=2)
    assert tokens.shape == (B, W, T + NEW) and (lengths == T + NEW).all()
    assert (tokens[:, :, :T] == idx[:, None]).all()
    hparent, htok, hscore = _histories(model, W, slice(T, T + NEW))
    assert np.array_equal(tokens[:, :, T:].cpu().numpy(), _backtrack(hparent, htok))
    assert bit_equal(scores.cpu(), torch.from_numpy(hscore[:, :, -1].copy()))
    with torch.no_grad():
        ref = gen._GpuCache(model, idx, BS, rows=R)
        logits = ref.beam_prefill(idx, W)[:, :V]
        s = np.full((B, W), -np.inf)
        s[:, 0] = 0.0
        fin = np.zeros((B, W), dtype=bool)
        base = torch.arange(B).view(B, 1) * W
        sharp = 0
        for j in range(NEW):
            lf = logits.float().cpu().numpy().reshape(B, W, V)
            for b in range(B):
                sharp += O.band_check(s[b], fin[b], lf[b], 2, hparent[b, :, j], htok[b, :, j], hscore[b, :, j],
                                      what=f"step {j}, prompt {b}")
            s = hscore[:, :, j].astype(np.float64)
            if j + 1 < NEW:
                rows = (base + torch.from_numpy(hparent[:, :, j]).long()).view(R).cuda()
                ref.kv.copy_(ref.kv.index_select(1, rows))
                tok = torch.from_numpy(htok[:, :, j]).long().view(R, 1).cuda()
                logits = ref.step(tok, T + j)
    print(f"sharp cut (chosen set equal to the oracle's) at {sharp} of {B * NEW} steps")


def test_scores_sorted_and_match_score(setup):
    """``scores[b]`` is non-increasing in w, and each beam's score is the sum of ``model.score``
    over its generated tokens within the tolerance of test_score_against_decode (MFMA prefill against
    skinny-GEMM decode logits): 2 * (2e-2 + 2e-2 * max |logit|) per token, summed."""
    model, idx, V = setup
    W = 4
    tokens, lengths, scores = model.generate_beam(idx[:2], NEW, W)
    assert (scores[:, :-1] >= scores[:, 1:]).all() and torch.isfinite(scores).all() and (scores < 0).all()
    for b in range(2):
        sc = model.score(tokens[b])
        with torch.no_grad():
            big = model(tokens[b])[0].float().abs().amax(-1)  # row j - 1 predicts column j
        tol = (2 * (2e-2 + 2e-2 * big[:, T - 1:-1])).sum(1)
        err = (sc[:, T:].sum(1) - scores[b]).abs()
        print(f"prompt {b}: max |sum of score - beam score| {float(err.max()):.4g}, allowed {float(tol.min()):.4g}")
        assert (err <= tol).all()


def test_stop_token(setup, monkeypatch):
    """The stop token is the best free-run beam's fourth generated token: with it set, that beam is
    among the results with length T + 4 (sooner if the token came up sooner), ends in it and is
    padded; a finished beam offers only the pad token at a frozen score from its finishing step on;
    reading the finished flags and stopping early changes nothing."""
    model, idx, V = setup
    W, pad = 4, 3
    idx = idx[:2].contiguous()
    free, _, _ = model.generate_beam(idx, NEW, W, pad_token=pad)
    best = free[0, 0, T:].tolist()
    eos = best[3]
    k = best.index(eos)  # its first occurrence: 3 unless the token came up before
    tokens, lengths, scores = model.generate_beam(idx, NEW, W, eos_token=eos, pad_token=pad)
    hit = [w for w in range(W) if tokens[0, w, T:T + k + 1].tolist() == best[:k + 1]]
    assert hit, f"the free run's best beam {best[:k + 1]} is not among {tokens[0, :, T:T + k + 1].tolist()}"
    w = hit[0]
    assert int(lengths[0, w]) == T + k + 1 and int(tokens[0, w, T + k]) == eos and (tokens[0, w, T + k + 1:] == pad).all()
    for b in range(2):
        for w in range(W):
            n = int(lengths[b, w])
            gen_toks = tokens[b, w, T:n].tolist()
            assert eos not in gen_toks[:-1] and (tokens[b, w, n:] == pad).all()
            assert n == T + NEW or gen_toks[-1] == eos
    monkeypatch.setattr(gen, "_EARLY_EXIT", False)
    full = model.generate_beam(idx, NEW, W, eos_token=eos, pad_token=pad)
    assert torch.equal(full[0], tokens) and torch.equal(full[1], lengths) and bit_equal(full[2], scores)
    hparent, htok, hscore = _histories(model, W, slice(T, T + NEW))  # every column: no early exit
    fin = np.zeros((2, W), dtype=bool)
    frozen = 0
    for j in range(NEW):
        for b in range(2):
            par = hparent[b, :, j]
            was = fin[b, par]
            if j:
                assert (htok[b, was, j] == pad).all()
                assert np.array_equal(hscore[b, was, j].view(np.int32), hscore[b, par[was], j - 1].view(np.int32))
                frozen += int(was.sum())
            fin[b] = was | (htok[b, :, j] == eos)
    assert frozen > 0


def test_repeat_and_eager_are_bit_equal(setup, monkeypatch):
    model, idx, V = setup
    idx = idx[:2].contiguous()
    a = model.generate_beam(idx, NEW, 4)
    b = model.generate_beam(idx, NEW, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bit_equal(a[2], b[2])
    assert model._mg_beam_cache._loops[("beam", 4)].graph is not None
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_beam_cache", None)
    c = model.generate_beam(idx, NEW, 4)
    assert model._mg_beam_cache._loops[("beam", 4)].graph is None
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and bit_equal(a[2], c[2])
    model.__dict__.pop("_mg_beam_cache", None)  # an eager-built state has no graphs: start over


def test_plain_loops_left_alone(setup):
    """Beam calls keep a decode state of their own: ``generate`` and ``generate_batch`` return what
    they returned before, from the same graph objects, under the same loop keys."""
    model, idx, V = setup
    idx = idx[:2].contiguous()
    model.__dict__.pop("_mg_decode_cache", None)
    g0 = model.generate(idx, NEW)
    loops = model._mg_decode_cache._loops
    graph = loops["greedy"].graph
    assert graph is not None
    model.generate_beam(idx, NEW, 4)
    model.generate_beam(idx, NEW, 1)  # two rows, as many as the plain state's
    assert model._mg_decode_cache._loops is loops and set(loops) == {"greedy"} and loops["greedy"].graph is graph
    assert torch.equal(model.generate(idx, NEW), g0) and loops["greedy"].graph is graph
    rows = [torch.randint(0, V, (n,), generator=torch.Generator().manual_seed(n)).cuda() for n in (5, 17, 9)]
    r0 = model.generate_batch(rows, 20)
    loops = model._mg_decode_cache._loops
    graph = loops[("ragged", True)].graph
    model.generate_beam(idx, NEW, 3)
    assert set(loops) == {("ragged", True)} and loops[("ragged", True)].graph is graph and graph is not None
    r1 = model.generate_batch(rows, 20)
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1]) and loops[("ragged", True)].graph is graph


def test_arguments(setup):
    model, idx, V = setup
    tokens, lengths, scores = model.generate_beam(idx, 0, 3)
    assert torch.equal(tokens, idx[:, None].expand(3, 3, T)) and (lengths == T).all() and (scores == 0).all()
    for kw, match in [(dict(num_beams=0), "num_beams"), (dict(num_beams=9), "num_beams"),
                      (dict(max_new_tokens=-1), "max_new_tokens"), (dict(max_new_tokens=BS - T + 1), "block_size"),
                      (dict(pad_token=V), "pad_token"), (dict(pad_token=-1), "pad_token"),
                      (dict(eos_token=V), "eos_token"), (dict(eos_token=-1), "eos_token"),
                      (dict(idx=torch.tensor([[0, V]]).cuda()), "outside"),
                      (dict(idx=torch.tensor([[0, -1]]).cuda()), "outside"),
                      (dict(idx=torch.tensor([1, 2]).cuda()), "idx")]:
        args = dict(idx=idx, max_new_tokens=4, num_beams=2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            generate_beam(model, **args)
    full = model.generate_beam(idx[:1], BS - T, 2)  # the last column of the window
    assert full[0].shape == (1, 2, BS) and (full[1] == BS).all()
