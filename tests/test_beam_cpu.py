"""``generate_beam`` on the CPU, the executable definition of beam search (the rule in common.h,
'Beam search'; ``ops.reference.beam_step`` on the KV-cache path), against an independent brute-force
search: explicit sequences, a full re-forward of ``model(idx)`` per step and a sort over all W * V
candidates in numpy float64."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig, generate_beam
from mingpt_distributed_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, BS, T, NEW = 96, 32, 4, 10
GAP = 1e-6  # the two paths' fp32 logits agree far better than this


def _model(vocab=V, seed=0):
    torch.manual_seed(seed)
    cfg = GPTConfig(model_type="gpt-nano", vocab_size=vocab, block_size=BS, embed_drop=0.0, resid_drop=0.0,
                    attn_drop=0.0)
    return GPT(cfg, verbose=False).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def idx():
    return torch.randint(0, V, (2, T), generator=torch.Generator().manual_seed(5))


def _logprobs(model, seqs):
    """fp64 log-softmax of the last position of every sequence (all of one length), full forward."""
    with torch.no_grad():
        logits, _ = model(torch.tensor(seqs, dtype=torch.long))
    l = logits[:, -1].double().numpy()
    m = l.max(-1, keepdims=True)
    return l - m - np.log(np.exp(l - m).sum(-1, keepdims=True))


def _brute(model, prompt, n, W, eos, pad):
    """Beam search on one prompt, nothing shared with the package: returns (tokens [W, n] padded,
    lengths [W], scores [W], the smallest gap between two candidates whose order mattered)."""
    beams = [(list(prompt), 0.0, False)]
    gap = np.inf
    for _ in range(n):
        live = [i for i, (_, _, f) in enumerate(beams) if not f]
        cands = []  # (c, beam, token)
        if live:
            width = max(len(beams[i][0]) for i in live)
            assert all(len(beams[i][0]) == width for i in live)
            lp = _logprobs(model, [beams[i][0] for i in live])
            for row, i in enumerate(live):
                cands += [(beams[i][1] + lp[row, t], i, t) for t in range(lp.shape[1])]
        cands += [(s, i, pad) for i, (_, s, f) in enumerate(beams) if f]
        cands.sort(key=lambda x: (-x[0], x[1], x[2]))
        for a, b in zip(cands[:W], cands[1:W + 1]):  # the order of the chosen, and the cut
            gap = min(gap, a[0] - b[0])
        new = []
        for c, i, t in cands[:W]:
            seq, _, f = beams[i]
            new.append((seq if f else seq + [t], c, f or (eos is not None and t == eos)))
        beams = new
    T0 = len(prompt)
    toks = np.full((W, n), pad, dtype=np.int64)
    for w, (seq, _, _) in enumerate(beams):
        toks[w, :len(seq) - T0] = seq[T0:]
    return toks, np.array([len(b[0]) for b in beams]), np.array([b[1] for b in beams]), gap


def _check(model, idx, W, eos, pad=3):
    tokens, lengths, scores = generate_beam(model, idx, NEW, W, eos_token=eos, pad_token=pad)
    B = idx.size(0)
    assert tokens.shape == (B, W, T + NEW) and tokens.dtype == torch.long
    assert lengths.shape == (B, W) and lengths.dtype == torch.long
    assert scores.shape == (B, W) and scores.dtype == torch.float32
    for b in range(B):
        toks, lens, sc, gap = _brute(model, idx[b].tolist(), NEW, W, eos, pad)
        assert gap > GAP, f"prompt {b}: a gap of {gap:.3g} decides the order: pick another seed"
        assert (tokens[b, :, :T] == idx[b]).all()
        assert np.array_equal(tokens[b, :, T:].numpy(), toks), f"prompt {b}"
        assert np.array_equal(lengths[b].numpy(), lens)
        np.testing.assert_allclose(scores[b].double().numpy(), sc, rtol=1e-5, atol=1e-5)
    return tokens, lengths, scores


@pytest.mark.parametrize("W", [1, 2, 5])
def test_equals_brute_force(model, idx, W):
    tokens, lengths, scores = _check(model, idx, W, None)
    assert (lengths == T + NEW).all()
    if W == 1:  # one beam is greedy decoding with its summed log-probability
        g, lp = model.generate(idx, NEW, return_logprobs=True)
        assert torch.equal(tokens[:, 0], g)
        torch.testing.assert_close(scores[:, 0], lp.sum(1), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("W", [1, 2, 5])
def test_equals_brute_force_with_stop_token(model, idx, W):
    free, _, _ = generate_beam(model, idx, NEW, W)
    eos = int(free[0, 0, T + 3])  # the best free-run beam's fourth token
    tokens, lengths, _ = _check(model, idx, W, eos)
    hit = [(b, w) for b in range(2) for w in range(W) if int(lengths[b, w]) < T + NEW]
    assert hit, "no beam stopped early: the stop token never came up"
    for b, w in hit:
        n = int(lengths[b, w])
        assert int(tokens[b, w, n - 1]) == eos and (tokens[b, w, n:] == 3).all()
        assert (tokens[b, w, T:n - 1] != eos).all()


def test_exhaustive_two_steps():
    """W = V = 7, two steps: the best beam is the argmax over all V * V continuations."""
    model = _model(vocab=7, seed=3)
    idx = torch.tensor([[1, 5, 2]])
    tokens, lengths, scores = generate_beam(model, idx, 2, 7)
    first = _logprobs(model, [idx[0].tolist()])[0]
    second = _logprobs(model, [idx[0].tolist() + [t] for t in range(7)])
    total = first[:, None] + second  # [first token, second token]
    a, b = np.unravel_index(np.argmax(total), total.shape)
    flat = np.sort(total.reshape(-1))[::-1]
    assert flat[0] - flat[1] > GAP
    assert tokens[0, 0, 3:].tolist() == [a, b] and abs(float(scores[0, 0]) - total[a, b]) < 1e-5
    # every beam's score is the sum of its own two steps, and no two beams are the same sequence
    for w in range(7):
        x, y = tokens[0, w, 3:].tolist()
        assert abs(float(scores[0, w]) - total[x, y]) < 1e-5
    assert len({tuple(t) for t in tokens[0, :, 3:].tolist()}) == 7
    assert (scores[0, :-1] >= scores[0, 1:]).all()


def test_length_penalty_reranks(model, idx):
    free, _, _ = generate_beam(model, idx, NEW, 5)
    eos = int(free[0, 0, T + 3])
    base = generate_beam(model, idx, NEW, 5, eos_token=eos)
    assert (base[2][:, :-1] >= base[2][:, 1:]).all()  # the search's own order: by score
    for a in (1.0, 3.0):
        tokens, lengths, scores = generate_beam(model, idx, NEW, 5, eos_token=eos, length_penalty=a)
        key = scores.double() / (lengths - T).clamp(min=1).double() ** a
        assert (key[:, :-1] >= key[:, 1:]).all()
        for b in range(2):
            order = torch.sort(base[2][b].double() / (base[1][b] - T).clamp(min=1).double() ** a,
                               descending=True, stable=True).indices
            assert torch.equal(tokens[b], base[0][b][order]) and torch.equal(lengths[b], base[1][b][order])
            assert torch.equal(scores[b], base[2][b][order])  # the raw sums, moved with their beams
    assert not torch.equal(generate_beam(model, idx, NEW, 5, eos_token=eos, length_penalty=3.0)[0], base[0])


def test_zero_new_tokens_and_arguments(model, idx):
    tokens, lengths, scores = generate_beam(model, idx, 0, 3)
    assert torch.equal(tokens, idx[:, None].expand(2, 3, T)) and (lengths == T).all() and (scores == 0).all()
    for kw, match in [(dict(num_beams=0), "num_beams"), (dict(num_beams=9), "num_beams"),
                      (dict(max_new_tokens=-1), "max_new_tokens"), (dict(max_new_tokens=BS), "block_size"),
                      (dict(pad_token=V), "pad_token"), (dict(eos_token=-1), "eos_token"),
                      (dict(idx=torch.tensor([[0, V]])), "outside"), (dict(idx=torch.tensor([1, 2])), "idx")]:
        args = dict(idx=idx, max_new_tokens=4, num_beams=2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            generate_beam(model, **args)
    with pytest.raises(ValueError, match="vocabulary"):
        generate_beam(_model(vocab=7), torch.tensor([[1]]), 2, 8)


def test_reference_step_ties():
    """``ops.reference.beam_step`` on hand-built ties: equal scores on identical rows take the
    lower beam first; a maximum at three indices comes in index order; a finished beam offers only
    the pad token at its frozen score; -inf logits are never chosen before a finite candidate."""
    l = torch.zeros(1, 2, 6)
    l[0, :, 4] = 2.0
    par, tok, sc, fin = R.beam_step(torch.tensor([[-1.0, -1.0]]), torch.zeros(1, 2, dtype=torch.bool), l)
    assert par.tolist() == [[0, 1]] and tok.tolist() == [[4, 4]] and sc[0, 0] == sc[0, 1]
    l = torch.zeros(1, 3, 6)
    l[0, :, [1, 3, 5]] = 1.0
    start = torch.tensor([[0.0, float("-inf"), float("-inf")]])
    par, tok, _, _ = R.beam_step(start, torch.zeros(1, 3, dtype=torch.bool), l)
    assert par.tolist() == [[0, 0, 0]] and tok.tolist() == [[1, 3, 5]]
    l = torch.tensor([3.0, 1.0, 0.0, 0.0, 0.0, 0.0]).expand(1, 3, 6)  # the second entry is 2 below the first
    lp = torch.log_softmax(l.double(), -1)
    s = torch.tensor([[-0.5, float(lp[0, 0].max()) - 0.5 - 0.3, -9.0]], dtype=torch.float64)
    par, tok, sc, fin = R.beam_step(s, torch.tensor([[False, True, False]]), l, eos_token=None, pad_token=2)
    assert par[0, 1] == 1 and tok[0, 1] == 2 and sc[0, 1] == s[0, 1] and bool(fin[0, 1]) and not bool(fin[0, 0])
    l = torch.full((1, 2, 6), float("-inf"))
    l[0, :, 0] = 0.0
    par, tok, sc, _ = R.beam_step(torch.tensor([[0.0, -1.0]]), torch.zeros(1, 2, dtype=torch.bool), l)
    assert par.tolist() == [[0, 1]] and tok.tolist() == [[0, 0]] and torch.isfinite(sc).all()


def test_project_beams_flag():
    spec = importlib.util.spec_from_file_location("generate", os.path.join(ROOT, "projects/generate/generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    outs = mod.main(["--random-init", "--model-type", "gpt-micro", "--beams", "3", "--length-penalty", "1.0",
                     "--steps", "4", "--device", "cpu"])
    assert len(outs) == 3
