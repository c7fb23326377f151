"""Speculative greedy decoding on the CPU: ``ops.reference.ngram_draft`` / ``spec_accept`` against the
rule restated in numpy integers (tests/_spec_oracle.py), hand cases for every clause of the draft,
the argument checks of ``generate_speculative``, and its CPU path -- the executable definition of the
semantics -- against CPU ``generate`` on a tiny model."""
import numpy as np
import pytest
import torch

import _spec_oracle as O
from mingpt_distributed_amd.models import GPT, GPTConfig, generate, generate_speculative
from mingpt_distributed_amd.ops import reference as R

V, BS = 96, 64
GAP = 1e-3  # the plain run's top-two logit gap below which the two paths may pick differently


def _model(seed=0):
    torch.manual_seed(seed)
    cfg = GPTConfig(model_type="gpt-nano", vocab_size=V, block_size=BS, embed_drop=0.0, resid_drop=0.0,
                    attn_drop=0.0)
    return GPT(cfg, verbose=False).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


def _positions(ngram):
    return sorted({0, 1, ngram - 1, ngram, 40, 63})


@pytest.mark.parametrize("alphabet", [3, 997], ids=["3-symbols", "997-symbols"])
@pytest.mark.parametrize("ngram", [1, 2, 3, 4])
def test_reference_draft_equals_oracle(alphabet, ngram):
    """Random sequences of 64 tokens over a 3-symbol alphabet (matches everywhere) and over 0..996
    (almost none), p in {0, 1, ngram - 1, ngram, 40, 63}, K in {2, 4, 8}."""
    rng = np.random.default_rng(alphabet * 10 + ngram)
    drafts = 0
    for trial in range(8):
        s = rng.integers(0, alphabet, 64)
        for p in _positions(ngram):
            for K in (2, 4, 8):
                rows, pos, has = O.draft(s, p, K, ngram)
                got, ghas = R.ngram_draft(torch.from_numpy(s), p, K, ngram)
                assert ghas == has and list(got) == rows.tolist(), (alphabet, ngram, trial, p, K)
                assert pos.tolist() == list(range(p, p + K))
                drafts += has
    assert drafts > 0 if alphabet == 3 else True


@pytest.mark.parametrize("K", [2, 4, 8])
def test_reference_accept_equals_oracle(K):
    """Random rows over a 2-symbol alphabet with the picks confirming a planted number of drafts and
    random after that (every acceptance length occurs), with and without a draft, ``end`` far,
    cutting the emission, and reached."""
    rng = np.random.default_rng(K)
    seen = set()
    for trial in range(400):
        rows, g = rng.integers(0, 2, K), rng.integers(0, 2, K)
        a = trial % K
        g[:a] = rows[1:a + 1]
        has = bool(rng.integers(0, 4))
        p = 20
        end = int(rng.choice([20, 21, 22, 20 + K, 60]))
        want = O.accept(rows, g, has, p, end)
        assert R.spec_accept(rows.tolist(), g.tolist(), has, p, end) == want
        seen.add(want[1])
    assert seen == set(range(K + 1))


def test_period_two_drafts_through_itself():
    """a b a b ... at K = 8: the best match ends two tokens back, so only x[e + 1], x[e + 2] are
    committed -- the draft goes on through its own tokens."""
    s = [7, 9] * 5  # p = 9, s[p] = 9
    for mod, name in ((R, "reference"), (O, "oracle")):
        rows, has = (mod.ngram_draft(s, 9, 8, 3) if mod is R else O.draft(s, 9, 8, 3)[::2])
        assert has and list(rows) == [9, 7, 9, 7, 9, 7, 9, 7], name


def test_most_recent_tie():
    """Two ends match the suffix (4, 5) to the same length with different continuations: the later
    one is drafted; a longer match further back beats both."""
    s = [4, 5, 1, 1, 4, 5, 2, 2, 4, 5]
    assert R.ngram_draft(s, 9, 3, 2) == ([5, 2, 2], True)
    assert O.draft(s, 9, 3, 2)[0].tolist() == [5, 2, 2]
    s = [3, 4, 5, 1, 0, 4, 5, 2, 3, 4, 5]  # ngram 3: (3, 4, 5) at e = 2 beats (4, 5) at e = 6
    assert R.ngram_draft(s, 10, 3, 3) == ([5, 1, 0], True)
    assert R.ngram_draft(s, 10, 3, 2) == ([5, 2, 3], True)
    assert O.draft(s, 10, 3, 3)[0].tolist() == [5, 1, 0] and O.draft(s, 10, 3, 2)[0].tolist() == [5, 2, 3]


def test_no_match():
    s = [1, 2, 3, 4, 5]
    assert R.ngram_draft(s, 4, 4, 3) == ([5, 5, 5, 5], False)
    rows, pos, has = O.draft(s, 4, 4, 3)
    assert rows.tolist() == [5, 5, 5, 5] and pos.tolist() == [4, 5, 6, 7] and not has
    assert R.ngram_draft([8], 0, 2, 1) == ([8, 8], False)  # p = 0: no candidate end
    # a row that happens to repeat s[p] is not accepted without a draft
    assert R.spec_accept([5, 5, 5, 5], [5, 5, 5, 5], False, 4, 30) == (0, 1)
    assert R.spec_accept([5, 5, 5, 5], [5, 5, 5, 5], True, 4, 30) == (3, 4)


def test_argument_errors(model):
    idx = torch.randint(0, V, (1, 6), generator=torch.Generator().manual_seed(1))
    bad = [({"idx": idx.int()}, "idx"), ({"idx": idx[0]}, "idx"), ({"max_new_tokens": -1}, "max_new_tokens"),
           ({"draft_len": 0}, "draft_len"), ({"draft_len": 8}, "draft_len"), ({"draft_len": 1.5}, "draft_len"),
           ({"ngram": 0}, "ngram"), ({"ngram": 5}, "ngram"), ({"max_new_tokens": BS - 5}, "max_new_tokens"),
           ({"idx": idx.repeat(3, 1), "draft_len": 3}, "draft_len"), ({"idx": idx + V}, "token")]
    for over, name in bad:
        args = {"idx": idx, "max_new_tokens": 4, **over}
        with pytest.raises(ValueError, match=name):
            generate_speculative(model, **args)
    generate_speculative(model, idx.repeat(4, 1), 2, draft_len=1)  # 4 * 2 rows: the limit
    generate_speculative(model, idx, BS - 6)                       # T + n == block_size


def _gap_free_length(model, full, T):
    """The number of leading generated columns of the plain run ``full`` [B, T + n] whose top-two
    logit gap is at least GAP in every row (teacher-forced full forward)."""
    with torch.no_grad():
        logits, _ = model(full[:, :-1])
    top = logits[:, T - 1:].double().topk(2, dim=-1).values
    small = ((top[..., 0] - top[..., 1]) < GAP).any(dim=0).nonzero()
    return int(small[0]) if small.numel() else full.size(1) - T


@pytest.mark.parametrize("B,draft_len,ngram,seed", [(1, 3, 3, 0), (1, 7, 3, 1), (2, 3, 2, 2), (4, 1, 1, 4),
                                                     (1, 1, 4, 0)], ids=lambda x: str(x))
def test_cpu_path_is_greedy(B, draft_len, ngram, seed):
    """``generate_speculative`` on the CPU against CPU ``generate`` (greedy), compared up to the first
    position whose top-two gap in the plain run is under 1e-3 -- none with these seeds -- and the
    statistics: every row's histogram adds up to n - 1 tokens in ``steps`` steps, and they are what the
    rule gives when simulated over the greedy sequence."""
    model = _model(seed)
    T, n, K = 7, 40, draft_len + 1
    g = torch.Generator().manual_seed(100 + seed)
    idx = torch.randint(0, V, (B, 5), generator=g).repeat(1, 2)[:, :T]  # 5-periodic prompts
    want = generate(model, idx, n)
    ok = _gap_free_length(model, want, T)
    assert ok == n, f"seed {seed}: a top-two gap under {GAP} at generated column {ok}; choose another seed"
    got, stats = generate_speculative(model, idx, n, draft_len=draft_len, ngram=ngram, return_stats=True)
    assert got.dtype == torch.long and torch.equal(got, want)
    assert torch.equal(got, model.generate_speculative(idx, n, draft_len=draft_len, ngram=ngram))
    steps, hist = stats["steps"], stats["emitted_hist"]
    assert steps.shape == (B,) and hist.shape == (B, K + 1)
    e = torch.arange(K + 1)
    assert torch.equal((hist * e).sum(1), torch.full((B,), n - 1)) and torch.equal(hist.sum(1), steps)
    assert (hist[:, 0] == 0).all()
    for b in range(B):
        s_steps, s_hist = O.simulate(want[b].numpy(), T, K, ngram)
        assert int(steps[b]) == s_steps and hist[b].tolist() == s_hist.tolist()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_cpu_short_runs(model, n):
    idx = torch.randint(0, V, (2, 6), generator=torch.Generator().manual_seed(9))
    got, stats = generate_speculative(model, idx, n, draft_len=2, return_stats=True)
    assert torch.equal(got, generate(model, idx, n))
    assert stats["steps"].tolist() == [max(n - 1, 0)] * 2
    assert stats["emitted_hist"].sum().item() == 2 * max(n - 1, 0)
