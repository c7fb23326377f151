"""Per-token log-probabilities on the CPU: ``generate`` / ``generate_batch`` with
``return_logprobs=True`` and ``score``, against the rule restated in numpy float64
(tests/_logprob_oracle.py) on the logits of the model's own full forward over each prefix.

The model is fp32 here, so the cache path and the full forward agree to ~1e-6 on the logits and a
log-probability to twice that: the tolerance is 1e-5."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _logprob_oracle as L
from mingpt_distributed_amd.models import GPT, GPTConfig, generate, generate_batch, score
from mingpt_distributed_amd.ops import reference as R

V, BS = 1000, 64
LENS = [3, 9, 5, 1]
NEW = 10
TOL = 1e-5
SEEDED = dict(do_sample=True, top_k=20, top_p=0.9, temperature=0.7, seed=4321)
MODES = {"greedy": {}, "seeded": SEEDED}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=V, block_size=BS, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, V, (n,), generator=g) for n in LENS]


def want_lp(model, row):
    """The oracle's lp of row[j] given row[:j] for j >= 1, from ONE full forward over the row."""
    with torch.no_grad():
        logits = model(row.view(1, -1))[0][0].double().numpy()
    return L.logprob(logits[:-1], row[1:].numpy())


def check_rows(model, tokens, lengths, lp, starts):
    """lp [B, W] against the oracle at the generated positions starts[b] .. lengths[b] - 1 of every
    row, and exactly 0.0 everywhere else."""
    assert lp.shape == tokens.shape and lp.dtype == torch.float32
    for b in range(tokens.size(0)):
        n, s = int(lengths[b]), starts[b]
        want = want_lp(model, tokens[b, :n])
        got = lp[b].numpy()
        assert n > s and np.isfinite(got[s:n]).all() and (got[s:n] < 0).all(), f"row {b}"
        assert np.abs(got[s:n] - want[s - 1:]).max() <= TOL, f"row {b}: {got[s:n]} vs {want[s - 1:]}"
        assert (got[:s] == 0.0).all() and (got[n:] == 0.0).all(), f"row {b}: prompt / padding not 0.0"


@pytest.mark.parametrize("use_cache", [True, False], ids=["cache", "no_cache"])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate(model, mode, use_cache):
    kw = MODES[mode]
    idx = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(2))
    plain = generate(model, idx, NEW, use_cache=use_cache, **kw)
    tokens, lp = generate(model, idx, NEW, use_cache=use_cache, return_logprobs=True, **kw)
    assert torch.equal(tokens, plain)
    check_rows(model, tokens, [5 + NEW] * 2, lp, [5, 5])
    m_tokens, m_lp = model.generate(idx, NEW, use_cache=use_cache, return_logprobs=True, **kw)
    assert torch.equal(m_tokens, tokens) and torch.equal(m_lp, lp)
    assert torch.is_tensor(model.generate(idx, 2, use_cache=use_cache, **kw))  # the keyword's default


def test_generate_unseeded_and_empty(model):
    idx = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(5)
    plain = generate(model, idx, NEW, do_sample=True, top_k=10)
    torch.manual_seed(5)
    tokens, lp = generate(model, idx, NEW, do_sample=True, top_k=10, return_logprobs=True)
    assert torch.equal(tokens, plain)
    check_rows(model, tokens, [5 + NEW] * 2, lp, [5, 5])
    tokens, lp = generate(model, idx, 0, return_logprobs=True)
    assert torch.equal(tokens, idx) and lp.shape == idx.shape and (lp == 0.0).all()


def test_generate_past_the_window(model):
    """Past block_size the condition is the cropped window, as for the token itself."""
    idx = torch.randint(0, V, (1, BS - 2), generator=torch.Generator().manual_seed(3))
    tokens, lp = generate(model, idx, 5, return_logprobs=True)
    assert torch.equal(tokens, generate(model, idx, 5)) and lp.shape == (1, BS + 3)
    for j in range(BS - 2, BS + 3):
        with torch.no_grad():
            logits = model(tokens[:, max(0, j - BS):j])[0][0, -1].double().numpy()
        assert abs(float(lp[0, j]) - L.logprob(logits, int(tokens[0, j]))) <= TOL, j


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_batch_with_eos(model, prompts, mode):
    kw = MODES[mode]
    free, _ = generate_batch(model, prompts, NEW, **kw)
    eos = int(free[1, LENS[1] + 3])  # row 1's fourth generated token: row 1 stops there at the latest
    plain, plain_len = generate_batch(model, prompts, NEW, eos_token=eos, pad_token=7, **kw)
    tokens, lengths, lp = generate_batch(model, prompts, NEW, eos_token=eos, pad_token=7, return_logprobs=True, **kw)
    assert torch.equal(tokens, plain) and torch.equal(lengths, plain_len)
    assert int(lengths[1]) <= LENS[1] + 4 and int(tokens[1, lengths[1] - 1]) == eos
    assert float(lp[1, lengths[1] - 1]) < 0  # the stop token is a generated token and has its lp
    check_rows(model, tokens, lengths, lp, LENS)
    m = model.generate_batch(prompts, NEW, eos_token=eos, pad_token=7, return_logprobs=True, **kw)
    assert torch.equal(m[0], tokens) and torch.equal(m[1], lengths) and torch.equal(m[2], lp)
    # score of what was generated is the same number at every generated position
    sc = score(model, tokens, lengths)
    assert sc.shape == tokens.shape and sc.dtype == torch.float32
    for b, n0 in enumerate(LENS):
        n = int(lengths[b])
        assert (sc[b, n0:n] - lp[b, n0:n]).abs().max() <= TOL, f"row {b}"
        assert float(sc[b, 0]) == 0.0 and (sc[b, n:] == 0.0).all()
        assert np.abs(sc[b, 1:n].numpy() - want_lp(model, tokens[b, :n])).max() <= TOL
    listed = score(model, [tokens[b, :int(lengths[b])] for b in range(4)])
    assert (listed - sc[:, :int(lengths.max())]).abs().max() <= TOL
    assert torch.equal(model.score(tokens, lengths), sc) and torch.equal(score(model, (tokens, lengths)), sc)
    z = generate_batch(model, prompts, 0, return_logprobs=True)
    assert len(z) == 3 and z[2].shape == z[0].shape and (z[2] == 0.0).all()


def test_filters_leave_the_models_logprob(model):
    """Temperature, top-k and top-p change the tokens, not what a token's lp means: at T = 0.7 with
    top_k = 3 the lp is still the log-softmax of the unscaled, unfiltered logits."""
    idx = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(2))
    kw = dict(do_sample=True, seed=11)
    wide, _ = generate(model, idx, NEW, return_logprobs=True, **kw)
    tokens, lp = generate(model, idx, NEW, temperature=0.7, top_k=3, return_logprobs=True, **kw)
    assert not torch.equal(tokens, wide)
    check_rows(model, tokens, [5 + NEW] * 2, lp, [5, 5])
    # not the filtered distribution's: among 3 kept tokens the drawn one would often be above ln(1/3)
    assert (lp[:, 5:] < np.log(1 / 3)).all()


def test_score_is_minus_cross_entropy(model):
    idx = torch.randint(0, V, (3, 33), generator=torch.Generator().manual_seed(4))
    sc = score(model, idx)
    with torch.no_grad():
        logits = model(idx)[0]
    ce = F.cross_entropy(logits[:, :-1].reshape(-1, V), idx[:, 1:].reshape(-1), reduction="none").view(3, 32)
    assert sc.shape == (3, 33) and (sc[:, 0] == 0.0).all()
    assert (sc[:, 1:] + ce).abs().max() <= TOL
    assert np.abs(sc[0, 1:].numpy() - want_lp(model, idx[0])).max() <= TOL
    model.train()
    try:  # eval mode inside, the flag restored
        assert torch.equal(score(model, idx), sc) and model.training
    finally:
        model.eval()
    assert torch.equal(score(model, idx[:, :1]), torch.zeros(3, 1))


def test_token_logprob_reference():
    l = torch.tensor([[0.5, -1.0, float("-inf"), 2.0]])
    got = R.token_logprob(l, torch.tensor([[3]]))
    assert got.dtype == torch.float32 and got.shape == (1,)
    assert abs(float(got) - L.logprob(l.numpy(), np.array([3]))[0]) < 1e-7
    assert float(R.token_logprob(l, torch.tensor([2]))) == float("-inf")
    b = l.to(torch.bfloat16)  # a bf16 model: the rule on the rounded values
    assert abs(float(R.token_logprob(b, torch.tensor([1]))) - L.logprob(b.float().numpy(), np.array([1]))[0]) < 1e-7


def test_score_rejects(model):
    with pytest.raises(ValueError, match="block_size"):
        score(model, torch.zeros(1, BS + 1, dtype=torch.long))
    with pytest.raises(ValueError, match="token outside"):
        score(model, torch.tensor([[1, V, 2]]))
    with pytest.raises(ValueError, match="token outside"):
        score(model, [torch.tensor([1, -1])])
    with pytest.raises(ValueError, match="length"):
        score(model, torch.zeros(2, 4, dtype=torch.long), torch.tensor([4, 5]))
    # a bad id past a row's length is padding, not a token
    ok = score(model, torch.tensor([[1, 2, V + 5]]), torch.tensor([2]))
    assert ok.shape == (1, 3) and float(ok[0, 2]) == 0.0 and float(ok[0, 1]) < 0


def test_cli_flag(monkeypatch, capsys):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "projects", "generate",
                        "generate.py")
    spec = importlib.util.spec_from_file_location("generate_project_logprobs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = []
    real, real_batch = GPT.generate, GPT.generate_batch

    def one(self, *a, **kw):
        seen.append(("generate", kw.get("return_logprobs")))
        return real(self, *a, **kw)

    def many(self, *a, **kw):
        seen.append(("generate_batch", kw.get("return_logprobs")))
        return real_batch(self, *a, **kw)

    monkeypatch.setattr(GPT, "generate", one)
    monkeypatch.setattr(GPT, "generate_batch", many)
    base = ["--random-init", "--model-type", "gpt-micro", "--num-samples", "2", "--steps", "3", "--device", "cpu"]
    mod.main(base)
    assert "logprob" not in capsys.readouterr().out
    mod.main(base + ["--logprobs"])
    mod.main(base + ["--logprobs", "--prompt", "1 2 3", "--prompt", "4 5"])
    assert seen == [("generate", None), ("generate", True), ("generate_batch", True)]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[logprob ")]
    assert len(lines) == 2 + 4
    for ln in lines:
        words = ln.strip("[]").replace(",", "").split()  # logprob X over N tokens perplexity Y
        total, n, ppl = float(words[1]), int(words[3]), float(words[6])
        assert n == 3 and np.isfinite(total) and total < 0 and np.isfinite(ppl) and ppl > 1
