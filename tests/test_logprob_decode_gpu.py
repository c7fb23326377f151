"""Log-probabilities through the decode path on the GPU: the device loops with the lse kernel inside
the captured step (``"greedy_lp"``, ``"sample_lp"``, ``("ragged_lp", greedy)``), the prefill-picked
first token, ``generate`` / ``generate_batch`` with ``return_logprobs=True`` and ``score``, against
the rule restated in numpy float64 (tests/_logprob_oracle.py) on the very bf16 logits each step
produced.  Tolerance: four times the bound derived in common.h (``L.tol``), unless stated."""
import gc

import numpy as np
import pytest
import torch

import _logprob_oracle as L
from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig, score
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

BS = 64
SEEDED = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.9, seed=1234567)
MODES = {"greedy": {}, "seeded": SEEDED}
LENS = [5, 17, 9]


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


def _model(vocab):
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=vocab, block_size=BS, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


@pytest.fixture(scope="module", params=[9000, 1000], ids=["9000-fused-argmax", "1000"])
def setup(request):
    """(model, idx [2, 5], V, a second model with the same weights for one-row runs)."""
    V = request.param
    idx = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(V)).cuda()
    return _model(V), idx, V, _model(V)


def _rows(V):
    g = torch.Generator().manual_seed(V + 1)
    return [torch.randint(0, V, (n,), generator=g).cuda() for n in LENS]


@pytest.mark.parametrize("mode", list(MODES))
def test_teacher_forced_parity(setup, mode):
    """The prefill's token and 30 device-loop tokens with their lp, then the same tokens fed one by
    one through the logits step of a second decode state (same kernels, so the same bf16 logits):
    every lp is the oracle's number on its step's logits, at all 2 x 31 tokens."""
    model, idx, V, _ = setup
    T0, n = idx.size(1), 31
    tokens, lp = model.generate(idx, n, return_logprobs=True, **MODES[mode])
    assert tokens.shape == lp.shape == (2, T0 + n) and (lp[:, :T0] == 0.0).all()
    got = lp.cpu().numpy().astype(np.float64)
    worst = 0.0
    with torch.no_grad():
        ref = gen._GpuCache(model, idx, BS)
        logits = ref.logits
        for j in range(n):
            col = T0 + j
            want = L.logprob(logits.float().cpu().numpy(), tokens[:, col].cpu().numpy())
            err, tol = np.abs(got[:, col] - want), L.tol(V, want)
            assert (err <= tol).all(), f"column {col}: device {got[:, col]}, rule {want}, allowed {tol}"
            worst = max(worst, float((err / tol).max()))
            if not MODES[mode]:  # greedy: the token is at the row maximum
                assert (tokens[:, col] == logits.float().argmax(-1)).all()
            if j + 1 < n:
                logits = ref.step(tokens[:, col:col + 1].contiguous(), col)
    print(f"worst error {worst:.3f} of the allowed")


@pytest.mark.parametrize("mode", list(MODES))
def test_tokens_unchanged_graph_eager_repeat(setup, mode, monkeypatch):
    """With the keyword the tokens are those without it; an eager run gives the same tokens and lp,
    bit for bit, as the captured one; a second call repeats both."""
    model, idx, V, _ = setup
    kw = MODES[mode]
    plain = model.generate(idx, 40, **kw)
    a = model.generate(idx, 40, return_logprobs=True, **kw)
    assert torch.equal(a[0], plain) and a[1].dtype == torch.float32
    assert (a[1][:, 5:] < 0).all() and torch.isfinite(a[1]).all()
    b = model.generate(idx, 40, return_logprobs=True, **kw)
    assert torch.equal(a[0], b[0]) and bit_equal(a[1], b[1])
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_decode_cache", None)
    c = model.generate(idx, 40, return_logprobs=True, **kw)
    assert torch.equal(a[0], c[0]) and bit_equal(a[1], c[1])
    monkeypatch.setattr(gen, "_GRAPH_DECODE", True)
    model.__dict__.pop("_mg_decode_cache", None)  # an eager-built state has no graphs: start over
    rows = _rows(V)
    free, _ = model.generate_batch(rows, 20, **kw)
    eos = int(free[1, LENS[1] + 3])
    want = model.generate_batch(rows, 20, eos_token=eos, **kw)
    got = model.generate_batch(rows, 20, eos_token=eos, return_logprobs=True, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    again = model.generate_batch(rows, 20, eos_token=eos, return_logprobs=True, **kw)
    assert torch.equal(got[0], again[0]) and bit_equal(got[2], again[2])
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_decode_cache", None)
    eager = model.generate_batch(rows, 20, eos_token=eos, return_logprobs=True, **kw)
    assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1]) and bit_equal(got[2], eager[2])
    model.__dict__.pop("_mg_decode_cache", None)


def test_plain_loops_intact(setup):
    """The plain loops' graph objects survive logprob calls, which live under keys of their own."""
    model, idx, V, _ = setup
    rows = _rows(V)
    model.__dict__.pop("_mg_decode_cache", None)
    g0 = model.generate(idx, 30)
    s0 = model.generate(idx, 30, **SEEDED)
    graphs = {k: model._mg_decode_cache._loops[k].graph for k in ("greedy", "sample")}
    model.generate(idx, 30, return_logprobs=True)
    model.generate(idx, 30, return_logprobs=True, **SEEDED)
    loops = model._mg_decode_cache._loops
    assert set(loops) == {"greedy", "sample", "greedy_lp", "sample_lp"}
    assert all(loops[k].graph is g and g is not None for k, g in graphs.items())
    assert torch.equal(model.generate(idx, 30), g0) and torch.equal(model.generate(idx, 30, **SEEDED), s0)
    assert all(loops[k].graph is g for k, g in graphs.items())
    r0 = model.generate_batch(rows, 20)  # B = 3: a new decode state
    r1 = model.generate_batch(rows, 20, **SEEDED)
    loops = model._mg_decode_cache._loops
    graphs = {k: loops[k].graph for k in (("ragged", True), ("ragged", False))}
    assert "lp" not in model._mg_decode_cache.ragged_state()
    model.generate_batch(rows, 20, return_logprobs=True)
    model.generate_batch(rows, 20, return_logprobs=True, **SEEDED)
    assert set(loops) == {("ragged", True), ("ragged", False), ("ragged_lp", True), ("ragged_lp", False)}
    assert all(loops[k].graph is g and g is not None for k, g in graphs.items())
    assert torch.equal(model.generate_batch(rows, 20)[0], r0[0])
    assert torch.equal(model.generate_batch(rows, 20, **SEEDED)[0], r1[0])
    assert all(loops[k].graph is g for k, g in graphs.items())


@pytest.mark.parametrize("mode", list(MODES))
def test_ragged_rows_equal_single_rows(setup, mode):
    """Lengths 5 / 17 / 9 with a stop token: row b's lp is what ``generate`` on row b alone gives, bit
    for bit, as far as the two runs' tokens agree (this model's ragged and one-row logits are
    equal, test_generate_batch_gpu.py RECT_DIFF; a seeded row b > 0 draws with its own row index,
    so only its first tokens may agree), and 0.0 at prompt and padding positions."""
    model, _, V, solo = setup
    kw = MODES[mode]
    rows, n = _rows(V), 24
    free, _ = model.generate_batch(rows, n, **kw)
    eos = int(free[1, LENS[1] + 3])
    tokens, lengths, lp = model.generate_batch(rows, n, eos_token=eos, pad_token=3, return_logprobs=True, **kw)
    assert lp.shape == tokens.shape == (3, max(LENS) + n) and lp.dtype == torch.float32
    assert int(lengths[1]) <= LENS[1] + 4 and int(tokens[1, lengths[1] - 1]) == eos
    for b, r in enumerate(rows):
        n0, n1 = r.numel(), int(lengths[b])
        assert (lp[b, :n0] == 0.0).all() and (lp[b, n1:] == 0.0).all()
        assert (lp[b, n0:n1] < 0).all() and torch.isfinite(lp[b, n0:n1]).all()  # the stop token included
        one, one_lp = solo.generate(r[None], n1 - n0, return_logprobs=True, **kw)
        same = (one[0, n0:n1] == tokens[b, n0:n1]).long().cumprod(0).bool()
        if not kw or b == 0:
            assert same.all(), f"row {b}: tokens differ from the row alone"
        assert bit_equal(lp[b, n0:n1][same], one_lp[0, n0:n1][same]), f"row {b}"


def test_past_the_window(setup):
    model, idx, V, _ = setup
    for kw in MODES.values():
        tokens, lp = model.generate(idx, 90, return_logprobs=True, **kw)
        assert tokens.shape == lp.shape == (2, 95) and torch.equal(tokens, model.generate(idx, 90, **kw))
        assert (lp[:, :5] == 0.0).all() and torch.isfinite(lp).all() and (lp[:, 5:] < 0).all()
        again = model.generate(idx, 90, return_logprobs=True, **kw)
        assert torch.equal(again[0], tokens) and bit_equal(again[1], lp)


def test_score_against_decode(setup):
    """``score`` of what ``generate_batch`` produced against the decode loop's lp.  The two differ
    only through the logits: score runs the MFMA prefill, decode the skinny GEMM, for which the
    project's tolerance is atol = rtol = 2e-2 on logits (test_generate_batch_gpu.py).  Shifting
    every logit of a row by at most eps moves a log-softmax entry by at most 2 eps, so the
    tolerance is 2 * (2e-2 + 2e-2 * max |logit|) of the row."""
    model, _, V, _ = setup
    rows = _rows(V)
    tokens, lengths, lp = model.generate_batch(rows, 24, return_logprobs=True, **SEEDED)
    sc = model.score(tokens, lengths)
    assert sc.shape == tokens.shape and sc.dtype == torch.float32 and (sc[:, 0] == 0.0).all()
    with torch.no_grad():
        big = model(tokens)[0].float().abs().amax(-1)  # [B, W]: row (b, j - 1) predicts column j
    for b, n0 in enumerate(LENS):
        n1 = int(lengths[b])
        tol = 2 * (2e-2 + 2e-2 * big[b, n0 - 1:n1 - 1])
        err = (sc[b, n0:n1] - lp[b, n0:n1]).abs()
        print(f"row {b}: max |score - decode| {float(err.max()):.4g}, allowed {float(tol.min()):.4g}")
        assert (err <= tol).all()
        assert (sc[b, n1:] == 0.0).all() and (sc[b, 1:n1] < 0).all()


def test_score_against_own_logits(setup, monkeypatch):
    """``score`` at B = 2, T = 64 against the oracle on ``model(idx)``'s own logits (the same
    kernels on the same rows, so the same bf16 values) within the kernel bound; once more with a
    cap of 40 rows of logits per LM-head chunk (four chunks, the last one short): bit-equal."""
    model, _, V, _ = setup
    idx = torch.randint(0, V, (2, BS), generator=torch.Generator().manual_seed(9)).cuda()
    lengths = torch.tensor([BS, 41])
    sc = score(model, idx, lengths)
    with torch.no_grad():
        logits = model(idx)[0].float().cpu().numpy().astype(np.float64)
    want = L.logprob(logits[:, :-1], idx[:, 1:].cpu().numpy())
    got = sc.cpu().numpy().astype(np.float64)
    for b, n in enumerate(lengths.tolist()):
        err, tol = np.abs(got[b, 1:n] - want[b, :n - 1]), L.tol(V, want[b, :n - 1])
        assert (err <= tol).all(), f"row {b}: worst {float((err / tol).max()):.3f} of the allowed"
        assert got[b, 0] == 0.0 and (got[b, n:] == 0.0).all()
    monkeypatch.setattr(gen, "_SCORE_LOGITS_BYTES", 40 * 2 * ((V + 7) // 8 * 8))
    assert bit_equal(score(model, idx, lengths), sc)
    with pytest.raises(ValueError, match="block_size"):
        score(model, torch.zeros(1, BS + 1, dtype=torch.long, device="cuda"))
    with pytest.raises(ValueError, match="token outside"):
        score(model, torch.tensor([[1, V]], device="cuda"))
