"""The logits processors on the CPU: ``ops.reference.process_logits`` against the rule restated in
numpy (tests/_process_oracle.py, which imports nothing from the package and is shared with the GPU
tests), the argument checks, and ``generate`` / ``generate_batch`` with the processors on."""
import numpy as np
import pytest
import torch

import _process_oracle as P
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.ops import reference as R

SETTINGS = {
    "repetition": dict(rp=1.3),
    "repetition_below_1": dict(rp=0.7),
    "presence": dict(pp=0.6),
    "frequency": dict(fp=0.37),
    "negative": dict(pp=-0.5, fp=-0.11),
    "ngram1": dict(g=1),
    "ngram2": dict(g=2),
    "ngram3": dict(g=3),
    "ngram8": dict(g=8),
    "all": dict(rp=1.7, pp=0.25, fp=0.13, g=2),
}
KW = dict(rp="repetition_penalty", pp="presence_penalty", fp="frequency_penalty", g="no_repeat_ngram_size")


def _kw(s):
    return {KW[k]: v for k, v in s.items()}


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def _rows(B, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    l = (torch.randn(B, V, generator=g) * 3.0).to(dtype)
    l[:, 1] = 0.0
    l[:, 2] = -0.0
    l[:, 3] = float("-inf")
    return l


def _model(block=16):
    torch.manual_seed(0)
    return GPT(GPTConfig(n_layer=2, n_head=2, n_embed=32, vocab_size=50, block_size=block), verbose=False).eval()


def test_oracle_by_hand():
    """The restatement itself on values worked out by hand (bf16: 1.5 = 0x3FC0, -2 = 0xC000)."""
    row = np.array([0x3FC0, 0xC000, 0x0000, 0xFF80, 0x3F80], dtype=np.uint16)
    out = P.process_row(row, [0, 1, 1, 3], rp=2.0)
    assert out.tolist() == [0x3F40, 0xC080, 0x0000, 0xFF80, 0x3F80]  # 0.75, -4, untouched, -inf, unseen
    out = P.process_row(row, [0, 1, 1], pp=0.5, fp=0.25)
    assert out.tolist() == [0x3F40, 0xC040, 0x0000, 0xFF80, 0x3F80]  # 1.5 - 0.75, -2 - 1
    assert P.process_row(row, [4, 0, 2, 4], g=2).tolist() == [0xFF80, 0xC000, 0x0000, 0xFF80, 0x3F80]
    assert P.process_row(row, [4, 0], g=3).tolist() == row.tolist()  # n < g
    assert P.process_row(row, [4, 0, 4], g=1).tolist() == [0xFF80, 0xC000, 0x0000, 0xFF80, 0xFF80]
    assert P.process_row(row, [7, -1, 0, 7, -1], g=3, V=5).tolist() == row.tolist()  # foreign ids match nothing
    assert P.f32_to_bf16(np.float32(1.00390625)) == 0x3F80 and P.f32_to_bf16(np.float32(1.01171875)) == 0x3F82
    assert P.no_repeat_holds([1, 2, 3, 1, 2, 4], 3, 3) and not P.no_repeat_holds([1, 2, 3, 1, 2, 3], 3, 3)
    assert P.no_repeat_holds([1, 2, 3, 9, 1, 2, 3], 4, 3, window=3)  # the earlier 3-gram left the window


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_reference_matches_oracle(name, dtype):
    """Bit for bit, each processor alone and all together, on histories of 1 .. 40 tokens over a
    small and a large alphabet, ids outside the vocabulary included."""
    s = SETTINGS[name]
    V, B = 61, 6
    logits = _rows(B, V, dtype, 3)
    for n, alpha in [(1, V), (2, 2), (7, 3), (40, 5), (40, V)]:
        g = torch.Generator().manual_seed(n * 100 + alpha)
        hist = torch.randint(0, alpha, (B, n), generator=g)
        hist[0] = hist[0, 0]  # all one token: c = n
        if n >= 7:
            hist[1, 2], hist[1, n - 1] = V + 3, -1
            hist[2, n - 2:] = torch.tensor([0, V - 1])
        got = R.process_logits(logits, hist, **_kw(s))
        assert got.dtype == dtype and got.shape == logits.shape
        want = P.process(_bits(logits), hist.tolist(), **s)
        assert np.array_equal(_bits(got), want), (name, n, alpha)
    assert torch.equal(logits, _rows(B, V, dtype, 3))  # the input is left as it was


def test_reference_off_is_identity():
    logits = _rows(4, 33, torch.bfloat16, 5)
    hist = torch.randint(0, 33, (4, 9))
    assert np.array_equal(_bits(R.process_logits(logits, hist)), _bits(logits))


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                                dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
                                dict(presence_penalty=float("nan")), dict(presence_penalty=float("inf")),
                                dict(frequency_penalty=float("-inf")), dict(frequency_penalty=float("nan")),
                                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9),
                                dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
                                dict(repetition_penalty=None)])
def test_argument_validation(kw):
    m = _model()
    idx = torch.randint(0, 50, (1, 4))
    with pytest.raises(ValueError):
        R.check_process_args(**kw)
    with pytest.raises(ValueError):
        m.generate(idx, 2, **kw)
    with pytest.raises(ValueError):
        m.generate_batch([idx[0]], 2, **kw)
    assert R.check_process_args() is False and R.check_process_args(no_repeat_ngram_size=8) is True
    assert R.check_process_args(repetition_penalty=1, presence_penalty=0) is False


def test_defaults_change_nothing():
    m = _model()
    idx = torch.randint(0, 50, (2, 5))
    off = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram_size=0)
    for kw in (dict(), dict(do_sample=True, seed=4, top_k=7), dict(use_cache=False), dict(return_logprobs=True)):
        a, b = m.generate(idx, 20, **kw), m.generate(idx, 20, **kw, **off)
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(x, y)
    rows = [idx[0], idx[1, :2]]
    for kw in (dict(), dict(do_sample=True, seed=4, top_p=0.9, return_logprobs=True)):
        for x, y in zip(m.generate_batch(rows, 9, **kw), m.generate_batch(rows, 9, **kw, **off)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("mode", ["greedy", "seeded", "global"])
def test_generate_follows_the_rule(mode, use_cache):
    """Every generated token's history is the context the model saw (block 16, 30 columns: the
    window slides): re-deriving the processed row from a full forward and the oracle, the produced
    token is its argmax (greedy), and the reported log-probability is the processed row's."""
    m = _model()
    s = SETTINGS["all"]
    idx = torch.randint(0, 50, (2, 4))
    kw = dict(greedy={}, seeded=dict(do_sample=True, seed=3, temperature=0.8),
              **{"global": dict(do_sample=True, top_k=6)})[mode]
    torch.manual_seed(1)
    out, lp = m.generate(idx, 26, use_cache=use_cache, return_logprobs=True, **kw, **_kw(s))
    assert P_holds(out, 4, s["g"], 16)
    checked = 0
    with torch.no_grad():
        for col in range(4, 30):
            ctx = out[:, max(0, col - 16):col]
            raw = m(ctx)[0][:, -1]
            want = torch.from_numpy(P.process(raw.numpy(), ctx.tolist(), **s))
            tok = out[:, col]
            assert torch.isfinite(want.gather(1, tok.view(-1, 1))).all()  # never a banned token
            top2 = want.topk(2, dim=-1).values
            ok = (top2[:, 0] - top2[:, 1]) > 1e-3  # the KV-cache path and the forward differ in rounding
            if mode == "greedy":
                assert torch.equal(tok[ok], want.argmax(-1)[ok])
                checked += int(ok.sum())
            ref = torch.log_softmax(want.double(), -1).gather(1, tok.view(-1, 1)).view(-1)
            assert torch.allclose(lp[:, col].double(), ref, atol=1e-3)
    assert mode != "greedy" or checked >= 40


def P_holds(out, start, g, window=None):
    return all(P.no_repeat_holds(r.tolist(), start, g, window) for r in out)


@pytest.mark.parametrize("g", [1, 2, 3])
def test_no_repeated_ngram(g):
    """A 6-symbol vocabulary repeats within a few tokens when left alone; with the ban on, no g-gram
    ending in a generated token occurs earlier in that token's history."""
    torch.manual_seed(0)
    m = GPT(GPTConfig(n_layer=1, n_head=2, n_embed=32, vocab_size=24, block_size=16), verbose=False).eval()
    idx = torch.randint(0, 24, (3, 3))
    n = 9 if g == 1 else 25  # g = 1 runs out of tokens: 24 symbols, a window of 16
    plain = m.generate(idx, n)
    assert not P_holds(plain, 3, max(g, 2), 16)  # greedy decoding loops on its own
    for kw in (dict(), dict(do_sample=True, seed=1), dict(use_cache=False)):
        out = m.generate(idx, n, no_repeat_ngram_size=g, **kw)
        assert P_holds(out, 3, g, 16), (g, kw)
    toks, lens = m.generate_batch([idx[0], idx[1, :1]], 10 if g > 1 else 9, no_repeat_ngram_size=g)
    for r, L, T0 in zip(toks, lens.tolist(), (3, 1)):
        assert P.no_repeat_holds(r[:L].tolist(), T0, g)


def test_generate_batch_rows_have_their_own_history():
    """Each row of a ragged batch equals ``generate`` on the row alone, processors on."""
    m = _model(block=32)
    s = _kw(SETTINGS["all"])
    rows = [torch.randint(0, 50, (n,)) for n in (1, 5, 11, 3)]
    for kw in (dict(), dict(do_sample=True, seed=9, temperature=0.9, top_k=12)):
        toks, lens, lp = m.generate_batch(rows, 12, return_logprobs=True, **kw, **s)
        for b, r in enumerate(rows):
            if kw and b:  # generate() draws for batch row 0; the ragged rule uses the row's own index
                continue
            one, one_lp = m.generate(r.view(1, -1), 12, return_logprobs=True, **kw, **s)
            n = r.numel() + 12
            assert int(lens[b]) == n and torch.equal(toks[b, :n], one[0])
            assert torch.allclose(lp[b, :n], one_lp[0], atol=1e-5)
    # pad and neighbours play no part: the same rows in another order and padding
    t2, l2 = m.generate_batch(rows[::-1], 12, pad_token=7, **s)
    t1, l1 = m.generate_batch(rows, 12, **s)
    for b in range(4):
        n = int(l1[b])
        assert torch.equal(t1[b, :n], t2[3 - b, :n])
