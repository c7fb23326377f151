"""The device decode loops at 9..64 rows, where every projection and the LM head run on the rows
GEMM (csrc/kernels/gemm_rows.hip) behind a LayerNorm launch: the route is taken; greedy ``generate``
is the argmax of its own logits, the same captured or eager; the logits are the B = 1 path's to
within the MFMA fallback's own distance from it; ``generate_batch`` is indifferent to the order of
its prompts; beam search on B * W > 8 rows scores what it says; and ``_ROWS_GEMM`` off restores the
fallback.  Models of 2 layers without dropout: "n128" (n_embed 128) and "w1280" (n_embed 1280: the
MLP output projection has K = 5120)."""
import functools
import gc

import numpy as np
import pytest
import torch

import _logprob_oracle as L
import _sample_oracle as O
from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops import reference as R
from mingpt_distributed_amd.ops._ext import ext

gpu = pytest.mark.gpu

BS = 96
CONFIGS = {"n128": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=1000, block_size=BS),
           "w1280": dict(n_layer=2, n_head=20, n_embed=1280, vocab_size=512, block_size=BS)}
CASES = [("n128", 9), ("n128", 16), ("n128", 33), ("n128", 64), ("w1280", 9)]
T, NEW = 12, 30
MARGIN = 1e-3
RAGGED_LENS = list(range(1, 32, 2))  # 16 prompts of 1, 3, .. 31 tokens
SEED, TEMP, TOPK = 5, 0.8, 20

# Check 3's allowance: twice the largest |logits difference| between the decode step on the MFMA
# GEMM fallback at B rows (what the parent commit ran; here ``_ROWS_GEMM`` off) and the rectangular
# B = 1 path (skinny GEMM) teacher-forced with the same tokens, over the cases of CASES for each
# model -- prompts of 12 tokens, 30 tokens per row (PERF.md 'Rows GEMM';
# test_fallback_distance_is_what_rows_diff_records measures them again and prints them):
#   n128   B = 9 / 16 / 33 / 64: 0.0078125 / 0.00390625 / 0.0078125 / 0.0078125 (logits std 0.22)
#   w1280  B = 9:                0.015625                                       (logits std 0.71)
ROWS_DIFF = {"n128": 0.0078125, "w1280": 0.015625}


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


@functools.lru_cache(maxsize=None)
def _model(name):
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, **CONFIGS[name])
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


def _idx(name, B, seed=1):
    g = torch.Generator().manual_seed(seed + B)
    return torch.randint(0, CONFIGS[name]["vocab_size"], (B, T), generator=g).cuda()


@functools.lru_cache(maxsize=None)
def _driven(name, B, rows_gemm=True):
    """The greedy loop one step per call on a state of its own: per produced token the logits the
    pick read (fp32, on the device), the input token and its position.  Computed once per case.
    ``rows_gemm`` False: with ``_ROWS_GEMM`` off, the parent commit's route (the MFMA GEMM)."""
    model, idx = _model(name), _idx(name, B)
    if not rows_gemm:
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(gen, "_ROWS_GEMM", False)
            return _driven.__wrapped__(name, B)
    with torch.no_grad():
        cache = gen._GpuCache(model, idx, BS)
        logits = cache.logits.float().clone()
        tok = logits.argmax(-1)
        rec = [dict(logits=logits, tok_in=None, pos_in=T - 1, tok_out=tok.clone())]
        for j in range(NEW - 1):
            new = cache.greedy(tok.view(B, 1), T + j, 1).reshape(B).clone()
            rec.append(dict(logits=cache._loops["greedy"].logits.float().clone(), tok_in=tok, pos_in=T + j,
                            tok_out=new))
            tok = new
    return idx, rec


# ------------------------------------------------------------------ 1. the route is taken
@gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_goes_through_the_rows_gemm(name, monkeypatch):
    """Without this, every other test here could pass on the MFMA fallback."""
    model, C = _model(name), ext()
    D = CONFIGS[name]["n_embed"]
    assert C.gemm_rows_supported(16, 4 * D) and not C.gemv_supported(16, 4 * D)
    widths, skinny = [], []
    real, real_gemv = C.gemm_rows, C.gemv

    def counted(x, *args, **kw):
        widths.append(x.size(-1))
        return real(x, *args, **kw)

    def counted_gemv(x, *args, **kw):
        skinny.append(x.size(-1))
        return real_gemv(x, *args, **kw)

    idx = _idx(name, 16)
    model.__dict__.pop("_mg_decode_cache", None)  # a fresh state: the step is built (and called) again
    monkeypatch.setattr(C, "gemm_rows", counted)
    monkeypatch.setattr(C, "gemv", counted_gemv)
    got = model.generate(idx, NEW)
    monkeypatch.undo()
    model.__dict__.pop("_mg_decode_cache", None)
    assert widths.count(4 * D) >= 1, f"no rows GEMM call on {4 * D} columns (widths seen: {sorted(set(widths))})"
    assert widths.count(D) >= 3 * widths.count(4 * D)  # qkv, attention projection, MLP in (and the LM head)
    assert not skinny
    assert got.shape == (16, T + NEW)


# ------------------------------------------------------------------ 2. greedy generate
@gpu
@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_greedy_graph_equals_eager_and_is_the_argmax(name, B, monkeypatch):
    model = _model(name)
    idx, rec = _driven(name, B)
    for j, r in enumerate(rec):
        assert torch.equal(r["tok_out"], r["logits"].argmax(-1)), f"step {j}"
    want = torch.cat([idx] + [r["tok_out"].view(B, 1) for r in rec], dim=1)
    model.__dict__.pop("_mg_decode_cache", None)
    a = model.generate(idx, NEW)
    graph = model._mg_decode_cache._loops["greedy"].graph
    b = model.generate(idx, NEW)  # replays the captured graph
    assert graph is not None and model._mg_decode_cache._loops["greedy"].graph is graph
    assert torch.equal(a, want), f"first difference at column {int((a != want).any(0).nonzero()[0])} (T = {T})"
    assert torch.equal(a, b)
    monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
    model.__dict__.pop("_mg_decode_cache", None)
    c = model.generate(idx, NEW)
    assert model._mg_decode_cache._loops["greedy"].graph is None
    assert torch.equal(a, c)
    model.__dict__.pop("_mg_decode_cache", None)  # an eager-built state has no graphs: start over


# ------------------------------------------------------------------ 3. logits against B = 1
def _b1_worst(model, idx, rec):
    """max |difference| between each row's logits in ``rec`` and the rectangular B = 1 path's,
    teacher-forced with the same tokens (test_generate_batch_gpu._check_logits's method)."""
    worst = torch.zeros((), device="cuda")
    ref = None
    with torch.no_grad():
        for b in range(idx.size(0)):
            p = idx[b:b + 1]
            if ref is None:
                ref = gen._GpuCache(model, p, BS)
            else:
                ref.prefill(p)
            worst = torch.maximum(worst, (ref.logits.float()[0] - rec[0]["logits"][b]).abs().max())
            for r in rec[1:]:
                l = ref.step(r["tok_in"][b].view(1, 1), r["pos_in"])
                worst = torch.maximum(worst, (l.float()[0] - r["logits"][b]).abs().max())
    return float(worst)


@gpu
@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_logits_match_rectangular_b1(name, B):
    """See ROWS_DIFF: the allowance is the fallback's own distance from the B = 1 path, doubled."""
    idx, rec = _driven(name, B)
    worst = _b1_worst(_model(name), idx, rec)
    print(f"{name} B = {B}: max |rows - B=1| logits difference {worst:.6g} (allowed {2 * ROWS_DIFF[name]:.6g}), "
          f"logits std {float(rec[-1]['logits'].std()):.3g}")
    assert worst <= 2 * ROWS_DIFF[name]


@gpu
@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_fallback_distance_is_what_rows_diff_records(name, B):
    """Where ROWS_DIFF comes from: the same drive with ``_ROWS_GEMM`` off (every projection on the
    MFMA GEMM, as on the parent commit) against the B = 1 path.  Printed per case; the recorded
    value is the largest over a model's cases, so none may exceed it."""
    idx, rec = _driven(name, B, False)
    worst = _b1_worst(_model(name), idx, rec)
    print(f"{name} B = {B}: max |MFMA fallback - B=1| logits difference {worst:.6g} (ROWS_DIFF {ROWS_DIFF[name]:.6g})")
    assert worst <= ROWS_DIFF[name]


# ------------------------------------------------------------------ 4. row permutation
def _prompts(lens, vocab=1000, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g) for n in lens]


def _drive_ragged(model, prompts, n, greedy):
    """test_generate_batch_gpu._drive at this file's seed: the ragged loop one step per call."""
    words = gen._ragged_words(SEED, TEMP, TOPK, None)
    B = len(prompts)
    idx = torch.zeros(B, max(p.numel() for p in prompts), dtype=torch.long, device="cuda")
    for b, p in enumerate(prompts):
        idx[b, :p.numel()] = p
    lens = torch.tensor([p.numel() for p in prompts])
    with torch.no_grad():
        cache = gen._GpuCache(model, idx, BS, last=lens.cuda() - 1)
        first = cache.logits.float().clone()
        st = cache.ragged_start(idx, lens.cuda(), words, greedy)
        rec = [dict(logits=first.cpu(), pos_in=lens - 1, tok_out=st["tok"].view(-1).cpu())]
        for _ in range(n):
            pos_in = st["pos"].cpu().long()
            cache.ragged(1, words, greedy)
            rec.append(dict(logits=cache._loops[("ragged", greedy)].logits.float().cpu(), pos_in=pos_in,
                            tok_out=st["tok"].view(-1).cpu()))
    return rec


@gpu
def test_greedy_batch_follows_a_permutation_of_its_prompts():
    model = _model("n128")
    prompts = [p.cuda() for p in _prompts(RAGGED_LENS)]
    tokens, lengths = generate_batch(model, prompts, NEW)
    perm = torch.randperm(len(prompts), generator=torch.Generator().manual_seed(2)).tolist()
    assert perm != sorted(perm)
    tokens2, lengths2 = generate_batch(model, [prompts[i] for i in perm], NEW)
    assert torch.equal(tokens2, tokens[perm]) and torch.equal(lengths2, lengths[perm])
    assert lengths.tolist() == [n + NEW for n in RAGGED_LENS]


@gpu
@pytest.mark.parametrize("order", ["given", "permuted"])
def test_seeded_batch_rows_follow_the_rule(order):
    """Every seeded token is the numpy restatement's pick from its own step's logits, with draw
    counter pos + 1 and b = the row's index in this call, wherever the fp64 top-two gap is at least
    1e-3; at most 4 % of the 496 draws (16 rows, the first pick and 30 steps) may fall under that
    margin (the existing ragged test's cap is 4 of 120).  With seed 5 the CPU path's fp32 logits put
    none there (test_seed_margin_on_cpu)."""
    model = _model("n128")
    prompts = [p.cuda() for p in _prompts(RAGGED_LENS)]
    if order == "permuted":
        perm = torch.randperm(len(prompts), generator=torch.Generator().manual_seed(2)).tolist()
        prompts = [prompts[i] for i in perm]
    rec = _drive_ragged(model, prompts, NEW, False)
    skipped = draws = 0
    for j, r in enumerate(rec):
        logits = r["logits"].numpy()
        for b in range(logits.shape[0]):
            want, gap = O.sample(logits[b:b + 1], TEMP, TOPK, SEED, int(r["pos_in"][b]) + 1, row0=b)
            draws += 1
            skipped += int(gap[0] < MARGIN)
            if gap[0] >= MARGIN:
                got = int(r["tok_out"][b])
                assert got == int(want[0]), f"step {j} row {b}: device {got}, rule {want[0]}, gap {gap[0]}"
    print(f"skipped {skipped} of {draws}")
    assert draws == 16 * (NEW + 1) and skipped <= 0.04 * draws
    tokens, _ = generate_batch(model, prompts, NEW + 1, do_sample=True, top_k=TOPK, temperature=TEMP, seed=SEED)
    for b, p in enumerate(prompts):
        n = p.numel()
        assert tokens[b, n:n + NEW + 1].tolist() == [int(r["tok_out"][b]) for r in rec], f"row {b}"


def test_seed_margin_on_cpu():
    """Seed 5 on the CPU path's fp32 logits: none of the 496 draws is under the margin."""
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, **CONFIGS["n128"])
    model = GPT(cfg, verbose=False).to(torch.bfloat16).float().eval()
    under = 0
    with torch.no_grad():
        for b, p in enumerate(_prompts(RAGGED_LENS)):
            cache = gen._CpuCache(model, p[None])
            logits, n = cache.logits, p.numel()
            for j in range(NEW + 1):
                tok, gap = O.sample(logits.numpy(), TEMP, TOPK, SEED, n, row0=b)
                under += int(gap[0] < MARGIN)
                logits = cache.step(torch.tensor([[int(tok[0])]]), n)
                n += 1
    print(f"draws under the margin on the CPU: {under} of {16 * (NEW + 1)}")
    assert under == 0


# ------------------------------------------------------------------ 5. beam search past 8 rows
def _teacher_forced(model, idx, tokens, n):
    """fp64 log-probabilities [rows, n] of ``tokens[:, T:T + n]`` on the logits of a second decode
    state fed the same tokens one by one (test_decode_wide_gpu._teacher_forced)."""
    out = []
    with torch.no_grad():
        ref = gen._GpuCache(model, idx, BS)
        logits = ref.logits
        for j in range(n):
            col = T + j
            out.append(R.token_logprob(logits, tokens[:, col]).double().cpu().numpy())
            if j + 1 < n:
                logits = ref.step(tokens[:, col:col + 1].contiguous(), col)
    return np.stack(out, axis=1)


@gpu
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("P,W", [(3, 4), (2, 8)], ids=["3x4", "2x8"])
def test_beams_past_8_rows(name, P, W):
    model, V = _model(name), CONFIGS[name]["vocab_size"]
    idx = _idx(name, P, seed=17)
    n = 20
    tokens, lengths, scores = model.generate_beam(idx, n, W)
    assert tokens.shape == (P, W, T + n) and (lengths == T + n).all() and scores.dtype == torch.float32
    assert torch.isfinite(scores).all() and (scores[:, :-1] >= scores[:, 1:]).all()
    again = model.generate_beam(idx, n, W)
    assert torch.equal(again[0], tokens) and torch.equal(again[1], lengths) and bit_equal(again[2], scores)
    # every beam's score is the sum of its tokens' log-probabilities: teacher-forced as P * W rows
    want = _teacher_forced(model, idx.repeat_interleave(W, 0), tokens.view(P * W, T + n), n)
    tol = L.tol(V, want).sum(1) + n * 2.0 ** -23 * np.abs(want).sum(1)  # n lp errors + n fp32 adds
    err = np.abs(scores.view(-1).double().cpu().numpy() - want.sum(1))
    print(f"worst beam-score error / allowed: {float((err / tol).max()):.3f}")
    assert (err <= tol).all()


# ------------------------------------------------------------------ 6. the switch
@gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_switch_off_restores_the_fallback(name, monkeypatch):
    """With ``_ROWS_GEMM`` off no rows GEMM is launched, and the tokens are the switched-on run's up
    to the first column where the fallback's two best logits are closer than 0.05
    (test_decode_wide_gpu.test_greedy_follows_the_uncached_reference's rule)."""
    model, C = _model(name), ext()
    idx, rec = _driven(name, 16)
    got = torch.cat([idx] + [r["tok_out"].view(-1, 1) for r in rec], dim=1)
    calls = []
    real = C.gemm_rows

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(gen, "_ROWS_GEMM", False)
    monkeypatch.setattr(C, "gemm_rows", counted)
    model.__dict__.pop("_mg_decode_cache", None)
    want = model.generate(idx, NEW)
    monkeypatch.undo()
    model.__dict__.pop("_mg_decode_cache", None)
    assert not calls
    agree = 0
    with torch.no_grad():
        for b in range(idx.size(0)):
            diff = (got[b] != want[b]).nonzero()
            col = int(diff[0]) if diff.numel() else T + NEW
            agree += col - T
            if diff.numel():
                top = model(want[b:b + 1, :col])[0][0, -1].float().topk(2).values
                gap = float(top[0] - top[1])
                print(f"row {b} leaves the fallback at column {col}: top-two gap {gap:.4f}")
                assert gap < 0.05, f"row {b} differs at column {col} where the fallback's gap is {gap:.4f}"
    print(f"{name}: {agree} of {idx.size(0) * NEW} tokens compared, all equal")
