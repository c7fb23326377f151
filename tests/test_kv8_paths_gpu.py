"""``kv_cache="int8"`` on ``generate_beam``, ``generate_speculative`` and ``score``: the KV8 model of
``generate(kv_cache="int8")`` on every entry point that keeps or reads K/V.

* Beam and speculative calls run on int8 caches in states of their own (``_mg_beam_kv8_cache``,
  ``_mg_spec_kv8_cache``) through ``kv8_store(rep=W)``, ``attention_decode_kv8`` (grouped for the verify
  rows) and ``beam_reorder_kv8``, and with ``_KV8_DECODE`` off through the bf16 kernels on snapped rows:
  equal results and bit-equal stored logits either way.
* ``score(kv_cache="int8")`` is bit-equal to a prefill body built here whose ``keep`` overwrites the K/V
  thirds with the numpy oracle's s q.

The two 2-layer models of ``test_kv8_decode_gpu``: n_embed 128, n_head 2, vocab 1000 and 8200, block_size 96."""
import functools
import gc

import numpy as np
import pytest
import torch

import _kv8_oracle as O
from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

BS = 96
CONFIGS = {"v1000": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=1000, block_size=BS),
           "v8200": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=8200, block_size=BS)}
T, NEW, L = 12, 24, 2
SLOTS = ("_mg_decode_cache", "_mg_kv8_cache", "_mg_beam_cache", "_mg_beam_kv8_cache", "_mg_spec_cache",
         "_mg_spec_kv8_cache")
KERNELS = ("attention_decode", "attention_decode_kv8", "kv8_store", "beam_reorder", "beam_reorder_kv8")


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


def _build(name):
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, **CONFIGS[name])
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


_model = functools.lru_cache(maxsize=None)(_build)


def _idx(name, B, T=T, seed=1):
    g = torch.Generator().manual_seed(seed + B)
    return torch.randint(0, CONFIGS[name]["vocab_size"], (B, T), generator=g).cuda()


def _periodic(name, B, T, seed):
    """A random 5-token pattern repeated: the n-gram draft matches at once."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, CONFIGS[name]["vocab_size"], (B, 5), generator=g).repeat(1, T // 5 + 1)[:, :T].contiguous().cuda()


def _drop_states(model):
    for k in SLOTS:
        model.__dict__.pop(k, None)


def _run(model, fn, kv8, graph=True):
    """(fn(model)'s tensors, {(slot, loop): its stored logits}, launches per binding, the slots in use) on
    fresh decode states with ``_KV8_DECODE`` = ``kv8``."""
    C = ext()
    calls = {k: 0 for k in KERNELS}
    real = {k: getattr(C, k) for k in calls}

    def counted(k):
        def f(*a, **kw):
            calls[k] += 1
            return real[k](*a, **kw)
        return f

    _drop_states(model)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(gen, "_KV8_DECODE", kv8)
        mp.setattr(gen, "_GRAPH_DECODE", graph)
        for k in calls:
            mp.setattr(C, k, counted(k))
        out = fn(model)
    out = [o.clone() for o in (out if isinstance(out, (tuple, list)) else (out,)) if isinstance(o, torch.Tensor)]
    logits, slots = {}, []
    for k in SLOTS:
        c = model.__dict__.get(k)
        if c is not None:
            slots.append(k)
        for key, lp in (c._loops.items() if c is not None else ()):
            if lp.logits is not None:
                logits[(k, key)] = lp.logits.clone()
    _drop_states(model)
    return out, logits, calls, slots


def _same(a, b, what):
    assert len(a) == len(b) and len(a) >= 1
    for i, (x, y) in enumerate(zip(a, b)):
        assert bit_equal(x, y), f"{what}: output {i} differs"


# ------------------------------------------------------------------ beam search
def _beam_fn(idx, W, eos):
    """generate_beam's results and the device histories of the steps (columns T .. T + NEW - 1)."""
    def fn(m):
        tokens, lengths, scores = gen.generate_beam(m, idx, NEW, W, eos_token=eos, kv_cache="int8")
        st = m._mg_beam_kv8_cache.beam_state(W)
        return (tokens, lengths, scores) + tuple(st[k][:, :, T:T + NEW].clone() for k in ("hparent", "htok", "hscore"))
    return fn


@functools.lru_cache(maxsize=None)
def _eos_for(name, B, W):
    """A stop token that the free-run best beam of prompt 0 produces as its fourth token."""
    out, _, _, _ = _run(_model(name), _beam_fn(_idx(name, B), W, None), True)
    return int(out[0][0, 0, T + 3])


@pytest.mark.parametrize("stop", [False, True], ids=["free", "eos"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_beam_on_and_off(name, W, B, stop):
    model, idx = _model(name), _idx(name, B)
    eos = _eos_for(name, B, W) if stop else None
    fn = _beam_fn(idx, W, eos)
    on, lon, con, son = _run(model, fn, True)
    off, loff, coff, soff = _run(model, fn, False)
    _same(on, off, "attention_decode_kv8 / beam_reorder_kv8 against the bf16 kernels")
    key = ("_mg_beam_kv8_cache", ("beam", W))
    assert key in lon and set(lon) == set(loff) == {key} and bit_equal(lon[key], loff[key])
    assert son == soff == ["_mg_beam_kv8_cache"], "a KV8 beam call creates the KV8 beam state alone"
    # on: n_layer attention_decode_kv8 per step body and one beam_reorder_kv8 per tail (one more tail
    # follows the prefill), no bf16 decode or reorder; off: the reverse
    bodies = con["attention_decode_kv8"] // L
    assert bodies >= 1 and con["attention_decode_kv8"] == bodies * L and con["beam_reorder_kv8"] == bodies + 1, con
    assert con["attention_decode"] == 0 and con["beam_reorder"] == 0, con
    assert coff["attention_decode"] == bodies * L and coff["beam_reorder"] == bodies + 1, coff
    assert coff["attention_decode_kv8"] == 0 and coff["beam_reorder_kv8"] == 0, coff
    assert con["kv8_store"] == L and coff["kv8_store"] == (1 + bodies) * L, (con, coff)
    tokens, lengths, scores, hparent = on[0], on[1], on[2], on[3]
    assert tokens.shape == (B, W, T + NEW) and scores.dtype == torch.float32
    if W >= 3 and not stop:  # a run that never reorders shows nothing
        moved = (hparent != torch.arange(W, device="cuda").view(1, W, 1)).any(1)
        assert bool(moved[:, 1:].any()), "no step had a non-identity parent row: choose another seed"
    if stop:
        assert bool((tokens[:, :, T:] == eos).any()) and bool((lengths < T + NEW).any())
    # graph and eager, and a repeated call
    eager, leag, _, _ = _run(model, fn, True, graph=False)
    _same(on, eager, "graph against eager")
    assert bit_equal(lon[key], leag[key])
    twice, _, _, _ = _run(model, lambda m: (fn(m), fn(m))[1], True)
    _same(on, twice, "a repeated call")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_beam_is_kv8_greedy(name):
    model, idx = _model(name), _idx(name, 2)
    tokens, lengths, scores = gen.generate_beam(model, idx, NEW, 1, kv_cache="int8")
    g, lp = model.generate(idx, NEW, return_logprobs=True, kv_cache="int8")
    assert torch.equal(tokens[:, 0], g) and (lengths == T + NEW).all()
    lp = lp.cpu().numpy()
    for b in range(2):
        s = np.float32(0.0)
        for x in lp[b, T:]:
            s = np.float32(s + np.float32(x))
        assert np.float32(scores[b, 0].item()) == s, f"row {b}: {scores[b, 0].item()!r} vs {s!r}"
    _drop_states(model)


# ------------------------------------------------------------------ speculative decoding
SPEC_SHAPES = [(1, 4), (2, 4), (1, 8)]  # (B, K)


@functools.lru_cache(maxsize=None)
def _spec_case(name, B, K):
    """One case, run once: every check of the speculative path; returns the emitted histogram summed over
    the batch (kept, so the coverage test re-runs nothing)."""
    model = _model(name)
    idx = _periodic(name, B, T, seed=7 * B + K)

    def fn(m):
        out, stats = gen.generate_speculative(m, idx, NEW, draft_len=K - 1, return_stats=True, kv_cache="int8")
        return out, stats["steps"], stats["emitted_hist"]

    on, lon, con, son = _run(model, fn, True)
    off, loff, coff, soff = _run(model, fn, False)
    _same(on, off, "grouped attention_decode_kv8 against the bf16 kernels")
    key = ("_mg_spec_kv8_cache", ("spec", K))
    assert key in lon and set(lon) == set(loff) == {key} and bit_equal(lon[key], loff[key])
    assert son == soff == ["_mg_spec_kv8_cache"]
    assert con["attention_decode"] == 0 and con["attention_decode_kv8"] >= L and con["attention_decode_kv8"] % L == 0
    assert coff["attention_decode_kv8"] == 0 and coff["attention_decode"] == con["attention_decode_kv8"], (con, coff)
    want = model.generate(idx, NEW, kv_cache="int8")
    assert torch.equal(on[0], want), f"first difference at column {int((on[0] != want).any(0).nonzero()[0])}"
    hist = on[2].cpu()
    assert torch.equal((hist * torch.arange(K + 1)).sum(1), torch.full((B,), NEW - 1))
    _drop_states(model)
    return hist.sum(0)


@pytest.mark.parametrize("B,K", SPEC_SHAPES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_speculative_on_and_off(name, B, K):
    _spec_case(name, B, K)


def test_speculative_steps_of_both_kinds():
    """Over the cases some step emitted more than one token and some step rejected a draft (emitted
    fewer than K)."""
    many = few = 0
    for name in CONFIGS:
        for B, K in SPEC_SHAPES:
            hist = _spec_case(name, B, K)
            many += int(hist[2:].sum())
            few += int(hist[1:K].sum())
    assert many > 0 and few > 0, (many, few)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_speculative_to_the_last_cache_position(name):
    model = _model(name)
    n = 30
    idx = _periodic(name, 1, BS - n, seed=3)
    got = gen.generate_speculative(model, idx, n, draft_len=3, kv_cache="int8")
    assert got.shape == (1, BS) and torch.equal(got, model.generate(idx, n, kv_cache="int8"))
    _drop_states(model)


# ------------------------------------------------------------------ score
@pytest.mark.parametrize("name", list(CONFIGS))
def test_score_equals_a_body_snapped_by_the_oracle(name):
    model, cfg = _model(name), CONFIGS[name]
    D, H, V = cfg["n_embed"], cfg["n_head"], cfg["vocab_size"]
    B, Ts = 3, 20
    idx = _idx(name, B, T=Ts, seed=5)
    lengths = torch.tensor([Ts, 7, 13])
    got = gen.score(model, idx, lengths, kv_cache="int8")
    body = gen._Body(model)

    def keep(i, qkv):  # the K and V thirds through the numpy oracle
        kv = qkv[..., D:].float().cpu().numpy().reshape(*qkv.shape[:-1], 2 * H, D // H)
        qkv[..., D:].copy_(torch.from_numpy(O.snap(kv)[2]).to(torch.bfloat16).reshape(*qkv.shape[:-1], 2 * D))

    with torch.no_grad():
        padded = idx.clone()
        for b in range(B):
            padded[b, int(lengths[b]):] = 0  # score's own padding
        x = body._prompt(padded, keep).view(B * Ts, D)
        valid = torch.arange(1, Ts, device="cuda").view(1, -1) < lengths.cuda().view(B, 1)
        targets = torch.full((B, Ts), -1, dtype=torch.long, device="cuda")
        targets[:, :-1] = torch.where(valid, padded[:, 1:], targets[:, 1:])
        lp = torch.zeros(B * Ts, dtype=torch.float32, device="cuda")
        body.C.logits_lse(body._head(x, "mfma"), V, targets.view(-1), None, lp)
    want = torch.zeros(B, Ts, dtype=torch.float32, device="cuda")
    want[:, 1:] = lp.view(B, Ts)[:, :-1]
    assert bit_equal(got, want)
    assert not torch.equal(got, gen.score(model, idx, lengths)), "the KV8 model scores as the bf16 one everywhere"
    for b in range(B):
        assert (got[b, int(lengths[b]):] == 0).all() and got[b, 0] == 0 and (got[b, 1:int(lengths[b])] < 0).all()
    assert bit_equal(gen.score(model, idx, lengths, kv_cache="bf16"), gen.score(model, idx, lengths))


# ------------------------------------------------------------------ states, bytes, arguments
def test_kv_cache_nbytes_reports_the_new_states():
    model, cfg = _build("v1000"), CONFIGS["v1000"]
    D, H, B, W = cfg["n_embed"], cfg["n_head"], 2, 3
    gen.generate_beam(model, _idx("v1000", B), 4, W, kv_cache="int8")
    assert gen.kv_cache_nbytes(model) == {"_mg_beam_kv8_cache": L * B * W * BS * (2 * D + 8 * H)}
    gen.generate_beam(model, _idx("v1000", B), 4, W)
    gen.generate_speculative(model, _idx("v1000", 1), 4, kv_cache="int8")
    nb = gen.kv_cache_nbytes(model)
    assert nb == {"_mg_beam_cache": L * B * W * BS * 6 * D, "_mg_beam_kv8_cache": L * B * W * BS * (2 * D + 8 * H),
                  "_mg_spec_kv8_cache": L * BS * (2 * D + 8 * H)}
    assert nb["_mg_beam_kv8_cache"] * 6 * D == nb["_mg_beam_cache"] * (2 * D + 8 * H)


def test_the_bf16_states_are_left_alone():
    model, idx = _build("v1000"), _idx("v1000", 2)
    want = gen.generate_beam(model, idx, NEW, 3)
    state = model._mg_beam_cache
    loop = state._loops[("beam", 3)]
    gen.generate_beam(model, idx, NEW, 3, kv_cache="int8")
    assert model._mg_beam_cache is state and state._loops[("beam", 3)] is loop and not state.kv8
    assert model._mg_beam_kv8_cache.kv8 and model._mg_beam_kv8_cache.kqs is not None
    again = gen.generate_beam(model, idx, NEW, 3, kv_cache="bf16")
    assert all(torch.equal(a, b) for a, b in zip(want, again)) and state._loops[("beam", 3)].graph is loop.graph


def test_value_errors():
    model, idx = _model("v1000"), _idx("v1000", 1)
    with pytest.raises(ValueError):
        gen.generate_beam(model, idx, 2, 2, kv_cache="fp8")
    with pytest.raises(ValueError):
        gen.generate_speculative(model, idx, 2, kv_cache="fp8")
    with pytest.raises(ValueError):
        gen.score(model, idx, kv_cache="fp8")
