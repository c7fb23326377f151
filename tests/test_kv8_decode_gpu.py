"""KV8 decode: ``kv_cache="int8"`` runs every device decode loop on ``attention_decode_kv8`` over int8
caches (csrc/kernels/attention_kv8.hip) and produces what the same KV8 model produces on the bf16 kernels
(``_KV8_DECODE`` off: bf16 caches holding snapped rows, ``kv8_store`` in place, ``attention_decode``) --
equal tokens and bit-equal stored logits, in every decode mode -- and what a step body built in this file
from the numpy oracle and ``attention_decode`` produces.  Models of 2 layers without dropout: "v1000"
(torch argmax) and "v8200" (the wide LM head with the fused argmax), block_size 96."""
import functools
import gc

import pytest
import torch

import _kv8_oracle as O
from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

BS = 96
CONFIGS = {"v1000": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=1000, block_size=BS),
           "v8200": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=8200, block_size=BS)}
T, NEW, L = 12, 24, 2
CACHES = ("_mg_decode_cache", "_mg_kv8_cache")
KERNELS = ("attention_decode", "attention_decode_kv8", "kv8_store")


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


def _drop_states(model):
    for k in CACHES:
        model.__dict__.pop(k, None)


def _run(model, fn, kv8, graph=True):
    """(fn(model)'s tensors, {(state, loop): its stored logits}, launches per binding) on fresh decode
    states with ``_KV8_DECODE`` = ``kv8``."""
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
    logits = {}
    for k in CACHES:
        c = model.__dict__.get(k)
        for key, lp in (c._loops.items() if c is not None else ()):
            if lp.logits is not None:
                logits[(k, key)] = lp.logits.clone()
    _drop_states(model)
    return out, logits, calls


def _check_on_off(model, fn, loop, graph=True):
    """``fn`` with the switch on and off: equal outputs, bit-equal stored logits of ``loop``.  On, every
    step body launches n_layer attention_decode_kv8 and no attention_decode; off, the reverse."""
    on, lon, con = _run(model, fn, True, graph)
    off, loff, coff = _run(model, fn, False, graph)
    loop = ("_mg_kv8_cache", loop)
    assert loop in lon and set(lon) == set(loff), (sorted(map(str, lon)), sorted(map(str, loff)))
    assert all(k[0] == "_mg_kv8_cache" for k in lon)
    bodies = coff["attention_decode"] // L
    assert bodies >= 1 and coff["attention_decode"] == bodies * L and coff["attention_decode_kv8"] == 0, coff
    assert con["attention_decode_kv8"] == bodies * L and con["attention_decode"] == 0, (con, coff)
    prefills = con["kv8_store"] // L  # on: the prefills' stores alone; off: one more per layer and step body
    assert prefills >= 1 and con["kv8_store"] == prefills * L and coff["kv8_store"] == (prefills + bodies) * L, (con, coff)
    assert len(on) == len(off) and len(on) >= 1
    for a, b in zip(on, off):
        assert bit_equal(a, b), "outputs differ between attention_decode_kv8 and attention_decode"
    for k in lon:
        assert bit_equal(lon[k], loff[k]), f"stored logits of loop {k} differ"
    return on


# ------------------------------------------------------------------ 1. on and off: the same bits
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_greedy(name, graph):
    idx = _idx(name, 2)
    on = _check_on_off(_model(name), lambda m: m.generate(idx, NEW, kv_cache="int8"), "greedy", graph)
    assert on[0].shape == (2, T + NEW)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_graph_against_eager(name):
    idx = _idx(name, 2)
    fn = lambda m: m.generate(idx, NEW, kv_cache="int8", return_logprobs=True)
    g, lg, _ = _run(_model(name), fn, True, True)
    e, le, _ = _run(_model(name), fn, True, False)
    assert all(bit_equal(a, b) for a, b in zip(g, e)) and set(lg) == set(le)
    assert all(bit_equal(lg[k], le[k]) for k in lg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_greedy_sixteen_rows(name):
    """16 rows: the rows GEMM route, and 32 (b, h) pairs."""
    idx = _idx(name, 16)
    on = _check_on_off(_model(name), lambda m: m.generate(idx, NEW, kv_cache="int8"), "greedy")
    assert on[0].shape == (16, T + NEW)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_seeded_sampling_top_k_top_p(name):
    idx = _idx(name, 2)
    _check_on_off(_model(name), lambda m: m.generate(idx, NEW, temperature=0.8, do_sample=True, top_k=20, top_p=0.9,
                                                      seed=5, kv_cache="int8"), "sample")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_logprobs(name):
    idx = _idx(name, 2)
    on = _check_on_off(_model(name), lambda m: m.generate(idx, NEW, return_logprobs=True, kv_cache="int8"), "greedy_lp")
    assert len(on) == 2 and on[1].dtype == torch.float32


@pytest.mark.parametrize("name", list(CONFIGS))
def test_logits_processor(name):
    idx = _idx(name, 2)
    _check_on_off(_model(name), lambda m: m.generate(idx, NEW, repetition_penalty=1.3, no_repeat_ngram_size=3,
                                                      kv_cache="int8"), "greedy_proc")


def test_unseeded_sampling_steps_from_the_host():
    """``seed=None``: the host loop over ``step()``, torch's generator seeded by the test."""
    idx = _idx("v1000", 2)

    def fn(m):
        torch.manual_seed(5)
        return m.generate(idx, 10, do_sample=True, top_k=20, kv_cache="int8")

    _check_on_off(_model("v1000"), fn, "step")


@pytest.mark.parametrize("B", [2, 16])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_ragged_batch_greedy(name, B):
    g = torch.Generator().manual_seed(3)
    lens = [(1, 7, 3, 12, 2, 9, 5, 4)[b % 8] for b in range(B)]
    prompts = [torch.randint(0, CONFIGS[name]["vocab_size"], (n,), generator=g).cuda() for n in lens]
    on = _check_on_off(_model(name), lambda m: generate_batch(m, prompts, NEW, kv_cache="int8"), ("ragged", True))
    assert on[1].tolist() == [n + NEW for n in lens]


def test_ragged_batch_seeded_with_a_stop_token():
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(0, 1000, (n,), generator=g).cuda() for n in (5, 1, 8)]
    fn = lambda m: m.generate_batch(prompts, NEW, do_sample=True, seed=9, top_k=5, temperature=1.5, eos_token=3,
                                    pad_token=1, kv_cache="int8", return_logprobs=True)
    _check_on_off(_model("v1000"), fn, ("ragged_lp", False))
    fn = lambda m: m.generate_batch(prompts, NEW, eos_token=3, kv_cache="int8")
    _check_on_off(_model("v1000"), fn, ("ragged", True))


def test_window_slide():
    """T + n > block_size: a prefill per window past the end (each through kv8_store), then nothing to loop."""
    idx = _idx("v8200", 2, T=80)
    on = _check_on_off(_model("v8200"), lambda m: m.generate(idx, 30, kv_cache="int8"), "greedy")
    assert on[0].shape == (2, 110) and 110 > BS


# ------------------------------------------------------------------ 2. which kernels run
def test_bf16_calls_neither_new_binding_and_keeps_its_state():
    model = _model("v8200")
    idx = _idx("v8200", 2)
    out, _, calls = _run(model, lambda m: m.generate(idx, NEW, kv_cache="bf16"), True)
    assert calls["attention_decode_kv8"] == 0 and calls["kv8_store"] == 0 and calls["attention_decode"] >= L
    plain, _, _ = _run(model, lambda m: m.generate(idx, NEW), True)
    assert bit_equal(out[0], plain[0])
    want = model.generate(idx, NEW)
    state = model._mg_decode_cache
    model.generate(idx, NEW, kv_cache="int8")
    kv8 = model._mg_kv8_cache
    assert kv8 is not state and kv8.kv8 and not state.kv8
    assert torch.equal(model.generate(idx, NEW), want) and model._mg_decode_cache is state
    model.generate(idx, NEW, kv_cache="int8")
    assert model._mg_kv8_cache is kv8
    _drop_states(model)


def test_flipping_the_switch_never_replays_the_other_kernels_graph(monkeypatch):
    """One KV8 state kept across the flips: each flip swaps the caches and drops the captured loops, so
    the step body is called again (warm-up and capture) on the kernel the switch names."""
    model, C = _build("v8200"), ext()
    idx = _idx("v8200", 2)
    calls = {k: 0 for k in KERNELS}
    for k in calls:
        def counted(*a, _k=k, _real=getattr(C, k), **kw):
            calls[_k] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(C, k, counted)
    monkeypatch.setattr(gen, "_KV8_DECODE", True)
    want = model.generate(idx, NEW, kv_cache="int8")
    state = model._mg_kv8_cache
    n = calls["attention_decode_kv8"]  # the warm-up and the capture: whole step bodies
    assert calls["attention_decode"] == 0 and n >= L and n % L == 0
    assert state.kq and not state.caches
    assert torch.equal(model.generate(idx, NEW, kv_cache="int8"), want) and calls["attention_decode_kv8"] == n
    monkeypatch.setattr(gen, "_KV8_DECODE", False)
    assert torch.equal(model.generate(idx, NEW, kv_cache="int8"), want) and model._mg_kv8_cache is state
    assert calls["attention_decode"] == n and calls["attention_decode_kv8"] == n
    assert state.caches and not state.kq
    monkeypatch.setattr(gen, "_KV8_DECODE", True)
    assert torch.equal(model.generate(idx, NEW, kv_cache="int8"), want)
    assert calls["attention_decode"] == n and calls["attention_decode_kv8"] == 2 * n


def test_kv_cache_nbytes():
    model = _build("v1000")
    cfg = CONFIGS["v1000"]
    D, H, B = cfg["n_embed"], cfg["n_head"], 3
    assert gen.kv_cache_nbytes(model) == {}
    model.generate(_idx("v1000", B), 4, kv_cache="int8")
    assert gen.kv_cache_nbytes(model) == {"_mg_kv8_cache": L * B * BS * (2 * D + 8 * H)}
    model.generate(_idx("v1000", B), 4)
    assert gen.kv_cache_nbytes(model) == {"_mg_decode_cache": L * B * BS * 6 * D,
                                          "_mg_kv8_cache": L * B * BS * (2 * D + 8 * H)}


def test_value_errors_on_the_gpu():
    model, idx = _model("v1000"), _idx("v1000", 1)
    with pytest.raises(ValueError):
        model.generate(idx, 2, kv_cache="int8", use_cache=False)
    with pytest.raises(ValueError):
        model.generate(idx, 2, kv_cache="fp8")
    with pytest.raises(ValueError):
        model.generate_batch([idx[0]], 2, kv_cache="int4")


# ------------------------------------------------------------------ 3. an anchor outside the code under test
@pytest.mark.parametrize("name,B", [("v1000", 2), ("v8200", 3), ("v1000", 16)])
def test_anchor_oracle_snap_and_the_bf16_kernel(name, B):
    """Prefill and three steps built here from ``_Body._blocks``: the attend snaps K / V through the numpy
    oracle and calls ``attention_decode`` on this test's bf16 caches.  The KV8 state's logits -- int8
    caches, ``kv8_store``, ``attention_decode_kv8`` -- equal them bit for bit."""
    model, cfg = _model(name), CONFIGS[name]
    D, H, V = cfg["n_embed"], cfg["n_head"], cfg["vocab_size"]
    idx = _idx(name, B)
    body = gen._Body(model)
    C, bf, tr = body.C, body.bf, model.transformer
    caches = [torch.zeros(B, BS, 3 * D, dtype=torch.bfloat16, device="cuda") for _ in range(L)]
    part = torch.empty(C.attention_decode_part_floats(B, H, D // H), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(B * H, dtype=torch.int32, device="cuda")

    def snap_(qkv):  # the K and V thirds of qkv [..., 3D] in place, per head, through the oracle
        kv = qkv[..., D:].float().cpu().numpy().reshape(*qkv.shape[:-1], 2 * H, D // H)
        d = torch.from_numpy(O.snap(kv)[2]).to(torch.bfloat16).reshape(*qkv.shape[:-1], 2 * D)
        qkv[..., D:].copy_(d)

    def keep(i, qkv):
        snap_(qkv)
        caches[i][:, :T].copy_(qkv)

    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setattr(gen, "_KV8_DECODE", True)
        _drop_states(model)
        state = gen._state_for(model, "_mg_kv8_cache", idx, BS)
        assert state.kv8 and state.kq and not state.caches
        x = body._prompt(idx, keep)[:, -1]
        logits = body._head(x.contiguous(), "mfma")[:, :V]
        assert bit_equal(state.logits, logits), "prefill logits"
        route = body._route(B)
        for pos in range(T, T + 3):
            tok = logits.argmax(-1).view(B, 1)
            got = state.step(tok, pos)
            pd = torch.full((1,), pos, dtype=torch.int32, device="cuda")

            def attend(i, qkv):
                snap_(qkv)
                return C.attention_decode(qkv, caches[i], H, pos, pd, part, cnt, 0)

            x = C.embedding_fwd(tok, bf(tr.wte.weight), bf(tr.wpe.weight), 0.0, 0, pd, None, None, 0).view(B, D)
            logits = body._head(body._blocks(x, attend, route), route)[:, :V]
            assert bit_equal(got, logits), f"step at position {pos}"
        # the int8 cache holds the oracle's integers of what the test's cache holds
        kv = caches[1][:, :T + 3, D:].float().cpu().numpy().reshape(B, T + 3, 2, H, D // H)
        q, s, _ = O.snap(kv)
        assert torch.equal(state.kq[1][:, :, :, :T + 3].cpu(), torch.from_numpy(q).permute(0, 2, 3, 1, 4))
        assert torch.equal(state.ks[1][:, :, :, :T + 3].cpu(), torch.from_numpy(s).permute(0, 2, 3, 1))
        _drop_states(model)
