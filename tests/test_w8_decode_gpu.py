"""W8 decode: on a model snapped by ``quantize_int8_`` the device decode loops of up to 8 rows run
every projection and the LM head on ``gemv_w8`` (int8 weight rows, csrc/kernels/gemv.hip) and
produce what the bf16 kernel produces on the same snapped model -- equal tokens and bit-equal stored
logits with ``_W8_DECODE`` on and off, in every decode mode.  Models of 2 layers without dropout:
"v1000" (n_embed 128; torch argmax), "v8200" (n_embed 128; the wide LM head with the fused argmax)
and "w1280" (n_embed 1280, 20 heads: the MLP output projection takes the long-row path)."""
import functools
import gc

import pytest
import torch

from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

BS = 96
CONFIGS = {"v1000": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=1000, block_size=BS),
           "v8200": dict(n_layer=2, n_head=2, n_embed=128, vocab_size=8200, block_size=BS),
           "w1280": dict(n_layer=2, n_head=20, n_embed=1280, vocab_size=512, block_size=BS)}
T, NEW = 12, 24
CACHES = ("_mg_decode_cache", "_mg_beam_cache", "_mg_spec_cache")


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    yield
    gc.collect()


def _build(name):
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, **CONFIGS[name])
    model = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    report = model.quantize_int8_()
    assert model._mg_w8 and all(0 < v < 1 / 127 for v in report.values())
    return model


_model = functools.lru_cache(maxsize=None)(_build)


def _idx(name, B, T=T, seed=1):
    g = torch.Generator().manual_seed(seed + B)
    return torch.randint(0, CONFIGS[name]["vocab_size"], (B, T), generator=g).cuda()


def _drop_states(model):
    for k in CACHES:
        model.__dict__.pop(k, None)


def _run(model, fn, w8, graph=True):
    """(fn(model)'s tensors, {(state, loop): its stored logits}) on fresh decode states with
    ``_W8_DECODE`` = ``w8``; the launches counted per kernel."""
    C = ext()
    calls = {"gemv": 0, "gemv_w8": 0}
    real = {k: getattr(C, k) for k in calls}

    def counted(k):
        def f(*a, **kw):
            calls[k] += 1
            return real[k](*a, **kw)
        return f

    _drop_states(model)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(gen, "_W8_DECODE", w8)
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


def _check_on_off(model, fn, loop, graph=True, bf16_calls=0):
    """``fn`` with the switch on and off: equal outputs, bit-equal stored logits of ``loop``; on, the
    skinny GEMM launches are gemv_w8's (but ``bf16_calls`` per step body call); off, none is."""
    on, lon, con = _run(model, fn, True, graph)
    off, loff, coff = _run(model, fn, False, graph)
    assert loop in lon and set(lon) == set(loff), (sorted(map(str, lon)), sorted(map(str, loff)))
    per = 4 * len(model.transformer.h) + 1  # skinny GEMM launches of one step body
    assert coff["gemv_w8"] == 0 and coff["gemv"] >= per and coff["gemv"] % per == 0, coff
    bodies = coff["gemv"] // per
    assert con == {"gemv": bodies * bf16_calls, "gemv_w8": bodies * (per - bf16_calls)}, (con, coff)
    assert len(on) == len(off) and len(on) >= 1
    for a, b in zip(on, off):
        assert bit_equal(a, b), "outputs differ between gemv_w8 and gemv"
    for k in lon:
        assert bit_equal(lon[k], loff[k]), f"stored logits of loop {k} differ"
    return on


# ------------------------------------------------------------------ 1. the route is taken
@pytest.mark.parametrize("name", list(CONFIGS))
def test_decode_goes_through_gemv_w8(name):
    """A generate on a quantized model launches gemv_w8 for every projection and the LM head and no
    gemv; at 16 rows (the rows GEMM) it launches neither."""
    model, C = _model(name), ext()
    D, L = CONFIGS[name]["n_embed"], CONFIGS[name]["n_layer"]
    widths = []
    real = C.gemv_w8

    def counted(x, q, s, *a, **kw):
        assert q.dtype == torch.int8 and s.dtype == torch.float32 and s.numel() == q.size(0)
        widths.append((q.size(0), q.size(1)))
        return real(x, q, s, *a, **kw)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(C, "gemv_w8", counted)
        out, _, calls = _run(model, lambda m: m.generate(_idx(name, 2), NEW), True)
    assert out[0].shape == (2, T + NEW)
    assert calls["gemv"] == 0 and calls["gemv_w8"] >= 4 * L + 1
    V = CONFIGS[name]["vocab_size"]
    body = [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)] * L + [(V, D)]
    assert widths[:len(body)] == body and len(widths) % len(body) == 0
    assert all(gen.w8_status(model).values())
    _, _, calls = _run(model, lambda m: m.generate(_idx(name, 16), 4), True)
    assert calls == {"gemv": 0, "gemv_w8": 0}


def test_an_unquantized_model_takes_no_new_branch():
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, **CONFIGS["v1000"])
    model = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    _, _, calls = _run(model, lambda m: m.generate(_idx("v1000", 2), 4), True)
    assert calls["gemv_w8"] == 0 and calls["gemv"] > 0
    assert "_mg_w8_weights" not in model.__dict__ or not model.__dict__["_mg_w8_weights"]


# ------------------------------------------------------------------ 2. on and off: the same bits
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_greedy(name, graph):
    idx = _idx(name, 3)
    on = _check_on_off(_model(name), lambda m: m.generate(idx, NEW), ("_mg_decode_cache", "greedy"), graph)
    assert on[0].shape == (3, T + NEW)


@pytest.mark.parametrize("name", ["v1000", "v8200"])
def test_seeded_sampling_top_k_top_p(name):
    idx = _idx(name, 4)
    _check_on_off(_model(name), lambda m: m.generate(idx, NEW, temperature=0.8, do_sample=True, top_k=20, top_p=0.9,
                                                      seed=5), ("_mg_decode_cache", "sample"))


@pytest.mark.parametrize("name", ["v1000", "v8200"])
def test_logprobs(name):
    idx = _idx(name, 2)
    on = _check_on_off(_model(name), lambda m: m.generate(idx, NEW, return_logprobs=True),
                       ("_mg_decode_cache", "greedy_lp"))
    assert len(on) == 2 and on[1].dtype == torch.float32


@pytest.mark.parametrize("name", ["v1000", "v8200"])
def test_logits_processor(name):
    idx = _idx(name, 2)
    _check_on_off(_model(name), lambda m: m.generate(idx, NEW, repetition_penalty=1.3, no_repeat_ngram_size=3),
                  ("_mg_decode_cache", "greedy_proc"))


@pytest.mark.parametrize("name", ["v1000", "v8200"])
def test_ragged_batch(name):
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, CONFIGS[name]["vocab_size"], (n,), generator=g).cuda() for n in (1, 7, 3, 12, 2)]
    on = _check_on_off(_model(name), lambda m: generate_batch(m, prompts, NEW), ("_mg_decode_cache", ("ragged", True)))
    assert on[1].tolist() == [n + NEW for n in (1, 7, 3, 12, 2)]


@pytest.mark.parametrize("name", ["v1000", "v8200"])
def test_beam(name):
    idx = _idx(name, 2)
    on = _check_on_off(_model(name), lambda m: m.generate_beam(idx, 16, 4), ("_mg_beam_cache", ("beam", 4)))
    assert on[0].shape == (2, 4, T + 16)


@pytest.mark.parametrize("name", ["v1000", "v8200"])
def test_speculative(name):
    idx = _idx(name, 2)
    idx[:, 6:] = idx[:, :6]  # a repetition: drafts exist
    on = _check_on_off(_model(name), lambda m: m.generate_speculative(idx, NEW, draft_len=3),
                       ("_mg_spec_cache", ("spec", 4)))
    assert torch.equal(on[0], _model(name).generate(idx, NEW))
    _drop_states(_model(name))


def test_window_slide():
    """T + n > block_size: the window slides (a prefill per window on the snapped bf16 weights, then
    the W8 loop again)."""
    idx = _idx("v8200", 2, T=80)
    on = _check_on_off(_model("v8200"), lambda m: m.generate(idx, 30), ("_mg_decode_cache", "greedy"))
    assert on[0].shape == (2, 110) and 110 > BS


def test_flipping_the_switch_never_replays_the_other_kernels_graph(monkeypatch):
    """One decode state kept across the flips: each flip drops the captured loops, so the step body is
    called again (warm-up and capture) on the kernel the switch names."""
    model, C = _build("v8200"), ext()
    idx = _idx("v8200", 2)
    calls = {"gemv": 0, "gemv_w8": 0}
    for k in calls:
        def counted(*a, _k=k, _real=getattr(C, k), **kw):
            calls[_k] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(C, k, counted)
    want = model.generate(idx, NEW)
    state = model._mg_decode_cache
    n = calls["gemv_w8"]  # the warm-up and the capture: whole step bodies
    assert calls["gemv"] == 0 and n >= 4 * 2 + 1 and n % (4 * 2 + 1) == 0
    assert torch.equal(model.generate(idx, NEW), want) and calls["gemv_w8"] == n  # a replay calls nothing
    monkeypatch.setattr(gen, "_W8_DECODE", False)
    assert torch.equal(model.generate(idx, NEW), want) and model._mg_decode_cache is state
    assert calls == {"gemv": n, "gemv_w8": n}
    monkeypatch.setattr(gen, "_W8_DECODE", True)
    assert torch.equal(model.generate(idx, NEW), want)
    assert calls == {"gemv": n, "gemv_w8": 2 * n}


# ------------------------------------------------------------------ 3. a weight that moves
def test_a_changed_weight_leaves_the_w8_path():
    """After an in-place change the LM head's weight no longer equals a dequantized twin: it goes back
    to the bf16 kernel (one gemv per step body), the rest stays on gemv_w8, decode equals the
    switch-off run and the status says which weight left."""
    model = _build("v8200")
    idx = _idx("v8200", 2)
    _check_on_off(model, lambda m: m.generate(idx, NEW), ("_mg_decode_cache", "greedy"))
    assert all(gen.w8_status(model).values())
    with torch.no_grad():
        model.lm_head.weight.add_(1e-3)
    _check_on_off(model, lambda m: m.generate(idx, NEW), ("_mg_decode_cache", "greedy"), bf16_calls=1)
    status = gen.w8_status(model)
    assert status.pop("lm_head.weight") is False and all(status.values())
