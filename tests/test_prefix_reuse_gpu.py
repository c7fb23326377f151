"""``generate(reuse_cache=True)`` on the GPU: a prompt that starts with the tokens the decode state's KV
cache holds runs only the tokens behind them (``_GpuCache.extend``, ``attention_extend``).  The extension
is taken and leaves the right record; its logits are as close to a float32 CPU forward as a fresh
prefill's (within a factor of two: both round the same quantities to bf16, in other orders); greedy
tokens follow a fresh call's up to a near-tie; and without the argument nothing changes."""
import functools

import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

V, BS, NEW = 512, 96, 6


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, n_layer=2, n_head=20, n_embed=1280,
                    vocab_size=V, block_size=BS)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


def _prompt(B, T, seed=3):
    return torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _extended(model, idx, P, n, first=None):
    """``generate(idx, n, reuse_cache=True)`` on a state that holds ``first`` (default: idx[:, :P])."""
    model.__dict__.pop("_mg_decode_cache", None)
    model.generate(idx[:, :P] if first is None else first, 1, reuse_cache=True)
    return model.generate(idx, n, reuse_cache=True)


# (B, P, Tq, the column where the last row of the held prompt differs, or None): the skinny route, the rows
# GEMM, the MFMA GEMM, and a prefix cut short by one row
CASES = [(1, 40, 3, None), (2, 30, 20, None), (2, 8, 60, None), (2, 30, 20, 5)]


@pytest.mark.parametrize("B,P,Tq,differ", CASES)
def test_extension_is_taken_and_recorded(B, P, Tq, differ, monkeypatch):
    """With ``_REUSE_GATE`` off: the path itself on every GEMM route, also where the measured rule
    (``_reuse_pays``) would prefill -- 120 new rows on 16 saved ones -- which the last lines check."""
    monkeypatch.setattr(gen, "_REUSE_GATE", False)
    model, idx = _model(), _prompt(B, P + Tq)
    first = idx[:, :P].clone()
    if differ is not None:
        first[-1, differ] = (first[-1, differ] + 1) % V
    out = _extended(model, idx, P, NEW, first)
    st = model._mg_decode_cache
    assert st.reused == (P if differ is None else differ)
    assert st.nheld == P + Tq + NEW - 1 and torch.equal(st.held[:, :st.nheld], out[:, :-1])
    monkeypatch.undo()
    _extended(model, idx, P, NEW, first)
    Pe = P if differ is None else differ
    assert model._mg_decode_cache.reused == (Pe if gen._reuse_pays(B, Pe, P + Tq - Pe) else 0)


def test_logits_against_float32():
    model, (B, P, Tq) = _model(), (2, 30, 20)
    idx = _prompt(B, P + Tq, seed=4)
    cpu = GPT(model.config, verbose=False).eval()  # the same bf16-valued weights in float32
    cpu.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        ref = cpu(idx.cpu())[0][:, -1]
    model.__dict__.pop("_mg_decode_cache", None)
    model.generate(idx, 1)
    fresh = model._mg_decode_cache.logits.float().cpu()
    _extended(model, idx, P, 1)
    assert model._mg_decode_cache.reused == P
    e_fresh = float((fresh - ref).abs().max())
    e_ext = float((model._mg_decode_cache.logits.float().cpu() - ref).abs().max())
    print(f"PREFIX logits: max |fresh - ref| {e_fresh:.5f}, max |extended - ref| {e_ext:.5f}")
    assert e_ext <= 2 * e_fresh, (e_ext, e_fresh)


def test_greedy_follows_a_fresh_call():
    """The rule of test_decode_wide_gpu.py::test_greedy_follows_the_uncached_reference: a row may leave
    the reference only where its two best logits are closer than 0.05, compared up to that column."""
    model, (B, P, Tq, n) = _model(), (2, 30, 20, 40)
    idx = _prompt(B, P + Tq, seed=5)
    model.__dict__.pop("_mg_decode_cache", None)
    want = model.generate(idx, n)
    got = _extended(model, idx, P, n)
    assert model._mg_decode_cache.reused == P
    for b in range(B):
        diff = (got[b] != want[b]).nonzero()
        if diff.numel():
            col = int(diff[0])
            top = model(want[b:b + 1, :col])[0][0, -1].float().topk(2).values
            gap = float(top[0] - top[1])
            print(f"row {b} leaves the fresh call at column {col}: top-two gap {gap:.4f}")
            assert gap < 0.05, f"row {b} differs at column {col} where the gap is {gap:.4f}"


def test_default_is_untouched():
    model, idx = _model(), _prompt(2, 50, seed=6)
    model.__dict__.pop("_mg_decode_cache", None)
    a = model.generate(idx, NEW)
    st = model._mg_decode_cache
    graph = st._loops["greedy"].graph
    model.generate(idx, NEW, reuse_cache=True)  # leaves a record ...
    assert st.nheld == 50 + NEW - 1
    b = model.generate(idx, NEW)  # ... that a call without the argument clears
    assert model._mg_decode_cache is st and st.nheld == 0 and st.reused == 0
    assert torch.equal(a, b)
    assert graph is not None and st._loops["greedy"].graph is graph
