"""``generate(num_return_sequences=N, kv_cache="int8")`` through the shared KV8 state (``_mg_shared_kv8_cache``,
``attention_decode_shared_kv8``), both gates off.  ``_KV8_DECODE`` off must give the same tokens and
log-probability bits; against the repeated batch on the plain KV8 state a row may leave only at a step whose
two best logits are closer than 0.05 (the near-tie rule of test_num_return_sequences_gpu.py)."""
import functools

import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen

pytestmark = pytest.mark.gpu

V, BS, T, NEW, SEED = 512, 96, 20, 12, 7
CASES = [(1, 2), (1, 9), (2, 3)]  # (B, N): the skinny GEMM, the rows GEMM, two prompts
SLOT = "_mg_shared_kv8_cache"


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, n_layer=3, n_head=3, n_embed=48, vocab_size=V,
                    block_size=BS)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


def _shared(monkeypatch, B, N):
    monkeypatch.setattr(gen, "_SHARED_GATE", False)
    monkeypatch.setattr(gen, "_SHARED_KV8_GATE", False)
    model = _model()
    model.__dict__.pop(SLOT, None)
    idx = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(3)).cuda()
    return model, idx, lambda **kw: model.generate(idx, NEW, num_return_sequences=N, kv_cache="int8", **kw)


@pytest.mark.parametrize("B,N", CASES)
def test_same_bits_on_both_kernels_and_follows_the_repeated_batch(B, N, monkeypatch):
    model, idx, run = _shared(monkeypatch, B, N)
    seeded = dict(do_sample=True, seed=SEED, return_logprobs=True)
    (tok, lp), got = run(**seeded), run()
    st, cfg = model.__dict__[SLOT], model.config
    assert st.shared and st._kv8_on() and st.kq and st.own_q and not st.caches and not st.own
    assert gen.kv_cache_nbytes(model)[SLOT] == cfg.n_layer * (B * BS + B * N * 64) * (2 * cfg.n_embed + 8 * cfg.n_head)
    want, left = model.generate(idx.repeat_interleave(N, 0), NEW, kv_cache="int8"), 0
    for r in range(B * N):  # greedy against the definition: the KV8 model's logits from a prefill of the row
        diff = (got[r] != want[r]).nonzero()
        if diff.numel():
            col, left = int(diff[0]), left + 1
            top = gen._state_for(model, "_mg_kv8_cache", want[r:r + 1, :col], BS).logits[0].float().topk(2).values
            assert float(top[0] - top[1]) < 0.05, f"row {r} differs at column {col}: gap {float(top[0] - top[1]):.4f}"
    print(f"(B, N) = ({B}, {N}): {left} of {B * N} rows left the repeated batch at a near-tie")
    monkeypatch.setattr(gen, "_KV8_DECODE", False)  # the same KV8 model on the bf16 kernel
    tok_off, lp_off = run(**seeded)
    assert model.__dict__[SLOT] is st and st.caches and st.own and not st.kq and not st.own_q
    assert tok.shape == (B * N, T + NEW) and torch.equal(tok, tok_off) and torch.equal(lp, lp_off)
    assert not all(bool((tok[b * N:(b + 1) * N] == tok[b * N]).all()) for b in range(B))  # seeded rows diverge


def test_without_num_return_sequences_there_is_no_shared_kv8_state(monkeypatch):
    model, idx, _ = _shared(monkeypatch, 2, 3)
    model.generate(idx, NEW, kv_cache="int8")
    assert SLOT not in model.__dict__
