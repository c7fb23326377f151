"""KV8 on the CPU: ``ops.quant.snap_vectors`` against the numpy oracle of the rule (``_kv8_oracle``),
and the KV8 model -- every attention on snap(K), snap(V) -- through ``generate`` / ``generate_batch``
with ``kv_cache="int8"`` on a 2-layer fp64 model, against this file's own full re-forward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _kv8_oracle as O
from mingpt_distributed_amd.models import GPT, GPTConfig, generate, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops.quant import snap_vectors


def _np(t):
    return (t.double() if t.dtype == torch.float64 else t.float()).numpy()


def _check(x):
    """snap_vectors(x) equals the oracle: integers, scale bits (NaN where the oracle says NaN) and the
    dequantized values' bits."""
    q, s, d = snap_vectors(x)
    oq, os_, od = O.snap(_np(x))
    assert q.dtype == torch.int8 and q.shape == x.shape and s.shape == x.shape[:-1] and d.dtype == x.dtype
    assert np.array_equal(q.numpy(), oq)
    assert np.array_equal(_np(s), os_.astype(_np(s).dtype), equal_nan=True)
    assert np.array_equal(_np(d), od, equal_nan=True)
    return q, s, d


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64])
def test_random_vectors(dtype):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(4, 3, 7, 24, generator=g) * torch.logspace(-6, 6, 7).view(1, 1, 7, 1)).to(dtype)
    q, s, d = _check(x)
    a = x.double().abs().amax(-1)
    assert bool((q.abs().amax(-1) >= 64).all())  # a / s > 63.5
    assert bool(((x.double() - d.double()).abs() <= s.double().unsqueeze(-1) / 2).all())
    assert bool((s.double() / 2 < a / 127).all())


def test_zero_vectors():
    x = torch.zeros(3, 8, dtype=torch.bfloat16)
    x[1, 2] = 0.5
    q, s, d = _check(x)
    assert s.tolist() == [1.0, 2.0 ** -7, 1.0] and int(q[0].abs().max()) == 0 and q[1, 2] == 64
    assert torch.equal(d, x)


def test_both_frexp_branches():
    """a with significand 254/256 (m = 127/128: 2^(e-7), q = 127) and 255/256 (m > 127/128: 2^(e-6), q = 64
    after rounding 63.75)."""
    x = torch.tensor([[254.0 / 256, 0.1], [255.0 / 256, 0.1], [254.0 / 64, -0.3], [-255.0 / 64, 0.3]],
                     dtype=torch.bfloat16)
    assert x[1, 0].item() == 255.0 / 256  # exact in bf16
    q, s, _ = _check(x)
    assert s.tolist() == [2.0 ** -7, 2.0 ** -6, 2.0 ** -5, 2.0 ** -4]
    assert q[:, 0].tolist() == [127, 64, 127, -64]
    _check(x.float())
    y = torch.tensor([[1.0 - 2.0 ** -20, 0.0]], dtype=torch.float32)  # fp32: m just above 127/128
    assert _check(y)[1].item() == 2.0 ** -6


def test_exact_halves_round_to_even():
    x = torch.tensor([[1.0, 2.5 * 2 ** -6, 3.5 * 2 ** -6, -2.5 * 2 ** -6, -3.5 * 2 ** -6, 0.5 * 2 ** -6, 1.5 * 2 ** -6,
                       0.0]], dtype=torch.bfloat16)
    q, s, _ = _check(x)
    assert s.item() == 2.0 ** -6 and q[0].tolist() == [64, 2, 4, -2, -4, 0, 2, 0]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_tiny_scale(dtype):
    """a = 2^-120: the scale stops at 2^-126 (q = 64); elements below it round on the same grid."""
    x = torch.tensor([[2.0 ** -120, 2.0 ** -126, 2.0 ** -127, 3 * 2.0 ** -128, -2.0 ** -121, 0.0, 2.0 ** -133, 0.0],
                      [2.0 ** -130, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -2.0 ** -127]], dtype=dtype)
    q, s, d = _check(x)
    assert s.tolist() == [2.0 ** -126, 2.0 ** -126]
    assert q[0].tolist() == [64, 1, 0, 1, -32, 0, 0, 0] and q[1].tolist() == [0] * 8
    assert d[0, 3].item() == 2.0 ** -126


def test_non_finite_vectors_are_isolated():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 16, generator=g).bfloat16()
    clean = snap_vectors(x)
    x[1, 3] = float("nan")
    x[3, 0] = float("-inf")
    q, s, d = _check(x)
    assert torch.isnan(s[[1, 3]]).all() and int(q[[1, 3]].abs().max()) == 0 and torch.isnan(d[[1, 3]]).all()
    for r in (0, 2, 4):
        assert torch.equal(q[r], clean[0][r]) and s[r] == clean[1][r] and torch.equal(d[r], clean[2][r])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64])
def test_snap_is_idempotent(dtype):
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(6, 5, 40, generator=g) * 3).to(dtype)
    x[0, 0] = 0
    q, s, d = snap_vectors(x)
    q2, s2, d2 = snap_vectors(d)
    assert torch.equal(q, q2) and torch.equal(s, s2) and torch.equal(d, d2)
    assert torch.equal(d.double(), q.double() * s.double().unsqueeze(-1))  # s * q is exact in the dtype


def test_snap_vectors_rejects_other_inputs():
    with pytest.raises(ValueError):
        snap_vectors(torch.zeros(3, 4, dtype=torch.float16))
    with pytest.raises(ValueError):
        snap_vectors(torch.zeros(3, 0))


# ------------------------------------------------------------------ the KV8 model, fp64
V, BS = 61, 24


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=32, vocab_size=V, block_size=BS, embed_drop=0.0, resid_drop=0.0,
                    attn_drop=0.0)
    return GPT(cfg, verbose=False).double().eval()


def _snap_t(t):
    return torch.from_numpy(O.snap(t.numpy())[2])


@torch.no_grad()
def _reforward(model, idx):
    """Last-position logits of the KV8 model on idx [B, T], the whole sequence at once: the model's own
    LayerNorms, projections and MLP, this file's attention on oracle-snapped K / V."""
    tr, H = model.transformer, model.config.n_head
    B, T = idx.shape
    x = tr.wte.weight[idx] + tr.wpe.weight[:T]
    C = x.size(-1)
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for blk in tr.h:
        q, k, v = F.linear(blk.ln_1(x), blk.attn.c_attn.weight, blk.attn.c_attn.bias).split(C, dim=2)
        q, k, v = (t.view(B, T, H, C // H).transpose(1, 2) for t in (q, k, v))
        k, v = _snap_t(k.contiguous()), _snap_t(v.contiguous())
        att = (q @ k.transpose(-1, -2)) / (C // H) ** 0.5
        att = att.masked_fill(~mask, float("-inf")).softmax(dim=-1)
        y = (att @ v).transpose(1, 2).reshape(B, T, C)
        x = x + F.linear(y, blk.attn.c_proj.weight, blk.attn.c_proj.bias)
        x = x + blk.mlp(blk.ln_2(x))
    return model.lm_head(tr.ln_f(x[:, -1]))


@torch.no_grad()
def test_generate_int8_is_the_kv8_model(model):
    """Every step's logits (the cache path's own, and through the reported log-probabilities) against
    the full re-forward within 1e-9 -- fp64 round-off with four orders of margin -- and equal tokens."""
    idx = torch.randint(0, V, (2, 5), generator=torch.Generator().manual_seed(3))
    n = 12
    out, lp = generate(model, idx, n, kv_cache="int8", return_logprobs=True)
    assert out.shape == (2, 5 + n) and torch.equal(out[:, :5], idx)
    cache = gen._CpuCache(model, idx, kv8=True)
    logits = cache.logits
    for j in range(n):
        want = _reforward(model, out[:, :5 + j])
        assert float((logits - want).abs().max()) <= 1e-9
        assert torch.equal(want.argmax(-1), out[:, 5 + j])
        got_lp = lp[:, 5 + j].double()
        want_lp = want.log_softmax(-1).gather(1, out[:, 5 + j:6 + j]).view(-1)
        assert float((got_lp - want_lp).abs().max()) <= 1e-6  # the reported numbers are float32
        if j + 1 < n:
            logits = cache.step(out[:, 5 + j:6 + j], 5 + j)
    plain = model(idx)[0][:, -1]  # the unsnapped model: the plain cache computes it, the KV8 one does not
    assert float((gen._CpuCache(model, idx).logits - plain).abs().max()) <= 1e-9
    assert float((gen._CpuCache(model, idx, kv8=True).logits - plain).abs().max()) > 1e-6


def test_generate_int8_slides_past_block_size(model):
    idx = torch.randint(0, V, (1, BS - 3), generator=torch.Generator().manual_seed(4))
    out = generate(model, idx, 6, kv_cache="int8")
    for j in range(6):
        ctx = out[:, max(0, BS - 3 + j - BS):BS - 3 + j]
        assert torch.equal(_reforward(model, ctx).argmax(-1), out[:, BS - 3 + j])


def test_generate_batch_rows_equal_generate_alone(model):
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, V, (n,), generator=g) for n in (1, 6, 3)]
    tokens, lengths = generate_batch(model, prompts, 7, kv_cache="int8")
    for b, p in enumerate(prompts):
        alone = generate(model, p.view(1, -1), 7, kv_cache="int8")
        assert int(lengths[b]) == p.numel() + 7 and torch.equal(tokens[b, :p.numel() + 7], alone[0])
    seeded = generate_batch(model, prompts, 7, do_sample=True, seed=11, top_k=10, kv_cache="int8")
    again = model.generate_batch(prompts, 7, do_sample=True, seed=11, top_k=10, kv_cache="int8")
    assert torch.equal(seeded[0], again[0])


def test_value_errors(model):
    idx = torch.randint(0, V, (1, 4))
    with pytest.raises(ValueError):
        generate(model, idx, 2, kv_cache="int8", use_cache=False)
    for bad in ("fp8", "int4", "INT8", None, 8):
        with pytest.raises(ValueError):
            generate(model, idx, 2, kv_cache=bad)
        with pytest.raises(ValueError):
            generate_batch(model, [idx[0]], 2, kv_cache=bad)
    with pytest.raises(TypeError):
        model.generate_beam(idx, 2, 2, kv_cache="int8")
    with pytest.raises(TypeError):
        model.generate_speculative(idx, 2, kv_cache="int8")
    with pytest.raises(TypeError):
        model.score(idx, kv_cache="int8")


def test_bf16_is_the_call_without_the_argument(model):
    idx = torch.randint(0, V, (2, 4), generator=torch.Generator().manual_seed(6))
    a = model.generate(idx, 8, return_logprobs=True)
    b = model.generate(idx, 8, return_logprobs=True, kv_cache="bf16")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(model.generate(idx, 5, use_cache=False), model.generate(idx, 5, use_cache=False, kv_cache="bf16"))
    prompts = [idx[0], idx[1, :2]]
    x, y = model.generate_batch(prompts, 6), model.generate_batch(prompts, 6, kv_cache="bf16")
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    torch.manual_seed(9)
    s1 = model.generate(idx, 6, do_sample=True)
    torch.manual_seed(9)
    s2 = model.generate(idx, 6, do_sample=True, kv_cache="bf16")
    assert torch.equal(s1, s2)


def test_kv_cache_nbytes_of_a_model_without_states(model):
    assert gen.kv_cache_nbytes(model) == {}
