"""The W8 rule (csrc/include/common.h 'W8', ops/quant.py) on the CPU: its four consequences on random
and edge-case matrices, the refusal of non-finite weights, ``quantize_int8_`` on a tiny GPT, and the
numpy restatement of the kernel: ``s * fold(lane_sums(x, q))`` equals ``fold(lane_sums(x, s q))`` bit
for bit (tests/_gemv_oracle.py), before and after the exactly restated epilogues."""
import copy

import numpy as np
import pytest
import torch

import _gemv_oracle as O
from mingpt_distributed_amd.models import GPT, GPTConfig, quantize_int8_
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops.quant import dequantize_rows, quantize_rows

BF = torch.bfloat16


def _matrix(dtype, seed=0, N=40, K=72):
    """Random rows of different magnitudes plus the edge rows: 0 all zero, 1 one outlier, 2 a maximum
    of exactly 127 * 2^-5, 3 a maximum of exactly 128 * 2^-9 (both exact in bf16), 4 a negative maximum."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.logspace(-4, 3, N)[:, None]
    w[0] = 0
    w[1] *= 1e-3
    w[1, 17] = 31.0
    w[2] = w[2].clamp(-3.0, 3.0)
    w[2, 5] = 127 * 2.0 ** -5
    w[3] = w[3].clamp(-0.2, 0.2)
    w[3, 70] = 128 * 2.0 ** -9
    w[4] = w[4].clamp(-1.0, 1.0)
    w[4, 0] = -1.75
    return w.to(dtype)


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("seed", [0, 1])
def test_rule_consequences(dtype, seed):
    w = _matrix(dtype, seed)
    q, s = quantize_rows(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (w.shape[0],)
    w64, s64, q64 = w.double(), s.double(), q.double()
    a = w64.abs().amax(1)
    # scales: powers of two; 1 for the zero row; the smallest with a / s <= 127
    m, _ = torch.frexp(s)
    assert (m == 0.5).all()
    assert s[0] == 1 and (q[0] == 0).all()
    nz = a > 0
    assert (a[nz] / s64[nz] <= 127).all() and (a[nz] / (s64[nz] / 2) > 127).all()
    assert s[2] == 2.0 ** -5 and q[2, 5] == 127          # a maximum of exactly 127 * 2^e keeps 2^e
    assert s[3] == 2.0 ** -8 and q[3, 70] == 64          # 128 * 2^e moves to 2^(e + 1)
    assert q[4, 0] == -112 and s[4] == 2.0 ** -6
    assert q.abs().max() <= 127
    # 1. |W - s q| <= s / 2 < a / 127
    err = (w64 - s64[:, None] * q64).abs().amax(1)
    assert (err <= s64 / 2).all() and (s64[nz] / 2 < a[nz] / 127).all()
    # 2. max |q| >= 64 on every non-zero row
    assert (q64.abs().amax(1)[nz] >= 64).all()
    # 3. s q is exact in bf16
    d = dequantize_rows(q, s, BF)
    assert torch.equal(d.double(), s64[:, None] * q64)
    # 4. the quantizer is idempotent on its own output, in either dtype
    for dt in (BF, torch.float32):
        q2, s2 = quantize_rows(dequantize_rows(q, s, dt))
        assert torch.equal(q2, q) and torch.equal(s2, s)
    # q is the nearest integer, halves to even
    want = torch.from_numpy(np.rint((w64 / s64[:, None]).numpy())).clamp(-127, 127)
    assert torch.equal(q64, want)


def test_round_half_to_even_and_outlier_row():
    w = torch.zeros(2, 8)
    w[0] = torch.tensor([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5])
    w[1, 3] = 1000.0
    w[1, 4] = 3.9
    q, s = quantize_rows(w)
    assert s.tolist() == [1.0, 8.0]
    assert q[0].tolist() == [127, 0, 2, 2, 0, -2, -2, 64]
    assert q[1].tolist() == [0, 0, 0, 125, 0, 0, 0, 0]  # 3.9 / 8 = 0.4875 rounds to 0: an outlier costs the row


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_non_finite_weights_are_refused(bad, dtype):
    w = _matrix(dtype)
    w[7, 3] = bad
    with pytest.raises(ValueError, match="non-finite"):
        quantize_rows(w)


def test_other_inputs_are_refused():
    with pytest.raises(ValueError):
        quantize_rows(torch.zeros(8))
    with pytest.raises(ValueError):
        quantize_rows(torch.zeros(4, 8, dtype=torch.float16))


# ---------------------------------------------------------------------- quantize_int8_ on a tiny GPT
def _tiny(dtype=torch.float32):
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=32, vocab_size=61, block_size=16, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).to(dtype).eval()


LISTED = ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_quantize_int8_on_a_tiny_gpt(dtype):
    model = _tiny(dtype)
    before = copy.deepcopy(model.state_dict())
    assert not model.__dict__.get("_mg_w8", False)
    report = model.quantize_int8_()
    assert model._mg_w8 is True
    after = copy.deepcopy(model.state_dict())
    # exactly the listed weights changed (lm_head.weight is the tied wte: both names show it)
    listed = {k for k in before if k.endswith(LISTED)} | {"lm_head.weight", "transformer.wte.weight"}
    assert model.lm_head.weight is model.transformer.wte.weight
    for k in before:
        if k in listed:
            assert not torch.equal(before[k], after[k]), k
            q, s = quantize_rows(before[k])
            assert torch.equal(after[k], dequantize_rows(q, s, dtype)), k
        else:
            assert torch.equal(before[k], after[k]), f"{k} changed"
    # the report: one entry per snapped weight, the rule's bound
    assert set(report) == {k for k in before if k.endswith(LISTED)} | {"lm_head.weight"}
    assert all(0 < v < 1 / 127 for v in report.values()), report
    # idempotent: nothing moves (not even a version counter), the report is all zeros
    versions = [p._version for p in model.parameters()]
    again = quantize_int8_(model)
    assert set(again) == set(report) and all(v == 0.0 for v in again.values())
    assert [p._version for p in model.parameters()] == versions
    for k, v in model.state_dict().items():
        assert torch.equal(v, after[k]), k
    # the snapped model is a model: one built from the dequantized state dict computes the same
    twin = _tiny(dtype)
    sd = {}
    for k, v in before.items():
        if k in listed:
            q, s = quantize_rows(v)
            v = dequantize_rows(q, s, dtype)
        sd[k] = v
    twin.load_state_dict(sd)
    idx = torch.randint(0, 61, (3, 16), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.equal(model(idx)[0], twin(idx)[0])
        assert torch.equal(model.generate(idx[:, :5], 8), twin.generate(idx[:, :5], 8))


def test_w8_twins_follow_the_weight():
    """``w8_weights``: a twin per snapped weight; K no multiple of 8 and a weight that no longer equals
    its dequantized twin give None, the latter for good until ``quantize_int8_`` starts over."""
    model = _tiny()
    model.quantize_int8_()
    get = gen.w8_weights(model)
    w = model.transformer.h[0].mlp.c_fc.weight
    q, s = get(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and torch.equal(dequantize_rows(q, s, w.dtype), w)
    assert get(w)[0] is q  # cached under the stamp
    assert get(torch.zeros(4, 12)) is None
    name = "transformer.h.0.mlp.c_fc.weight"
    assert gen.w8_status(model)[name] is True and gen.w8_status(model)["lm_head.weight"] is None
    with torch.no_grad():
        w.mul_(1.0)  # a new version, the same values: the twin is rebuilt
    assert get(w) is not None and get(w)[0] is not q
    with torch.no_grad():
        w.add_(1e-3)
    assert get(w) is None and gen.w8_status(model)[name] is False
    with torch.no_grad():
        q2, s2 = quantize_rows(w)
        w.copy_(dequantize_rows(q2, s2, w.dtype))
    assert get(w) is None  # for good
    model.quantize_int8_()
    assert get(w) is not None and gen.w8_status(model)[name] is True


# ---------------------------------------------------------------------- the kernel's arithmetic, restated
def _bf_np(t):
    return t.to(BF).float().numpy()


@pytest.mark.parametrize("lanes", [O.LANES, O.WIDE_LANES])
@pytest.mark.parametrize("B,N,K", [(3, 23, 520), (8, 12, 4104), (1, 5, 8)], ids=str)
def test_restatement_scale_commutes_with_the_chain(lanes, B, N, K):
    g = torch.Generator().manual_seed(K + B)
    x = _bf_np(torch.randn(B, K, generator=g))
    w = torch.randn(N, K, generator=g) * 0.05
    w[1] = 0
    q, s = quantize_rows(w)
    qf, sf = q.float().numpy(), s.numpy()
    wd = _bf_np(dequantize_rows(q, s, BF))
    assert np.array_equal(wd, sf[:, None] * qf)
    bias, resid = _bf_np(torch.randn(N, generator=g)), _bf_np(torch.randn(B, N, generator=g))
    w8 = sf[None, :] * O.fold(O.lane_sums(x, qf, lanes), lanes)
    bf = O.fold(O.lane_sums(x, wd, lanes), lanes)
    assert w8.dtype == np.float32 and np.array_equal(w8.view(np.uint32), bf.view(np.uint32))
    for epi in (0, 1, 3):
        a = O.epilogue(w8, epi, bias if epi else None, resid)[0]
        b = O.epilogue(bf, epi, bias if epi else None, resid)[0]
        assert np.array_equal(a, b), f"epilogue {epi}"
