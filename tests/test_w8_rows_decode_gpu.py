"""W8 decode at 9..64 rows: on a model snapped by ``quantize_int8_``, with the module switch ``_W8_ROWS`` set (it is
off by default, PERF.md 'W8 rows'), the decode loops' step bodies run every projection and the LM head on
``gemm_rows_w8`` and give the outputs and stored logits of ``gemm_rows`` on the same model, bit for bit."""
import pytest
import torch

from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
L, V = 2, 1000
_tok = lambda *shape: torch.randint(0, V, shape, generator=torch.Generator().manual_seed(sum(shape))).cuda()
CALLS = {"generate, 9 rows": lambda m: m.generate(_tok(9, 12), 24),
         "generate_batch, 9 ragged rows, int8 KV cache": lambda m: m.generate_batch(
             [_tok(n) for n in (1, 7, 3, 12, 2, 9, 5, 11, 4)], 24, kv_cache="int8"),
         "generate_beam 3 x 4": lambda m: m.generate_beam(_tok(3, 12), 16, 4)}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, n_layer=L, n_head=2, n_embed=128, vocab_size=V,
                    block_size=96)
    m = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    m.quantize_int8_()
    return m


@pytest.mark.parametrize("name", list(CALLS))
def test_rows_decode_on_and_off(model, name, monkeypatch):
    C, per, calls, runs = ext(), 4 * L + 1, {"gemm_rows": 0, "gemm_rows_w8": 0}, {}
    for k in calls:
        def counted(*a, _k=k, _real=getattr(C, k), **kw):
            calls[_k] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(C, k, counted)
    monkeypatch.setattr(gen, "_W8_ROWS", True)
    for w8 in (True, False):  # fresh decode states under each setting of the switch
        monkeypatch.setattr(gen, "_W8_DECODE", w8)
        out = CALLS[name](model)
        states = [model.__dict__.pop(k) for k in gen._STATE_SLOTS if k in model.__dict__]
        logits = [lp.logits for c in states for lp in c._loops.values() if lp.logits is not None]
        runs[w8] = [t.clone() for t in (*(out if isinstance(out, tuple) else (out,)), *logits)], dict(calls)
        calls.update(gemm_rows=0, gemm_rows_w8=0)
    (on, con), (off, coff) = runs[True], runs[False]
    assert con["gemm_rows"] == 0 and con["gemm_rows_w8"] >= per and con["gemm_rows_w8"] % per == 0, con
    assert coff == {"gemm_rows": con["gemm_rows_w8"], "gemm_rows_w8": 0}, (con, coff)
    assert len(on) == len(off) >= 2 and all(bit_equal(a, b) for a, b in zip(on, off)), "outputs or stored logits differ"
