"""``generate(kv_cache="int8", reuse_cache=True)`` on the GPU (``_mg_kv8_cache``, ``attention_extend_kv8``): the
extension is taken and recorded; tokens and logits are bit-equal with ``_KV8_DECODE`` off (``kv8_store`` +
``attention_extend``) and as close to the float32 CPU KV8 model as a fresh int8 prefill's (factor two, as on bf16)."""
import pytest
import torch

from _guard import bit_equal
from mingpt_distributed_amd.models import GPT
from mingpt_distributed_amd.models import generation as gen
from test_prefix_reuse_gpu import NEW, _model, _prompt  # the small model: 2 layers, n_embed 1280, block_size 96

pytestmark = pytest.mark.gpu
SLOT, KW = "_mg_kv8_cache", dict(kv_cache="int8", reuse_cache=True)


def _extended(model, idx, P, n):  # generate(idx, n, **KW) on a fresh KV8 state that holds idx[:, :P]: (tokens, state)
    model.__dict__.pop(SLOT, None)
    model.generate(idx[:, :P], 1, **KW)
    return model.generate(idx, n, **KW), model.__dict__[SLOT]


# (B, P, Tq): the skinny route, the rows GEMM (also against the float32 KV8 model), the MFMA GEMM
@pytest.mark.parametrize("B,P,Tq,against_f32", [(1, 40, 3, False), (2, 30, 20, True), (2, 8, 60, False)])
def test_extension_is_taken_and_equals_the_bf16_kernels(B, P, Tq, against_f32, monkeypatch):
    monkeypatch.setattr(gen, "_REUSE_KV8_GATE", False)
    model, idx = _model(), _prompt(B, P + Tq)
    out, st = _extended(model, idx, P, NEW)
    assert st.kv8 and st.kq and st.reused == P
    assert st.nheld == P + Tq + NEW - 1 and torch.equal(st.held[:, :st.nheld], out[:, :-1])
    st = _extended(model, idx, P, 1)[1]  # one token: ``logits`` are still the extension's
    logits = st.logits.clone()
    if against_f32:
        cpu = GPT(model.config, verbose=False).eval()  # the same bf16-valued weights in float32
        cpu.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            ref = gen._CpuCache(cpu, idx.cpu(), kv8=True).logits
        model.generate(idx, 1, kv_cache="int8")  # a fresh int8 prefill of the same state
        assert model.__dict__[SLOT] is st and st.reused == 0
        e_fresh = float((st.logits.float().cpu() - ref).abs().max())
        e_ext = float((logits.float().cpu() - ref).abs().max())
        print(f"PREFIX kv8 logits: max |fresh - ref| {e_fresh:.5f}, max |extended - ref| {e_ext:.5f}")
        assert e_ext <= 2 * e_fresh, (e_ext, e_fresh)
    monkeypatch.setattr(gen, "_KV8_DECODE", False)  # the same model on kv8_store + attention_extend
    out_bf, st_bf = _extended(model, idx, P, NEW)
    assert st_bf.caches and not st_bf.kq and st_bf.reused == P and torch.equal(out_bf, out)
    assert bit_equal(_extended(model, idx, P, 1)[1].logits, logits)


def test_a_flip_of_the_kernel_switch_prefills(monkeypatch):
    monkeypatch.setattr(gen, "_REUSE_KV8_GATE", False)
    model, idx = _model(), _prompt(2, 50, seed=5)
    model.__dict__.pop(SLOT, None)
    model.generate(idx[:, :30], 1, **KW)
    st = model.__dict__[SLOT]
    assert st.nheld == 30
    monkeypatch.setattr(gen, "_KV8_DECODE", False)  # the storage is swapped: the record is of the other buffers
    model.generate(idx, NEW, **KW)
    assert model.__dict__[SLOT] is st and st.reused == 0 and st.caches and not st.kq


def test_default_is_untouched():
    model, idx = _model(), _prompt(2, 50, seed=6)
    model.__dict__.pop(SLOT, None)
    a = model.generate(idx, NEW, kv_cache="int8")
    st = model.__dict__[SLOT]
    graph = st._loops["greedy"].graph
    assert st.nheld == 0 and graph is not None
    model.generate(idx, NEW, **KW)  # leaves a record ...
    assert st.nheld == 50 + NEW - 1
    b = model.generate(idx, NEW, kv_cache="int8")  # ... that a call without the argument clears
    assert model.__dict__[SLOT] is st and st.nheld == 0 and st.reused == 0
    assert torch.equal(a, b) and st._loops["greedy"].graph is graph
