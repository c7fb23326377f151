"""``reuse_cache`` where it has no effect (the CPU) and where it is refused (``kv_cache="int8"``)."""
import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig


def _model():
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, n_layer=2, n_head=2, n_embed=32, vocab_size=64,
                    block_size=32)
    return GPT(cfg, verbose=False).eval()


def test_cpu_reuse_cache_changes_nothing():
    model = _model()
    idx = torch.randint(0, 64, (2, 9), generator=torch.Generator().manual_seed(1))
    want = model.generate(idx, 8)
    assert torch.equal(model.generate(idx, 8, reuse_cache=True), want)
    assert torch.equal(model.generate(idx, 8, reuse_cache=True, use_cache=False), want)


def test_int8_cache_refuses_reuse():
    with pytest.raises(ValueError, match="reuse_cache"):
        _model().generate(torch.zeros(1, 4, dtype=torch.long), 2, kv_cache="int8", reuse_cache=True)
