"""``generate_batch(reuse_cache=...)`` where it has no effect (the CPU) and where it is refused (``kv_cache="int8"``)."""
import pytest
import torch

from test_prefix_reuse_cpu import _model


def _prompts():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 64, (n,), generator=g) for n in (9, 3, 14)]


def test_cpu_reuse_cache_changes_nothing():
    model = _model()
    want, lens = model.generate_batch(_prompts(), 8)
    for _ in range(2):
        got, glens = model.generate_batch(_prompts(), 8, reuse_cache=True)
        assert torch.equal(got, want) and torch.equal(glens, lens)


def test_int8_cache_refuses_reuse():
    with pytest.raises(ValueError, match="reuse_cache"):
        _model().generate_batch(_prompts(), 2, kv_cache="int8", reuse_cache=True)
