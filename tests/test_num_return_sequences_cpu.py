"""``generate(num_return_sequences=N)`` on the CPU is the repeated batch, exactly: seeded, greedy and
``seed=None`` under a fixed torch seed, with and without the cache."""
import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig

MODES = {"seeded": dict(do_sample=True, seed=11, top_k=20), "greedy": {}, "unseeded": dict(do_sample=True)}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(embed_drop=0.0, resid_drop=0.0, attn_drop=0.0, n_layer=2, n_head=2, n_embed=32, vocab_size=64,
                    block_size=24)
    return GPT(cfg, verbose=False).eval()


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("mode", list(MODES))
def test_equals_the_repeated_batch(model, mode, use_cache):
    idx = torch.randint(0, 64, (2, 5), generator=torch.Generator().manual_seed(1))
    kw = dict(MODES[mode], use_cache=use_cache, return_logprobs=True)
    torch.manual_seed(5)
    got, lp = model.generate(idx, 7, num_return_sequences=3, **kw)
    torch.manual_seed(5)
    want, lp_want = model.generate(idx.repeat_interleave(3, 0), 7, **kw)
    assert got.shape == (6, 12) and torch.equal(got, want) and torch.equal(lp, lp_want)
    if mode == "seeded":  # the batch row is hashed into the draw: the rows of a prompt diverge
        assert not torch.equal(got[0], got[1])


def test_below_one_is_a_value_error(model):
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(torch.zeros(1, 3, dtype=torch.long), 2, num_return_sequences=0)
