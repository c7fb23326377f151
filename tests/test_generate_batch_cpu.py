"""``generate_batch`` on the CPU, the executable definition of ragged batched generation: every row
is the single-prompt cache path applied to that row alone, with the batch row index and the row's
own column as the draw counter; a row stops after the stop token."""
import pytest
import torch

from mingpt_distributed_amd.models import GPT, GPTConfig, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops import reference as R

V, BS = 1000, 64
LENS = [1, 5, 17, 3]
NEW = 12
SAMPLED = dict(do_sample=True, top_k=20, temperature=0.8, seed=4321)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=V, block_size=BS, embed_drop=0.0,
                    resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).eval()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, V, (n,), generator=g) for n in LENS]


def _single(model, prompt, b, n, kw):
    """The existing single-prompt CPU cache path on one row, as batch row b."""
    with torch.no_grad():
        cache = gen._CpuCache(model, prompt.view(1, -1))
        out, logits = prompt.clone(), cache.logits
        for _ in range(n):
            col = out.numel()
            if kw.get("do_sample"):
                nxt = R.sample_gumbel(logits, kw["temperature"], kw["top_k"], kw["seed"], col, row0=b)
            else:
                nxt = logits.argmax(-1, keepdim=True)
            out = torch.cat([out, nxt.view(1)])
            logits = cache.step(nxt, col)
    return out


@pytest.mark.parametrize("kw", [{}, SAMPLED], ids=["greedy", "seeded"])
def test_mixed_lengths(model, prompts, kw):
    tokens, lengths = generate_batch(model, prompts, NEW, pad_token=7, **kw)
    assert tokens.shape == (4, max(LENS) + NEW) and tokens.dtype == torch.long
    assert lengths.tolist() == [n + NEW for n in LENS] and lengths.dtype == torch.long
    for b, p in enumerate(prompts):
        want = _single(model, p, b, NEW, kw)
        assert torch.equal(tokens[b, :lengths[b]], want), f"row {b}"
        assert (tokens[b, lengths[b]:] == 7).all()
    if not kw:  # greedy on one row alone is the single-prompt generate()
        assert torch.equal(tokens[2, :17 + NEW], model.generate(prompts[2].view(1, -1), NEW)[0])
    m_tokens, m_lengths = model.generate_batch(prompts, NEW, pad_token=7, **kw)
    assert torch.equal(m_tokens, tokens) and torch.equal(m_lengths, lengths)


def _pick_eos(tokens, lens, new):
    """A token some row produced at generated step >= 3 that is new to that row's generated part."""
    for b, n in enumerate(lens):
        gen_part = tokens[b, n:n + new].tolist()
        for j in range(3, new):
            if gen_part[j] not in gen_part[:j]:
                return gen_part[j]
    raise AssertionError("no usable stop token")


@pytest.mark.parametrize("kw", [{}, SAMPLED], ids=["greedy", "seeded"])
def test_eos(model, prompts, kw):
    full, _ = generate_batch(model, prompts, NEW, **kw)
    eos = _pick_eos(full, LENS, NEW)
    tokens, lengths = generate_batch(model, prompts, NEW, eos_token=eos, pad_token=3, **kw)
    stopped = 0
    for b, n in enumerate(LENS):
        gen_part = full[b, n:n + NEW].tolist()
        keep = gen_part.index(eos) + 1 if eos in gen_part else NEW
        stopped += keep < NEW
        assert int(lengths[b]) == n + keep
        assert torch.equal(tokens[b, :n + keep], full[b, :n + keep])
        assert (tokens[b, n + keep:] == 3).all()
    assert stopped >= 1


def test_input_forms(model, prompts):
    a_tok, a_len = generate_batch(model, prompts, NEW, **SAMPLED)
    idx = torch.full((4, 20), 999)  # wider than the longest prompt, arbitrary padding
    for b, p in enumerate(prompts):
        idx[b, :p.numel()] = p
    b_tok, b_len = generate_batch(model, (idx, torch.tensor(LENS)), NEW, **SAMPLED)
    assert torch.equal(a_tok, b_tok) and torch.equal(a_len, b_len)
    idx[0, 1:] = -5  # not even token ids: positions past the length are ignored
    c_tok, c_len = generate_batch(model, (idx, LENS), NEW, **SAMPLED)
    assert torch.equal(a_tok, c_tok) and torch.equal(a_len, c_len)


def test_unseeded_sampling_draws_a_seed(model, prompts):
    torch.manual_seed(5)
    a = generate_batch(model, prompts, 4, do_sample=True, top_k=10)[0]
    torch.manual_seed(5)
    b = generate_batch(model, prompts, 4, do_sample=True, top_k=10)[0]
    assert torch.equal(a, b)


def test_zero_new_tokens(model, prompts):
    tokens, lengths = generate_batch(model, prompts, 0, pad_token=1)
    assert tokens.shape == (4, 17) and lengths.tolist() == LENS
    assert torch.equal(tokens[1], torch.cat([prompts[1], torch.ones(12, dtype=torch.long)]))


def test_generate_project_takes_several_prompts(tmp_path):
    """projects/generate/generate.py: repeated --prompt and --prompt-file go through one
    generate_batch call (token-id prompts here: no BPE vocabulary in the test environment)."""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "projects", "generate",
                        "generate.py")
    spec = importlib.util.spec_from_file_location("generate_project", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    f = tmp_path / "prompts.txt"
    f.write_text("4 5 6 7 8\n\n9\n")
    outs = mod.main(["--random-init", "--model-type", "gpt-micro", "--num-samples", "2", "--steps", "4", "--device",
                     "cpu", "--prompt", "1 2 3", "--prompt-file", str(f)])
    assert len(outs) == 6
    if isinstance(outs[0], list):  # no vocabulary: the rows are token ids
        assert [o[:-4] for o in outs] == [[1, 2, 3]] * 2 + [[4, 5, 6, 7, 8]] * 2 + [[9]] * 2
        assert all(len(o) == n + 4 for o, n in zip(outs, (3, 3, 5, 5, 1, 1)))


@pytest.mark.parametrize("bad", [
    dict(max_new_tokens=BS - 17 + 1),
    dict(prompts="empty"),
    dict(pad_token=V), dict(pad_token=-1),
    dict(eos_token=V), dict(eos_token=-1),
    dict(top_k=0, do_sample=True, seed=1),
    dict(temperature=0.0, do_sample=True, seed=1),
], ids=["block_size", "empty_prompt", "pad_high", "pad_neg", "eos_high", "eos_neg", "top_k", "temperature"])
def test_value_errors(model, prompts, bad):
    kw = dict(max_new_tokens=4)
    kw.update(bad)
    p = kw.pop("prompts", prompts)
    if p == "empty":
        p = prompts[:2] + [torch.zeros(0, dtype=torch.long)]
    with pytest.raises(ValueError):
        generate_batch(model, p, **kw)
    generate_batch(model, prompts, BS - 17)  # exactly block_size is fine
