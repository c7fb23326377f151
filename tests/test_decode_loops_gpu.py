"""The decode loops' host code (models/generation.py) as a whole: which loops the entry points build
under which keys, that a second call replays the first one's graphs to the same bits -- for the seeded
loops the test that the draw counter is uploaded again with unchanged words -- that the parameter
blocks serve other settings through the same graphs and come back, and that ``score`` builds no
decode state.  What each loop computes is checked against the rules in the loops' own test files."""
import copy
import gc

import pytest
import torch

from _guard import bit_equal
from mingpt_distributed_amd.models import GPT, GPTConfig, score

pytestmark = pytest.mark.gpu

NEW, LENS, SEED = 20, [1, 5, 17, 3], 1234567
PROC = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, no_repeat_ngram_size=3)
PROC2 = dict(repetition_penalty=1.1, presence_penalty=0.0, frequency_penalty=0.4, no_repeat_ngram_size=2)
SAMPLED = dict(do_sample=True, seed=SEED, temperature=0.8, top_k=20, top_p=0.9)
SAMPLED2 = dict(do_sample=True, seed=SEED, temperature=1.3, top_k=20, top_p=0.6)
SLOTS = ("_mg_decode_cache", "_mg_beam_cache", "_mg_spec_cache")
FORMS = [(proc, lp) for proc in (False, True) for lp in (False, True)]
FORM_IDS = ["plain", "lp", "proc", "proc_lp"]


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    """A model and its decode state refer to each other: collect dropped ones here, not inside a
    later test's capture."""
    yield
    gc.collect()


def _model(V=1000):
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=V, block_size=64, embed_drop=0.0, resid_drop=0.0,
                    attn_drop=0.0)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def tiny():
    return _model()


def _idx(V=1000):
    return torch.randint(0, V, (4, 5), generator=torch.Generator().manual_seed(2)).cuda()


def _rows(V=1000):
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, V, (n,), generator=g).cuda() for n in LENS]


def _key(base, proc, lp):
    return base + ("_proc" if proc else "") + ("_lp" if lp else "")


def _generate(sampled, proc, lp, samp=SAMPLED, procs=PROC):
    """(call, slot, loop key) of one ``generate`` form."""
    kw = dict(samp if sampled else {}, return_logprobs=lp, **(procs if proc else {}))
    return (lambda m: m.generate(_idx(), NEW, **kw)), SLOTS[0], _key("sample" if sampled else "greedy", proc, lp)


def _batch(sampled, proc, lp, samp=SAMPLED, procs=PROC):
    """(call, slot, loop key) of one ``generate_batch`` form."""
    kw = dict(samp if sampled else {}, return_logprobs=lp, **(procs if proc else {}))
    return (lambda m: m.generate_batch(_rows(), NEW, **kw)), SLOTS[0], (_key("ragged", proc, lp), not sampled)


def _beam():
    return (lambda m: m.generate_beam(_idx()[:1], NEW, 4)), SLOTS[1], ("beam", 4)


def _spec():
    return (lambda m: m.generate_speculative(_idx()[:1], NEW, draft_len=3)), SLOTS[2], ("spec", 4)


CASES = {f"{name}-{'seeded' if s else 'greedy'}-{fid}": (make, s, proc, lp)
         for name, make in (("generate", _generate), ("batch", _batch)) for s in (False, True)
         for (proc, lp), fid in zip(FORMS, FORM_IDS)}


def _graphs(model):
    return {(slot, key): loop.graph for slot in SLOTS if slot in model.__dict__
            for key, loop in model.__dict__[slot]._loops.items()}


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(bit_equal(x, y) for x, y in zip(a, b))


def _twice(model, call, slot, key):
    """``call`` twice: the second result is the first bit for bit and every loop the model has
    keeps its graph.  Returns the result."""
    a = call(model)
    a = tuple(t.clone() for t in a) if isinstance(a, tuple) else a.clone()
    graphs = _graphs(model)
    assert graphs[(slot, key)] is not None
    assert _same(call(model), a)
    again = _graphs(model)
    assert again.keys() == graphs.keys() and all(again[k] is g for k, g in graphs.items())
    return a


def test_loop_table():
    """Every entry point once on a fresh model: the three states hold exactly the loops of the
    table in the module docstring of generation.py."""
    model = _model()
    for make, s, proc, lp in CASES.values():
        make(s, proc, lp)[0](model)
    model.generate(_idx(), 3, do_sample=True)  # torch's generator draws on the host: the "step" loop
    _beam()[0](model)
    _spec()[0](model)
    rect = {_key(base, proc, lp) for base in ("greedy", "sample") for proc, lp in FORMS}
    ragged = {(_key("ragged", proc, lp), greedy) for proc, lp in FORMS for greedy in (True, False)}
    assert set(model._mg_decode_cache._loops) == {"step"} | rect | ragged
    assert set(model._mg_beam_cache._loops) == {("beam", 4)}
    assert set(model._mg_spec_cache._loops) == {("spec", 4)}
    assert "lp" in model._mg_decode_cache.ragged_state()


def test_ragged_state_has_no_lp_until_asked():
    """The ragged state's ``lp`` buffer is allocated by the first call that asks for log-probabilities."""
    model = _model()
    _batch(True, True, False)[0](model)
    assert "lp" not in model._mg_decode_cache.ragged_state()
    _batch(True, True, True)[0](model)
    assert "lp" in model._mg_decode_cache.ragged_state()


@pytest.mark.parametrize("case", list(CASES))
def test_twice(tiny, case):
    """A second call with the same arguments: the same bits from the same graphs.  A seeded
    ``generate`` whose sample block were not uploaded again would draw with the counter its own
    replays advanced (the ragged draws count by the row's position instead)."""
    make, s, proc, lp = CASES[case]
    call, slot, key = make(s, proc, lp)
    _twice(tiny, call, slot, key)
    assert key in tiny.__dict__[slot]._loops


@pytest.mark.parametrize("make", [_beam, _spec], ids=["beam", "spec"])
def test_twice_beam_spec(tiny, make):
    """Beam search at W = 4 and speculative decoding at draft_len 3 on one prompt, twice."""
    _twice(tiny, *make())


def test_twice_fused_argmax():
    """V = 8200, the smallest vocabulary whose greedy loop is the LM head's fused argmax."""
    model = _model(8200)
    call = lambda m: m.generate(_idx(8200), NEW)
    _twice(model, call, SLOTS[0], "greedy")
    assert model._mg_decode_cache._loops["greedy"].state["part"] is not None
    assert set(model._mg_decode_cache._loops) == {"greedy"}


REUSE = {k: v for k, v in CASES.items() if v[1] or (v[0] is _batch and v[2])}  # seeded, or ragged with processors


@pytest.mark.parametrize("case", list(REUSE))
def test_parameter_blocks_reused(tiny, case):
    """Another temperature, top_p and processor settings through the same captured steps: other
    tokens, the same graphs, and the first settings afterwards give the first tokens again."""
    make, s, proc, lp = REUSE[case]
    call, slot, key = make(s, proc, lp)
    other = make(s, proc, lp, SAMPLED2, PROC2)[0]
    first = lambda r: r[0] if isinstance(r, tuple) else r
    a = _twice(tiny, call, slot, key)
    graphs = _graphs(tiny)
    b = other(tiny)
    assert first(b).shape == first(a).shape and not torch.equal(first(b), first(a))
    assert _same(call(tiny), a)
    again = _graphs(tiny)
    assert again.keys() == graphs.keys() and all(again[k] is g for k, g in graphs.items())


def test_score_builds_no_decode_state():
    """``score`` on a model that has never decoded leaves no decode state on it, and agrees with the
    CPU path: the tolerance of test_logprob_decode_gpu.py for ``score`` against another GEMM path,
    2 * (2e-2 + 2e-2 * max |logit| of the row)."""
    model = _model()
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, 1000, (4, 24), generator=g)
    lengths = torch.tensor([24, 5, 17, 2])
    sc = score(model, tokens.cuda(), lengths)
    assert not any(slot in model.__dict__ for slot in SLOTS)
    ref = copy.deepcopy(model).float().cpu()
    want = score(ref, tokens, lengths)
    with torch.no_grad():
        big = ref(tokens)[0].abs().amax(-1)  # [B, T]: row (b, j - 1) predicts column j
    tol = 2 * (2e-2 + 2e-2 * big[:, :-1])
    err = (sc.cpu() - want)[:, 1:].abs()
    print(f"max |gpu - cpu| {float(err.max()):.4g}, allowed at least {float(tol.min()):.4g}")
    assert (err <= tol).all() and (sc[:, 0] == 0).all()
    assert not any(slot in model.__dict__ for slot in SLOTS)
