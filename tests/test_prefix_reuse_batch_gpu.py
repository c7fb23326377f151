"""``generate_batch(reuse_cache=True)`` on the GPU: each row keeps the prefix of its prompt that its own KV cache
rows still hold and runs only the tokens behind it (``_GpuCache.extend_ragged``, ``attention_extend_ragged``).  The
extension is taken and leaves the right per-row record on every GEMM route; its logits are as close to a float32
CPU forward as the padded prefill's (within a factor of two: both round the same quantities to bf16, in other
orders); greedy tokens follow the same call without the argument up to a near-tie; and without the argument
nothing changes.  The model is that of tests/test_prefix_reuse_gpu.py."""
import pytest
import torch

from mingpt_distributed_amd.models import GPT
from mingpt_distributed_amd.models import generation as gen
from test_prefix_reuse_gpu import V, _model

pytestmark = pytest.mark.gpu

NEW = 4
LENS0 = [12, 20, 9, 1]  # the histories' prompts; two tokens are generated behind each
CUT, FRESH = (2, 9), 3  # row 2's held prefix is cut short at column 9; row 3 shares nothing with its record
# the new tokens per row, by the GEMM route of the packed rows (the cut and the fresh row rerun more than their
# turn): 7 rows -- the skinny GEMM; 27 -- the rows GEMM; 103 -- the MFMA GEMM
TURNS = {"gemv": [1, 1, 1, 1], "rows": [5, 9, 4, 6], "mfma": [30, 40, 20, 10]}


def _setup(model, tq, seed=3):
    """(the second turn's prompts, the P_b the ragged extension should keep) on a state that holds the first
    turn: row b's prompt is its first output less the last token (what its cache holds) plus tq[b] new tokens."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda n: torch.randint(0, V, (n,), generator=g).cuda()
    model.__dict__.pop("_mg_decode_cache", None)
    out, lens = model.generate_batch([rnd(n) for n in LENS0], 2, reuse_cache=True)
    prompts = [torch.cat([out[b, :n - 1], rnd(t)]) for b, (n, t) in enumerate(zip(lens.tolist(), tq))]
    keep = [n - 1 for n in lens.tolist()]
    for b, col in (CUT, (FRESH, 0)):
        prompts[b][col] = (prompts[b][col] + 1) % V
        keep[b] = col
    return prompts, keep


@pytest.mark.parametrize("route", list(TURNS))
def test_extension_is_taken_and_recorded(route, monkeypatch):
    monkeypatch.setattr(gen, "_REUSE_BATCH_GATE", False)
    model, tq = _model(), TURNS[route]
    prompts, keep = _setup(model, tq)
    st = model._mg_decode_cache
    assert st._route(sum(p.numel() - k for p, k in zip(prompts, keep))) == route
    out, lens = model.generate_batch(prompts, NEW, reuse_cache=True)
    assert model._mg_decode_cache is st and st.reused == keep
    held = [n - 1 for n in lens.tolist()]
    assert st.hlen == held and st.nheld == min(held)
    assert all(torch.equal(st.held[b, :n], out[b, :n]) for b, n in enumerate(held))
    monkeypatch.undo()  # the gate as shipped: the path taken is what the rule says
    prompts, keep = _setup(model, tq)
    model.generate_batch(prompts, NEW, reuse_cache=True)
    pays = gen._reuse_batch_pays(keep, [p.numel() - k for p, k in zip(prompts, keep)])
    assert model._mg_decode_cache.reused == (keep if pays else 0)


def test_logits_against_float32(monkeypatch):
    monkeypatch.setattr(gen, "_REUSE_BATCH_GATE", False)
    model = _model()
    cpu = GPT(model.config, verbose=False).eval()  # the same bf16-valued weights in float32
    cpu.load_state_dict({k: v.float().cpu() for k, v in model.state_dict().items()})
    prompts, keep = _setup(model, TURNS["rows"], seed=4)
    with torch.no_grad():
        ref = torch.cat([cpu(p.cpu().view(1, -1))[0][:, -1] for p in prompts])
    model.generate_batch(prompts, 1, reuse_cache=True)
    assert model._mg_decode_cache.reused == keep
    ext = model._mg_decode_cache.logits.float().cpu()
    model.generate_batch(prompts, 1)
    assert model._mg_decode_cache.reused == 0
    e_fresh = float((model._mg_decode_cache.logits.float().cpu() - ref).abs().max())
    e_ext = float((ext - ref).abs().max())
    print(f"PREFIX batch logits: max |fresh - ref| {e_fresh:.5f}, max |extended - ref| {e_ext:.5f}")
    assert e_ext <= 2 * e_fresh, (e_ext, e_fresh)


def test_greedy_follows_the_call_without_the_argument(monkeypatch):
    """The rule of test_decode_wide_gpu.py::test_greedy_follows_the_uncached_reference: a row may leave the
    reference only where its two best logits are closer than 0.05, compared up to that column."""
    monkeypatch.setattr(gen, "_REUSE_BATCH_GATE", False)
    model, n = _model(), 30
    prompts, keep = _setup(model, TURNS["rows"], seed=5)
    got, glens = model.generate_batch(prompts, n, reuse_cache=True)
    assert model._mg_decode_cache.reused == keep
    want, wlens = model.generate_batch(prompts, n)
    assert torch.equal(glens, wlens)
    for b, L in enumerate(wlens.tolist()):
        diff = (got[b, :L] != want[b, :L]).nonzero()
        if diff.numel():
            col = int(diff[0])
            top = model(want[b:b + 1, :col])[0][0, -1].float().topk(2).values
            gap = float(top[0] - top[1])
            print(f"row {b} leaves the padded prefill's call at column {col}: top-two gap {gap:.4f}")
            assert gap < 0.05, f"row {b} differs at column {col} where the gap is {gap:.4f}"


def test_default_is_untouched(monkeypatch):
    monkeypatch.setattr(gen, "_REUSE_BATCH_GATE", False)
    model = _model()
    prompts, keep = _setup(model, TURNS["rows"], seed=6)
    a, alens = model.generate_batch(prompts, NEW)
    st = model._mg_decode_cache
    graph = st._loops[("ragged", True)].graph
    assert st.hlen is None and st.nheld == 0
    model.generate_batch(prompts, NEW, reuse_cache=True)  # a padded prefill that leaves a record ...
    assert st.reused == 0 and st.hlen is not None
    model.generate_batch(prompts, NEW, reuse_cache=True)  # ... which the next call extends ...
    assert st.reused == [p.numel() - 1 for p in prompts]
    b, blens = model.generate_batch(prompts, NEW)  # ... and a call without the argument clears
    assert model._mg_decode_cache is st and st.nheld == 0 and st.hlen is None and st.reused == 0
    assert torch.equal(a, b) and torch.equal(alens, blens)
    assert graph is not None and st._loops[("ragged", True)].graph is graph
