"""Ragged batched generation on the GPU: ``generate_batch`` and the device loop behind it
(``_GpuCache.ragged``: per-row positions and finished flags in device memory, one captured step),
against ``generate``, the rule restated in numpy (tests/_sample_oracle.py) and the rectangular
B = 1 decode path."""
import gc

import pytest
import torch

import _sample_oracle as O
from _guard import guarded
from mingpt_distributed_amd.models import GPT, GPTConfig, generate_batch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
BS = 64
LENS = [1, 5, 17, 3]
STEPS = 30
SEED, TEMP, TOPK = 1234567, 0.8, 20

# Check 3's tolerance: twice the max |logits difference| between the rectangular decode path at
# B rows and at B = 1 (equal-length prompts, teacher-forced with the B-row path's greedy tokens,
# same model), measured on the parent commit for each model of this file (PERF.md 'Ragged
# batched generation'):
#   tiny      B = 4, lengths 1 / 3 / 5 / 17, 30 steps                  0 each  -> equality required
#   split256  block_size 320, B = 3, lengths 3 / 130 / 250, 20 steps    0 each  -> equality required
#   split128  block_size 192, 4 heads, B = 9 (MFMA GEMM against the B = 1 skinny GEMM), lengths
#             120 / 128 / 135, 16 steps: 0.0078125 / 0.00390625 / 0.0078125 (logits std 0.23)
RECT_DIFF = {"tiny": 0.0, "split256": 0.0, "split128": 0.0078125}


@pytest.fixture(autouse=True)
def _collect_dropped_models():
    """A model and its decode state refer to each other, so the models these tests drop (and their
    hipGraphs) wait for the cycle collector: run it here, not inside a later test's capture."""
    yield
    gc.collect()


def _model(vocab, n_head=2, block_size=BS):
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=n_head, n_embed=128, vocab_size=vocab, block_size=block_size,
                    embed_drop=0.0, resid_drop=0.0, attn_drop=0.0)
    return GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()


def _prompts(lens, vocab=1000, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).cuda() for n in lens]


def _padded(prompts, fill=0):
    idx = torch.full((len(prompts), max(p.numel() for p in prompts)), fill, dtype=torch.long, device="cuda")
    for b, p in enumerate(prompts):
        idx[b, :p.numel()] = p
    return idx, torch.tensor([p.numel() for p in prompts], device="cuda")


def _start(model, prompts, words, greedy, bs):
    idx, lengths = _padded(prompts)
    cache = gen._GpuCache(model, idx, bs, last=lengths - 1)
    first = cache.logits.float().clone()
    st = cache.ragged_start(idx, lengths, words, greedy)
    return cache, st, first


def _drive(model, prompts, n, greedy, bs=BS, seed=SEED):
    """The ragged loop one step per call.  Returns per step (the first pick is step 0): the logits
    the pick read, the position and input token of every row going in, and the token coming out."""
    words = gen._ragged_words(seed, TEMP, TOPK, None)
    with torch.no_grad():
        cache, st, first = _start(model, prompts, words, greedy, bs)
        lens = torch.tensor([p.numel() for p in prompts])
        rec = [dict(logits=first.cpu(), pos_in=lens - 1, tok_in=None, tok_out=st["tok"].view(-1).cpu())]
        for _ in range(n):
            pos_in, tok_in = st["pos"].cpu().long(), st["tok"].view(-1).cpu()
            cache.ragged(1, words, greedy)
            rec.append(dict(logits=cache._loops[("ragged", greedy)].logits.float().cpu(), pos_in=pos_in, tok_in=tok_in,
                            tok_out=st["tok"].view(-1).cpu()))
        final = {k: st[k].clone() for k in ("seq", "pos", "done")}
    return rec, final


@pytest.fixture(scope="module")
def tiny():
    return _model(1000)


@pytest.fixture(scope="module", params=[True, False], ids=["greedy", "seeded"])
def driven(request, tiny):
    prompts = _prompts(LENS)
    rec, final = _drive(tiny, prompts, STEPS, request.param)
    return tiny, prompts, request.param, rec, final


def _check_pick(rec, greedy, seed=SEED):
    """Check 2: every token is the rule's pick from the logits its step produced."""
    skipped = draws = 0
    for j, r in enumerate(rec):
        logits = r["logits"].numpy()
        for b in range(logits.shape[0]):
            got = int(r["tok_out"][b])
            if greedy:
                assert got == int(r["logits"][b].argmax()), f"step {j} row {b}"
                continue
            want, gap = O.sample(logits[b:b + 1], TEMP, TOPK, seed, int(r["pos_in"][b]) + 1, row0=b)
            if j > 0:
                draws += 1
                skipped += int(gap[0] < MARGIN)
            if gap[0] >= MARGIN:
                assert got == int(want[0]), f"step {j} row {b}: device {got}, rule {want[0]}, gap {gap[0]}"
    return skipped, draws


def _check_logits(model, prompts, rec, bs, tol):
    """Check 3: row b's logits at every step are the rectangular B = 1 path's on the row's unpadded
    sequence, teacher-forced with the device's tokens."""
    worst = 0.0
    ref = None
    with torch.no_grad():
        for b, p in enumerate(prompts):
            if ref is None:
                ref = gen._GpuCache(model, p[None], bs)
            else:
                ref.prefill(p[None])
            worst = max(worst, float((ref.logits.float().cpu()[0] - rec[0]["logits"][b]).abs().max()))
            for j, r in enumerate(rec[1:]):
                assert int(r["pos_in"][b]) == p.numel() + j
                l = ref.step(r["tok_in"][b].view(1, 1).cuda(), int(r["pos_in"][b]))
                worst = max(worst, float((l.float().cpu()[0] - r["logits"][b]).abs().max()))
    print(f"max |ragged - B=1 rectangular| logits difference: {worst:.6g} (allowed {2 * tol:.6g})")
    if tol == 0:
        assert worst == 0
    else:
        assert worst <= 2 * tol
    return worst


# ------------------------------------------------------------------ 1. equal lengths = generate
@pytest.mark.parametrize("vocab,kw", [(1000, {}), (9000, {}),
                                      (1000, dict(do_sample=True, top_k=20, temperature=0.8, seed=99))],
                         ids=["greedy-1000", "greedy-9000-fused-argmax", "seeded-1000"])
def test_equal_lengths_reduce_to_generate(vocab, kw):
    model = _model(vocab)
    idx = torch.randint(0, vocab, (3, 7), device="cuda")
    want = model.generate(idx, 40, **kw)
    tokens, lengths = model.generate_batch(list(idx), 40, **kw)
    assert torch.equal(tokens, want) and lengths.tolist() == [47] * 3
    tokens2, _ = generate_batch(model, (idx, torch.full((3,), 7)), 40, **kw)
    assert torch.equal(tokens2, want)
    # ragged, then the rectangular loop, then ragged again with unchanged words: each loop has its
    # own parameter block, and the ragged one is not uploaded again
    assert torch.equal(model.generate(idx, 40, **kw), want)
    tokens3, _ = model.generate_batch(list(idx), 40, **kw)
    assert torch.equal(tokens3, want)


# ------------------------------------------------------------------ 2. the pick follows the rule
def test_pick_follows_the_rule(driven):
    """Lengths [1, 5, 17, 3], 30 one-step calls.  Greedy: the token is the argmax of its row's
    logits, exactly.  Seeded: the token is the numpy restatement's pick with draw counter pos + 1
    and batch row b wherever the fp64 top-two gap is at least 1e-3; at most 4 of the 120 draws may
    fall under that margin.  With seed 1234567 the CPU path's fp32 logits put 0 draws under it
    (test_seed_margin_on_cpu counts them)."""
    model, prompts, greedy, rec, final = driven
    skipped, draws = _check_pick(rec, greedy)
    if not greedy:
        print(f"skipped {skipped} of {draws}")
        assert draws == 120 and skipped <= 4
    assert final["pos"].tolist() == [n + STEPS for n in LENS] and not final["done"].any()


def test_seed_margin_on_cpu():
    """The seed of check 2 on the CPU path's fp32 logits: at most 1 of the 120 draws is under the
    margin (measured: 0)."""
    model = _model(1000).float().cpu()
    under = 0
    with torch.no_grad():
        for b, p in enumerate(_prompts(LENS)):
            p = p.cpu()
            cache = gen._CpuCache(model, p[None])
            logits, n = cache.logits, p.numel()
            for j in range(STEPS + 1):
                tok, gap = O.sample(logits.numpy(), TEMP, TOPK, SEED, n, row0=b)
                under += int(j > 0 and gap[0] < MARGIN)
                logits = cache.step(torch.tensor([[int(tok[0])]]), n)
                n += 1
    print(f"draws under the margin on the CPU: {under} of 120")
    assert under <= 1


# ------------------------------------------------------------------ 3. right row, right position
def test_logits_match_rectangular_b1(driven):
    """Measured on the parent commit between the rectangular B = 4 and B = 1 paths (this model,
    equal-length prompts of 1, 3, 5 and 17 tokens, 30 teacher-forced steps): see RECT_DIFF."""
    model, prompts, greedy, rec, final = driven
    _check_logits(model, prompts, rec, BS, RECT_DIFF["tiny"])


# ------------------------------------------------------------------ 4. loop = steps, graph = eager
def test_loop_equals_steps(driven, monkeypatch):
    model, prompts, greedy, rec, final = driven
    words = gen._ragged_words(SEED, TEMP, TOPK, None)
    with torch.no_grad():
        cache, st, _ = _start(model, prompts, words, greedy, BS)
        cache.ragged(STEPS, words, greedy)
        for k in final:
            assert torch.equal(st[k], final[k]), f"one call of {STEPS} steps: {k}"
        monkeypatch.setattr(gen, "_GRAPH_DECODE", False)
        cache, st, _ = _start(model, prompts, words, greedy, BS)
        cache.ragged(STEPS - 7, words, greedy)
        cache.ragged(7, words, greedy)
        assert cache._loops[("ragged", greedy)].graph is None
        for k in final:
            assert torch.equal(st[k], final[k]), f"eager: {k}"


# ------------------------------------------------------------------ 5. row isolation
@pytest.mark.parametrize("kw", [{}, dict(do_sample=True, top_k=20, temperature=0.8, seed=5)], ids=["greedy", "seeded"])
def test_row_isolation(tiny, kw):
    prompts = _prompts(LENS)
    a, la = generate_batch(tiny, prompts, 30, **kw)
    other = _prompts(LENS, seed=2)
    idx = torch.randint(0, 1000, (4, 17), device="cuda")  # random valid ids in every padding position
    for b, p in ((0, other[0]), (1, other[1][:2]), (2, prompts[2]), (3, other[3])):
        idx[b, :p.numel()] = p
    b_, lb = generate_batch(tiny, (idx, torch.tensor([1, 2, 17, 3])), 30, **kw)
    assert torch.equal(a[2], b_[2]) and int(la[2]) == int(lb[2]) == 47
    assert not torch.equal(a[0], b_[0])
    idx2 = idx.clone()
    idx2[0, 1:] = 0
    idx2[1, 2:] = 999
    idx2[3, 3:] = 1
    c, lc = generate_batch(tiny, (idx2, torch.tensor([1, 2, 17, 3])), 30, **kw)
    assert torch.equal(c, b_) and torch.equal(lc, lb)


# ------------------------------------------------------------------ 6. split boundaries per row
@pytest.mark.parametrize("name,n_head,bs,lens,n", [
    ("split256", 2, 320, [250, 3, 130], 20),
    ("split128", 4, 192, [120, 122, 124, 126, 127, 128, 130, 133, 135], 16),
])
def test_split_boundaries_differ_per_row(name, n_head, bs, lens, n):
    """Rows of one launch use different split counts: B * H <= 32 splits every 256 keys (row 0
    crosses 256 while rows 1 and 2 stay in one split), B * H > 32 every 128 (rows cross 128 at
    different steps; B = 9 runs the step on the MFMA GEMM path).  Held to checks 2 (greedy) and 3,
    the latter against the rectangular paths' own B vs B = 1 difference on this model."""
    model = _model(1000, n_head, bs)
    prompts = _prompts(lens, seed=3)
    rec, final = _drive(model, prompts, n - 1, True, bs)  # the first pick + n - 1 steps = n tokens
    assert final["pos"].tolist() == [m + n - 1 for m in lens]
    _check_pick(rec, True)
    _check_logits(model, prompts, rec, bs, RECT_DIFF[name])


# ------------------------------------------------------------------ 7. EOS on the device
def _pick_eos(tokens, lens, new):
    for b, n in enumerate(lens):
        part = tokens[b, n:n + new].tolist()
        for j in range(3, new):
            if part[j] not in part[:j]:
                return part[j]
    raise AssertionError("no usable stop token")


@pytest.mark.parametrize("kw", [{}, dict(do_sample=True, top_k=20, temperature=0.8, seed=5)], ids=["greedy", "seeded"])
def test_eos_on_device(tiny, kw, monkeypatch):
    prompts, new = _prompts(LENS), 40
    full, _ = generate_batch(tiny, prompts, new, **kw)
    eos = _pick_eos(full, LENS, new)
    tokens, lengths = generate_batch(tiny, prompts, new, eos_token=eos, pad_token=3, **kw)
    want = torch.full_like(full, 3)
    keep, hit = [], []
    for b, n in enumerate(LENS):
        part = full[b, n:n + new].tolist()
        hit.append(eos in part)
        keep.append(n + (part.index(eos) + 1 if eos in part else new))
        want[b, :keep[b]] = full[b, :keep[b]]
    assert torch.equal(tokens, want) and lengths.tolist() == keep
    assert any(k < n + new for k, n in zip(keep, LENS))
    # a finished row's state stops changing; the others move on
    cache = tiny._mg_decode_cache
    st = cache.ragged_state()
    fin = st["done"].bool().clone()
    assert fin.tolist() == hit
    before = {k: st[k].clone() for k in ("pos", "done", "tok", "seq")}
    assert int(before["pos"].max()) + 3 < BS
    cache.ragged(3, gen._ragged_words(kw.get("seed", 0), kw.get("temperature", 1.0), kw.get("top_k"), eos),
                 not kw)
    for k in before:
        assert torch.equal(st[k][fin], before[k][fin]), k
    moved = ~fin & ~st["done"].bool()
    assert torch.equal(st["pos"][moved], before["pos"][moved] + 3)
    # every row finished long before max_new_tokens: stopping early or not gives the same result
    # (a one-row batch, the first prompt whose first 8 tokens hold a usable stop token)
    for p in prompts:
        one, n0 = [p], p.numel()
        f1, _ = generate_batch(tiny, one, new, **kw)
        part = f1[0, n0:n0 + 8].tolist()
        if any(part[j] not in part[:j] for j in range(3, 8)):
            break
    eos1 = _pick_eos(f1, [n0], 8)
    n1 = n0 + f1[0, n0:].tolist().index(eos1) + 1
    early = generate_batch(tiny, one, new, eos_token=eos1, **kw)
    monkeypatch.setattr(gen, "_EARLY_EXIT", False)
    late = generate_batch(tiny, one, new, eos_token=eos1, **kw)
    assert int(early[1]) == n1 <= n0 + 8 and torch.equal(early[0], late[0]) and torch.equal(early[1], late[1])
    assert torch.equal(early[0][0, :n1], f1[0, :n1]) and (early[0][0, n1:] == 0).all()


# ------------------------------------------------------------------ 8. state reuse
def test_state_reuse_and_recapture():
    model, fresh = _model(1000), lambda: _model(1000)
    kw = dict(do_sample=True, top_k=20, temperature=0.8, seed=7)
    a = generate_batch(model, _prompts(LENS), 30, **kw)
    graph = model._mg_decode_cache._loops[("ragged", False)].graph
    for lens, kw2 in (([9, 2, 4, 11], kw), ([9, 2, 4, 11], dict(do_sample=True, top_k=3, temperature=1.7, seed=8)),
                      (LENS, kw)):
        got = generate_batch(model, _prompts(lens, seed=4), 30, **kw2)
        want = generate_batch(fresh(), _prompts(lens, seed=4), 30, **kw2)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert model._mg_decode_cache._loops[("ragged", False)].graph is graph
    assert torch.equal(generate_batch(model, _prompts(LENS), 30, **kw)[0], a[0])
    other = fresh()
    with torch.no_grad():
        for m in (model, other):
            m.transformer.wpe.weight.mul_(3.0)  # in place: the version changes, the pointer does not
    got = generate_batch(model, _prompts(LENS), 30, **kw)
    assert model._mg_decode_cache._loops[("ragged", False)].graph is not graph
    assert torch.equal(got[0], generate_batch(other, _prompts(LENS), 30, **kw)[0])
    assert not torch.equal(got[0], a[0])


# ------------------------------------------------------------------ 9. guard bands
def _state(B, L, pos, done):
    return {"pos": torch.tensor(pos, dtype=torch.int32, device="cuda"),
            "done": torch.tensor(done, dtype=torch.int32, device="cuda"),
            "tok": torch.full((B, 1), 5, dtype=torch.long, device="cuda"),
            "seq": torch.full((B, L), 7, dtype=torch.long, device="cuda")}


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "seeded"])
@pytest.mark.parametrize("V", [1000, 1003, 9001])
def test_guard_bands_pick(V, greedy):
    """The pick kernels with seq, tok, pos and done between sentinel margins and the logits between
    NaN margins (the padding columns >= V NaN as well): no margin byte changes, the outputs equal
    the plain run's, a finished row and a row at the last position are left alone."""
    C = ext()
    B, L, ld = 4, 40, (V + 7) // 8 * 8
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(B, ld, generator=g).to("cuda", torch.bfloat16)
    logits[:, V:] = float("nan")
    logits[0, V - 1] = 30.0  # the last valid column wins row 0 (greedy)
    params = torch.tensor(gen._ragged_words(11, 0.9, 50, V - 1), dtype=torch.int32, device="cuda")
    pos, done = [0, 17, 38, 9], [0, 0, 0, 1]  # row 2: pos + 1 would reach L - 1
    _, r = guarded(lambda logits, params, pos, done, tok, seq: C.pick_ragged(logits, V, params, pos, done, tok, seq, greedy),
                   {"logits": logits, "params": params}, _state(B, L, pos, done), name="pick_ragged")
    want = _state(B, L, pos, done)
    for b in (0, 1):
        if greedy:
            t = int(logits[b, :V].float().argmax())
        else:
            t = int(O.sample(logits[b:b + 1, :V].float().cpu().numpy(), 0.9, 50, 11, pos[b] + 1, row0=b)[0][0])
        want["tok"][b] = t
        want["seq"][b, pos[b] + 1] = t
        want["pos"][b] += 1
        want["done"][b] = int(t == V - 1)
    if greedy:
        assert int(r["tok"][0]) == V - 1 and int(r["done"][0]) == 1
    for k in want:
        assert torch.equal(r[k], want[k]), k


@pytest.mark.parametrize("H,hd,Tmax,pos", [(2, 64, 300, [0, 255, 256, 299]), (9, 24, 200, [127, 128, 5, 199])])
def test_guard_bands_attention_decode_per_row(H, hd, Tmax, pos):
    """Per-row decode attention with every operand between margins: each row appends at its own
    cache row and attends to its own key range (rows on both sides of a split boundary in one
    launch), and equals the same row run alone through the scalar-position path."""
    C = ext()
    B, D = len(pos), H * hd
    g = torch.Generator().manual_seed(H)
    cache = torch.randn(B, Tmax, 3 * D, generator=g).to("cuda", torch.bfloat16)
    qkv = torch.randn(B, 3 * D, generator=g).to("cuda", torch.bfloat16)
    pos_dev = torch.tensor(pos, dtype=torch.int32, device="cuda")
    np_ = C.attention_decode_part_floats(B, H, hd)
    (out,), r = guarded(lambda qkv_new, pos_dev, cache, part, counters:
                        C.attention_decode(qkv_new, cache, H, 1, pos_dev, part, counters, pos_stride=1),
                        {"qkv_new": qkv, "pos_dev": pos_dev},
                        {"cache": cache, "part": torch.zeros(np_, device="cuda"),
                         "counters": torch.zeros(B * H, device="cuda", dtype=torch.int32)},
                        name="attention_decode per row", skip=("part",))
    assert (r["counters"] == 0).all()
    want = cache.clone()
    for b, p in enumerate(pos):
        want[b, p, D:] = qkv[b, D:]
    assert torch.equal(r["cache"], want), "the cache changed outside each row's own K/V slots"
    for b, p in enumerate(pos):
        alone = C.attention_decode(qkv[b:b + 1].contiguous(), cache[b:b + 1].clone(), H, p)
        if B * H <= 32:  # the row alone splits its keys the same way: the same arithmetic
            assert torch.equal(out[b:b + 1], alone), f"row {b}"
        else:
            torch.testing.assert_close(out[b:b + 1].float(), alone.float(), atol=2e-2, rtol=2e-2)
