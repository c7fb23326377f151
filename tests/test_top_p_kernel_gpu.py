"""The nucleus (top-p) stage of the sample kernel (csrc/kernels/sample.hip) driven stand-alone through
``ext().sample_logits`` / ``ext().sample_kept`` against the rule restated in numpy float64
(tests/_nucleus_oracle.py).

Exactness.  The kernel sums integer masses floor(w 2^32) of fp32 weights; common.h derives
|A^/Z^ - A/Z| <= 8.8e-6 * A/Z + V 2^-32, i.e. a relative shift of top_p by at most
``8.8e-6 + V * 2^-32 / top_p`` at the boundary.  ``N.delta`` is four times that (never above 1e-3): the
kernel's kept set must lie between the fp64 rule's at top_p (1 - delta) and top_p (1 + delta) at
every row -- with the few distinct values of a bf16 row the two almost always coincide and the check
is equality.  A draw is compared when the fp64 token is the same under both and both top-two score
gaps are at least 1e-3 (the score error of common.h); at most 1 % of a case's draws may be skipped."""
import struct

import numpy as np
import pytest
import torch

import _nucleus_oracle as N
import _sample_oracle as O
from _guard import POISON, SENTINEL, arena, assert_intact

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
MAX_SKIP = 0.01


@pytest.fixture(scope="module")
def C():
    from mingpt_distributed_amd.ops._ext import ext

    return ext()


def f32_bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def words(seed, draw, temperature, top_k, top_p):
    s32 = lambda x: ((x & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    return [s32(seed), s32(seed >> 32), s32(draw), f32_bits(1.0 / temperature), int(top_k or 0), 0,
            f32_bits(top_p) if top_p else 0, 0]


def block(seed, draw, temperature, top_k, top_p):
    return torch.tensor(words(seed, draw, temperature, top_k, top_p), dtype=torch.int32, device="cuda")


def make_logits(B, V, ld, scale=3.0, gen_seed=0, pad=0.0, identical=True):
    g = torch.Generator().manual_seed(gen_seed)
    rows = torch.randn(1 if identical else B, V, generator=g) * scale
    full = torch.full((B, ld), pad, dtype=torch.float32)
    full[:, :V] = rows
    return full.to(torch.bfloat16).cuda()


def bf16_value(bits):
    return np.array([struct.unpack("<f", struct.pack("<I", (int(b) & 0xFFFF) << 16))[0] for b in bits])


def host_rows(logits, V):
    """The distinct rows of the logits on the host, and the map row -> distinct row."""
    l = logits[:, :V].float().cpu().numpy()
    if (l == l[:1]).all():
        return l[:1], np.zeros(len(l), dtype=np.int64)
    return l, np.arange(len(l))


def check_case(C, logits, V, seed, T, k, p, draws, draw0=0):
    """Threshold bracket at every row, then ``draws`` launches on one parameter block against the
    oracle.  Returns the tokens [draws, B]."""
    B = logits.shape[0]
    rows, of = host_rows(logits, V)
    d = N.delta(V, p)
    keep_lo, keep_hi = N.keep(rows, T, k, p * (1 - d)), N.keep(rows, T, k, p * (1 + d))
    v_lo, c_lo = N.threshold(rows, T, k, p * (1 - d))  # the smaller set: the higher lowest value
    v_hi, c_hi = N.threshold(rows, T, k, p * (1 + d))
    v_off, c_off = N.threshold(rows, T, k, None)
    kept = C.sample_kept(logits, V, block(seed, draw0, T, k, p)).cpu().numpy()
    got_v, got_c = bf16_value(kept[:, 0]), kept[:, 1]
    print(f"V {V} k {k} T {T} p {p}: delta {d:.2e}, kept {got_c[0]} (bracket {c_lo[0]}..{c_hi[0]}), "
          f"without top_p {c_off[0]}")
    assert (v_hi[of] <= got_v).all() and (got_v <= v_lo[of]).all(), (got_v, v_hi[of], v_lo[of])
    assert (c_lo[of] <= got_c).all() and (got_c <= c_hi[of]).all(), (got_c, c_lo[of], c_hi[of])
    assert (c_hi < c_off).any(), "the case has no teeth: the nucleus drops nothing"

    pb = block(seed, draw0, T, k, p)
    got = torch.stack([C.sample_logits(logits, V, pb) for _ in range(draws)]).cpu().numpy()
    assert int(pb[2].item()) & 0xFFFFFFFF == (draw0 + draws) & 0xFFFFFFFF
    assert pb.tolist()[:2] + pb.tolist()[3:] == words(seed, 0, T, k, p)[:2] + words(seed, 0, T, k, p)[3:]
    l = logits[:, :V].float().cpu().numpy()
    same = np.array_equal(keep_lo, keep_hi)
    ok = np.empty((draws, B), dtype=bool)
    want = np.empty((draws, B), dtype=np.int64)
    for i in range(draws):
        ta, ga = N.sample(l, T, k, None, seed, draw0 + i, kept=keep_lo[of])
        tb, gb = (ta, ga) if same else N.sample(l, T, k, None, seed, draw0 + i, kept=keep_hi[of])
        want[i], ok[i] = ta, (ta == tb) & (ga >= MARGIN) & (gb >= MARGIN)
    assert got.shape == want.shape and (got >= 0).all() and (got < V).all()
    skipped = 1.0 - ok.mean()
    print(f"draws {ok.size}, skipped {skipped:.4%}, mismatches {(got[ok] != want[ok]).sum()}")
    assert skipped <= MAX_SKIP, f"{skipped:.2%} of the draws are under the margin"
    bad = np.argwhere(ok & (got != want))
    assert len(bad) == 0, (f"{len(bad)} of {ok.sum()} draws differ from the fp64 rule, first (draw, row) "
                           f"{bad[0].tolist()}: kernel {got[tuple(bad[0])]}, rule {want[tuple(bad[0])]}")
    assert keep_hi[of][np.arange(B)[None, :], got].all(), "a token outside the nucleus was drawn"
    return got


# (V, ld, top_k, temperature, top_p, B, launches, identical rows): B x launches >= 200 draws per case
CASES = [
    (7, 8, None, 1.0, 0.5, 3, 70, True),
    (7, 8, 3, 0.5, 0.9, 8, 25, True),
    (1000, 1000, None, 1.0, 0.9, 64, 4, True),
    (1000, 1000, 10, 1.0, 0.5, 64, 4, True),
    (50257, 50264, None, 1.0, 0.9, 64, 4, True),
    (50257, 50264, None, 1.0, 0.3, 64, 4, True),
    (50257, 50264, 40, 0.8, 0.9, 64, 4, True),
    (50257, 50264, None, 1.3, 0.95, 8, 25, False),
    (50257, 50264, 40, 1.0, 0.9, 33, 7, True),       # the decode shape past the skinny GEMM's B <= 8
    (65536, 65536, None, 1.0, 0.9, 3, 67, True),     # the longest row the kernel keeps in registers
    (65536, 65536, 40, 1.0, 0.6, 3, 67, True),
    (65544, 65544, None, 1.0, 0.9, 3, 67, True),     # one vector more: every pass streams the row
    (65544, 65544, 40, 1.0, 0.6, 3, 67, True),
    (70001, 70008, None, 1.0, 0.9, 8, 25, True),
    (70001, 70008, 40, 0.9, 0.6, 8, 25, True),
]


@pytest.mark.parametrize("V,ld,k,T,p,B,n,identical", CASES)
def test_threshold_and_tokens(C, V, ld, k, T, p, B, n, identical):
    logits = make_logits(B, V, ld, gen_seed=V + (k or 0), scale=1.0 if V < 100 else 3.0, identical=identical)
    got = check_case(C, logits, V, 0x1234_5678_9ABC_DEF0 + V, T, k, p, n)
    assert len(np.unique(got)) > 1


def test_off_and_one_are_the_existing_rule(C):
    """Word 6 = 0 and top_p = 1.0 (and anything that is not a float in (0, 1)) leave the tokens of
    the top-k rule, which the kept set confirms."""
    for V, ld, k in [(1000, 1000, 10), (50257, 50264, None), (50257, 50264, 40), (70001, 70008, None)]:
        B = 8
        logits = make_logits(B, V, ld, identical=False, gen_seed=3)
        l = logits[:, :V].float().cpu().numpy()
        for draw in range(3):
            off = C.sample_logits(logits, V, block(7, draw, 0.9, k, None))
            for p in (1.0, 2.0, -0.5):
                assert torch.equal(C.sample_logits(logits, V, block(7, draw, 0.9, k, p)), off), (V, k, p)
            want, gap = O.sample(l, 0.9, k, 7, draw)
            ok = gap >= MARGIN
            assert np.array_equal(off.cpu().numpy()[ok], want[ok])
        low, cnt = N.threshold(l, 0.9, k, None)
        for p in (None, 1.0):
            kept = C.sample_kept(logits, V, block(7, 0, 0.9, k, p)).cpu().numpy()
            assert np.array_equal(bf16_value(kept[:, 0]), low) and np.array_equal(kept[:, 1], cnt)


@pytest.mark.parametrize("V,ld,k", [(1000, 1000, None), (50257, 50264, 40), (70001, 70008, None)])
def test_tiny_top_p_draws_only_maxima(C, V, ld, k):
    B = 64
    logits = make_logits(B, V, ld, gen_seed=9)
    top = [5, V // 2, V - 1]
    logits[:, top] = logits[:, :V].max() + 1.0
    kept = C.sample_kept(logits, V, block(3, 0, 1.0, k, 1e-6)).cpu().numpy()
    assert (kept[:, 1] == 3).all() and (bf16_value(kept[:, 0]) == logits[0, 5].item()).all()
    got = torch.stack([C.sample_logits(logits, V, block(3, d, 1.0, k, 1e-6)) for d in range(4)]).cpu().numpy()
    assert set(np.unique(got).tolist()) == set(top)


def test_tie_group_at_the_boundary(C):
    """3.0 once, 2.0 four times, the next bf16 below once, -1.0 for the rest at T = 1: top_p = 0.5 is
    reached inside the tie group (the mass above 2.0 is 0.33 of the total, above 1.984375 0.82)."""
    V = 16
    l = torch.full((V,), -1.0)
    l[2] = 3.0
    l[[0, 5, 11, 15]] = 2.0
    l[7] = 1.984375
    logits = l.to(torch.bfloat16).view(1, V).repeat(64, 1).cuda()
    for k in (None, 6):  # top-6 keeps 1.984375 too
        kept = C.sample_kept(logits, V, block(9, 0, 1.0, k, 0.5)).cpu().numpy()
        assert (kept[:, 0] == 0x4000).all() and (kept[:, 1] == 5).all()
        got = check_case(C, logits, V, 9, 1.0, k, 0.5, 32)
        assert set(np.unique(got).tolist()) == {0, 2, 5, 11, 15}
    kept = C.sample_kept(logits, V, block(9, 0, 1.0, None, 0.3)).cpu().numpy()
    assert (kept[:, 0] == 0x4040).all() and (kept[:, 1] == 1).all()


@pytest.mark.parametrize("k", [None, 1, 5])
def test_single_finite_entry(C, k):
    V, ld, B = 1000, 1000, 4
    l = torch.full((B, ld), float("-inf"), dtype=torch.bfloat16, device="cuda")
    where = torch.tensor([0, 999, 512, 7], device="cuda")
    l[torch.arange(B), where] = torch.tensor([0.0, -5.0, 80.0, -3e38], dtype=torch.bfloat16, device="cuda")
    for d in range(4):
        assert torch.equal(C.sample_logits(l, V, block(1, d, 1.0, k, 0.5)), where)
    kept = C.sample_kept(l, V, block(1, 0, 1.0, k, 0.5))
    assert kept[:, 1].tolist() == [1, 1, 1, 1]
    assert kept[:, 0].tolist() == (l[torch.arange(B), where].view(torch.int16).int() & 0xFFFF).tolist()


def test_huge_logits_small_temperature(C):
    """+-3e38 at T = 0.01: the weights of the losers underflow to 0, never to NaN; only the entries
    at the maximum are kept and drawn."""
    V, ld, B = 1000, 1000, 64
    g = torch.Generator().manual_seed(1)
    l = torch.where(torch.rand(V, generator=g) < 0.02, 3e38, -3e38)
    l[::7][:20] = 0.0
    logits = l.to(torch.bfloat16).view(1, V).repeat(B, 1).cuda()
    top = torch.nonzero(logits[0].float() > 1e38).view(-1).tolist()
    for k in (None, 5):
        kept = C.sample_kept(logits, V, block(6, 0, 0.01, k, 0.9)).cpu().numpy()
        assert (kept[:, 1] == len(top)).all() and (bf16_value(kept[:, 0]) > 1e38).all()
        got = torch.stack([C.sample_logits(logits, V, block(6, d, 0.01, k, 0.9)) for d in range(4)]).cpu().numpy()
        assert set(np.unique(got).tolist()) <= set(top)
        l64 = logits.float().cpu().numpy()
        for d in range(4):
            want, gap = N.sample(l64, 0.01, k, 0.9, 6, d)
            ok = gap >= MARGIN
            assert np.array_equal(got[d][ok], want[ok])


@pytest.mark.parametrize("V,ld,k", [(7, 8, None), (997, 1000, 10), (50257, 50264, 40), (50257, 50264, None)])
def test_pad_columns_never_read(C, V, ld, k):
    B = 8
    base = make_logits(B, V, ld, identical=False, gen_seed=2)
    ref = C.sample_logits(base, V, block(3, 0, 1.0, k, 0.7))
    ref_kept = C.sample_kept(base, V, block(3, 0, 1.0, k, 0.7))
    for pad in (float("inf"), float("nan")):
        l = base.clone()
        l[:, V:] = pad
        tok = C.sample_logits(l, V, block(3, 0, 1.0, k, 0.7))
        assert (tok < V).all() and (tok >= 0).all()
        assert torch.equal(tok, ref), f"pad {pad} changed the tokens"
        assert torch.equal(C.sample_kept(l, V, block(3, 0, 1.0, k, 0.7)), ref_kept)


@pytest.mark.parametrize("V,ld,k,B", [(7, 8, 3, 3), (9000, 9000, None, 8), (50257, 50264, 40, 2),
                                      (50257, 50264, None, 2), (70001, 70008, None, 2)])
def test_guard_bands(C, V, ld, k, B):
    """As the sampler's own guard-band test, with top_p on: every margin intact, the same result as
    the plain run, and of the parameter block only word 2 (the draw counter) changes.  sample_kept
    writes nothing but its result."""
    L, pos, draw = 12, 5, 40
    logits = make_logits(B, V, ld, identical=False, gen_seed=11)
    w = words(77, draw, 0.8, k, 0.8)

    def run(wrap):
        lg = wrap("logits", logits, POISON)
        p = wrap("params", torch.tensor(w, dtype=torch.int32, device="cuda"), SENTINEL)
        pd = wrap("pos", torch.tensor([pos], dtype=torch.int32, device="cuda"), SENTINEL)
        tok = wrap("tok", torch.full((B, 1), -7, dtype=torch.long, device="cuda"), SENTINEL)
        seq = wrap("seq", torch.full((B, L), -9, dtype=torch.long, device="cuda"), SENTINEL)
        kept = C.sample_kept(lg, V, p)
        assert p.tolist() == w
        ret = C.sample_logits(lg, V, p, pd, tok, seq)
        assert ret.data_ptr() == tok.data_ptr()
        return p, pd, tok, seq, kept

    plain = run(lambda name, t, fill: t)
    bufs = {}

    def wrap(name, t, fill):
        bufs[name], v = arena(t, fill)
        bufs[name + "_view"] = v
        return v

    guarded = run(wrap)
    for name in ("logits", "params", "pos", "tok", "seq"):
        assert_intact(bufs[name], bufs[name + "_view"], name)
    for a, b in zip(plain, guarded):
        assert torch.equal(a, b)
    p, pd, tok, seq, kept = plain
    assert p.tolist() == w[:2] + [draw + 1] + w[3:]
    assert pd.item() == pos + 1
    assert ((tok >= 0) & (tok < V)).all()
    want = torch.full((B, L), -9, dtype=torch.long, device="cuda")
    want[:, pos + 1] = tok.view(B)
    assert torch.equal(seq, want)
    assert torch.equal(tok.view(B), C.sample_logits(logits, V, block(77, draw, 0.8, k, 0.8)))
    assert kept.shape == (B, 2) and kept.dtype == torch.int32 and (kept[:, 1] >= 1).all()


def test_row_isolation(C):
    B, V, ld = 8, 9000, 9000
    a = make_logits(B, V, ld, identical=False, gen_seed=21)
    ta = C.sample_logits(a, V, block(5, 2, 1.0, None, 0.9))
    ka = C.sample_kept(a, V, block(5, 2, 1.0, None, 0.9))
    for b in (0, 3, 7):
        other = make_logits(B, V, ld, identical=False, gen_seed=22 + b, scale=5.0)
        other[b] = a[b]
        tb = C.sample_logits(other, V, block(5, 2, 1.0, None, 0.9))
        kb = C.sample_kept(other, V, block(5, 2, 1.0, None, 0.9))
        assert tb[b].item() == ta[b].item() and torch.equal(kb[b], ka[b])
        assert not torch.equal(tb, ta) and not torch.equal(kb, ka)


def test_ragged_pick_takes_top_p(C):
    """The ragged form of the kernel reads the same word: rows at position p draw with counter
    p + 1, a finished row is left alone."""
    B, V, ld, L = 4, 1000, 1000, 16
    logits = make_logits(B, V, ld, identical=False, gen_seed=41)
    pos = torch.tensor([3, 7, 0, 5], dtype=torch.int32, device="cuda")
    done = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device="cuda")
    tok = torch.full((B, 1), -7, dtype=torch.long, device="cuda")
    seq = torch.full((B, L), -9, dtype=torch.long, device="cuda")
    w = words(11, 0, 0.9, None, 0.5)
    w[5] = -1
    p = torch.tensor(w, dtype=torch.int32, device="cuda")
    C.pick_ragged(logits, V, p, pos, done, tok, seq, False)
    assert p.tolist() == w and pos.tolist() == [4, 8, 0, 6] and tok[2].item() == -7
    l = logits[:, :V].float().cpu().numpy()
    kept = N.keep(l, 0.9, None, 0.5)
    for b in (0, 1, 3):
        want, gap = N.sample(l[b:b + 1], 0.9, None, 0.5, 11, [4, 8, 0, 6][b], row0=b)
        assert kept[b, tok[b].item()]
        if gap[0] >= MARGIN:
            assert tok[b].item() == want[0]
        assert seq[b, [4, 8, 0, 6][b]].item() == tok[b].item()


def test_parameter_block_and_graph_replay(C):
    """One captured launch serves every top_p written into the block, a replay equals an eager
    launch, and the same block state replayed twice gives the same tokens."""
    B, V, ld = 64, 1000, 1000
    logits = make_logits(B, V, ld, gen_seed=31)
    l = logits[:, :V].float().cpu().numpy()
    p = block(1, 0, 1.0, 10, 0.5)
    tok = torch.zeros(B, dtype=torch.long, device="cuda")
    C.sample_logits(logits, V, p, None, tok)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        C.sample_logits(logits, V, p, None, tok)

    seen = []
    for k, top_p in [(10, 0.5), (None, 0.9), (None, 0.3), (None, None)]:
        p.copy_(block(1, 0, 1.0, k, top_p))
        graph.replay()
        got = tok.clone()
        p.copy_(block(1, 0, 1.0, k, top_p))
        graph.replay()
        assert torch.equal(tok, got), "the same block state replayed twice differs"
        eager = C.sample_logits(logits, V, block(1, 0, 1.0, k, top_p))
        assert torch.equal(got, eager), "replay differs from the eager launch"
        d = N.delta(V, top_p) if top_p else 0.0
        lo = N.keep(l[:1], 1.0, k, top_p * (1 - d) if top_p else None)
        hi = N.keep(l[:1], 1.0, k, top_p * (1 + d) if top_p else None)
        assert np.array_equal(lo, hi)
        want, gap = N.sample(l, 1.0, k, None, 1, 0, kept=lo)
        ok = gap >= MARGIN
        assert np.array_equal(got.cpu().numpy()[ok], want[ok])
        assert all(not torch.equal(got, s) for s in seen), "a changed block did not change the draws"
        seen.append(got)
