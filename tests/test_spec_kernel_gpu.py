"""The speculative-decoding kernels (csrc/kernels/spec.hip) driven stand-alone through
``ext().spec_draft``, ``spec_argmax`` and ``spec_accept``: the draft against the rule restated in
numpy integers (tests/_spec_oracle.py), exactly; the row argmax and the accept rule on logits with
planted maxima -- every acceptance length, the no-draft flag, an exact tie, ``end`` cutting the
emission, a finished sequence -- and both between guard bands."""
import numpy as np
import pytest
import torch

import _spec_oracle as O
from _guard import guarded
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

L = 64  # tokens per sequence in the draft cases
VOCABS = [(1000, 1000), (9000, 9000), (50257, 50264)]


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).reshape(-1).cuda()


def _draft(seq, pos, ngram, K, end=0):
    """The draft kernel on host ``seq`` [B, L] / ``pos`` [B], outputs pre-filled with sentinels:
    (tok [B, K], pos_rows [B, K], has [B]) as numpy."""
    B = seq.shape[0]
    tok = torch.full((B * K, 1), -5, dtype=torch.long).cuda()
    pos_rows, has = _i32([-7] * (B * K)), _i32([-9] * B)
    ext().spec_draft(torch.as_tensor(seq, dtype=torch.long).cuda().contiguous(), _i32(pos), _i32([ngram, end, 0, 0]),
                     K, tok, pos_rows, has)
    torch.cuda.synchronize()
    return tok.view(B, K).cpu().numpy(), pos_rows.view(B, K).cpu().numpy(), has.cpu().numpy()


@pytest.mark.parametrize("alphabet", [3, 997], ids=["3-symbols", "997-symbols"])
@pytest.mark.parametrize("B,K", [(1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (4, 2)], ids=lambda x: str(x))
def test_draft_equals_oracle(alphabet, B, K):
    """Random sequences of 64 tokens over a 3-symbol alphabet and over 0..996, every p of {0, 1,
    ngram - 1, ngram, 40, 63} and ngram 1..4 (rows of a batch at different positions), exact."""
    rng = np.random.default_rng(alphabet + 16 * B + K)
    drafts = 0
    for ngram in (1, 2, 3, 4):
        ps = sorted({0, 1, ngram - 1, ngram, 40, 63})
        for i, p0 in enumerate(ps):
            seq = rng.integers(0, alphabet, (B, L))
            pos = [ps[(i + b) % len(ps)] for b in range(B)]
            tok, pos_rows, has = _draft(seq, pos, ngram, K)
            for b in range(B):
                rows, prow, h = O.draft(seq[b], pos[b], K, ngram)
                what = f"ngram {ngram}, p {pos[b]}, row {b}"
                assert tok[b].tolist() == rows.tolist(), what
                assert pos_rows[b].tolist() == prow.tolist() and int(has[b]) == int(h), what
                drafts += int(h)
    assert drafts > 0 or alphabet != 3


def test_draft_hand_cases():
    """Period-2 text at K = 8 (the draft extends through itself), a most-recent tie, a longer match
    further back, no match, and p = 0."""
    pad = lambda s: np.array([s + [0] * (L - len(s))])
    tok, pos_rows, has = _draft(pad([7, 9] * 5), [9], 3, 8)
    assert tok[0].tolist() == [9, 7, 9, 7, 9, 7, 9, 7] and pos_rows[0].tolist() == list(range(9, 17)) and has[0] == 1
    s = [4, 5, 1, 1, 4, 5, 2, 2, 4, 5]
    assert _draft(pad(s), [9], 2, 3)[0][0].tolist() == [5, 2, 2]
    s = [3, 4, 5, 1, 0, 4, 5, 2, 3, 4, 5]
    assert _draft(pad(s), [10], 3, 3)[0][0].tolist() == [5, 1, 0]
    assert _draft(pad(s), [10], 2, 3)[0][0].tolist() == [5, 2, 3]
    tok, _, has = _draft(pad([1, 2, 3, 4, 5]), [4], 3, 4)
    assert tok[0].tolist() == [5, 5, 5, 5] and has[0] == 0
    tok, pos_rows, has = _draft(pad([8]), [0], 1, 2)
    assert tok[0].tolist() == [8, 8] and pos_rows[0].tolist() == [0, 1] and has[0] == 0


def _logits(R, V, ld, winners, seed):
    """bf16 logits [R, ld] in [-2, 2] with row r's maximum 8.0 planted at column winners[r]; the pad
    columns hold NaN (never read)."""
    g = torch.Generator().manual_seed(seed)
    l = torch.full((R, ld), float("nan"))
    l[:, :V] = torch.rand(R, V, generator=g) * 4.0 - 2.0
    for r, w in enumerate(winners):
        l[r, w] = 8.0
    return l.to(torch.bfloat16)


def _accept(logits, V, K, rows, has, pos, end, Lseq=40):
    """Row argmax + accept on ``logits`` [B * K, ld] with input rows ``rows`` [B, K]: returns (g [B, K],
    seq, pos, steps, hist) as numpy; ``seq`` starts as -3 everywhere."""
    B = len(pos)
    C = ext()
    seq = torch.full((B, Lseq), -3, dtype=torch.long).cuda()
    p, steps, hist = _i32(pos), _i32([0] * B), _i32([0] * (B * (K + 1))).view(B, K + 1)
    g = torch.full((B * K,), -1, dtype=torch.int32).cuda()
    C.spec_argmax(logits.cuda(), V, g)
    C.spec_accept(g, torch.as_tensor(rows, dtype=torch.long).reshape(B * K, 1).cuda(), _i32(has), K, p,
                  _i32([3, end, 0, 0]), seq, steps, hist)
    torch.cuda.synchronize()
    return g.view(B, K).cpu().numpy(), seq.cpu().numpy(), p.cpu().numpy(), steps.cpu().numpy(), hist.cpu().numpy()


def _check(g, seq, p, steps, hist, b, p0, cnt, K):
    """Sequence b emitted ``cnt`` tokens g[b, :cnt] at columns p0 + 1 .., moved to p0 + cnt, counted
    one step -- or, cnt == 0, changed nothing -- and nothing else of its ``seq`` row was written."""
    want = np.full(seq.shape[1], -3)
    want[p0 + 1:p0 + 1 + cnt] = g[b, :cnt]
    assert seq[b].tolist() == want.tolist(), f"sequence {b}"
    assert p[b] == p0 + cnt and steps[b] == (1 if cnt else 0), f"sequence {b}"
    h = np.zeros(K + 1, dtype=np.int64)
    if cnt:
        h[cnt] = 1
    assert hist[b].tolist() == h.tolist(), f"sequence {b}"


@pytest.mark.parametrize("V,ld", VOCABS, ids=[f"V{v}" for v, _ in VOCABS])
def test_accept_planted(V, ld):
    """K = 4, four sequences in one launch: every draft confirmed; none; confirmed up to r = 2; and
    all confirmed but the no-draft flag set.  The maxima sit at the first, the last and inner columns."""
    K, p0 = 4, 10
    win = [[0, V - 1, 17, 5], [V - 1, 3, 4, 5], [V // 2, 7, V - 2, 9], [1, 1, 1, 1]]
    rows = [[2, 0, V - 1, 17], [2, 0, 3, 4], [2, V // 2, 7, 6], [1, 1, 1, 1]]
    has = [1, 1, 1, 0]
    logits = _logits(4 * K, V, ld, sum(win, []), seed=V)
    g, seq, p, steps, hist = _accept(logits, V, K, rows, has, [p0] * 4, 35)
    assert g.tolist() == win
    for b, cnt in enumerate([4, 1, 3, 1]):
        assert O.accept(rows[b], win[b], bool(has[b]), p0, 35)[1] == cnt
        _check(g, seq, p, steps, hist, b, p0, cnt, K)


@pytest.mark.parametrize("V,ld", VOCABS, ids=[f"V{v}" for v, _ in VOCABS])
def test_accept_tie_end_and_finished(V, ld):
    """An exact two-way tie of the maximum (the lower index wins and decides the acceptance, both
    ways), ``end`` cutting a fully confirmed step, and a sequence with p == end left untouched."""
    K, p0 = 4, 10
    lo, hi = 11, V - 3
    win = [[lo, 4, 5, 6], [lo, 4, 5, 6], [1, 2, 3, 4], [1, 2, 3, 4]]
    rows = [[0, lo, 4, 5], [0, hi, 4, 5], [0, 1, 2, 3], [0, 1, 2, 3]]
    logits = _logits(4 * K, V, ld, sum(win, []), seed=V + 1)
    logits[0, hi] = 8.0  # the same bf16 value at a higher column of row 0 of sequences 0 and 1
    logits[K, hi] = 8.0
    pos, end = [p0, p0, p0, 12], 12
    g, seq, p, steps, hist = _accept(logits, V, K, rows, [1, 1, 1, 1], pos, end)
    assert g.tolist() == win
    for b, cnt in enumerate([2, 1, 2, 0]):
        assert O.accept(rows[b], win[b], True, pos[b], end)[1] == cnt
        _check(g, seq, p, steps, hist, b, pos[b], cnt, K)


@pytest.mark.parametrize("B,K", [(1, 8), (2, 4), (4, 2)], ids=lambda x: str(x))
def test_accept_shapes(B, K):
    """Every (B, K) with B * K = 8 at V = 9000: sequence b confirms b drafts (at most K - 1)."""
    V, p0 = 9000, 5
    win = [[100 * b + r + 1 for r in range(K)] for b in range(B)]
    rows = [[0] + [win[b][r - 1] if r <= min(b, K - 1) else 8999 for r in range(1, K)] for b in range(B)]
    g, seq, p, steps, hist = _accept(_logits(B * K, V, V, sum(win, []), seed=K), V, K, rows, [1] * B, [p0] * B, 39)
    assert g.tolist() == win
    for b in range(B):
        _check(g, seq, p, steps, hist, b, p0, min(b, K - 1) + 1, K)


def test_guard_bands():
    """Both kernels and the row argmax with every operand between guard bands: nothing outside an
    operand is read into the result or written."""
    C = ext()
    B, K, V, ld = 2, 4, 1003, 1008
    rng = np.random.default_rng(0)
    seq = torch.from_numpy(rng.integers(0, 3, (B, L))).cuda()

    def draft(seq, pos, ctl, tok, pos_rows, has):
        C.spec_draft(seq, pos, ctl, K, tok, pos_rows, has)

    _, io = guarded(draft, {"seq": seq, "pos": _i32([40, 63]), "ctl": _i32([3, 70, 0, 0])},
                    {"tok": torch.full((B * K, 1), -5, dtype=torch.long).cuda(), "pos_rows": _i32([-7] * (B * K)),
                     "has": _i32([-9] * B)}, name="spec_draft")
    for b, p in enumerate([40, 63]):
        rows, prow, h = O.draft(seq[b].cpu().numpy(), p, K, 3)
        assert io["tok"].view(B, K)[b].tolist() == rows.tolist() and int(io["has"][b]) == int(h)
        assert io["pos_rows"].view(B, K)[b].tolist() == prow.tolist()

    win = [5, 6, 7, 8, 1002, 0, 3, 4]
    logits = _logits(B * K, V, ld, win, seed=3).cuda()  # rows 1008 apart, 1003 wide
    logits[:, V:] = 0.0  # inside the operand: finite, and never the maximum's column

    def argmax(logits, g):
        C.spec_argmax(logits, V, g)

    _, io = guarded(argmax, {"logits": logits}, {"g": _i32([-1] * (B * K))}, name="spec_argmax")
    assert io["g"].tolist() == win

    def accept(g, tok, has, ctl, pos, seq, steps, hist):
        C.spec_accept(g, tok, has, K, pos, ctl, seq, steps, hist)

    rows = torch.tensor([[0, 5, 6, 9], [0, 1002, 0, 3]], dtype=torch.long).reshape(B * K, 1).cuda()
    _, io = guarded(accept, {"g": _i32(win), "tok": rows, "has": _i32([1, 1]), "ctl": _i32([3, 30, 0, 0])},
                    {"pos": _i32([10, 28]), "seq": torch.full((B, 32), -3, dtype=torch.long).cuda(),
                     "steps": _i32([0, 0]), "hist": _i32([0] * (B * (K + 1))).view(B, K + 1)}, name="spec_accept")
    assert io["pos"].tolist() == [13, 30] and io["steps"].tolist() == [1, 1]
    assert io["seq"][0, 11:14].tolist() == [5, 6, 7] and io["seq"][1, 29:31].tolist() == [1002, 0]
    assert int((io["seq"] != -3).sum()) == 5
    assert io["hist"].tolist() == [[0, 0, 0, 1, 0], [0, 0, 1, 0, 0]]
