"""The process kernel (csrc/kernels/process.hip) against the rule restated in numpy
(tests/_process_oracle.py), bit for bit over every column of the logits buffer, padding included."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _guard as G
import _process_oracle as P
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPES = [(1000, 1000), (997, 1000), (50257, 50264)]
SETTINGS = {
    "repetition": dict(rp=1.3),
    "repetition_below_1": dict(rp=0.7),
    "presence": dict(pp=0.6),
    "frequency": dict(fp=0.37),
    "ngram1": dict(g=1),
    "ngram2": dict(g=2),
    "ngram3": dict(g=3),
    "ngram4": dict(g=4),
    "ngram8": dict(g=8),
    "all": dict(rp=1.7, pp=0.25, fp=-0.13, g=3),
}
ALL = SETTINGS["all"]
PAD = 123.0  # what the padding columns V .. ld - 1 hold going in


def _words(s):
    w = gen._proc_words(s.get("rp", 1.0), s.get("pp", 0.0), s.get("fp", 0.0), s.get("g", 0))
    return torch.tensor(w, dtype=torch.int32, device="cuda")


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _logits(R, V, ld, seed):
    """bf16 [R, ld]: positive and negative values with +0, -0 and -inf sprinkled over a quarter of
    the row (its finite maximum stays), PAD in the padding."""
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(R, ld, generator=g) * 3.0
    kind = torch.randint(0, 12, (R, ld), generator=g)
    l[kind == 0] = 0.0
    l[kind == 1] = -0.0
    l[kind == 2] = float("-inf")
    l[:, V:] = PAD
    return l.to(torch.bfloat16).cuda()


def _hist(R, n, V, alpha, seed):
    """int64 [R, n] over the first ``alpha`` symbols; row 0 is all one token (c = n), and the tail of
    row R - 1 repeats its head, so every n-gram size up to 8 finds a match."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randint(0, alpha, (R, n), generator=g)
    h[0] = h[0, 0]
    if n >= 20:
        h[R - 1, n - 9:] = h[R - 1, :9]
    return h.cuda()


def _run(logits, V, hist, pos, s, done=None):
    """The kernel on a copy of ``logits``: ``pos`` int32 [1] or [R] on the device."""
    out = logits.clone()
    ext().logits_process(out, V, hist, pos, int(pos.numel() > 1), done, _words(s))
    return out


def _want(logits, V, hist, pos, s, done=None):
    R = logits.size(0)
    p = pos.cpu().tolist() * (R if pos.numel() == 1 else 1)
    h = hist.cpu().tolist()
    bits = _bits(logits)
    rows = []
    for r in range(R):
        skip = done is not None and int(done[r])
        rows.append(bits[r] if skip else P.process_row(bits[r], h[r][:p[r] + 1], V=V, **s))
    return np.stack(rows)


def _check(logits, V, hist, pos, s, done=None, what=""):
    got = _bits(_run(logits, V, hist, pos, s, done))
    want = _want(logits, V, hist, pos, s, done)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} elements differ, first at (row, col) {tuple(bad[0])}: "
                           f"got {got[tuple(bad[0])]:#06x}, want {want[tuple(bad[0])]:#06x}")
    return got


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("n,R", [(1, 1), (2, 3), (255, 64), (256, 3), (257, 1), (1024, 3), (4096, 64)])
def test_shapes_rows_and_history_lengths(V, ld, n, R):
    """All processors together at every shape, row count and history length, with one position for
    the batch and with one per row (rows then stop 0, 1, 2 ... tokens short: the columns past a
    row's position are not its history)."""
    R = 3 if (R == 64 and V > 1000 and n == 4096) else R  # 64 rows x 4096 ids is covered at V = 1000
    logits = _logits(R, V, ld, n)
    hist = _hist(R, n, V, 50, n + 1)
    _check(logits, V, hist, _i32([n - 1]), ALL, what="one pos")
    per_row = _i32([max(0, n - 1 - (r % 5)) for r in range(R)])
    got = _check(logits, V, hist, per_row, ALL, what="per-row pos")
    assert (got[:, V:] == _bits(logits)[:, V:]).all()  # the padding is as it was


@pytest.mark.parametrize("name", list(SETTINGS))
def test_processors_and_history_contents(name):
    """Each processor alone and all together (g = 1, 2, 3, 4, 8, histories shorter than g included)
    over histories of one token, of tokens 0 and V - 1, and of alphabets of 2, 50 and V symbols;
    the sprinkled logits put +0, -0, -inf, positive and negative values under history tokens."""
    s = SETTINGS[name]
    V, ld, R = 997, 1000, 3
    logits = _logits(R, V, ld, 7)
    logits[0, 0], logits[1, 0], logits[2, 0] = 0.0, -0.0, float("-inf")
    logits[0, V - 1], logits[1, V - 1], logits[2, 1] = -0.0, 2.5, -1.25
    for n in (3, 7, 300):
        for alpha in (1, 2, 50, V):
            hist = _hist(R, n, V, alpha, n * 7 + alpha)
            _check(logits, V, hist, _i32([n - 1]), s, what=f"{name} n={n} alphabet={alpha}")
        ends = (torch.randint(0, 2, (R, n)) * (V - 1)).cuda()  # tokens 0 and V - 1 only
        _check(logits, V, ends, _i32([n - 1, n - 2, n - 3]), s, what=f"{name} n={n} ends")


def test_identity_when_off():
    for V, ld in SHAPES:
        logits = _logits(3, V, ld, 1)
        hist = _hist(3, 300, V, 50, 2)
        out = _run(logits, V, hist, _i32([299]), {})
        assert G.bit_equal(out, logits)


def test_finished_rows_are_left_alone():
    V, ld, R = 997, 1000, 5
    logits = _logits(R, V, ld, 3)
    hist = _hist(R, 40, V, 5, 4)
    done = _i32([0, 1, 0, 1, 1])
    pos = _i32([39, 39, 20, 0, 39])
    out = _run(logits, V, hist, pos, ALL, done=done)
    want = _want(logits, V, hist, pos, ALL, done=done.cpu().tolist())
    assert np.array_equal(_bits(out), want)
    assert G.bit_equal(out[1], logits[1]) and G.bit_equal(out[3], logits[3]) and G.bit_equal(out[4], logits[4])
    assert not G.bit_equal(out[0], logits[0]) and not G.bit_equal(out[2], logits[2])
    neg = _run(logits, V, hist, _i32([-1]), ALL)  # no history: nothing to do
    assert G.bit_equal(neg, logits)


def test_graph_replay_equals_eager():
    """A captured launch replays to the eager result, and a second replay on fresh logits with other
    settings in the parameter block equals the eager run of those: nothing is kept between launches
    and nothing comes from the host."""
    V, ld, R, n = 997, 1000, 3, 300
    C = ext()
    fresh = _logits(R, V, ld, 5)
    hist = _hist(R, n, V, 50, 6)
    pos = _i32([n - 1, n - 5, 17])
    eager = _run(fresh, V, hist, pos, ALL)
    buf, words = fresh.clone(), _words(ALL)
    C.logits_process(buf, V, hist, pos, 1, None, words)  # warm-up
    buf.copy_(fresh)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        C.logits_process(buf, V, hist, pos, 1, None, words)
    buf.copy_(fresh)
    graph.replay()
    first = buf.clone()
    assert G.bit_equal(first, eager)
    buf.copy_(fresh)
    graph.replay()
    assert G.bit_equal(buf, first)
    other = dict(rp=0.8, pp=-0.3, fp=0.05, g=2)
    words.copy_(_words(other))
    pos.copy_(_i32([5, n - 1, 40]))
    buf.copy_(fresh)
    graph.replay()
    assert G.bit_equal(buf, _run(fresh, V, hist, pos, other))


@pytest.mark.parametrize("V,ld", SHAPES)
def test_guard_bands(V, ld):
    """Logits and history inside guard bands: the margins are untouched, and NaN / zero ids beside the
    operands do not reach the result; history columns past a row's position are never read (ids
    far outside the vocabulary there change nothing)."""
    R, n = 3, 257
    logits = _logits(R, V, ld, 8)
    hist = _hist(R, n, V, 50, 9)
    pos = _i32([n - 1, 100, 0])
    plain = _run(logits, V, hist, pos, ALL)
    lbuf, lview = G.arena(logits, G.SENTINEL)
    hbuf, hview = G.arena(hist, G.POISON)
    for r, p in enumerate(pos.cpu().tolist()):
        hview[r, p + 1:] = 1 << 40
    ext().logits_process(lview, V, hview, pos, 1, None, _words(ALL))
    G.assert_intact(lbuf, lview, "logits")
    G.assert_intact(hbuf, hview, "hist")
    assert G.bit_equal(lview, plain)
    assert np.array_equal(_bits(plain), _want(logits, V, hist, pos, ALL))


def test_row_isolation():
    """A row's result is the same alone and among 63 others, and a strided history view works."""
    V, ld, n = 997, 1000, 300
    logits = _logits(64, V, ld, 10)
    wide = _hist(64, n + 11, V, 50, 11)
    hist = wide[:, :n]  # rows n + 11 apart
    pos = _i32([max(0, n - 1 - 3 * r) for r in range(64)])
    full = _run(logits, V, hist, pos, ALL)
    for r in (0, 17, 63):
        alone = _run(logits[r:r + 1], V, hist[r:r + 1].contiguous(), pos[r:r + 1].clone(), ALL)
        assert G.bit_equal(alone[0], full[r]), r


def test_ids_outside_the_vocabulary_count_for_nothing():
    """V, V + 5 (a padding column), -1 and 2^32 + 3 inside the history: no count, no ban, equal to
    nothing in an n-gram comparison -- not even to each other or to token 3."""
    V, ld, n = 997, 1000, 40
    logits = _logits(3, V, ld, 12)
    for g in (1, 2, 3):
        hist = _hist(3, n, V, 5, 13)
        hist[0, 3], hist[0, 17], hist[0, n - 1] = V, -1, V + 5
        hist[1, n - 2:] = torch.tensor([-1, 2], device="cuda")
        hist[1, 4:6] = torch.tensor([-1, 2], device="cuda")
        hist[2, ::2] = (1 << 32) + 3
        got = _check(logits, V, hist, _i32([n - 1]), dict(ALL, g=g), what=f"foreign ids, g={g}")
        assert (got[:, V:] == _bits(logits)[:, V:]).all()


def test_binding_rejects_bad_arguments():
    C = ext()
    logits, hist, pos, w = _logits(2, 997, 1000, 1), _hist(2, 8, 997, 5, 1), _i32([7]), _words(ALL)
    with pytest.raises(RuntimeError):
        C.logits_process(logits, 997, torch.zeros(2, 4097, dtype=torch.long, device="cuda"), pos, 0, None, w)
    with pytest.raises(RuntimeError):
        C.logits_process(logits, 997, hist.int(), pos, 0, None, w)
    with pytest.raises(RuntimeError):
        C.logits_process(logits, 997, hist, pos, 1, None, w)  # per-row pos needs R entries
    with pytest.raises(RuntimeError):
        C.logits_process(logits, 997, hist[:1], pos, 0, None, w)
    with pytest.raises(RuntimeError):
        C.logits_process(logits, 997, hist, pos, 0, None, w[:4])


CHILD = r'''
import torch
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import DeviceCheckError, ext

C = ext()
assert C.debug_build(), "expected the MG_DEBUG build"
V = 997
logits = torch.randn(2, 1000, device="cuda").to(torch.bfloat16)
words = torch.tensor(gen._proc_words(1.5, 0.1, 0.1, 2), dtype=torch.int32, device="cuda")
pos = torch.tensor([5], dtype=torch.int32, device="cuda")
hist = torch.randint(0, V, (2, 8), device="cuda")
C.logits_process(logits, V, hist, pos, 0, None, words)  # valid ids: no check fires
bad = hist.clone()
bad[1, 7] = V + 5  # past the position: never read
C.logits_process(logits, V, bad, pos, 0, None, words)
for v in (V, -1):
    bad = hist.clone()
    bad[1, 3] = v
    try:
        C.logits_process(logits, V, bad, pos, 0, None, words)
    except DeviceCheckError as e:
        assert "logits_process" in str(e) and "history token id" in str(e), str(e)
        print("caught:", e)
    else:
        raise AssertionError("out-of-range history id not reported")
    assert C.debug_error_bits() == 0
print("debug checks ok")
'''


def test_debug_build_reports_out_of_range_history_ids():
    so = os.path.join(ROOT, "build", "debug", "_C.so")
    assert os.path.exists(so), "build/debug/_C.so missing: python build_ext.py --debug"
    env = dict(os.environ, MINGPT_EXT_SO=so, MINGPT_DEBUG_CHECKS="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=150)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "debug checks ok" in r.stdout
    assert r.stdout.count("caught:") == 2
