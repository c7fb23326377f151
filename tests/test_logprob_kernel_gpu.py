"""The log-probability kernel (csrc/kernels/sample.hip, ``ext().logits_lse``) and the ``lse`` / ``lp``
arguments of the pick kernels (``sample_logits``, ``pick_ragged``), stand-alone, against the rule
restated in numpy float64 (tests/_logprob_oracle.py) on the same bf16 values.

Tolerance: four times the bound derived in common.h ('Per-token log-probabilities'),
``L.tol(V, lp)`` -- at every row, nothing skipped.  {m, lnz} is a function of the row's values alone
(integer mass sums), which the column-permutation test checks bitwise."""
import struct

import numpy as np
import pytest
import torch

import _logprob_oracle as L
from _guard import bit_equal, guarded

pytestmark = pytest.mark.gpu

KINDS = ["gauss", "equal", "spike", "neg_inf"]
UNTOUCHED = 123.0


@pytest.fixture(scope="module")
def C():
    from mingpt_distributed_amd.ops._ext import ext

    return ext()


def make_rows(kind, B, V, seed):
    """fp32 [B, V] whose bf16 rounding is the test row."""
    g = torch.Generator().manual_seed(seed)
    if kind == "gauss":
        return torch.randn(B, V, generator=g) * 3.0
    if kind == "equal":
        return torch.full((B, V), 1.375)
    if kind == "spike":  # one element at +80, the rest at -80: every other mass truncates to 0
        x = torch.full((B, V), -80.0)
        x[torch.arange(B), torch.randint(0, V, (B,), generator=g)] = 80.0
        return x
    x = torch.randn(B, V, generator=g) * 3.0  # neg_inf: about one entry in ten, never the maximum
    drop = torch.rand(B, V, generator=g) < 0.1
    drop[torch.arange(B), x.argmax(-1)] = False
    return x.masked_fill(drop, float("-inf"))


def padded(rows, pad=float("nan")):
    """bf16 [B, ld] on the GPU, ld = V rounded up to 8, ``pad`` in the columns from V on."""
    B, V = rows.shape
    full = torch.full((B, (V + 7) // 8 * 8), pad, dtype=torch.float32)
    full[:, :V] = rows
    return full.to(torch.bfloat16).cuda()


def pick_targets(l, shift):
    """Row r's target by (r + shift) % 3: the maximum, the lowest finite entry, or -1 (skipped)."""
    t = np.empty(len(l), dtype=np.int64)
    for r, row in enumerate(l):
        k = (r + shift) % 3
        t[r] = row.argmax() if k == 0 else (np.where(np.isneginf(row), np.inf, row).argmin() if k == 1 else -1)
    return t


def check_lse(lse, l, V):
    m, lnz = L.lse(l)
    got = lse.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, 0], m), "the row maximum is exact"
    err = np.abs(got[:, 1] - lnz)
    assert (err <= L.tol(V, 0.0)).all(), f"lnz off by {err.max():.3e}, allowed {L.tol(V, 0.0):.3e}"


@pytest.mark.parametrize("V", [1, 7, 8, 9, 1000, 4099, 50257, 65544])  # 65544: the streamed path
@pytest.mark.parametrize("B", [1, 3, 8])
def test_lse_and_targets(C, B, V):
    worst = 0.0
    for kind in KINDS:
        logits = padded(make_rows(kind, B, V, 7 * V + B))
        l = logits[:, :V].float().cpu().numpy().astype(np.float64)
        assert C.logits_lse(logits, V).shape == (B, 2)
        for shift in range(3):
            t = pick_targets(l, shift)
            lp0 = torch.full((B,), UNTOUCHED, dtype=torch.float32, device="cuda")
            lse, lp = C.logits_lse(logits, V, torch.from_numpy(t).cuda(), None, lp0)
            assert lp.data_ptr() == lp0.data_ptr() and lse.dtype == lp.dtype == torch.float32
            check_lse(lse, l, V)
            assert bit_equal(lse, C.logits_lse(logits, V)), "targets change {m, lnz}"
            got = lp.cpu().numpy().astype(np.float64)
            on = t >= 0
            assert (got[~on] == UNTOUCHED).all(), "a skipped row's lp was written"
            want = L.logprob(l[on], t[on])
            err, tol = np.abs(got[on] - want), L.tol(V, want)
            assert np.isfinite(got[on]).all() and (err <= tol).all(), (kind, shift, got[on], want, tol)
            worst = max(worst, float((err / tol).max()) if on.any() else 0.0)
    print(f"B {B} V {V}: worst error {worst:.3f} of the allowed")


def test_special_targets(C):
    """A target at a -inf logit gets -inf; a target >= V is skipped like a negative one; without a
    buffer the skipped entries are 0.0."""
    V = 1000
    rows = make_rows("gauss", 3, V, 5)
    rows[0, 17] = float("-inf")
    logits = padded(rows)
    lse, lp = C.logits_lse(logits, V, torch.tensor([17, V, -5], device="cuda"))
    assert lp.tolist() == [float("-inf"), 0.0, 0.0]
    check_lse(lse, logits[:, :V].float().cpu().numpy().astype(np.float64), V)


def test_rows_outside_the_rule(C):
    """A row without a finite maximum (all -inf, or holding NaN or +inf) is outside the rule: it may
    yield any value, and the other rows of the same launch are what they are without it."""
    V = 1000
    rows = make_rows("gauss", 4, V, 3)
    rows[0] = float("-inf")
    rows[1, 5] = float("nan")
    rows[2, 7] = float("inf")
    logits = padded(rows)
    t = torch.tensor([3, 3, 3, 3], device="cuda")
    lse, lp = C.logits_lse(logits, V, t)
    torch.cuda.synchronize()
    alone = C.logits_lse(logits[3:], V, t[3:])
    assert bit_equal(lse[3:], alone[0]) and bit_equal(lp[3:], alone[1])
    l = logits[3:, :V].float().cpu().numpy().astype(np.float64)
    want = L.logprob(l, np.array([3]))
    assert abs(float(lp[3]) - want[0]) <= L.tol(V, want[0])


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("V", [1000, 50257, 65544])
def test_order_independent_bitwise(C, B, V):
    """{m, lnz} of a row equals {m, lnz} of a column-permuted copy of it, bit for bit: the masses are
    integers, so which thread, wave or pass adds which element does not matter."""
    g = torch.Generator().manual_seed(V + B)
    for kind in ["gauss", "neg_inf"]:
        rows = make_rows(kind, B, V, V + B)
        perm = torch.stack([torch.randperm(V, generator=g) for _ in range(B)])
        a = C.logits_lse(padded(rows), V)
        b = C.logits_lse(padded(rows.gather(1, perm)), V)
        assert bit_equal(a, b), (kind, a, b)
        # and each row alone equals the row inside the batch (the workgroup sees only its row)
        one = C.logits_lse(padded(rows[B - 1:]), V)
        assert bit_equal(one, a[B - 1:])


@pytest.mark.parametrize("V", [9, 4099, 65544])
def test_guard_bands(C, V):
    """Inputs between NaN margins, outputs between sentinel margins: the results equal the plain
    run's and no margin byte changes (the NaN pad columns are part of the operand already)."""
    B = 3
    logits = padded(make_rows("gauss", B, V, V))
    l = logits[:, :V].float().cpu().numpy().astype(np.float64)
    t = pick_targets(l, 0)
    t[2] = V - 1  # the last column: one element before the NaN padding
    out, io = guarded(lambda logits, targets, lse, lp: C.logits_lse(logits, V, targets, lse, lp),
                      {"logits": logits, "targets": torch.from_numpy(t).cuda()},
                      {"lse": torch.zeros(B, 2, device="cuda"), "lp": torch.zeros(B, device="cuda")},
                      name=f"logits_lse V={V}")
    check_lse(io["lse"], l, V)
    want = L.logprob(l, t)
    assert (np.abs(io["lp"].cpu().numpy() - want) <= L.tol(V, want)).all()


def f32_bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def block(seed, draw, temperature, top_k, top_p, eos=-1):
    s32 = lambda x: ((x & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    return torch.tensor([s32(seed), s32(seed >> 32), s32(draw), f32_bits(1.0 / temperature), int(top_k or 0), eos,
                         f32_bits(top_p) if top_p else 0, 0], dtype=torch.int32, device="cuda")


def check_lp_plane(lp, seq, l, V, written):
    """lp [B, L] holds the oracle's number for token seq[b, c] at every (b, c) in ``written`` and
    UNTOUCHED everywhere else."""
    got = lp.cpu().numpy().astype(np.float64)
    mask = np.zeros(got.shape, dtype=bool)
    for b, c in written:
        mask[b, c] = True
        want = L.logprob(l[b], int(seq[b, c]))
        assert abs(got[b, c] - want) <= L.tol(V, want), (b, c, got[b, c], want)
    assert (got[~mask] == UNTOUCHED).all(), "lp written outside the advanced rows' [b, pos + 1]"


@pytest.mark.parametrize("V", [1000, 9000])
def test_sample_logits_with_lp(C, V):
    B, Lseq, p0 = 3, 12, 4
    logits = padded(make_rows("gauss", B, V, V + 1))
    l = logits[:, :V].float().cpu().numpy().astype(np.float64)
    lse = C.logits_lse(logits, V)

    def run(pos, with_lp):
        pb = block(99, 6, 0.9, 50, 0.9)
        pd = torch.tensor([pos], dtype=torch.int32, device="cuda")
        tok = torch.full((B,), -7, dtype=torch.long, device="cuda")
        seq = torch.full((B, Lseq), -3, dtype=torch.long, device="cuda")
        lp = torch.full((B, Lseq), UNTOUCHED, dtype=torch.float32, device="cuda")
        C.sample_logits(logits, V, pb, pd, tok, seq, *((lse, lp) if with_lp else ()))
        return pb, pd, tok, seq, lp

    plain, got = run(p0, False), run(p0, True)
    for a, b in zip(plain[:4], got[:4]):
        assert torch.equal(a, b), "the tokens or the state changed with lse / lp given"
    assert int(got[1]) == p0 + 1 and ((got[2] >= 0) & (got[2] < V)).all()
    check_lp_plane(got[4], got[3].cpu().numpy(), l, V, [(b, p0 + 1) for b in range(B)])
    assert (plain[4] == UNTOUCHED).all()
    # at capacity (column pos + 1 is past the plane): neither the token nor its lp is stored
    plain, got = run(Lseq - 1, False), run(Lseq - 1, True)
    for a, b in zip(plain[:4], got[:4]):
        assert torch.equal(a, b)
    assert (got[3] == -3).all() and (got[4] == UNTOUCHED).all()
    with pytest.raises(RuntimeError, match="lse and lp go together"):
        C.sample_logits(logits, V, block(1, 0, 1.0, 0, None), None, None, None, lse, None)


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("V", [1000, 9000])
def test_pick_ragged_with_lp(C, V, greedy):
    """Row 0 advances, row 1 is at capacity (its next column would be the last), row 2 is finished:
    only lp[0, pos[0] + 1] is written, and everything else is what the call without lse / lp leaves."""
    B, Lseq = 3, 12
    logits = padded(make_rows("gauss", B, V, V + 2))
    l = logits[:, :V].float().cpu().numpy().astype(np.float64)
    lse = C.logits_lse(logits, V)

    def run(with_lp, eos=-1):
        pb = block(99, 0, 0.9, 50, 0.9, eos)
        pos = torch.tensor([2, Lseq - 2, 5], dtype=torch.int32, device="cuda")
        done = torch.tensor([0, 0, 1], dtype=torch.int32, device="cuda")
        tok = torch.full((B, 1), -7, dtype=torch.long, device="cuda")
        seq = torch.full((B, Lseq), -3, dtype=torch.long, device="cuda")
        lp = torch.full((B, Lseq), UNTOUCHED, dtype=torch.float32, device="cuda")
        C.pick_ragged(logits, V, pb, pos, done, tok, seq, greedy, *((lse, lp) if with_lp else ()))
        return pb, pos, done, tok, seq, lp

    plain, got = run(False), run(True)
    for a, b in zip(plain[:5], got[:5]):
        assert torch.equal(a, b), "the tokens or the state changed with lse / lp given"
    assert got[1].tolist() == [3, Lseq - 2, 5] and got[2].tolist() == [0, 0, 1]
    t0 = int(got[4][0, 3])
    assert 0 <= t0 < V and (not greedy or t0 == int(l[0].argmax()))
    check_lp_plane(got[5], got[4].cpu().numpy(), l, V, [(0, 3)])
    if greedy:  # the greedy token sits at the maximum: lp = -lnz exactly
        assert float(got[5][0, 3]) == -float(lse[0, 1])
    # the stop token is a generated token: its lp is written in the launch that finishes the row
    plain, got = run(False, t0), run(True, t0)
    for a, b in zip(plain[:5], got[:5]):
        assert torch.equal(a, b)
    assert got[2].tolist() == [1, 0, 1]
    check_lp_plane(got[5], got[4].cpu().numpy(), l, V, [(0, 3)])
