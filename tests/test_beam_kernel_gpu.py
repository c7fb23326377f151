"""The beam-search kernels (csrc/kernels/beam.hip) driven stand-alone through ``ext().beam_rows``,
``beam_merge`` and ``beam_reorder``: the row and merge kernels against the rule restated in numpy
float64 (tests/_beam_oracle.py) with the derived band ``d = L.tol(V, lp) + 2^-23 |c|``, hand-built
exact cases for every tie-break, the in-place cache reorder against ``index_select`` bit for bit, and
all three between guard bands."""
import numpy as np
import pytest
import torch

import _beam_oracle as O
from _guard import bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1000, 1000), (2, 4, 997, 1000), (1, 8, 9000, 9000), (3, 3, 50257, 50264), (1, 2, 66001, 66008)]
LH, COL = 6, 4  # history length and the column the step writes
NINF = float("-inf")


def _logits(R, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    l = torch.full((R, ld), float("nan"))  # the pad columns are never read
    l[:, :V] = torch.randn(R, V, generator=g) * 3.0
    return l.to(torch.bfloat16).cuda()


def _state(B, W, scores, fin=None, pad=0, eos=-1, pos=10, lens=None):
    R = B * W
    i32 = lambda x: torch.as_tensor(x, dtype=torch.int32).reshape(-1).cuda()
    return {"score": torch.as_tensor(scores, dtype=torch.float32).reshape(R).cuda(),
            "fin": i32(fin if fin is not None else [0] * R), "len": i32(lens if lens is not None else [7] * R),
            "ctl": i32([COL, eos, pad, 0]), "pos": i32([pos]),
            "tok": torch.full((R, 1), -5, dtype=torch.long).cuda(), "parent": i32([-7] * R),
            "cand_tok": i32([-9] * (R * W)).view(R, W), "cand_c": torch.full((R, W), 123.0).cuda(),
            "lse": torch.full((R, 2), 123.0).cuda(),
            "hparent": i32([-3] * (R * LH)).view(B, W, LH), "htok": i32([-3] * (R * LH)).view(B, W, LH),
            "hscore": torch.full((B, W, LH), 77.0).cuda()}


def _step(logits, V, W, st):
    """The row kernel then the merge on ``st`` (in place); returns the state going in (host copies)."""
    before = {k: st[k].clone() for k in ("score", "fin", "len")}
    C = ext()
    C.beam_rows(logits, V, W, st["score"], st["fin"], st["ctl"], st["cand_tok"], st["cand_c"], st["lse"])
    C.beam_merge(W, V, st["cand_tok"], st["cand_c"], st["score"], st["fin"], st["len"], st["tok"], st["parent"],
                 st["hparent"], st["htok"], st["hscore"], st["pos"], st["ctl"])
    torch.cuda.synchronize()
    return before


def _bookkeeping(st, before, B, W, pos0=10):
    """What the merge writes besides the choice itself: the history column, the next input token,
    the lengths, the position -- and nothing in the other history columns."""
    par, tok = st["parent"].view(B, W).long(), st["tok"].view(B, W)
    assert int(st["pos"]) == pos0 + 1 and int(st["ctl"][0]) == COL
    assert torch.equal(st["hparent"][:, :, COL].long(), par) and torch.equal(st["htok"][:, :, COL].long(), tok)
    assert torch.equal(st["hscore"].view(torch.int32)[:, :, COL], st["score"].view(torch.int32).view(B, W))
    keep = [c for c in range(LH) if c != COL]
    assert (st["hparent"][:, :, keep] == -3).all() and (st["htok"][:, :, keep] == -3).all()
    assert (st["hscore"][:, :, keep] == 77.0).all()
    pfin = before["fin"].view(B, W).gather(1, par)
    assert torch.equal(st["len"].view(B, W), before["len"].view(B, W).gather(1, par) + (1 - pfin))
    eos = int(st["ctl"][1])
    assert torch.equal(st["fin"].view(B, W).bool(), pfin.bool() | ((tok == eos) if eos >= 0 else False))


@pytest.mark.parametrize("B,W,V,ld", SHAPES, ids=[f"B{b}-W{w}-V{v}" for b, w, v, _ in SHAPES])
def test_band_check_random(B, W, V, ld):
    """Random normal logits (sigma 3) and random finite scores: the band check on every prompt,
    {m, lnz} bit-equal to ``logits_lse``, the bookkeeping; one beam of a three-beam prompt frozen."""
    R = B * W
    logits = _logits(R, V, ld, seed=V + W)
    g = torch.Generator().manual_seed(V)
    scores = -torch.rand(R, generator=g) * 40.0
    fin = [0] * R
    if W == 3:
        fin[1 * W + 2] = 1  # prompt 1, beam 2
    st = _state(B, W, scores, fin, pad=5, eos=int(torch.randint(0, V, (1,), generator=g)))
    before = _step(logits, V, W, st)
    assert bit_equal(st["lse"], ext().logits_lse(logits, V))
    _bookkeeping(st, before, B, W)
    lf = logits[:, :V].float().cpu().numpy()
    sharp = 0
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        sharp += O.band_check(before["score"][rows].cpu().numpy(), before["fin"][rows].cpu().numpy() != 0, lf[rows], 5,
                              st["parent"][rows].cpu().numpy(), st["tok"][rows, 0].cpu().numpy(),
                              st["score"][rows].cpu().numpy(), what=f"prompt {b}")
    print(f"sharp cut (chosen set equal to the oracle's) at {sharp} of {B} prompts")


def test_equal_scores_lower_beam_first():
    V, W = 1000, 2
    logits = _logits(1, V, V, seed=1).expand(2, V).contiguous()
    st = _state(1, W, [-1.0, -1.0])
    _step(logits, V, W, st)
    top = int(logits[0].float().argmax())
    assert st["parent"].tolist() == [0, 1] and st["tok"].view(-1).tolist() == [top, top]
    assert bit_equal(st["score"][:1], st["score"][1:])


def test_maximum_at_three_indices_and_start_state():
    """Only beam 0 is live at the start: the W chosen are its first W entries in (logit descending,
    index ascending) order -- three equal maxima in index order, then bf16 ties as a stable sort."""
    V, W = 1000, 3
    logits = _logits(W, V, V, seed=2)
    logits[:, [17, 400, 999]] = 50.0
    st = _state(1, W, [0.0, NINF, NINF])
    _step(logits, V, W, st)
    assert st["parent"].tolist() == [0, 0, 0] and st["tok"].view(-1).tolist() == [17, 400, 999]
    V, W = 997, 8
    logits = _logits(W, V, 1000, seed=3)
    st = _state(1, W, [0.0] + [NINF] * 7)
    _step(logits, V, W, st)
    want = torch.sort(logits[0, :V].float(), descending=True, stable=True).indices[:W]
    assert st["parent"].tolist() == [0] * W and torch.equal(st["tok"].view(-1), want)
    lp = O.candidates([0.0], [False], logits[:1, :V].float().cpu().numpy(), 0)
    err = np.abs(st["score"].cpu().numpy().astype(np.float64) - lp[0][0, want.cpu().numpy()])
    assert (err <= lp[1][0, want.cpu().numpy()]).all()


def test_finished_beam_in_the_middle():
    V, W, pad = 1000, 3, 11
    row = torch.zeros(V)
    row[0], row[1] = 3.0, 1.0  # the second entry is 2 below the first
    logits = row.to(torch.bfloat16).expand(W, V).contiguous().cuda()
    c, _, _ = O.candidates([-0.5], [False], row[None].numpy(), pad)
    frozen = np.float32(c[0, 0] - 0.3)  # below beam 0's best, above everything else
    st = _state(1, W, [-0.5, float(frozen), -9.0], fin=[0, 1, 0], pad=pad, lens=[7, 5, 7])
    before = _step(logits, V, W, st)
    _bookkeeping(st, before, 1, W)
    assert st["parent"].tolist() == [0, 1, 0] and st["tok"].view(-1).tolist() == [0, pad, 1]
    assert st["score"][1].item() == frozen and st["fin"].tolist() == [0, 1, 0] and st["len"].tolist() == [8, 5, 8]


def test_minus_inf_logits_rank_last():
    V, W = 1000, 4
    row = torch.full((V,), NINF)
    row[[300, 20]] = torch.tensor([1.0, 0.5])
    logits = row.to(torch.bfloat16).expand(W, V).contiguous().cuda()
    st = _state(1, W, [-1.0, -2.0, -3.0, -4.0])
    _step(logits, V, W, st)  # eight finite candidates: none of the -inf ones is chosen
    assert torch.isfinite(st["score"]).all() and set(st["tok"].view(-1).tolist()) <= {300, 20}
    assert (st["score"][:-1] >= st["score"][1:]).all()
    st = _state(1, W, [0.0, NINF, NINF, NINF])
    _step(logits, V, W, st)  # two finite candidates, then beam 0's first -inf entries
    assert st["parent"].tolist() == [0] * 4 and st["tok"].view(-1).tolist() == [300, 20, 0, 1]
    assert torch.isfinite(st["score"][:2]).all() and (st["score"][2:] == NINF).all()


def _cache(L, R, Tmax, D, seed, finite=False):
    g = torch.Generator().manual_seed(seed)
    if finite:
        return torch.randn(L, R, Tmax, 3 * D, generator=g).to(torch.bfloat16).cuda()
    bits = torch.randint(-32768, 32768, (L, R, Tmax, 3 * D), generator=g, dtype=torch.int16)
    return bits.view(torch.bfloat16).cuda()


@pytest.mark.parametrize("pos", [0, 5, 63])
@pytest.mark.parametrize("W,L", [(4, 1), (8, 2), (3, 2)])
def test_reorder_equals_index_select(pos, W, L):
    """Random bits, D = 128, Tmax = 64, prompts with random parents, the identity and all-from-one:
    rows 0..pos of the K / V columns equal ``index_select``; later rows, the Q columns and an
    identity prompt are bit-unchanged; the history column advances when ctl is given."""
    D, Tmax, B = 128, 64, 3
    R = B * W
    kv = _cache(L, R, Tmax, D, seed=pos + W)
    g = torch.Generator().manual_seed(W)
    parent = torch.stack([torch.randint(0, W, (W,), generator=g), torch.arange(W), torch.full((W,), W - 1)])
    rows = (torch.arange(B).view(B, 1) * W + parent).view(R).cuda()
    want = kv.clone()
    want[:, :, :pos + 1, D:] = kv.index_select(1, rows)[:, :, :pos + 1, D:]
    got = kv.clone()
    ctl = torch.tensor([9, -1, 0, 0], dtype=torch.int32).cuda()
    n = torch.tensor([pos + 1], dtype=torch.int32).cuda()
    ext().beam_reorder(got, W, parent.view(R).to(torch.int32).cuda(), n, ctl)
    assert bit_equal(got, want)
    assert ctl.tolist() == [10, -1, 0, 0] and int(n) == pos + 1
    one = kv.clone()  # layer by layer, without ctl
    for i in range(L):
        ext().beam_reorder(one[i:i + 1], W, parent.view(R).to(torch.int32).cuda(), n)
    assert bit_equal(one, want)


def test_guard_bands():
    """All three kernels between NaN input margins and sentinel output margins."""
    C = ext()
    B, W, V, ld = 2, 4, 997, 1000
    R = B * W
    st = _state(B, W, -torch.rand(R, generator=torch.Generator().manual_seed(0)) * 10.0)
    logits = _logits(R, V, ld, seed=9)
    logits[:, V:] = 0.0  # guarded() wants finite operands; the margins carry the NaN
    _, io = guarded(lambda **k: C.beam_rows(k["logits"], V, W, k["score"], k["fin"], k["ctl"], k["cand_tok"],
                                            k["cand_c"], k["lse"]),
                    {k: v for k, v in (("logits", logits), ("score", st["score"]), ("fin", st["fin"]),
                                       ("ctl", st["ctl"]))},
                    {k: st[k] for k in ("cand_tok", "cand_c", "lse")}, name="beam_rows")
    names = ("score", "fin", "len", "tok", "parent", "hparent", "htok", "hscore", "pos")
    guarded(lambda **k: C.beam_merge(W, V, k["cand_tok"], k["cand_c"], k["score"], k["fin"], k["len"], k["tok"],
                                     k["parent"], k["hparent"], k["htok"], k["hscore"], k["pos"], k["ctl"]),
            {"cand_tok": io["cand_tok"], "cand_c": io["cand_c"], "ctl": st["ctl"]},
            {k: st[k] for k in names}, name="beam_merge")
    kv = _cache(2, R, 64, 128, seed=4, finite=True)
    parent = torch.tensor([2, 0, 0, 3, 1, 1, 0, 2], dtype=torch.int32).cuda()
    guarded(lambda **k: C.beam_reorder(k["kv"], W, k["parent"], k["pos"], k["ctl"]),
            {"parent": parent, "pos": torch.tensor([40], dtype=torch.int32).cuda()},
            {"kv": kv, "ctl": st["ctl"].clone()}, name="beam_reorder")
