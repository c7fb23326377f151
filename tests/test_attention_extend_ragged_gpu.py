"""``attention_extend_ragged`` (varlen chunk attention over the KV cache) against fp64 on the peaked two-target
probes of tests/_attn_probe.py, as tests/test_attention_extend_gpu.py does for the uniform kernel: sequence b is
its own probe of length base_b + Tq_b; its rows below base_b are the cache (K/V thirds only, everything else
NaN), the rest go into the packed chunk.  Tolerance: ``_attn_probe.OUT_TOL``; each case prints its violation
(error / tolerance) before it asserts.  The cases: nothing cached, the 64-key tile edge and the 32-query block
edge; a mixed plan (two sequences split, one not); five query blocks beside one with the straddling tile; the head
dims of the other instantiations.

On an MI355X the violations are listed in PERF.md 'Prefix reuse, ragged'."""
import pytest
import torch

import _attn_probe as P
from _guard import bit_equal
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 2
MIXED = (64, ((700, 20), (3, 2), (960, 64)))
CASES = [(64, ((0, 5), (63, 1), (64, 33))), MIXED, (64, ((200, 130), (65, 31))),
         (128, ((300, 40), (10, 7))), (80, ((300, 40), (10, 7))), (8, ((300, 40), (10, 7)))]


def _setup(hd, seqs, seed):
    """(packed qkv_new [M, 3D], cache [B, Tmax, 3D] with NaN wherever the call may not look, the probes by
    sequence [T_b, 3D], the lists tq and base)."""
    D, Tmax = H * hd, max(b + t for b, t in seqs) + 37
    cache = torch.full((len(seqs), Tmax, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    new, probes = [], []
    for b, (base, Tq) in enumerate(seqs):
        qkv = P.probe_qkv(1, base + Tq, H, hd, seed + b)[0].to(DEV)
        cache[b, :base, D:] = qkv[:base, D:]
        new.append(qkv[base:])
        probes.append(qkv)
    return torch.cat(new).contiguous(), cache, probes, [t for _, t in seqs], [b for b, _ in seqs]


def _run(new, cache, tq, base):
    C = ext()
    return C.attention_extend_ragged(new, cache, H, tq, base, C.attention_extend_ragged_plan(tq, base, H, cache).to(DEV))


@pytest.mark.parametrize("hd,seqs", CASES)
def test_against_fp64(hd, seqs):
    D = H * hd
    new, cache, probes, tq, base = _setup(hd, seqs, seed=hd + sum(tq for _, tq in seqs))
    before = cache.clone()
    if (hd, seqs) == MIXED:
        S = ext().attention_extend_ragged_splits(tq, base, H, cache)
        assert S[0] > 1 and S[1] == 1 and S[2] > 1, S
    out = _run(new, cache, tq, base)
    assert torch.isfinite(out.float()).all()
    cu = 0
    for b, (p, t) in enumerate(seqs):
        T = p + t
        ref = P.ref64(probes[b], torch.zeros(T, D, device=DEV), 1, T, H)[0][p:]
        v = P.violation(out[cu:cu + t], ref, **P.OUT_TOL)
        print(f"PROBE extend_ragged hd={hd} seq={b} base={p} Tq={t}: out {v:.3f}")
        assert v <= 1, (b, v)
        # the chunk's K / V thirds appended bit for bit; everything else keeps its bits
        assert bit_equal(cache[b, p:T, D:], new[cu:cu + t, D:])
        assert bit_equal(cache[b, :p], before[b, :p]) and bit_equal(cache[b, T:], before[b, T:])
        cu += t
    assert bit_equal(cache[:, :, :D], before[:, :, :D])


@pytest.mark.parametrize("hd,seqs,keep", [MIXED + (0,), (64, ((200, 130), (65, 31)), 1)])
def test_a_sequence_sees_only_itself(hd, seqs, keep):
    new, cache, _, tq, base = _setup(hd, seqs, seed=5)
    out = _run(new, cache.clone(), tq, base)
    new2, cache2, _, _, _ = _setup(hd, seqs, seed=50)
    lo = sum(tq[:keep])
    rows = slice(lo, lo + tq[keep])
    new2[rows] = new[rows]
    cache2[keep] = cache[keep]
    out2 = _run(new2, cache2, tq, base)
    assert bit_equal(out2[rows], out[rows])
    for b in range(len(seqs)):
        if b != keep:
            r = slice(sum(tq[:b]), sum(tq[:b + 1]))
            assert not bit_equal(out2[r], out[r])
