"""``attention_extend`` (chunk attention over the KV cache) against fp64 on the peaked two-target probes
of tests/_attn_probe.py: rows below ``base`` of a probe of length base + Tq are the cache, the rest are
the new chunk, and every cache element the kernel must not read into a result -- rows at or past base,
every Q third -- is NaN going in.  Tolerance: ``_attn_probe.OUT_TOL`` (the training forward's); each case
prints its violation (error / tolerance) before it asserts.  The cases are the smallest at which each
mechanism can go wrong: base against the 64-key tile edge, Tq against the 32-query wave, two query
blocks, key splits with the combine launch, and the head dims of the other instantiations.

On an MI355X the violations were 0.087 (hd 8) to 0.227 ((64, 0, 200)); the list is in PERF.md 'Prefix reuse'."""
import pytest
import torch

import _attn_probe as P
from _guard import bit_equal
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 2, 2
SPLIT = [(64, 700, 20), (64, 960, 64)]  # S > 1: partial states and the combine launch
CASES = [(64, 0, 200), (64, 1, 1), (64, 63, 1), (64, 64, 33), (64, 65, 31), (64, 200, 130)] + SPLIT + [
    (128, 300, 40), (80, 300, 40), (8, 300, 40)]


def _setup(hd, base, Tq, seed):
    """(qkv_new [B * Tq, 3D], cache [B, Tmax, 3D] with NaN wherever the call may not look, the whole probe)."""
    T, D = base + Tq, H * hd
    qkv, _, _ = P.probe_qkv(B, T, H, hd, seed)
    qkv = qkv.to(DEV).view(B, T, 3 * D)
    cache = torch.full((B, T + 37, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    cache[:, :base, D:] = qkv[:, :base, D:]
    return qkv[:, base:].reshape(B * Tq, 3 * D).contiguous(), cache, qkv


@pytest.mark.parametrize("hd,base,Tq", CASES)
def test_against_fp64(hd, base, Tq):
    C, T, D = ext(), base + Tq, H * hd
    new, cache, qkv = _setup(hd, base, Tq, seed=hd + base + Tq)
    before = cache.clone()
    assert C.attention_extend_splits(B, Tq, H, base) > 1 or (hd, base, Tq) not in SPLIT
    out = C.attention_extend(new, cache, H, base)
    ref = P.ref64(qkv.view(B * T, 3 * D), torch.zeros(B * T, D, device=DEV), B, T, H)[0]
    v = P.violation(out, ref.view(B, T, D)[:, base:].reshape(B * Tq, D), **P.OUT_TOL)
    print(f"PROBE extend hd={hd} base={base} Tq={Tq}: out {v:.3f}")
    assert torch.isfinite(out.float()).all() and v <= 1, v
    # the chunk's K / V thirds appended bit for bit; everything else keeps its bits
    assert bit_equal(cache[:, base:T, D:], new.view(B, Tq, 3 * D)[:, :, D:])
    assert bit_equal(cache[:, :base], before[:, :base]) and bit_equal(cache[:, T:], before[:, T:])
    assert bit_equal(cache[:, :, :D], before[:, :, :D])


@pytest.mark.parametrize("hd,base,Tq", [(64, 65, 31), (64, 700, 20)])
def test_a_sequence_sees_only_itself(hd, base, Tq):
    C, D = ext(), H * hd
    new, cache, _ = _setup(hd, base, Tq, seed=5)
    out = C.attention_extend(new, cache.clone(), H, base)
    new2, cache2, _ = _setup(hd, base, Tq, seed=6)
    new2.view(B, Tq, 3 * D)[0] = new.view(B, Tq, 3 * D)[0]
    cache2[0] = cache[0]
    out2 = C.attention_extend(new2, cache2, H, base)
    assert bit_equal(out2[:Tq], out[:Tq]) and not bit_equal(out2[Tq:], out[Tq:])
