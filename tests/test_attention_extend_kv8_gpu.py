"""``attention_extend_kv8``: (a) it appends the numpy oracle's (q, s) of the chunk's K/V at base .. base + Tq - 1 and
changes no other cache byte or scale bit; (b) ``out`` is bit-equal to ``attention_extend`` for qkv_new with snapped K/V
over a bf16 cache of the dequantized rows; (c) ``qkv_new`` keeps its bits.  Stale going in: bytes, scales, twin rows."""
from types import SimpleNamespace

import pytest
import torch

import _attn_probe as P_
import _kv8_oracle as O
from _guard import bit_equal
from mingpt_distributed_amd.ops._ext import ext
from test_attention_shared_kv8_gpu import B, DEV, H, _bits, _rand_rows  # B = H = 2; rows of magnitudes 2^-8 .. 2^8

pytestmark = pytest.mark.gpu
SPLIT = [(64, 700, 20), (64, 960, 64)]  # S > 1: partial states and the combine launch
CASES = [(64, 0, 200), (64, 1, 1), (64, 63, 1), (64, 64, 33), (64, 65, 31), (64, 200, 130)] + SPLIT + [
    (128, 300, 40), (80, 300, 40), (24, 300, 40), (8, 300, 40)]


def _case(hd, base, Tq, seed, probe=False, edit=None):
    """Both forms of one call's inputs.  ``probe``: ``_attn_probe.probe_qkv`` rows, an fp64 reference on snapped K/V."""
    T, D, Tmax = base + Tq, H * hd, base + Tq + 37
    g = torch.Generator().manual_seed(seed)
    q, k, v = (P_.probe_qkv(B, T, H, hd, seed)[0].float().view(B, T, 3, H, hd).unbind(2) if probe
               else [_rand_rows((B, T, D), g).view(B, T, H, hd) for _ in range(3)])
    edit and edit(k, v)
    kv = torch.stack([k, v], dim=2)  # [B, T, 2, H, hd]
    oq, os_, od = (torch.from_numpy(a) for a in O.snap(kv.numpy()))
    planes = lambda t: t.movedim(1, 3)                           # [B, keys, 2, H, ..] -> [B, 2, H, keys, ..]
    rows = lambda t: t.reshape(B, -1, 2 * D).to(torch.bfloat16)  # [B, keys, 2, H, hd] -> [B, keys, 2D]
    c = SimpleNamespace(kq=torch.randint(-128, 128, (B, 2, H, Tmax, hd), generator=g, dtype=torch.int8),
                        ks=torch.full((B, 2, H, Tmax), float("nan")),
                        cache=torch.full((B, Tmax, 3 * D), float("nan"), dtype=torch.bfloat16))
    c.kq[:, :, :, :base], c.ks[:, :, :, :base] = planes(oq[:, :base]), planes(os_[:, :base])
    c.cache[:, :base, D:] = rows(od[:, :base])
    qb = q[:, base:].reshape(B, Tq, D).to(torch.bfloat16)
    c.new, c.snapped = (torch.cat([qb, rows(t[:, base:])], dim=2).view(B * Tq, 3 * D) for t in (kv, od))
    c.want_q, c.want_s = c.kq.clone(), c.ks.clone()
    c.want_q[:, :, :, base:T], c.want_s[:, :, :, base:T] = planes(oq[:, base:]), planes(os_[:, base:])
    if probe:
        full = torch.cat([q.reshape(B, T, D), od.reshape(B, T, 2 * D)], dim=2).view(B * T, 3 * D).to(DEV)
        c.ref = P_.ref64(full, torch.zeros(B * T, D, device=DEV), B, T, H)[0].view(B, T, D)[:, base:].reshape(B * Tq, D)
    for name in ("kq", "ks", "cache", "new", "snapped", "want_q", "want_s"):
        setattr(c, name, getattr(c, name).contiguous().to(DEV))
    return c


def _both(c, base):  # (KV8 out, bf16 out on the twins, kq, ks after the call), on copies of the caches
    C, kq, ks = ext(), c.kq.clone(), c.ks.clone()
    out = C.attention_extend_kv8(c.new, kq, ks, H, base)
    return out, C.attention_extend(c.snapped, c.cache.clone(), H, base), kq, ks


@pytest.mark.parametrize("hd,base,Tq,probe", [(*c, False) for c in CASES] + [  # ... and snapped probes against fp64
    (64, 65, 31, True), (64, 700, 20, True), (8, 300, 40, True)])
def test_appends_the_oracle_and_equals_the_bf16_kernel(hd, base, Tq, probe):
    c = _case(hd, base, Tq, seed=hd + base + Tq, probe=probe)
    assert ext().attention_extend_splits(B, Tq, H, base) > 1 or (hd, base, Tq) not in SPLIT
    new0 = c.new.clone()
    out, ref, kq, ks = _both(c, base)
    assert torch.equal(kq, c.want_q) and torch.equal(_bits(ks), _bits(c.want_s)), "(a) the append"
    assert bit_equal(out, ref), f"(b) {int((out.view(torch.int16) != ref.view(torch.int16)).sum())} outputs differ"
    assert torch.isfinite(out.float()).all() and bit_equal(c.new, new0), "(b) out is not finite, or (c) qkv_new changed"
    if probe:
        v = P_.violation(out, c.ref, **P_.OUT_TOL)
        print(f"PROBE extend kv8 hd={hd} base={base} Tq={Tq}: out {v:.3f}")
        assert v <= 1, v


def test_a_nan_cached_key_reaches_its_sequence_and_head_only():
    hd, base, Tq = 64, 200, 33
    clean, _, _, _ = _both(_case(hd, base, Tq, seed=4), base)
    out, ref, _, _ = _both(_case(hd, base, Tq, seed=4, edit=lambda k, v: k[0, 70, 0, 5:6].fill_(float("nan"))), base)
    hit = torch.zeros_like(out, dtype=torch.bool)
    hit[:Tq, :hd] = True  # sequence 0's rows, head 0
    assert torch.equal(out.isnan(), hit) and torch.equal(ref.isnan(), hit)
    assert bit_equal(out[~hit], clean[~hit])
