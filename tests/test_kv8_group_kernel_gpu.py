"""The grouped int8-cache decode attention (``attention_decode_kv8(..., group=K)``: K rows of one sequence
at K consecutive positions of one int8 cache row, csrc/kernels/attention_kv8.hip), on the caches of
``test_kv8_kernel_gpu._Case`` and in the pattern of ``test_spec_attention_gpu``.  Per case:

* the appended (q, s) at base .. base + K - 1 are the numpy oracle's, no other cache byte or scale
  changes and ``qkv_new`` is unchanged;
* ``out`` and the final cache are bit-equal to K plain ``attention_decode_kv8`` calls at base + r on a copy;
* ``out`` is bit-equal to the bf16 ``attention_decode(group=K)`` on the snapped rows over the dequantized
  cache;
* the counters are zero.

Then a captured call replayed at three bases, the cancelling-values construction continued through the
group's own rows, tiny-scale and zero vectors in a group row, NaN isolation in time, guard bands and the
argument checks."""
import functools

import pytest
import torch

from _guard import bit_equal, guarded
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext
from test_kv8_kernel_gpu import _Case, _oracle_kv, _rand_rows, _same_scales

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, TMAX = 2, 300
SHAPES = [(1, 2), (1, 8), (2, 4), (4, 2)]


def _cancel(hist):
    """K[t] = K[t - 1] and V[t] = -V[t - 1] for odd t (``test_kv8_kernel_gpu``'s construction)."""
    D = hist.shape[-1] // 3
    n = hist.shape[1]
    hist[:, 1::2, D:2 * D] = hist[:, 0:n - 1:2, D:2 * D]
    hist[:, 1::2, 2 * D:] = -hist[:, 0:n - 1:2, 2 * D:]


@functools.lru_cache(maxsize=None)
def _case(B, heads, hd, Tmax=TMAX, seed=0, cancel=False):
    """The shared history: built once per shape and never written (every call below works on clones)."""
    return _Case(B, heads, hd, Tmax, seed=seed, edit=_cancel if cancel else None)


def _workspace(C, rows, heads, hd):
    part = torch.full((C.attention_decode_part_floats(rows, heads, hd),), float("nan"), device=DEV)
    return part, torch.zeros(rows * heads, dtype=torch.int32, device=DEV)


def _pos_rows(bases, K):
    return torch.tensor([b0 + r for b0 in bases for r in range(K)], dtype=torch.int32, device=DEV)


def _snapped(x, heads):
    """(oracle q [R, 2, H, hd], oracle s [R, 2, H], the rows with their K/V thirds replaced by s q)."""
    D = x.shape[-1] // 3
    oq, os_, od = _oracle_kv(x, heads)
    sn = x.clone()
    sn[:, D:] = od.reshape(x.shape[0], 2 * D)
    return oq, os_, sn


def _grouped(c, x, bases, K):
    """The grouped KV8 call on copies of the case's int8 cache: (out, kq, ks, counters)."""
    C = c.C
    kq, ks = c.kq.clone(), c.ks.clone()
    part, cnt = _workspace(C, c.B * K, c.H, c.hd)
    xd = x.to(DEV)
    out = C.attention_decode_kv8(xd, kq, ks, c.H, 0, _pos_rows(bases, K), part, cnt, 1, K)
    torch.cuda.synchronize()
    assert bit_equal(xd.cpu(), x), "qkv_new was modified"
    return out, kq, ks, cnt


def _plain(c, x, bases, K):
    """K plain KV8 calls on copies: call r takes row r of every sequence at base + r (pos_stride 1);
    rows past the end are left out.  (out rows, which rows ran, kq, ks)."""
    C, B = c.C, c.B
    kq, ks = c.kq.clone(), c.ks.clone()
    xd = x.to(DEV)
    out = torch.zeros(B * K, c.D, dtype=torch.bfloat16, device=DEV)
    ran = torch.zeros(B * K, dtype=torch.bool)
    for r in range(K):
        live = [b for b in range(B) if bases[b] + r <= c.Tmax - 1]
        if len(live) != B:
            assert B == 1 or not live, "the cases keep a batch's sequences together"
            continue
        rows = torch.tensor([b * K + r for b in range(B)], device=DEV)
        pos = torch.tensor([bases[b] + r for b in range(B)], dtype=torch.int32, device=DEV)
        part, cnt = _workspace(C, B, c.H, c.hd)
        out[rows] = C.attention_decode_kv8(xd[rows].contiguous(), kq, ks, c.H, 1, pos, part, cnt, 1)
        ran[rows.cpu()] = True
        assert not cnt.any()
    torch.cuda.synchronize()
    return out, ran, kq, ks


def _bf16_grouped(c, sn, bases, K):
    """The bf16 grouped kernel on the snapped rows over a copy of the dequantized cache."""
    part, cnt = _workspace(c.C, c.B * K, c.H, c.hd)
    return c.C.attention_decode(sn.to(DEV), c.cache.clone(), c.H, 0, _pos_rows(bases, K), part, cnt, 1, K)


def _check(c, bases, K, x=None, seed=1, label=""):
    """Every per-case property of the module docstring; returns the grouped output."""
    B, Tmax = c.B, c.Tmax
    if x is None:
        x = _rand_rows((B * K, 3 * c.D), 5000 + seed, c.H)
    oq, os_, sn = _snapped(x, c.H)
    out, kq, ks, cnt = _grouped(c, x, bases, K)
    want_q, want_s = c.kq.clone(), c.ks.clone()
    live = torch.zeros(B * K, dtype=torch.bool)
    for b in range(B):
        for r in range(K):
            if bases[b] + r <= Tmax - 1:
                live[b * K + r] = True
                want_q[b, :, :, bases[b] + r] = oq[b * K + r].to(DEV)
                want_s[b, :, :, bases[b] + r] = os_[b * K + r].to(DEV)
    assert torch.equal(kq, want_q), f"{label}: the int8 cache is not the old one plus the oracle's rows"
    assert _same_scales(ks, want_s), f"{label}: the scales are not the old ones plus the oracle's"
    assert not cnt.any(), f"{label}: counters not zero"
    pout, ran, pq, ps = _plain(c, x, bases, K)
    assert torch.equal(ran, live)
    diff = int((out.view(torch.int16) != pout.view(torch.int16)).sum())
    print(f"{label}: {diff} of {out.numel()} outputs differ from K plain KV8 calls")
    assert diff == 0, f"{label}: {diff} of {out.numel()} outputs differ from K plain attention_decode_kv8 calls"
    assert torch.equal(kq, pq) and _same_scales(ks, ps), f"{label}: final cache differs from K plain calls"
    assert (out[~live.to(DEV)].view(torch.int16) == 0).all(), f"{label}: a row past the end is not zero"
    bout = _bf16_grouped(c, sn, bases, K)
    diff = int((out.view(torch.int16) != bout.view(torch.int16)).sum())
    print(f"{label}: {diff} of {out.numel()} outputs differ from the bf16 grouped kernel")
    assert diff == 0, f"{label}: {diff} of {out.numel()} outputs differ from attention_decode(group={K})"
    return out


@pytest.mark.parametrize("hd", [64, 24, 128])
@pytest.mark.parametrize("B,K", SHAPES, ids=[f"B{b}-K{k}" for b, k in SHAPES])
@pytest.mark.parametrize("base", [0, 5, 250, 255, 256, 292])
def test_grouped_contract(hd, B, K, base):
    """One split (base + r <= 255), the 256-key boundary crossed inside a group, and two splits; hd = 128
    with K = 8 keeps all 256 snap threads busy."""
    _check(_case(B, H, hd), [base] * B, K, seed=base + K, label=f"hd {hd} B {B} K {K} base {base}")


@pytest.mark.parametrize("base", [126, 127, 128])
def test_many_pairs_split_at_128_keys(base):
    """B * H = 36 > 32: 128 keys per split, chosen from the number of sequences and not of rows."""
    _check(_case(3, 12, 8), [base] * 3, 2, seed=base, label=f"B*H 36 base {base}")


@pytest.mark.parametrize("hd", [64, 24])
def test_different_bases_per_sequence(hd):
    _check(_case(2, H, hd), [7, 254], 4, seed=3, label=f"bases 7/254 hd {hd}")


@pytest.mark.parametrize("hd", [64, 24, 128])
def test_rows_past_the_cache_end(hd):
    """base = 297 with K = 8 at Tmax = 300: rows 3 .. 7 append nothing, touch no counter and write zeros."""
    out = _check(_case(1, H, hd), [297], 8, seed=hd, label=f"past the end hd {hd}")
    assert (out[3:].view(torch.int16) == 0).all()


@pytest.mark.parametrize("pos_stride", [0, 1])
def test_group_one_is_the_plain_call(pos_stride):
    c = _case(2, H, 64)
    x = _rand_rows((c.B, 3 * c.D), 77, H).to(DEV)
    pos = torch.tensor([260, 40][:c.B if pos_stride else 1], dtype=torch.int32, device=DEV)
    res = []
    for extra in ((), (1,)):
        kq, ks = c.kq.clone(), c.ks.clone()
        part, cnt = _workspace(c.C, c.B, H, c.hd)
        res.append((c.C.attention_decode_kv8(x, kq, ks, H, 1, pos, part, cnt, pos_stride, *extra), kq, ks))
        assert not cnt.any()
    assert bit_equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and _same_scales(res[0][2], res[1][2])


def test_a_captured_grouped_call_replays_at_three_bases():
    c = _case(2, H, 64)
    C, K = c.C, 4
    x = _rand_rows((c.B * K, 3 * c.D), 78, H)
    oq, os_, sn = _snapped(x, H)
    xd = x.to(DEV)
    kq, ks = c.kq.clone(), c.ks.clone()
    part, cnt = _workspace(C, c.B * K, H, c.hd)
    # bases from the top down: a call rewrites rows base .. base + K - 1 of this test's copy, and the
    # reference below reads the shared history, so every later base must read below the rewritten rows
    pos = _pos_rows([296, 296], K)
    call = lambda: C.attention_decode_kv8(xd, kq, ks, H, 0, pos, part, cnt, 1, K)
    call()  # warm-up
    graph, out = gen._capture(call)
    for base in (296, 254, 40):
        pos.copy_(_pos_rows([base, base], K))
        graph.replay()
        ref = _bf16_grouped(c, sn, [base, base], K)
        assert bit_equal(out, ref), f"replay at base {base}"
        assert not cnt.any()
        for b in range(c.B):
            for r in range(K):
                assert torch.equal(kq[b, :, :, base + r].cpu(), oq[b * K + r])
                assert _same_scales(ks[b, :, :, base + r], os_[b * K + r])


@pytest.mark.parametrize("hd", [64, 24])
def test_cancelling_values_through_the_group(hd):
    """``test_kv8_kernel_gpu``'s cancelling construction -- K[t] = K[t - 1], V[t] = -V[t - 1] for odd t --
    continued through the group's own rows: what comes out is the rounding residue of the PV chains, so
    one differently rounded fp32 step between the grouped KV8 kernel, the plain one and the bf16 grouped
    one changes most outputs."""
    B, K = 2, 8
    c = _case(B, 4, hd, 600, 11, True)
    D = c.D
    for base in (248, 591, 300, 31):
        x = _rand_rows((B * K, 3 * D), 6000 + base, c.H)
        for b in range(B):
            for r in range(K):
                if (base + r) % 2:
                    src = c.cache[b, base - 1].cpu() if r == 0 else x[b * K + r - 1]
                    x[b * K + r, D:2 * D] = src[D:2 * D]
                    x[b * K + r, 2 * D:] = -src[2 * D:]
        _check(c, [base] * B, K, x=x, label=f"cancelling hd {hd} base {base}")


def test_tiny_scale_and_zero_vectors_in_a_group_row():
    B, K, hd = 2, 4, 64
    c = _case(B, H, hd)
    D = c.D
    x = _rand_rows((B * K, 3 * D), 79, H)
    r = x[1]                                        # row 1 of sequence 0
    r[D] = 2.0 ** -120                              # K of head 0: a = 2^-120
    r[D + 1] = 2.0 ** -127
    r[D + 2:D + hd] = 0
    r[2 * D + hd:2 * D + 2 * hd] = 0                # V of head 1: a = 2^-120
    r[2 * D + hd + 5] = -2.0 ** -120
    x[K + 2, D:D + hd] = 0                          # row 2 of sequence 1: a zero K and a zero V vector
    x[K + 2, 2 * D:2 * D + hd] = 0
    for base in (8, 253, 296):
        _check(c, [base] * B, K, x=x, label=f"tiny base {base}")


def test_a_nan_key_stays_in_its_rows_and_its_head():
    """A NaN in the K of group row 2 of (sequence 1, head 1): rows 2 .. K - 1 of that (sequence, head) are
    NaN; rows 0 and 1 of it and every other (sequence, head) are bit-equal to the clean run."""
    B, K, hd, base = 2, 4, 24, 150
    c = _case(B, H, hd)
    x = _rand_rows((B * K, 3 * c.D), 80, H)
    bad = x.clone()
    bad[K + 2, c.D + hd + 3] = float("nan")
    want = _grouped(c, x, [base] * B, K)[0].view(B, K, H, hd)
    got, _, ks, _ = _grouped(c, bad, [base] * B, K)
    got = got.view(B, K, H, hd)
    assert bool(got[1, 2:, 1].isnan().all())
    assert bool(ks[1, 0, 1, base + 2].isnan()) and int(ks.isnan().sum()) == 1
    keep = torch.ones(B, K, H, dtype=torch.bool, device=DEV)
    keep[1, 2:, 1] = False
    assert not got[keep].isnan().any() and bit_equal(got[keep], want[keep])


def test_grouped_guard_bands():
    """Every operand between guard bands, one group across the split boundary."""
    B, K, hd = 2, 4, 24
    c = _case(B, H, hd)
    x = _rand_rows((B * K, 3 * c.D), 81, H).to(DEV)
    pos = torch.tensor([254, 255, 256, 257, 3, 4, 5, 6], dtype=torch.int32, device=DEV)
    part, cnt = _workspace(c.C, B * K, H, hd)
    part.zero_()
    fn = lambda qkv_new, pos_dev, kq, ks, part, counters: c.C.attention_decode_kv8(qkv_new, kq, ks, H, 0, pos_dev,
                                                                                  part, counters, 1, K)
    guarded(fn, {"qkv_new": x, "pos_dev": pos}, {"kq": c.kq.clone(), "ks": c.ks.clone(), "part": part, "counters": cnt},
            name="attention_decode_kv8 grouped", skip=("part",))


def test_grouped_argument_checks():
    C = ext()
    hd, K = 32, 4
    D = H * hd
    x = torch.zeros(K, 3 * D, dtype=torch.bfloat16, device=DEV)
    kq = torch.zeros(1, 2, H, TMAX, hd, dtype=torch.int8, device=DEV)
    ks = torch.zeros(1, 2, H, TMAX, dtype=torch.float32, device=DEV)
    pos = torch.arange(K, dtype=torch.int32, device=DEV)
    C.attention_decode_kv8(x, kq, ks, H, 0, pos, None, None, 1, K)  # the valid call
    with pytest.raises(RuntimeError, match="group"):
        C.attention_decode_kv8(x, kq, ks, H, 0, None, None, None, 0, K)   # no pos_dev
    with pytest.raises(RuntimeError, match="group"):
        C.attention_decode_kv8(x, kq, ks, H, 0, pos, None, None, 1, 9)    # more rows than the kernels take
    with pytest.raises(RuntimeError):
        C.attention_decode_kv8(x, kq, ks, H, 0, pos, None, None, 1, 2)    # qkv_new has 4 rows, not 2
    with pytest.raises(RuntimeError):
        C.attention_decode_kv8(x[:3], kq, ks, H, 0, pos, None, None, 1, 2)  # rows not a multiple of the group
