"""The grouped decode attention (``attention_decode(..., group=K)``: K rows of one sequence at K
consecutive positions of one cache row, csrc/kernels/attention.hip) against the plain kernel called K
times, r = 0 .. K - 1, with one position per row on a copy of the cache: the ``out`` rows and the final
cache must be bit-equal.  Bases below, across and past the 256-key split boundary, rows past the end
of the cache, different bases per sequence, and ``group = 1`` against the call without the argument."""
import pytest
import torch

from _guard import bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu

H, TMAX = 2, 300
SHAPES = [(1, 2), (1, 8), (2, 4), (4, 2)]


def _data(B, K, hd, seed):
    """(qkv_new [B * K, 3D], cache [B, Tmax, 3D]) random bf16; the cache is full of finite values, so
    a read of a stale row would change the result rather than hide."""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    qkv = torch.randn(B * K, 3 * D, generator=g).to(torch.bfloat16).cuda()
    cache = torch.randn(B, TMAX, 3 * D, generator=g).to(torch.bfloat16).cuda()
    return qkv, cache


def _workspace(C, rows, hd):
    part = torch.full((C.attention_decode_part_floats(rows, H, hd),), float("nan"), device="cuda")
    return part, torch.zeros(rows * H, dtype=torch.int32, device="cuda")


def _grouped(C, qkv, cache, bases, K, hd):
    """The grouped call on a copy of ``cache``; pos_dev holds base + r for row r (the kernel reads row
    0's).  Returns (out, cache after, counters after)."""
    B = cache.size(0)
    pos = torch.tensor([b0 + r for b0 in bases for r in range(K)], dtype=torch.int32).cuda()
    part, cnt = _workspace(C, B * K, hd)
    c = cache.clone()
    out = C.attention_decode(qkv, c, H, 0, pos, part, cnt, 1, K)
    torch.cuda.synchronize()
    return out, c, cnt


def _plain(C, qkv, cache, bases, K, hd):
    """The plain kernel K times on a copy of ``cache``: call r takes row r of every sequence at
    position base + r (pos_stride 1), rows past the cache's end left out.  Returns (out rows, a mask of
    the rows that ran, the cache after)."""
    B = cache.size(0)
    D = H * hd
    c = cache.clone()
    out = torch.zeros(B * K, D, dtype=torch.bfloat16, device="cuda")
    ran = torch.zeros(B * K, dtype=torch.bool)
    for r in range(K):
        live = [b for b in range(B) if bases[b] + r <= TMAX - 1]
        if len(live) != B:  # sequences out of room: run the others one by one at the same split rule
            assert B == 1 or not live, "the cases keep a batch's sequences together"
            continue
        rows = torch.tensor([b * K + r for b in range(B)]).cuda()
        pos = torch.tensor([bases[b] + r for b in range(B)], dtype=torch.int32).cuda()
        part, cnt = _workspace(C, B, hd)
        out[rows] = C.attention_decode(qkv[rows].contiguous(), c, H, 1, pos, part, cnt, 1)
        ran[rows.cpu()] = True
        assert not cnt.any()
    torch.cuda.synchronize()
    return out, ran, c


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("B,K", SHAPES, ids=[f"B{b}-K{k}" for b, k in SHAPES])
@pytest.mark.parametrize("base", [0, 5, 250, 255, 256, 292])
def test_grouped_equals_plain(hd, B, K, base):
    """One split (base + r <= 255), the 256-key boundary crossed inside a group (250, 255 with K = 8),
    and two splits (256, 292)."""
    C = ext()
    qkv, cache = _data(B, K, hd, seed=base + K)
    bases = [base] * B
    out, c, cnt = _grouped(C, qkv, cache, bases, K, hd)
    want, ran, wc = _plain(C, qkv, cache, bases, K, hd)
    assert ran.all() and bit_equal(out, want) and bit_equal(c, wc)
    assert not cnt.any()  # the kernel leaves its counters zero
    # the appended rows are the new K / V, the Q columns and every other row are untouched
    D = H * hd
    for b in range(B):
        assert bit_equal(c[b, base:base + K, D:], qkv.view(B, K, 3 * D)[b, :, D:])
        assert bit_equal(c[b, base:base + K, :D], cache[b, base:base + K, :D])
        assert bit_equal(c[b, :base], cache[b, :base]) and bit_equal(c[b, base + K:], cache[b, base + K:])


@pytest.mark.parametrize("hd", [32, 64])
def test_rows_past_the_cache_end(hd):
    """base = 297 with K = 8 at Tmax = 300: rows 0 .. 2 are the plain kernel's, rows 3 .. 7 write
    zeros, append nothing and leave the counters zero."""
    C = ext()
    K, base = 8, 297
    qkv, cache = _data(1, K, hd, seed=hd)
    out, c, cnt = _grouped(C, qkv, cache, [base], K, hd)
    want, ran, wc = _plain(C, qkv, cache, [base], K, hd)
    assert ran.tolist() == [True] * 3 + [False] * 5
    assert bit_equal(out[:3], want[:3]) and bit_equal(c, wc)
    assert (out[3:].view(torch.int16) == 0).all() and not cnt.any()


@pytest.mark.parametrize("hd", [32, 64])
def test_different_bases_per_sequence(hd):
    """B = 2, K = 4: one sequence in a single split, the other crossing into two."""
    C = ext()
    K, bases = 4, [7, 254]
    qkv, cache = _data(2, K, hd, seed=3)
    out, c, cnt = _grouped(C, qkv, cache, bases, K, hd)
    want, ran, wc = _plain(C, qkv, cache, bases, K, hd)
    assert ran.all() and bit_equal(out, want) and bit_equal(c, wc) and not cnt.any()


@pytest.mark.parametrize("pos_stride", [0, 1])
def test_group_one_is_the_plain_call(pos_stride):
    """``group = 1`` is bit-equal to the same call without the argument, out and cache."""
    C = ext()
    hd, B = 64, 2
    qkv, cache = _data(B, 1, hd, seed=11)
    pos = torch.tensor([260, 40][:B if pos_stride else 1], dtype=torch.int32).cuda()
    res = []
    for extra in ((), (1,)):
        part, cnt = _workspace(C, B, hd)
        c = cache.clone()
        res.append((C.attention_decode(qkv, c, H, 1, pos, part, cnt, pos_stride, *extra), c))
        assert not cnt.any()
    assert bit_equal(res[0][0], res[1][0]) and bit_equal(res[0][1], res[1][1])


def test_grouped_argument_checks():
    C = ext()
    qkv, cache = _data(1, 4, 32, seed=0)
    pos = torch.arange(4, dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError, match="group"):
        C.attention_decode(qkv, cache, H, 0, None, None, None, 0, 4)   # no pos_dev
    with pytest.raises(RuntimeError, match="group"):
        C.attention_decode(qkv, cache, H, 0, pos, None, None, 1, 9)    # more rows than the kernels take
    with pytest.raises(RuntimeError, match="shape"):
        C.attention_decode(qkv, cache, H, 0, pos, None, None, 1, 2)    # qkv_new has 4 rows, not 2


def test_grouped_guard_bands():
    """The grouped call with every operand between guard bands, a group across the split boundary."""
    C = ext()
    hd, B, K = 32, 2, 4
    qkv, cache = _data(B, K, hd, seed=5)
    pos = torch.tensor([254, 255, 256, 257, 3, 4, 5, 6], dtype=torch.int32).cuda()
    part, cnt = _workspace(C, B * K, hd)
    part.zero_()
    guarded(lambda qkv_new, pos_dev, cache, part, counters: C.attention_decode(qkv_new, cache, H, 0, pos_dev, part,
                                                                                counters, 1, K),
            {"qkv_new": qkv, "pos_dev": pos}, {"cache": cache, "part": part, "counters": cnt},
            name="attention_decode grouped", skip=("part",))
