"""The beam kernels of the int8 KV cache (csrc/kernels/attention_kv8.hip):

* ``beam_reorder_kv8`` against ``index_select`` on random bytes and random scale bit patterns (NaN patterns
  included), compared as integers: positions t < min(pos, Tmax) of every (K | V, head) of beam r become
  those of beam parent[r] of the same prompt; later positions and identity prompts are bit-unchanged;
  ``ctl[0]`` advances; layer-by-layer calls equal the one call; an out-of-range parent is the identity.
  The shapes include blocks that are only 8-byte aligned (hd % 16 == 8 with odd Tmax) and scale rows that
  are only 4-byte aligned (odd Tmax).
* ``kv8_store(rep=W)``: every beam row of a prompt holds the numpy oracle's (q, s)."""
import pytest
import torch

from _guard import bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext
from test_kv8_kernel_gpu import _oracle_kv, _rand_rows, _same_scales

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
SHAPES = [(2, 64, 64), (3, 24, 37), (1, 8, 37), (2, 128, 33)]  # (H, hd, Tmax)


def _caches(L, R, H, hd, Tmax, seed, finite=False):
    g = torch.Generator().manual_seed(seed)
    kq = torch.randint(-128, 128, (L, R, 2, H, Tmax, hd), generator=g, dtype=torch.int8)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (L, R, 2, H, Tmax), generator=g, dtype=torch.int64).to(torch.int32)
    if finite:
        bits = (bits & 0x3FFFFFFF)  # exponent below 128: finite
    else:
        bits[0, 0, 0, 0, 0] = 0x7FC00001  # NaN payloads move as bits
        bits[-1, -1, 1, -1, -1] = -1
    return kq.to(DEV), bits.view(torch.float32).to(DEV)


def _parents(kind, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":  # prompt 1 keeps the identity
        p = torch.randint(0, W, (B, W), generator=g)
        p[1] = torch.arange(W)
    elif kind == "identity":
        p = torch.arange(W).repeat(B, 1)
    else:  # all from one beam
        p = torch.full((B, W), W - 1)
        p[1] = torch.arange(W)
    return p.to(torch.int32)


def _want(kq, ks, parent, W, n):
    """index_select by parent on positions t < n, as integers."""
    L, R = kq.shape[:2]
    rows = (torch.arange(R // W).view(-1, 1) * W + parent.long()).view(-1).to(kq.device)
    wq, ws = kq.clone(), ks.view(torch.int32).clone()
    wq[..., :n, :] = kq.index_select(1, rows)[..., :n, :]
    ws[..., :n] = ks.view(torch.int32).index_select(1, rows)[..., :n]
    return wq, ws


@pytest.mark.parametrize("H,hd,Tmax", SHAPES)
@pytest.mark.parametrize("W", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("L", [1, 3])
def test_reorder_matches_index_select(L, W, H, hd, Tmax):
    C = ext()
    R = B * W
    kq0, ks0 = _caches(L, R, H, hd, Tmax, seed=W * 100 + hd + L)
    for kind in ("random", "identity", "one"):
        parent = _parents(kind, W, seed=W + hd)
        for n in (1, 2, 31, Tmax, Tmax + 5):
            kq, ks = kq0.clone(), ks0.clone()
            pos = torch.tensor([n], dtype=torch.int32, device=DEV)
            ctl = torch.tensor([7, -1, 0, 0], dtype=torch.int32, device=DEV)
            C.beam_reorder_kv8(kq, ks, W, parent.view(-1).to(DEV), pos, ctl)
            wq, ws = _want(kq0, ks0, parent, W, min(n, Tmax))
            label = f"L {L} W {W} H {H} hd {hd} Tmax {Tmax} {kind} n {n}"
            assert torch.equal(kq, wq), f"{label}: int8 bytes"
            assert torch.equal(ks.view(torch.int32), ws), f"{label}: scale words"
            assert ctl.tolist() == [8, -1, 0, 0] and int(pos) == n, f"{label}: ctl / pos"
            # positions past n and the identity prompt, bit for bit
            m = min(n, Tmax)
            assert torch.equal(kq[..., m:, :], kq0[..., m:, :])
            assert torch.equal(ks.view(torch.int32)[..., m:], ks0.view(torch.int32)[..., m:])
            assert torch.equal(kq[:, W:2 * W], kq0[:, W:2 * W])
            assert torch.equal(ks.view(torch.int32)[:, W:2 * W], ks0.view(torch.int32)[:, W:2 * W])


@pytest.mark.parametrize("H,hd,Tmax", SHAPES)
def test_layer_by_layer_equals_one_call(H, hd, Tmax):
    C, L, W = ext(), 3, 3
    kq0, ks0 = _caches(L, B * W, H, hd, Tmax, seed=5)
    parent = _parents("random", W, seed=9).view(-1).to(DEV)
    pos = torch.tensor([Tmax - 2], dtype=torch.int32, device=DEV)
    one_q, one_s = kq0.clone(), ks0.clone()
    ctl = torch.zeros(4, dtype=torch.int32, device=DEV)
    C.beam_reorder_kv8(one_q, one_s, W, parent, pos, ctl)
    lay_q, lay_s = kq0.clone(), ks0.clone()
    ctl2 = torch.zeros(4, dtype=torch.int32, device=DEV)
    for i in range(L):
        C.beam_reorder_kv8(lay_q[i:i + 1], lay_s[i:i + 1], W, parent, pos, ctl2 if i == 0 else None)
    assert torch.equal(one_q, lay_q) and torch.equal(one_s.view(torch.int32), lay_s.view(torch.int32))
    assert not torch.equal(one_q, kq0)
    assert int(ctl[0]) == 1 and int(ctl2[0]) == 1


def test_an_out_of_range_parent_is_the_identity():
    C, L, W, (H, hd, Tmax) = ext(), 1, 3, SHAPES[1]
    kq0, ks0 = _caches(L, B * W, H, hd, Tmax, seed=6)
    parent = torch.tensor([[2, 0, 1], [0, 7, -1], [1, 1, 3]], dtype=torch.int32)
    fixed = torch.tensor([[2, 0, 1], [0, 1, 2], [1, 1, 2]], dtype=torch.int32)
    kq, ks = kq0.clone(), ks0.clone()
    pos = torch.tensor([20], dtype=torch.int32, device=DEV)
    C.beam_reorder_kv8(kq, ks, W, parent.view(-1).to(DEV), pos)
    wq, ws = _want(kq0, ks0, fixed, W, 20)
    assert torch.equal(kq, wq) and torch.equal(ks.view(torch.int32), ws)


@pytest.mark.parametrize("H,hd,Tmax", [SHAPES[1], SHAPES[3]])
def test_reorder_guard_bands(H, hd, Tmax):
    C, L, W = ext(), 2, 3
    kq, ks = _caches(L, B * W, H, hd, Tmax, seed=7, finite=True)
    parent = _parents("random", W, seed=3).view(-1).to(DEV)
    pos = torch.tensor([Tmax], dtype=torch.int32, device=DEV)
    ctl = torch.zeros(4, dtype=torch.int32, device=DEV)
    guarded(lambda parent, pos, kq, ks, ctl: C.beam_reorder_kv8(kq, ks, W, parent, pos, ctl),
            {"parent": parent, "pos": pos}, {"kq": kq, "ks": ks, "ctl": ctl}, name="beam_reorder_kv8")


def test_reorder_argument_checks():
    C, L, W, H, hd, Tmax = ext(), 2, 2, 2, 16, 8
    R = B * W
    kq, ks = _caches(L, R, H, hd, Tmax, seed=8)
    parent = torch.zeros(R, dtype=torch.int32, device=DEV)
    pos = torch.ones(1, dtype=torch.int32, device=DEV)
    C.beam_reorder_kv8(kq, ks, W, parent, pos)  # the valid call
    big = _caches(1, 9, H, hd, Tmax, seed=8)
    bad = [
        (kq.to(torch.int16), ks, W, parent, pos), (kq.view(torch.uint8), ks, W, parent, pos),   # dtype
        (kq, ks.double(), W, parent, pos), (kq, ks, W, parent.long(), pos),
        (kq, ks[:, :, :, :, :-1].contiguous(), W, parent, pos), (kq, ks[:1], W, parent, pos),   # kq / ks mismatch
        (kq, ks[:, :-1], W, parent, pos), (kq[:, 0], ks[:, 0], W, parent, pos),
        (kq, ks, 4, parent, pos),                                                               # W does not divide R
        (big[0], big[1], 9, torch.zeros(9, dtype=torch.int32, device=DEV), pos),                # W > 8
        (kq, ks, 0, parent, pos), (kq, ks, W, parent[:-1], pos), (kq.cpu(), ks.cpu(), W, parent, pos),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            C.beam_reorder_kv8(*args)


# ------------------------------------------------------------------ kv8_store(rep=)
@pytest.mark.parametrize("Bp,T,H,hd,rep", [(2, 5, 2, 64, 3), (1, 3, 3, 24, 8), (2, 1, 1, 8, 2)])
def test_kv8_store_rep(Bp, T, H, hd, rep):
    C, D, Tmax = ext(), H * hd, T + 3
    x = _rand_rows((Bp, T, 3 * D), 17, H)
    oq, os_, od = _oracle_kv(x, H)  # [Bp, T, 2, H, hd], [Bp, T, 2, H]
    qkv = x.to(DEV)
    kq = torch.full((Bp * rep, 2, H, Tmax, hd), 0x5A, dtype=torch.int8, device=DEV)
    ks = torch.full((Bp * rep, 2, H, Tmax), -3.0, dtype=torch.float32, device=DEV)
    C.kv8_store(qkv, H, kq, ks, rep)
    wq = oq.permute(0, 2, 3, 1, 4).repeat_interleave(rep, dim=0)
    ws = os_.permute(0, 2, 3, 1).repeat_interleave(rep, dim=0)
    assert torch.equal(kq[:, :, :, :T].cpu(), wq) and _same_scales(ks[:, :, :, :T], ws)
    assert bool((kq[:, :, :, T:] == 0x5A).all()) and bool((ks[:, :, :, T:] == -3.0).all())
    assert bit_equal(qkv[..., D:].cpu(), od.reshape(Bp, T, 2 * D)) and bit_equal(qkv[..., :D].cpu(), x[..., :D])
    for wrong in (Bp * rep + 1, Bp):  # a row count other than Bp * rep
        if wrong == Bp * rep:
            continue
        with pytest.raises(RuntimeError):
            C.kv8_store(x.to(DEV), H, kq.new_zeros(wrong, 2, H, Tmax, hd), ks.new_zeros(wrong, 2, H, Tmax), rep)


def test_kv8_store_rep_one_is_the_plain_call():
    C, Bp, T, H, hd = ext(), 2, 4, 2, 24
    D = H * hd
    x = _rand_rows((Bp, T, 3 * D), 18, H)
    res = []
    for extra in ((), (1,)):
        qkv = x.to(DEV)
        kq = torch.full((Bp, 2, H, T + 2, hd), 0x33, dtype=torch.int8, device=DEV)
        ks = torch.full((Bp, 2, H, T + 2), -5.0, dtype=torch.float32, device=DEV)
        C.kv8_store(qkv, H, kq, ks, *extra)
        res.append((qkv, kq, ks))
    assert all(bit_equal(a, b) for a, b in zip(*res))
    with pytest.raises(RuntimeError):
        C.kv8_store(x.to(DEV), H, None, None, 2)  # rep goes with a cache
