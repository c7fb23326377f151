"""``attention_decode_shared`` (decode attention for N rows per prompt over a shared prefix) against fp64.

Inputs are peaked probes on ``_attn_probe._sign_keys`` keys: row m's query is c (k_x + k_y) / 2 with x a
prefix key -- cycling through 0, 63, 64, P - 1 and the last key of each prefix split over the rows of a
group -- and y a private key, alternately the newest (``pos``, taken from qkv_new) and the oldest
(``P``, the first ``own`` row), so one lost, doubled or misplaced key, or one taken from another row's
``own``, is an O(1) error.  Everything the call must not read into a result is NaN going in: ``pre`` rows
at or past P, ``own`` rows at or past pos - P, every Q third of both and the margins up to Tpre / Town.
Tolerance: ``_attn_probe.OUT_TOL``; each case prints its violation (error / tolerance) before it asserts.
Cases (hd, P, N, own_len), pos = P + own_len: P against the 64-key tile, N against the 32-query fragment,
prefix key splits with the wave fold, a second own split, and the other head-dim instantiations.

On an MI355X the violations were 0.081 (hd 8) to 0.556 ((128, 300, 3, 2)); the list is in PERF.md 'Shared prefix'."""
import math

import pytest
import torch

import _attn_probe as P_
from _guard import bit_equal
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 2, 2
SPLIT = (64, 960, 4, 5)
CASES = [(64, 1, 2, 0), (64, 63, 2, 1), (64, 64, 2, 1), (64, 65, 2, 1), (64, 200, 1, 3), (64, 200, 31, 3),
         (64, 200, 33, 3), SPLIT, (64, 70, 2, 300), (8, 300, 3, 2), (80, 300, 3, 2), (128, 300, 3, 2)]


def _setup(hd, P, N, own_len, seed, room=None):
    """(qkv_new [R, 3D], pre [B, Tpre, 3D], own [R, Town, 3D], fp64 reference out [R, D]); ``room``: (Tpre, Town)."""
    C, D, R, no = ext(), H * hd, B * N, own_len + 1
    Tpre, Town = room or (P + 37, own_len + 6)
    g = torch.Generator().manual_seed(seed)
    k = P_._sign_keys((B, P + N * no, H), hd, g)  # one magnitude per (b, h, d): every q below is exact
    v = torch.randn(B, P + N * no, H, hd, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    kp, vp = k[:, :P], v[:, :P]
    ko, vo = k[:, P:].view(B, N, no, H, hd), v[:, P:].view(B, N, no, H, hd)
    tiles = -(-(-(-Tpre // 64)) // C.attention_decode_shared_splits(B, H, Tpre))  # ceil(ceil(Tpre / 64) / splits)
    ends = [min(e, P) - 1 for e in range(tiles * 64, P + tiles * 64, tiles * 64)]
    xs = list(dict.fromkeys(x for x in [0, 63, 64, P - 1] + ends if x < P))
    x = torch.tensor([xs[j % len(xs)] for j in range(N)])
    y = torch.tensor([own_len if j % 2 == 0 else 0 for j in range(N)])
    q = 0.5 * P_.default_c(hd) * (kp[:, x] + ko[:, torch.arange(N), y])  # [B, N, H, hd]
    q = q.to(torch.bfloat16).double()
    ka = torch.cat([kp[:, None].expand(B, N, P, H, hd), ko], dim=2)
    va = torch.cat([vp[:, None].expand(B, N, P, H, hd), vo], dim=2)
    p = (torch.einsum("bnhd,bnlhd->bnhl", q, ka) / math.sqrt(hd)).softmax(-1)
    ref = torch.einsum("bnhl,bnlhd->bnhd", p, va).reshape(R, D)
    bf = lambda t: t.to(DEV, torch.bfloat16)
    new = bf(torch.cat([q.reshape(R, D), ko[:, :, -1].reshape(R, D), vo[:, :, -1].reshape(R, D)], dim=1))
    pre = torch.full((B, Tpre, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    pre[:, :P, D:2 * D], pre[:, :P, 2 * D:] = bf(kp.reshape(B, P, D)), bf(vp.reshape(B, P, D))
    own = torch.full((R, Town, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    own[:, :own_len, D:2 * D] = bf(ko[:, :, :-1].reshape(R, own_len, D))
    own[:, :own_len, 2 * D:] = bf(vo[:, :, :-1].reshape(R, own_len, D))
    return new, pre, own, ref.to(DEV)


def _lens(P, own_len):
    return (torch.tensor([P + own_len], dtype=torch.int32, device=DEV),
            torch.tensor([P], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("hd,P,N,own_len", CASES)
def test_against_fp64(hd, P, N, own_len):
    C, D = ext(), H * hd
    new, pre, own, ref = _setup(hd, P, N, own_len, seed=hd + P + N + own_len)
    pre0, own0 = pre.clone(), own.clone()
    assert C.attention_decode_shared_splits(B, H, pre.size(1)) > 1 or (hd, P, N, own_len) != SPLIT
    out = C.attention_decode_shared(new, pre, own, H, N, *_lens(P, own_len))
    v = P_.violation(out, ref, **P_.OUT_TOL)
    print(f"PROBE shared hd={hd} P={P} N={N} own={own_len}: out {v:.3f}")
    assert torch.isfinite(out.float()).all() and v <= 1, v
    # the row's K / V thirds appended bit for bit; every other byte of own and all of pre keep their bits
    assert bit_equal(own[:, own_len, D:], new[:, D:])
    assert bit_equal(own[:, :own_len], own0[:, :own_len]) and bit_equal(own[:, own_len + 1:], own0[:, own_len + 1:])
    assert bit_equal(own[:, :, :D], own0[:, :, :D]) and bit_equal(pre, pre0)


def test_surplus_splits_are_neutral():
    """Caches far longer than the lengths in use, as a decode state's are: the grid is sized from them, and the
    prefix and own splits that hold no key at this (P, pos) must add nothing."""
    C, (hd, P, N, own_len) = ext(), (64, 65, 2, 1)
    new, pre, own, ref = _setup(hd, P, N, own_len, seed=3, room=(1024, 600))
    assert C.attention_decode_shared_splits(B, H, 1024) > 1
    out = C.attention_decode_shared(new, pre, own, H, N, *_lens(P, own_len))
    v = P_.violation(out, ref, **P_.OUT_TOL)
    print(f"PROBE shared long caches hd={hd} P={P} N={N} own={own_len}: out {v:.3f}")
    assert torch.isfinite(out.float()).all() and v <= 1, v


@pytest.mark.parametrize("hd,P,N,own_len", [(64, 65, 3, 1), SPLIT])
def test_a_row_sees_only_itself_and_its_prompt(hd, P, N, own_len):
    C = ext()
    run = lambda new, pre, own: C.attention_decode_shared(new, pre, own.clone(), H, N, *_lens(P, own_len))
    new, pre, own, _ = _setup(hd, P, N, own_len, seed=5)
    out = run(new, pre, own)
    new2, pre2, own2, _ = _setup(hd, P, N, own_len, seed=6)  # every other row and the other prompt replaced
    new2[0], own2[0], pre2[0] = new[0], own[0], pre[0]
    out2 = run(new2, pre2, own2)
    assert bit_equal(out2[0], out[0]) and not bit_equal(out2[1:N], out[1:N]) and not bit_equal(out2[N:], out[N:])
    swap = [N - 1] + list(range(1, N - 1)) + [0] + list(range(N, B * N))  # row 0 to the last slot of its group
    out3 = run(new[swap].contiguous(), pre, own[swap].contiguous())
    assert bit_equal(out3[N - 1], out[0]) and bit_equal(out3[N:], out[N:])


def test_graph_replays_equal_eager_at_two_positions():
    C, (hd, P, N, own_len) = ext(), (64, 200, 3, 3)
    new, pre, own, _ = _setup(hd, P, N, own_len, seed=9)
    part = torch.empty(C.attention_decode_shared_part_floats(B, N, H, hd, pre.size(1), own.size(1)), device=DEV)
    pos, plen = _lens(P, own_len)
    own_e, own_g = own.clone(), own.clone()
    eager = []
    for _ in range(2):
        eager.append(C.attention_decode_shared(new, pre, own_e, H, N, pos, plen, part).clone())
        pos += 1
    pos -= 2
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = C.attention_decode_shared(new, pre, own_g, H, N, pos, plen, part)
    for want in eager:
        graph.replay()
        assert bit_equal(out, want)
        pos += 1
    assert bit_equal(own_g, own_e)
