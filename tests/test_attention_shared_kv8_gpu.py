"""``attention_decode_shared_kv8`` against the numpy oracle of the KV8 rule and ``attention_decode_shared``:
(a) it appends the oracle's (q, s) of the step's K/V at own key pos - P and changes no other cache byte or scale
bit; (b) ``out`` is bit-equal to ``attention_decode_shared`` for qkv_new with snapped K/V over bf16 ``pre`` /
``own`` holding the dequantized rows; (c) ``qkv_new`` is not modified.  What the call must not read into a result
is stale going in (random bytes, NaN scales, NaN twin rows).  The fp64 probes are snapped first (PERF.md)."""
from types import SimpleNamespace

import pytest
import torch

import _attn_probe as P_
import _kv8_oracle as O
from _guard import bit_equal
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV, B, H = "cuda", 2, 2
SPLIT = (64, 960, 4, 5)
CASES = [(64, 1, 2, 0), (64, 63, 2, 1), (64, 64, 2, 1), (64, 65, 2, 1), (64, 200, 31, 3), (64, 200, 33, 3), SPLIT,
         (64, 70, 2, 300), (8, 300, 3, 2), (24, 300, 3, 2), (80, 300, 3, 2), (128, 300, 3, 2)]


def _rand_rows(shape, g):  # float32 values of bf16 rows [..., H * hd], vector magnitudes 2^-8 .. 2^8
    mag = torch.randint(-8, 9, (*shape[:-1], H), generator=g).float().exp2().repeat_interleave(shape[-1] // H, dim=-1)
    return (torch.randn(*shape, generator=g) * mag).to(torch.bfloat16).float()


def _case(hd, P, N, own_len, seed, probe=False, edit=None):
    """Both forms of one call's inputs.  ``probe``: row j's query is c (k_x + k_y) / 2, x a prefix key cycling
    over 0, 63, 64, P - 1, y its newest or oldest own key, and an fp64 reference on the snapped K/V."""
    D, R, no, L = H * hd, B * N, own_len + 1, P + N * (own_len + 1)
    Tpre, Town = P + 37, own_len + 6
    g = torch.Generator().manual_seed(seed)
    if probe:
        k = P_._sign_keys((B, L, H), hd, g).float()
        v = torch.randn(B, L, H, hd, generator=g).to(torch.bfloat16).float()
        xs = list(dict.fromkeys(x for x in (0, 63, 64, P - 1) if x < P))
        x = torch.tensor([xs[j % len(xs)] for j in range(N)])
        y = torch.tensor([own_len if j % 2 == 0 else 0 for j in range(N)])
        ko = k[:, P:].view(B, N, no, H, hd)
        q = (0.5 * P_.default_c(hd) * (k[:, x] + ko[:, torch.arange(N), y])).to(torch.bfloat16).float()
    else:
        k, v = (_rand_rows((B, L, D), g).view(B, L, H, hd) for _ in range(2))
        q = _rand_rows((B, N, D), g).view(B, N, H, hd)
    edit and edit(k, v)
    kv = torch.stack([k, v], dim=2)  # [B, L, 2, H, hd]
    oq, os_, od = (torch.from_numpy(a) for a in O.snap(kv.numpy()))
    planes = lambda t, n: t.reshape(n, -1, *t.shape[2:]).movedim(1, 3)  # [n, keys, 2, H, ..] -> [n, 2, H, keys, ..]
    rows = lambda t, n: t.reshape(n, -1, 2 * D).to(torch.bfloat16)      # [n, keys, 2, H, hd] -> [n, keys, 2D]
    c = SimpleNamespace(N=N, D=D, own_len=own_len)
    c.pre_q = torch.randint(-128, 128, (B, 2, H, Tpre, hd), generator=g, dtype=torch.int8)
    c.own_q = torch.randint(-128, 128, (R, 2, H, Town, hd), generator=g, dtype=torch.int8)
    c.pre_s, c.own_s = torch.full((B, 2, H, Tpre), float("nan")), torch.full((R, 2, H, Town), float("nan"))
    c.pre, c.own = (torch.full((n, t, 3 * D), float("nan"), dtype=torch.bfloat16) for n, t in ((B, Tpre), (R, Town)))
    c.pre_q[:, :, :, :P], c.pre_s[:, :, :, :P] = planes(oq[:, :P], B), planes(os_[:, :P], B)
    c.pre[:, :P, D:] = rows(od[:, :P], B)
    own = lambda t: t[:, P:].reshape(R, no, *t.shape[2:])  # the rows' own keys and, last, the step's
    c.own_q[:, :, :, :own_len], c.own_s[:, :, :, :own_len] = planes(own(oq)[:, :-1], R), planes(own(os_)[:, :-1], R)
    c.own[:, :own_len, D:] = rows(own(od)[:, :-1], R)
    qb = q.reshape(R, D).to(torch.bfloat16)
    c.new = torch.cat([qb, rows(own(kv)[:, -1:], R)[:, 0]], dim=1)
    c.snapped = torch.cat([qb, rows(own(od)[:, -1:], R)[:, 0]], dim=1)
    c.want_q, c.want_s = own(oq)[:, -1], own(os_)[:, -1]  # [R, 2, H, hd], [R, 2, H]
    if probe:
        kd, vd = od[:, :, 0].double(), od[:, :, 1].double()
        ka, va = (torch.cat([t[:, None, :P].expand(B, N, P, H, hd), t[:, P:].view(B, N, no, H, hd)], dim=2)
                  for t in (kd, vd))
        p = (torch.einsum("bnhd,bnlhd->bnhl", q.double(), ka) / hd ** 0.5).softmax(-1)
        c.ref = torch.einsum("bnhl,bnlhd->bnhd", p, va).reshape(R, D).to(DEV)
    for name in ("pre_q", "pre_s", "own_q", "own_s", "pre", "own", "new", "snapped"):
        setattr(c, name, getattr(c, name).contiguous().to(DEV))
    c.lens = lambda P=P, pos=P + own_len: tuple(torch.tensor([t], dtype=torch.int32, device=DEV) for t in (pos, P))
    return c


def _both(c):  # (KV8 out, bf16 out on the twins, own_q, own_s after the call), on copies of the own caches
    C, own_q, own_s, lens = ext(), c.own_q.clone(), c.own_s.clone(), c.lens()
    out = C.attention_decode_shared_kv8(c.new, c.pre_q, c.pre_s, own_q, own_s, H, c.N, *lens)
    return out, C.attention_decode_shared(c.snapped, c.pre, c.own.clone(), H, c.N, *lens), own_q, own_s


_bits = lambda t: t.view(torch.int32)  # scale words: NaN patterns compare as integers


@pytest.mark.parametrize("hd,P,N,own_len", CASES)
def test_appends_the_oracle_and_equals_the_bf16_kernel(hd, P, N, own_len):
    c = _case(hd, P, N, own_len, seed=hd + P + N + own_len)
    assert ext().attention_decode_shared_splits(B, H, c.pre.size(1)) > 1 or (hd, P, N, own_len) != SPLIT
    new0, pre_q0, pre_s0 = c.new.clone(), c.pre_q.clone(), c.pre_s.clone()
    out, ref, own_q, own_s = _both(c)
    want_q, want_s = c.own_q.clone(), c.own_s.clone()
    want_q[:, :, :, own_len], want_s[:, :, :, own_len] = c.want_q.to(DEV), c.want_s.to(DEV)
    assert torch.equal(own_q, want_q) and torch.equal(_bits(own_s), _bits(want_s)), "(a) the append"
    assert torch.equal(c.pre_q, pre_q0) and torch.equal(_bits(c.pre_s), _bits(pre_s0)), "(a) the prompt's cache"
    assert torch.isfinite(out.float()).all()
    assert bit_equal(out, ref), f"(b) {int((out.view(torch.int16) != ref.view(torch.int16)).sum())} outputs differ"
    assert bit_equal(c.new, new0), "(c) qkv_new was modified"


@pytest.mark.parametrize("hd,P,N,own_len", [(64, 65, 2, 1), SPLIT, (8, 300, 3, 2)])
def test_against_fp64_on_snapped_probes(hd, P, N, own_len):
    c = _case(hd, P, N, own_len, seed=hd + P, probe=True)
    out, ref, _, _ = _both(c)
    v = P_.violation(out, c.ref, **P_.OUT_TOL)
    print(f"PROBE shared kv8 hd={hd} P={P} N={N} own={own_len}: out {v:.3f}")
    assert bit_equal(out, ref) and v <= 1, v


def test_a_nan_prompt_key_reaches_its_prompt_and_head_only():
    hd, P, N, own_len = 64, 200, 3, 2
    clean, _, _, _ = _both(_case(hd, P, N, own_len, seed=4))
    out, ref, _, _ = _both(_case(hd, P, N, own_len, seed=4, edit=lambda k, v: k[0, 70, 0, 5:6].fill_(float("nan"))))
    hit = torch.zeros_like(out, dtype=torch.bool)
    hit[:N, :hd] = True  # prompt 0's rows, head 0
    assert torch.equal(out.isnan(), hit) and torch.equal(ref.isnan(), hit)
    assert bit_equal(out[~hit], clean[~hit])


def test_graph_replays_equal_eager_at_two_lengths():
    C, N, c = ext(), 3, _case(64, 200, 3, 3, seed=9)
    part = torch.empty(C.attention_decode_shared_part_floats(B, N, H, 64, c.pre.size(1), c.own.size(1)), device=DEV)
    pos, plen = c.lens()
    steps = [(200, 203), (150, 154)]  # (P, pos): the second reads the own key the first appended
    call = lambda oq, os_: C.attention_decode_shared_kv8(c.new, c.pre_q, c.pre_s, oq, os_, H, N, pos, plen, part)
    eager_state, graph_state = ((c.own_q.clone(), c.own_s.clone()) for _ in range(2))
    eager = [(plen.fill_(P), pos.fill_(at), call(*eager_state).clone())[2] for P, at in steps]
    plen.fill_(steps[0][0]), pos.fill_(steps[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(*graph_state)
    for (P, at), want in zip(steps, eager):
        plen.fill_(P), pos.fill_(at)
        graph.replay()
        assert bit_equal(out, want)
    assert torch.equal(graph_state[0], eager_state[0]) and torch.equal(_bits(graph_state[1]), _bits(eager_state[1]))
