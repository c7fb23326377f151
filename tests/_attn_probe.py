"""Peaked two-target probes for the attention kernels: inputs on which a single key matters.

With ``randn`` inputs the causal softmax is diffuse: key ``j`` carries about ``1 / (i + 1)`` of row
``i``, less than the tolerances of the attention tests at any length where tile tails and key-block
hand-offs exist, so a kernel that drops, doubles or misplaces one key passes them.  ``probe_qkv``
builds inputs on which every row puts about half of its softmax mass on each of two chosen keys --
its own (the diagonal) and one picked to sit at a place where the kernels change tile, block or
code path -- so such a fault moves the result by O(1).  Two targets, not one: a key read twice
still normalises to ~1 in a one-hot row but gives 2/3 against 1/3 here, and dS = P * (dP - delta)
is non-zero, so dQ and dK are exercised as well as dV.

A helper module, not a conftest; importable (and used, tests/test_attn_probe_cpu.py) without a GPU.
"""
from __future__ import annotations

import math

import torch

# the tolerances of tests/test_attention_gpu.py::test_attention_fwd_bwd
OUT_TOL = dict(atol=2e-2, rtol=2e-2)
LSE_TOL = dict(atol=2e-2, rtol=1e-3)
BWD_ATOL, BWD_RTOL = 3e-2, 5e-2

# Most second targets of one key come from rows that name it as "the first / last key of a block";
# the backward atol scales with |g|max, so a key that many rows lean on (large dK, dV) would loosen
# the bound of every other element of its slot.
FAN_IN = 4

# (B, T, H, hd) of the GPU probes: every head dim at T = 200 (four forward tiles with a tail of 8
# keys, one or two backward key blocks), then T = 257 (a second 256-key block of one key), 520 and
# 777 (a partial last tile, four 256-key blocks), and the two-half kernels past one key block.
HEAD_DIMS = (8, 16, 24, 32, 48, 64, 80, 96, 112, 128)
SHAPES = [(2, 200, 2, hd) for hd in HEAD_DIMS] + [(2, 257, 2, 64), (2, 520, 2, 64), (2, 777, 2, 64),
                                                 (2, 520, 2, 80), (2, 300, 2, 128)]


def default_c(hd: int) -> float:
    """The query gain: target scores c * sqrt(hd) / 2 * (1 + cos(k_a, k_b)) against N(0, ~0.65 c^2)
    for every other key.  4 at every head dim: a power of two, so q = +-c m_d is exact in bf16 and
    rounds, once scaled, exactly as the key it came from does (see _sign_keys); 5 and 6 separate
    hd <= 32 a little better in fp64 but cost 3x in rounding error of dqkv."""
    return 4.0


def _second_target(i: int, T: int) -> list[int]:
    """Candidates for row i's second key, in order of preference (the first valid one that is not
    over-subscribed wins).  The tile sizes behind the offsets: 64-key forward tiles, 32-query wave
    slices of 128-query forward blocks; backward query tiles of 64 / 128 rows in 32-row subtiles,
    key blocks of 256 (hd <= 64) or 128 keys (hd > 64), split 16 keys at a time inside a wave."""
    if i == T - 1:
        # the last row: its own key T - 1 and one far back -- unless it is alone in the last tile
        # (T = 257), where the hand-off to see is from the last key of the tile before
        return [i - 1 if i % 64 == 0 else i // 3]
    s, u = i % 8, i // 8
    if s == 0:
        cand = [i - 64]  # exactly one forward tile back
    elif s == 1:  # the keys a block-boundary slip loses: named by a few rows each
        cand = [[(i // 128) * 128 - 1, (i // 256) * 256 - 1, (i // 64) * 64,
                 (i // 128) * 128, (i // 256) * 256, 0][u % 6]]
    elif s == 2:
        cand = [i - 1]  # the row before: the last key of the previous tile when i starts one
    elif s == 3:
        cand = [[i - 63, i - 65][u % 2]]
    elif s == 4:
        cand = []
    elif s == 5:
        cand = [[i - 127, i - 128, i - 129][u % 3], i - 31]
    elif s == 6:
        cand = [[i - 255, i - 256, i - 257][u % 3], i - 33]
    else:
        cand = [[i - 32, i - 16, i - 17, i - 15][u % 4]]
    return cand + [i // 2]


def probe_targets(T: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(a, b), int64 [T]: a(i) = i, b(i) <= i the second key of row i (b(0) = 0: one target)."""
    a = torch.arange(T)
    b = torch.zeros(T, dtype=torch.int64)
    fan = [0] * T
    for i in range(1, T):
        pick = i // 2
        for j in _second_target(i, T):
            if 0 <= j < i and fan[j] < FAN_IN:
                pick = j
                break
        fan[pick] += 1
        b[i] = pick
    return a, b


def _sign_keys(shape, hd, g):
    """Keys [*shape, hd] of one magnitude per dimension and head, m_d (uniform in [0.5, 1.5], scaled
    to |m|^2 = hd, bf16-exact), and a random sign per key and dimension: k_j = sigma_j * m.

    Why not randn keys: the kernels round Q * log2(e) / sqrt(hd) (forward) and K * log2(e) /
    sqrt(hd) (backward) to bf16, an error of 2^-9 relative in every product q_d k_d.  On a diffuse
    row that is nothing; at the ~23 log2 units of a peaked row's target scores it moves the two
    targets apart by ~0.02, P by ~1 % and out / dqkv by 1 to 2 times the tolerances (measured: the
    kernels and ``emulate`` agree on it to three digits), which would leave a lost key only ~10x
    above the noise.  With |k_j,d| = m_d for every key, q = c (k_a + k_b) / 2 is +-c m_d where the
    two targets agree and 0 elsewhere, so both target scores are the same sum of the same rounded
    products: their rounding error is common to the two, and a common score error cancels in the
    softmax (forward) or scales P_a and P_b alike (backward, absorbed by rtol; with c a power of two
    the forward's scaled q_d and the backward's scaled k_d round alike and that goes too).  What is
    left in ``emulate``: 0.16 of the tolerance for out, 0.8 for lse, 0.4 for dqkv.  Every key is still
    its own sign pattern, and another key's score is N(0, ~0.65 c^2) as with randn keys."""
    m = torch.rand(*shape[:1], 1, *shape[2:], hd, generator=g, dtype=torch.float64) + 0.5
    m = (m * (math.sqrt(hd) / m.norm(dim=-1, keepdim=True))).to(torch.bfloat16).double()
    return m * (torch.randint(0, 2, (*shape, hd), generator=g).double() * 2 - 1)


def probe_qkv(B, T, H, hd, seed, c=None):
    """(qkv bf16 [B * T, 3D], a, b).  Keys: _sign_keys, |k|^2 = hd; q_i = c * (k_a(i) + k_b(i)) / 2,
    whose two target scores are equal, after the bf16 rounding too; v: randn."""
    c = default_c(hd) if c is None else c
    g = torch.Generator().manual_seed(seed)
    a, b = probe_targets(T)
    k = _sign_keys((B, T, H), hd, g)
    v = torch.randn(B, T, H, hd, generator=g, dtype=torch.float64)
    q = (0.5 * c * (k[:, a] + k[:, b])).to(torch.bfloat16).double()
    qkv = torch.stack([q, k, v], dim=2).reshape(B * T, 3 * H * hd)  # [B, T, 3, H, hd]
    return qkv.to(torch.bfloat16), a, b


def _heads(x, B, T, H):
    return x.reshape(B, T, H, -1).transpose(1, 2)  # [B, H, T, hd]


def ref64(qkv, dout, B, T, H, keep=None, keep_scale=1.0, mask=None, dup=None):
    """Causal attention in fp64 on qkv's device: out [B * T, D], lse [B, H, T] in the log2 domain
    (as the kernel stores it; of the undropped softmax) and dqkv [B * T, 3D] by autograd for the
    output gradient dout.  keep [B, H, T, T] (0 / 1) * keep_scale multiplies the probabilities.
    The mutants: ``mask`` bool [T, T] replaces the causal mask; ``dup`` [T, T] multiplies the
    unnormalised probabilities (2 where a key is counted twice)."""
    D = qkv.shape[-1] // 3
    hd = D // H
    x = qkv.detach().double().requires_grad_()
    q, k, v = (_heads(t, B, T, H) for t in x.view(B, T, 3 * D).split(D, dim=2))
    if mask is None:
        mask = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~mask.to(qkv.device), float("-inf"))
    lse = torch.logsumexp(s, -1)
    if dup is None:
        p = (s - lse[..., None]).exp()
    else:
        e = (s - s.amax(-1, keepdim=True)).exp() * dup.to(qkv.device, torch.float64)
        p = e / e.sum(-1, keepdim=True)
    if keep is not None:
        p = p * (keep.double() * keep_scale)
    out = (p @ v).transpose(1, 2).reshape(B * T, D)
    out.backward(dout.double())
    return out.detach(), (lse / math.log(2.0)).detach(), x.grad


def _bf(x):
    return x.to(torch.bfloat16).float()


def emulate(qkv, dout, B, T, H, keep=None, keep_scale=1.0):
    """The kernels' arithmetic in fp32 torch with their rounding points (attention_fwd.hip,
    attention_train.hip), for deriving a bound: what error is rounding, whatever the kernel.
    Forward: Q * log2(e) / sqrt(hd) rounded to bf16 (the MFMA operand), S in the log2 domain, P
    rounded to bf16 before P V, out to bf16.  Backward: K * log2(e) / sqrt(hd) rounded to bf16, P
    = exp2(S - lse) with the forward's lse, delta from the bf16 out, the dropped P and dS rounded
    to bf16 before their products, dQ / dK / dV to bf16.  Returns (out, lse, dqkv) as fp32."""
    D = qkv.shape[-1] // 3
    hd = D // H
    c = math.log2(math.e) / math.sqrt(hd)
    q, k, v = (_heads(t, B, T, H) for t in qkv.float().view(B, T, 3 * D).split(D, dim=2))
    do = _heads(dout.float(), B, T, H)
    causal = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
    z = 1.0 if keep is None else keep.float()
    # forward
    s = (_bf(q * c) @ k.transpose(-1, -2)).masked_fill(~causal, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    out = _bf((_bf(p * z) @ v) * (keep_scale / l))
    lse = m + torch.log2(l)
    # backward
    ck = _bf(k * c)
    p = torch.exp2((q @ ck.transpose(-1, -2)).masked_fill(~causal, float("-inf")) - lse)
    pd = p * z
    delta = (do * out).sum(-1, keepdim=True)
    ds = _bf(pd * (do @ v.transpose(-1, -2)) - p * (delta / keep_scale))  # dS / keep_scale
    dq = _bf((ds @ ck) * (math.log(2.0) * keep_scale))
    dk = _bf((ds.transpose(-1, -2) @ q) * (keep_scale / math.sqrt(hd)))
    dv = _bf((_bf(pd).transpose(-1, -2) @ do) * keep_scale)
    flat = lambda t: t.transpose(1, 2).reshape(B, T, D)
    dqkv = torch.cat([flat(dq), flat(dk), flat(dv)], dim=2).reshape(B * T, 3 * D)
    return flat(out).reshape(B * T, D), lse[..., 0], dqkv


def target_mass(qkv, a, b, B, T, H):
    """fp64 softmax mass of row i on key a(i) and on key b(i): two [B, H, T] tensors."""
    D = qkv.shape[-1] // 3
    q, k, _ = (_heads(t, B, T, H) for t in qkv.double().view(B, T, 3 * D).split(D, dim=2))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D // H)
    p = s.masked_fill(~torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril(), float("-inf")).softmax(-1)
    idx = lambda t: t.to(qkv.device).expand(B, H, T)[..., None]
    return p.gather(-1, idx(a))[..., 0], p.gather(-1, idx(b))[..., 0]


def mutants(T):
    """name -> keyword arguments of ref64 that model one fault of a flash kernel.  Column-wide: a
    key lost (or counted twice) for every row past its block; single-row: the last key, the last
    row's diagonal, the key one tile back of each row."""
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    row, col = torch.arange(T)[:, None], torch.arange(T)[None, :]
    out = {}
    for key, first in ((64, 64), (127, 128), (255, 256), (256, 256)):
        if T > first:  # some row past the block exists
            out[f"col{key}_dropped_from_row{first}"] = dict(mask=causal & ~((col == key) & (row >= first)))
    out["last_col_dropped"] = dict(mask=causal & (col != T - 1))
    out["last_row_no_diagonal"] = dict(mask=causal & ~((row == T - 1) & (col == T - 1)))
    if T > 64:
        out["one_tile_back_dropped"] = dict(mask=causal & (col != row - 64))
        out["col64_twice"] = dict(dup=1.0 + ((col == 64) & (row >= 64)).double())
    out["last_col_twice"] = dict(dup=1.0 + (col == T - 1).expand(T, T).double())
    return out


COLUMN_WIDE = ("col64_dropped_from_row64", "col127_dropped_from_row128")


def violation(got, want, atol, rtol):
    """max |got - want| / (atol + rtol * |want|): <= 1 is what assert_close accepts."""
    want = want.double()
    return ((got.double() - want).abs() / (atol + rtol * want.abs())).max().item()


def bwd_violation(got, want, atol=BWD_ATOL, rtol=BWD_RTOL):
    """The backward tolerance of test_attention_fwd_bwd, atol = 3e-2 * max(1, |g|max / 4), with
    |g|max taken per slot (dQ, dK, dV): one key's large dV does not loosen dQ's bound.  Returns the
    largest violation of the three slots."""
    D = want.shape[-1] // 3
    worst = 0.0
    for s in range(3):
        w = want[:, s * D:(s + 1) * D]
        a = atol * max(1.0, w.abs().max().item() / 4)
        worst = max(worst, violation(got[:, s * D:(s + 1) * D], w, a, rtol))
    return worst


def dropout_scale(p):
    """The keep scale of attention_fwd / attention_bwd (attention_dropout_threshold and
    attention_dropout_scale, attention_fwd.hip): 16-bit decisions, p = thr / 65536."""
    if not p > 0:
        return 1.0
    thr = min(max(round(p * 65536.0), 1), 65535)
    return 65536.0 / (65536.0 - thr)


def _dense_keep(mask, B, T, H):
    """Dense [B, H, T(query), T(key)] keep matrix from the keep-bit row words (layout and bit
    order: attention_fwd.hip attn_dropmask_kernel; words of tiles past the diagonal are
    unspecified)."""
    ntw = 2 * ((T + 63) // 64)
    words = mask.view(B * H, ntw, T).to(torch.int64) & 0xFFFFFFFF  # [bh, j, q]
    key = torch.arange(T, device=mask.device)
    kk = key % 64
    j = (key // 64) * 2 + ((kk >> 2) & 1)
    e = 16 * (kk >> 5) + 4 * ((kk >> 3) & 3) + (kk & 3)  # the forward lane's value index
    bit = 16 * (e & 1) + (e >> 1)  # attn_common.h drop_bit: packed pair e >> 1
    w = words[:, j, :]  # [bh, key, q]
    return ((w >> bit[None, :, None]) & 1).transpose(1, 2).reshape(B, H, T, T).float()
