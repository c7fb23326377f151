"""The int8 KV cache kernels (csrc/kernels/attention_kv8.hip) against the numpy oracle of the KV8 rule
(``_kv8_oracle``) and against the bf16 decode kernel:

* ``kv8_store``: exact integers and scale bits, the in-place thirds equal s * q, Q untouched, positions
  past T untouched;
* ``attention_decode_kv8``: (a) it appends the rule's (q, s) of the new row and changes no other cache
  byte, (b) its output equals ``attention_decode`` on the snapped row over a bf16 cache of the
  dequantized rows bit for bit, (c) the counters return to zero and a captured call replays at other
  device positions;
* fp32 softmax(q K^T) V on the dequantized cache, NaN isolation, guard bands, argument checks."""
import pytest
import torch

import _kv8_oracle as O
from _guard import bit_equal, guarded
from mingpt_distributed_amd.models import generation as gen
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _oracle_kv(x, H):
    """(q int8 [..., 2, H, hd], s fp32 [..., 2, H], s * q bf16 [..., 2, H, hd]) of the K and V thirds of
    x [..., 3D] (bf16), on the CPU."""
    D = x.shape[-1] // 3
    kv = x[..., D:].float().cpu().numpy().reshape(*x.shape[:-1], 2, H, D // H)
    q, s, d = O.snap(kv)
    return torch.from_numpy(q), torch.from_numpy(s), torch.from_numpy(d).to(torch.bfloat16)


def _same_scales(got, want):
    got, want = got.cpu(), want.cpu()
    return (torch.equal(got.isnan(), want.isnan())
            and torch.equal(got.nan_to_num(-1.0).view(torch.int32), want.nan_to_num(-1.0).view(torch.int32)))


def _rand_rows(shape, seed, H):
    """bf16 rows [..., 3D] whose vectors span magnitudes 2^-8 .. 2^8."""
    g = torch.Generator().manual_seed(seed)
    D = shape[-1] // 3
    x = torch.randn(*shape, generator=g)
    mag = torch.randint(-8, 9, (*shape[:-1], 3 * H), generator=g).float().exp2().repeat_interleave(D // H, dim=-1)
    return (x * mag).to(torch.bfloat16)


# ------------------------------------------------------------------ kv8_store
STORE_SHAPES = [(2, 5, 2, 64), (1, 3, 3, 24), (1, 2, 1, 128), (2, 1, 2, 8)]


@pytest.mark.parametrize("B,T,H,hd", STORE_SHAPES)
def test_kv8_store_matches_the_oracle(B, T, H, hd):
    C, D, Tmax = ext(), H * hd, T + 3
    x = _rand_rows((B, T, 3 * D), 7, H)
    x[0, 0, D:D + hd] = 0                       # a zero K vector
    x[0, T - 1, 2 * D + 1] = 2.0 ** -120        # tiny elements beside ordinary ones
    x[B - 1, 0, 2 * D:2 * D + hd] = 0
    x[B - 1, 0, 2 * D + hd - 1] = -2.0 ** -120  # a V vector with a = 2^-120
    oq, os_, od = _oracle_kv(x, H)
    qkv = x.to(DEV)
    kq = torch.full((B, 2, H, Tmax, hd), 0x5A, dtype=torch.int8, device=DEV)
    ks = torch.full((B, 2, H, Tmax), -3.0, dtype=torch.float32, device=DEV)
    C.kv8_store(qkv, H, kq, ks)
    assert torch.equal(kq[:, :, :, :T].cpu(), oq.permute(0, 2, 3, 1, 4))
    assert _same_scales(ks[:, :, :, :T], os_.permute(0, 2, 3, 1))
    assert bool((kq[:, :, :, T:] == 0x5A).all()) and bool((ks[:, :, :, T:] == -3.0).all())
    assert bit_equal(qkv[..., D:].cpu(), od.reshape(B, T, 2 * D))
    assert bit_equal(qkv[..., :D].cpu(), x[..., :D])
    again = x.to(DEV)
    C.kv8_store(again, H)  # without a cache: the in-place half alone
    assert bit_equal(again, qkv)
    C.kv8_store(again, H)  # idempotent
    assert bit_equal(again, qkv)


def test_kv8_store_non_finite_vectors():
    C, B, T, H, hd = ext(), 1, 4, 2, 24
    D = H * hd
    x = _rand_rows((B, T, 3 * D), 8, H)
    x[0, 1, D + 3] = float("nan")          # K of head 0 at t = 1
    x[0, 2, 2 * D + hd] = float("inf")     # V of head 1 at t = 2
    oq, os_, od = _oracle_kv(x, H)
    qkv = x.to(DEV)
    kq = torch.zeros((B, 2, H, T, hd), dtype=torch.int8, device=DEV)
    ks = torch.zeros((B, 2, H, T), dtype=torch.float32, device=DEV)
    C.kv8_store(qkv, H, kq, ks)
    assert torch.equal(kq.cpu(), oq.permute(0, 2, 3, 1, 4)) and _same_scales(ks, os_.permute(0, 2, 3, 1))
    assert bool(ks[0, 0, 0, 1].isnan()) and bool(ks[0, 1, 1, 2].isnan()) and int(ks.isnan().sum()) == 2
    got = qkv[..., D:].cpu().view(B, T, 2, H, hd)
    assert torch.equal(got.isnan(), od.isnan()) and bit_equal(got.nan_to_num(0.0), od.nan_to_num(0.0))
    assert int(got.isnan().sum()) == 2 * hd


def test_kv8_store_guard_bands():
    C, B, T, H, hd = ext(), 2, 3, 3, 40
    D = H * hd
    x = _rand_rows((B, T, 3 * D), 9, H).to(DEV)
    kq = torch.zeros((B, 2, H, T + 1, hd), dtype=torch.int8, device=DEV)
    ks = torch.zeros((B, 2, H, T + 1), dtype=torch.float32, device=DEV)
    guarded(lambda qkv, kq, ks: C.kv8_store(qkv, H, kq, ks), {}, {"qkv": x, "kq": kq, "ks": ks}, name="kv8_store")


# ------------------------------------------------------------------ attention_decode_kv8
class _Case:
    """A history of random qkv rows [B, Tmax, 3D] as both caches -- int8 (kq, ks) from the oracle and bf16
    holding the dequantized rows -- plus one workspace per kernel, kept across consecutive calls."""

    def __init__(self, B, H, hd, Tmax, seed=0, edit=None):
        self.C, self.B, self.H, self.hd, self.Tmax, self.D = ext(), B, H, hd, Tmax, H * hd
        D = self.D
        hist = _rand_rows((B, Tmax, 3 * D), seed, H)
        if edit is not None:
            edit(hist)
        q, s, d = _oracle_kv(hist, H)
        self.kq = q.permute(0, 2, 3, 1, 4).contiguous().to(DEV)
        self.ks = s.permute(0, 2, 3, 1).contiguous().to(DEV)
        hist[..., D:] = d.reshape(B, Tmax, 2 * D)
        self.cache = hist.to(DEV)
        nf = self.C.attention_decode_part_floats(B, H, hd)
        self.part, self.part_ref = (torch.empty(nf, dtype=torch.float32, device=DEV) for _ in range(2))
        self.cnt, self.cnt_ref = (torch.zeros(B * H, dtype=torch.int32, device=DEV) for _ in range(2))
        self.seed = seed

    def new_row(self, edit=None):
        self.seed += 1
        x = _rand_rows((self.B, 3 * self.D), 1000 + self.seed, self.H)
        if edit is not None:
            edit(x)
        return x

    def step(self, pos, pos_dev=None, pos_stride=0, row=None, check=True):
        """One call of both kernels at ``pos`` (an int, or one per row with ``pos_stride`` 1); checks
        contract (a), (b), the counters and the fp32 reference; returns the KV8 output."""
        C, B, H, hd, D = self.C, self.B, self.H, self.hd, self.D
        x = self.new_row() if row is None else row
        oq, os_, od = _oracle_kv(x, H)  # [B, 2, H, hd], [B, 2, H]
        snapped = x.clone()
        snapped[:, D:] = od.reshape(B, 2 * D)
        rows = [pos] * B if isinstance(pos, int) else list(pos)
        want_q, want_s = self.kq.clone(), self.ks.clone()
        for b, p in enumerate(rows):
            want_q[b, :, :, p] = oq[b].to(DEV)
            want_s[b, :, :, p] = os_[b].to(DEV)
        xd = x.to(DEV)
        hpos = rows[0] if pos_dev is None else min(rows)
        out = C.attention_decode_kv8(xd, self.kq, self.ks, H, hpos, pos_dev, self.part, self.cnt, pos_stride)
        ref = C.attention_decode(snapped.to(DEV), self.cache, H, hpos, pos_dev, self.part_ref, self.cnt_ref, pos_stride)
        if not check:
            return out, ref
        assert bit_equal(xd.cpu(), x), "qkv_new was modified"
        assert torch.equal(self.kq, want_q), f"(a) int8 cache at pos {pos}"
        assert _same_scales(self.ks, want_s), f"(a) scales at pos {pos}"
        assert bit_equal(out, ref), (f"(b) pos {pos}: {int((out.view(torch.int16) != ref.view(torch.int16)).sum())} of "
                                     f"{out.numel()} outputs differ from attention_decode")
        assert int(self.cnt.abs().sum()) == 0, "(c) counters not back to zero"
        self.check_fp32(xd, out, rows)
        return out, ref

    def check_fp32(self, xd, out, rows):
        """fp32 softmax(q K^T / sqrt(hd)) V on the dequantized cache (the new row's snapped K / V are in
        ``cache`` by now), atol = rtol = 2e-2."""
        B, H, hd, D = self.B, self.H, self.hd, self.D
        for b, p in enumerate(rows):
            q = xd[b, :D].float().view(H, 1, hd)
            k = self.cache[b, :p + 1, D:2 * D].float().view(p + 1, H, hd).transpose(0, 1)
            v = self.cache[b, :p + 1, 2 * D:].float().view(p + 1, H, hd).transpose(0, 1)
            want = ((q @ k.transpose(1, 2)) / hd ** 0.5).softmax(-1) @ v
            torch.testing.assert_close(out[b].float().view(H, 1, hd), want, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("hd", [64, 128, 24])
def test_contract_three_rows(hd):
    """B * H = 6 (256 keys per split): one workgroup, two and three splits, the last position, and a
    short context again on the same counters."""
    c = _Case(3, 2, hd, 700)
    for i, pos in enumerate((0, 63, 64, 127, 128, 500, 699, 64)):
        pd = torch.tensor([pos], dtype=torch.int32, device=DEV) if i % 2 else None
        c.step(pos, pd)


def test_contract_many_pairs():
    """B * H = 36 > 32: 128 keys per split."""
    c = _Case(9, 4, 8, 300)
    for pos in (127, 128, 129, 299):
        c.step(pos, torch.tensor([pos], dtype=torch.int32, device=DEV))


def test_contract_all_sixteen_splits():
    c = _Case(1, 1, 8, 4096)
    for pos in (2048, 4095):
        c.step(pos)


@pytest.mark.parametrize("hd", [64, 40])
def test_contract_per_row_positions(hd):
    c = _Case(3, 2, hd, 700, seed=3)
    for rows in ((0, 130, 699), (699, 1, 256), (64, 64, 63)):
        c.step(rows, torch.tensor(rows, dtype=torch.int32, device=DEV), 1)


def test_a_captured_call_replays_at_three_device_positions():
    c = _Case(2, 2, 64, 600, seed=4)
    C, H = c.C, c.H
    x = c.new_row()
    xd = x.to(DEV)
    pd = torch.tensor([5], dtype=torch.int32, device=DEV)
    C.attention_decode_kv8(xd, c.kq, c.ks, H, 1, pd, c.part, c.cnt, 0)  # warm-up, then the same on the bf16 side
    snapped = x.clone()
    snapped[:, c.D:] = _oracle_kv(x, H)[2].reshape(c.B, 2 * c.D)
    sd = snapped.to(DEV)
    C.attention_decode(sd, c.cache, H, 1, pd, c.part_ref, c.cnt_ref, 0)
    graph, out = gen._capture(lambda: C.attention_decode_kv8(xd, c.kq, c.ks, H, 1, pd, c.part, c.cnt, 0))
    for pos in (40, 300, 599):
        pd.fill_(pos)
        graph.replay()
        ref = C.attention_decode(sd, c.cache, H, 1, pd, c.part_ref, c.cnt_ref, 0)
        assert bit_equal(out, ref), f"replay at {pos}"
        assert int(c.cnt.abs().sum()) == 0
        q, s, _ = _oracle_kv(x, H)
        assert torch.equal(c.kq[:, :, :, pos].cpu(), q) and _same_scales(c.ks[:, :, :, pos], s)


def test_tiny_scale_and_zero_vectors():
    """A K and a V vector with a = 2^-120 and a zero vector, in the cache and in the new row: the case
    that decides whether a scale may be folded out of a sum (here none is)."""
    B, H, hd, Tmax = 2, 2, 64, 300
    D = H * hd

    def tiny(x):
        r = x[:, 7] if x.dim() == 3 else x                 # the cache's row 7, or the new row itself
        r[0, D] = 2.0 ** -120                              # K of head 0: a = 2^-120
        r[0, D + 1] = 2.0 ** -127
        r[0, D + 2:D + hd] = 0
        r[1, 2 * D + hd:2 * D + 2 * hd] = 0                # V of head 1: a = 2^-120
        r[1, 2 * D + hd + 5] = -2.0 ** -120
        r[1, D:D + hd] = 0                                 # a zero K vector
        r[0, 2 * D:2 * D + hd] = 0                         # a zero V vector

    c = _Case(B, H, hd, Tmax, seed=5, edit=tiny)
    assert float(c.ks[0, 0, 0, 7]) == 2.0 ** -126 and float(c.ks[1, 1, 1, 7]) == 2.0 ** -126
    assert float(c.ks[1, 0, 0, 7]) == 1.0 and int(c.kq[1, 0, 0, 7].abs().max()) == 0
    for pos in (8, 140, 299):
        c.step(pos, row=c.new_row(edit=tiny))


@pytest.mark.parametrize("hd", [64, 24])
def test_cancelling_values_expose_every_rounding_step(hd):
    """Keys equal in pairs (K[t] = K[t - 1], so equal probabilities) over values that cancel in pairs
    (V[t] = -V[t - 1]): over the reals the cached keys contribute nothing, and what comes out is the
    rounding residue of the PV chains.  One differently rounded fp32 step -- a product p * v fused
    into the add in one kernel and rounded first in the other -- changes most outputs, where random
    inputs hide it behind the final rounding to bf16 in all but one output in ten thousand.  (The
    score products q * k are exact in fp32, both factors being bf16.)"""
    B, H, Tmax = 4, 4, 600
    D = H * hd

    def edit(hist):
        hist[:, 1::2, D:2 * D] = hist[:, 0:Tmax - 1:2, D:2 * D]
        hist[:, 1::2, 2 * D:] = -hist[:, 0:Tmax - 1:2, 2 * D:]

    c = _Case(B, H, hd, Tmax, seed=11, edit=edit)
    for pos in (255, 599, 300, 31):
        c.step(pos, torch.tensor([pos], dtype=torch.int32, device=DEV))
    for rows in ((599, 127, 128, 400),):
        c.step(rows, torch.tensor(rows, dtype=torch.int32, device=DEV), 1)


def test_a_nan_key_stays_in_its_own_head():
    B, H, hd, Tmax, pos = 3, 2, 24, 200, 150
    clean, dirty = _Case(B, H, hd, Tmax, seed=6), _Case(B, H, hd, Tmax, seed=6)
    x = clean.new_row()
    dirty.new_row()
    bad = x.clone()
    bad[1, clean.D + hd + 3] = float("nan")  # K of (b = 1, h = 1)
    want, _ = clean.step(pos, row=x)
    got, _ = dirty.step(pos, row=bad, check=False)
    assert bool(got.view(B, H, hd)[1, 1].isnan().all())
    assert bool(dirty.ks[1, 0, 1, pos].isnan()) and int(dirty.ks.isnan().sum()) == 1
    keep = torch.ones(B, H, dtype=torch.bool, device=DEV)
    keep[1, 1] = False
    assert bit_equal(got.view(B, H, hd)[keep], want.view(B, H, hd)[keep])
    # a NaN vector already in the cache: the same isolation on a later step
    y = clean.new_row()
    dirty.new_row()
    want, _ = clean.step(pos + 1, row=y)
    got, _ = dirty.step(pos + 1, row=y, check=False)
    assert bool(got.view(B, H, hd)[1, 1].isnan().all())
    assert bit_equal(got.view(B, H, hd)[keep], want.view(B, H, hd)[keep])


@pytest.mark.parametrize("B,H,hd,Tmax,pos", [(2, 2, 64, 300, 299), (1, 3, 24, 130, 0), (1, 3, 24, 130, 129)])
def test_decode_guard_bands(B, H, hd, Tmax, pos):
    """Inputs between NaN margins, caches and workspace between sentinels: nothing outside changes, and
    the result is the plain run's."""
    c = _Case(B, H, hd, Tmax, seed=7)
    x = c.new_row().to(DEV)
    pd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    fn = lambda qkv_new, pos_dev, kq, ks, part, counters: c.C.attention_decode_kv8(qkv_new, kq, ks, H, pos, pos_dev,
                                                                                  part, counters, 0)
    guarded(fn, {"qkv_new": x, "pos_dev": pd}, {"kq": c.kq, "ks": c.ks, "part": c.part.zero_(), "counters": c.cnt},
            name="attention_decode_kv8", skip=("part",))


def test_argument_checks():
    C = ext()
    B, H, hd, Tmax = 2, 2, 16, 32
    D = H * hd
    x = torch.zeros(B, 3 * D, dtype=torch.bfloat16, device=DEV)
    kq = torch.zeros(B, 2, H, Tmax, hd, dtype=torch.int8, device=DEV)
    ks = torch.zeros(B, 2, H, Tmax, dtype=torch.float32, device=DEV)
    C.attention_decode_kv8(x, kq, ks, H, Tmax - 1)  # the valid call
    bad = [
        (x.float(), kq, ks, H, 0), (x, kq.to(torch.int32), ks, H, 0), (x, kq, ks.double(), H, 0),
        (x, kq.view(torch.uint8), ks, H, 0), (x, kq[:1], ks, H, 0), (x, kq, ks[:, :, :, :-1], H, 0),
        (x, kq.view(B, 2, H * Tmax, hd), ks, H, 0), (x, kq, ks, H + 1, 0), (x[:, :-3], kq, ks, H, 0),
        (x, kq, ks, H, Tmax), (x, kq, ks, H, -1), (x.cpu(), kq, ks, H, 0), (x, kq.cpu(), ks.cpu(), H, 0),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            C.attention_decode_kv8(*args)
    with pytest.raises(RuntimeError):  # pos_stride without pos_dev, a short pos_dev, a short workspace
        C.attention_decode_kv8(x, kq, ks, H, 0, None, None, None, 1)
    with pytest.raises(RuntimeError):
        C.attention_decode_kv8(x, kq, ks, H, 0, torch.zeros(1, dtype=torch.int32, device=DEV), None, None, 1)
    with pytest.raises(RuntimeError):
        C.attention_decode_kv8(x, kq, ks, H, 0, None, torch.zeros(8, device=DEV),
                               torch.zeros(B * H, dtype=torch.int32, device=DEV))
    # hd % 8 != 0, hd > 128, Tmax > 4096
    for h, t in ((12, 16), (136, 16), (8, 4097)):
        xx = torch.zeros(1, 3 * h, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError):
            C.attention_decode_kv8(xx, torch.zeros(1, 2, 1, t, h, dtype=torch.int8, device=DEV),
                                   torch.zeros(1, 2, 1, t, dtype=torch.float32, device=DEV), 1, 0)
    q3 = torch.zeros(B, 4, 3 * D, dtype=torch.bfloat16, device=DEV)
    C.kv8_store(q3, H, kq, ks)  # the valid call
    for args in ((q3.float(), H, kq, ks), (q3, H, kq, None), (q3, H, None, ks), (q3, H, kq[:1], ks[:1]),
                 (torch.zeros(B, Tmax + 1, 3 * D, dtype=torch.bfloat16, device=DEV), H, kq, ks),
                 (q3, H + 1, kq, ks), (q3.view(B * 4, 3 * D), H, kq, ks),
                 (torch.zeros(1, 2, 36, dtype=torch.bfloat16, device=DEV), 1, None, None)):
        with pytest.raises(RuntimeError):
            C.kv8_store(*args)
