"""Chained hd = 64 attention backward (attn_bwdchain_kernel, attention_set_bwd_mode(3): one workgroup
per (b, h) running its key blocks in order, dQ as a running fp32 sum, bf16 dQ rows stored by the last
contributor) against the key-block schedule with fp32 partials and a finalize pass (mode 2).

The chained kernel adds the key blocks' dQ in the finalize's order from the finalize's zero, and
scales and rounds as it does, so all of dqkv is bitwise equal; the fused qkv bias gradient agrees up
to the order of its cross-workgroup atomics (the tolerance of tests/test_attention_gpu.py)."""
import pytest
import torch

from _guard import guarded
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DB_TOL = dict(atol=1e-3, rtol=1e-4)


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ext().attention_set_bwd_mode(0)


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, BF)


def _inputs(B, T, H, hd, p, seed=3):
    C = ext()
    D = H * hd
    qkv, dout = _bf(B * T, 3 * D, seed=seed), _bf(B * T, D, seed=seed + 1)
    out, lse, mask = C.attention_fwd(qkv, B, T, H, p, 11)
    return qkv, out, dout, lse, mask


def _bwd(mode, ins, B, T, H, p, scrub=False):
    C = ext()
    qkv, out, dout, lse, mask = ins
    C.attention_set_bwd_mode(mode)
    db = torch.zeros(qkv.shape[1], device=DEV)
    if scrub:
        # the caching allocator hands the block of a freed same-sized tensor to dqkv: a row the kernel
        # forgot shows NaN instead of another call's result
        junk = torch.full((B * T, qkv.shape[1]), float("nan"), device=DEV, dtype=BF)
        torch.cuda.synchronize()
        del junk
    dqkv = C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 11, db)
    return dqkv, db


def _check(B, T, H, hd, p, mode=3, db_mode=2):
    ins = _inputs(B, T, H, hd, p)
    got, got_db = _bwd(mode, ins, B, T, H, p, scrub=True)  # the mode under test first
    ref, ref_db = _bwd(2, ins, B, T, H, p)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {got.numel()} elements differ"
    if db_mode != 2:
        ref_db = _bwd(db_mode, ins, B, T, H, p)[1]
    torch.testing.assert_close(got_db, ref_db, **DB_TOL)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,H", [(1, 257, 1), (2, 384, 2), (1, 512, 3), (1, 777, 2), (3, 1000, 1), (2, 1024, 2),
                                   (1, 2048, 2)])
def test_chained_equals_partials(B, T, H, p):
    """T = 257: the second block holds one key; T = 2048: eight key blocks, the finalize's second
    group of four."""
    _check(B, T, H, 64, p)


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_more_chains_than_workgroups():
    """B * H = n_cu + n_cu / 4: a quarter of the workgroups take a second chain from the counter and
    cross the chain-to-chain transition."""
    n = _n_cu()
    _check((n + n // 4) // 4, 512, 4, 64, 0.1)


def test_auto_dispatch_full_round():
    """Mode 0 with B * H = n_cu (fill 1.0, where auto takes the chained schedule) equals mode 2."""
    _check(_n_cu() // 4, 512, 4, 64, 0.1, mode=0)


@pytest.mark.parametrize("B,T,H,hd", [(2, 256, 2, 64), (1, 200, 3, 64), (2, 512, 2, 32)])
def test_mode3_falls_back(B, T, H, hd):
    """No chained schedule for a single key block or another head size: mode 3 takes mode 0's choice,
    and dqkv still equals mode 2's bitwise (with one key block the dQ summed in place is the same
    single term).  The bias gradient is compared with mode 0's own: with one key block that is the
    persistent schedule, whose column sums are taken over the bf16-rounded dqkv, not before the
    rounding as in mode 2 -- the two differ by that rounding noise in the parent already
    (test_attention_bwd_fused_bias_grad), which is not what a fallback has to preserve."""
    _check(B, T, H, hd, 0.1, db_mode=0)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", [257, 777])
def test_chained_guard_bands(T, p):
    C = ext()
    B, H = 2, 2
    qkv, out, dout, lse, mask = _inputs(B, T, H, 64, p)
    ins = {"qkv": qkv, "out": out, "dout": dout, "lse": lse, "mask": mask}
    C.attention_set_bwd_mode(3)
    (got,), _ = guarded(lambda qkv, out, dout, lse, mask: C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 11),
                        ins, name="attention_bwd chained")
    _, io = guarded(lambda qkv, out, dout, lse, mask, dbias: C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 11, dbias),
                    ins, {"dbias": torch.full((3 * H * 64,), 0.5, device=DEV)}, {"dbias": (1e-3, 1e-4)},
                    name="attention_bwd chained + dbias")
    C.attention_set_bwd_mode(2)
    db = torch.full((3 * H * 64,), 0.5, device=DEV)
    ref = C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 11, db)
    assert torch.equal(got, ref)
    torch.testing.assert_close(io["dbias"], db, **DB_TOL)


def _attn(qkv, dout, B, T, H, p):
    C = ext()
    out, lse, mask = C.attention_fwd(qkv, B, T, H, p, 7)
    C.attention_set_bwd_mode(3)
    return C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 7).view(B, T, -1)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_chained_batch_isolation(p):
    """Sequence 1 replaced (values 8x larger): dqkv of sequences 0 and 2 unchanged, bitwise."""
    B, T, H, D = 3, 600, 2, 128
    qkv, dout = _bf(B * T, 3 * D, seed=1), _bf(B * T, D, seed=2)
    base = _attn(qkv, dout, B, T, H, p)
    qkv2, dout2 = qkv.clone(), dout.clone()
    qkv2[T:2 * T] = _bf(T, 3 * D, scale=8.0, seed=3)
    dout2[T:2 * T] = _bf(T, D, scale=8.0, seed=4)
    other = _attn(qkv2, dout2, B, T, H, p)
    for s in (0, 2):
        assert torch.equal(base[s], other[s]), f"dqkv of sequence {s} depends on sequence 1"
    assert not torch.equal(base[1], other[1])


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_chained_head_isolation(p):
    """Head 1's q, k, v and dout columns replaced: the gradients of heads 0 and 2 unchanged, bitwise."""
    B, T, H, hd = 2, 300, 3, 64
    D = H * hd
    qkv, dout = _bf(B * T, 3 * D, seed=5), _bf(B * T, D, seed=6)
    base = _attn(qkv, dout, B, T, H, p)
    qkv2, dout2 = qkv.clone(), dout.clone()
    h1 = slice(hd, 2 * hd)
    qkv2.view(B * T, 3, D)[:, :, h1] = _bf(B * T, 3, hd, scale=8.0, seed=7)
    dout2[:, h1] = _bf(B * T, hd, scale=8.0, seed=8)
    other = _attn(qkv2, dout2, B, T, H, p)
    for h in (0, 2):
        cols = slice(h * hd, (h + 1) * hd)
        assert torch.equal(base.view(B, T, 3, D)[..., cols], other.view(B, T, 3, D)[..., cols]), \
            f"dqkv of head {h} depends on head 1"
    assert not torch.equal(base.view(B, T, 3, D)[..., h1], other.view(B, T, 3, D)[..., h1])
