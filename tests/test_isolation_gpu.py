"""Isolation: what a kernel computes for one sequence, head or row must not depend on the data of
another.  Every comparison is bitwise, in the style of test_attention_causality: the staging of the
attention kernels reads rows of the next sequence and columns of the neighbouring head (masked
afterwards), LayerNorm pairs two rows per wave, the fused cross-entropy shares one reduction buffer
per workgroup -- a dropped mask multiplies the neighbour's data by 0 and stays invisible to a
tolerance test until that data is Inf or NaN.
"""
import pytest
import torch

from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, BF)


@pytest.fixture(params=[1, 2], ids=["bwd_persistent", "bwd_partials"])
def bwd_mode(request):
    ext().attention_set_bwd_mode(request.param)
    yield request.param
    ext().attention_set_bwd_mode(0)


def _attn(qkv, dout, B, T, H, p):
    C = ext()
    out, lse, mask = C.attention_fwd(qkv, B, T, H, p, 7)
    dqkv = C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 7)
    D = qkv.shape[1] // 3
    return out.view(B, T, D), lse.view(B, H, T), dqkv.view(B, T, 3 * D)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("hd", [64, 48])
@pytest.mark.parametrize("T", [77, 200])
def test_attention_batch_isolation(T, hd, p, bwd_mode):
    """Sequence 1 replaced (values 8x larger): out, lse and dqkv of sequences 0 and 2 unchanged."""
    B, H = 3, 2
    D = H * hd
    qkv, dout = _bf(B * T, 3 * D, seed=1), _bf(B * T, D, seed=2)
    base = _attn(qkv, dout, B, T, H, p)
    qkv2, dout2 = qkv.clone(), dout.clone()
    qkv2[T:2 * T] = _bf(T, 3 * D, scale=8.0, seed=3)
    dout2[T:2 * T] = _bf(T, D, scale=8.0, seed=4)
    other = _attn(qkv2, dout2, B, T, H, p)
    for name, a, b in zip(("out", "lse", "dqkv"), base, other):
        for s in (0, 2):
            assert torch.equal(a[s], b[s]), f"{name} of sequence {s} depends on sequence 1"
        assert not torch.equal(a[1], b[1])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("hd", [48, 80])
def test_attention_head_isolation(hd, p, bwd_mode):
    """hd = 48, 80: the 64-column staging reads into the neighbouring head.  Head 1's q, k, v and dout
    columns replaced: heads 0 and 2 unchanged in out, lse and every gradient."""
    B, T, H = 2, 130, 3
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
        assert torch.equal(base[0][..., cols], other[0][..., cols]), f"out of head {h} depends on head 1"
        assert torch.equal(base[1][:, h], other[1][:, h]), f"lse of head {h} depends on head 1"
        g0, g1 = (t.view(B, T, 3, D)[..., cols] for t in (base[2], other[2]))
        assert torch.equal(g0, g1), f"dqkv of head {h} depends on head 1"
    assert not torch.equal(base[0][..., h1], other[0][..., h1])
    assert not torch.equal(base[2].view(B, T, 3, D)[..., h1], other[2].view(B, T, 3, D)[..., h1])


@pytest.mark.parametrize("row", [2, 6, 9, 12])  # the pair partners (r, r + 4) of both 8-row blocks, and the last row
@pytest.mark.parametrize("D", [48, 520, 1600, 2056])
def test_layernorm_row_isolation(D, row):
    C = ext()
    M = 13
    x, w, b = _bf(M, D, seed=1), _bf(D, seed=2) * 0.1 + 1, _bf(D, seed=3) * 0.1
    dy, res = _bf(M, D, seed=4), _bf(M, D, seed=5)

    def run(x, dy, res):
        y, mean, rstd = C.layernorm_fwd(x, w, b, 1e-5)
        z = lambda: torch.zeros(D, device=DEV)  # noqa: E731
        dx = C.layernorm_bwd(dy, x, w, mean, rstd, z(), z(), res)
        dx2, dz = C.layernorm_bwd_dropout(dy, x, w, mean, rstd, z(), z(), res, z(), 0.1, 77)
        return y, mean, rstd, dx, dx2, dz

    base = run(x, dy, res)
    x2, dy2, res2 = x.clone(), dy.clone(), res.clone()
    x2[row], dy2[row], res2[row] = _bf(D, scale=8.0, seed=6) + 30, _bf(D, scale=8.0, seed=7), _bf(D, scale=8.0, seed=8)
    other = run(x2, dy2, res2)
    keep = torch.arange(M, device=DEV) != row
    for name, a, c in zip(("y", "mean", "rstd", "dx", "dx (dropout form)", "dz"), base, other):
        assert torch.equal(a[keep], c[keep]), f"{name}: a row other than {row} changed"
        assert not torch.equal(a[row], c[row])


@pytest.mark.parametrize("row", [0, 6, 12])
@pytest.mark.parametrize("V,ld", [(50257, 50304), (24577, 24584)])
def test_xent_fused_row_isolation(V, ld, row):
    C = ext()
    M = 13
    logits = _bf(M, ld, scale=3.0, seed=9)
    g = torch.Generator(device="cpu").manual_seed(1)
    tgt = torch.randint(0, V, (M,), generator=g).to(DEV)
    tgt[3] = -1
    out, dl = C.xent_fused(logits, tgt, V)
    logits2, tgt2 = logits.clone(), tgt.clone()
    logits2[row] = _bf(ld, scale=3.0, seed=10) + 40
    tgt2[row] = (int(tgt[row]) + 1) % V  # still a valid target: 1 / n_valid is the same
    out2, dl2 = C.xent_fused(logits2, tgt2, V)
    keep = torch.arange(M, device=DEV) != row
    assert torch.equal(dl[keep], dl2[keep]), f"dlogits of a row other than {row} changed"
    assert not torch.equal(dl[row], dl2[row]) and out[1].item() == out2[1].item() and out[0].item() != out2[0].item()
