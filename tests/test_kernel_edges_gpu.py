"""Edge shapes and dispatch branches that no fp32 comparison reached: LayerNorm's rstd (returned and
consumed by every backward, never asserted), tiny M, constant rows and rows with a large mean;
cross-entropy with every target ignored, with shifted logits, with the target in the last valid
column and through every fused instantiation; every K-loop tail of the GEMM kernels.  All oracles
are plain fp64 / fp32 torch.
"""
import pytest
import torch

from mingpt_distributed_amd.ops import gemm as G
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
EPS = 1e-5


def _bf(*shape, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(DEV, BF)


# ------------------------------------------------------------------------------ LayerNorm
LN_SHAPES = [(64, 48), (1000, 768), (257, 1600), (33, 192), (300, 4096),  # test_layernorm_fwd_bwd's
             (1, 48), (5, 768), (7, 1024), (8, 512), (31, 2048)]


def _stats64(x):
    xd = x.double()
    return xd.mean(-1), (xd.var(-1, unbiased=False) + EPS).rsqrt()


@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_rstd(M, D):
    """rstd against fp64.  Standard-normal rows: rtol 1e-3 (what test_layernorm_fwd_bwd uses for
    mean).  Rows with mean 30 and std 0.5: rtol 1e-5 -- the kernel's two-pass (mean, then centred
    variance) fp32 arithmetic is within ~2e-7 of fp64 there, a one-pass E[x^2] - mean^2 form is off
    by 2e-4 or more, so the bound separates the two with > 20x margin on each side."""
    C = ext()
    w, b = _bf(D, seed=2) * 0.1 + 1, _bf(D, seed=3) * 0.1
    x = _bf(M, D, seed=1)
    y, mean, rstd = C.layernorm_fwd(x, w, b, EPS)
    mu64, rs64 = _stats64(x)
    torch.testing.assert_close(mean.double(), mu64, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(rstd.double(), rs64, atol=0, rtol=1e-3)
    yr = torch.nn.functional.layer_norm(x.float(), (D,), w.float(), b.float(), EPS)
    torch.testing.assert_close(y.float(), yr, atol=3e-2, rtol=0.02)
    x = _bf(M, D, scale=0.5, shift=30.0, seed=4)
    y, mean, rstd = C.layernorm_fwd(x, w, b, EPS)
    mu64, rs64 = _stats64(x)
    torch.testing.assert_close(mean.double(), mu64, atol=0, rtol=1e-5)
    torch.testing.assert_close(rstd.double(), rs64, atol=0, rtol=1e-5)
    xh = ((x.double() - mu64[:, None]) * rs64[:, None]).float()
    torch.testing.assert_close(y.float(), xh * w.float() + b.float(), atol=3e-2, rtol=0.02)


@pytest.mark.parametrize("M,D", [(1, 48), (5, 768), (13, 1600), (9, 4096)])
def test_layernorm_constant_rows(M, D):
    """x = 3 everywhere: mean 3, variance 0, rstd = 1 / sqrt(eps), y = bf16(b) exactly, dx finite."""
    C = ext()
    w, b = _bf(D, seed=2) * 0.1 + 1, _bf(D, seed=3) * 0.1
    x = torch.full((M, D), 3.0, device=DEV, dtype=BF)
    y, mean, rstd = C.layernorm_fwd(x, w, b, EPS)
    assert torch.equal(mean, torch.full_like(mean, 3.0))
    torch.testing.assert_close(rstd.double(), torch.full_like(rstd, 0).double() + EPS ** -0.5, atol=0, rtol=1e-5)
    assert torch.equal(y, b.expand(M, D))
    dw, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dy = _bf(M, D, seed=4)
    dx = C.layernorm_bwd(dy, x, w, mean, rstd, dw, db, None)
    assert torch.isfinite(dx.float()).all() and torch.isfinite(dw).all()
    torch.testing.assert_close(db, dy.float().sum(0), atol=1e-3, rtol=1e-4)
    assert (dw == 0).all()  # xhat = 0


# ------------------------------------------------------------------------------ cross-entropy
FUSED_ODD = [(50257, 50304), (24577, 24584), (49150, 49152), (65529, 65536)]  # V % 8 != 0; NV = 7, 4, 6, 8


def _both_paths(C, logits, tgt, V, gs):
    """(name, loss, 1 / n_valid, dlogits scaled by gs) of the two-kernel and the fused path."""
    g = torch.tensor([gs], device=DEV)
    out, lse = C.xent_fwd(logits, tgt, V)
    yield "xent_fwd/bwd", out, C.xent_bwd(logits, tgt, lse, g, out, V)
    res = C.xent_fused(logits, tgt, V)
    if res:
        out, dl = res
        C.xent_scale_(dl, g)
        yield "xent_fused", out, dl


def _xent_check(C, logits, tgt, V, gs=2.0):
    lr = logits.float()[:, :V].clone().requires_grad_()
    ref = torch.nn.functional.cross_entropy(lr, tgt, ignore_index=-1)
    ref.backward(torch.tensor(gs, device=DEV))
    names = []
    for name, out, dl in _both_paths(C, logits, tgt, V, gs):
        torch.testing.assert_close(out[0], ref.detach(), atol=1e-3, rtol=1e-3, msg=lambda m: f"{name} loss: {m}")
        torch.testing.assert_close(dl[:, :V].float(), lr.grad, atol=2e-3, rtol=0.02, msg=lambda m: f"{name}: {m}")
        assert (dl[:, V:] == 0).all(), name
        names.append(name)
    return names


@pytest.mark.parametrize("M,V,ld", [(5, 65, 72), (3, 50257, 50304), (2, 24577, 24584)])
def test_xent_all_targets_ignored(M, V, ld):
    """n_valid = 0 (the n > 0 ? 1 / n : 0 branch): loss 0, 1 / n_valid 0, dlogits all zero."""
    C = ext()
    logits = _bf(M, ld, scale=3.0, seed=8)
    tgt = torch.full((M,), -1, device=DEV, dtype=torch.int64)
    paths = list(_both_paths(C, logits, tgt, V, 2.0))
    assert len(paths) == (2 if ld >= 24584 else 1)
    for name, out, dl in paths:
        assert out[0].item() == 0.0 and out[1].item() == 0.0, (name, out)
        assert torch.isfinite(dl.float()).all() and (dl == 0).all(), name


@pytest.mark.parametrize("M,V,ld", [(17, 65, 72), (9, 50257, 50304), (9, 32768, 32768)])
def test_xent_shifted_logits(M, V, ld):
    """Logits around +60 with scale 3: exp() of the raw values overflows fp32 (e^88), so the result is
    right only if the row maximum is subtracted first."""
    C = ext()
    logits = _bf(M, ld, scale=3.0, shift=60.0, seed=8)
    g = torch.Generator(device="cpu").manual_seed(2)
    tgt = torch.randint(0, V, (M,), generator=g).to(DEV)
    tgt[::5] = -1
    assert len(_xent_check(C, logits, tgt, V)) == (2 if ld >= 24584 else 1)


@pytest.mark.parametrize("V,ld", FUSED_ODD + [(13, 16), (65, 72)])
def test_xent_target_in_last_valid_column(V, ld):
    """V % 8 != 0 and the target in column V - 1 (the partial 16-byte vector), M = 9: against fp32
    through every path the row width allows -- the fused kernel's instantiations with 4, 6, 7 and 8
    vectors per lane among them (5: tests/test_kernels_gpu.py's 40064)."""
    C = ext()
    M = 9
    logits = _bf(M, ld, scale=3.0, seed=9)
    logits[:, V:] = 1e4  # a pad column that is read would dominate every row
    g = torch.Generator(device="cpu").manual_seed(3)
    tgt = torch.randint(0, V, (M,), generator=g).to(DEV)
    tgt[0] = tgt[4] = tgt[8] = V - 1
    tgt[2] = -1
    assert len(_xent_check(C, logits, tgt, V, gs=1.0)) == (2 if ld >= 24584 else 1)


# ------------------------------------------------------------------------------ GEMM K-loop tails
@pytest.fixture(params=[0, 1, 5, 6], ids=["auto", "t128", "w4", "w4n192"])
def tile_config(request):
    ext().gemm_set_variant(request.param)
    yield request.param
    ext().gemm_set_variant(0)


def _check(out, ref, K):  # tests/test_gemm_gpu.py
    tol = 2e-2 * (K ** 0.5) * 0.25 + 2e-2
    torch.testing.assert_close(out.float(), ref, atol=tol, rtol=2e-2)


K_TAILS = [64, 128, 192, 256, 320, 384, 328]  # 1..6 K-tiles of 64 (every count mod 6), and 5 + a partial one


@pytest.mark.parametrize("K", K_TAILS)
def test_gemm_k_tails(K, tile_config):
    """NT, NN and TN against fp32 for every K-tile count mod 6 (the W4 loop is unrolled over a ring of
    slots and finishes with a tail of 1-5 tiles) plus a partial K-tile.  A is the identity-like
    probe's opposite: random data, so a K-tile that is skipped or read twice moves every output."""
    M, N = 130, 72
    a, b = _bf(M, K, seed=1), _bf(N, K, seed=2)
    _check(G.gemm_nt(a, b), a.float() @ b.float().t(), K)
    bn = _bf(K, N, seed=3)
    _check(G.gemm_nn(a, bn), a.float() @ bn.float(), K)
    ta, tb = _bf(K, N, seed=4), _bf(K, 136, seed=5)  # TN: the reduction runs over the K rows
    c0 = torch.randn(N, 136, device=DEV)
    c = c0.clone()
    G.gemm_tn_acc(ta, tb, c)
    _check(c, c0 + ta.float().t() @ tb.float(), K)
