"""The row-wise training kernels (layernorm.hip, xent.hip, elementwise.hip, embedding.hip) against
references that can see a single row or a single 16-byte vector, on the probes of tests/_row_probe.py
(checked in test_row_probe_cpu.py):

* exact integers: LayerNorm backward dw / db (mean and rstd are handed in as integers and powers of
  two), dx == dres with w = 0, the fused dropout backward dz / dzb, bias_grad, dropout_bias_grad, the
  elementwise epilogues and the embedding.  Every value is exact in bf16 and fp32 in any summation or
  atomic order, every accumulator starts from a nonzero integer vector, and the comparison has no
  tolerance (integers are compared by value: the sign of a zero is the only bit that may differ);
* shapes that reach the branches the assert_close tests never ran: LayerNorm's capped grid (asserted
  through layernorm_bwd_grid), ln_colsum's partial second chunk, the second grid-stride trip of the
  elementwise kernels and of xent_scale, bias_grid's halving loop, the second 512-column trip of the
  embedding kernels, cross-entropy finalize / count past 1024 rows;
* per-element allowances in place of atol / rtol: LayerNorm dx and y, GELU', cross-entropy dlogits and
  lse against fp64, within one bf16 ulp plus a few fp32 ulps of the terms that cancel.

The dropout keep set comes from test_dropout_mask_oracle_gpu.oracle_keep; p = 0.5, so the keep scale
is exactly 2."""
import numpy as np
import pytest
import torch

import _row_probe as P
from _guard import bit_equal
from mingpt_distributed_amd.ops._ext import ext
from test_kernel_edges_gpu import LN_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _bf(t):
    """int8 (any device) -> bf16 on the GPU, exactly."""
    return t.to(DEV).to(torch.float32).to(BF)


def _f32(t):
    return t.to(DEV).to(torch.float32)


def _keep(M, N):
    return P.keep_mask(M, N, device=DEV)


# ------------------------------------------------------------------------------ a. LayerNorm backward census
def _ln_dev(c):
    d = {k: _bf(c[k]) for k in ("x", "dy", "dres", "w")}
    d.update(mean=_f32(c["mean"]), rstd=_f32(c["rstd2"]) / 2, dw0=_f32(c["dw0"]), db0=_f32(c["db0"]),
             dzb0=_f32(c["dzb0"]), w0=torch.zeros(c["D"], dtype=BF, device=DEV))
    return d


def _ln_bwd(d, w, dres, drop):
    """(dx, dw, db, dz, dzb) with the accumulators started from their nonzero initial values."""
    C = ext()
    dw, db = d["dw0"].clone(), d["db0"].clone()
    if not drop:
        return C.layernorm_bwd(d["dy"], d["x"], w, d["mean"], d["rstd"], dw, db, dres), dw, db, None, None
    dzb = d["dzb0"].clone()
    dx, dz = C.layernorm_bwd_dropout(d["dy"], d["x"], w, d["mean"], d["rstd"], dw, db, dres, dzb, P.DROP_P, P.DROP_SEED)
    return dx, dw, db, dz, dzb


def _ln_census_checks(c, drops=(False, True)):
    """dw == dw0 + sum dy xhat and db == db0 + sum dy with integer w; with w = 0 and dres also
    dx == dres, and under the fused dropout dz == 2 keep dres, dzb == dzb0 + sum dz."""
    M, D = c["M"], c["D"]
    cg, d = P.to_dev(c, DEV), _ln_dev(c)
    dw_want, db_want = P.ln_census(cg)
    tag = f"({M}, {D})"
    if False in drops:
        _, dw, db, _, _ = _ln_bwd(d, d["w"], None, False)
        P.exact(dw, dw_want, f"{tag} dw")
        P.exact(db, db_want, f"{tag} db")
        dx, dw, db, _, _ = _ln_bwd(d, d["w0"], d["dres"], False)
        P.exact(dx, cg["dres"], f"{tag} dx == dres")
        P.exact(dw, dw_want, f"{tag} dw (w = 0)")
        P.exact(db, db_want, f"{tag} db (w = 0)")
    if True in drops:
        dz_want, dzb_want = P.ln_dz(cg, _keep(M, D))
        dx, dw, db, dz, dzb = _ln_bwd(d, d["w0"], d["dres"], True)
        P.exact(dx, cg["dres"], f"{tag} dropout dx == dres")
        P.exact(dz, dz_want, f"{tag} dz")
        P.exact(dzb, dzb_want, f"{tag} dzb")
        P.exact(dw, dw_want, f"{tag} dropout dw")
        P.exact(db, db_want, f"{tag} dropout db")


@pytest.mark.parametrize("D", P.LN_D)
@pytest.mark.parametrize("M", P.LN_M_SMALL + (P.LN_M_CHUNK,))
def test_ln_bwd_census(M, D):
    """M = 1, 5, 12, 37: one block (grid = max(1, M / 32)) whose waves stride over the rows, the pair
    partner r0 + 4 absent and present.  M = 1063: grid 33, so ln_colsum_kernel's second 32-row chunk
    holds one partial row (asserted through layernorm_bwd_grid), with and without the dropout plane."""
    C = ext()
    if M == P.LN_M_CHUNK:
        assert C.layernorm_bwd_grid(M, D, False) == 33 and C.layernorm_bwd_grid(M, D, True) == 33
    else:
        assert C.layernorm_bwd_grid(M, D, False) == max(1, M // 32)
    _ln_census_checks(P.ln_case(M, D))


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("D", P.LN_D_PER_NV)
def test_ln_bwd_census_capped_grid(D, drop):
    """ln_bwd_grid caps the grid at one resident wave of blocks: with M = 32 cap + 45 rows the grid is
    cap < M / 32, so blocks take a second trip of the row loop, the last one partial."""
    C = ext()
    cap = C.layernorm_bwd_grid(1 << 20, D, drop)
    M = 32 * cap + 45
    assert C.layernorm_bwd_grid(M, D, drop) == cap < M // 32
    assert M * D * 2 <= 256 << 20
    print(f"D {D} dropout {drop}: cap {cap}, M {M}")
    _ln_census_checks(P.make_ln_case(M, D), drops=(drop,))


# ------------------------------------------------------------------------------ b. LayerNorm per element
@pytest.mark.parametrize("D", P.LN_D)
@pytest.mark.parametrize("M", [12, 37])
def test_ln_dx_per_element(M, D):
    """dx against fp64 rs (g w - s1 - xhat s2) (+ dres) within 2^-7 |ref| + 8 2^-24 rs (|g w| + |s1| +
    |xhat s2| + |dres|), integer w in [-2, 2]; plain and fused-dropout launches.
    Measured on an MI355X: worst error / allowance 0.498 (the bf16 rounding)."""
    c = P.ln_case(M, D)
    d = _ln_dev(c)
    for with_dres in (False, True):
        ref, allow = P.ln_dx_ref(c, with_dres)
        for drop in (False, True):
            dx = _ln_bwd(d, d["w"], d["dres"] if with_dres else None, drop)[0]
            P.within(dx.cpu(), ref, allow, f"dx ({M}, {D}) dres {with_dres} dropout {drop}")


@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_ln_fwd_per_element(M, D):
    """y on the standard-normal data of test_layernorm_rstd against fp64 LayerNorm of the bf16 inputs
    within 2^-7 |ref| + 8 2^-24 (|xhat w| + |b|).  (That test's second data set, rows with mean 30 and
    standard deviation 0.5, is outside this allowance by construction: it has no term for the fp32
    error of a mean 60 standard deviations from zero, and a plain fp32 evaluation leaves it 100-fold
    where xhat w + b cancels -- test_row_probe_cpu.py::test_ln_fwd_allowance_is_for_centred_rows.)
    Measured on an MI355X: worst error / allowance 0.498 (the bf16 rounding) over the ten shapes."""
    c = P.ln_fwd_case(M, D)
    ref, allow = P.ln_fwd_ref(c)
    y, _, _ = ext().layernorm_fwd(c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), 1e-5)
    P.within(y.cpu(), ref, allow, f"y ({M}, {D})")


# ------------------------------------------------------------------------------ c. bias gradients
def _bias_checks(c):
    C = ext()
    M, N = c["dy"].shape
    cg = P.to_dev(c, DEV)
    dy = _bf(c["dy"])
    db = _f32(c["db0"])
    C.bias_grad(dy, db)
    P.exact(db, P.bias_census(cg), f"({M}, {N}) bias_grad db")
    dx_want, db_want = P.bias_census(cg, _keep(M, N))
    db = _f32(c["db0"])
    dx = C.dropout_bias_grad(dy, db, P.DROP_P, P.DROP_SEED)
    assert bit_equal(dx, dx_want.to(BF)), f"({M}, {N}) dropout_bias_grad dx"
    P.exact(db, db_want, f"({M}, {N}) dropout_bias_grad db")


@pytest.mark.parametrize("N", P.BIAS_N)
@pytest.mark.parametrize("M", P.BIAS_M)
def test_bias_grad_census(M, N):
    """db == db0 + sum dy; dx == 2 keep dy bit for bit and db == db0 + sum dx.  N covers 32- and
    64-lane column blocks (768, 2304: 32) and a partial column block (4104 = 8 x 512 + 8); M covers one
    row, one short of / exactly one block row (ry = M / 64) and 64 block rows + 3."""
    _bias_checks(P.bias_case(M, N))


def test_bias_grad_census_halving():
    """(32773, 3072): cx = 3072 / 512 = 6 column blocks, ry = min(512, 32773 / 64) = 512, 6 x 512 = 3072
    > 2048, so bias_grid halves ry 512 -> 256 (1536 blocks)."""
    M, N = P.BIAS_HALVING
    assert N % 512 == 0 and M // 64 >= 512 and (N // 512) * 512 > 2048 >= (N // 512) * 256
    _bias_checks(P.make_bias_case(M, N))


# ------------------------------------------------------------------------------ d. elementwise grid-stride
@pytest.mark.parametrize("M,N", P.ELT_SHAPES)
def test_elementwise_integers(M, N):
    """bias_act (act 0), bias_dropout_residual at p = 0 and 0.5, dropout_bwd at 0.5.  At (2740, 3072) the
    grid is capped at 4096 blocks of 256 lanes x 8 elements, so every loop takes a second trip."""
    C = ext()
    if M > 3:
        assert 4096 * 256 * 8 < M * N
    c = P.elt_case(M, N)
    cg = P.to_dev(c, DEV)
    x, b, r, dy = (_bf(c[k]) for k in ("x", "b", "r", "dy"))
    xb = cg["x"].int() + cg["b"].int()
    keep = _keep(M, N)
    P.exact(C.bias_act(x, b, None, 0), xb, "bias_act")
    P.exact(C.bias_act(x, None, None, 0), cg["x"], "bias_act without bias")
    P.exact(C.bias_dropout_residual(x, b, r, 0.0, P.DROP_SEED), cg["r"].int() + xb, "bias_dropout_residual p = 0")
    P.exact(C.bias_dropout_residual(x, b, r, P.DROP_P, P.DROP_SEED), cg["r"].int() + torch.where(keep, 2 * xb, 0),
            "bias_dropout_residual p = 0.5")
    want = torch.where(keep, 2 * cg["dy"].int(), 0).to(torch.float32).to(BF)
    assert bit_equal(C.dropout_bwd(dy, P.DROP_P, P.DROP_SEED), want), "dropout_bwd"


@pytest.mark.parametrize("M,N", P.ELT_SHAPES)
def test_gelu_bwd_grid_stride(M, N):
    """dx against fp64 dy GELU'(pre) (tanh form) within 2^-7 |ref| + |dy| 2^-18, dy ~ N(0, 1), pre ~
    2 N(0, 1).  The absolute term covers the kernel's sigmoid form (common.h gelu_grad) where the
    derivative crosses zero and the relative term vanishes: with s = rcp(1 + exp2(t)), t = x (E1 x^2 +
    E0), three roundings in t (3 x 2^-24 |t| ln 2 relative in exp2's result), 1 ulp of exp2, the
    rounding of 1 + e and 1 ulp of rcp give |ds| <= s (1 - s) (3 x 2^-24 ln 2 |t| + 2^-23) + 1.5 x 2^-23 s;
    GELU' = s + P, P = 2 K0 x s (1 - s) (1 + 3 K1 x^2), moves by |1 + 2 K0 x (1 - 2 s) (1 + 3 K1 x^2)| |ds|,
    the product's own roundings add 8 x 2^-24 |P| and the final fma 2^-24 |GELU'|.  Over every bf16 x
    the sum stays below 2^-8 |GELU'| + 2^-18, the room the allowance leaves beside the bf16 rounding
    (test_row_probe_cpu.py::test_gelu_error_model evaluates it: at most 0.022 of that room, at x =
    -0.754, the zero crossing).
    Measured on an MI355X: worst error / allowance 0.428 at (3, 24), 0.498 at (2740, 3072)."""
    if M > 3:
        assert 4096 * 256 * 8 < M * N
    c = P.elt_case(M, N)
    ref, allow = P.gelu_bwd_ref(P.to_dev(c, DEV))
    dx = ext().gelu_bwd(c["gdy"].to(DEV), c["pre"].to(DEV))
    P.within(dx, ref, allow, f"gelu_bwd ({M}, {N})")


# ------------------------------------------------------------------------------ e. embedding
@pytest.mark.parametrize("B,T", P.EMB_BT)
@pytest.mark.parametrize("D", P.EMB_D)
def test_embedding_census(D, B, T):
    """Forward wte[idx] + wpe[t] (p = 0) and 2 keep (...) (p = 0.5); backward dwte == dwte0 + index_add
    and dwpe[:T] == dwpe0[:T] + sum_b, p = 0 and 0.5; the six unused rows of dwte and rows >= T of dwpe keep
    their bits.  D = 520, 768, 1600 take the second (and fourth) trip of the 512-column loops; M = B T =
    21 and 256: M % 4 nonzero and zero."""
    C = ext()
    c = P.emb_case(B, T, D)
    cg = P.to_dev(c, DEV)
    idx, wte, wpe, dout = cg["idx"], _bf(c["wte"]), _bf(c["wpe"]), _bf(c["dout"])
    unused = [v for v in range(P.EMB_V) if v not in P.EMB_TOKENS]
    for p, keep in ((0.0, None), (P.DROP_P, _keep(B * T, D))):
        out = C.embedding_fwd(idx, wte, wpe, p, P.DROP_SEED)
        P.exact(out.view(B * T, D), P.emb_fwd_expected(cg, keep), f"embedding_fwd p = {p}")
        dwte, dwpe = _f32(c["dwte0"]), _f32(c["dwpe0"])
        C.embedding_bwd(idx, dout, dwte, dwpe, p, P.DROP_SEED)
        dwte_want, dwpe_want = P.emb_bwd_expected(cg, keep)
        P.exact(dwte, dwte_want, f"dwte p = {p}")
        P.exact(dwpe, dwpe_want, f"dwpe p = {p}")
        assert bit_equal(dwte[unused], _f32(c["dwte0"])[unused]), "an unused row of dwte was written"
        assert bit_equal(dwpe[T:], _f32(c["dwpe0"])[T:]), "a row >= T of dwpe was written"


# ------------------------------------------------------------------------------ f. cross-entropy
def _both_paths(logits, tgt, V, gs):
    """(name, out, lse or None, dlogits scaled by gs) of the two-kernel and, where the row width
    allows, the fused path; the number of paths is asserted: both from ld = 24584 on."""
    C = ext()
    g = torch.tensor([gs], device=DEV)
    out, lse = C.xent_fwd(logits, tgt, V)
    paths = [("xent_fwd/bwd", out, lse, C.xent_bwd(logits, tgt, lse, g, out, V))]
    res = C.xent_fused(logits, tgt, V)
    if res:
        out, dl = res
        C.xent_scale_(dl, g)
        paths.append(("xent_fused", out, None, dl))
    assert len(paths) == (2 if logits.shape[1] >= P.XENT_FUSED_MIN_LD else 1)
    return paths


def _ulp32(v):
    return float(np.spacing(np.float32(v)))


@pytest.mark.parametrize("shift", [0.0, 60.0])
@pytest.mark.parametrize("M,V,ld", P.XENT_SHAPES)
def test_xent_per_element(M, V, ld, shift):
    """dlogits against fp64 (softmax - onehot) gs / n_valid from the bf16 logits within 2^-7 |ref| +
    g 2^-20, g = gs / n_valid, gs = 2; ignored rows and pad columns (which hold 1e4 in the logits)
    exactly 0; lse of xent_fwd within 16 2^-24 max(|lse|, 1); out == {mean loss, 1 / n_valid}.  Targets:
    every 5th row ignored, row 1 in column V - 1, row 2 at its row's argmax.  Both paths from ld = 24584.
    Measured on an MI355X, worst error / allowance over the ten cases: dlogits 0.492 on both paths (the
    bf16 rounding); lse 0.054."""
    c = P.xent_case(M, V, ld, shift)
    logits, tgt = c["logits"].to(DEV), c["tgt"].to(DEV)
    n_valid = int((c["tgt"] >= 0).sum())
    lse64, d64, allow, loss64 = P.xent_ref(logits, tgt, V, 2.0 / n_valid)
    loss = float(loss64.sum()) / n_valid
    tag = f"{(M, V, ld)} shift {shift}"
    for name, out, lse, dl in _both_paths(logits, tgt, V, 2.0):
        P.within(dl, d64, allow, f"{name} dlogits {tag}")
        if lse is not None:
            P.within(lse, lse64, P.lse_allow(lse64), f"{name} lse {tag}")
        want = np.float32(1) / np.float32(n_valid)
        assert abs(out[1].item() - float(want)) <= _ulp32(want), (name, out)
        assert abs(out[0].item() - loss) <= 2.0 ** -20 * abs(loss) + float(P.lse_allow(lse64).max()), (name, out, loss)


@pytest.mark.parametrize("M,V,ld,k", P.XENT_LONG)
def test_xent_single_valid_row_past_1024(M, V, ld, k):
    """xent_finalize_kernel and xent_count_kernel stride by 1024 threads: with every target -1 except
    row r, r = 0, 1023, 1024, M - 1, out[1] == 1, out[0] == lse_r - logit_r[t] (within the lse allowance
    + 2^-22) and dlogits is nonzero in row r only (and inside the per-element allowance there).
    Measured on an MI355X, worst error / allowance: row r of dlogits 0.474 (xent_fwd/bwd), 0.445
    (xent_fused); lse 0.059."""
    logits = P.xent_long_logits(M, V, ld).to(DEV)
    for r in (0, 1023, 1024, M - 1):
        tgt = torch.full((M,), -1, dtype=torch.int64, device=DEV)
        tgt[r] = (7 * r + 3) % V
        lse64, d64, allow, loss64 = P.xent_ref(logits[r:r + 1], tgt[r:r + 1], V, 2.0)
        others = torch.arange(M, device=DEV) != r
        for name, out, lse, dl in _both_paths(logits, tgt, V, 2.0):
            assert out[1].item() == 1.0, (name, r, out)
            assert abs(out[0].item() - loss64.item()) <= P.lse_allow(lse64).item() + 2.0 ** -22, (name, r, out, loss64)
            assert (dl[others] == 0).all(), f"{name}: a row other than {r} is nonzero"
            assert (dl[r, :V] != 0).any(), f"{name}: row {r} is zero"
            P.within(dl[r:r + 1], d64, allow, f"{name} row {r} of {M}")
            if lse is not None:
                P.within(lse[r:r + 1], lse64, P.lse_allow(lse64), f"{name} lse row {r}")


@pytest.mark.parametrize("M,V,ld,k", P.XENT_LONG)
def test_xent_count_past_1024(M, V, ld, k):
    """k valid rows scattered over M > 1024: out[1] == float32(1) / float32(k) within 1 ulp, out[0]
    against the fp64 mean within 2^-20 |loss| + the lse allowance.
    Measured on an MI355X: |loss - fp64| at most 0.0085 of the tolerance, 1 / n_valid equal."""
    logits = P.xent_long_logits(M, V, ld).to(DEV)
    g = torch.Generator().manual_seed(M)
    rows = torch.randperm(M, generator=g)[:k]
    assert int((rows >= 1024).sum()) > 0
    tgt = torch.full((M,), -1, dtype=torch.int64)
    tgt[rows] = torch.randint(0, V, (k,), generator=g)
    tgt = tgt.to(DEV)
    lse64 = P.xent_lse64(logits, V)
    valid = tgt >= 0
    picked = logits.double()[torch.arange(M, device=DEV), tgt.clamp(min=0)]
    loss = float((lse64 - picked)[valid].sum()) / k
    tol = 2.0 ** -20 * abs(loss) + float(P.lse_allow(lse64[valid]).max())
    want = np.float32(1) / np.float32(k)
    for name, out, _, _ in _both_paths(logits, tgt, V, 1.0):
        assert abs(out[1].item() - float(want)) <= _ulp32(want), (name, out, want)
        print(f"{name} M {M}: |loss - fp64| / tolerance {abs(out[0].item() - loss) / tol:.3g}")
        assert abs(out[0].item() - loss) <= tol, (name, out, loss)


def test_xent_scale_exact():
    """xent_scale_ on the fused dlogits of M = 1030 rows of 24584: 3.2 M vectors on a grid capped at 2048
    blocks x 256 lanes, seven trips of the loop.  gs = 0.5 gives the bits of bf16(float(dl) x 0.5)
    (halving is exact), gs = 1 leaves every byte unchanged."""
    C = ext()
    M, V, ld, k = P.XENT_LONG[1]
    assert 2048 * 256 * 8 < M * ld
    logits = P.xent_long_logits(M, V, ld).to(DEV)
    tgt = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(5)).to(DEV)
    tgt[::5] = -1
    _, dl = C.xent_fused(logits, tgt, V)
    assert (dl != 0).any()
    half = dl.clone()
    C.xent_scale_(half, torch.tensor([0.5], device=DEV))
    assert bit_equal(half, (dl.float() * 0.5).to(BF)), "gs = 0.5"
    same = dl.clone()
    C.xent_scale_(same, torch.tensor([1.0], device=DEV))
    assert bit_equal(same, dl), "gs = 1"
