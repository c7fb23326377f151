"""The probes of tests/_row_probe.py, checked on the CPU.

* Every integer expectation is reproduced bit for bit by an fp32 accumulation that starts from the
  accumulator's initial value and adds the rows in a shuffled order: exactness is a property of the
  data, not of an order.  The magnitude bounds behind that are asserted for the largest row counts
  the GPU tests use.
* A plain fp32 torch evaluation of each toleranced formula, rounded to bf16, stays inside the
  allowance with margin (at most 0.6 of it: the bf16 rounding alone is 0.5), so an allowance cannot
  quietly be widened later.
* The share of cross-entropy gradient elements below the absolute tolerance of the assert_close
  tests: why those tests could not see the softmax half of the gradient.
* Sensitivity: a row dropped from a census, or one 8-column vector of a softmax row zeroed, fails the
  comparison helpers the GPU tests use."""
import pytest
import torch

import _row_probe as P

F32 = torch.float32


def _acc_fp32(init, terms, seed=0):
    """init + the rows of terms [R, ...], added one at a time in fp32 in a shuffled order."""
    acc = init.to(F32).clone()
    for i in torch.randperm(terms.shape[0], generator=torch.Generator().manual_seed(seed)).tolist():
        acc += terms[i]
    return acc


# --------------------------------------------------------------------------- magnitudes
def test_census_magnitudes():
    """The largest sums the GPU tests form, in the unit of their terms, stay below 2^24: LayerNorm dw
    in halves over 32 x 2048 + 45 rows (the capped grid of at most 8 blocks on each of 256 CUs), the
    dropout column sums, the bias gradients over 32773 rows, the embedding over 4 x 64 tokens."""
    rows = 32 * 2048 + 45
    assert rows > P.LN_ROWS_MAX
    assert 2 * 40 * rows + 2 * 9 < 2 ** 24       # dw: |dy xhat| <= 40, multiples of 0.5
    assert 4 * rows + 9 < 2 ** 24                # db
    assert 16 * rows + 9 < 2 ** 24               # dzb: |2 dres| <= 16
    assert 8 * P.BIAS_HALVING[0] + 9 < 2 ** 24   # dropout_bias_grad: |2 dy| <= 8
    assert 8 * 4 * 64 + 9 < 2 ** 24              # embedding: |2 dout| <= 8
    c = P.ln_case(37, 520)
    xh2 = P.ln_xhat2(c)
    assert int(xh2.abs().max()) <= 20 and int((c["dy"].int() * xh2).abs().max()) <= 80
    for k in ("dw0", "db0", "dzb0"):
        assert (c[k] != 0).all()
    assert set(c["rstd2"].tolist()) == {1, 2, 4} and set(c["mean"].tolist()) == {-1, 0, 1, 2}


# --------------------------------------------------------------------------- census, any order
@pytest.mark.parametrize("M,D", [(37, 48), (37, 2056), (P.LN_M_CHUNK, 520)])
def test_ln_census_any_order(M, D):
    c = P.ln_case(M, D)
    dw, db = P.ln_census(c)
    xhat = P.ln_xhat2(c).to(F32) / 2
    dy = c["dy"].to(F32)
    P.exact(_acc_fp32(c["dw0"], dy * xhat, 1), dw, "dw")
    P.exact(_acc_fp32(c["db0"], dy, 2), db, "db")
    keep = P.keep_mask(M, D)
    dz, dzb = P.ln_dz(c, keep)
    z = torch.where(keep, c["dres"].to(F32) * 2.0, torch.zeros(()))
    P.exact(z.to(P.BF), dz, "dz")  # exact in bf16
    P.exact(_acc_fp32(c["dzb0"], z, 3), dzb, "dzb")
    # sensitivity: one row lost, one row counted twice, the initial value overwritten
    with pytest.raises(AssertionError):
        P.exact(_acc_fp32(c["dw0"], (dy * xhat)[:-1], 1), dw, "dw without its last row")
    with pytest.raises(AssertionError):
        P.exact(_acc_fp32(c["db0"], torch.cat([dy, dy[:1]]), 2), db, "db with row 0 twice")
    with pytest.raises(AssertionError):
        P.exact(_acc_fp32(torch.zeros(D), z, 3), dzb, "dzb overwritten")


@pytest.mark.parametrize("M,N", [(130, 520), (4099, 24)])
def test_bias_census_any_order(M, N):
    c = P.bias_case(M, N)
    dy = c["dy"].to(F32)
    P.exact(_acc_fp32(c["db0"], dy, 4), P.bias_census(c), "db")
    keep = P.keep_mask(M, N)
    dx, db = P.bias_census(c, keep)
    g = torch.where(keep, dy * 2.0, torch.zeros(()))
    P.exact(g.to(P.BF), dx, "dx")
    P.exact(_acc_fp32(c["db0"], g, 5), db, "dropout db")
    with pytest.raises(AssertionError):
        P.exact(_acc_fp32(c["db0"], dy[1:], 4), P.bias_census(c), "db without row 0")


@pytest.mark.parametrize("B,T", P.EMB_BT)
def test_embedding_census_any_order(B, T):
    D = 520
    c = P.emb_case(B, T, D)
    assert set(c["idx"].unique().tolist()) <= set(P.EMB_TOKENS) and (c["dwte0"] != 0).all() and (c["dwpe0"] != 0).all()
    for keep in (None, P.keep_mask(B * T, D)):
        out = P.emb_fwd_expected(c, keep)
        assert int(out.abs().max()) <= 128
        P.exact(P.bf(out), out, "forward is exact in bf16")
        dwte, dwpe = P.emb_bwd_expected(c, keep)
        g = c["dout"].to(F32).view(B * T, D)
        if keep is not None:
            g = torch.where(keep, g * 2.0, torch.zeros(()))
        aw, ap = c["dwte0"].to(F32).clone(), c["dwpe0"].to(F32).clone()
        for m in torch.randperm(B * T, generator=torch.Generator().manual_seed(6)).tolist():
            aw[c["idx"].view(-1)[m]] += g[m]
            ap[m % T] += g[m]
        P.exact(aw, dwte, "dwte")
        P.exact(ap, dwpe, "dwpe")
        unused = [v for v in range(P.EMB_V) if v not in P.EMB_TOKENS]
        assert len(unused) == 6 and torch.equal(dwte[unused], c["dwte0"].long()[unused])
        assert torch.equal(dwpe[T:], c["dwpe0"].long()[T:])


def test_elementwise_integers_fit_bf16():
    """|x + b|, |r + x + b| and |r + 2 (x + b)| stay at or below 128: exact in bf16."""
    for M, N in P.ELT_SHAPES:
        c = P.elt_case(M, N)
        xb = c["x"].int() + c["b"].int()
        for v in (xb, c["r"].int() + xb, c["r"].int() + 2 * xb):
            assert int(v.abs().max()) <= 128
            P.exact(P.bf(v), v, "bf16")


# --------------------------------------------------------------------------- allowances against fp32
@pytest.mark.parametrize("D", P.LN_D)
def test_ln_dx_allowance_holds_fp32(D):
    """Plain fp32, rounded to bf16: at most 0.6 of the allowance (measured 0.5: the rounding)."""
    for M in (12, 37):
        c = P.ln_case(M, D)
        for with_dres in (False, True):
            ref, allow = P.ln_dx_ref(c, with_dres)
            assert P.within(P.ln_dx_fp32(c, with_dres), ref, allow, f"dx fp32 ({M}, {D}) dres {with_dres}") <= 0.6


def test_ln_dx_sensitivity():
    """One row's dx replaced by its neighbour's, or one element off by two bf16 ulps, is outside."""
    c = P.ln_case(12, 768)
    ref, allow = P.ln_dx_ref(c, True)
    got = P.ln_dx_fp32(c, True)
    swapped = got.clone()
    swapped[3] = got[7]
    with pytest.raises(AssertionError):
        P.within(swapped, ref, allow, "rows 3 <- 7")
    i = int(ref[5].abs().argmax())
    off = got.clone()
    off[5, i] = (ref[5, i] * (1 + 2 * P.BF_ULP)).to(P.BF)
    with pytest.raises(AssertionError):
        P.within(off, ref, allow, "two ulps")


@pytest.mark.parametrize("M,D", [(64, 48), (33, 192), (257, 1600), (31, 2048)])
def test_ln_fwd_allowance_holds_fp32(M, D):
    c = P.ln_fwd_case(M, D)
    ref, allow = P.ln_fwd_ref(c)
    x, w, b = (c[k].float() for k in ("x", "w", "b"))
    mu = x.mean(1, keepdim=True)
    rs = ((x - mu) ** 2).mean(1, keepdim=True).add(1e-5).rsqrt()
    assert P.within(((x - mu) * rs * w + b).to(P.BF), ref, allow, f"y fp32 ({M}, {D})") <= 0.6


def test_ln_fwd_allowance_is_for_centred_rows():
    """The forward allowance has no term for the fp32 error of the mean: on rows with mean 30 and
    standard deviation 0.5 (the second data set of test_layernorm_rstd) a plain two-pass fp32
    evaluation leaves it where xhat w + b cancels (measured 131x at (1000, 768)), so the GPU test
    holds the kernel to it on the centred rows only."""
    c = P.ln_fwd_case(1000, 768, shifted=True)
    ref, allow = P.ln_fwd_ref(c)
    x, w, b = (c[k].float() for k in ("x", "w", "b"))
    mu = x.mean(1, keepdim=True)
    rs = ((x - mu) ** 2).mean(1, keepdim=True).add(1e-5).rsqrt()
    with pytest.raises(AssertionError):
        P.within(((x - mu) * rs * w + b).to(P.BF), ref, allow, "y fp32, mean 30")


def test_gelu_bwd_allowance_holds_fp32():
    c = P.elt_case(*P.ELT_SHAPES[0])
    big = {"gdy": P.randn_bf16(256, 3072, seed=1), "pre": P.randn_bf16(256, 3072, scale=2.0, seed=2)}
    for case in (c, big):
        ref, allow = P.gelu_bwd_ref(case)
        assert P.within(P.gelu_bwd_fp32(case), ref, allow, "gelu_bwd fp32") <= 0.6


def test_gelu_error_model():
    """The allowance 2^-7 |ref| + |dy| 2^-18 leaves 2^-8 |GELU'| + 2^-18 (per unit of |dy|) beside the bf16
    rounding; the error model of the kernel's sigmoid form (_row_probe.gelu_error_model: 1 ulp for
    exp2 and for rcp) stays inside it for every finite bf16 x."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(P.BF).double()
    x = x[torch.isfinite(x) & (x.abs() <= 2.0 ** 20)]
    err, grad = P.gelu_error_model(x)
    room = 2.0 ** -8 * grad + 2.0 ** -18
    worst = float((err / room).max())
    print(f"gelu error model: worst bound / room {worst:.3g} at x = {float(x[(err / room).argmax()]):.4g}; "
          f"worst absolute {float(err.max()):.3g}")
    assert torch.isfinite(err).all() and worst <= 0.05  # measured 0.022, at the zero crossing x = -0.754


@pytest.mark.parametrize("shift", [0.0, 60.0])
@pytest.mark.parametrize("M,V,ld", P.XENT_SHAPES)
def test_xent_allowance_holds_fp32(M, V, ld, shift):
    """fp32 logsumexp and softmax, dlogits rounded to bf16: at most 0.6 of the dlogits allowance
    (measured at most 0.5), lse at least 4x inside its own; ignored rows and pad columns exactly 0."""
    c = P.xent_case(M, V, ld, shift)
    n_valid = int((c["tgt"] >= 0).sum())
    g = 2.0 / n_valid
    lse, d, allow, _ = P.xent_ref(c["logits"], c["tgt"], V, g)
    lse32, d32 = P.xent_fp32(c["logits"], c["tgt"], V, g)
    assert P.within(d32, d, allow, f"dlogits fp32 {(M, V, ld)} shift {shift}") <= 0.6
    assert P.within(lse32, lse, P.lse_allow(lse), f"lse fp32 {(M, V, ld)} shift {shift}") <= 0.25
    assert c["tgt"][1] == V - 1 and c["tgt"][0] == -1 and c["logits"][2, c["tgt"][2]] == c["logits"][2, :V].max()


@pytest.mark.parametrize("M,V,ld", P.XENT_SHAPES)
def test_old_tolerance_was_blind(M, V, ld):
    """The share of valid-row, valid-column dlogits elements with |ref| below the 2e-3 absolute
    tolerance of the assert_close tests (measured 0.872 at V = 65, >= 0.999 from V = 24577 on): such
    an element passes those tests whatever the kernel writes below the tolerance."""
    c = P.xent_case(M, V, ld)
    valid = c["tgt"] >= 0
    _, d, _, _ = P.xent_ref(c["logits"], c["tgt"], V, 2.0 / int(valid.sum()))
    share = float((d[valid][:, :V].abs() < P.OLD_ATOL).double().mean())
    print(f"{(M, V, ld)}: share of |dlogits| < {P.OLD_ATOL}: {share:.4f}")
    assert share > (0.99 if V >= 24577 else 0.85)


@pytest.mark.parametrize("M,V,ld", P.XENT_SHAPES)
def test_xent_zeroed_vector_is_seen(M, V, ld):
    """One 16-byte vector (8 columns) of a valid row zeroed -- a vector never written, or stale -- fails
    `within`.  The allowance's absolute term g 2^-20 hides a vector only if all 8 of its probabilities
    are below about 2^-20; with N(0, 3^2) logits an element is above that with probability >= 0.3, so
    at least 1 - 0.7^8 = 0.94 of the vectors are visible: asserted > 0.9 over every valid row."""
    c = P.xent_case(M, V, ld)
    valid = c["tgt"] >= 0
    g = 2.0 / int(valid.sum())
    _, d, allow, _ = P.xent_ref(c["logits"], c["tgt"], V, g)
    _, d32 = P.xent_fp32(c["logits"], c["tgt"], V, g)
    P.within(d32, d, allow, "intact")
    V8 = V // 8 * 8
    seen = (d[valid][:, :V8].abs() > allow[valid][:, :V8]).view(int(valid.sum()), V8 // 8, 8).any(-1)
    share = float(seen.double().mean())
    print(f"{(M, V, ld)}: share of 8-column vectors whose loss is seen: {share:.4f}")
    assert share > 0.9
    row = int(valid.nonzero()[-1])
    vec = int(seen[-1].nonzero()[len(seen[-1].nonzero()) // 2])  # a visible vector in the middle of the row
    broken = d32.clone()
    broken[row, 8 * vec: 8 * vec + 8] = 0
    with pytest.raises(AssertionError):
        P.within(broken, d, allow, "one vector zeroed")
    # the softmax half off by 2x: every non-target element doubles
    doubled = d32.clone()
    doubled[row, :V] = (d32[row, :V].float() * 2).to(P.BF)
    with pytest.raises(AssertionError):
        P.within(doubled, d, allow, "softmax doubled")


def test_lse_allowance_sees_a_missing_vector():
    """16 2^-24 max(|lse|, 1) is 1.4e-5 at lse = 15; a 16-byte vector left out of the sum moves lse by
    about 8 / 50257 = 1.6e-4 on average, 10x outside."""
    M, V, ld = P.XENT_SHAPES[1]
    c = P.xent_case(M, V, ld)
    lse = P.xent_lse64(c["logits"], V)
    cut = c["logits"][:, :V].double().clone()
    cut[:, 4096:4104] = -float("inf")
    with pytest.raises(AssertionError):
        P.within(torch.logsumexp(cut, 1), lse, P.lse_allow(lse), "lse without one vector")
