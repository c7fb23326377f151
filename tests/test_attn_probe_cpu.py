"""The evidence that tests/test_attention_probe_gpu.py has teeth, checked without a GPU.

On the probe inputs of tests/_attn_probe.py an fp64 reference with one fault built in (a key column
lost past its block, the last key lost, a key counted twice, ...) must miss the unmutated fp64
reference by a wide multiple of the tolerances the GPU file applies to the kernels: a kernel with
that fault cannot pass.  The last test keeps the motivation executable: on ``randn`` inputs the same
faults stay inside the tolerances of test_attention_fwd_bwd."""
import functools

import pytest
import torch

import _attn_probe as P

SHAPE_IDS = [f"T{T}-hd{hd}" for _, T, _, hd in P.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(B, T, H, hd):
    qkv, a, b = P.probe_qkv(B, T, H, hd, seed=hd + T)
    dout = torch.randn(B * T, H * hd, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16)
    return qkv, a, b, dout, P.ref64(qkv, dout, B, T, H)


def test_targets_are_causal_and_spread():
    for T in sorted({s[1] for s in P.SHAPES}):
        a, b = P.probe_targets(T)
        i = torch.arange(T)
        assert torch.equal(a, i) and (b <= i).all() and (b[1:] < i[1:]).all()
        assert torch.bincount(b[1:], minlength=T).max() <= P.FAN_IN
        # the keys on both sides of the 64 / 128 / 256 boundaries are second targets of later rows
        for edge in (64, 128, 256, 512):
            for key in (edge - 1, edge):
                if key + 64 < T:
                    assert (b == key).any(), (T, key)
        # the last row's second key is far back, or the last of the tile before a one-row tail
        assert b[T - 1] == (T - 2 if T % 64 == 1 else (T - 1) // 3)


@pytest.mark.parametrize("B,T,H,hd", [s for s in P.SHAPES if s[3] >= 32],
                         ids=[i for i, s in zip(SHAPE_IDS, P.SHAPES) if s[3] >= 32])
def test_mass_on_both_targets(B, T, H, hd):
    """At least 95 % of the rows with two distinct targets carry fp64 softmax mass >= 0.25 on each."""
    qkv, a, b, _, _ = _case(B, T, H, hd)
    ma, mb = P.target_mass(qkv, a, b, B, T, H)
    two = (a != b).expand_as(ma)
    ok = ((ma >= 0.25) & (mb >= 0.25))[two].double().mean().item()
    print(f"T={T} hd={hd}: {ok:.4f} of rows >= 0.25 on both, median {ma[two].median().item():.3f}")
    assert ok >= 0.95


@pytest.mark.parametrize("B,T,H,hd", P.SHAPES, ids=SHAPE_IDS)
def test_mutants_are_caught(B, T, H, hd):
    """Every mutant misses the reference by >= 10x the forward tolerance and >= 3x the backward
    one.  hd < 32 (random keys in so few dimensions cannot be separated as cleanly): asserted for
    the column-wide mutants, the others printed."""
    qkv, _, _, dout, (out, _, dqkv) = _case(B, T, H, hd)
    for name, kw in P.mutants(T).items():
        m_out, _, m_dqkv = P.ref64(qkv, dout, B, T, H, **kw)
        vo, vg = P.violation(m_out, out, **P.OUT_TOL), P.bwd_violation(m_dqkv, dqkv)
        print(f"T={T} hd={hd} {name}: out {vo:.1f} dqkv {vg:.1f}")
        if hd >= 32 or name in P.COLUMN_WIDE:
            assert vo >= 10 and vg >= 3, (name, vo, vg)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,H,hd", P.SHAPES, ids=SHAPE_IDS)
def test_rounding_alone_is_inside_the_tolerances(B, T, H, hd, p):
    """The kernels' rounding points in fp32 torch (``emulate``) stay inside the tolerances on the
    probe inputs, so the GPU file can keep the project's own bounds: what it fails on is a fault.
    (With randn keys and gains of 4 to 6 instead of _sign_keys the same emulation reaches 2.0 for
    out and 1.8 for dqkv, and the kernels gave the same figures.)"""
    qkv, _, _, dout, ref = _case(B, T, H, hd)
    keep = None
    if p:
        keep = (torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(5)) >= p).float()
        ref = P.ref64(qkv, dout, B, T, H, keep, P.dropout_scale(p))
    out, lse, dqkv = P.emulate(qkv, dout, B, T, H, keep, P.dropout_scale(p))
    vo, vl = P.violation(out, ref[0], **P.OUT_TOL), P.violation(lse, ref[1], **P.LSE_TOL)
    vg = P.bwd_violation(dqkv, ref[2])
    print(f"T={T} hd={hd} p={p}: emulated out {vo:.3f} lse {vl:.3f} dqkv {vg:.3f}")
    assert vo <= 1 and vl <= 1 and vg <= 1, (vo, vl, vg)


def test_randn_inputs_hide_the_last_key():
    """Why the probes exist: with Gaussian inputs at T = 777, hd = 64 a kernel that loses the last
    key column, or the last row's diagonal, is inside test_attention_fwd_bwd's tolerances."""
    B, T, H, hd = 1, 777, 2, 64
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * T, 3 * H * hd, generator=g).to(torch.bfloat16)
    dout = torch.randn(B * T, H * hd, generator=g).to(torch.bfloat16)
    out, _, dqkv = P.ref64(qkv, dout, B, T, H)
    atol = P.BWD_ATOL * max(1.0, dqkv.abs().max().item() / 4)  # one |g|max, as that test takes it
    muts = P.mutants(T)
    for name in ("last_col_dropped", "last_row_no_diagonal"):
        m_out, _, m_dqkv = P.ref64(qkv, dout, B, T, H, **muts[name])
        assert P.violation(m_out, out, **P.OUT_TOL) < 1
        assert P.violation(m_dqkv, dqkv, atol, P.BWD_RTOL) < 1
