"""The rows GEMM (csrc/kernels/gemm_rows.hip): y[M, ldy] = epi(x[M, K] @ W[N, K]^T) at 1 <= M <= 64
rows on MFMA, through the binding.

* exact integers: small integer operands whose every partial sum is exact in fp32 and bf16, so a
  lost, doubled or misplaced k-chunk, fragment lane or split partial is an O(1) error;
* a one-hot probe: y[m, n] is W[n, k_m] bit for bit;
* random bf16 against fp64 inside a bound made of the number formats' precision;
* row independence: a row's bits do not depend on M, its slot or the other rows (NaN included);
* guard bands around x, W, bias and resid, and sentinel pad columns;
* graph replay equals eager launches; argument checks.

Inputs and references of a shape are computed once (lru_cache) and left unchanged."""
import functools
import math

import numpy as np
import pytest
import torch

from _guard import SENTINEL_BYTE, bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

INT_M = (1, 9, 16, 17, 33, 48, 64)
INT_K = (8, 48, 136, 1024, 4096, 5120, 8192)
INT_N = (1, 16, 40, 136)


def _int_x(K, rows=64, seed=0):
    """[rows, K] with 8 entries of +-1 per row.  Row m: one in the last 8 columns, K - 8 + m % 8; the
    i-th of the others at a random column congruent to (7 m + i) mod 64 where K has one (over 64 rows
    every residue 7 times), else anywhere; repeats inside a row are redrawn."""
    rng = np.random.default_rng(1000 + K + seed)
    x = np.zeros((rows, K), dtype=np.float32)
    for m in range(rows):
        cols = [K - 8 + m % 8]
        for i in range(7):
            base = (7 * m + i) % 64
            c = base + 64 * int(rng.integers(0, (K - base + 63) // 64)) if base < K else int(rng.integers(0, K))
            while c in cols:
                c = int(rng.integers(0, K))
            cols.append(c)
        x[m, cols] = rng.choice([-1.0, 1.0], size=8)
    return x


def test_integer_probe_covers_every_k_position():
    """Over the M = 64 cases the nonzeros hit every k modulo 64 and each of the last 8 columns."""
    for K in INT_K:
        nz = np.argwhere(_int_x(K) != 0)
        assert (np.bincount(nz[:, 0], minlength=64) == 8).all()
        assert set(range(K - 8, K)) <= set(nz[:, 1].tolist())
        if K >= 128:
            assert set((nz[:, 1] % 64).tolist()) == set(range(64))


@functools.lru_cache(maxsize=None)
def _int_case(K, N=136, M=64, ldy=0):
    ldy = ldy or N
    rng = np.random.default_rng(K + N)
    x = _int_x(K, M)
    w = rng.integers(-4, 5, size=(N, K)).astype(np.float32)
    bias = rng.integers(-8, 9, size=N).astype(np.float32)
    resid = rng.integers(-8, 9, size=(M, ldy)).astype(np.float32)
    prod = x.astype(np.float64) @ w.astype(np.float64).T
    t = lambda a: torch.from_numpy(a).to(BF).to(DEV)
    return {"x": t(x), "w": t(w), "bias": t(bias), "resid": t(resid), "prod": prod, "bias_np": bias, "resid_np": resid}


def _int_check(c, M, N, ldy=0):
    C = ext()
    ldy = ldy or N
    x, w, bias = c["x"][:M].contiguous(), c["w"][:N].contiguous(), c["bias"][:N].contiguous()
    resid = c["resid"][:M, :ldy].contiguous()
    for epi in (0, 1, 3):
        y = C.gemm_rows(x, w, epi, bias if epi else None, resid if epi == 3 else None, ldy)
        assert y.shape == (M, ldy) and y.dtype == BF
        want = c["prod"][:M, :N].copy()
        if epi:
            want += c["bias_np"][:N]
        if epi == 3:
            want += c["resid_np"][:M, :N]
        assert np.abs(want).max() <= 48
        got = y[:, :N].float().cpu().numpy().astype(np.float64)
        bad = got != want
        assert not bad.any(), (f"M {M} N {N} K {x.shape[1]} epi {epi}: {int(bad.sum())} of {bad.size} wrong, first at "
                               f"(row, column) {tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {want[bad][0]}")


@pytest.mark.parametrize("K", INT_K)
def test_exact_integers(K):
    """Every element equals the integer result, at every (M, N) of the grid and epilogues 0, 1, 3."""
    c = _int_case(K)
    for M in INT_M:
        for N in INT_N:
            _int_check(c, M, N)


def test_exact_integers_wide_padded():
    """N = 9000 columns in rows of ldy = 9008: 563 column tiles, the last one half full."""
    _int_check(_int_case(128, N=9000, M=33, ldy=9008), 33, 9000, ldy=9008)


@pytest.mark.parametrize("K", [48, 6400])
def test_one_hot_probe(K):
    """x row m is 1.0 at column (37 m + 5) % K: y[m, n] is W[n, k_m], bit for bit."""
    C = ext()
    M, N = 64, 200
    g = torch.Generator(device="cpu").manual_seed(K)
    w = torch.randn(N, K, generator=g).to(BF).to(DEV)
    km = torch.tensor([(37 * m + 5) % K for m in range(M)], device=DEV)
    x = torch.zeros(M, K, dtype=BF, device=DEV)
    x[torch.arange(M, device=DEV), km] = 1.0
    y = C.gemm_rows(x, w, 0, None, None, 0)
    assert bit_equal(y, w[:, km].t().contiguous())


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _gelu64(v):
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


@functools.lru_cache(maxsize=None)
def _rand_case(M, N, K):
    x, w = _bf(M, K, seed=K + M), _bf(N, K, scale=0.05, seed=K + N + 1)
    bias, resid = _bf(N, seed=K + 2), _bf(M, N, seed=K + 3)
    x64, w64 = x.double().numpy(), w.double().numpy()
    return {"x": x.to(DEV), "w": w.to(DEV), "bias": bias.to(DEV), "resid": resid.to(DEV),
            "prod": x64 @ w64.T, "abs": np.abs(x64) @ np.abs(w64).T,
            "bias64": bias.double().numpy(), "resid64": resid.double().numpy()}


@pytest.mark.parametrize("M,N,K", [(9, 384, 128), (33, 2304, 768), (64, 1600, 6400), (16, 1000, 1600)],
                         ids=lambda v: str(v))
def test_random_against_fp64(M, N, K):
    """|got - ref| <= 1.13 (2^-8 |ref| + 2 K 2^-24 S), S = sum_k |x_k w_k| + |bias| + |resid|: one bf16
    rounding (2^-9 relative, doubled), any-order fp32 accumulation (K 2^-24 S, doubled), and the
    largest |GELU'| (below 1.13) on the way through epilogue 2."""
    C, c = ext(), _rand_case(M, N, K)
    for epi in (0, 1, 2, 3):
        y = C.gemm_rows(c["x"], c["w"], epi, c["bias"] if epi else None, c["resid"] if epi == 3 else None, N)
        assert y.shape == (M, N)
        ref, S = c["prod"].copy(), c["abs"].copy()
        if epi:
            ref += c["bias64"]
            S += np.abs(c["bias64"])
        if epi == 2:
            ref = _gelu64(ref)
        if epi == 3:
            ref += c["resid64"]
            S += np.abs(c["resid64"])
        allow = 1.13 * (2.0 ** -8 * np.abs(ref) + 2 * K * 2.0 ** -24 * S)
        err = np.abs(y.double().cpu().numpy() - ref)
        print(f"({M}, {N}, {K}) epilogue {epi}: worst error / allowance {float((err / allow).max()):.3f}")
        assert (err <= allow).all(), f"epilogue {epi}: {int((err > allow).sum())} elements outside the allowance"


@pytest.mark.parametrize("K", [768, 5120])
def test_rows_are_independent(K):
    """The same 5 rows at slots 0..4 of M = 9 and at slots 59..63 of M = 64, among random rows and
    among NaN rows: their outputs are bit-equal in all four runs."""
    C = ext()
    N = 72
    w, bias = _bf(N, K, scale=0.05, seed=1).to(DEV), _bf(N, seed=2).to(DEV)
    rows, rres = _bf(5, K, seed=3).to(DEV), _bf(5, N, seed=4).to(DEV)
    for epi in (0, 3):
        outs = []
        for M, at in ((9, 0), (64, 59)):
            for fill in ("random", "nan"):
                if fill == "random":
                    x, resid = _bf(M, K, seed=5 + M).to(DEV), _bf(M, N, seed=6 + M).to(DEV)
                else:
                    x = torch.full((M, K), float("nan"), dtype=BF, device=DEV)
                    resid = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
                x[at:at + 5], resid[at:at + 5] = rows, rres
                y = C.gemm_rows(x, w, epi, bias if epi else None, resid if epi == 3 else None, 0)
                assert torch.isfinite(y[at:at + 5]).all()
                outs.append(((M, fill), y[at:at + 5].clone()))
        for tag, o in outs[1:]:
            assert bit_equal(o, outs[0][1]), f"epilogue {epi}: the rows at {tag} differ from those at {outs[0][0]}"


@pytest.mark.parametrize("epi,M,N,K,ld", [(0, 17, 136, 48, 136), (1, 64, 1, 8, 8), (2, 33, 16, 8192, 16),
                                          (3, 9, 23, 136, 24), (3, 64, 40, 5120, 48)])
def test_guard_bands_and_padding(epi, M, N, K, ld):
    """NaN margins around x, W, the bias and the residual, whose pad columns N..ld-1 hold the
    sentinel: columns 0..N-1 are finite and equal the plain run, and no margin byte changes."""
    C = ext()
    x, w = _bf(M, K, seed=31).to(DEV), _bf(N, K, scale=0.05, seed=32).to(DEV)
    b, r = _bf(N, seed=33).to(DEV), _bf(M, ld, seed=34).to(DEV)
    if ld > N:
        pad = torch.empty(M, ld - N, dtype=BF, device=DEV)
        pad.view(torch.uint8).fill_(SENTINEL_BYTE)
        r[:, N:] = pad
    if epi == 0:
        guarded(lambda x, W: C.gemm_rows(x, W, 0, None, None, ld)[:, :N], {"x": x, "W": w}, name="gemm_rows epi 0")
    elif epi == 3:
        guarded(lambda x, W, bias, resid: C.gemm_rows(x, W, 3, bias, resid, ld)[:, :N],
                {"x": x, "W": w, "bias": b, "resid": r}, name="gemm_rows epi 3")
    else:
        guarded(lambda x, W, bias: C.gemm_rows(x, W, epi, bias, None, ld)[:, :N], {"x": x, "W": w, "bias": b},
                name=f"gemm_rows epi {epi}")


def test_pad_columns_are_left_untouched():
    """ldy = 24 > N = 23: y is allocated on a block just filled with the sentinel and freed (the
    caching allocator hands the same block back; asserted), and its pad column keeps it."""
    C = ext()
    M, N, K, ld = 33, 23, 136, 24
    x, w = _bf(M, K, seed=41).to(DEV), _bf(N, K, scale=0.05, seed=42).to(DEV)
    want = C.gemm_rows(x, w, 0, None, None, N)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    block = torch.empty(M, ld, dtype=BF, device=DEV)
    block.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    ptr = block.data_ptr()
    del block
    y = C.gemm_rows(x, w, 0, None, None, ld)
    assert y.shape == (M, ld) and y.data_ptr() == ptr, "y did not land on the sentinel block: nothing was checked"
    assert bit_equal(y[:, :N], want)
    assert (y[:, N:].contiguous().view(-1).view(torch.uint8) == SENTINEL_BYTE).all(), "a pad column was written"


def test_graph_equals_eager():
    """Three chained calls captured once and replayed twice give the eager calls' bits."""
    from mingpt_distributed_amd.models.generation import _capture

    C = ext()
    M, D = 33, 256
    x = _bf(M, D, seed=51).to(DEV)
    w1, b1 = _bf(4 * D, D, scale=0.05, seed=52).to(DEV), _bf(4 * D, seed=53).to(DEV)
    w2, b2 = _bf(D, 4 * D, scale=0.05, seed=54).to(DEV), _bf(D, seed=55).to(DEV)
    w3 = _bf(1001, D, scale=0.05, seed=56).to(DEV)

    def chain():
        u = C.gemm_rows(x, w1, 2, b1, None, 0)
        h = C.gemm_rows(u, w2, 3, b2, x, 0)
        return C.gemm_rows(h, w3, 0, None, None, 1008)[:, :1001]

    eager = chain().clone()
    assert torch.isfinite(eager).all()
    graph, out = _capture(chain)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert bit_equal(out, eager)
    assert bit_equal(chain(), eager)


def test_refusals():
    C = ext()
    z = lambda *s, dt=BF: torch.zeros(*s, dtype=dt, device=DEV)
    err = (ValueError, RuntimeError)
    with pytest.raises(err):  # M = 65
        C.gemm_rows(z(65, 8), z(16, 8), 0, None, None, 0)
    with pytest.raises(err):  # K = 8200
        C.gemm_rows(z(9, 8200), z(16, 8200), 0, None, None, 0)
    with pytest.raises(err):  # K % 8 != 0
        C.gemm_rows(z(9, 12), z(16, 12), 0, None, None, 0)
    with pytest.raises(err):  # dtypes
        C.gemm_rows(z(9, 16, dt=torch.float32), z(16, 16), 0, None, None, 0)
    with pytest.raises(err):
        C.gemm_rows(z(9, 16), z(16, 16, dt=torch.float16), 0, None, None, 0)
    with pytest.raises(err):  # resid of the wrong shape: [M, N] where [M, ldy] is needed
        C.gemm_rows(z(9, 16), z(16, 16), 3, z(16), z(9, 16), 24)
    with pytest.raises(err):  # ldy < N
        C.gemm_rows(z(9, 16), z(16, 16), 0, None, None, 8)
    assert C.gemm_rows(z(9, 16), z(16, 16), 3, z(16), z(9, 24), 24).shape == (9, 24)


def test_gemm_rows_supported():
    C = ext()
    assert C.gemm_rows_supported(64, 8192) and C.gemm_rows_supported(1, 8)
    assert not C.gemm_rows_supported(65, 8) and not C.gemm_rows_supported(9, 8196)
    assert not C.gemm_rows_supported(0, 8) and not C.gemm_rows_supported(9, 8200)
