"""The training GEMM (csrc/kernels/gemm.hip) against references that can see a single product, under
every tile configuration, on the probes of tests/_gemm_probe.py (checked in test_gemm_probe_cpu.py):

* exact integers, NT / NN / TN, every epilogue that has an integer form (0, 1, 3 at p = 0, 4, 7) and
  the fused dbias column sums: every value is an integer below 256, exact in bf16 and fp32 in any
  accumulation or atomic order, so a lost, doubled or misplaced k-chunk, fragment lane, split
  partial or dbias row is an O(1) error and the comparison has no tolerance (integers are compared
  by value: the sign of a zero, e.g. -5 x 0, is the only bit that may differ);
* TN reduction lengths that force 1, 2 and 7 splits (derivation at test_int_tn);
* the fragment-ordered plane (epilogues 6 / 7) against a plane written by the test in the
  documented order, not against epilogues 2 / 4 of the same kernel;
* one-hot probes, bit for bit, in all three layouts;
* random bf16 against fp64 inside the allowance of test_gemm_rows_gpu.py::test_random_against_fp64;
* row and column independence: a NaN row of A or B changes no bit of any other row or column.

Shapes are the smallest that reach every tile edge (tests/_gemm_probe.py SHAPES); inputs and
references of a shape are computed once (lru_cache) and left unchanged."""
import functools

import numpy as np
import pytest
import torch

import _gemm_probe as P
from _guard import SENTINEL_BYTE, bit_equal
from mingpt_distributed_amd.ops import gemm as G
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
IDS = [f"{m}x{n}x{k}" for m, n, k in P.SHAPES]
RAND_SHAPES = [(300, 264, 776), (130, 200, 328)]


@pytest.fixture(autouse=True, params=[0, 1, 5, 6], ids=["auto", "t128", "w4", "w4n192"])
def tile_config(request):
    """Run every GEMM test under each tile configuration of gemm.hip (0 = per-shape choice)."""
    ext().gemm_set_variant(request.param)
    yield request.param
    ext().gemm_set_variant(0)


def _exact(got, want, what):
    """Every element of the tensor equals the integer reference."""
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} for {want.shape}"
    bad = got != want  # NaN != anything: counted
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} wrong, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][0]} for {want[bad][0]}")


def _sent(*shape, dtype=BF):
    t = torch.empty(*shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    return t


def _untouched(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == SENTINEL_BYTE).all())


@functools.lru_cache(maxsize=None)
def _int_dev(M, N, K):
    c = P.int_case(M, N, K)
    d = {k: P.bf(c[k]).to(DEV) for k in ("a", "b_nk", "b_kn", "bias", "resid", "aux")}
    d["dbias0"] = torch.from_numpy(c["dbias0"].astype(np.float32)).to(DEV)
    return d


def _dbias_want(c, want):
    return c["dbias0"] + want.sum(0)


# ------------------------------------------------------------------------------ a. integers, NT
@pytest.mark.parametrize("M,N,K", P.SHAPES, ids=IDS)
def test_int_nt(M, N, K):
    """Epilogues 0, 1, 3 (p = 0) and 4 (row-major aux; without and with dbias; directly and as
    gemm_dgrad's NT against a transposed copy): every element equals the int64 reference, and dbias
    equals its nonzero initial value plus the exact column sums."""
    c, d = P.int_case(M, N, K), _int_dev(M, N, K)
    a, b = d["a"], d["b_nk"]
    _exact(G.gemm_nt(a, b), P.int_expected(c, 0), "NT epilogue 0")
    _exact(G.gemm_nt(a, b, bias=d["bias"], epi="bias"), P.int_expected(c, 1), "NT epilogue 1")
    _exact(G.gemm_nt(a, b, bias=d["bias"], epi="resid", resid=d["resid"], p=0.0), P.int_expected(c, 3),
           "NT epilogue 3")
    want = P.int_expected(c, 4)
    _exact(G.gemm_nt(a, b, epi="gelu_bwd", aux=d["aux"]), want, "NT epilogue 4")
    db = d["dbias0"].clone()
    _exact(G.gemm_nt(a, b, epi="gelu_bwd", aux=d["aux"], dbias=db), want, "NT epilogue 4 + dbias")
    _exact(db, _dbias_want(c, want), "NT epilogue 4 dbias")
    wt = G.transpose(d["b_kn"], K)
    assert bit_equal(wt, b)
    db = d["dbias0"].clone()
    _exact(G.gemm_dgrad(a, d["b_kn"], epi="gelu_bwd", aux=d["aux"], wt=wt, dbias=db), want, "dgrad NT epilogue 4")
    _exact(db, _dbias_want(c, want), "dgrad NT dbias")
    _exact(G.gemm_dgrad(a, d["b_kn"], wt=wt), P.int_expected(c, 0), "dgrad NT epilogue 0")


@pytest.mark.parametrize("epi", [0, 1, 4])
@pytest.mark.parametrize("M,N,K", P.SHAPES, ids=IDS)
def test_int_nt_padded_row_stride(M, N, K, epi):
    """ld = N + 8 > N (N is a multiple of 8), c three rows taller than M, all on the sentinel: columns
    < N of rows < M are exact; rows >= M stay untouched; the pad columns of rows < M are exactly 0
    after epilogue 0 and untouched after every other one (the contract of
    test_guard_bands_gpu.py::test_gemm_nt_padded_row_stride).  aux's pad columns hold NaN."""
    c, d = P.int_case(M, N, K), _int_dev(M, N, K)
    ld = (N + 7) // 8 * 8 + 8
    out = _sent(M + 3, ld)
    aux = db = None
    if epi == 4:
        aux = torch.full((M + 3, ld), float("nan"), dtype=BF, device=DEV)
        aux[:M, :N] = d["aux"]
        db = d["dbias0"].clone()
    ext().gemm(d["a"], d["b_nk"], out, 0, epi, d["bias"] if epi == 1 else None, aux, None, 0.0, 0, M, N, db)
    want = P.int_expected(c, epi)
    _exact(out[:M, :N], want, f"NT epilogue {epi}, ld {ld}")
    assert _untouched(out[M:]), "rows >= M of c were written"
    if epi == 0:
        assert bit_equal(out[:M, N:], torch.zeros(M, ld - N, dtype=BF, device=DEV)), "pad columns are not +0"
    else:
        assert _untouched(out[:M, N:]), "a pad column was written"
    if epi == 4:
        _exact(db, _dbias_want(c, want), "dbias")


# ------------------------------------------------------------------------------ b. integers, NN
@pytest.mark.parametrize("M,N,K", P.SHAPES, ids=IDS)
def test_int_nn(M, N, K):
    """Epilogue 0, and 4 without and with dbias, from the [K, N] operand."""
    c, d = P.int_case(M, N, K), _int_dev(M, N, K)
    a, b = d["a"], d["b_kn"]
    _exact(G.gemm_nn(a, b), P.int_expected(c, 0), "NN epilogue 0")
    want = P.int_expected(c, 4)
    _exact(G.gemm_nn(a, b, epi="gelu_bwd", aux=d["aux"]), want, "NN epilogue 4")
    db = d["dbias0"].clone()
    _exact(G.gemm_nn(a, b, epi="gelu_bwd", aux=d["aux"], dbias=db), want, "NN epilogue 4 + dbias")
    _exact(db, _dbias_want(c, want), "NN epilogue 4 dbias")
    _exact(G.gemm_dgrad(a, b), P.int_expected(c, 0), "dgrad NN")  # the dispatcher's NN route


@pytest.mark.parametrize("M,N,K", P.SHAPES, ids=IDS)
def test_int_nn_short_b(M, N, K):
    """Kb = K - 7 rows of B (the padded reduction of the LM-head data gradient): A's columns >= Kb are
    zero, B's rows Kb..K-1 do not exist and read as zero."""
    c, d = P.int_case(M, N, K), _int_dev(M, N, K)
    Kb = K - 7
    a = d["a"].clone()
    a[:, Kb:] = 0
    b = d["b_kn"][:Kb].contiguous()
    prod = P.imatmul(c["a"][:, :Kb], c["b_kn"][:Kb])
    _exact(G.gemm_nn(a, b), prod, "NN epilogue 0, Kb < K")
    want = prod * c["aux"].astype(np.int64)
    db = d["dbias0"].clone()
    _exact(G.gemm_nn(a, b, epi="gelu_bwd", aux=d["aux"], dbias=db), want, "NN epilogue 4, Kb < K")
    _exact(db, _dbias_want(c, want), "NN epilogue 4 dbias, Kb < K")


# ------------------------------------------------------------------------------ c. integers, TN
@functools.lru_cache(maxsize=None)
def _tn_dev(Mr, N, K):
    c = P.tn_int_case(Mr, N, K)
    return {"a": P.bf(c["a"]).to(DEV), "b": P.bf(c["b"]).to(DEV),
            "c0": torch.from_numpy(c["c0"].astype(np.float32)).to(DEV)}


@pytest.mark.parametrize("Mr", P.TN_MR)
def test_int_tn(Mr):
    """c == c0 + A^T B for outputs [72, 776], [200, 72] and [264, 328].  Split counts, from
    choose_split / set_split (maxsp = min(32, nkt / 4); cost = rounds x (ceil(nkt / sp) + overhead), a
    further split only if it saves 5 %; every launch here is one round: at most 21 tiles x 8 splits
    on 512 slots (T128), 8 x 8 on 256 (W4)):
      Mr =  136, nkt =  3: maxsp 0 -> 1 split, both configurations;
      Mr =  520, nkt =  9: maxsp 2; W4 15 -> 11, T128 12 -> 8: 2 splits, kchunk 320: 320 + 200;
      Mr = 2056, nkt = 33: maxsp 8; W4 39, 23, 17, 15, 13, 12, 11, (11); T128 36, 20, 14, 12, 10, 9, 8,
                 (8): 7 splits, kchunk 5 x 64 = 320: 6 x 320 + 136.
    (auto picks T128 for these outputs, M N < 2^18; W4-192 has no TN form and runs W4-256.)  A lost,
    doubled or overlapping split is an integer error; _gemm_probe.tn_splits restates the rule and
    test_gemm_probe_cpu.py holds it to these counts."""
    for N, K in P.TN_OUT:
        c, d = P.tn_int_case(Mr, N, K), _tn_dev(Mr, N, K)
        out = d["c0"].clone()
        G.gemm_tn_acc(d["a"], d["b"], out)
        _exact(out, c["want"], f"TN Mr {Mr} -> [{N}, {K}]")


def test_int_tn_n_valid():
    """n_valid = 197 of N = 200 columns of A, two splits: rows >= 197 of c keep their bits."""
    Mr, N, K, nv = P.TN_NVALID
    c, d = P.tn_int_case(Mr, N, K), _tn_dev(Mr, N, K)
    out = d["c0"].clone()
    G.gemm_tn_acc(d["a"], d["b"], out, n_valid=nv)
    _exact(out[:nv], c["want"][:nv], "TN n_valid")
    assert bit_equal(out[nv:], d["c0"][nv:]), "rows >= n_valid of c were written"


# ------------------------------------------------------------------------------ d. fragment plane, integers
def test_int_fragment_plane():
    """Epilogue 7 (NN, W4-256 under every configuration) reads an aux plane this test wrote in the
    documented order (_gemm_probe.rowmajor_to_frag_plane, the inverse of frag_plane_rowmajor), at
    M = 300, N = 264: whole and partial 256^2 tiles.  Positions outside [M, N] hold 1.0: they meet
    zero accumulators only.  The result and dbias equal the int64 reference."""
    M, N, K = 300, 264, 776
    c, d = P.int_case(M, N, K), _int_dev(M, N, K)
    plane = P.rowmajor_to_frag_plane(d["aux"], pad=1.0)
    assert plane.numel() == G.frag_aux_elems(M, N) and bit_equal(G.frag_plane_rowmajor(plane, M, N), d["aux"])
    want = P.int_expected(c, 4)
    _exact(G.gemm_nn(d["a"], d["b_kn"], epi="gelu_bwd", aux=plane, aux_frag=True), want, "NN epilogue 7")
    db = d["dbias0"].clone()
    _exact(G.gemm_dgrad(d["a"], d["b_kn"], epi="gelu_bwd", aux=plane, dbias=db, aux_frag=True), want,
           "NN epilogue 7 + dbias")
    _exact(db, _dbias_want(c, want), "NN epilogue 7 dbias")


# ------------------------------------------------------------------------------ e. one-hot probes
@pytest.mark.parametrize("M,N,K", P.SHAPES, ids=IDS)
def test_one_hot_nt_nn(M, N, K):
    """NT, A one-hot: C[m, :] == B[:, k(m)].  NT, B one-hot: C[:, n] == A[:, k(n)].  NN, A one-hot:
    C[m, :] == B[k(m), :].  Bit for bit."""
    x, k = P.one_hot(M, K)
    x, k = x.to(DEV), k.to(DEV)
    b = P.wide_bf16(N, K).to(DEV)
    assert bit_equal(G.gemm_nt(x, b), b[:, k].t().contiguous()), "NT, A one-hot"
    xb, kb = P.one_hot(N, K)
    xb, kb = xb.to(DEV), kb.to(DEV)
    a = P.wide_bf16(M, K, seed=1).to(DEV)
    assert bit_equal(G.gemm_nt(a, xb), a[:, kb].contiguous()), "NT, B one-hot"
    bn = P.wide_bf16(K, N, seed=2).to(DEV)
    assert bit_equal(G.gemm_nn(x, bn), bn[k].contiguous()), "NN, A one-hot"


@pytest.mark.parametrize("Mr,N,K", [(mr,) + nk for mr, nk in zip(P.TN_MR, P.TN_OUT)], ids=lambda v: str(v))
def test_one_hot_tn(Mr, N, K):
    """A's column n is one-hot at row r(n), c0 = 0: c[n, :] == float(B[r(n), :]), through 1, 2 and 7
    splits (the other splits add exact zeros)."""
    x, r = P.one_hot(N, Mr)
    a = x.t().contiguous().to(DEV)
    b = P.wide_bf16(Mr, K, seed=3).to(DEV)
    out = torch.zeros(N, K, device=DEV)
    G.gemm_tn_acc(a, b, out)
    assert bit_equal(out, b[r.to(DEV)].float()), "TN, A one-hot"


# ------------------------------------------------------------------------------ f. random bf16 against fp64
@functools.lru_cache(maxsize=None)
def _rand_dev(M, N, K):
    c = P.rand_case(M, N, K)
    return {k: c[k].to(DEV) for k in ("a", "b_nk", "b_kn", "bias", "resid", "aux")}


def _within(got, ref, S, K, what, rounded=True, extra=0.0):
    allow = P.allowance(ref, S, K, rounded) + extra
    err = np.abs(got.detach().double().cpu().numpy() - ref)
    print(f"{what}: worst error / allowance {float((err / allow).max()):.3g}")
    assert (err <= allow).all(), f"{what}: {int((~(err <= allow)).sum())} elements outside the allowance"


@pytest.mark.parametrize("M,N,K", RAND_SHAPES, ids=lambda v: str(v))
def test_random_against_fp64(M, N, K, tile_config):
    """|got - ref| <= 1.13 (2^-8 |ref| + 2 K 2^-24 S), S = sum_k |a_k b_k| + |bias| + |resid| (the
    allowance of test_gemm_rows_gpu.py): NT epilogues 0, 1, 2 (y against GELU(z), the side plane
    against GELU'(z) with |ref| = |GELU'(z)|, tanh form in fp64), 3, 4 (aux = a stored GELU', |aux| <=
    1.125) and 6 (both planes, the second through frag_plane_rowmajor); NN epilogues 0 and 4.
    Nothing is widened.  Measured on an MI355X, worst error / allowance over the four configurations:
    y planes and plain outputs 0.74 - 0.83 (the bf16 rounding, at most 1 / 1.13), the GELU' planes
    0.57 at (300, 264, 776) and 0.79 at (130, 200, 328)."""
    c, d = P.rand_case(M, N, K), _rand_dev(M, N, K)
    a, b, tag = d["a"], d["b_nk"], f"({M}, {N}, {K}) config {tile_config}"
    z, Sz = c["prod"] + c["bias64"], c["abs"] + np.abs(c["bias64"])
    _within(G.gemm_nt(a, b), c["prod"], c["abs"], K, f"{tag} NT epilogue 0")
    _within(G.gemm_nt(a, b, bias=d["bias"], epi="bias"), z, Sz, K, f"{tag} NT epilogue 1")
    pre = torch.empty(M, N, dtype=BF, device=DEV)
    y = G.gemm_nt(a, b, bias=d["bias"], epi="gelu", pre_out=pre)
    _within(y, P.gelu64(z), Sz, K, f"{tag} NT epilogue 2 y")
    _within(pre, P.gelu_grad64(z), Sz, K, f"{tag} NT epilogue 2 GELU'")
    _within(G.gemm_nt(a, b, bias=d["bias"], epi="resid", resid=d["resid"], p=0.0), z + c["resid64"],
            Sz + np.abs(c["resid64"]), K, f"{tag} NT epilogue 3")
    _within(G.gemm_nt(a, b, epi="gelu_bwd", aux=d["aux"]), c["prod"] * c["aux64"], c["abs"], K, f"{tag} NT epilogue 4")
    fr = torch.empty(G.frag_aux_elems(M, N), dtype=BF, device=DEV)
    y = G.gemm_nt(a, b, bias=d["bias"], epi="gelu", pre_out=fr, frag=True)
    _within(y, P.gelu64(z), Sz, K, f"{tag} NT epilogue 6 y")
    _within(G.frag_plane_rowmajor(fr, M, N), P.gelu_grad64(z), Sz, K, f"{tag} NT epilogue 6 GELU'")
    _within(G.gemm_nn(a, d["b_kn"]), c["prod"], c["abs"], K, f"{tag} NN epilogue 0")
    _within(G.gemm_nn(a, d["b_kn"], epi="gelu_bwd", aux=d["aux"]), c["prod"] * c["aux64"], c["abs"], K,
            f"{tag} NN epilogue 4")


@pytest.mark.parametrize("Mr,N,K", [(776, 264, 328), (328, 200, 72)], ids=lambda v: str(v))
def test_random_against_fp64_tn(Mr, N, K, tile_config):
    """TN, reductions of 776 (three splits) and 328 (one): fp32 output, never rounded to bf16, so
    |got - ref| <= 1.13 (2 Mr 2^-24 S) + 2^-23 |c0|, S = sum_r |a_r b_r|."""
    c = P.tn_rand_case(Mr, N, K)
    out = c["c0"].to(DEV)
    G.gemm_tn_acc(c["a"].to(DEV), c["b"].to(DEV), out)
    _within(out, c["c064"] + c["prod"], c["abs"], Mr, f"({Mr}, {N}, {K}) config {tile_config} TN", rounded=False,
            extra=2.0 ** -23 * np.abs(c["c064"]))


# ------------------------------------------------------------------------------ g. rows and columns do not mix
def _nan_probe(run, a, b, a_row, b_slice, out_col):
    """run(a, b) with A's row a_row, then B's b_slice, filled with NaN: that output row / column is
    NaN and every other bit equals the clean run."""
    base = run(a, b)
    assert torch.isfinite(base).all()
    a2 = a.clone()
    a2[a_row] = float("nan")
    out = run(a2, b)
    keep = torch.arange(base.shape[0], device=DEV) != a_row
    assert torch.isnan(out[a_row]).all(), "the NaN row of A did not reach its output row"
    assert bit_equal(out[keep], base[keep]), f"A's row {a_row} leaked into another row"
    b2 = b.clone()
    b2[b_slice] = float("nan")
    out = run(a, b2)
    keep = torch.arange(base.shape[1], device=DEV) != out_col
    assert torch.isnan(out[:, out_col]).all(), "the NaN row / column of B did not reach its output column"
    assert bit_equal(out[:, keep], base[:, keep]), f"B's {out_col} leaked into another column"


@pytest.mark.parametrize("row,col", [(17, 17), (299, 263)], ids=["full-tile", "partial-tile"])
def test_rows_and_columns_are_independent(row, col):
    """M = 300, N = 264: row 17 / column 17 lie in a full tile of every configuration, row 299 and
    column 263 in a partial one.  NT epilogues 0 and 1 (the staged epilogue), NN epilogue 0."""
    M, N, K = 300, 264, 776
    d = _rand_dev(M, N, K)
    _nan_probe(lambda a, b: G.gemm_nt(a, b), d["a"], d["b_nk"], row, col, col)
    _nan_probe(lambda a, b: G.gemm_nt(a, b, bias=d["bias"], epi="bias"), d["a"], d["b_nk"], row, col, col)
    _nan_probe(lambda a, b: G.gemm_nn(a, b), d["a"], d["b_kn"], row, (slice(None), col), col)
