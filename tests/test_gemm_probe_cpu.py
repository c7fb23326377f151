"""The probes of tests/_gemm_probe.py, checked without a GPU: what tests/test_gemm_exact_gpu.py feeds
the training GEMM really has the properties its exactness argument and its reach depend on.

* the integer references stay within |v| <= 128 + 16, column sums far below 2^24;
* the sparse operand's nonzeros hit every reduction index inside every 128-row band of the output
  (a row tile of T128, the smallest tile), every index modulo 64 inside every 16-row band (one MFMA
  fragment row) and each of the last 8 reduction indices (the partial K-tile) there too;
* the TN reduction lengths give one split, two splits with a partial last one, and seven with a
  shorter last one, under the cost constants of both tile families, and every split is hit;
* the one-hot rows hit K - 1 and every index modulo 64;
* rowmajor_to_frag_plane and ops.gemm.frag_plane_rowmajor undo each other.

A 128-row band with fewer than K / 32 rows cannot hit K indices with 32 nonzeros per row: the 2-row
tail of M = 130 (any K >= 72) and, in TN, the 8-row tail of N = 264 at Mr = 520 and 2056.  There the
rows are full (32 distinct indices each, no index twice in a 16-row band) and the other two
conditions hold; every other band meets all three.  M = 130, 300, 520 and N = 264 are kept because
they are the tile edges under test."""
import numpy as np
import pytest
import torch

import _gemm_probe as P
from mingpt_distributed_amd.ops import gemm as G

NT_IDS = [f"{m}x{n}x{k}" for m, n, k in P.SHAPES]
TN_CASES = [(mr, n, k) for mr in P.TN_MR for n, k in P.TN_OUT] + [P.TN_NVALID[:3]]


def _check_sparse(x, K):
    """x [rows, K]: the conditions on the nonzeros of a sparse operand (rows = output rows)."""
    R = x.shape[0]
    assert set(np.unique(x).tolist()) <= {-1, 0, 1}
    per_row = (x != 0).sum(1)
    assert per_row.max() <= P.NNZ and (per_row == min(P.NNZ, K)).all()
    for b0 in range(0, R, 128):
        band = x[b0:b0 + 128]
        hit = (band != 0).any(0)
        if P.NNZ * band.shape[0] >= K:
            assert hit.all(), f"rows {b0}..: reduction indices {np.flatnonzero(~hit)[:8]} never hit"
        else:  # too short to hit K indices: the largest number of distinct ones its rows can hold
            assert (b0, R, K) in {(128, 130, 328), (256, 264, 520), (256, 264, 2056)}, (b0, R, K)
            assert band.shape[0] <= 16 and hit.sum() == P.NNZ * band.shape[0]
    for s0 in range(0, R, 16):
        sub = x[s0:s0 + 16]
        cols = np.flatnonzero((sub != 0).any(0))
        assert set((cols % 64).tolist()) == set(range(64)), f"rows {s0}..: a residue modulo 64 is never hit"
        assert set(range(K - 8, K)) <= set(cols.tolist()), f"rows {s0}..: the partial K-tile is not hit"


@pytest.mark.parametrize("M,N,K", P.SHAPES, ids=NT_IDS)
def test_integer_operands_nt_nn(M, N, K):
    c = P.int_case(M, N, K)
    assert c["a"].shape == (M, K) and c["b_nk"].shape == (N, K) and c["b_kn"].shape == (K, N)
    _check_sparse(c["a"], K)
    b = c["b_nk"].astype(np.int64)
    assert (b != 0).all() and np.abs(b).max() == 4
    assert np.array_equal(c["prod"], c["a"].astype(np.int64) @ b.T)  # the BLAS route is exact
    assert np.abs(c["prod"]).max() <= P.BOUND
    assert np.abs(c["prod"]).max() >= 32, "the products are too small to exercise anything"
    for v, lim in ((c["bias"], 8), (c["resid"], 8), (c["aux"], 1)):
        assert np.abs(v).max() == lim
    assert set(np.unique(c["aux"]).tolist()) == {-1, 0, 1}
    assert (c["dbias0"] != 0).all() and np.abs(c["dbias0"]).max() <= 9
    for epi in (0, 1, 3, 4):
        want = P.int_expected(c, epi)
        assert np.abs(want).max() <= P.BOUND + 16 < 256
        # bf16 and fp32 hold every such value exactly
        assert np.array_equal(P.bf(want).double().numpy(), want.astype(np.float64))
        assert np.abs(want).sum(0).max() + 9 < 2 ** 24  # any partial column sum, dbias0 included


@pytest.mark.parametrize("Mr,N,K", TN_CASES, ids=lambda v: str(v))
def test_integer_operands_tn(Mr, N, K):
    c = P.tn_int_case(Mr, N, K)
    assert c["a"].shape == (Mr, N) and c["b"].shape == (Mr, K) and c["want"].shape == (N, K)
    _check_sparse(np.ascontiguousarray(c["a"].T), Mr)  # column n of a: at most 32 nonzeros along Mr
    assert (c["b"] != 0).all() and np.abs(c["b"]).max() == 4
    assert np.abs(c["c0"]).max() == 8
    prod = c["a"].astype(np.int64).T @ c["b"].astype(np.int64)
    assert np.array_equal(c["want"], c["c0"] + prod)
    assert np.abs(prod).max() <= P.BOUND and np.abs(c["want"]).max() <= P.BOUND + 8
    # any subset of the split partials is an integer of magnitude <= 128 as well: the atomics are exact
    for w4 in (False, True):
        for k0, k1 in P.tn_splits(Mr, N, K, w4):
            part = c["a"][k0:k1].astype(np.int64).T @ c["b"][k0:k1].astype(np.int64)
            assert np.abs(part).max() <= P.BOUND
            # and every split matters to every 128-row band of the output
            for b0 in range(0, N, 128):
                assert (c["a"][k0:k1, b0:b0 + 128] != 0).any(), (w4, k0, b0)
            assert (part != 0).any()


@pytest.mark.parametrize("w4", [False, True], ids=["t128", "w4"])
def test_tn_reduction_lengths_force_the_splits(w4):
    """Mr = 136: one split.  Mr = 520: 9 K-tiles, two splits of 320 and 200.  Mr = 2056: 33 K-tiles,
    seven splits, 6 x 320 and 136.  The same under W4 (256 slots, overhead 6) and T128 (512 slots,
    overhead 3), at every output shape used (all of them fit one round of blocks)."""
    for N, K in P.TN_OUT + ((200, 328),):
        assert P.tn_splits(136, N, K, w4) == [(0, 136)]
        assert P.tn_splits(520, N, K, w4) == [(0, 320), (320, 520)]
        s = P.tn_splits(2056, N, K, w4)
        assert len(s) == 7 and s[-1] == (1920, 2056) and all(k1 - k0 == 320 for k0, k1 in s[:-1])
        assert len(P.tn_splits(776, N, K, w4)) == 3  # the random fp64 case is a multi-split launch too


def test_one_hot_rows():
    for R in (72, 130, 200, 264, 300, 520):
        for K in (72, 136, 328, 520, 776, 2056):
            x, k = P.one_hot(R, K)
            k = k.numpy()
            assert x.shape == (R, K) and (x.sum(1) == 1).all() and (x.float().abs().sum(1) == 1).all()
            assert (x[np.arange(R), k] == 1).all()
            assert k.min() >= 0 and k.max() == K - 1 and k[0] == K - 1
            assert set((k % 64).tolist()) == set(range(64))
            for s0 in range(1, R - 15, 16):  # a fragment row's 16 rows sit at 16 different residues
                assert len(set((k[s0:s0 + 16] % 64).tolist())) == 16
            if R > 64 * -(-K // 64):
                assert set(k.tolist()) == set(range(K))
            else:  # spread over the whole range: every K-tile that 64 rows can reach
                assert len(set((k // 64).tolist())) >= min(-(-K // 64), (R - 1) // 64)


def test_wide_bf16_operand():
    v = P.wide_bf16(264, 776)
    f = v.float()
    nz = f[f != 0].abs()
    assert nz.min() >= 2.0 ** -6 * (1 - 2.0 ** -8) and nz.max() <= 2.0 ** 6
    assert nz.min() < 2.0 ** -5 and nz.max() > 2.0 ** 5
    assert 0.3 < (f < 0).float().mean() < 0.7
    assert 0 < (f == 0).sum() < 0.03 * f.numel()
    assert not ((f == 0) & torch.signbit(f)).any()  # no -0: x + 0 would not return it bit for bit


@pytest.mark.parametrize("M,N", [(300, 264), (130, 200), (520, 72), (256, 512), (1, 1)])
def test_plane_order_inverse(M, N):
    """frag_plane_rowmajor(rowmajor_to_frag_plane(x)) == x and back, on distinct values; the pad
    positions hold the pad value."""
    x = torch.arange(M * N, dtype=torch.float32).reshape(M, N)
    plane = P.rowmajor_to_frag_plane(x, pad=-1.0)
    assert plane.shape == (G.frag_aux_elems(M, N),)
    assert torch.equal(G.frag_plane_rowmajor(plane, M, N), x)
    assert (plane == -1.0).sum() == plane.numel() - M * N
    # the other way round, from a full plane of distinct values
    tm, tn = -(-M // 256), -(-N // 256)
    p2 = torch.arange(tm * tn * 65536, dtype=torch.float32)
    assert torch.equal(P.rowmajor_to_frag_plane(G.frag_plane_rowmajor(p2, tm * 256, tn * 256)), p2)
    # and the documented position of one element: tile (0, 0), wave (wm, wn), fragment (i, j), lane 16 g + r
    if M >= 256 and N >= 256:
        wm, wn, i, j, g, r, e = 1, 0, 5, 3, 2, 9, 1
        at = ((wm * 2 + wn) * 8 + i) * 2048 + (j // 2) * 512 + (16 * g + r) * 8 + (j % 2) * 4 + e
        assert plane[at] == x[128 * wm + 16 * i + r, 128 * wn + 16 * j + 4 * g + e]


def test_fp64_gelu_forms():
    z = np.linspace(-6, 6, 2401)
    h = 1e-6
    assert np.abs((P.gelu64(z + h) - P.gelu64(z - h)) / (2 * h) - P.gelu_grad64(z)).max() < 1e-8
    assert np.abs(P.gelu_grad64(z)).max() < 1.13
    c = P.rand_case(130, 200, 328)
    assert np.abs(c["aux64"]).max() == 1.125 and c["aux64"].min() < 0  # inside the allowance's 1.13
