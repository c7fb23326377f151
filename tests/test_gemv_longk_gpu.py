"""The skinny GEMM (csrc/kernels/gemv.hip) at 4096 < K <= 8192 -- the MLP output projection of
gpt2-large (K = 5120) and gpt2-xl (K = 6400), x staged through LDS in two segments -- against the
kernel's arithmetic restated in numpy float32 (tests/_gemv_oracle.py).

Epilogues 0 (none), 1 (bias) and 3 (bias + residual) are compared bit for bit, at the shapes the
kernel took before as well (which pins the restatement to the kernel) and at the new ones; epilogue
2 (bias + GELU) goes through the device's tanh and is compared with ``test_gemv_epilogues``'
tolerance (atol 2e-2, rtol 2e-2).  The inputs and the lane sums of a shape are computed once and
shared by the tests of that shape.

The wide path (N > 8192: 16 lanes per output column, a capped grid striding over 16-column blocks) is
pinned the same way against the restatement at 16 lanes, and its fused argmax against the first
index of the maximum of the stored row.

The binding allocates y itself, so sentinel margins cannot be put around it.  Stores next to y are
looked for in two ways instead: ``guarded`` (NaN margins around every input; the residual is one) and
a y that lands on a block just filled with the sentinel, whose pad columns N..ldy-1 must keep it."""
import functools
import os

import numpy as np
import pytest
import torch

import _gemv_oracle as O
from _guard import SENTINEL_BYTE, bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

OLD_SHAPES = [(1, 2304, 768), (3, 768, 3072), (5, 100, 64), (8, 24, 4096)]
NEW_SHAPES = [(1, 1280, 5120),   # gpt2-large
              (8, 1600, 6400),   # gpt2-xl
              (3, 100, 8192),    # the longest row
              (5, 23, 4104),     # one chunk over a segment, K no multiple of 512, N no multiple of 4
              (2, 7, 4608),      # a segment and one full round of the 64 lanes
              (8, 8192, 5120)]   # the last N on the one-column-per-wave path
WIDE_SHAPES = [(3, 8200, 64),     # 513 column blocks on a grid capped at 512: one workgroup strides to a second
               (1, 16400, 64),    # the B <= 2 cap of 1024, with a second item; N no multiple of 16
               (8, 8208, 1032),   # two K segments, the second holding a single chunk
               (5, 8193, 4096)]   # the longest row of the wide path; one column in the last block
_I64_MIN = -(1 << 63)


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _np(t):
    return t.float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(B, N, K):
    """Inputs on the device (left unchanged) and the folded lane sums of the restatement."""
    x, w = _bf(B, K, seed=K + B), _bf(N, K, scale=0.05, seed=K + N + 1)
    bias, resid = _bf(N, seed=K + 2), _bf(B, N, seed=K + 3)
    lanes = O.WIDE_LANES if N > O.WIDE_N else O.LANES
    sums = O.fold(O.lane_sums(_np(x), _np(w), lanes), lanes)
    return {"x": x.to(DEV), "w": w.to(DEV), "bias": bias.to(DEV), "resid": resid.to(DEV), "sums": sums,
            "bias_np": _np(bias), "resid_np": _np(resid)}


def _bits(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _check_epilogues(B, N, K):
    C, c = ext(), _case(B, N, K)
    for epi in (0, 1, 2, 3):
        bias = c["bias"] if epi else None
        y = C.gemv(c["x"], c["w"], epi, bias, c["resid"] if epi == 3 else None, 0)
        assert y.shape == (B, N) and y.dtype == BF
        want_bits, want = O.epilogue(c["sums"], epi, c["bias_np"] if epi else None, c["resid_np"])
        if epi == 2:
            np.testing.assert_allclose(_np(y), want, atol=2e-2, rtol=2e-2)
            continue
        diff = _bits(y) != want_bits
        print(f"({B}, {N}, {K}) epilogue {epi}: {int(diff.sum())} of {diff.size} outputs differ from the restatement")
        assert not diff.any(), (f"epilogue {epi}: first difference at (row, column) {tuple(np.argwhere(diff)[0])}, "
                                f"worst |difference| {float(np.abs(_np(y) - want).max()):.4g}")


@pytest.mark.parametrize("B,N,K", OLD_SHAPES, ids=lambda v: str(v))
def test_restatement_pinned_at_whole_row_shapes(B, N, K):
    """K <= 4096, x staged whole: the restatement equals the kernel bit for bit."""
    _check_epilogues(B, N, K)


@pytest.mark.parametrize("B,N,K", NEW_SHAPES, ids=lambda v: str(v))
def test_long_rows_equal_the_restatement(B, N, K):
    """4096 < K <= 8192, x staged in two segments: the same chain of fmas, bit for bit."""
    assert ext().gemv_supported(B, K)
    _check_epilogues(B, N, K)


@pytest.mark.parametrize("B,N,K", WIDE_SHAPES, ids=lambda v: str(v))
def test_wide_path_equals_the_restatement(B, N, K):
    """N > 8192: 16 lanes per column, grid-strided; the same chain at 16 lanes, bit for bit."""
    C = ext()
    if "MINGPT_GEMV_WIDE_GRID" not in os.environ:  # the shapes do what their comments say
        assert C.gemv_argmax_groups(8200, 3) == 512 and C.gemv_argmax_groups(16400, 1) == 1024
    _check_epilogues(B, N, K)


def _check_padded(B, N, K, ld, epi):
    C, c = ext(), _case(B, N, K)
    resid = None
    if epi == 3:
        resid = torch.zeros(B, ld, dtype=BF, device=DEV)
        resid[:, :N] = c["resid"]
    bias = c["bias"] if epi else None
    want_bits, _ = O.epilogue(c["sums"], epi, c["bias_np"] if epi else None, c["resid_np"])
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    block = torch.empty(B, ld, dtype=BF, device=DEV)
    block.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    ptr = block.data_ptr()
    del block
    y = C.gemv(c["x"], c["w"], epi, bias, resid, ld)
    assert y.shape == (B, ld) and y.data_ptr() == ptr, "y did not land on the sentinel block: nothing was checked"
    assert np.array_equal(_bits(y[:, :N]), want_bits)
    assert (y[:, N:].contiguous().view(-1).view(torch.uint8) == SENTINEL_BYTE).all(), "a pad column was written"


@pytest.mark.parametrize("epi", [0, 3])
def test_padded_leading_dimension(epi):
    """ldy = 24 > N = 23: columns 0..22 are the ldy = N result, and the pad column keeps what the
    block held before -- y is allocated on a block this test has just filled with the sentinel and
    freed (the caching allocator hands the same block back; asserted)."""
    _check_padded(5, 23, 4104, 24, epi)


@pytest.mark.parametrize("epi", [0, 3])
def test_wide_padded_leading_dimension(epi):
    """The wide path at one chunk per row, ldy = 8208 > N = 8200: the pad columns keep the sentinel."""
    _check_padded(2, 8200, 8, 8208, epi)


def test_wide_fused_argmax():
    """gemv with am_part at (3, 8200, 64), 512 workgroups: after the host reduction generation.py
    applies to the last step's keys (unsigned max, 0xFFFFFFFF - low word) every row gives the FIRST
    index of the maximum of its stored bf16 logits.  Row 0's maximum ties between columns of two
    different workgroups (two equal weight rows), row 1's sits in the last, partly filled column
    block (the second item of workgroup 0); am_pos advances by one; y is the plain call's."""
    B, N, K = 3, 8200, 64
    C, c = ext(), _case(B, N, K)
    G = C.gemv_argmax_groups(N, B)
    w = c["w"].clone()
    w[100] = w[5000] = 0.5 * c["x"][0]   # column blocks 6 and 312: different workgroups whatever the grid
    w[N - 1] = 0.5 * c["x"][1]
    plain = C.gemv(c["x"], w, 0, None, None, 0)
    part = torch.full((B, G), -1, dtype=torch.long, device=DEV)  # every entry must be written
    pos = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    y = C.gemv(c["x"], w, 0, None, None, 0, None, None, 1e-5, part, pos)
    assert bit_equal(y, plain)
    assert int(pos.item()) == 8
    rows = _np(y[:, :N])
    want = rows.argmax(axis=1)  # numpy: the first index of the maximum
    assert want[0] == 100 and rows[0, 100] == rows[0, 5000] and want[1] == N - 1, "the case is not what it says"
    k = (part ^ _I64_MIN).max(dim=1).values ^ _I64_MIN
    got = (0xFFFFFFFF - (k & 0xFFFFFFFF)).cpu().numpy()
    assert np.array_equal(got, want), f"argmax {got.tolist()}, first maximum at {want.tolist()}"


@pytest.mark.parametrize("N,K", [(100, 6400), (23, 4104)])
def test_rows_are_independent(N, K):
    """Row r of a B-row call equals the one-row call on that row, bit for bit, for every epilogue:
    a row's sum does not depend on how many rows share the staging buffer."""
    C = ext()
    w, bias = _bf(N, K, scale=0.05, seed=1).to(DEV), _bf(N, seed=2).to(DEV)
    x, resid = _bf(8, K, seed=3).to(DEV), _bf(8, N, seed=4).to(DEV)
    one = {epi: [C.gemv(x[r:r + 1].contiguous(), w, epi, bias if epi else None,
                        resid[r:r + 1].contiguous() if epi == 3 else None, 0) for r in range(8)]
           for epi in (0, 1, 2, 3)}
    for B in (2, 5, 8):
        for epi in (0, 1, 2, 3):
            y = C.gemv(x[:B].contiguous(), w, epi, bias if epi else None,
                       resid[:B].contiguous() if epi == 3 else None, 0)
            for r in range(B):
                assert bit_equal(y[r:r + 1], one[epi][r]), f"B = {B}, epilogue {epi}, row {r}"


@pytest.mark.parametrize("epi,B,N,K", [(0, 3, 23, 4104), (1, 2, 7, 4608), (2, 5, 100, 8192), (3, 8, 41, 6400)])
def test_guard_bands(epi, B, N, K):
    """NaN margins around x, W, the bias and the residual: the result is finite and equals the plain
    run, and no margin byte changes."""
    C = ext()
    x, w = _bf(B, K, seed=31).to(DEV), _bf(N, K, scale=0.05, seed=32).to(DEV)
    b, r = _bf(N, seed=33).to(DEV), _bf(B, N, seed=34).to(DEV)
    if epi == 0:
        ld = (N + 7) // 8 * 8  # the pad columns are never written: left out of the comparison
        guarded(lambda x, W: C.gemv(x, W, 0, None, None, ld)[:, :N], {"x": x, "W": w}, name="gemv long K epi 0")
    elif epi == 3:
        guarded(lambda x, W, bias, resid: C.gemv(x, W, 3, bias, resid, 0), {"x": x, "W": w, "bias": b, "resid": r},
                name="gemv long K epi 3")
    else:
        guarded(lambda x, W, bias: C.gemv(x, W, epi, bias, None, 0), {"x": x, "W": w, "bias": b},
                name=f"gemv long K epi {epi}")


def test_refusals():
    C = ext()
    x = torch.zeros(1, 8200, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="K <= 8192"):
        C.gemv(x, torch.zeros(8, 8200, dtype=BF, device=DEV), 0, None, None, 0)
    x = torch.zeros(2, 4104, dtype=BF, device=DEV)
    ln = torch.ones(4104, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="K > 4096 cannot take LayerNorm"):
        C.gemv(x, torch.zeros(8, 4104, dtype=BF, device=DEV), 1, torch.zeros(8, dtype=BF, device=DEV), None, 0,
               ln, ln, 1e-5)
    with pytest.raises(RuntimeError, match="K > 4096 needs N <= 8192"):
        C.gemv(x, torch.zeros(8200, 4104, dtype=BF, device=DEV), 0, None, None, 0)


def test_gemv_supported():
    C = ext()
    assert C.gemv_supported(8, 8192) and C.gemv_supported(1, 4104)
    assert not C.gemv_supported(8, 8200) and not C.gemv_supported(9, 4096)
    assert not C.gemv_supported(0, 4096) and not C.gemv_supported(1, 8188)
