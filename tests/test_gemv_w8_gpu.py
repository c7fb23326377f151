"""The int8-weight skinny GEMM (``gemv_w8``, csrc/kernels/gemv.hip; the W8 rule in common.h) on the
smallest shapes that reach each path's edges.  Every comparison is exact:

* epilogues 0, 1 and 3 against the numpy restatement ``epilogue(s * fold(lane_sums(x, q)))``
  (tests/_gemv_oracle.py), bit for bit;
* all four epilogues, GELU included, against ``C.gemv`` on the dequantized bf16 matrix s q, bit for
  bit (both kernels run the same device tanh on the same fp32 value);
* on the wide path the fused argmax keys and the position advance against the bf16 kernel's;
* the fused LayerNorm against ``C.gemv`` with the same LayerNorm arguments;
* a padded ``ldy`` keeps its pad columns; q inside an int8 buffer whose margins hold 127 and x, bias,
  residual and scale between NaN margins (tests/_guard.py) change nothing.

The inputs and the restatement's sums of a shape are computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import _gemv_oracle as O
from _guard import FRONT, BACK, SENTINEL_BYTE, bit_equal, guarded
from mingpt_distributed_amd.ops._ext import ext
from mingpt_distributed_amd.ops.quant import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

NARROW = [(1, 5, 8),          # one chunk, one lane busy, N no multiple of 4
          (3, 23, 520),       # a full round of the 64 lanes and one chunk
          (8, 24, 4096)]      # the longest whole-row shape
LONG = [(5, 23, 4104),        # one chunk over a segment
        (2, 7, 4608),         # a segment and one full round
        (8, 12, 8192)]        # the longest row
WIDE = [(3, 8200, 64),        # 513 column blocks on a grid capped at 512
        (1, 16400, 64),       # the B <= 2 cap of 1024, with a second item; N no multiple of 16
        (8, 8208, 1032)]      # two K segments, the second holding a single chunk
SHAPES = NARROW + LONG + WIDE
LN_SHAPES = [(2, 16, 768), (8, 16, 1040), (4, 8200, 64)]  # rows held in registers | re-read | the wide path


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _np(t):
    return t.float().cpu().numpy()


def _bits(y):
    return y.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _case(B, N, K):
    """Inputs on the device (left unchanged), the int8 rows and scales of a random matrix, its
    dequantized bf16 form and the restatement's scaled sums."""
    x, w = _bf(B, K, seed=K + B), _bf(N, K, scale=0.05, seed=K + N + 1)
    if N > 2:
        w[2] = 0  # a zero row: scale 1, q 0
    q, s = quantize_rows(w)
    wd = dequantize_rows(q, s, BF)
    bias, resid = _bf(N, seed=K + 2), _bf(B, N, seed=K + 3)
    lanes = O.WIDE_LANES if N > O.WIDE_N else O.LANES
    sums = s.numpy()[None, :] * O.fold(O.lane_sums(_np(x), q.float().numpy(), lanes), lanes)
    assert sums.dtype == np.float32
    return {"x": x.to(DEV), "q": q.to(DEV), "s": s.to(DEV), "wd": wd.to(DEV), "bias": bias.to(DEV),
            "resid": resid.to(DEV), "sums": sums, "bias_np": _np(bias), "resid_np": _np(resid)}


@pytest.mark.parametrize("B,N,K", SHAPES, ids=str)
def test_equals_the_restatement_and_the_bf16_kernel(B, N, K):
    C, c = ext(), _case(B, N, K)
    assert C.gemv_w8_supported(B, K)
    for epi in (0, 1, 2, 3):
        bias, resid = (c["bias"] if epi else None), (c["resid"] if epi == 3 else None)
        y = C.gemv_w8(c["x"], c["q"], c["s"], epi, bias, resid, 0)
        assert y.shape == (B, N) and y.dtype == BF
        ref = C.gemv(c["x"], c["wd"], epi, bias, resid, 0)
        diff = _bits(y) != _bits(ref)
        print(f"({B}, {N}, {K}) epilogue {epi}: {int(diff.sum())} of {diff.size} outputs differ from gemv on s q")
        assert not diff.any(), f"epilogue {epi} against gemv: first difference at {tuple(np.argwhere(diff)[0])}"
        if epi != 2:
            want_bits, want = O.epilogue(c["sums"], epi, c["bias_np"] if epi else None, c["resid_np"])
            diff = _bits(y) != want_bits
            print(f"({B}, {N}, {K}) epilogue {epi}: {int(diff.sum())} of {diff.size} outputs differ from the restatement")
            assert not diff.any(), (f"epilogue {epi} against the restatement: first difference at "
                                    f"{tuple(np.argwhere(diff)[0])}, worst {float(np.abs(_np(y) - want).max()):.4g}")


@pytest.mark.parametrize("B,N,K", WIDE, ids=str)
def test_wide_argmax_keys_and_position(B, N, K):
    """The fused argmax: every (row, workgroup) key and the position advance equal the bf16 kernel's."""
    C, c = ext(), _case(B, N, K)
    G = C.gemv_argmax_groups(N, B)
    out = []
    for w8 in (True, False):
        part = torch.full((B, G), -1, dtype=torch.long, device=DEV)  # every entry must be written
        pos = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        if w8:
            y = C.gemv_w8(c["x"], c["q"], c["s"], 0, None, None, 0, None, None, 1e-5, part, pos)
        else:
            y = C.gemv(c["x"], c["wd"], 0, None, None, 0, None, None, 1e-5, part, pos)
        out.append((y, part, pos))
    (y8, part8, pos8), (y16, part16, pos16) = out
    assert bit_equal(y8, y16) and bit_equal(y8, C.gemv_w8(c["x"], c["q"], c["s"], 0, None, None, 0))
    assert torch.equal(part8, part16) and not (part8 == -1).any()
    assert int(pos8.item()) == 8 == int(pos16.item())
    k = (part8 ^ -(1 << 63)).max(dim=1).values ^ -(1 << 63)
    got = (0xFFFFFFFF - (k & 0xFFFFFFFF)).cpu().numpy()
    assert np.array_equal(got, _np(y8).argmax(axis=1))


@pytest.mark.parametrize("B,N,K", LN_SHAPES, ids=str)
def test_fused_layernorm_equals_the_bf16_kernel(B, N, K):
    """The LayerNorm-fused staging of x: the same bits as the bf16 kernel stages, epilogues 1 and 2."""
    C = ext()
    x = (_bf(B, K, seed=5) * 1.5 + 0.25).to(DEV)
    q, s = quantize_rows(_bf(N, K, scale=0.05, seed=6))
    wd = dequantize_rows(q, s, BF).to(DEV)
    q, s = q.to(DEV), s.to(DEV)
    lnw, lnb, bias = (_bf(K, seed=7) * 0.1 + 1).to(BF).to(DEV), _bf(K, scale=0.1, seed=8).to(DEV), _bf(N, seed=9).to(DEV)
    for epi in (0, 1, 2):
        b = bias if epi else None
        y = C.gemv_w8(x, q, s, epi, b, None, 0, lnw, lnb, 1e-5)
        ref = C.gemv(x, wd, epi, b, None, 0, lnw, lnb, 1e-5)
        diff = _bits(y) != _bits(ref)
        print(f"({B}, {N}, {K}) LayerNorm, epilogue {epi}: {int(diff.sum())} of {diff.size} outputs differ")
        assert not diff.any(), f"epilogue {epi}: first difference at {tuple(np.argwhere(diff)[0])}"
    xn = C.layernorm_fwd(x, lnw, lnb, 1e-5)[0]  # and the staging is that kernel's output
    assert bit_equal(C.gemv_w8(x, q, s, 1, bias, None, 0, lnw, lnb, 1e-5), C.gemv_w8(xn, q, s, 1, bias, None, 0))


@pytest.mark.parametrize("B,N,K,ld", [(5, 23, 4104, 24), (3, 23, 520, 32), (2, 8200, 8, 8208)], ids=str)
@pytest.mark.parametrize("epi", [0, 3])
def test_padded_leading_dimension(B, N, K, ld, epi):
    """ldy > N: columns 0..N-1 are the ldy = N result and the pad columns keep what the block held -- y
    is allocated on a block this test has just filled with the sentinel and freed (asserted)."""
    C = ext()
    x, bias = _bf(B, K, seed=11).to(DEV), _bf(N, seed=12).to(DEV)
    q, s = quantize_rows(_bf(N, K, scale=0.05, seed=13))
    q, s = q.to(DEV), s.to(DEV)
    r = _bf(B, N, seed=14).to(DEV)
    want = C.gemv_w8(x, q, s, epi, bias if epi else None, r if epi == 3 else None, 0)
    resid = None
    if epi == 3:
        resid = torch.zeros(B, ld, dtype=BF, device=DEV)
        resid[:, :N] = r
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    block = torch.empty(B, ld, dtype=BF, device=DEV)
    block.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    ptr = block.data_ptr()
    del block
    y = C.gemv_w8(x, q, s, epi, bias if epi else None, resid, ld)
    assert y.shape == (B, ld) and y.data_ptr() == ptr, "y did not land on the sentinel block: nothing was checked"
    assert bit_equal(y[:, :N], want)
    assert (y[:, N:].contiguous().view(-1).view(torch.uint8) == SENTINEL_BYTE).all(), "a pad column was written"


@pytest.mark.parametrize("epi,B,N,K", [(3, 3, 23, 520), (1, 5, 23, 4104), (2, 8, 12, 8192), (0, 3, 8200, 64),
                                       (3, 8, 8208, 1032)], ids=str)
def test_guard_bands(epi, B, N, K):
    """q inside a larger int8 buffer whose margins hold 127 (the largest weight: a read outside a row
    moves the sums); x, bias, residual and scale between NaN margins.  The outputs are finite, equal
    the plain run's, and no margin byte changes."""
    C, c = ext(), _case(B, N, K)
    buf = torch.full((FRONT + N * K + BACK,), 127, dtype=torch.int8, device=DEV)
    qv = buf[FRONT:FRONT + N * K].view(N, K)
    qv.copy_(c["q"])
    inputs = {"x": c["x"], "scale": c["s"]}
    if epi:
        inputs["bias"] = c["bias"]
    if epi == 3:
        inputs["resid"] = c["resid"]

    def run(x, scale, bias=None, resid=None):
        return C.gemv_w8(x, qv, scale, epi, bias, resid, 0)

    out, _ = guarded(run, inputs, name=f"gemv_w8 ({B}, {N}, {K}) epi {epi}")
    assert bit_equal(out[0], C.gemv_w8(c["x"], c["q"], c["s"], epi, inputs.get("bias"), inputs.get("resid"), 0))
    assert (buf[:FRONT] == 127).all() and (buf[FRONT + N * K:] == 127).all() and torch.equal(qv, c["q"])


def test_refusals():
    C = ext()
    x = torch.zeros(2, 64, dtype=BF, device=DEV)
    q = torch.zeros(8, 64, dtype=torch.int8, device=DEV)
    s = torch.ones(8, device=DEV)
    assert C.gemv_w8(x, q, s, 0).shape == (2, 8)
    with pytest.raises(RuntimeError, match="int8"):
        C.gemv_w8(x, q.to(BF), s, 0)
    with pytest.raises(RuntimeError, match="int8"):
        C.gemv_w8(x, q.to(torch.uint8), s, 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.gemv_w8(x, torch.zeros(8, 128, dtype=torch.int8, device=DEV)[:, ::2], s, 0)
    with pytest.raises(RuntimeError, match="scale"):
        C.gemv_w8(x, q, torch.ones(7, device=DEV), 0)
    with pytest.raises(RuntimeError, match="fp32"):
        C.gemv_w8(x, q, s.to(BF), 0)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        C.gemv_w8(x, torch.zeros(8 * 64 + 4, dtype=torch.int8, device=DEV)[4:].view(8, 64), s, 0)
    with pytest.raises(RuntimeError, match="K <= 8192"):
        C.gemv_w8(torch.zeros(9, 64, dtype=BF, device=DEV), q, s, 0)
    assert C.gemv_w8_supported(8, 8192) and not C.gemv_w8_supported(9, 64) and not C.gemv_w8_supported(1, 12)
