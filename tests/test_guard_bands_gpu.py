"""Guard bands around every HIP kernel's operands (tests/_guard.py).

Each kernel runs twice through the raw extension: on plain tensors, and with every input inside an
allocation whose margins are NaN and every caller-provided output inside one whose margins hold a
sentinel.  The second run must be finite, equal the first, and leave every margin bitwise intact:
a read outside an operand that reaches the result, or a store outside an output, fails here even
though the values inside the tensors are right.  Outputs the bindings allocate themselves (LayerNorm
y / mean / rstd / dx / dz, embedding out, the cross-entropy results, the elementwise results, GEMV
y, attention out / lse / mask / dqkv) cannot be guarded; they are compared with the plain run.

Outputs summed with cross-workgroup atomics or split-K are compared with the tolerance the
existing test of that kernel uses for the same quantity (cited where used).
"""
import math
import os

import pytest
import torch

from _guard import FRONT, SENTINEL, SENTINEL_BYTE, arena, assert_intact, bit_equal, guarded
from mingpt_distributed_amd.ops import gemm as G
from mingpt_distributed_amd.ops._ext import ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, BF)


def _f32(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _sent(*shape, dtype=BF):
    """A tensor whose every byte is the sentinel: 'this element was never written'."""
    t = torch.empty(*shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    return t


def _untouched(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == SENTINEL_BYTE).all())


@pytest.fixture(params=[0, 1, 5, 6], ids=["auto", "t128", "w4", "w4n192"])
def tile_config(request):
    """Each tile configuration of gemm.hip (0 = per-shape choice), as tests/test_gemm_gpu.py."""
    ext().gemm_set_variant(request.param)
    yield request.param
    ext().gemm_set_variant(0)


# ------------------------------------------------------------------------------ positive control
def test_positive_control_oversized_destination_is_flagged():
    """The harness sees a real kernel's stores: f32_to_bf16 into a destination view that includes 8
    margin elements (still inside this test's allocation) must make assert_intact raise."""
    C = ext()
    n = 64
    buf, view = arena(torch.zeros(n, device=DEV, dtype=BF), SENTINEL)
    C.f32_to_bf16(_f32(n), view)
    assert_intact(buf, view)
    wide = buf[FRONT // 2: FRONT // 2 + n + 8]
    C.f32_to_bf16(_f32(n + 8), wide)
    with pytest.raises(AssertionError, match=rf"offset {2 * n} relative"):
        assert_intact(buf, view)


# ------------------------------------------------------------------------------ layernorm
LN_SHAPES = [(5, 48), (33, 192), (13, 520), (9, 1600), (9, 2056)]


@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_fwd(M, D):
    C = ext()
    guarded(lambda x, w, b: C.layernorm_fwd(x, w, b, 1e-5),
            {"x": _bf(M, D, seed=1), "w": _bf(D, seed=2) * 0.1 + 1, "b": _bf(D, seed=3) * 0.1}, name="layernorm_fwd")


@pytest.mark.parametrize("with_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_bwd(M, D, with_dres):
    C = ext()
    x, w, b = _bf(M, D, seed=1), _bf(D, seed=2) * 0.1 + 1, _bf(D, seed=3) * 0.1
    _, mean, rstd = C.layernorm_fwd(x, w, b, 1e-5)
    ins = {"dy": _bf(M, D, seed=4), "x": x, "w": w, "mean": mean, "rstd": rstd,
           "dres": _bf(M, D, seed=5) if with_dres else None}
    acc = {"dw": torch.ones(D, device=DEV), "db": torch.ones(D, device=DEV)}
    # dw / db: tests/test_kernels_gpu.py:65-66 (block partials folded with atomics)
    tol = {"dw": (1e-4, 1e-5), "db": (1e-4, 1e-5)}
    guarded(lambda dy, x, w, mean, rstd, dres, dw, db: C.layernorm_bwd(dy, x, w, mean, rstd, dw, db, dres),
            ins, acc, tol, name="layernorm_bwd")
    # dz_bias: tests/test_kernels_gpu.py:68
    tol["dz_bias"] = (1e-4 * math.sqrt(M), 1e-4)
    acc["dz_bias"] = torch.ones(D, device=DEV)
    guarded(lambda dy, x, w, mean, rstd, dres, dw, db, dz_bias:
            C.layernorm_bwd_dropout(dy, x, w, mean, rstd, dw, db, dres, dz_bias, 0.1, 77),
            ins, acc, tol, name="layernorm_bwd_dropout")


# ------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embedding(p):
    C = ext()
    B, T, V, D = 3, 5, 11, 24
    g = torch.Generator(device="cpu").manual_seed(0)
    idx = torch.randint(0, V, (B, T), generator=g).to(DEV)  # index margins: 0, a valid token
    guarded(lambda idx, wte, wpe: C.embedding_fwd(idx, wte, wpe, p, 1234),
            {"idx": idx, "wte": _bf(V, D, seed=5), "wpe": _bf(2 * T, D, seed=6)}, name="embedding_fwd")
    dwpe0 = _f32(2 * T, D, seed=8)
    # dwte / dwpe: tests/test_kernels_gpu.py:102-103
    _, io = guarded(lambda idx, dout, dwte, dwpe: C.embedding_bwd(idx, dout, dwte, dwpe, p, 1234),
                    {"idx": idx, "dout": _bf(B, T, D, seed=7)}, {"dwte": _f32(V, D, seed=9), "dwpe": dwpe0},
                    {"dwte": (1e-3, 1e-3), "dwpe": (1e-3, 1e-3)}, name="embedding_bwd")
    assert bit_equal(io["dwpe"][T:], dwpe0[T:]), "dwpe rows >= T were written"
    assert not torch.equal(io["dwpe"][:T], dwpe0[:T])


# ------------------------------------------------------------------------------ cross-entropy
def _xent_inputs(M, V, ld, seed=8):
    logits = _bf(M, ld, scale=3.0, seed=seed)
    logits[:, V:] = float("nan")  # xent.hip: "the pad columns are never read"
    g = torch.Generator(device="cpu").manual_seed(seed)
    tgt = torch.randint(0, V, (M,), generator=g).to(DEV)
    tgt[0] = V - 1
    tgt[1] = -1
    return logits, tgt


@pytest.mark.parametrize("M,V,ld", [(3, 13, 16), (5, 65, 72)])
def test_xent_fwd_bwd(M, V, ld):
    C = ext()
    logits, tgt = _xent_inputs(M, V, ld)
    (out, lse), _ = guarded(lambda logits, targets: C.xent_fwd(logits, targets, V),
                            {"logits": logits, "targets": tgt}, name="xent_fwd")
    (dl,), _ = guarded(lambda logits, targets, lse, gscale, out: C.xent_bwd(logits, targets, lse, gscale, out, V),
                       {"logits": logits, "targets": tgt, "lse": lse,
                        "gscale": torch.tensor([2.0], device=DEV), "out": out}, name="xent_bwd")
    assert (dl[:, V:] == 0).all()


XENT_FUSED = [(50257, 50304), (24577, 24584), (32768, 32768), (49150, 49152), (65529, 65536), (40000, 40064)]


def _fused_nv(ld):  # xent.hip xent_fused_nv: 16-byte vectors per lane of the 1024-thread workgroup
    return (ld // 8 + 1023) // 1024


def test_xent_fused_shapes_cover_every_instantiation():
    assert sorted({_fused_nv(ld) for _, ld in XENT_FUSED}) == [4, 5, 6, 7, 8]


@pytest.mark.parametrize("V,ld", XENT_FUSED)
def test_xent_fused_and_scale(V, ld):
    C = ext()
    M = 2
    logits, tgt = _xent_inputs(M, V, ld)
    tgt[1] = 7
    (out, dl), _ = guarded(lambda logits, targets: C.xent_fused(logits, targets, V),
                           {"logits": logits, "targets": tgt}, name=f"xent_fused<{_fused_nv(ld)}>")
    assert (dl[:, V:] == 0).all()
    _, io = guarded(lambda gscale, dlogits: C.xent_scale_(dlogits, gscale),
                    {"gscale": torch.tensor([3.0], device=DEV)}, {"dlogits": dl}, name="xent_scale_")
    assert (io["dlogits"][:, V:] == 0).all() and not torch.equal(io["dlogits"], dl)


# ------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("M,N", [(3, 24), (5, 520)])
def test_elementwise(M, N):
    C = ext()
    x, b, r, dy = _bf(M, N, seed=9), _bf(N, seed=10), _bf(M, N, seed=11), _bf(M, N, seed=12)
    for act in (0, 1):
        _, io = guarded(lambda x, b, pre: C.bias_act(x, b, pre, act), {"x": x, "b": b}, {"pre": _sent(M, N)},
                        name="bias_act")
        assert act == 0 or not _untouched(io["pre"])
    for p in (0.0, 0.3):
        guarded(lambda x, b, r: C.bias_dropout_residual(x, b, r, p, 7), {"x": x, "b": b, "r": r},
                name="bias_dropout_residual")
        guarded(lambda dy: C.dropout_bwd(dy, p, 7), {"dy": dy}, name="dropout_bwd")
        # db: tests/test_kernels_gpu.py:264
        guarded(lambda dy, db: C.dropout_bias_grad(dy, db, p, 7), {"dy": dy}, {"db": torch.ones(N, device=DEV)},
                {"db": (2e-2, 1e-3)}, name="dropout_bias_grad")
    guarded(lambda dy, pre: C.gelu_bwd(dy, pre), {"dy": dy, "pre": x}, name="gelu_bwd")
    # db: tests/test_kernels_gpu.py:260
    guarded(lambda dy, db: C.bias_grad(dy, db), {"dy": dy}, {"db": torch.ones(N, device=DEV)}, {"db": (2e-2, 1e-3)},
            name="bias_grad")


def test_transpose():
    C = ext()
    R, Cc, ld = 13, 24, 16
    src = _bf(R, Cc, seed=17)
    (t,), _ = guarded(lambda src: C.transpose(src, ld), {"src": src}, name="transpose")
    assert torch.equal(t[:, :R], src.t()) and (t[:, R:] == 0).all()


# ------------------------------------------------------------------------------ AdamW / grad norm
def _fill_gaps(t, pieces):
    """Sentinel bytes everywhere outside the pieces; returns the outside mask."""
    outside = torch.ones(t.numel(), dtype=torch.bool, device=DEV)
    for a, b in pieces:
        outside[a:b] = False
    t[outside] = _sent(int(outside.sum()), dtype=t.dtype)
    return outside


@pytest.mark.parametrize("zero_grad", [False, True], ids=["keepgrad", "zerograd"])
@pytest.mark.parametrize("gdtype", [torch.float32, BF], ids=["g32", "g16"])
@pytest.mark.parametrize("packed", [False, True], ids=["whole", "pieces"])
def test_adamw_and_grad_norm(packed, gdtype, zero_grad):
    """whole: the parameters of test_adamw_matches_torch (1000, 37, 4096, 5 elements, back to back);
    pieces: the ZeRO-1 form of test_adamw_pieces_packed_moments scaled to n = 20000, packed moments.
    Everything between and after the pieces holds the sentinel and must stay bitwise unchanged."""
    from mingpt_distributed_amd.optim import make_chunk_table

    C = ext()
    if packed:
        n = 20_000
        pieces = [(0, 4000, 0.1, 0), (7040, 14016, 0.0, 4000), (15040, 19968, 0.1, 10976)]
        nm = sum(b - a for a, b, _, _ in pieces)
    else:
        n = nm = 1000 + 37 + 4096 + 5 + 6  # 6 elements of padding behind the last parameter
        pieces, off = [], 0
        for s, wd in zip([1000, 37, 4096, 5], [0.1, 0.0, 0.1, 0.0]):
            pieces.append((off, off + s, wd, None))
            off += s + (-s) % 4  # piece starts are multiples of 4 (make_chunk_table)
    t = make_chunk_table(pieces, DEV, n, nm if packed else None)
    spans = [(a, b) for a, b, _, _ in pieces]
    master, grad = _f32(n, seed=1), _f32(n, seed=2).to(gdtype)
    out_f = _fill_gaps(master, spans)
    param = master.to(BF)
    _fill_gaps(param, spans)
    zg = torch.ones(n, device=DEV)
    _fill_gaps(zg, spans)
    m, v = torch.zeros(nm, device=DEV), torch.zeros(nm, device=DEV)
    if not packed:
        _fill_gaps(m, spans)
        _fill_gaps(v, spans)
    ins = {"cs": t.start, "cl": t.len, "cw": t.wd, "cm": t.mstart if packed else None, "grad": grad}
    io = {"norm": _sent(2, dtype=torch.float32), "master": master, "param": param, "m": m, "v": v,
          "zg": zg if zero_grad else None}

    def step(cs, cl, cw, cm, grad, norm, master, param, m, v, zg):
        C.grad_sumsq_chunks(cs, cl, grad, 0.5, norm, t.end)
        C.adamw_step(cs, cl, cw, cm, master, param, grad, m, v, norm, 1e-3, 0.9, 0.95, 1e-8, 1, 0.5, 1.0,
                     t.end, t.mend, zg)

    _, res = guarded(step, ins, io, name="adamw_step")
    sq = sum((grad.float()[a:b] * 0.5).pow(2).sum() for a, b in spans)
    torch.testing.assert_close(res["norm"][1], sq.sqrt(), rtol=1e-4, atol=1e-4)  # test_kernels_gpu.py:213
    inside = ~out_f
    assert not torch.equal(res["master"][inside], master[inside])
    for k, ref in (("master", master), ("param", param)) + ((("m", m), ("v", v)) if not packed else ()):
        assert bit_equal(res[k][out_f], ref[out_f]), f"{k}: elements outside the pieces were written"
    if zero_grad:
        assert (res["zg"][inside] == 0).all() and bit_equal(res["zg"][out_f], zg[out_f])

    if not packed and gdtype == torch.float32 and not zero_grad:
        # the whole-buffer norm kernel and the master -> bf16 conversion, on the same buffers
        _, r2 = guarded(lambda grad, norm: C.grad_sumsq(grad, 0.5, norm), {"grad": _f32(n, seed=2)},
                        {"norm": _sent(2, dtype=torch.float32)}, name="grad_sumsq")
        torch.testing.assert_close(r2["norm"][1], (_f32(n, seed=2) * 0.5).pow(2).sum().sqrt(), rtol=1e-4, atol=1e-4)
        for k in (n, 37, 5):
            _, r3 = guarded(lambda src, dst: C.f32_to_bf16(src, dst), {"src": _f32(k, seed=3)},
                            {"dst": _sent(k)}, name="f32_to_bf16")
            assert torch.equal(r3["dst"], _f32(k, seed=3).to(BF))


# ------------------------------------------------------------------------------ GEMV
@pytest.mark.parametrize("B,N,K", [(1, 100, 64), (5, 72, 136), (8, 257, 72)])
def test_gemv(B, N, K):
    C = ext()
    assert C.gemv_supported(B, K)
    x, w, b, r = _bf(B, K, seed=21), _bf(N, K, scale=0.05, seed=22), _bf(N, seed=23), _bf(B, N, seed=24)
    ld = (N + 7) // 8 * 8
    # y's pad columns N..ld-1 are never written (the binding's uninitialised allocation): left out
    (y0,), _ = guarded(lambda x, W: C.gemv(x, W, 0, None, None, ld)[:, :N], {"x": x, "W": w}, name="gemv epi 0")
    torch.testing.assert_close(y0.float(), x.float() @ w.float().t(), atol=2e-2, rtol=2e-2)
    for epi in (1, 2):
        guarded(lambda x, W, bias: C.gemv(x, W, epi, bias, None, 0), {"x": x, "W": w, "bias": b}, name=f"gemv epi {epi}")
    guarded(lambda x, W, bias, resid: C.gemv(x, W, 3, bias, resid, 0), {"x": x, "W": w, "bias": b, "resid": r},
            name="gemv epi 3")
    guarded(lambda x, W, bias, lnw, lnb: C.gemv(x, W, 1, bias, None, 0, lnw, lnb, 1e-5),
            {"x": x, "W": w, "bias": b, "lnw": _bf(K, seed=25) * 0.1 + 1, "lnb": _bf(K, seed=26) * 0.1},
            name="gemv fused LayerNorm")


# ------------------------------------------------------------------------------ GEMM
def _dbias_tol(out):  # tests/test_gemm_gpu.py:149-150
    return (6e-3 * out.float().pow(2).sum(0).max().item() ** 0.5 + 1e-2, 1e-3)


@pytest.mark.parametrize("M,N,K", [(130, 72, 136), (300, 200, 320)])
def test_gemm_nt(M, N, K, tile_config):
    """c is taller than M: rows >= M (and both margins) stay bitwise untouched."""
    C = ext()
    Mc = M + 5
    a, b, bias = _bf(M, K, seed=1), _bf(N, K, seed=2), _bf(N, seed=3)
    side = _bf(Mc, N, seed=4)

    def run(epi, ins, io, tol=None, p=0.0):
        def fn(a, b, c, bias=None, aux=None, resid=None, dbias=None):
            C.gemm(a, b, c, 0, epi, bias, aux, resid, p, 11, M, N, dbias)
        _, res = guarded(fn, dict(a=a, b=b, **ins), dict(c=_sent(Mc, N), **io), tol, name=f"gemm NT epi {epi}")
        assert _untouched(res["c"][M:]), f"epi {epi}: rows >= M of c were written"
        assert not _untouched(res["c"][:M])
        return res

    r0 = run(0, {}, {})
    tol = 2e-2 * (K ** 0.5) * 0.25 + 2e-2  # test_gemm_gpu.py _check
    torch.testing.assert_close(r0["c"][:M].float(), a.float() @ b.float().t(), atol=tol, rtol=2e-2)
    run(1, {"bias": bias}, {})
    r2 = run(2, {"bias": bias}, {"aux": _sent(Mc, N)})
    assert _untouched(r2["aux"][M:]) and not _untouched(r2["aux"][:M])
    run(3, {"bias": bias, "resid": side}, {}, p=0.3)
    plain = torch.empty(Mc, N, device=DEV, dtype=BF)
    C.gemm(a, b, plain, 0, 4, None, side, None, 0.0, 0, M, N, None)
    run(4, {"aux": side}, {"dbias": torch.ones(N, device=DEV)}, {"dbias": _dbias_tol(plain[:M])})


@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_nt_padded_row_stride(epi, tile_config):
    """gemm NT with ld > N (the padded logits).  What gemm.hip does to the pad columns N..ld-1 of
    rows < M, read from its epilogues (nlim = ldc for the plain epilogue, N for all others):
      * epilogue 0 (none): they are WRITTEN, with the products against B's rows N..ld-1, which lie
        past B's buffer extent and read as zero -- so the pad columns are exactly 0 (cross-entropy's
        dlogits path and the LM-head data gradient rely on finite pads);
      * every other epilogue: untouched.
    With B inside NaN margins the zeros also prove that B's extent ends at row N."""
    C = ext()
    M, N, K, ld = 130, 72, 136, 80
    a, b, bias = _bf(M, K, seed=1), _bf(N, K, seed=2), _bf(N, seed=3)
    _, res = guarded(lambda a, b, bias, c: C.gemm(a, b, c, 0, epi, bias if epi else None, None, None, 0.0, 0, M, N, None),
                     {"a": a, "b": b, "bias": bias}, {"c": _sent(M + 3, ld)}, name="gemm NT ld > N")
    c = res["c"]
    assert _untouched(c[M:])
    ref = a.float() @ b.float().t() + (bias.float() if epi else 0)
    torch.testing.assert_close(c[:M, :N].float(), ref, atol=2e-2 * (K ** 0.5) * 0.25 + 2e-2, rtol=2e-2)
    if epi == 0:
        assert (c[:M, N:] == 0).all()
    else:
        assert _untouched(c[:M, N:])


@pytest.mark.parametrize("M,N,K,Kb", [(100, 64, 72, 72), (130, 256, 1008, 1001)])
def test_gemm_nn(M, N, K, Kb, tile_config):
    """b has Kb <= K rows; rows Kb..K-1 lie in the NaN margin and must read as zero (a's columns
    past Kb are zero, as the engine's padded operands are)."""
    C = ext()
    a, b, gd = _bf(M, K, seed=10), _bf(Kb, N, seed=11), _bf(M + 5, N, seed=12)
    a[:, Kb:] = 0
    ref = a.float()[:, :Kb] @ b.float()
    tol = 2e-2 * (K ** 0.5) * 0.25 + 2e-2
    _, r = guarded(lambda a, b, c: C.gemm(a, b, c, 1, 0, None, None, None, 0.0, 0, M, N, None),
                   {"a": a, "b": b}, {"c": _sent(M + 5, N)}, name="gemm NN epi 0")
    assert _untouched(r["c"][M:])
    torch.testing.assert_close(r["c"][:M].float(), ref, atol=tol, rtol=2e-2)
    _, r = guarded(lambda a, b, aux, c, dbias: C.gemm(a, b, c, 1, 4, None, aux, None, 0.0, 0, M, N, dbias),
                   {"a": a, "b": b, "aux": gd}, {"c": _sent(M + 5, N), "dbias": torch.ones(N, device=DEV)},
                   {"dbias": _dbias_tol(ref * gd[:M].float())}, name="gemm NN epi 4")
    assert _untouched(r["c"][M:])
    torch.testing.assert_close(r["c"][:M].float(), ref * gd[:M].float(), atol=tol, rtol=2e-2)


@pytest.mark.parametrize("Mr,N,K,nv", [(192, 72, 136, None), (328, 200, 72, None), (128, 72, 64, 69)])
def test_gemm_tn_acc(Mr, N, K, nv, tile_config):
    """c[N, K] += a[Mr, N]^T b[Mr, K] (split-K atomics: tests/test_gemm_gpu.py:175's tolerance);
    c is taller than the rows written (n_valid form: a has N columns, nv of them valid)."""
    C = ext()
    a, b = _bf(Mr, N, seed=13), _bf(Mr, K, seed=14)
    rows = nv or N
    c0 = torch.cat([_f32(rows, K, seed=15), _sent(3, K, dtype=torch.float32)])
    _, r = guarded(lambda a, b, c: C.gemm(a, b, c, 2, 0, None, None, None, 0.0, 0, rows, K, None),
                   {"a": a, "b": b}, {"c": c0}, {"c": (1e-3, 1e-4)}, name="gemm TN")
    assert _untouched(r["c"][rows:])
    ref = c0[:rows] + a.float()[:, :rows].t() @ b.float()
    torch.testing.assert_close(r["c"][:rows], ref, atol=2e-2 * (Mr ** 0.5) * 0.25 + 2e-2, rtol=2e-2)


def test_gemm_fragment_plane(tile_config):
    """Epilogues 6 / 7: the fragment-ordered GELU' plane (whole 256 x 256 tiles) in a sentinel arena
    when written, in a NaN arena when read."""
    C = ext()
    M, N, K = 300, 256, 192
    x, w, bias = _bf(M, K, seed=41), _bf(N, K, seed=42, scale=0.05), _bf(N, seed=43, scale=0.1)
    _, r = guarded(lambda a, b, bias, c, aux: C.gemm(a, b, c, 0, 6, bias, aux, None, 0.0, 0, M, N, None),
                   {"a": x, "b": w, "bias": bias}, {"c": _sent(M + 5, N), "aux": _sent(G.frag_aux_elems(M, N))},
                   name="gemm NT epi 6")
    assert _untouched(r["c"][M:])
    pre = torch.empty(M, N, device=DEV, dtype=BF)
    y = G.gemm_nt(x, w, bias=bias, epi="gelu", pre_out=pre)
    torch.testing.assert_close(r["c"][:M], y, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(G.frag_plane_rowmajor(r["aux"], M, N), pre, atol=2e-2, rtol=2e-2)
    dz, wp = _bf(M, K, seed=44), _bf(K, N, seed=45, scale=0.05)
    ref = (dz.float() @ wp.float()) * pre.float()
    _, r7 = guarded(lambda a, b, aux, c, dbias: C.gemm(a, b, c, 1, 7, None, aux, None, 0.0, 0, M, N, dbias),
                    {"a": dz, "b": wp, "aux": r["aux"]}, {"c": _sent(M + 5, N), "dbias": torch.ones(N, device=DEV)},
                    {"dbias": _dbias_tol(ref)}, name="gemm NN epi 7")
    assert _untouched(r7["c"][M:])
    torch.testing.assert_close(r7["c"][:M].float(), ref, atol=2e-2 * (K ** 0.5) * 0.25 + 2e-2, rtol=2e-2)


# ------------------------------------------------------------------------------ attention
@pytest.fixture(params=[1, 2], ids=["bwd_persistent", "bwd_partials"])
def bwd_mode(request):
    ext().attention_set_bwd_mode(request.param)
    yield request.param
    ext().attention_set_bwd_mode(0)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,H,hd", [(2, 77, 2, 64), (1, 130, 3, 48), (2, 65, 1, 80), (1, 200, 2, 128)])
def test_attention_fwd_bwd(B, T, H, hd, p, bwd_mode):
    C = ext()
    D = H * hd
    qkv, dout = _bf(B * T, 3 * D, seed=1), _bf(B * T, D, seed=2)
    (out, lse, mask), _ = guarded(lambda qkv: C.attention_fwd(qkv, B, T, H, p, 7), {"qkv": qkv}, name="attention_fwd",
                                  skip=("out2",))  # keep words of tiles past the diagonal are unspecified
    ins = {"qkv": qkv, "out": out, "dout": dout, "lse": lse, "mask": mask}  # keep words: margins 0
    try:
        for b64 in ((1, 0) if hd == 64 else (1,)):
            C.attention_set_bwd64(b64)
            guarded(lambda qkv, out, dout, lse, mask: C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 7),
                    ins, name=f"attention_bwd bwd64={b64}")
            # dbias: tests/test_attention_gpu.py:104 (the order of its cross-workgroup atomics)
            guarded(lambda qkv, out, dout, lse, mask, dbias: C.attention_bwd(qkv, out, dout, lse, mask, B, T, H, p, 7, dbias),
                    ins, {"dbias": torch.full((3 * D,), 0.5, device=DEV)}, {"dbias": (1e-3, 1e-4)},
                    name=f"attention_bwd + dbias bwd64={b64}")
    finally:
        C.attention_set_bwd64(int(os.environ.get("MINGPT_ATTN_BWD64", "1")))


@pytest.mark.parametrize("pos", [0, 63, 64, 129])
@pytest.mark.parametrize("hd", [24, 64])
def test_attention_decode(hd, pos):
    C = ext()
    B, H, Tmax = 3, 2, 130
    D = H * hd
    cache, qkv = _bf(B, Tmax, 3 * D, seed=hd), _bf(B, 3 * D, seed=pos + 1)
    np_ = C.attention_decode_part_floats(B, H, hd)
    (out,), r = guarded(lambda qkv_new, cache, part, counters: C.attention_decode(qkv_new, cache, H, pos, None, part, counters),
                        {"qkv_new": qkv}, {"cache": cache, "part": torch.zeros(np_, device=DEV),
                                           "counters": torch.zeros(B * H, device=DEV, dtype=torch.int32)},
                        name="attention_decode", skip=("part",))  # part: workspace
    c = r["cache"]
    assert (r["counters"] == 0).all()
    assert torch.equal(c[:, pos, D:], qkv[:, D:])  # K/V appended
    want = cache.clone()
    want[:, pos, D:] = qkv[:, D:]
    assert bit_equal(c, want), "the cache changed outside row pos's K/V slots"
    q = qkv[:, :D].float().view(B, H, hd)
    k = c[:, :pos + 1, D:2 * D].float().view(B, pos + 1, H, hd)
    v = c[:, :pos + 1, 2 * D:].float().view(B, pos + 1, H, hd)
    att = torch.einsum("bhd,bthd->bht", q, k) / hd ** 0.5
    ref = torch.einsum("bht,bthd->bhd", att.softmax(-1), v).reshape(B, D)
    torch.testing.assert_close(out.float(), ref, atol=2e-2, rtol=2e-2)
