"""The skinny GEMM's arithmetic (csrc/kernels/gemv.hip) restated in numpy float32, operation for
operation.  A helper module, not a conftest: tests import what they use.

An output column is summed by L lanes: L = 64 on the one-column-per-wave paths (N <= 8192), L = 16 on
the wide path (N > 8192), whose rounds of 128 columns run across its 1024-column segments in the same
ascending order.  For row b, column n and lane j in 0..L-1:

* ``acc_j = 0``; for u = 0, 1, ... with c = 8 j + 8 L u < K and e = 0..7 in order,
  ``acc_j = fmaf(W[n, c + e], x[b, c + e], acc_j)``.  The product of two bf16 values has at most 16
  significant bits, so it is exact in fp32 and ``float32(acc + w * x)`` IS the fma.  Chunks past K
  are zero here (the kernel skips them): adding +0 changes nothing.
* the xor-shuffle fold: for o = 1, 2, 4, ..., L / 2 every lane takes ``acc_j + acc_{j ^ o}``.
* the epilogue in fp32: ``v = acc + bias`` (0.0 without a bias), epilogue 2 ``v = gelu(v)`` (tanh
  form; the device's tanh differs in the last bits, so this one is compared by tolerance),
  epilogue 3 ``v = v + resid``; then one round-to-nearest-even to bf16.

Epilogues 0, 1 and 3 are therefore reproducible bit for bit; ``bound`` is what any fp32 evaluation
in this order may differ from the real dot product by."""
import numpy as np

LANES, CHUNK = 64, 8
WIDE_LANES, WIDE_N = 16, 8192  # N > WIDE_N: the wide path, WIDE_LANES lanes per output column


def bf16_round(v):
    """float32 ``v`` rounded to nearest-even bf16: (the bf16 bit patterns as uint16, their float32 values)."""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    r = (bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return r.astype(np.uint16), (r << np.uint32(16)).view(np.float32)


def lane_sums(x, w, lanes=LANES):
    """acc [B, N, lanes] (float32): every lane's fma chain.  ``x`` [B, K], ``w`` [N, K]: float32 arrays
    of bf16 values, K a multiple of 8."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    (B, K), N = x.shape, w.shape[0]
    assert w.shape[1] == K and K % CHUNK == 0
    rnd = lanes * CHUNK  # columns of one load round of a row
    U = -(-K // rnd)
    xp = np.zeros((B, U * rnd), dtype=np.float32)
    xp[:, :K] = x
    wp = np.zeros((N, U * rnd), dtype=np.float32)
    wp[:, :K] = w
    xs = np.ascontiguousarray(xp.reshape(B, U, lanes, CHUNK).transpose(1, 3, 0, 2))  # [U, 8, B, lanes]
    ws = np.ascontiguousarray(wp.reshape(N, U, lanes, CHUNK).transpose(1, 3, 0, 2))  # [U, 8, N, lanes]
    acc = np.zeros((B, N, lanes), dtype=np.float32)
    for u in range(U):
        for e in range(CHUNK):
            for b in range(B):
                acc[b] += ws[u, e] * xs[u, e, b]  # exact product, one fp32 rounding: the fma
    return acc


def fold(acc, lanes=LANES):
    """The xor-shuffle fold over the last axis (``lanes`` lanes): every lane ends with the same sum;
    lane 0's."""
    assert acc.shape[-1] == lanes
    idx = np.arange(lanes)
    o = 1
    while o < lanes:
        acc = acc + acc[..., idx ^ o]
        o *= 2
    return acc[..., 0]


def gelu(v):
    v = v.astype(np.float64)
    return (0.5 * v * (1.0 + np.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))).astype(np.float32)


def epilogue(sums, epi=0, bias=None, resid=None):
    """(bits uint16 [B, N], values float32 [B, N]) of the kernel's output for the folded sums ``sums``
    [B, N] and epilogue ``epi`` (0 none, 1 bias, 2 bias + GELU, 3 bias + residual); ``bias`` [N],
    ``resid`` [B, N]: float32 arrays of bf16 values."""
    v = sums + (np.asarray(bias, dtype=np.float32)[None, :] if bias is not None else np.float32(0.0))
    if epi == 2:
        v = gelu(v)
    if epi == 3:
        v = v + np.asarray(resid, dtype=np.float32)
    return bf16_round(v)


def gemv(x, w, epi=0, bias=None, resid=None, lanes=LANES):
    """``epilogue`` of the folded lane sums of ``x`` [B, K] against ``w`` [N, K]."""
    return epilogue(fold(lane_sums(x, w, lanes), lanes), epi, bias, resid)


def bound(x, w, lanes=LANES):
    """|y - ref| allowed against the real dot product ``ref`` [B, N] (returned with it, fp64), with L =
    ``lanes``: 2^-8 |ref| (the bf16 rounding: half an ulp of 8 significant bits is at most 2^-8 of the
    value) + 2 (K / L + log2 L) 2^-24 sum_k |w_k x_k| (K / L fmas per lane and log2 L fold adds, each to
    half an ulp -- 2^-24 -- of a partial sum that sum_k |w_k x_k| bounds; doubled, which also covers
    the rounding acting on the fp32 sum instead of on ref)."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ref = x64 @ w64.T
    mass = np.abs(x64) @ np.abs(w64).T
    K = x64.shape[1]
    return ref, 2.0 ** -8 * np.abs(ref) + 2.0 * (K / lanes + np.log2(lanes)) * 2.0 ** -24 * mass
