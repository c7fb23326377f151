"""Probe inputs for the training GEMM (csrc/kernels/gemm.hip), built on the CPU with numpy and torch.

tests/test_gemm_exact_gpu.py runs them through the kernels; tests/test_gemm_probe_cpu.py checks the
probes themselves (the magnitude bound, which reduction indices the nonzeros hit, the plane order).

* Integer operands.  One operand is sparse with entries in {-1, 0, +1}, at most NNZ = 32 of them
  along the reduction index of any output element; the other is dense with integers in [-4, 4] and
  no zero, so every nonzero of the sparse one moves the result.  |sum| <= 32 * 4 = 128, bias / resid
  / c0 are integers in [-8, 8], aux is in {-1, 0, 1}: every value a kernel may form is an integer of
  magnitude <= 144 < 256, exact in fp32 and bf16 in any accumulation or atomic order, and column
  sums over <= 520 rows stay below 2^24.  A lost, doubled or misplaced product is an O(1) error.
* One-hot operands: row m holds a single 1 at reduction index k(m); the product is a row or column of
  the other operand, bit for bit.
* Random bf16 operands with their fp64 products and absolute-value sums (the allowance's S).
* The inverse of ops.gemm.frag_plane_rowmajor."""
import functools
import math

import numpy as np
import torch

BF = torch.bfloat16
NNZ = 32          # nonzeros of the sparse operand per output element
BOUND = 128       # |sparse . dense| <= NNZ * 4
BK = 64           # K-tile of gemm.hip

# NT / NN shapes (M, N, K): every value of M in {130, 300, 520}, N in {72, 200, 264} and K in
# {72, 328, 776} once.  130 = a full T128 row tile + 2 rows; 300 = a W4 tile + 44; 520 = two W4 tiles
# + 8; 200 = 192 + 8 (W4-192), 264 = 256 + 8 (W4-256); K = 1, 5, 12 K-tiles of 64 + a partial one of 8.
SHAPES = ((130, 200, 328), (300, 264, 776), (520, 72, 72))
# TN (weight gradient) c[N, K] += A[Mr, N]^T B[Mr, K]: reduction lengths Mr and output shapes (N, K)
TN_MR = (136, 520, 2056)
TN_OUT = ((72, 776), (200, 72), (264, 328))
TN_NVALID = (520, 200, 328, 197)  # Mr, N, K and the n_valid < N rows of c that may be written


# --------------------------------------------------------------------------- split-K, restated
def _cdiv(a, b):
    return -(-a // b)


def choose_split(tiles, slots, nkt, ovh):
    """gemm.hip choose_split: the split count minimising rounds x (K-tiles per block + overhead),
    a further split taken only if it saves 5 %."""
    best, bc = 1, -1
    for sp in range(1, max(1, min(32, nkt // 4)) + 1):
        c = _cdiv(tiles * sp, slots) * (_cdiv(nkt, sp) + ovh)
        if bc < 0 or c * 20 < bc * 19:
            bc, best = c, sp
    return best


def tn_splits(Mr, N, K, w4):
    """K ranges [(k0, k1), ...] of the splits gemm.hip set_split gives the TN launch of reduction
    length Mr and output [N, K]: W4 (256^2 tiles, 256 slots, overhead 6) or T128 (128^2, 512, 3)."""
    tile, slots, ovh = (256, 256, 6) if w4 else (128, 512, 3)
    nkt = _cdiv(Mr, BK)
    sp = choose_split(_cdiv(N, tile) * _cdiv(K, tile), slots, nkt, ovh)
    kchunk = _cdiv(nkt, sp) * BK
    return [(k0, min(Mr, k0 + kchunk)) for k0 in range(0, Mr, kchunk)]


# --------------------------------------------------------------------------- integer operands
def sparse_rows(R, K, seed=0):
    """int8 [R, K] in {-1, 0, +1}, exactly min(NNZ, K) nonzeros per row.  Inside every band of 16 rows
    (the last one may be shorter) the nonzeros hit each of the last 8 indices and every index modulo
    64; inside every band of 128 rows they hit every index, where the band's rows can hold that many
    (NNZ * rows >= K); a shorter band's rows are still full.  Raises if a band cannot be filled."""
    rng = np.random.default_rng(7919 * R + K + seed)
    x = np.zeros((R, K), dtype=np.int8)
    per = min(NNZ, K)
    last8 = list(range(K - 8, K))
    for b0 in range(0, R, 128):
        b1 = min(R, b0 + 128)
        subs = [(s0, min(b1, s0 + 16)) for s0 in range(b0, b1, 16)]
        cap = [per * (s1 - s0) for s0, s1 in subs]
        cover = sum(cap) >= K
        # the band's share of [0, K) for each sub-band: contiguous ranges in proportion to its rows
        cuts = np.floor(np.cumsum([0] + cap) / sum(cap) * K + 0.5).astype(int) if cover else None
        for j, (s0, s1) in enumerate(subs):
            need = set(last8)
            if cover:
                need |= set(range(cuts[j], cuts[j + 1]))
            have = {k % 64 for k in need}
            for rho in range(min(64, K)):  # one index for every residue modulo 64 still missing
                if rho not in have:
                    need.add(rho + 64 * int(rng.integers(0, _cdiv(K - rho, 64))))
            need = sorted(need)
            rows = s1 - s0
            if len(need) > per * rows:
                raise ValueError(f"rows {s0}..{s1 - 1} cannot hold {len(need)} indices of K = {K}")
            cols = [need[i::rows] for i in range(rows)]
            used = set(need)
            for i, c in enumerate(cols):  # fill the row up, with indices new to the sub-band while there are any
                free = np.setdiff1d(np.arange(K), sorted(used))
                if len(free) < per - len(c):
                    free = np.setdiff1d(np.arange(K), c)
                c = list(c) + rng.choice(free, size=per - len(c), replace=False).tolist()
                used |= set(c)
                x[s0 + i, c] = rng.choice(np.array([-1, 1], dtype=np.int8), size=per)
    return x


def dense_ints(rows, cols, seed=0):
    """Integers in [-4, 4] without zero."""
    rng = np.random.default_rng(104729 + 31 * rows + cols + seed)
    return rng.choice(np.array([-4, -3, -2, -1, 1, 2, 3, 4], dtype=np.int8), size=(rows, cols))


def small_ints(shape, lo, hi, seed=0):
    rng = np.random.default_rng(15485863 + seed)
    return rng.integers(lo, hi + 1, size=shape).astype(np.int8)


def bf(a):
    """numpy integers -> bf16 tensor (exact for |v| <= 256)."""
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).to(BF)


def imatmul(a, b):
    """Exact integer product through fp64 BLAS (every partial sum is far below 2^53)."""
    return np.rint(a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def int_case(M, N, K):
    """NT / NN integers: a [M, K] sparse; b_nk [N, K] dense (NT) and its transpose b_kn (NN: the same
    products); bias [N], resid [M, N] in [-8, 8], aux [M, N] in {-1, 0, 1}, dbias0 [N] nonzero."""
    a, b_nk = sparse_rows(M, K), dense_ints(N, K)
    c = {"a": a, "b_nk": b_nk, "b_kn": np.ascontiguousarray(b_nk.T),
         "bias": small_ints(N, -8, 8, seed=M + 1), "resid": small_ints((M, N), -8, 8, seed=K + 2),
         "aux": small_ints((M, N), -1, 1, seed=N + 3),
         "dbias0": small_ints(N, 1, 9, seed=4).astype(np.int64) * np.where(np.arange(N) % 2, -1, 1)}
    c["prod"] = imatmul(a, b_nk.T)
    return c


def int_expected(c, epi):
    """int64 reference of epilogue 0 (none) | 1 (+ bias) | 3 (+ bias + resid, p = 0) | 4 (x aux)."""
    want = c["prod"].copy()
    if epi in (1, 3):
        want += c["bias"].astype(np.int64)
    if epi == 3:
        want += c["resid"].astype(np.int64)
    if epi == 4:
        want *= c["aux"].astype(np.int64)
    return want


@functools.lru_cache(maxsize=None)
def tn_int_case(Mr, N, K):
    """TN integers: a [Mr, N] sparse along Mr (column n is sparse_rows' row n), b [Mr, K] dense,
    c0 [N, K] in [-8, 8]; want = c0 + a^T b."""
    a = np.ascontiguousarray(sparse_rows(N, Mr, seed=1).T)
    b, c0 = dense_ints(Mr, K, seed=2), small_ints((N, K), -8, 8, seed=Mr + N)
    return {"a": a, "b": b, "c0": c0, "want": c0.astype(np.int64) + imatmul(a.T, b)}


# --------------------------------------------------------------------------- one-hot operands
def one_hot_index(R, K):
    """k(m) for m < R: k(0) = K - 1; rows 1 + 64 q .. 64 + 64 q take the residues 0..63 in turn, each in
    a 64-block that advances with q, so every 64 rows hit every index modulo 64 and, once R > 64
    ceil(K / 64), the rows hit all of [0, K)."""
    k = np.empty(R, dtype=np.int64)
    k[0] = K - 1
    for m in range(1, R):
        rho, q = (m - 1) % 64, (m - 1) // 64
        if rho >= K:
            rho %= K
        k[m] = rho + 64 * ((q + 3 * rho) % _cdiv(K - rho, 64))
    return k


def one_hot(R, K):
    """(bf16 [R, K] with row m = e_k(m), k as an int64 tensor)."""
    k = torch.from_numpy(one_hot_index(R, K))
    x = torch.zeros(R, K, dtype=BF)
    x[torch.arange(R), k] = 1.0
    return x, k


def wide_bf16(rows, cols, seed=0):
    """Arbitrary bf16: mixed signs, magnitudes 2^-6 .. 2^6 (log-uniform), about 1 % exact (+0) zeros."""
    g = torch.Generator().manual_seed(2971 + 13 * rows + cols + seed)
    mag = torch.exp2(torch.rand(rows, cols, generator=g) * 12 - 6)
    sign = torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    v = (mag * sign).to(BF)
    v[torch.rand(rows, cols, generator=g) < 0.01] = 0.0
    return v


# --------------------------------------------------------------------------- random bf16 vs fp64
def gelu64(z):
    """tanh-form GELU in fp64."""
    return 0.5 * z * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def gelu_grad64(z):
    """d/dz of gelu64."""
    c = math.sqrt(2.0 / math.pi)
    t = np.tanh(c * (z + 0.044715 * z ** 3))
    return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * z * z)


def randn_bf16(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


@functools.lru_cache(maxsize=None)
def rand_case(M, N, K):
    """a [M, K] ~ N(0, 1), b_nk [N, K] ~ 0.05 N(0, 1) (b_kn its transpose), bias [N], resid [M, N], aux
    [M, N] = a stored GELU' (bf16 of GELU'(N(0, 1)), |aux| < 1.13); fp64 prod = a b^T and abs = |a| |b|^T."""
    a, b_nk = randn_bf16(M, K, seed=K + M), randn_bf16(N, K, scale=0.05, seed=K + N + 1)
    bias, resid = randn_bf16(N, seed=K + 2), randn_bf16(M, N, seed=K + 3)
    # (GELU' peaks at 1.129, which bf16 rounds up to 1.1328: clipped to the bf16 value below 1.13)
    aux = torch.from_numpy(np.clip(gelu_grad64(randn_bf16(M, N, seed=K + 4).double().numpy()), -1.125, 1.125)).to(BF)
    a64, b64 = a.double().numpy(), b_nk.double().numpy()
    return {"a": a, "b_nk": b_nk, "b_kn": b_nk.t().contiguous(), "bias": bias, "resid": resid, "aux": aux,
            "prod": a64 @ b64.T, "abs": np.abs(a64) @ np.abs(b64).T, "bias64": bias.double().numpy(),
            "resid64": resid.double().numpy(), "aux64": aux.double().numpy()}


@functools.lru_cache(maxsize=None)
def tn_rand_case(Mr, N, K):
    a, b = randn_bf16(Mr, N, seed=Mr + N), randn_bf16(Mr, K, scale=0.05, seed=Mr + K + 1)
    c0 = torch.randn(N, K, generator=torch.Generator().manual_seed(Mr + 2))
    a64, b64 = a.double().numpy(), b.double().numpy()
    return {"a": a, "b": b, "c0": c0, "c064": c0.double().numpy(), "prod": a64.T @ b64,
            "abs": np.abs(a64).T @ np.abs(b64)}


def allowance(ref, S, K, rounded=True):
    """1.13 (2^-8 |ref| + 2 K 2^-24 S): one bf16 rounding (2^-9 relative, doubled), any-order fp32
    accumulation over K products (K 2^-24 S, doubled), and the largest |GELU'| (below 1.13).  fp32
    outputs (rounded=False) keep the accumulation term only."""
    return 1.13 * ((2.0 ** -8 * np.abs(ref) if rounded else 0.0) + 2 * K * 2.0 ** -24 * S)


# --------------------------------------------------------------------------- the fragment-ordered plane
def rowmajor_to_frag_plane(x, pad=0.0):
    """Inverse of ops.gemm.frag_plane_rowmajor: the [M, N] matrix x in the fragment order of the W4
    256 x 256 tiles, ceil(M / 256) * ceil(N / 256) * 65536 elements; positions outside x hold ``pad``.
    Per tile: (wave row wm, wave col wn, fragment row i, fragment-column pair jp, lane = 16 g + r, jj, 4)
    with row 128 wm + 16 i + r and columns 128 wn + 16 (2 jp + jj) + 4 g .. + 3."""
    M, N = x.shape
    tm, tn = _cdiv(M, 256), _cdiv(N, 256)
    full = torch.full((tm * 256, tn * 256), pad, dtype=x.dtype, device=x.device)
    full[:M, :N] = x
    # rows (tm wm i r), cols (tn wn jp jj g e) -> tm tn wm wn i jp g r jj e
    v = full.view(tm, 2, 8, 16, tn, 2, 4, 2, 4, 4).permute(0, 4, 1, 5, 2, 6, 8, 3, 7, 9)
    return v.reshape(-1).contiguous()
