"""Probe inputs, references and comparison helpers for the row-wise training kernels (LayerNorm,
cross-entropy, the elementwise epilogues, the bias-gradient reductions, the embedding), built on the
CPU with numpy and torch from fixed seeds.

tests/test_row_exact_gpu.py runs them through the kernels; tests/test_row_probe_cpu.py checks the
probes themselves (exactness in any order, the allowances against a plain fp32 evaluation, and that
the comparison helpers fail on a dropped row or a zeroed vector).

* Integer ("census") cases.  Every input is a small integer (or a half-integer), exact in bf16, and
  every sum a kernel may form stays far below 2^24 in the unit of its terms: exact in fp32 in any
  summation or atomic order.  A lost, doubled or misplaced row is an O(1) error and `exact` compares
  with no tolerance.  Every accumulator starts from a nonzero integer vector.
* The references are plain torch int64 / fp64 and work on whatever device their inputs are on: the
  GPU tests move a case to the device first, so a 100 MB case costs no CPU seconds.
* The per-element allowances of the toleranced checks (LayerNorm dx and y, GELU', cross-entropy)."""
import functools
import math

import numpy as np
import torch

BF = torch.bfloat16
U = 2.0 ** -24      # half an fp32 ulp, relative
BF_ULP = 2.0 ** -7  # one bf16 ulp, relative (the rounding itself is at most half of it)

# LayerNorm: D values that reach every NV (1: D <= 512, 2: <= 1024, 4: <= 2048, 8: <= 4096), each
# boundary, and a partial last group of 64 lanes x 8 columns
LN_D = (48, 512, 520, 768, 1024, 1600, 2048, 2056, 4096)
LN_D_PER_NV = (48, 768, 1600, 4096)
LN_M_SMALL = (1, 5, 12, 37)    # pair partner r0 + 4 absent / present, partial last block
LN_M_CHUNK = 1063              # grid 33: ln_colsum's second 32-row chunk holds one partial row
LN_ROWS_MAX = 1 << 16          # the sums stay exact up to this many rows (and a little past it)

BIAS_N = (24, 520, 768, 2304, 3072, 4104)  # CVB 64, 64, 32, 32, 64, 64; 4104: a partial column block
BIAS_M = (1, 63, 64, 130, 4099)
BIAS_HALVING = (32773, 3072)

ELT_SHAPES = ((3, 24), (2740, 3072))
EMB_D = (48, 512, 520, 768, 1600)
EMB_BT = ((3, 7), (4, 64))
EMB_V = 11
EMB_TOKENS = (1, 3, 4, 8, 10)  # the 5 tokens idx draws from: 6 rows of wte are never used

XENT_SHAPES = ((17, 65, 72), (9, 50257, 50304), (9, 24577, 24584), (5, 65529, 65536), (9, 40000, 40064))
XENT_LONG = ((2085, 65, 72, 1500), (1030, 24577, 24584, 1027))  # M, V, ld, valid rows of the count probe
XENT_FUSED_MIN_LD = 24584
OLD_ATOL = 2e-3  # the absolute tolerance of the assert_close cross-entropy tests

DROP_P = 0.5     # threshold 32768, keep scale exactly 2
DROP_SEED = (5 << 32) + 7


# --------------------------------------------------------------------------- helpers
def ints(shape, lo, hi, seed):
    """int8 tensor of integers in [lo, hi] (numpy's PCG64 from a fixed seed)."""
    rng = np.random.default_rng(1_000_003 * seed + 17)
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape, dtype=np.int8))


def nonzero_ints(n, seed):
    """int8 [n]: magnitudes 1..9 with alternating signs -- an accumulator's initial value."""
    v = ints(n, 1, 9, seed)
    return torch.where(torch.arange(n) % 2 == 1, -v, v)


def bf(t):
    """small integers -> bf16 (exact for |v| <= 256)."""
    return t.to(torch.float32).to(BF)


def randn_bf16(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF)


def exact(got, want, what):
    """Every element of got equals the reference by value, no tolerance: only the sign of a zero may
    differ, NaN counts as wrong.  Compared on got's device."""
    got = got.detach().double()
    want = torch.as_tensor(want).to(got.device).double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} for {tuple(want.shape)}"
    bad = got != want  # NaN != anything: counted
    if bad.any():
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} wrong, first at {first}: "
                             f"{got[first].item()} for {want[first].item()}")


def within(got, ref, allow, what):
    """|got - ref| <= allow for every element (NaN counts as outside); prints and returns the worst
    error / allowance (an element with allowance 0 must be equal and counts as 0)."""
    ref = ref.double()
    err = (got.detach().double().to(ref.device) - ref).abs()
    allow = allow.double().expand_as(ref)
    bad = ~(err <= allow)
    ratio = float(torch.where(allow > 0, err / allow, torch.zeros_like(err)).max()) if err.numel() else 0.0
    print(f"{what}: worst error / allowance {ratio:.3g}")
    if bad.any():
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the allowance, first at "
                             f"{first}: error {err[first].item():.3g}, allowed {allow[first].item():.3g}, "
                             f"reference {ref[first].item():.6g}")
    return ratio


def to_dev(c, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def keep_mask(M, N, device="cpu"):
    """The residual-stream dropout keep set at (DROP_P, DROP_SEED), from the oracle of
    tests/test_dropout_mask_oracle_gpu.py (imported, not restated)."""
    from test_dropout_mask_oracle_gpu import keep_scale, oracle_keep

    assert keep_scale(DROP_P) == 2.0
    return oracle_keep(M, N, DROP_P, DROP_SEED, device=device)


# --------------------------------------------------------------------------- LayerNorm
def make_ln_case(M, D, seed=0):
    """x in [-3, 3], mean in [-1, 2] and rstd in {0.5, 1, 2} per row (rstd2 = 2 rstd), dy in [-4, 4],
    dres in [-8, 8], w in [-2, 2]; dw0 / db0 / dzb0 nonzero.  xhat = (x - mean) rstd is a half-integer,
    |xhat| <= 10, and dy xhat a multiple of 0.5, |.| <= 40."""
    s = 7919 * M + 31 * D + seed
    return {"M": M, "D": D,
            "x": ints((M, D), -3, 3, s), "dy": ints((M, D), -4, 4, s + 1), "dres": ints((M, D), -8, 8, s + 2),
            "mean": ints(M, -1, 2, s + 3), "rstd2": torch.tensor([1, 2, 4], dtype=torch.int8)[ints(M, 0, 2, s + 4).long()],
            "w": ints(D, -2, 2, s + 5), "dw0": nonzero_ints(D, s + 6), "db0": nonzero_ints(D, s + 7),
            "dzb0": nonzero_ints(D, s + 8)}


ln_case = functools.lru_cache(maxsize=None)(make_ln_case)


def ln_xhat2(c):
    """2 xhat as int32 [M, D]."""
    return (c["x"].int() - c["mean"].int()[:, None]) * c["rstd2"].int()[:, None]


def ln_census(c):
    """fp64 (dw, db) = (dw0 + sum_m dy xhat, db0 + sum_m dy), from int64 sums."""
    dy = c["dy"].int()
    dw2 = (dy * ln_xhat2(c)).sum(0, dtype=torch.int64)
    return c["dw0"].double() + dw2.double() / 2, (c["db0"].long() + dy.sum(0, dtype=torch.int64)).double()


def ln_dz(c, keep):
    """(dz, dzb) of the fused dropout backward when dx == dres: dz = 2 keep dres, dzb = dzb0 + sum_m dz."""
    dz = torch.where(keep, 2 * c["dres"].int(), 0)
    return dz.double(), (c["dzb0"].long() + dz.sum(0, dtype=torch.int64)).double()


def ln_dx_ref(c, with_dres):
    """fp64 dx = rs (g w - s1 - xhat s2) (+ dres), s1 = mean_D(g w), s2 = mean_D(g w xhat), and the
    allowance 2^-7 |ref| + 8 2^-24 rs (|g w| + |s1| + |xhat s2| + |dres|): one bf16 ulp, and a few fp32
    ulps of the cancelling terms (the row sums are exact integers: nothing grows with D)."""
    xh, rs = ln_xhat2(c).double() / 2, c["rstd2"].double()[:, None] / 2
    gw = c["dy"].double() * c["w"].double()
    s1, s2 = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
    res = c["dres"].double() if with_dres else torch.zeros_like(gw)
    ref = rs * (gw - s1 - xh * s2) + res
    return ref, BF_ULP * ref.abs() + 8 * U * rs * (gw.abs() + s1.abs() + (xh * s2).abs() + res.abs())


def ln_dx_fp32(c, with_dres):
    """The same formula in plain fp32 torch, rounded to bf16."""
    xh, rs = ln_xhat2(c).float() / 2, c["rstd2"].float()[:, None] / 2
    gw = c["dy"].float() * c["w"].float()
    D = gw.shape[1]
    s1, s2 = gw.sum(1, keepdim=True) / D, (gw * xh).sum(1, keepdim=True) / D
    o = rs * (gw - s1 - xh * s2)
    if with_dres:
        o = o + c["dres"].float()
    return o.to(BF)


@functools.lru_cache(maxsize=None)
def ln_fwd_case(M, D, shifted=False):
    """The data of test_kernel_edges_gpu.py::test_layernorm_rstd: x ~ N(0, 1) (shifted: 30 + 0.5 N(0, 1)),
    w = 1 + 0.1 N, b = 0.1 N, all bf16."""
    w, b = randn_bf16(D, seed=2) * 0.1 + 1, randn_bf16(D, seed=3) * 0.1
    x = randn_bf16(M, D, scale=0.5, shift=30.0, seed=4) if shifted else randn_bf16(M, D, seed=1)
    return {"x": x, "w": w, "b": b}


def ln_fwd_ref(c, eps=1e-5):
    """fp64 LayerNorm of the bf16 inputs and the allowance 2^-7 |ref| + 8 2^-24 (|xhat w| + |b|)."""
    x, w, b = c["x"].double(), c["w"].double(), c["b"].double()
    xh = (x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    ref = xh * w + b
    return ref, BF_ULP * ref.abs() + 8 * U * ((xh * w).abs() + b.abs())


# --------------------------------------------------------------------------- bias gradients
def make_bias_case(M, N):
    s = 104729 * M + N
    return {"dy": ints((M, N), -4, 4, s), "db0": nonzero_ints(N, s + 1)}


bias_case = functools.lru_cache(maxsize=None)(make_bias_case)


def bias_census(c, keep=None):
    """fp64 db0 + sum_m dy; with keep: (dx, db) = (2 keep dy, db0 + sum_m dx)."""
    dy = c["dy"].int()
    if keep is None:
        return (c["db0"].long() + dy.sum(0, dtype=torch.int64)).double()
    dx = torch.where(keep, 2 * dy, 0)
    return dx.double(), (c["db0"].long() + dx.sum(0, dtype=torch.int64)).double()


# --------------------------------------------------------------------------- elementwise
@functools.lru_cache(maxsize=None)
def elt_case(M, N):
    """x in [-24, 24], b in [-8, 8], r in [-64, 64]: |r + 2 (x + b)| <= 128; dy in [-4, 4]; and random bf16
    gdy ~ N(0, 1), pre ~ 2 N(0, 1) for GELU'."""
    s = 611953 * M + N
    return {"x": ints((M, N), -24, 24, s), "b": ints(N, -8, 8, s + 1), "r": ints((M, N), -64, 64, s + 2),
            "dy": ints((M, N), -4, 4, s + 3), "gdy": randn_bf16(M, N, seed=s + 4),
            "pre": randn_bf16(M, N, scale=2.0, seed=s + 5)}


def gelu_grad64(z):
    """d/dz of the tanh-form GELU, fp64 torch."""
    k = math.sqrt(2.0 / math.pi)
    t = torch.tanh(k * (z + 0.044715 * z ** 3))
    return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * k * (1.0 + 3 * 0.044715 * z * z)


def gelu_bwd_ref(c):
    """fp64 dy GELU'(pre) and the allowance 2^-7 |ref| + |dy| 2^-18 (derivation: test_row_exact_gpu.py
    test_gelu_bwd_grid_stride)."""
    dy = c["gdy"].double()
    ref = dy * gelu_grad64(c["pre"].double())
    return ref, BF_ULP * ref.abs() + dy.abs() * 2.0 ** -18


def gelu_error_model(x):
    """fp64 (bound on |computed GELU'(x) - GELU'(x)| before the bf16 rounding, |GELU'(x)|) for the sigmoid
    form of csrc/include/common.h (gelu_sigmoid, gelu_grad_from) with exp2 and rcp good to 1 ulp:
      t = x (E1 x^2 + E0), three roundings: |dt| <= 3 2^-24 |t|;  e = exp2(t): de / e <= ln 2 |dt| + 2^-23;
      s = rcp(1 + e): ds <= s (1 - s) de / e + (2^-24 + 2^-23) s               (ds / de = -s^2, s e = 1 - s);
      GELU' = s + P, P = 2 K0 x s (1 - s) (1 + 3 K1 x^2): d GELU' / d s = 1 + 2 K0 x (1 - 2 s) (1 + 3 K1 x^2);
      the product's own roundings: 8 2^-24 |P|; the final fma: 2^-24 |GELU'|.
    For large positive x (e < 2^-25) s is exactly 1 and the computed value exactly 1: the error is |P|."""
    k0, k1 = math.sqrt(2.0 / math.pi), 0.044715
    u2 = 2 * k0 * (x + k1 * x ** 3)
    t = u2.abs() / math.log(2.0)
    s = torch.sigmoid(u2)
    poly = 1 + 3 * k1 * x * x
    ds = s * (1 - s) * (math.log(2.0) * 3 * U * t + 2 * U) + 3 * U * s
    prod = 2 * k0 * x * s * (1 - s) * poly
    grad = s + prod
    err = (1 + 2 * k0 * x * (1 - 2 * s) * poly).abs() * ds + 8 * U * prod.abs() + U * grad.abs()
    # e < 2^-25: 1 + e rounds to 1, s = rcp(1) = 1 and P = 0 exactly; the computed value is 1, off by |P|
    return torch.where(u2 > 25 * math.log(2.0), prod.abs() + U, err), grad.abs()


def gelu_bwd_fp32(c):
    """dy GELU'(pre) in plain fp32 torch through the sigmoid form of csrc/include/common.h, rounded to bf16."""
    x, k0, k1 = c["pre"].float(), math.sqrt(2.0 / math.pi), 0.044715
    sg = torch.sigmoid(2 * k0 * (x + k1 * x ** 3))
    return (c["gdy"].float() * (sg + 2 * k0 * x * sg * (1 - sg) * (1 + 3 * k1 * x * x))).to(BF)


# --------------------------------------------------------------------------- embedding
@functools.lru_cache(maxsize=None)
def emb_case(B, T, D):
    """wte [11, D] and wpe [2 T, D] in [-32, 32], idx [B, T] from EMB_TOKENS, dout in [-4, 4], dwte0 [11, D]
    and dwpe0 [2 T, D] nonzero."""
    s = 15485863 + 1009 * B + 97 * T + D
    pick = ints((B, T), 0, len(EMB_TOKENS) - 1, s).long()
    return {"B": B, "T": T, "D": D, "wte": ints((EMB_V, D), -32, 32, s + 1), "wpe": ints((2 * T, D), -32, 32, s + 2),
            "idx": torch.tensor(EMB_TOKENS)[pick], "dout": ints((B, T, D), -4, 4, s + 3),
            "dwte0": nonzero_ints(EMB_V * D, s + 4).view(EMB_V, D), "dwpe0": nonzero_ints(2 * T * D, s + 5).view(2 * T, D)}


def emb_fwd_expected(c, keep=None):
    """int32 wte[idx] + wpe[t] as [B T, D]; with keep: 2 keep (...)."""
    B, T, D = c["B"], c["T"], c["D"]
    out = (c["wte"].int()[c["idx"]] + c["wpe"].int()[:T][None]).view(B * T, D)
    return out if keep is None else torch.where(keep, 2 * out, 0)


def emb_bwd_expected(c, keep=None):
    """int64 (dwte, dwpe): dwte0 + index_add of g, dwpe0[:T] + sum_b g (rows >= T unchanged); g = dout, or
    2 keep dout."""
    B, T, D = c["B"], c["T"], c["D"]
    g = c["dout"].long().view(B * T, D)
    if keep is not None:
        g = torch.where(keep, 2 * g, 0)
    dwte = c["dwte0"].long().index_add(0, c["idx"].reshape(-1), g)
    dwpe = c["dwpe0"].long().clone()
    dwpe[:T] += g.view(B, T, D).sum(0)
    return dwte, dwpe


# --------------------------------------------------------------------------- cross-entropy
def make_xent_logits(M, V, ld, shift=0.0, seed=8):
    """bf16 [M, ld]: 3 N(0, 1) + shift in the V valid columns, 1e4 in the pad columns (a pad column that is
    read dominates its row).  Seed 8: the logits of test_kernel_edges_gpu.py::test_xent_shifted_logits."""
    logits = randn_bf16(M, ld, scale=3.0, shift=shift, seed=seed)
    logits[:, V:] = 1e4
    return logits


@functools.lru_cache(maxsize=None)
def xent_case(M, V, ld, shift=0.0):
    """Targets: random, every 5th row ignored, row 1's in column V - 1, row 2's at the row's argmax."""
    logits = make_xent_logits(M, V, ld, shift)
    tgt = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(2))
    tgt[::5] = -1
    tgt[1] = V - 1
    tgt[2] = logits[2, :V].float().argmax()
    return {"logits": logits, "tgt": tgt, "V": V}


xent_long_logits = functools.lru_cache(maxsize=None)(make_xent_logits)


def xent_lse64(logits, V):
    return torch.logsumexp(logits[:, :V].double(), dim=1)


def lse_allow(lse64):
    """16 2^-24 max(|lse|, 1)."""
    return 16 * U * lse64.abs().clamp(min=1.0)


def xent_ref(logits, tgt, V, g):
    """fp64 from the bf16 logits: (lse [M], dlogits [M, ld] = g (softmax - onehot) on valid rows and valid
    columns, 0 elsewhere, its allowance 2^-7 |ref| + g 2^-20 (0 on ignored rows and pad columns), row
    losses lse - logit[target] (0 on ignored rows)).  g = grad_out / n_valid."""
    M, ld = logits.shape
    lse = xent_lse64(logits, V)
    valid = tgt >= 0
    t = tgt.clamp(min=0)
    d = torch.zeros(M, ld, dtype=torch.float64, device=logits.device)
    d[:, :V] = torch.exp(logits[:, :V].double() - lse[:, None])
    rows = torch.arange(M, device=logits.device)
    d[rows, t] -= 1.0
    d *= g
    d[~valid] = 0
    d[:, V:] = 0
    allow = BF_ULP * d.abs() + g * 2.0 ** -20
    allow[~valid] = 0
    allow[:, V:] = 0
    loss = torch.where(valid, lse - logits.double()[rows, t], torch.zeros_like(lse))
    return lse, d, allow, loss


def xent_fp32(logits, tgt, V, g):
    """(lse, dlogits rounded to bf16) of the same formula in plain fp32 torch."""
    M, ld = logits.shape
    x = logits[:, :V].float()
    lse = torch.logsumexp(x, dim=1)
    d = torch.zeros(M, ld)
    d[:, :V] = torch.exp(x - lse[:, None])
    d[torch.arange(M), tgt.clamp(min=0)] -= 1.0
    d *= torch.tensor(g, dtype=torch.float32)
    d[tgt < 0] = 0
    d[:, V:] = 0
    return lse, d.to(BF)
