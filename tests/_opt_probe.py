"""Probe inputs, references and allowances for the optimizer kernels of csrc/kernels/adamw.hip
(grad_sumsq, grad_sumsq_chunks, adamw_step, f32_to_bf16), built on the CPU with numpy and torch from
fixed hashes and seeds.

tests/test_adamw_exact_gpu.py runs them through the kernels; tests/test_opt_probe_cpu.py checks the
probes themselves (the census expectations against `ref64`, `ref64` against torch.optim.AdamW, and the
two conditions on the allowance below).

* Census cases.  Every input is a small integer: exact in bf16 and fp32, every sum of squares below
  2^24 (exact in any summation order), and with b1 = b2 = 0.5 the moments are exact whatever the
  compiler contracts to fma.  A dropped, doubled or misplaced element is an O(1) error; everything is
  compared bit for bit, the buffers' sentinel gaps and margins included.
* `ref64`: the documented AdamW rule in fp64 on the float32 values of the hyperparameters.
* The allowance of the toleranced checks, in units of u = 2^-24 (the largest relative error of one
  correctly rounded fp32 operation).  The build uses no fast-math flag, and hipcc divides and takes
  square roots correctly rounded by default, so `/` and sqrtf cost one u each.

  Count, first order, for  gg = g gs;  m = b1 m0 + (1 - b1) gg;  v = b2 v0 + (1 - b2) gg gg;
  p = p0 decay - (step m) / (sqrtf(v) / bc2_sqrt + eps):

    c   error of gs.  Clip off or inactive: gs is grad_scale as given, c = 0.  Active: sqrtf, times
        grad_scale, plus 1e-6, clip / ., gs times coef: c = 5.
    m   gg carries c + 1; (1 - b1) is exact for b1 in [0.5, 1] (Sterbenz); the product (1 - b1) gg one
        more; b1 m0 one; the sum one on |m| <= mass.  |dm| <= (c + 3) u (|b1 m0| + |(1 - b1) g'|).
    v   ((1 - b2) gg) gg: 2 (c + 1) + 2; b2 v0 one; the sum one.  |dv| <= (2 c + 5) u v  (no
        cancellation: every term is positive).
    e1  error of bc1 = 1 - powf(b1, t): a powf good to P ulps is off by 2 P u b1^t, seen from bc1 that is
        2 P b1^t / bc1, plus one for the subtraction.  Where b1^t is an fp32 number and P < 1 the power is
        exact.  (Step 2 at b1 = 0.9: 2 * 0.81 / 0.19 = 8.5 P.)
    e2  error of bc2_sqrt = sqrtf(1 - powf(b2, t)): half of the same count for b2, plus one.
    p   decay = 1 - lr wd: two; p0 decay: one; the final subtraction one on |p| <= |p0 decay| + |update|:
        4 on the decay term.  The update: step = lr / bc1: 1 + e1; times m: 1 + (c + 3); sqrtf(v):
        1 + (2 c + 5) / 2; / bc2_sqrt: 1 + e2; + eps: 1; the quotient: 1; the final subtraction: 1:
        12.5 + 2 c + e1 + e2, which is the larger of the two and the count for p.
        (Where b1 m0 and (1 - b1) g' cancel, dm is relative to the mass and not to |m|; the update is
        then small against lr, and |p0 decay| in the bound carries it.  Condition 1 checks that on the
        data, not only on paper.)

  P: glibc documents its powf at 0.82 ulp (POW_ULPS_HOST); the device's (graph mode) is taken at 1 ulp
  (POW_ULPS_DEVICE), so it is never assumed exact.

  The allowance is N = HEADROOM * count with HEADROOM = 2: the count is first order and follows one
  order of evaluation; the kernel may contract to fma or associate (1 - b2) gg gg the other way, and a
  legitimate float32 evaluation must use at most half the allowance (condition 1 of
  test_opt_probe_cpu.py).  Condition 2 there: every documented way of getting the rule wrong (`MUTANTS`)
  exceeds the allowance at least 4 times on one of the case sets.  N is never raised past that."""
import math
from fractions import Fraction
from typing import NamedTuple

import numpy as np
import torch

BF = torch.bfloat16
U = 2.0 ** -24
HEADROOM = 2.0
POW_ULPS_HOST = 0.82
POW_ULPS_DEVICE = 1.0
GRID_TRIP = 1024 * 256 * 4  # elements one trip of grad_sumsq's grid covers

SUMSQ_N = (1, 3, 4, 5, 1024, GRID_TRIP, GRID_TRIP + 4 * 300 + 3)
SUMSQ_CHUNK_LENS = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 2048, 2051, 32767, 32768)
SUMSQ_MANY = tuple(1 + k % 9 for k in range(300))  # more chunks than sumsq_final_kernel has threads
ADAMW_LENS = (1, 2, 3, 4, 5, 7, 8, 1020, 1023, 1024, 1025, 1028, 1029, 2047, 2048, 2049, 2052, 3071, 3072,
              3073, 3076, 4099, 32767, 32768)

GAP_GRAD = 1024.0    # gradient value between chunks: exact in bf16; one counted adds 2^20
SENT_MASTER = 7777.0
SENT_MOMENT = -555.0  # a negative v that is read gives NaN
SENT_PARAM = 0x5A5A   # bf16 bits


def f32(x):
    """x rounded to float32, as a Python float: what a kernel argument declared `float` holds."""
    return float(np.float32(x))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def bf16_bits(bits32):
    """uint32 fp32 bit patterns -> uint16 bf16 bit patterns, round to nearest even (non-NaN inputs)."""
    b = bits32.astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def as_bf16(bits16):
    """uint16 numpy bit patterns -> torch bf16 tensor."""
    return torch.from_numpy(bits16.astype(np.uint16).view(np.int16).copy()).view(BF)


# --------------------------------------------------------------------------- norm census
def census_values(n, variant):
    """float32 [n] from {+-1, +-2, +-3}: two unrelated assignments (variant 0 / 1)."""
    rng = np.random.default_rng(7_654_321 * (variant + 1) + n)
    return torch.from_numpy(rng.choice(np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32), size=n))


def sumsq_exact(x):
    """Sum of squares of integer-valued x as a Python int (int64 arithmetic)."""
    v = x.double().round().long()
    return int((v * v).sum())


def sumsq_onehot_positions(n):
    n4 = 4 * (n // 4)
    return sorted({p for p in (0, n4 - 1, n4, n - 1, GRID_TRIP - 1, GRID_TRIP) if 0 <= p < n})


def check_norm(norm, sumsq, grad_scale, what):
    """norm[0] is the exact integer, norm[1] within 2 fp32 ulps of sqrt(norm[0]) grad_scale."""
    got0, got1 = float(norm[0]), float(norm[1])
    assert got0 == float(sumsq), f"{what}: sum of squares {got0} for {sumsq}"
    want1 = math.sqrt(sumsq) * grad_scale
    assert abs(got1 - want1) <= 2 * ulp32(want1), f"{what}: norm {got1} for {want1}"


# --------------------------------------------------------------------------- hand-built chunk tables
class Table(NamedTuple):
    starts: tuple   # multiples of 4
    lens: tuple
    mstarts: tuple  # packed moment offsets: multiples of 4, never equal to the chunk's start
    n: int          # flat buffer size (a margin after the last chunk)
    nm: int         # packed moment buffer size
    end: int        # one past the last element a chunk touches
    mend: int


def _up4(x):
    return (x + 3) // 4 * 4


def hand_table(lens, lead=8, gap=4, mlead=12, mgap=8, tail=8):
    """One chunk per length, 4..7 elements between chunks in the flat buffer (8..11 between their packed
    moments), a margin before the first and after the last."""
    starts, mstarts, pos, mpos = [], [], lead, mlead
    for L in lens:
        starts.append(pos)
        mstarts.append(mpos)
        end, mend = pos + L, mpos + L
        pos, mpos = _up4(end + gap), _up4(mend + mgap)
    return Table(tuple(starts), tuple(lens), tuple(mstarts), end + tail, mend + tail, end, mend)


def inside_mask(starts, lens, n):
    mask = np.zeros(n, dtype=bool)
    for s, L in zip(starts, lens):
        mask[s:s + L] = True
    return mask


def table_tensors(t, device, wd=None):
    """(chunk_start, chunk_len, chunk_wd, moment_start) device tensors of a Table."""
    wd = [0.0] * len(t.lens) if wd is None else wd
    return (torch.tensor(t.starts, dtype=torch.int64, device=device),
            torch.tensor(t.lens, dtype=torch.int32, device=device),
            torch.tensor(wd, dtype=torch.float32, device=device),
            torch.tensor(t.mstarts, dtype=torch.int64, device=device))


def chunk_onehot_positions(starts, lens):
    """[(position, expected sum)]: the first and last element of the first and last chunk (1) and the
    element just outside each (0)."""
    out = {}
    for s, L in ((starts[0], lens[0]), (starts[-1], lens[-1])):
        out.update({s: 1, s + L - 1: 1})
    for s, L in ((starts[0], lens[0]), (starts[-1], lens[-1])):
        out.setdefault(s - 1, 0)
        out.setdefault(s + L, 0)
    return sorted(out.items())


# --------------------------------------------------------------------------- adamw census
class HP(NamedTuple):
    lr: float
    b1: float
    b2: float
    eps: float
    step: int
    grad_scale: float
    clip: float


CENSUS_A = HP(lr=0.0, b1=0.5, b2=0.5, eps=1e-8, step=1, grad_scale=0.5, clip=0.0)
CENSUS_B = HP(lr=0.5, b1=0.5, b2=0.5, eps=1e-8, step=1, grad_scale=0.5, clip=0.0)


def _hash(i, a, b, c):
    return i * a + (i >> 2) * b + (i >> 10) * c


def census_grad(n):
    """float32 [n]: multiples of 4, |g| <= 252, a function of the flat position; elements 1, 4, 1024 and
    2048 apart differ (checked in test_opt_probe_cpu.py)."""
    i = np.arange(n, dtype=np.int64)
    return (4 * (_hash(i, 1, 7, 13) % 127 - 63)).astype(np.float32)


def census_moments(nm):
    """(m0, v0) float32 [nm]: even integers, functions of the moment position; |m0| <= 60, 0 <= v0 <= 192."""
    j = np.arange(nm, dtype=np.int64)
    return ((2 * (_hash(j, 3, 5, 11) % 61 - 30)).astype(np.float32),
            (2 * (_hash(j, 5, 3, 7) % 97)).astype(np.float32))


ROUNDING_LOWS = (0x7FFF, 0x8000, 0x8001)


def census_master_rounding(n):
    """float32 [n] in +-[2, 4): the low half cycles through 0x7FFF, 0x8000, 0x8001 (just below, at and just
    above the bf16 tie) over even and odd bf16 mantissas; the upper half depends on the position."""
    i = np.arange(n, dtype=np.int64)
    low = np.array(ROUNDING_LOWS, dtype=np.int64)[(i + (i >> 2)) % 3]
    hi = 0x4000 + (_hash(i, 3, 1, 5) % 128)  # bit 0: even / odd mantissa
    sign = ((_hash(i, 1, 1, 1) % 5) == 0).astype(np.int64) << 31
    return (sign | (hi << 16) | low).astype(np.uint32).view(np.float32)


def census_master_ints(n):
    """float32 [n]: nonzero multiples of 4, |.| <= 256."""
    i = np.arange(n, dtype=np.int64)
    k = _hash(i, 5, 9, 3) % 128 - 64
    return (4 * np.where(k == 0, 64, k)).astype(np.float32)


def adamw_census(kind, table, packed):
    """Inputs and expected outputs of one census launch, numpy arrays over whole buffers (the gaps and
    margins hold sentinels, and the expected outputs keep them).

    kind "a": CENSUS_A, hashed gradients and moments, rounding-probe master: m = m0 / 2 + g' / 2,
    v = v0 / 2 + g'^2 / 2 with g' = g / 2, master unchanged, param its bf16 rounding.
    kind "b": CENSUS_B, g = 0, m0 = 0, wd alternating 0.5 / 0: master 0.75 master or master, m = 0,
    v = v0 / 2."""
    n, nm = table.n, (table.nm if packed else table.n)
    mst = table.mstarts if packed else table.starts
    ins = inside_mask(table.starts, table.lens, n)
    mins = inside_mask(mst, table.lens, nm)
    wd = [0.5 if c % 2 == 0 else 0.0 for c in range(len(table.lens))]
    wd_elem = np.zeros(n, dtype=np.float32)
    for s, L, w in zip(table.starts, table.lens, wd):
        wd_elem[s:s + L] = w
    m0f, v0f = census_moments(nm)
    if kind == "a":
        master = census_master_rounding(n)
        grad = census_grad(n)
    else:
        master = census_master_ints(n)
        grad = np.zeros(n, dtype=np.float32)
        m0f = np.zeros(nm, dtype=np.float32)
    master = np.where(ins, master, np.float32(SENT_MASTER)).astype(np.float32)
    grad = np.where(ins, grad, np.float32(GAP_GRAD)).astype(np.float32)
    m0 = np.where(mins, m0f, np.float32(SENT_MOMENT)).astype(np.float32)
    v0 = np.where(mins, v0f, np.float32(SENT_MOMENT)).astype(np.float32)
    # the moments of chunk c sit at mst[c] ..., its gradients at starts[c] ...
    gm = np.zeros(nm, dtype=np.float64)
    for s, ms, L in zip(table.starts, mst, table.lens):
        gm[ms:ms + L] = grad[s:s + L].astype(np.float64) / 2
    want_m = np.where(mins, m0.astype(np.float64) / 2 + gm / 2, SENT_MOMENT).astype(np.float32)
    want_v = np.where(mins, v0.astype(np.float64) / 2 + gm * gm / 2, SENT_MOMENT).astype(np.float32)
    if kind == "a":
        want_master = master.copy()
    else:
        want_master = np.where(ins, master * (1 - 0.5 * wd_elem), master).astype(np.float32)
    want_param = np.where(ins, bf16_bits(want_master.view(np.uint32)), np.uint16(SENT_PARAM)).astype(np.uint16)
    return {"n": n, "nm": nm, "mend": table.mend if packed else table.end, "wd": wd, "wd_elem": wd_elem,
            "inside": ins, "minside": mins, "mstarts": mst,
            "master": master, "grad": grad, "m": m0, "v": v0,
            "want_master": want_master, "want_param": want_param, "want_m": want_m, "want_v": want_v}


def same_bits(got, want, what):
    """Bitwise equality of a tensor with a numpy array or tensor of the same element width."""
    if isinstance(want, np.ndarray):
        want = torch.from_numpy(np.ascontiguousarray(want).view({2: np.int16, 4: np.int32}[want.dtype.itemsize]).copy())
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    g, w = got.detach().contiguous().view(it), want.to(got.device).contiguous().view(it)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} for {tuple(w.shape)}"
    bad = g != w
    if bad.any():
        first = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {first}: bits "
                             f"{int(g[first]) & 0xFFFFFFFF:#x} for {int(w[first]) & 0xFFFFFFFF:#x}")


# --------------------------------------------------------------------------- the rule in fp64
MUTANTS = ("decay_after", "eps_in_sqrt", "eps_before_bc", "bc2_not_sqrt", "no_bc1", "prev_m", "clip_no_scale",
           "clip_always")


def clip_active(hp, norm0):
    """Whether the rule scales the gradients: clip > 0 and clip / (sqrt(norm0) grad_scale + 1e-6) < 1."""
    if not f32(hp.clip) > 0:
        return False
    return f32(hp.clip) / (math.sqrt(norm0) * f32(hp.grad_scale) + f32(1e-6)) < 1


def ref64(p0, g, m0, v0, wd, norm0, hp, mutant=None):
    """One AdamW step in fp64 (torch, on the inputs' device) on the float32 values of the hyperparameters:
    global-norm clip (coef = clip / (sqrt(norm0) grad_scale + 1e-6), applied when coef < 1 and clip > 0;
    norm0 is not read when clip <= 0), decoupled decay p (1 - lr wd), both bias corrections, eps added after
    sqrt(v) / sqrt(bc2).  wd: per element.  Returns p, m, v and the masses the allowances scale with.
    `mutant`: one of MUTANTS, a wrong rule (for the tests of the allowance, never for a kernel check)."""
    assert mutant is None or mutant in MUTANTS
    lr, b1, b2, eps, gs, clip = (f32(x) for x in (hp.lr, hp.b1, hp.b2, hp.eps, hp.grad_scale, hp.clip))
    t = float(hp.step)
    p0, g, m0, v0, wd = (torch.as_tensor(x).double() for x in (p0, g, m0, v0, wd))
    if clip > 0:
        tn = math.sqrt(norm0) * (1.0 if mutant == "clip_no_scale" else gs)
        coef = clip / (tn + f32(1e-6))
        if coef < 1 or mutant == "clip_always":
            gs = gs * coef
    gg = g * gs
    ma, mb = b1 * m0, (1 - b1) * gg
    m = ma + mb
    v = b2 * v0 + (1 - b2) * gg * gg
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    decay = 1 - lr * wd
    den = v.sqrt() / math.sqrt(bc2) + eps
    if mutant == "eps_in_sqrt":
        den = (v / bc2 + eps).sqrt()
    elif mutant == "eps_before_bc":
        den = (v.sqrt() + eps) / math.sqrt(bc2)
    elif mutant == "bc2_not_sqrt":
        den = v.sqrt() / bc2 + eps
    upd = (lr if mutant == "no_bc1" else lr / bc1) * (m0 if mutant == "prev_m" else m) / den
    p = (p0 - upd) * decay if mutant == "decay_after" else p0 * decay - upd
    return {"p": p, "m": m, "v": v, "p_mass": (p0 * decay).abs() + upd.abs(), "m_mass": ma.abs() + mb.abs(),
            "v_mass": v}


def _pow_units(b, t, pow_ulps):
    """Relative error of 1 - powf(b, t) in units of u."""
    b = Fraction(f32(b))
    exact = b ** int(t)
    pw = float(exact)
    try:
        representable = Fraction(float(np.float32(pw))) == exact
    except (OverflowError, ValueError):
        representable = False
    e = 0.0 if (representable and pow_ulps < 1) else 2 * pow_ulps * pw / (1 - pw)
    return e + 1


def units(hp, norm0, pow_ulps=POW_ULPS_HOST):
    """The allowances N of one step, {"m", "v", "p"}, in units of u times the element's mass: HEADROOM
    times the count of the module docstring."""
    c = 5 if clip_active(hp, norm0) else 0
    e1 = _pow_units(hp.b1, hp.step, pow_ulps)
    e2 = _pow_units(hp.b2, hp.step, pow_ulps) / 2 + 1
    return {"m": HEADROOM * (c + 3), "v": HEADROOM * (2 * c + 5), "p": HEADROOM * (12.5 + 2 * c + e1 + e2)}


def violations(got, ref, n_units):
    """{"m", "v", "p"}: the worst |got - ref| / (N u mass) over the elements (NaN counts as infinite; an
    element of mass 0 must be equal)."""
    out = {}
    for k in ("m", "v", "p"):
        r = ref[k]
        err = (torch.as_tensor(got[k]).to(r.device).double() - r).abs()
        allow = n_units[k] * U * ref[k + "_mass"]
        ratio = torch.where(allow > 0, err / allow, torch.where(err == 0, torch.zeros_like(err),
                                                                torch.full_like(err, math.inf)))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        out[k] = float(ratio.max())
    return out


def restate32(p0, g, m0, v0, wd, norm0, hp, fma=False):
    """The kernel's expression in float32 numpy, every operation rounded; fma=True: b m0 + (.) and
    p0 decay - (.) rounded once (the product and the sum formed in fp64)."""
    F, D = np.float32, np.float64
    p0, g, m0, v0, wd = (np.asarray(x, dtype=F) for x in (p0, g, m0, v0, wd))
    lr, b1, b2, eps, gs, clip = (F(x) for x in (hp.lr, hp.b1, hp.b2, hp.eps, hp.grad_scale, hp.clip))
    one, t = F(1), F(hp.step)
    bc1 = one - np.power(b1, t)
    bc2_sqrt = np.sqrt(one - np.power(b2, t))
    if clip > 0:
        tn = np.sqrt(F(norm0)) * gs
        coef = clip / (tn + F(1e-6))
        if coef < 1:
            gs = gs * coef
    step = lr / bc1
    decay = one - lr * wd
    gg = g * gs
    tm, tv = (one - b1) * gg, (one - b2) * gg * gg
    if fma:
        m = (D(b1) * m0.astype(D) + tm.astype(D)).astype(F)
        v = (D(b2) * v0.astype(D) + tv.astype(D)).astype(F)
    else:
        m, v = b1 * m0 + tm, b2 * v0 + tv
    q = step * m / (np.sqrt(v) / bc2_sqrt + eps)
    p = (p0.astype(D) * decay.astype(D) - q.astype(D)).astype(F) if fma else p0 * decay - q
    assert m.dtype == F and v.dtype == F and p.dtype == F and q.dtype == F
    return {"p": torch.from_numpy(p), "m": torch.from_numpy(m), "v": torch.from_numpy(v)}


# --------------------------------------------------------------------------- the toleranced cases
BOUND_N = 200_000
BOUND_PIECES = ((0, 40_003, 0.1), (40_008, 105_549, 0.0), (105_552, 105_553, 0.1), (105_556, 199_999, 0.0))
BOUND_STEPS = (1, 2, 1000)
NORM_ACTIVE = 4.0 ** 4  # sqrt = 16, times grad_scale 0.5: 8 > clip = 1


class CaseSet(NamedTuple):
    name: str
    lr: float
    b1: float
    b2: float
    eps: float
    wd: tuple       # the decaying pieces' weight decay, and the others'
    g_scale: float  # gradient magnitude


TRAINING = CaseSet("training", 1e-3, 0.9, 0.95, 1e-8, (0.1, 0.0), 1.0)
STRESS = CaseSet("stress", 0.25, 0.5, 0.75, 2.0 ** -10, (0.1, 0.0), 2.0 ** -9)
CASE_SETS = {"training": TRAINING, "stress": STRESS}
# clip branches: (clip, norm[0] handed in): active, inactive, off (norm is NaN and must not be read)
CLIP_BRANCHES = {"active": (1.0, NORM_ACTIVE), "inactive": (1e6, NORM_ACTIVE), "off": (0.0, math.nan)}


def bound_pieces(cs, packed):
    """pieces for optim.make_chunk_table: [(start, end, wd, moment_start)], odd tails; and the moment
    buffer's size (packed: the pieces one after another, each start rounded up to 4)."""
    out, mpos = [], 0
    for k, (a, b, _) in enumerate(BOUND_PIECES):
        out.append((a, b, cs.wd[k % 2], mpos if packed else None))
        mpos = _up4(mpos + b - a)
    return out, (mpos if packed else BOUND_N)


def bound_hp(cs, step, branch):
    clip, norm0 = CLIP_BRANCHES[branch]
    return HP(cs.lr, cs.b1, cs.b2, cs.eps, step, 0.5, clip), norm0


def bound_data(cs, bf16_grads):
    """master [n] ~ N(0, 1) and one gradient [n] per entry of BOUND_STEPS, ~ g_scale N(0, 1) (rounded to
    bf16 first when the kernel reads bf16 gradients), float32 torch tensors."""
    gen = torch.Generator().manual_seed(20_240 + len(cs.name))
    master = torch.randn(BOUND_N, generator=gen)
    grads = [torch.randn(BOUND_N, generator=gen) * cs.g_scale for _ in BOUND_STEPS]
    if bf16_grads:
        grads = [x.to(BF) for x in grads]
    return master, grads


def moments_to_flat(pieces, buf, n):
    """The (packed) moment buffer laid out at the flat positions (0 outside the pieces)."""
    out = torch.zeros(n, dtype=buf.dtype, device=buf.device)
    for a, b, _, ma in pieces:
        ma = a if ma is None else ma
        out[a:b] = buf[ma:ma + b - a]
    return out


def wd_elements(pieces, n):
    out = torch.zeros(n, dtype=torch.float32)
    for a, b, wd, _ in pieces:
        out[a:b] = wd
    return out


# --------------------------------------------------------------------------- f32_to_bf16
F2BF_LOWS = (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def f2bf_bits():
    """uint32 [5 * 65536]: every upper half with each of F2BF_LOWS."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    return np.concatenate([hi | np.uint32(lo) for lo in F2BF_LOWS])


def f2bf_long_bits():
    """uint32 [GRID_TRIP + 5]: the non-NaN patterns of f2bf_bits, repeated in a shuffled order."""
    bits = f2bf_bits()
    bits = bits[~np.isnan(bits.view(np.float32))]
    idx = np.random.default_rng(11).integers(0, bits.size, size=GRID_TRIP + 5)
    return bits[idx]
