"""The optimizer kernels of csrc/kernels/adamw.hip against references that can see a single element, on
the probes of tests/_opt_probe.py (checked in test_opt_probe_cpu.py):

1. grad_sumsq / grad_sumsq_chunks on small integers: norm[0] by value, one-hot probes at every boundary;
2. adamw_step on integer data with b1 = b2 = 0.5: moments, master and the bf16 param bit for bit, every
   buffer's gaps and margins untouched, at every chunk length where the kernel changes path;
3. adamw_step against the fp64 rule within N 2^-24 of each element's mass (N derived in _opt_probe.py),
   one step at a time from the kernel's own state, on the three clip branches;
4. the same bound in graph mode ({lr, step} from device memory), eager and on graph replays;
5. f32_to_bf16 on every rounding case.

Each toleranced check prints its violation (error / allowance) before it asserts; PERF.md, "Optimizer
probes", holds the measured ones."""
import math

import numpy as np
import pytest
import torch

import _opt_probe as P
from mingpt_distributed_amd.ops._ext import ext
from mingpt_distributed_amd.optim import CHUNK, make_chunk_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GDTYPES = [torch.float32, torch.bfloat16]


def _nan_norm():
    return torch.full((2,), math.nan, device=DEV)


# --------------------------------------------------------------------------- 1. norm census
@pytest.mark.parametrize("n", P.SUMSQ_N)
def test_grad_sumsq_census(n):
    C = ext()
    for variant in (0, 1):
        x = P.census_values(n, variant)
        norm = _nan_norm()
        C.grad_sumsq(x.to(DEV), 0.5, norm)
        P.check_norm(norm, P.sumsq_exact(x), 0.5, f"grad_sumsq n={n} variant {variant}")
    z = torch.zeros(n, device=DEV)
    for pos in P.sumsq_onehot_positions(n):
        z[pos] = 1.0
        norm = _nan_norm()
        C.grad_sumsq(z, 0.5, norm)
        assert norm.tolist() == [1.0, 0.5], (n, pos, norm.tolist())
        z[pos] = 0.0


def _norm_tables():
    lens = P.hand_table(P.SUMSQ_CHUNK_LENS)
    one = P.hand_table((1027,))
    many = P.hand_table(P.SUMSQ_MANY)
    return {"lengths": (lens.starts, lens.lens, lens.n), "one": (one.starts, one.lens, one.n),
            "many": (many.starts, many.lens, many.n)}


@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("which", ["lengths", "one", "many", "pieces"])
def test_grad_sumsq_chunks_census(which, gdtype):
    C = ext()
    if which == "pieces":  # the table the optimizer builds: a full chunk and a 4100-element rest
        n = 8 + CHUNK + 4100 + 8
        t = make_chunk_table([(8, 8 + CHUNK + 4100, 0.0, None)], DEV, n)
        cs, cl = t.start, t.len
        starts, lens = t.start.tolist(), t.len.tolist()
    else:
        starts, lens, n = _norm_tables()[which]
        cs = torch.tensor(starts, dtype=torch.int64, device=DEV)
        cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    end = max(s + L for s, L in zip(starts, lens))
    inside = torch.from_numpy(P.inside_mask(starts, lens, n))
    for variant in (0, 1):
        x = torch.where(inside, P.census_values(n, variant), torch.tensor(P.GAP_GRAD))
        norm = _nan_norm()
        C.grad_sumsq_chunks(cs, cl, x.to(DEV).to(gdtype), 0.5, norm, end)
        P.check_norm(norm, P.sumsq_exact(x[inside]), 0.5, f"grad_sumsq_chunks {which} variant {variant}")
    z = torch.zeros(n, device=DEV, dtype=gdtype)
    for pos, want in P.chunk_onehot_positions(starts, lens):
        z[pos] = 1.0
        norm = _nan_norm()
        C.grad_sumsq_chunks(cs, cl, z, 0.5, norm, end)
        assert norm.tolist() == [float(want), 0.5 * want], (which, pos, norm.tolist())
        z[pos] = 0.0


# --------------------------------------------------------------------------- 2. adamw census
def _census_launch(kind, gdtype, packed, fused=False):
    C = ext()
    t = P.hand_table(P.ADAMW_LENS)
    c = P.adamw_census(kind, t, packed)
    hp = P.CENSUS_A if kind == "a" else P.CENSUS_B
    cs, cl, cw, cm = P.table_tensors(t, DEV, c["wd"])
    master = torch.from_numpy(c["master"]).to(DEV)
    param = P.as_bf16(np.full(c["n"], P.SENT_PARAM, dtype=np.uint16)).to(DEV)
    grad = torch.from_numpy(c["grad"]).to(DEV).to(gdtype)
    grad0 = grad.clone()
    m, v = torch.from_numpy(c["m"]).to(DEV), torch.from_numpy(c["v"]).to(DEV)
    C.adamw_step(cs, cl, cw, cm if packed else None, master, param, grad, m, v, _nan_norm(), hp.lr, hp.b1, hp.b2,
                 hp.eps, hp.step, hp.grad_scale, hp.clip, t.end, c["mend"], grad if fused else None)
    what = f"census {kind} {gdtype} packed={packed}"
    P.same_bits(m, c["want_m"], what + ": m")
    P.same_bits(v, c["want_v"], what + ": v")
    P.same_bits(master, c["want_master"], what + ": master")
    P.same_bits(param, c["want_param"], what + ": param")
    return c, grad0, grad


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("kind", ["a", "b"])
def test_adamw_census(kind, gdtype, packed):
    _, grad0, grad = _census_launch(kind, gdtype, packed)
    P.same_bits(grad, grad0, "the gradients are read only")


def test_adamw_census_fused_zero_grad():
    c, grad0, grad = _census_launch("a", torch.float32, False, fused=True)
    inside = torch.from_numpy(c["inside"]).to(DEV)
    want = torch.where(inside, torch.zeros_like(grad0), grad0)
    P.same_bits(grad, want, "the gradients: zero inside the chunks, untouched outside")


# --------------------------------------------------------------------------- 3. fp64 bound
def _masked(d, mask):
    return {k: x[mask] for k, x in d.items()}


def _bound_step(C, t, pieces, packed, state, g, wd, inside, hp, norm0, what, host_args=None, launch=None,
                pow_ulps=P.POW_ULPS_HOST):
    """One kernel step from `state` = (master, param, m, v), checked against ref64 of the state before it.
    launch: runs the step instead of a direct call (a graph replay); host_args: (lr, step) the call is given
    instead of hp's (graph mode reads the real ones from device memory)."""
    master, param, m, v = state
    before = (master.clone(), P.moments_to_flat(pieces, m, P.BOUND_N), P.moments_to_flat(pieces, v, P.BOUND_N))
    if launch is None:
        lr, step = (hp.lr, hp.step) if host_args is None else host_args
        norm = torch.tensor([norm0, math.nan], device=DEV)
        C.adamw_step(t.start, t.len, t.wd, t.mstart if packed else None, master, param, g, m, v, norm, lr, hp.b1,
                     hp.b2, hp.eps, step, hp.grad_scale, hp.clip, t.end, t.mend)
    else:
        launch()
    ref = _masked(P.ref64(before[0], g.float(), before[1], before[2], wd, norm0, hp), inside)
    got = _masked({"p": master, "m": P.moments_to_flat(pieces, m, P.BOUND_N),
                   "v": P.moments_to_flat(pieces, v, P.BOUND_N)}, inside)
    N = P.units(hp, norm0, pow_ulps)
    viol = P.violations(got, ref, N)
    print(f"{what}: violation (error / allowance) m {viol['m']:.3f} of N = {N['m']:g}, v {viol['v']:.3f} of "
          f"N = {N['v']:g}, master {viol['p']:.3f} of N = {N['p']:.1f}")
    P.same_bits(master[~inside], before[0][~inside], what + ": master outside the pieces")
    P.same_bits(param[inside], master[inside].to(P.BF), what + ": param is the bf16 rounding of master")
    assert (param[~inside].view(torch.int16) == P.SENT_PARAM).all(), what + ": param outside the pieces"
    return viol


def _bound_setup(cs, gdtype, packed):
    pieces, nm = P.bound_pieces(cs, packed)
    t = make_chunk_table(pieces, DEV, P.BOUND_N, nm if packed else None)
    master0, grads = P.bound_data(cs, gdtype == torch.bfloat16)
    wd = P.wd_elements(pieces, P.BOUND_N).to(DEV)
    inside = torch.zeros(P.BOUND_N, dtype=torch.bool, device=DEV)
    for a, b, _, _ in pieces:
        inside[a:b] = True

    def fresh():
        return (master0.to(DEV), P.as_bf16(np.full(P.BOUND_N, P.SENT_PARAM, dtype=np.uint16)).to(DEV),
                torch.zeros(nm, device=DEV), torch.zeros(nm, device=DEV))

    return pieces, t, [g.to(DEV) for g in grads], wd, inside, fresh


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("set_name", list(P.CASE_SETS))
def test_adamw_within_fp64_bound(set_name, gdtype, packed):
    C = ext()
    cs = P.CASE_SETS[set_name]
    pieces, t, grads, wd, inside, fresh = _bound_setup(cs, gdtype, packed)
    worst = {}
    for branch in P.CLIP_BRANCHES:
        state = fresh()
        for step, g in zip(P.BOUND_STEPS, grads):
            hp, norm0 = P.bound_hp(cs, step, branch)
            what = f"{set_name} {str(gdtype)[6:]} {'packed' if packed else 'flat'} clip {branch} step {step}"
            worst[what] = _bound_step(C, t, pieces, packed, state, g, wd, inside, hp, norm0, what)
    bad = {k: v for k, v in worst.items() if not max(v.values()) <= 1.0}
    assert not bad, bad


# --------------------------------------------------------------------------- 4. graph mode
def test_adamw_graph_mode_reads_lr_and_step_from_the_device():
    C = ext()
    cs = P.TRAINING
    pieces, t, grads, wd, inside, fresh = _bound_setup(cs, torch.float32, False)
    state = fresh()
    master, param, m, v = state
    g = grads[0]
    hp_dev = torch.tensor([1e-3, 7.0], dtype=torch.float32, device=DEV)
    clip, norm0 = P.CLIP_BRANCHES["active"]
    norm = torch.tensor([norm0, math.nan], device=DEV)

    def hp_of(lr, step):
        return P.HP(lr, cs.b1, cs.b2, cs.eps, step, 0.5, clip)

    worst = {}
    C.set_graph_state(None, hp_dev)
    try:
        # the host's lr and step are wrong on purpose: the kernel must not use them
        worst["eager (1e-3, 7)"] = _bound_step(C, t, pieces, False, state, g, wd, inside, hp_of(1e-3, 7), norm0,
                                               "graph mode eager (1e-3, 7)", host_args=(0.0, 1),
                                               pow_ulps=P.POW_ULPS_DEVICE)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            C.adamw_step(t.start, t.len, t.wd, None, master, param, g, m, v, norm, 0.0, cs.b1, cs.b2, cs.eps, 1, 0.5,
                         clip, t.end, t.mend)
    finally:
        C.set_graph_state(None, None)

    def replay():
        graph.replay()
        torch.cuda.synchronize()

    for lr, step in ((1e-3, 8), (5e-4, 9)):
        hp_dev.copy_(torch.tensor([lr, float(step)], dtype=torch.float32))
        what = f"graph mode replay ({lr:g}, {step})"
        worst[what] = _bound_step(C, t, pieces, False, state, g, wd, inside, hp_of(lr, step), norm0, what,
                                  launch=replay, pow_ulps=P.POW_ULPS_DEVICE)
    del graph
    bad = {k: x for k, x in worst.items() if not max(x.values()) <= 1.0}
    assert not bad, bad


# --------------------------------------------------------------------------- 5. f32_to_bf16
def test_f32_to_bf16_every_rounding_case():
    C = ext()
    bits = P.f2bf_bits()
    src = torch.from_numpy(bits.view(np.float32).copy()).to(DEV)
    dst = torch.zeros(src.numel(), dtype=P.BF, device=DEV)
    C.f32_to_bf16(src, dst)
    nan = torch.isnan(src)
    assert int(nan.sum()) == 5 * 2 * 127 + 4 * 2  # exponent 255 and a nonzero mantissa
    assert torch.isnan(dst[nan]).all()
    ok = (~nan).cpu().numpy()
    P.same_bits(dst[~nan], P.bf16_bits(bits[ok]), "f32_to_bf16 against round-to-nearest-even")
    P.same_bits(dst[~nan], src[~nan].to(P.BF), "f32_to_bf16 against torch's conversion")


def test_f32_to_bf16_second_grid_trip():
    C = ext()
    bits = P.f2bf_long_bits()
    src = torch.from_numpy(bits.view(np.float32).copy()).to(DEV)
    dst = P.as_bf16(np.full(bits.size + 8, P.SENT_PARAM, dtype=np.uint16)).to(DEV)
    C.f32_to_bf16(src, dst[:bits.size])
    P.same_bits(dst[:bits.size], P.bf16_bits(bits), "f32_to_bf16 n = 2^20 + 5")
    assert (dst[bits.size:].view(torch.int16) == P.SENT_PARAM).all()
