#!/usr/bin/env python
"""Bit parity of the training GEMM (csrc/kernels/gemm.hip) between two builds of the extension.

    MINGPT_EXT_SO=build/ab/<sha>/_C.so python scripts/gemm_parity.py --out DIR_A
    python scripts/gemm_parity.py --out DIR_B               (the tree's own _C.so)
    python scripts/gemm_parity.py --compare DIR_A DIR_B     (no GPU: raw bytes of every array)

One process per build (``scripts/build_ab_base.sh`` makes the other one).  Inputs are the probes of
``tests/_gemm_probe.py`` at its SHAPES, under each tile configuration (gemm_set_variant 0, 1, 5, 6).
Every case is one whose result does not depend on the arrival order of an atomic add, so two builds
of one algorithm must agree in every byte; one .npy per result (bf16 as int16):

* NT, random operands: epilogues 0, 1, 2 (both planes), 3 at p = 0 and at p = 0.1 with a fixed seed,
  4, 6 (both planes); epilogue 0 with a padded row stride (ld = N + 8, pad columns included);
* NN, random operands: epilogues 0, 4 and 7;
* TN, random operands at Mr = 136 (one split: read-modify-write), integer operands at Mr = 520 and
  2056 (2 and 7 splits: integer sums are exact in any atomic order);
* the fused dbias, random operands at M = 120 (one row tile in every configuration: each column gets
  one atomic add and the order inside a tile is fixed, which pins whether rounded or unrounded
  outputs are summed): NT and NN epilogue 4, NN epilogue 7; and integer operands at the full shapes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

BF = torch.bfloat16
VARIANTS = (0, 1, 5, 6)
DBIAS_M = 120
SEED = 1234


def run(out):
    import _gemm_probe as P
    from mingpt_distributed_amd.ops import gemm as G
    from mingpt_distributed_amd.ops._ext import ext

    C = ext()
    os.makedirs(out, exist_ok=True)
    n = [0]

    def save(name, **arrays):
        for k, t in arrays.items():
            t = t.detach().contiguous()
            t = t.view(torch.int16) if t.dtype == BF else t
            np.save(os.path.join(out, f"{name}.{k}.npy"), t.cpu().numpy())
            n[0] += 1

    def dev(c, keys=("a", "b_nk", "b_kn", "bias", "resid", "aux")):
        return {k: (c[k] if torch.is_tensor(c[k]) else P.bf(c[k])).cuda() for k in keys}

    def dbias_cases(tag, d, db0):
        """Epilogue 4 (NT, NN) and 7 (NN) with the fused column sums added into a copy of db0."""
        plane = P.rowmajor_to_frag_plane(d["aux"], pad=1.0)
        for name, fn in (("nt.epi4", lambda db: G.gemm_nt(d["a"], d["b_nk"], epi="gelu_bwd", aux=d["aux"], dbias=db)),
                         ("nn.epi4", lambda db: G.gemm_nn(d["a"], d["b_kn"], epi="gelu_bwd", aux=d["aux"], dbias=db)),
                         ("nn.epi7", lambda db: G.gemm_nn(d["a"], d["b_kn"], epi="gelu_bwd", aux=plane, dbias=db,
                                                          aux_frag=True))):
            db = db0.clone()
            save(f"{tag}.{name}", y=fn(db), dbias=db)

    for v in VARIANTS:
        C.gemm_set_variant(v)
        for M, N, K in P.SHAPES:
            tag = f"v{v}.{M}x{N}x{K}"
            d = dev(P.rand_case(M, N, K))
            a, b, bn, bias, resid, aux = (d[k] for k in ("a", "b_nk", "b_kn", "bias", "resid", "aux"))
            save(f"{tag}.nt.epi0", y=G.gemm_nt(a, b))
            save(f"{tag}.nt.epi0_ld", y=G.gemm_nt(a, b, ld=N + 8))
            save(f"{tag}.nt.epi1", y=G.gemm_nt(a, b, bias=bias, epi="bias"))
            pre = torch.zeros(M, N, dtype=BF, device="cuda")
            save(f"{tag}.nt.epi2", y=G.gemm_nt(a, b, bias=bias, epi="gelu", pre_out=pre), pre=pre)
            save(f"{tag}.nt.epi3_p0", y=G.gemm_nt(a, b, bias=bias, epi="resid", resid=resid, p=0.0))
            save(f"{tag}.nt.epi3_p01", y=G.gemm_nt(a, b, bias=bias, epi="resid", resid=resid, p=0.1, seed=SEED))
            save(f"{tag}.nt.epi4", y=G.gemm_nt(a, b, epi="gelu_bwd", aux=aux))
            fr = torch.zeros(G.frag_aux_elems(M, N), dtype=BF, device="cuda")
            save(f"{tag}.nt.epi6", y=G.gemm_nt(a, b, bias=bias, epi="gelu", pre_out=fr, frag=True), plane=fr)
            save(f"{tag}.nn.epi0", y=G.gemm_nn(a, bn))
            save(f"{tag}.nn.epi4", y=G.gemm_nn(a, bn, epi="gelu_bwd", aux=aux))
            save(f"{tag}.nn.epi7", y=G.gemm_nn(a, bn, epi="gelu_bwd", aux=P.rowmajor_to_frag_plane(aux, pad=1.0),
                                               aux_frag=True))
            dbias_cases(f"{tag}.dbias_rand_M{DBIAS_M}", dev(P.rand_case(DBIAS_M, N, K)),
                        torch.zeros(N, device="cuda"))
            ci = P.int_case(M, N, K)
            dbias_cases(f"{tag}.dbias_int", dev(ci), torch.from_numpy(ci["dbias0"].astype(np.float32)).cuda())
        for N, K in P.TN_OUT:
            c = P.tn_rand_case(P.TN_MR[0], N, K)
            acc = c["c0"].cuda()
            G.gemm_tn_acc(c["a"].cuda(), c["b"].cuda(), acc)
            save(f"v{v}.tn_rand.Mr{P.TN_MR[0]}.{N}x{K}", c=acc)
            for Mr in P.TN_MR[1:]:
                c = P.tn_int_case(Mr, N, K)
                acc = torch.from_numpy(c["c0"].astype(np.float32)).cuda()
                G.gemm_tn_acc(P.bf(c["a"]).cuda(), P.bf(c["b"]).cuda(), acc)
                save(f"v{v}.tn_int.Mr{Mr}.{N}x{K}", c=acc)
        torch.cuda.synchronize()
    C.gemm_set_variant(0)
    print(f"gemm_parity: wrote {n[0]} arrays to {out} "
          f"(extension: {os.environ.get('MINGPT_EXT_SO') or 'in-tree'})", flush=True)


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(f"gemm_parity: different or empty file sets ({len(fa)} vs {len(fb)})")
        return 1
    bad = [f for f in fa if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
    for f in bad:
        print(f"  DIFFERS: {f}")
    print(f"gemm_parity: {len(fa) - len(bad)} of {len(fa)} arrays byte-equal between {a} and {b}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="run the cases on the loaded extension and write the arrays here")
    ap.add_argument("--compare", nargs=2, metavar="DIR", help="compare the arrays of two runs byte by byte")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not a.out:
        ap.error("--out DIR or --compare DIR_A DIR_B")
    with torch.no_grad():
        run(a.out)
