#!/usr/bin/env python
"""Bit parity of the decode projections (gemv.hip, gemm_rows.hip) between two builds of the extension.

    MINGPT_EXT_SO=build/ab/<sha>/_C.so python scripts/decode_proj_parity.py --out DIR_A
    python scripts/decode_proj_parity.py --out DIR_B               (the tree's own _C.so)
    python scripts/decode_proj_parity.py --compare DIR_A DIR_B     (no GPU: raw bytes of every array)

One process per build (``scripts/build_ab_base.sh`` makes the other one).  Nothing in these kernels
depends on an arrival order, so two builds of one algorithm must agree in every byte -- the tests'
tolerances are for the device's tanh, not for this.  Writes one .npy per result (bf16 as int16):
``gemv`` at B = 1..8 x epilogue 0..3 on each path -- one column per wave, long rows, wide (the last
shape with a padded ldy) -- the fused LayerNorm at K = 768, 1024, 1032 and 1600 on the one-column
and the wide path, the wide path with the fused argmax (y, keys, position); ``gemm_rows`` at
M = 1, 9, 16, 17, 33, 48, 64 x epilogue 0..3."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

BF = torch.bfloat16
GEMV_SHAPES = {  # path: (N, K, ldy)
    "col": [(100, 64, 0), (768, 3072, 0), (23, 4096, 0)],
    "long": [(23, 4104, 0), (1600, 6400, 0), (100, 8192, 0)],
    "wide": [(8200, 64, 0), (16400, 64, 0), (8208, 1032, 0), (8193, 4096, 0), (8200, 8, 8208), (50257, 768, 0)],
}
LN_K = [768, 1024, 1032, 1600]
ROWS_M = [1, 9, 16, 17, 33, 48, 64]
ROWS_SHAPES = [(40, 48), (136, 4096), (136, 8192)]


def bf(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).cuda()


def run(out):
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

    def operands(rows, N, K, ld):
        ld = ld or N
        resid = torch.zeros(rows, ld, dtype=BF, device="cuda")
        resid[:, :N] = bf(rows, N, seed=K + 3)
        return bf(rows, K, seed=K + rows), bf(N, K, scale=0.05, seed=K + N + 1), bf(N, seed=K + 2), resid

    for path, shapes in GEMV_SHAPES.items():
        for N, K, ld in shapes:
            for B in range(1, 9):
                x, w, bias, resid = operands(B, N, K, ld)
                for epi in range(4):
                    y = C.gemv(x, w, epi, bias if epi else None, resid if epi == 3 else None, ld)
                    save(f"gemv.{path}.N{N}_K{K}.B{B}.epi{epi}", y=y[:, :N])
        torch.cuda.synchronize()
    for K in LN_K:
        lw, lb = bf(K, scale=0.2, seed=K + 5) + 1.0, bf(K, scale=0.2, seed=K + 6)
        for path, N in (("col", 100), ("wide", 8200)):
            for B in range(1, 9):
                x, w, bias, _ = operands(B, N, K, 0)
                save(f"gemv_ln.{path}.N{N}_K{K}.B{B}", y=C.gemv(x, w, 1, bias, None, 0, lw, lb, 1e-5))
    for N, K in ((8200, 64), (50257, 768)):
        ld = (N + 7) // 8 * 8
        for B in range(1, 9):
            x, w, _, _ = operands(B, N, K, 0)
            part = torch.full((B, C.gemv_argmax_groups(N, B)), -1, dtype=torch.long, device="cuda")
            pos = torch.full((1,), 5, dtype=torch.int32, device="cuda")
            y = C.gemv(x, w, 0, None, None, ld, None, None, 1e-5, part, pos)
            save(f"gemv_argmax.N{N}_K{K}.B{B}", y=y[:, :N], part=part, pos=pos)
    for N, K in ROWS_SHAPES:
        for M in ROWS_M:
            x, w, bias, resid = operands(M, N, K, 0)
            for epi in range(4):
                y = C.gemm_rows(x, w, epi, bias if epi else None, resid if epi == 3 else None, 0)
                save(f"gemm_rows.N{N}_K{K}.M{M}.epi{epi}", y=y)
    torch.cuda.synchronize()
    print(f"decode_proj_parity: wrote {n[0]} arrays to {out} "
          f"(extension: {os.environ.get('MINGPT_EXT_SO') or 'in-tree'})", flush=True)


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(f"decode_proj_parity: different or empty file sets ({len(fa)} vs {len(fb)})")
        return 1
    bad = [f for f in fa if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
    for f in bad:
        print(f"  DIFFERS: {f}")
    print(f"decode_proj_parity: {len(fa) - len(bad)} of {len(fa)} arrays byte-equal between {a} and {b}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="run the ops on the loaded extension and write the arrays here")
    ap.add_argument("--compare", nargs=2, metavar="DIR", help="compare the arrays of two runs byte by byte")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    with torch.no_grad():
        run(a.out)
