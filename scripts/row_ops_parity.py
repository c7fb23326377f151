#!/usr/bin/env python
"""Bit parity of the logits-row ops (sample.hip, beam.hip) between two builds of the extension.

    MINGPT_EXT_SO=build/ab/<sha>/_C.so python scripts/row_ops_parity.py --out DIR_A
    python scripts/row_ops_parity.py --out DIR_B               (the tree's own _C.so)
    python scripts/row_ops_parity.py --compare DIR_A DIR_B     (no GPU: raw bytes of every array)

One process per build (``scripts/build_ab_base.sh`` makes the other one).  Every output of these
kernels is an integer sum, a maximum or a key, so nothing depends on an order and two builds of one
algorithm must agree in every byte -- the tests' tolerance bands are for the rule, not for this.
Writes one .npy per result: ``logits_lse`` with and without targets; ``sample_logits`` and
``sample_kept`` at top_k off / 40 x top_p off / 0.9 (the first with and without lse / lp);
``pick_ragged`` greedy and sampled, with and without lp, with and without a finished row;
``beam_rows`` + ``beam_merge`` at W = 1, 3, 8 on two prompts with one finished beam.  Each shape's
row 0 holds -inf entries and its last row a repeated maximum."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

SHAPES = [(1, 1000, 1000), (2, 997, 1000), (1, 9000, 9000), (3, 50257, 50264), (1, 66001, 66008)]  # rows, V, ld
SETTINGS = [(0, None), (40, None), (0, 0.9), (40, 0.9)]  # top_k, top_p


def make_logits(rows, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 3.0
    drop = torch.rand(V, generator=g) < 0.1
    drop[x[0].argmax()] = False
    x[0, drop] = float("-inf")
    x[-1, torch.randint(0, V, (3,), generator=g)] = x[-1].max()
    full = torch.full((rows, ld), float("nan"))
    full[:, :V] = x
    return full.to(torch.bfloat16).cuda()


def run(out):
    from mingpt_distributed_amd.models.generation import _ragged_words, _sample_words
    from mingpt_distributed_amd.ops._ext import ext

    C = ext()
    os.makedirs(out, exist_ok=True)
    dev = "cuda"
    n = [0]

    def save(name, **arrays):
        for k, t in arrays.items():
            np.save(os.path.join(out, f"{name}.{k}.npy"), t.detach().cpu().numpy())
            n[0] += 1

    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    for rows, V, ld in SHAPES:
        tag = f"r{rows}_V{V}"
        logits = make_logits(rows, V, ld, V)
        g = torch.Generator().manual_seed(V + 1)
        targets = torch.randint(0, V, (rows,), generator=g)
        targets[-1] = -1 if rows > 1 else targets[-1]
        lse = C.logits_lse(logits, V)
        lse_t, lp_t = C.logits_lse(logits, V, targets.cuda())
        save(f"{tag}.lse", lse=lse, lse_t=lse_t, lp_t=lp_t)
        for k, p in SETTINGS:
            st = f"{tag}.k{k}_p{p}"
            words = _sample_words(12345 + (7 << 40), 7, 0.9, k, p)
            save(f"{st}.kept", kept=C.sample_kept(logits, V, i32(words)))
            save(f"{st}.sample", tok=C.sample_logits(logits, V, i32(words)))
            pb, pos = i32(words), i32([3])
            tok = torch.full((rows,), -7, dtype=torch.long, device=dev)
            seq = torch.full((rows, 8), -3, dtype=torch.long, device=dev)
            lp = torch.full((rows, 8), 123.0, device=dev)
            C.sample_logits(logits, V, pb, pos, tok, seq, lse, lp)
            save(f"{st}.sample_lp", params=pb, pos=pos, tok=tok, seq=seq, lp=lp)
        for greedy in (True, False):
            for with_lp in (False, True):
                for fin in (False, True):
                    pb = i32(_ragged_words(99, 0.9, 40, None, 0.9))
                    pos = i32([2 + b for b in range(rows)])
                    done = i32([1 if fin and b == rows - 1 else 0 for b in range(rows)])
                    tok = torch.full((rows, 1), -7, dtype=torch.long, device=dev)
                    seq = torch.full((rows, 12), -3, dtype=torch.long, device=dev)
                    lp = torch.full((rows, 12), 123.0, device=dev)
                    C.pick_ragged(logits, V, pb, pos, done, tok, seq, greedy, *((lse, lp) if with_lp else ()))
                    save(f"{tag}.ragged_g{int(greedy)}_lp{int(with_lp)}_fin{int(fin)}", pos=pos, done=done, tok=tok,
                         seq=seq, lp=lp)
        for W in (1, 3, 8):
            R, Lh = 2 * W, 8  # two prompts; the last beam of the second is finished
            bl = logits[torch.arange(R, device=dev) % rows].contiguous()
            score = (-torch.rand(R, generator=g) * 20.0).cuda()
            fin = torch.zeros(R, dtype=torch.int32, device=dev)
            fin[-1] = 1
            ctl = i32([5, int(bl[0, :V].float().argmax()), 0, 0])  # row 0's best token is the stop token
            cand_tok = torch.full((R, W), -9, dtype=torch.int32, device=dev)
            cand_c = torch.full((R, W), 123.0, device=dev)
            blse = torch.full((R, 2), 123.0, device=dev)
            C.beam_rows(bl, V, W, score, fin, ctl, cand_tok, cand_c, blse)
            save(f"{tag}.beam_rows_W{W}", cand_tok=cand_tok, cand_c=cand_c, lse=blse)
            ln = torch.full((R,), 6, dtype=torch.int32, device=dev)
            tok = torch.full((R, 1), -7, dtype=torch.long, device=dev)
            parent = torch.full((R,), -1, dtype=torch.int32, device=dev)
            hp, ht = (torch.full((2, W, Lh), -5, dtype=torch.int32, device=dev) for _ in range(2))
            hs = torch.full((2, W, Lh), 123.0, device=dev)
            pos = i32([5])
            C.beam_merge(W, V, cand_tok, cand_c, score, fin, ln, tok, parent, hp, ht, hs, pos, ctl)
            save(f"{tag}.beam_merge_W{W}", score=score, fin=fin, len=ln, tok=tok, parent=parent, hist_parent=hp,
                 hist_tok=ht, hist_score=hs, pos=pos)
        torch.cuda.synchronize()
    print(f"row_ops_parity: wrote {n[0]} arrays to {out} "
          f"(extension: {os.environ.get('MINGPT_EXT_SO') or 'in-tree'})", flush=True)


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(f"row_ops_parity: different or empty file sets ({len(fa)} vs {len(fb)})")
        return 1
    bad = [f for f in fa if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
    print(f"row_ops_parity: {len(fa) - len(bad)} of {len(fa)} arrays byte-equal between {a} and {b}")
    for f in bad:
        print(f"  DIFFERS: {f}")
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
