#!/usr/bin/env python
"""Decode throughput at 8..64 rows on random weights of a GPT-2 preset: greedy ``generate`` (B prompts
of 32 tokens), greedy ``generate_batch`` (B prompts spread over 16..256 tokens) and ``generate_beam``
(prompts x beams = 8, 16, 16, 32, 32 rows), NEW (default 128) new tokens, median and range of REPS
(default 3) timed calls after a warm-up call.  The route past 8 rows is the environment's
MINGPT_ROWS_GEMM (default on: the rows GEMM, gemm_rows.hip; 0: the MFMA GEMM), so an A/B is two
processes of one tree.  One JSON line per point.

    python bench/bench_decode_rows.py MODEL_TYPE [rect,ragged,beam] [8,9,16,32,64]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mingpt_distributed_amd.models import GPT, GPTConfig  # noqa: E402
from mingpt_distributed_amd.models import generation as gen  # noqa: E402

mt = sys.argv[1]
modes = sys.argv[2].split(",") if len(sys.argv) > 2 else ["rect", "ragged", "beam"]
batches = [int(b) for b in (sys.argv[3].split(",") if len(sys.argv) > 3 else "8,9,16,32,64".split(","))]
NEW, REPS = int(os.environ.get("NEW", "128")), int(os.environ.get("REPS", "3"))
torch.manual_seed(0)
model = GPT(GPTConfig(model_type=mt, vocab_size=50257, block_size=1024), verbose=False).cuda().to(torch.bfloat16).eval()
tag = {"model": mt, "rows_gemm": gen._ROWS_GEMM, "new": NEW}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def report(what, rows, tokens, fn, **kw):
    with torch.no_grad():
        fn()
        ts = [timed(fn) for _ in range(REPS)]
    print(json.dumps(dict(tag, case=what, rows=rows, tok_s=round(tokens / statistics.median(ts), 1),
                          tok_s_range=[round(tokens / max(ts), 1), round(tokens / min(ts), 1)],
                          us_per_step=round(statistics.median(ts) / NEW * 1e6, 1), **kw)), flush=True)


for B in batches:
    g = torch.Generator().manual_seed(B)
    if "rect" in modes:
        idx = torch.randint(0, 50257, (B, 32), generator=g).cuda()
        report("generate", B, B * NEW, lambda: model.generate(idx, NEW))
    if "ragged" in modes:
        lens = [round(16 + (256 - 16) * i / max(B - 1, 1)) for i in range(B)]
        mixed = [torch.randint(0, 50257, (n,), generator=g).cuda() for n in lens]
        report("generate_batch mixed 16..256", B, B * NEW, lambda: model.generate_batch(mixed, NEW)[0])
if "beam" in modes:
    for P, W in ((2, 4), (4, 4), (2, 8), (8, 4), (4, 8)):
        idx = torch.randint(0, 50257, (P, 32), generator=torch.Generator().manual_seed(P)).cuda()
        report("generate_beam", P * W, P * NEW, lambda: model.generate_beam(idx, NEW, W)[0], prompts=P, beams=W)
