#!/usr/bin/env python
"""Time to the first token of a ``generate_batch`` turn with and without ``reuse_cache`` (ragged prefix reuse,
``_GpuCache.extend_ragged`` / ``attention_extend_ragged``) on one GPU.

A batch of B conversations whose histories are spread over ``--hist`` tokens gets a new turn of Tq tokens per row.
Before every timed call the decode state is made to hold the histories (a ``generate_batch(histories, 1,
reuse_cache=True)``, not timed); the timed call is ``generate_batch(histories + turn, 1)``, once with
``reuse_cache=True`` and once without -- the latter is the padded prefill, the path every call took before the
argument existed.  The two are interleaved after warm-up and the medians with their ranges are printed, one JSON
line per case.  Degenerate cases: ``same1`` (every row keeps one token: P_b = 1) and ``lone`` (one row with a long
history among rows with none).  The gate is off for the measurement (``--gated`` leaves it as shipped):
``generation._reuse_batch_pays`` is read from this table (PERF.md 'Prefix reuse, ragged')."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def histories(kind, B, lo, hi):
    """The rows' history lengths: spread evenly over lo..hi, one token each, or one long row among empty ones
    (a row needs a token: 1)."""
    if kind == "same1":
        return [1] * B
    if kind == "lone":
        return [hi] + [1] * (B - 1)
    return [lo + (hi - lo) * b // max(B - 1, 1) for b in range(B)]


def main(argv=None):
    from mingpt_distributed_amd.models import GPT, GPTConfig, generation

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-types", default="gpt2,gpt2-xl")
    ap.add_argument("--batches", default="2,8")
    ap.add_argument("--hist", default="100:900", help="lo:hi of the history lengths")
    ap.add_argument("--turns", default="5,20,100", help="new tokens per row")
    ap.add_argument("--kinds", default="spread,same1,lone")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gated", action="store_true", help="leave generation._REUSE_BATCH_GATE as shipped")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_prefix_reuse_batch: needs a GPU")
    if not a.gated:
        generation._REUSE_BATCH_GATE = False
    lo, hi = (int(v) for v in a.hist.split(":"))
    for mt in a.model_types.split(","):
        torch.manual_seed(0)
        model = GPT(GPTConfig(model_type=mt, vocab_size=50257, block_size=1024, embed_drop=0.0, resid_drop=0.0,
                              attn_drop=0.0), verbose=False).cuda().to(torch.bfloat16).eval()
        for B in (int(b) for b in a.batches.split(",")):
            for kind in a.kinds.split(","):
                for Tq in (int(t) for t in a.turns.split(",")):
                    hist = histories(kind, B, lo, hi)
                    g = torch.Generator().manual_seed(B + Tq)
                    full = [torch.randint(0, 50257, (n + Tq,), generator=g).cuda() for n in hist]
                    held = [f[:n] for f, n in zip(full, hist)]
                    times = {True: [], False: []}
                    first, reused = {}, None
                    with torch.no_grad():
                        for rep in range(a.warmup + a.reps):
                            for reuse in (True, False):
                                model.generate_batch(held, 1, reuse_cache=True)  # the state holds the histories
                                (out, lens), dt = timed(lambda: model.generate_batch(full, 1, reuse_cache=reuse))
                                if reuse:
                                    reused = model._mg_decode_cache.reused
                                first[reuse] = out.gather(1, (lens - 1).view(-1, 1))
                                if rep >= a.warmup:
                                    times[reuse].append(dt * 1e3)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    print(json.dumps({
                        "bench": "prefix_reuse_batch", "model": mt, "B": B, "kind": kind, "hist": hist, "Tq": Tq,
                        "reused": reused, "fresh_ms": round(med[False], 3), "reuse_ms": round(med[True], 3),
                        "fresh_range_ms": [round(min(times[False]), 3), round(max(times[False]), 3)],
                        "reuse_range_ms": [round(min(times[True]), 3), round(max(times[True]), 3)],
                        "speedup": round(med[False] / med[True], 3),
                        "same_first": bool(torch.equal(first[True], first[False]))}), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
