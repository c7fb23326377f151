#!/usr/bin/env python
"""Shared-prefix decode (``generate(num_return_sequences=N)``) against the repeated batch
``generate(idx.repeat_interleave(N, 0))`` -- the same call on the plain decode state and kernels.

Per model (--model-types, random weights), N (--ns) and prompt length P (--prompts), B = 1, seeded sampling,
in one process: the shared path (``generation._SHARED_GATE`` forced off, so it runs at every shape) and the
repeated batch alternate, --reps pairs after --warmup untimed ones, each call device-synchronised.  Two
quantities per path, medians with ranges: ``ttft_ms``, the time of a call for one new token (prefill, first
pick), and ``tok_s``, the N * (--new - 1) tokens of the decode loop over the time a call for --new tokens
takes beyond that.  ``cache_bytes`` is ``kv_cache_nbytes`` of each path's state, ``same_rows`` the share of
rows whose tokens equal the repeated batch's (they may part at a near-tie).  One JSON line per case.  A GPU is
required.  ``--kv-int8``: both arms with ``kv_cache="int8"`` -- the shared KV8 state (``_SHARED_KV8_GATE`` off
as well, ``attention_decode_shared_kv8``) against the repeated batch on the plain KV8 state."""
import argparse
import gc
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


def main(argv=None):
    from mingpt_distributed_amd.models import GPT, GPTConfig, generation

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-types", default="gpt2,gpt2-xl")
    ap.add_argument("--ns", default="2,8,16,64")
    ap.add_argument("--prompts", default="16,128,896,900",
                    help="prompt lengths; P + --new past block_size (900 + 128) does not fit one window, and the "
                         "timed loop is then the repeated batch's sliding window on both sides")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kv-int8", action="store_true", help="kv_cache='int8' on both arms")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_shared_prefix: needs a GPU")
    generation._SHARED_GATE = generation._SHARED_KV8_GATE = False
    kw = dict(do_sample=True, seed=1234, top_k=50, **({"kv_cache": "int8"} if a.kv_int8 else {}))
    slots = ("_mg_shared_kv8_cache", "_mg_kv8_cache") if a.kv_int8 else ("_mg_shared_cache", "_mg_decode_cache")
    med = statistics.median
    for mt in a.model_types.split(","):
        torch.manual_seed(0)
        model = GPT(GPTConfig(model_type=mt, vocab_size=50257, block_size=1024, embed_drop=0.0, resid_drop=0.0,
                              attn_drop=0.0), verbose=False).cuda().to(torch.bfloat16).eval()
        for N in (int(n) for n in a.ns.split(",")):
            for P in (int(p) for p in a.prompts.split(",")):
                idx = torch.randint(0, 50257, (1, P), generator=torch.Generator().manual_seed(P)).cuda()
                rep = idx.repeat_interleave(N, 0)
                run = {"shared": lambda n: model.generate(idx, n, num_return_sequences=N, **kw),
                       "repeated": lambda n: model.generate(rep, n, **kw)}
                ttft, loop, toks = {k: [] for k in run}, {k: [] for k in run}, {}
                with torch.no_grad():
                    for r in range(a.warmup + a.reps):
                        for name, fn in run.items():
                            _, t1 = timed(lambda: fn(1))
                            toks[name], tn = timed(lambda: fn(a.new))
                            if r >= a.warmup:
                                ttft[name].append(t1 * 1e3)
                                loop[name].append(N * (a.new - 1) / (tn - t1))
                nbytes = generation.kv_cache_nbytes(model)
                rng = lambda v, d: [round(min(v), d), round(max(v), d)]
                print(json.dumps({
                    "bench": "shared_prefix", "kv_cache": kw.get("kv_cache", "bf16"), "model": mt, "N": N, "P": P, "new": a.new,
                    **{f"{k}_ttft_ms": round(med(ttft[k]), 3) for k in run},
                    **{f"{k}_ttft_range_ms": rng(ttft[k], 3) for k in run},
                    **{f"{k}_tok_s": round(med(loop[k]), 1) for k in run},
                    **{f"{k}_tok_s_range": rng(loop[k], 1) for k in run},
                    "ttft_speedup": round(med(ttft["repeated"]) / med(ttft["shared"]), 3),
                    "loop_speedup": round(med(loop["shared"]) / med(loop["repeated"]), 3),
                    "cache_bytes": {"shared": nbytes[slots[0]], "repeated": nbytes[slots[1]]},
                    "same_rows": round(float((toks["shared"] == toks["repeated"]).all(1).float().mean()), 3)}),
                    flush=True)
        del model
        gc.collect()  # a model and its decode states refer to each other
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
