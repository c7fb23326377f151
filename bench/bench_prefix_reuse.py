#!/usr/bin/env python
"""Prefix reuse (``generate(reuse_cache=True)``): time to the first token on a decode state that already
holds the first P tokens of the prompt, against the fresh prefill of the default path.

Per model (--model-types, random weights), batch (--batches) and (P, Tq) of --cases, in one process: the
state is primed with ``generate(idx[:, :P], 1, reuse_cache=True)`` (untimed), then ``generate(idx, 1, ...)``
on the P + Tq tokens is timed, device-synchronised, with ``reuse_cache=True`` and then -- primed the same
way, so both see the same allocator and cache state -- with ``reuse_cache=False``; --reps alternating
pairs after --warmup untimed ones, median and range.  ``reused`` is what the state reports for the timed
reuse call (P: the extension ran; 0: ``generation._reuse_pays`` chose the prefill -- --ungated switches that
rule off).  The first tokens of the two paths are compared (``same_first``; they
may differ only at a near-tie).  One JSON line per case.  A GPU is required.

--kv-int8: the same protocol on the KV8 state (``kv_cache="int8"`` on every call, ``_mg_kv8_cache``; the
extension is ``attention_extend_kv8``), gated by ``generation._reuse_kv8_pays``; the comparison is the fresh
prefill of that same state.  --kernels: instead, the attention calls alone -- ``attention_extend_kv8``
against ``attention_extend`` at each (B, P, Tq) with the model's heads, the three launches of one layer by
device events, --reps alternating pairs."""
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


def main(argv=None):
    from mingpt_distributed_amd.models import GPT, GPTConfig

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-types", default="gpt2,gpt2-xl")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--cases", default="900:20,512:128,64:8,1:256", help="P:Tq pairs")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ungated", action="store_true",
                    help="take every common prefix, also where generation._reuse_pays would prefill (the "
                         "measurement the rule was read from)")
    ap.add_argument("--kv-int8", action="store_true", help="the KV8 state: kv_cache='int8' on every call")
    ap.add_argument("--kernels", action="store_true",
                    help="time attention_extend_kv8 against attention_extend alone (no model is run)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_prefix_reuse: needs a GPU")
    if a.ungated:
        from mingpt_distributed_amd.models import generation

        generation._REUSE_GATE = generation._REUSE_KV8_GATE = False
    kw = {"kv_cache": "int8"} if a.kv_int8 else {}
    slot = "_mg_kv8_cache" if a.kv_int8 else "_mg_decode_cache"
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")]
    if a.kernels:
        return kernels(a, cases)
    for mt in a.model_types.split(","):
        torch.manual_seed(0)
        model = GPT(GPTConfig(model_type=mt, vocab_size=50257, block_size=1024, embed_drop=0.0, resid_drop=0.0,
                              attn_drop=0.0), verbose=False).cuda().to(torch.bfloat16).eval()
        for B in (int(b) for b in a.batches.split(",")):
            for P, Tq in cases:
                idx = torch.randint(0, 50257, (B, P + Tq), generator=torch.Generator().manual_seed(P + Tq)).cuda()
                times = {True: [], False: []}
                first, reused = {}, None
                with torch.no_grad():
                    for rep in range(a.warmup + a.reps):
                        for reuse in (True, False):
                            model.generate(idx[:, :P], 1, reuse_cache=True, **kw)  # the state holds the P tokens
                            out, dt = timed(lambda: model.generate(idx, 1, reuse_cache=reuse, **kw))
                            if reuse:
                                reused = model.__dict__[slot].reused
                            first[reuse] = out[:, -1]
                            if rep >= a.warmup:
                                times[reuse].append(dt * 1e3)
                med = {k: statistics.median(v) for k, v in times.items()}
                print(json.dumps({
                    "bench": "prefix_reuse", "kv_cache": "int8" if a.kv_int8 else "bf16", "model": mt, "B": B, "P": P, "Tq": Tq, "reused": reused,
                    "fresh_ms": round(med[False], 3), "reuse_ms": round(med[True], 3),
                    "fresh_range_ms": [round(min(times[False]), 3), round(max(times[False]), 3)],
                    "reuse_range_ms": [round(min(times[True]), 3), round(max(times[True]), 3)],
                    "speedup": round(med[False] / med[True], 3),
                    "same_first": bool(torch.equal(first[True], first[False]))}), flush=True)
        del model
        torch.cuda.empty_cache()


def kernels(a, cases):
    """One layer's attention calls on random caches: each call is its append, attention and combine launches."""
    from mingpt_distributed_amd.models import GPTConfig
    from mingpt_distributed_amd.ops._ext import ext

    C = ext()
    for mt in a.model_types.split(","):
        cfg = GPTConfig(model_type=mt, vocab_size=50257, block_size=1024).resolve()
        H, D = cfg.n_head, cfg.n_embed
        for B in (int(b) for b in a.batches.split(",")):
            for P, Tq in cases:
                g = torch.Generator().manual_seed(P + Tq)
                new = torch.randn(B * Tq, 3 * D, generator=g).to(torch.bfloat16).cuda()
                cache = torch.randn(B, 1024, 3 * D, generator=g).to(torch.bfloat16).cuda()
                kq = torch.randint(-127, 128, (B, 2, H, 1024, D // H), generator=g, dtype=torch.int8).cuda()
                ks = torch.full((B, 2, H, 1024), 2.0 ** -6, device="cuda")
                calls = {"bf16": lambda: C.attention_extend(new, cache, H, P),
                         "int8": lambda: C.attention_extend_kv8(new, kq, ks, H, P)}
                times = {k: [] for k in calls}
                for rep in range(a.warmup + a.reps):
                    for k, fn in calls.items():
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                        ev[0].record()
                        for _ in range(20):
                            fn()
                        ev[1].record()
                        torch.cuda.synchronize()
                        if rep >= a.warmup:
                            times[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / 20)
                med = {k: statistics.median(v) for k, v in times.items()}
                print(json.dumps({
                    "bench": "prefix_reuse_kernels", "model": mt, "B": B, "H": H, "hd": D // H, "base": P, "Tq": Tq,
                    "splits": C.attention_extend_splits(B, Tq, H, P),
                    "extend_us": round(med["bf16"], 2), "extend_kv8_us": round(med["int8"], 2),
                    "extend_range_us": [round(min(times["bf16"]), 2), round(max(times["bf16"]), 2)],
                    "extend_kv8_range_us": [round(min(times["int8"]), 2), round(max(times["int8"]), 2)]}), flush=True)


if __name__ == "__main__":
    main()
