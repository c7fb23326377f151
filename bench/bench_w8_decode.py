#!/usr/bin/env python
"""W8 decode against the bf16 decode of the same snapped model, interleaved in one process.

Two models of a GPT-2 preset (--model-type) with the same random weights, both snapped by
``quantize_int8_``; one keeps the mark and decodes on ``gemv_w8``, the other has it taken off and
decodes on the bf16 ``gemv`` (the parent's kernels on the same numbers).  Each keeps its own decode
state and captured graphs, so the timed calls alternate without a re-capture.  Per batch size of
--batches: greedy ``generate`` of --new tokens after --prompt, --reps alternating runs, median and
range; the tokens are asserted equal.  --ragged B: one ``generate_batch`` case on B prompts spread over
--min-len .. --max-len.  --kernels: the four projection shapes of a block and the LM head alone, both
kernels, each captured as a graph over rotating copies of the weight (so no copy is re-read from a
cache: --rotate-mb of weights per graph), microseconds per launch and GB/s of weight bytes.
--logits: largest and RMS difference of the last-position logits before and after the snap, and the
per-weight report.  One JSON line per result."""
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


def ab(cases, reps):
    with torch.no_grad():
        outs = {k: fn() for k, fn in cases.items()}  # warm-up: states, twins, graph capture
        outs = {k: fn() for k, fn in cases.items()}
        times = {k: [] for k in cases}
        for _ in range(reps):
            for k, fn in cases.items():
                times[k].append(timed(fn)[1])
    return outs, times


def kernels(a, cfg):
    from mingpt_distributed_amd.ops._ext import ext
    from mingpt_distributed_amd.ops.quant import dequantize_rows, quantize_rows

    C = ext()
    D, V = cfg.n_embed, 50257
    shapes = [("c_attn", 3 * D, D, 1, True), ("attn.c_proj", D, D, 3, False), ("mlp.c_fc", 4 * D, D, 2, True),
              ("mlp.c_proj", D, 4 * D, 3, False), ("lm_head", V, D, 0, True)]
    for B in map(int, a.batches.split(",")):
        for name, N, K, epi, ln in shapes:
            g = torch.Generator().manual_seed(N + K)
            q, s = quantize_rows((torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16))
            copies = max(2, min(64, -(-a.rotate_mb * (1 << 20) // (2 * N * K))))
            qs = [q.cuda().clone() for _ in range(copies)]
            ws = [dequantize_rows(q, s, torch.bfloat16).cuda() for _ in range(copies)]
            s = s.cuda()
            x = torch.randn(B, K, generator=g).to(torch.bfloat16).cuda()
            ld = (N + 7) // 8 * 8
            bias = None if name == "lm_head" else torch.randn(N, generator=g).to(torch.bfloat16).cuda()
            resid = torch.randn(B, N, generator=g).to(torch.bfloat16).cuda() if epi == 3 else None
            lw = torch.ones(K, dtype=torch.bfloat16, device="cuda") if ln else None
            lb = torch.zeros(K, dtype=torch.bfloat16, device="cuda") if ln else None
            runs = {"bf16": lambda: [C.gemv(x, w, epi, bias, resid, ld, lw, lb, 1e-5) for w in ws],
                    "w8": lambda: [C.gemv_w8(x, qq, s, epi, bias, resid, ld, lw, lb, 1e-5) for qq in qs]}
            assert all(torch.equal(u[:, :N], v[:, :N]) for u, v in zip(runs["bf16"](), runs["w8"]()))
            graphs = {}
            for k, fn in runs.items():
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k]):
                    keep = fn()
            us = {k: [] for k in graphs}
            for _ in range(a.reps):
                for k, gr in graphs.items():
                    gr.replay()  # warm
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(10):
                        gr.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    us[k].append(e0.elapsed_time(e1) * 1e3 / (10 * copies))
            med = {k: statistics.median(v) for k, v in us.items()}
            print(json.dumps({"metric": "skinny GEMM us per launch, weights from HBM", "model": a.model_type, "B": B,
                              "weight": name, "N": N, "K": K, "epi": epi, "layernorm": ln, "copies": copies,
                              "bf16_us": round(med["bf16"], 2), "w8_us": round(med["w8"], 2),
                              "bf16_GBps": round(2 * N * K / med["bf16"] / 1e3, 1),
                              "w8_GBps": round(N * K / med["w8"] / 1e3, 1),
                              "w8_over_bf16_time": round(med["w8"] / med["bf16"], 3)}), flush=True)
            del graphs, keep, qs, ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-type", default="gpt2", choices=["gpt2", "gpt2-medium", "gpt2-large", "gpt2-xl"])
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ragged", type=int, default=0, help="also time generate_batch on this many mixed-length prompts")
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--kernels", action="store_true", help="time the projection and LM-head kernels alone instead")
    ap.add_argument("--rotate-mb", type=int, default=600)
    ap.add_argument("--logits", action="store_true", help="report the logits change of the snap and the per-weight report")
    a = ap.parse_args()
    from mingpt_distributed_amd.models import GPT, GPTConfig

    cfg = GPTConfig(model_type=a.model_type, vocab_size=50257, block_size=1024).resolve()
    if a.kernels:
        return kernels(a, cfg)
    torch.manual_seed(0)
    w8 = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    if a.logits:
        idx = torch.randint(0, 50257, (4, 64), generator=torch.Generator().manual_seed(7)).cuda()
        with torch.no_grad():
            before = w8(idx)[0][:, -1].float()
    report = w8.quantize_int8_()
    if a.logits:
        with torch.no_grad():
            d = w8(idx)[0][:, -1].float() - before
        by_kind = {}
        for k, v in report.items():
            kind = k.split(".", 3)[-1] if k.startswith("transformer.h.") else k
            by_kind[kind] = max(by_kind.get(kind, 0.0), v)
        print(json.dumps({"metric": "last-position logits, snapped - original (random init)", "model": a.model_type,
                          "max_abs": round(float(d.abs().max()), 5), "rms": round(float(d.pow(2).mean().sqrt()), 5),
                          "logits_std": round(float(before.std()), 4),
                          "worst_relative_rounding_error_by_weight": {k: round(v, 6) for k, v in by_kind.items()},
                          "bound": round(1 / 127, 6)}), flush=True)
    bf = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    bf.load_state_dict(w8.state_dict())  # the same snapped weights, not marked: the bf16 kernels
    assert w8._mg_w8 and not bf.__dict__.get("_mg_w8", False)
    for B in map(int, a.batches.split(",")):
        idx = torch.randint(0, 50257, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        outs, times = ab({"bf16": lambda: bf.generate(idx, a.new), "w8": lambda: w8.generate(idx, a.new)}, a.reps)
        assert torch.equal(outs["bf16"], outs["w8"]), "W8 decode differs from the bf16 decode of the snapped model"
        res = {"metric": "greedy decode tokens/s, bf16 vs W8 on the same snapped model", "model": f"{a.model_type} (random init)",
               "batch": B, "prompt": a.prompt, "new_tokens": a.new, "reps": a.reps, "tokens_equal": True}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(B * a.new / statistics.median(ts), 1)
            res[k + "_tok_s_range"] = [round(B * a.new / max(ts), 1), round(B * a.new / min(ts), 1)]
        res["w8_over_bf16"] = round(statistics.median(times["bf16"]) / statistics.median(times["w8"]), 3)
        print(json.dumps(res), flush=True)
    if a.ragged:
        B, g = a.ragged, torch.Generator().manual_seed(a.ragged)
        lens = [round(a.min_len + (a.max_len - a.min_len) * i / max(B - 1, 1)) for i in range(B)]
        prompts = [torch.randint(0, 50257, (n,), generator=g).cuda() for n in lens]
        outs, times = ab({"bf16": lambda: bf.generate_batch(prompts, a.new)[0],
                          "w8": lambda: w8.generate_batch(prompts, a.new)[0]}, a.reps)
        assert torch.equal(outs["bf16"], outs["w8"])
        res = {"metric": "ragged greedy generate_batch tokens/s, bf16 vs W8", "model": f"{a.model_type} (random init)",
               "batch": B, "lengths": lens, "new_tokens": a.new, "reps": a.reps, "tokens_equal": True}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(B * a.new / statistics.median(ts), 1)
            res[k + "_tok_s_range"] = [round(B * a.new / max(ts), 1), round(B * a.new / min(ts), 1)]
        res["w8_over_bf16"] = round(statistics.median(times["bf16"]) / statistics.median(times["w8"]), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
