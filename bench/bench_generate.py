#!/usr/bin/env python
"""Greedy-decode throughput (BASELINE config #4, the generate.ipynb path) on random weights of a
GPT-2 preset (--model-type, default gpt2 = 124M): this framework's ``GPT.generate`` (prefill once
on the gfx950 kernels, then one-token steps against the KV cache with the decode-attention
kernel) vs the reference's algorithm (``/root/reference/mingpt/model.py:322-356``: re-run the full forward over the whole prefix for
every new token, no cache) in stock PyTorch bf16 (autocast + SDPA).  Prints one JSON line per B.
``--int8``: the model is snapped by ``GPT.quantize_int8_`` after it is built, so decode steps of up to 8
rows read int8 weights (bench/bench_w8_decode.py times that against bf16, interleaved)."""
import argparse
import json
import os
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


def ragged(model, a):
    """Greedy tokens/s of ``generate_batch`` per batch size B: (a) B prompts of --prompt tokens each,
    next to the rectangular ``generate`` on the same prompts; (b) B prompts spread evenly over
    --min-len .. --max-len tokens; (c) the prompts of (b) as B sequential B = 1 ``generate`` calls.
    Every case is warmed up, then the cases are timed --reps times in turn; the median is reported
    with the spread.  Tokens counted: B * --new generated tokens per case."""
    import statistics

    for B in map(int, a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        equal = torch.randint(0, 50257, (B, a.prompt), generator=g).cuda()
        lens = [round(a.min_len + (a.max_len - a.min_len) * i / max(B - 1, 1)) for i in range(B)]
        mixed = [torch.randint(0, 50257, (n,), generator=g).cuda() for n in lens]
        # separate models for the B-row and the one-row states: a model keeps one decode state, and
        # alternating batch sizes on it would re-allocate and re-capture inside the timed window
        solo = type(model)(model.config, verbose=False).cuda().to(torch.bfloat16).eval()
        solo.load_state_dict(model.state_dict())
        if model.__dict__.get("_mg_w8"):  # --int8: the one-row model decodes on int8 weights too
            solo.quantize_int8_()
        cases = {
            "a_equal_generate_batch": lambda: model.generate_batch(list(equal), a.new)[0],
            "a_equal_generate_rectangular": lambda: model.generate(equal, a.new),
            "b_mixed_generate_batch": lambda: model.generate_batch(mixed, a.new)[0],
            "c_mixed_sequential_b1": lambda: [solo.generate(p[None], a.new) for p in mixed],
        }
        with torch.no_grad():
            for fn in cases.values():  # warm-up at the timed shapes (kernels, states, graph capture)
                fn()
            assert torch.equal(cases["a_equal_generate_batch"](), cases["a_equal_generate_rectangular"]())
            got = cases["b_mixed_generate_batch"]()
            for b, row in enumerate(cases["c_mixed_sequential_b1"]()):
                same = torch.equal(row[0], got[b, :lens[b] + a.new])
                if not same:  # B-row and one-row GEMMs may round differently: report, do not hide
                    print(json.dumps({"note": "mixed row differs from its B = 1 run", "row": b}), flush=True)
            times = {k: [] for k in cases}
            for _ in range(a.reps):
                for k, fn in cases.items():
                    times[k].append(timed(fn)[1])
        res = {"metric": "ragged greedy decode tokens/s", "model": f"{a.model_type} (random init)", "batch": B,
               "equal_prompt": a.prompt, "mixed_lengths": lens, "new_tokens": a.new, "reps": a.reps}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(B * a.new / statistics.median(ts), 1)
            res[k + "_tok_s_range"] = [round(B * a.new / max(ts), 1), round(B * a.new / min(ts), 1)]
        res["b_over_c"] = round(statistics.median(times["c_mixed_sequential_b1"]) /
                                statistics.median(times["b_mixed_generate_batch"]), 2)
        res["a_batch_over_rectangular"] = round(statistics.median(times["a_equal_generate_rectangular"]) /
                                                statistics.median(times["a_equal_generate_batch"]), 3)
        print(json.dumps(res), flush=True)


def logprobs(model, a):
    """Tokens/s of the same call without and with ``return_logprobs=True`` per batch size B:
    ``generate`` on B prompts of --prompt tokens (greedy, or with --sample [--seed] sampled), and
    with --ragged ``generate_batch`` on B prompts spread over --min-len .. --max-len instead.  Both
    cases are warmed up (each has its own captured loop), checked to give the same tokens, then
    timed --reps times in turn; the median is reported with the spread."""
    import statistics

    kw = {}
    if a.sample:
        kw = dict(do_sample=True, top_k=a.top_k or None, top_p=a.top_p, seed=a.seed)
    for B in map(int, a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        if a.ragged:
            lens = [round(a.min_len + (a.max_len - a.min_len) * i / max(B - 1, 1)) for i in range(B)]
            prompts = [torch.randint(0, 50257, (n,), generator=g).cuda() for n in lens]
            plain = lambda: model.generate_batch(prompts, a.new, **kw)[0]
            with_lp = lambda: model.generate_batch(prompts, a.new, return_logprobs=True, **kw)[0]
        else:
            lens = [a.prompt] * B
            idx = torch.randint(0, 50257, (B, a.prompt), generator=g).cuda()
            plain = lambda: model.generate(idx, a.new, **kw)
            with_lp = lambda: model.generate(idx, a.new, return_logprobs=True, **kw)[0]
        cases = {"plain": plain, "logprobs": with_lp}  # each returns the tokens
        with torch.no_grad():
            for fn in cases.values():  # warm-up at the timed shapes (kernels, states, graph capture)
                fn()
            if a.seed is not None or not a.sample:  # torch's global generator does not repeat
                assert torch.equal(cases["plain"](), cases["logprobs"]())
            times = {k: [] for k in cases}
            for _ in range(a.reps):
                for k, fn in cases.items():
                    times[k].append(timed(fn)[1])
        res = {"metric": "decode tokens/s without / with return_logprobs", "model": f"{a.model_type} (random init)",
               "batch": B, "entry": "generate_batch" if a.ragged else "generate", "prompt_lengths": lens,
               "new_tokens": a.new, "sample": bool(a.sample), "top_k": a.top_k if a.sample else None,
               "top_p": a.top_p if a.sample else None, "seed": a.seed, "reps": a.reps}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(B * a.new / statistics.median(ts), 1)
            res[k + "_tok_s_range"] = [round(B * a.new / max(ts), 1), round(B * a.new / min(ts), 1)]
            res[k + "_ms_per_step"] = round(statistics.median(ts) / a.new * 1e3, 4)
        res["logprobs_over_plain_time"] = round(statistics.median(times["logprobs"]) /
                                                statistics.median(times["plain"]), 4)
        print(json.dumps(res), flush=True)


def process(model, a):
    """Tokens/s of ``generate`` with the logits processors off against on per batch size B, greedy
    and seeded sampling (--top-k / --top-p / --seed, default seed 1): B prompts of --prompt tokens,
    --new tokens.  'On' is repetition_penalty 1.3, presence_penalty 0.2, frequency_penalty 0.1 and
    no_repeat_ngram_size 3.  The four cases are warmed up (each has its own captured loop), then
    timed --reps times in turn; the median is reported with the spread.  Greedy with the processors
    on also pays for leaving the LM head's fused argmax: ``greedy_logprobs`` -- the same
    construction without the process kernel, plus the lse kernel -- is timed beside it."""
    import statistics

    on = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, no_repeat_ngram_size=3)
    samp = dict(do_sample=True, top_k=a.top_k or None, top_p=a.top_p, seed=1 if a.seed is None else a.seed)
    for B in map(int, a.batches.split(",")):
        idx = torch.randint(0, 50257, (B, a.prompt), generator=torch.Generator().manual_seed(B)).cuda()
        cases = {"greedy_off": lambda: model.generate(idx, a.new),
                 "greedy_on": lambda: model.generate(idx, a.new, **on),
                 "greedy_logprobs": lambda: model.generate(idx, a.new, return_logprobs=True)[0],
                 "sample_off": lambda: model.generate(idx, a.new, **samp),
                 "sample_on": lambda: model.generate(idx, a.new, **samp, **on)}
        with torch.no_grad():
            for fn in cases.values():  # warm-up at the timed shapes (kernels, states, graph capture)
                fn()
            times = {k: [] for k in cases}
            for _ in range(a.reps):
                for k, fn in cases.items():
                    times[k].append(timed(fn)[1])
        res = {"metric": "decode tokens/s, logits processors off / on", "model": f"{a.model_type} (random init)", "batch": B,
               "prompt": a.prompt, "new_tokens": a.new, "top_k": a.top_k, "top_p": a.top_p, "seed": samp["seed"],
               "processors": on, "reps": a.reps}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(B * a.new / statistics.median(ts), 1)
            res[k + "_tok_s_range"] = [round(B * a.new / max(ts), 1), round(B * a.new / min(ts), 1)]
            res[k + "_us_per_step"] = round(statistics.median(ts) / a.new * 1e6, 1)
        med = lambda k: statistics.median(times[k])
        res["greedy_on_over_off_time"] = round(med("greedy_on") / med("greedy_off"), 4)
        res["greedy_logprobs_over_off_time"] = round(med("greedy_logprobs") / med("greedy_off"), 4)
        res["sample_on_over_off_time"] = round(med("sample_on") / med("sample_off"), 4)
        print(json.dumps(res), flush=True)


def beams(model, a):
    """Beam search per beam count W of --beams: ``generate_beam`` on --beam-prompts prompts (default
    one) of --prompt tokens, next to the same row count through
    ``generate_batch(return_logprobs=True)`` greedy (W copies of each
    prompt: the same decode step and lse kernel without the search).  Tokens/s of one prompt's best
    beam (--new tokens per call) and microseconds per step, median of --reps alternating runs with
    the spread.  --per-layer launches the cache reorder once per layer instead of once."""
    import statistics

    from mingpt_distributed_amd.models import generation as gen

    gen._BEAM_REORDER_PER_LAYER = bool(a.per_layer)
    P = a.beam_prompts  # the step runs on P * W rows (past 8: the rows GEMM, gemm_rows.hip)
    idx = torch.randint(0, 50257, (P, a.prompt), generator=torch.Generator().manual_seed(1)).cuda()
    for W in map(int, a.beams.split(",")):
        rows = [p for p in idx for _ in range(W)]
        cases = {"beam": lambda: model.generate_beam(idx, a.new, W)[0],
                 "rows_logprobs": lambda: model.generate_batch(rows, a.new, return_logprobs=True)[0]}
        with torch.no_grad():
            for fn in cases.values():  # warm-up at the timed shapes (kernels, states, graph capture)
                fn()
            times = {k: [] for k in cases}
            for _ in range(a.reps):
                for k, fn in cases.items():
                    times[k].append(timed(fn)[1])
        res = {"metric": "beam search: best-beam tokens/s and us per step", "model": f"{a.model_type} (random init)",
               "beams": W, "prompts": P, "prompt": a.prompt, "new_tokens": a.new, "reps": a.reps,
               "reorder": "per layer" if a.per_layer else "one launch"}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(a.new / statistics.median(ts), 1)
            res[k + "_tok_s_range"] = [round(a.new / max(ts), 1), round(a.new / min(ts), 1)]
            res[k + "_us_per_step"] = round(statistics.median(ts) / a.new * 1e6, 1)
        res["beam_over_rows_time"] = round(statistics.median(times["beam"]) /
                                           statistics.median(times["rows_logprobs"]), 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default=None,
                    help="time generate_beam at these beam counts (e.g. 1,4,8) on one prompt, beside the same "
                         "row count through generate_batch(return_logprobs=True)")
    ap.add_argument("--per-layer", action="store_true", help="--beams: one cache-reorder launch per layer")
    ap.add_argument("--beam-prompts", type=int, default=1,
                    help="--beams: this many prompts per call (the step runs on prompts x beams rows)")
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--sample", action="store_true",
                    help="time do_sample=True instead (this framework only, no reference run)")
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=None, help="with --sample: nucleus filtering (default: off)")
    ap.add_argument("--seed", type=int, default=None,
                    help="with --sample: the on-device seeded sampler; omitted: torch's generator (host loop)")
    ap.add_argument("--ragged", action="store_true",
                    help="time generate_batch (this framework only): equal lengths, mixed lengths, and the "
                         "mixed prompts as sequential B = 1 generate calls")
    ap.add_argument("--min-len", type=int, default=16, help="--ragged: shortest mixed prompt")
    ap.add_argument("--max-len", type=int, default=256, help="--ragged: longest mixed prompt")
    ap.add_argument("--reps", type=int, default=5,
                    help="--ragged / --logprobs: timed repetitions per case (alternating)")
    ap.add_argument("--logprobs", action="store_true",
                    help="time the same call without and with return_logprobs=True (this framework only): "
                         "generate, greedy or with --sample [--seed]; with --ragged generate_batch")
    ap.add_argument("--process", action="store_true",
                    help="time generate with the logits processors off and on, greedy and seeded (this "
                         "framework only)")
    ap.add_argument("--int8", action="store_true",
                    help="quantize_int8_ the model after building it (weight-only int8 decode)")
    ap.add_argument("--model-type", default="gpt2", choices=["gpt2", "gpt2-medium", "gpt2-large", "gpt2-xl"],
                    help="the preset whose shape is timed, on random weights (default: gpt2, 124M)")
    a = ap.parse_args()
    from mingpt_distributed_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    cfg = GPTConfig(model_type=a.model_type, vocab_size=50257, block_size=1024)
    ours = GPT(cfg, verbose=False)
    ours = ours.cuda().to(torch.bfloat16).eval()
    if a.int8:
        ours.quantize_int8_()
        a.model_type += " int8"  # the results' "model" field says so
    if a.beams:
        return beams(ours, a)
    if a.process:
        return process(ours, a)
    if a.logprobs:
        return logprobs(ours, a)
    if a.ragged:
        return ragged(ours, a)
    if a.sample:
        kw = dict(do_sample=True, top_k=a.top_k or None)
        if a.top_p is not None:
            kw["top_p"] = a.top_p
        if a.seed is not None:
            kw["seed"] = a.seed
        for B in map(int, a.batches.split(",")):
            idx = torch.randint(0, 50257, (B, a.prompt), device="cuda")
            with torch.no_grad():
                ours.generate(idx, 4, **kw)  # warm-up (kernels, caches, graph capture)
                out, t = timed(lambda: ours.generate(idx, a.new, **kw))
            assert out.shape == (B, a.prompt + a.new)
            print(json.dumps({"metric": "sampled decode tokens/s", "model": f"{a.model_type} (random init)", "batch": B,
                              "prompt": a.prompt, "new_tokens": a.new, "top_k": a.top_k, "top_p": a.top_p,
                              "seed": a.seed,
                              "tok_s": round(B * a.new / t, 1), "ms_per_step": round(t / a.new * 1e3, 4)}),
                  flush=True)
        return
    from bench.baseline_torch import GPT as TorchGPT

    ref = TorchGPT(L=cfg.n_layer, H=cfg.n_head, D=cfg.n_embed, p=0.0, attn="sdpa").cuda().eval()
    for B in map(int, a.batches.split(",")):
        idx = torch.randint(0, 50257, (B, a.prompt), device="cuda")
        with torch.no_grad():
            ours.generate(idx, 4, do_sample=False)  # warm-up (kernels, caches)
            out, t_ours = timed(lambda: ours.generate(idx, a.new, do_sample=False))

            def ref_generate():
                x = idx
                for _ in range(a.new):
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        logits, _ = ref(x[:, -1024:])
                    x = torch.cat([x, logits[:, -1, :].argmax(-1, keepdim=True)], dim=1)
                return x
            ref_generate() if a.new <= 8 else None
            _, t_ref = timed(ref_generate)
        assert out.shape == (B, a.prompt + a.new)
        print(json.dumps({"metric": "greedy decode tokens/s", "model": f"{a.model_type} (random init)", "batch": B,
                          "prompt": a.prompt, "new_tokens": a.new,
                          "ours_kv_cache_tok_s": round(B * a.new / t_ours, 1),
                          "reference_algorithm_torch_tok_s": round(B * a.new / t_ref, 1),
                          "speedup": round(t_ref / t_ours, 2)}), flush=True)


if __name__ == "__main__":
    main()
