#!/usr/bin/env python
"""Speculative greedy decoding (``GPT.generate_speculative``: n-gram drafts verified K = draft_len + 1
rows per step) next to plain greedy ``GPT.generate`` on random GPT-2 124M weights at B = 1.

Per case, warm (kernels, decode state, graph captured), then the cases are timed --reps times in turn
and the median is taken.  A call is prefill + first token + steps, so the same call with one new token
is timed too and subtracted: ``us_per_step`` = (t(new) - t(1)) / steps, with steps = new - 1 for plain
greedy and the verify steps the call took (``return_stats``) for a speculative case.

Random weights fall into repetition within a few tokens, so the acceptance here is close to ideal and
the tokens/s of the speculative cases is an upper bound.  The number that carries over to real text is
``step_cost_ratio`` = a K-row verify step over a 1-row greedy step: there, speed-up = mean tokens per
step / step_cost_ratio.  ``rows_K`` is plain greedy ``generate`` on K copies of the prompt (a model copy
per K, so no decode state is re-allocated inside the timed window): what K rows through the decode step
cost without the draft, row-argmax and accept kernels.  Prints one JSON line per case."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--draft-lens", default="1,3,7")
    ap.add_argument("--ngram", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from mingpt_distributed_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    model = GPT(GPTConfig(model_type="gpt2", vocab_size=50257, block_size=1024), verbose=False)
    model = model.cuda().to(torch.bfloat16).eval()
    idx = torch.randint(0, 50257, (1, a.prompt), generator=torch.Generator().manual_seed(1)).cuda()
    drafts = [int(d) for d in a.draft_lens.split(",")]
    cases = {"greedy": lambda n: model.generate(idx, n)}
    for d in drafts:
        cases[f"draft_len_{d}"] = lambda n, d=d: model.generate_speculative(idx, n, draft_len=d, ngram=a.ngram)
    for d in drafts:
        copy = GPT(model.config, verbose=False).cuda().to(torch.bfloat16).eval()
        copy.load_state_dict(model.state_dict())
        cases[f"rows_{d + 1}"] = lambda n, m=copy, x=idx.repeat(d + 1, 1): m.generate(x, n)
    with torch.no_grad():
        want = cases["greedy"](a.new)
        steps = {k: a.new - 1 for k in cases}
        hists = {}
        for d in drafts:
            out, st = model.generate_speculative(idx, a.new, draft_len=d, ngram=a.ngram, return_stats=True)
            assert torch.equal(out, want), f"draft_len {d}: not the greedy tokens"
            steps[f"draft_len_{d}"] = int(st["steps"][0])
            hists[f"draft_len_{d}"] = st["emitted_hist"][0].tolist()
        for fn in cases.values():  # warm-up at both timed lengths
            fn(1)
            fn(a.new)
        full = {k: [] for k in cases}
        first = {k: [] for k in cases}
        for _ in range(a.reps):
            for k, fn in cases.items():
                full[k].append(timed(lambda: fn(a.new))[1])
                first[k].append(timed(lambda: fn(1))[1])
    res = {}
    for k in cases:
        t, t1 = statistics.median(full[k]), statistics.median(first[k])
        res[k] = {"metric": "B = 1 greedy decode: plain vs speculative", "model": "gpt2 (random init)", "case": k,
                  "prompt": a.prompt, "new_tokens": a.new, "ngram": a.ngram, "reps": a.reps,
                  "tok_s": round(a.new / t, 1), "tok_s_range": [round(a.new / max(full[k]), 1),
                                                                round(a.new / min(full[k]), 1)],
                  "steps": steps[k], "tokens_per_step": round((a.new - 1) / steps[k], 3),  # of one sequence
                  "us_per_step": round((t - t1) / steps[k] * 1e6, 1), "prefill_and_first_token_us": round(t1 * 1e6, 1)}
        if k in hists:
            res[k]["emitted_hist"] = hists[k]
        if k != "greedy":
            res[k]["step_cost_ratio"] = round(res[k]["us_per_step"] / res["greedy"]["us_per_step"], 3)
            res[k]["speedup_here"] = round(t_greedy / t, 3)
        else:
            t_greedy = t
        print(json.dumps(res[k]), flush=True)


if __name__ == "__main__":
    main()
