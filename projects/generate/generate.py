#!/usr/bin/env python
"""Prompted text generation from a GPT-2 checkpoint (upstream ``generate.ipynb``, advertised by
``/root/reference/README.md:15``).

No network here: point ``--weights`` at a local GPT-2 checkpoint (HF ``model.safetensors`` /
``pytorch_model.bin`` directory, loaded with safe loaders) and ``MINGPT_BPE_DIR`` at a directory
holding ``encoder.json`` + ``vocab.bpe``.  ``--random-init`` runs the same path on random weights
(for smoke tests; the text is noise).  On a GPU the prompt is prefilled once and every new token
is one fused-kernel decode step against the KV cache.

    python projects/generate/generate.py --weights /path/to/gpt2 --prompt "Andrej Karpathy, the" \
        --num-samples 5 --steps 20 --device cuda

Several prompts (``--prompt`` repeated, and / or ``--prompt-file`` with one prompt per line) are
decoded together in one ragged batch (``GPT.generate_batch``): every prompt keeps its own length,
``--num-samples`` rows each, and a row stops at the tokenizer's ``<|endoftext|>``.

    python projects/generate/generate.py --weights /path/to/gpt2 --prompt "The capital of France" \
        --prompt "Once upon a time, in a land far away," --num-samples 2 --steps 40 --device cuda

``--beams N`` (1..8) runs beam search on the one prompt instead of sampling (``GPT.generate_beam``) and
prints the N beams best first with their summed log-probability; ``--length-penalty a`` re-ranks them
by ``score / n_generated ** a``.

``--speculative DRAFT_LEN`` (1..7) decodes the one prompt greedily with n-gram drafts verified
``DRAFT_LEN + 1`` rows per step (``GPT.generate_speculative``; ``--ngram N``, 1..4, is the longest
suffix the draft looks up) -- the text of ``--greedy``, in fewer steps -- and prints the steps taken
and the mean tokens per step.

``--int8`` snaps the model to int8-representable weights after loading (``GPT.quantize_int8_``: int8
rows times power-of-two scales; on a GPU the decode steps then read int8 weights) and prints the largest
relative rounding error.

``--kv-int8`` keeps the KV cache as int8 with one power-of-two scale per (position, layer, head) K and V
vector (``kv_cache="int8"``, the KV8 model: every attention reads the snapped K / V) and prints the cache
bytes; it goes with sampling, ``--greedy``, ``--logprobs``, several prompts, ``--beams`` and ``--speculative``.

``--logprobs`` prints, after each sample, the summed log-probability of its generated tokens under
the model (temperature 1, before top-k / top-p) and their per-token perplexity.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from mingpt_distributed_amd.models import GPT, GPTConfig
from mingpt_distributed_amd.utils import set_seed


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-type", default="gpt2")
    ap.add_argument("--weights", default=None, help="local GPT-2 checkpoint (file or HF directory)")
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--prompt", action="append", default=None,
                    help="prompt text; repeat it to decode several prompts in one ragged batch")
    ap.add_argument("--prompt-file", default=None, help="a file with one prompt per non-empty line")
    ap.add_argument("--num-samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--top-p", type=float, default=None,
                    help="nucleus filtering after the temperature and top-k (default: off)")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--greedy", action="store_true")
    ap.add_argument("--logprobs", action="store_true",
                    help="print each sample's summed log-probability and per-token perplexity")
    ap.add_argument("--repetition-penalty", type=float, default=1.0,
                    help="divide (positive) or multiply (negative) the logit of every token already in the "
                         "context by this (1.0: off)")
    ap.add_argument("--presence-penalty", type=float, default=0.0,
                    help="subtract this from the logit of every token already in the context (0.0: off)")
    ap.add_argument("--frequency-penalty", type=float, default=0.0,
                    help="subtract this times its count from the logit of every token in the context (0.0: off)")
    ap.add_argument("--no-repeat-ngram", type=int, default=0,
                    help="never complete an n-gram of this size (1..8) that is already in the context (0: off)")
    ap.add_argument("--beams", type=int, default=0,
                    help="beam search with this many beams (1..8) on one prompt instead of sampling")
    ap.add_argument("--length-penalty", type=float, default=0.0,
                    help="with --beams: re-rank the final beams by score / n_generated ** penalty")
    ap.add_argument("--speculative", type=int, default=0, metavar="DRAFT_LEN",
                    help="greedy decoding of one prompt with n-gram drafts of this many tokens (1..7) per step")
    ap.add_argument("--ngram", type=int, default=3,
                    help="with --speculative: the longest suffix (1..4) the draft looks up in the text so far")
    ap.add_argument("--int8", action="store_true",
                    help="weight-only int8: snap the projections and the LM head to int8 rows with power-of-two "
                         "scales (GPT.quantize_int8_) before generating")
    ap.add_argument("--kv-int8", action="store_true",
                    help="int8 KV cache: K and V vectors snapped to int8 with one power-of-two scale each "
                         "(kv_cache='int8'), on every decoding mode")
    ap.add_argument("--device", default="auto")
    ap.add_argument("--seed", type=int, default=3407,
                    help="initialisation seed and the sampler's seed (reproducible on-device sampling)")
    a = ap.parse_args(argv)
    dev = a.device if a.device != "auto" else ("cuda" if torch.cuda.is_available() else "cpu")
    set_seed(a.seed)
    if a.random_init:
        model = GPT(GPTConfig(model_type=a.model_type, vocab_size=50257, block_size=1024), verbose=False)
    else:
        model = GPT.from_pretrained(a.model_type, source=a.weights)
    model.to(dev).eval()
    if a.int8:
        report = model.quantize_int8_()
        print(f"(int8 weights: {len(report)} matrices snapped, largest |W - s q| / max|row| {max(report.values()):.5f})")

    tok = None
    try:
        from mingpt_distributed_amd.bpe import BPETokenizer

        tok = BPETokenizer()
    except Exception as e:  # vocab files absent: fall back to raw token ids
        print(f"(no BPE vocabulary available: {e}; printing token ids)")
    texts = list(a.prompt or [])
    if a.prompt_file:
        with open(a.prompt_file, "r", encoding="utf-8") as f:
            texts += [ln.rstrip("\n") for ln in f if ln.strip()]
    if a.beams and len(texts) > 1:
        ap.error("--beams takes one prompt")
    proc = process_args(a)
    if proc and (a.beams or a.speculative):
        ap.error("the logits processors do not go with --beams or --speculative")
    if a.speculative and (len(texts) > 1 or a.beams):
        ap.error("--speculative takes one prompt and does not go with --beams")
    if len(texts) > 1:
        return generate_many(model, tok, texts, a, dev)
    prompt = texts[0] if texts else ""
    if tok is not None and prompt:
        x = tok(prompt).to(dev)
    else:
        x = torch.tensor([[50256]], dtype=torch.long, device=dev)
    if a.beams:
        return generate_beams(model, tok, x, a)
    if a.speculative:
        return generate_speculative(model, tok, x, a)
    x = x.expand(a.num_samples, -1).contiguous()
    kw = dict({"return_logprobs": True} if a.logprobs else {}, **proc, **kv_args(a))
    y = model.generate(x, max_new_tokens=a.steps, temperature=a.temperature, do_sample=not a.greedy,
                       top_k=a.top_k, seed=a.seed, top_p=a.top_p, **kw)
    y, lp = y if a.logprobs else (y, None)
    print_kv_bytes(model, a)
    outs = []
    for i in range(a.num_samples):
        out = tok.decode(y[i].cpu().squeeze()) if tok is not None else y[i].tolist()
        outs.append(out)
        print("-" * 80)
        print(out)
        if lp is not None:
            print_logprob(lp[i, x.size(1):])
    return outs


def process_args(a):
    """The logits-processor arguments of ``generate`` / ``generate_batch`` that the command line
    moved from their off values (none: the call is what it is without them)."""
    kw = dict(repetition_penalty=a.repetition_penalty, presence_penalty=a.presence_penalty,
              frequency_penalty=a.frequency_penalty, no_repeat_ngram_size=a.no_repeat_ngram)
    off = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, no_repeat_ngram_size=0)
    return {k: v for k, v in kw.items() if v != off[k]}


def kv_args(a):
    """``kv_cache="int8"`` with ``--kv-int8``, else nothing (the call is what it is without it)."""
    return {"kv_cache": "int8"} if a.kv_int8 else {}


def print_kv_bytes(model, a):
    """With ``--kv-int8``: the bytes of the KV caches the model's decode states hold (GPU only)."""
    from mingpt_distributed_amd.models.generation import kv_cache_nbytes

    if a.kv_int8:
        print(f"(KV cache bytes by decode state: {kv_cache_nbytes(model) or 'none on this device'})")


def print_logprob(lp):
    """The summed log-probability of a sample's generated tokens ``lp`` (1-D) and their perplexity."""
    total, n = float(lp.double().sum()), lp.numel()
    ppl = math.exp(-total / n) if n else float("nan")
    print(f"[logprob {total:.4f} over {n} tokens, perplexity {ppl:.4f}]")


def generate_beams(model, tok, x, a):
    """``--beams``: beam search on the one prompt x [1, T] (``GPT.generate_beam``), the beams printed
    best first with their summed log-probability; a beam stops at ``<|endoftext|>`` when the
    tokenizer has one."""
    eos = tok.encoder.encoder.get("<|endoftext|>") if tok is not None else None
    from mingpt_distributed_amd.models import generation

    # the module-level entry point: it takes kv_cache, GPT.generate_beam does not
    y, n, scores = generation.generate_beam(model, x, a.steps, a.beams, eos_token=eos, length_penalty=a.length_penalty,
                                            **kv_args(a))
    print_kv_bytes(model, a)
    outs = []
    for w in range(a.beams):
        ids = y[0, w, :int(n[0, w])].cpu()
        out = tok.decode(ids) if tok is not None else ids.tolist()
        outs.append(out)
        print("-" * 80)
        print(out)
        print(f"[beam {w}: logprob {float(scores[0, w]):.4f} over {int(n[0, w]) - x.size(1)} tokens]")
    return outs


def generate_speculative(model, tok, x, a):
    """``--speculative``: greedy decoding of the one prompt x [1, T] with n-gram drafts
    (``GPT.generate_speculative``), then the verify steps taken and the mean tokens per step."""
    from mingpt_distributed_amd.models import generation

    # the module-level entry point: it takes kv_cache, GPT.generate_speculative does not
    y, stats = generation.generate_speculative(model, x, a.steps, draft_len=a.speculative, ngram=a.ngram,
                                               return_stats=True, **kv_args(a))
    print_kv_bytes(model, a)
    out = tok.decode(y[0].cpu()) if tok is not None else y[0].tolist()
    print("-" * 80)
    print(out)
    steps = int(stats["steps"][0])
    hist = stats["emitted_hist"][0].tolist()
    print(f"[speculative: {max(a.steps - 1, 0)} tokens in {steps} verify steps of {a.speculative + 1} rows, "
          f"{(a.steps - 1) / steps if steps else 0.0:.2f} tokens per step; steps by tokens emitted: {hist}]")
    return [out]


def generate_many(model, tok, texts, a, dev):
    """Several prompts in one ragged batch: ``--num-samples`` rows per prompt, each with its own
    length, stopped at ``<|endoftext|>`` when the tokenizer has one.  Without a vocabulary a prompt
    is a line of token ids."""
    if tok is not None:
        rows = [tok(t)[0] if t else torch.tensor([50256]) for t in texts]
        eos = tok.encoder.encoder.get("<|endoftext|>")
    else:
        rows = [torch.tensor([int(w) for w in t.split()] or [0], dtype=torch.long) for t in texts]
        eos = None
    rows = [r.to(dev) for r in rows for _ in range(a.num_samples)]
    kw = dict({"return_logprobs": True} if a.logprobs else {}, **process_args(a), **kv_args(a))
    y, n, *lp = model.generate_batch(rows, max_new_tokens=a.steps, temperature=a.temperature,
                                     do_sample=not a.greedy, top_k=a.top_k, seed=a.seed, eos_token=eos,
                                     top_p=a.top_p, **kw)
    print_kv_bytes(model, a)
    outs = []
    for i in range(len(rows)):
        ids = y[i, :int(n[i])].cpu()
        out = tok.decode(ids) if tok is not None else ids.tolist()
        outs.append(out)
        print("-" * 80)
        print(out)
        if lp:
            print_logprob(lp[0][i, rows[i].numel():int(n[i])])
    return outs


if __name__ == "__main__":
    main()
