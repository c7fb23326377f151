#!/usr/bin/env python
"""Int8 KV cache decode (``kv_cache="int8"``) against the bf16 cache, interleaved in one process.

Three variants of greedy decode on a GPT-2 preset (--model-type) with random weights, at long prompts
and many rows, where a step reads the cache and not the weights:

* ``bf16``      ``kv_cache="bf16"``: the unchanged path, and the time reference;
* ``kv8_off``   ``kv_cache="int8"`` with ``_KV8_DECODE`` off: the KV8 model on the bf16 kernels (bf16 caches
                holding snapped rows, ``kv8_store`` in place, then ``attention_decode``);
* ``kv8_on``    ``kv_cache="int8"`` with the switch on: int8 caches and ``attention_decode_kv8``.

The two int8 variants run on two models holding the same weights, so each keeps its own decode state and
captured graphs and the timed calls alternate without a re-capture; the switch is set before each call.
Per row count of --batches: ``generate_batch`` on prompts spread over the 64 lengths below
``block_size - new`` (--prompt 0) or of --prompt tokens each through ``generate``, --new tokens, --reps
alternating runs, median and range; the tokens of the two int8 variants are asserted equal, and
``kv_cache_nbytes`` is printed.  "spread" is the range of the repeated bf16 runs relative to their median:
a KV8 point within it is not distinguishable from the bf16 path here.

--beams W: ``generate_beam`` with W beams instead, the row counts of --batches being B * W decode rows (B =
rows / W prompts of --prompt tokens, default 128); tok/s counts the best beam's tokens, B * new per call.
--speculative DRAFT_LEN: ``generate_speculative`` at B = 1 on a periodic prompt of --prompt tokens (default
128) instead, with the tokens per verify step.  Both run the same three alternating variants.

--reorder: ``beam_reorder`` against ``beam_reorder_kv8`` alone at W = 4, one prompt, the model's layers in
one launch, position --positions (default for this mode: 190), each captured as a graph of 20 launches
with a fixed non-identity permutation; microseconds per launch.

--kernels: ``attention_decode`` against ``attention_decode_kv8`` alone at the model's (H, hd) and
Tmax = block_size, per row count and --positions, each captured as a graph over rotating cache copies
(--rotate-mb of cache per graph, so no copy is re-read from a cache); microseconds per launch and GB/s of
the K/V bytes a launch has to read, computed from the shapes.  One JSON line per result."""
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
        outs = {k: fn() for k, fn in cases.items()}  # warm-up: states, graph capture
        outs = {k: fn() for k, fn in cases.items()}
        times = {k: [] for k in cases}
        for _ in range(reps):
            for k, fn in cases.items():
                times[k].append(timed(fn)[1])
    return outs, times


def kernels(a, cfg):
    from mingpt_distributed_amd.ops._ext import ext
    from mingpt_distributed_amd.ops.quant import snap_vectors

    C = ext()
    D, H, Tmax = cfg.n_embed, cfg.n_head, cfg.block_size
    hd = D // H
    for B in map(int, a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        rows = torch.randn(B, Tmax, 3 * D, generator=g).to(torch.bfloat16).cuda()
        q, s, d = snap_vectors(rows[..., D:].view(B, Tmax, 2, H, hd))
        rows[..., D:] = d.view(B, Tmax, 2 * D)
        kq0, ks0 = q.permute(0, 2, 3, 1, 4).contiguous(), s.permute(0, 2, 3, 1).contiguous()
        copies = max(2, min(32, -(-a.rotate_mb * (1 << 20) // rows.numel() // 2)))
        caches = [rows.clone() for _ in range(copies)]
        kqs, kss = [kq0.clone() for _ in range(copies)], [ks0.clone() for _ in range(copies)]
        x = torch.randn(B, 3 * D, generator=g).to(torch.bfloat16).cuda()
        xs = x.clone()
        C.kv8_store(xs.view(B, 1, 3 * D), H)
        part = torch.empty(C.attention_decode_part_floats(B, H, hd), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(B * H, dtype=torch.int32, device="cuda")
        pd = torch.zeros(1, dtype=torch.int32, device="cuda")
        runs = {"bf16": lambda: [C.attention_decode(xs, c, H, 1, pd, part, cnt, 0) for c in caches],
                "kv8": lambda: [C.attention_decode_kv8(x, kq, ks, H, 1, pd, part, cnt, 0) for kq, ks in zip(kqs, kss)]}
        graphs = {}
        for k, fn in runs.items():
            fn()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                keep = fn()
        for pos in map(int, a.positions.split(",")):
            pos = min(pos, Tmax - 1)
            pd.fill_(pos)
            assert all(torch.equal(u, v) for u, v in zip(runs["bf16"](), runs["kv8"]()))
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
            kv_bf16, kv_int8 = B * (pos + 1) * 4 * D, B * (pos + 1) * (2 * D + 8 * H)
            print(json.dumps({"metric": "decode attention us per launch, cache from HBM", "model": a.model_type, "B": B,
                              "H": H, "hd": hd, "Tmax": Tmax, "pos": pos, "copies": copies, "outputs_equal": True,
                              "bf16_us": round(med["bf16"], 2), "kv8_us": round(med["kv8"], 2),
                              "bf16_kv_bytes": kv_bf16, "kv8_kv_bytes": kv_int8,
                              "bf16_GBps": round(kv_bf16 / med["bf16"] / 1e3, 1),
                              "kv8_GBps": round(kv_int8 / med["kv8"] / 1e3, 1),
                              "kv8_over_bf16_time": round(med["kv8"] / med["bf16"], 3)}), flush=True)
        del graphs, keep, caches, kqs, kss


def reorder(a, cfg):
    from mingpt_distributed_amd.ops._ext import ext

    C = ext()
    L, D, H, Tmax, W = cfg.n_layer, cfg.n_embed, cfg.n_head, cfg.block_size, 4
    g = torch.Generator().manual_seed(0)
    kv = torch.randn(L, W, Tmax, 3 * D, generator=g).to(torch.bfloat16).cuda()
    kq = torch.randint(-127, 128, (L, W, 2, H, Tmax, D // H), generator=g, dtype=torch.int8).cuda()
    ks = torch.rand(L, W, 2, H, Tmax, generator=g).cuda()
    parent = torch.tensor([1, 2, 3, 0], dtype=torch.int32, device="cuda")  # every beam moves
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    runs = {"bf16": lambda: [C.beam_reorder(kv, W, parent, pos) for _ in range(20)],
            "kv8": lambda: [C.beam_reorder_kv8(kq, ks, W, parent, pos) for _ in range(20)]}
    graphs = {}
    for k, fn in runs.items():
        fn()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            fn()
    for p in map(int, a.positions.split(",")):
        pos.fill_(min(p, Tmax))
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
                us[k].append(e0.elapsed_time(e1) * 1e3 / 200)
        n = min(p, Tmax)
        print(json.dumps({"metric": "beam cache reorder us per launch, all layers, every beam moved", "model": a.model_type,
                          "W": W, "layers": L, "pos": n, "reps": a.reps,
                          "bf16_us": round(statistics.median(us["bf16"]), 2),
                          "bf16_us_range": [round(min(us["bf16"]), 2), round(max(us["bf16"]), 2)],
                          "kv8_us": round(statistics.median(us["kv8"]), 2),
                          "kv8_us_range": [round(min(us["kv8"]), 2), round(max(us["kv8"]), 2)],
                          "bf16_bytes_moved": L * W * n * 4 * D, "kv8_bytes_moved": L * W * n * (2 * D + 8 * H)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-type", default="gpt2", choices=["gpt2", "gpt2-medium", "gpt2-large", "gpt2-xl"])
    ap.add_argument("--prompt", type=int, default=0,
                    help="tokens per prompt through generate(); 0: generate_batch on lengths just below block_size - new")
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="time the two decode-attention kernels alone instead")
    ap.add_argument("--beams", type=int, default=0, help="generate_beam with this many beams; --batches are B * W rows")
    ap.add_argument("--speculative", type=int, default=0, metavar="DRAFT_LEN",
                    help="generate_speculative at B = 1 with drafts of this many tokens")
    ap.add_argument("--reorder", action="store_true", help="time beam_reorder against beam_reorder_kv8 alone instead")
    ap.add_argument("--positions", default=None, help="--kernels: default 127,511,895,1023; --reorder: default 190")
    ap.add_argument("--rotate-mb", type=int, default=600)
    a = ap.parse_args()
    from mingpt_distributed_amd.models import GPT, GPTConfig
    from mingpt_distributed_amd.models import generation as gen

    cfg = GPTConfig(model_type=a.model_type, vocab_size=50257, block_size=1024).resolve()
    if a.positions is None:
        a.positions = "190" if a.reorder else "127,511,895,1023"
    if a.reorder:
        return reorder(a, cfg)
    if a.kernels:
        return kernels(a, cfg)
    if a.speculative:
        a.batches = "1"
    torch.manual_seed(0)
    on = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    off = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    off.load_state_dict(on.state_dict())

    def switched(value, fn):
        def run():
            gen._KV8_DECODE = value
            return fn()
        return run

    for B in map(int, a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        stats, rows = {}, B  # decode rows of the state; B: the sequences whose tokens are counted
        if a.beams:
            B, T = B // a.beams, a.prompt or 128
            idx = torch.randint(0, 50257, (B, T), generator=g).cuda()
            lens = [T] * B
            call = lambda m, kv: gen.generate_beam(m, idx, a.new, a.beams, kv_cache=kv)[0]
        elif a.speculative:
            T = a.prompt or 128
            idx = torch.randint(0, 50257, (B, 5), generator=g).repeat(1, T // 5 + 1)[:, :T].contiguous().cuda()
            lens = [T] * B

            def call(m, kv):
                out, st = gen.generate_speculative(m, idx, a.new, draft_len=a.speculative, return_stats=True, kv_cache=kv)
                stats[kv] = round((a.new - 1) / max(int(st["steps"].sum()), 1), 2)
                return out
        elif a.prompt:
            idx = torch.randint(0, 50257, (B, a.prompt), generator=g).cuda()
            lens = [a.prompt] * B
            call = lambda m, kv: m.generate(idx, a.new, kv_cache=kv)
        else:
            top = cfg.block_size - a.new
            lens = [top - (b * 64 // B) for b in range(B)]
            prompts = [torch.randint(0, 50257, (n,), generator=g).cuda() for n in lens]
            call = lambda m, kv: m.generate_batch(prompts, a.new, kv_cache=kv)[0]
        outs, times = ab({"bf16": lambda: call(on, "bf16"), "kv8_off": switched(False, lambda: call(off, "int8")),
                          "kv8_on": switched(True, lambda: call(on, "int8"))}, a.reps)
        gen._KV8_DECODE = True
        assert torch.equal(outs["kv8_on"], outs["kv8_off"]), "attention_decode_kv8 differs from the KV8 model on bf16"
        med = {k: statistics.median(ts) for k, ts in times.items()}
        mode = f"beam search W = {a.beams} (best beam)" if a.beams else (
            f"speculative greedy, drafts of {a.speculative}" if a.speculative else "greedy decode")
        res = {"metric": f"{mode} tokens/s: bf16 cache, KV8 on the bf16 kernels, KV8 on int8 caches", "rows": rows,
               "model": f"{a.model_type} (random init)", "batch": B, "prompt_lengths": [min(lens), max(lens)],
               "new_tokens": a.new, "reps": a.reps, "kv8_tokens_equal": True,
               "kv8_tokens_equal_bf16_tokens": bool(torch.equal(outs["kv8_on"], outs["bf16"]))}
        for k, ts in times.items():
            res[k + "_tok_s"] = round(B * a.new / med[k], 1)
            res[k + "_tok_s_range"] = [round(B * a.new / max(ts), 1), round(B * a.new / min(ts), 1)]
        res["bf16_spread"] = round((max(times["bf16"]) - min(times["bf16"])) / med["bf16"], 3)
        res["kv8_on_over_bf16"] = round(med["bf16"] / med["kv8_on"], 3)
        res["kv8_on_over_kv8_off"] = round(med["kv8_off"] / med["kv8_on"], 3)
        res["kv8_on_slower_than_bf16_beyond_spread"] = bool(med["kv8_on"] > med["bf16"] * (1 + res["bf16_spread"]))
        if stats:
            res["tokens_per_step"] = stats
        res["kv_cache_nbytes"] = {"on": gen.kv_cache_nbytes(on), "off": gen.kv_cache_nbytes(off)}
        print(json.dumps(res), flush=True)
        for m in (on, off):  # the next row count builds its own states
            for slot in gen._STATE_SLOTS:
                m.__dict__.pop(slot, None)


if __name__ == "__main__":
    main()
