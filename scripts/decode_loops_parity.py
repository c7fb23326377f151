#!/usr/bin/env python
"""Bit parity of the decode loops (models/generation.py) between two checkouts of the project.

    python scripts/decode_loops_parity.py --out DIR_A        (in an export of the other commit)
    python scripts/decode_loops_parity.py --out DIR_B        (in the tree)
    python scripts/decode_loops_parity.py --compare DIR_A DIR_B     (no GPU: raw bytes of every file)

One process per checkout; when ``csrc/`` is the same in both, point both at one build of the
extension with ``MINGPT_EXT_SO``.  Runs the calls of tests/test_decode_loops_gpu.py on its tiny model
at both vocabulary sizes and once snapped to int8 (the ``gemv_w8`` steps) -- every entry point,
greedy and seeded, with and without processors and log-probabilities, ragged (with a stop token),
beam, speculative, each twice, the seeded ones once more with other settings -- and writes every
returned tensor as .npy.  Then, on fresh models with ``_GRAPH_DECODE`` off and the extension behind a
recording proxy, one step of every loop: per loop key the ordered extension entry points of that
step, as ``launches.txt``.  Two checkouts whose files are all byte-equal compute the same and launch
the same."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

NEW, LENS, SEED = 20, [1, 5, 17, 3], 1234567
PROC = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, no_repeat_ngram_size=3)
PROC2 = dict(repetition_penalty=1.1, presence_penalty=0.0, frequency_penalty=0.4, no_repeat_ngram_size=2)
SAMPLED = dict(do_sample=True, seed=SEED, temperature=0.8, top_k=20, top_p=0.9)
SAMPLED2 = dict(do_sample=True, seed=SEED, temperature=1.3, top_k=20, top_p=0.6)
SLOTS = ("_mg_decode_cache", "_mg_beam_cache", "_mg_spec_cache")
MODELS = {"V1000": (1000, False), "V8200": (8200, False), "V1000w8": (1000, True)}  # name: (V, quantize_int8_)


def model_for(name):
    from mingpt_distributed_amd.models import GPT, GPTConfig

    V, w8 = MODELS[name]
    torch.manual_seed(0)
    cfg = GPTConfig(n_layer=2, n_head=2, n_embed=128, vocab_size=V, block_size=64, embed_drop=0.0, resid_drop=0.0,
                    attn_drop=0.0)
    model = GPT(cfg, verbose=False).cuda().to(torch.bfloat16).eval()
    if w8:
        model.quantize_int8_()
    return model


def calls(V):
    """(name, call(model) -> tensor or tuple of tensors), in the order they run."""
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, V, (4, 5), generator=g).cuda()
    rows = [torch.randint(0, V, (n,), generator=g).cuda() for n in LENS]
    out = []
    for lp in (False, True):
        for pname, proc in (("", {}), ("_proc", PROC), ("_proc2", PROC2)):
            for sname, samp in (("greedy", {}), ("seeded", SAMPLED), ("seeded2", SAMPLED2)):
                if sname == "seeded2" and pname == "_proc":
                    continue
                if sname == "greedy" and pname == "_proc2":
                    continue
                kw = dict(samp, return_logprobs=lp, **proc)
                tag = f"{sname}{pname}{'_lp' if lp else ''}"
                out.append((f"generate.{tag}", lambda m, kw=kw: m.generate(idx, NEW, **kw)))
                out.append((f"batch.{tag}", lambda m, kw=kw: m.generate_batch(rows, NEW, eos_token=3, **kw)))
    out.append(("beam", lambda m: m.generate_beam(idx[:1], NEW, 4, eos_token=3)))
    out.append(("spec", lambda m: m.generate_speculative(idx[:1], NEW, draft_len=3)))
    return out


class _Recorder:
    """Attribute proxy over the extension: the names of the entry points called, in order."""

    def __init__(self, mod):
        self._mod, self.names = mod, []

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if not callable(fn) or name.endswith(("_supported", "_floats", "_groups")):
            return fn  # shape queries launch nothing

        def call(*a, **kw):
            self.names.append(name)
            return fn(*a, **kw)

        return call


def launches(name, lines):
    """One eager step of every loop the calls build, on a fresh model: '<model> <slot> <key>: names'."""
    from mingpt_distributed_amd.models import generation as gen
    from mingpt_distributed_amd.ops import _ext

    real, rec = _ext.ext, _Recorder(_ext.ext())
    graph = gen._GRAPH_DECODE
    _ext.ext, gen._GRAPH_DECODE = (lambda: rec), False
    try:
        model = model_for(name)
        for _, call in calls(MODELS[name][0]):
            call(model)
        for slot in SLOTS:
            state = model.__dict__.get(slot)
            for key, loop in (state._loops.items() if state is not None else ()):
                del rec.names[:]
                loop.step()
                lines.append(f"{name} {slot} {key!r}: {' '.join(rec.names)}")
        torch.cuda.synchronize()
    finally:
        _ext.ext, gen._GRAPH_DECODE = real, graph


def run(out):
    os.makedirs(out, exist_ok=True)
    n, lines = 0, []
    for mname, (V, _) in MODELS.items():
        model = model_for(mname)
        for name, call in calls(V):
            for rep in (0, 1):  # twice: the second call replays the first one's graphs
                res = call(model)
                for i, t in enumerate(res if isinstance(res, tuple) else (res,)):
                    t = t.detach().contiguous()
                    np.save(os.path.join(out, f"{mname}.{name}.call{rep}.{i}.npy"), t.cpu().numpy())
                    n += 1
        keys = {slot: sorted(map(repr, model.__dict__[slot]._loops)) for slot in SLOTS}
        lines.append(f"{mname} keys: {keys}")
        launches(mname, lines)
    with open(os.path.join(out, "launches.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"decode_loops_parity: wrote {n} arrays and {len(lines)} launch lines to {out} "
          f"(extension: {os.environ.get('MINGPT_EXT_SO') or 'in-tree'})", flush=True)


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb or not fa:
        print(f"decode_loops_parity: different or empty file sets ({len(fa)} vs {len(fb)})")
        return 1
    bad = [f for f in fa if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
    for f in bad:
        print(f"  DIFFERS: {f}")
    print(f"decode_loops_parity: {len(fa) - len(bad)} of {len(fa)} files byte-equal between {a} and {b}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="run the decode calls in this checkout and write the files here")
    ap.add_argument("--compare", nargs=2, metavar="DIR", help="compare the files of two runs byte by byte")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    with torch.no_grad():
        run(a.out)
