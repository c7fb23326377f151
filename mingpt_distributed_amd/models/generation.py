"""Autoregressive generation with a KV cache: ``generate``, ``generate_batch``, ``generate_beam``,
``generate_speculative`` and ``score``.  What each computes is documented on the function; the rules
(sampling, log-probabilities, processors, beams, drafts, W8) are in common.h and ``ops.reference``.

Layout of this file, top to bottom:

* ``_sample``, ``_CpuCache``: the CPU path -- the same algorithm in plain PyTorch, and the executable
  definition of the semantics (the ``_cpu`` halves of the entry points further down).
* ``bf16_weights``, ``w8_weights``, ``w8_status``, ``quantize_int8_``: per-model weight twins.
* ``_Loop``: one device-side token loop -- eager warm-up, captured once as a hipGraph, replayed.
* ``_Params``: an 8-word device parameter block (``_sample_words``, ``_ragged_words``, ``_proc_words``).
* ``_Body``: the step bodies' plumbing -- ``_route`` / ``_lin`` (which GEMM a projection runs on),
  ``_blocks``, ``_head``, ``_prompt``.  ``score`` needs nothing else.
* ``_GpuCache(_Body)``: one decode state -- KV caches, workspaces, the weights' stamp, the two step
  bodies (``prefill``, ``_decode``) and every token loop as a closure around ``_decode`` that ends with
  the loop's own tail.  A model keeps up to six (``_state_for``): ``_mg_decode_cache``, ``_mg_beam_cache``
  (B * W rows) and ``_mg_spec_cache`` (B sequences, B * K step rows), and beside each the state of
  ``kv_cache="int8"`` (the KV8 model on int8 caches): ``_mg_kv8_cache``, ``_mg_beam_kv8_cache`` and
  ``_mg_spec_kv8_cache``.
* the word builders, ``_state_for``, then one section per entry point: checks, host loop, GPU half.

Who owns what.  A loop in ``_loops`` owns its graph and, for the rectangular loops, its ``tok`` /
``pos`` / ``seq`` (``_tok_state``); a weight change or a W8 / KV8 flip (``_stamp``) drops every loop.  The
decode state owns what outlives them: the caches, the ragged / beam / spec states (allocated on first
use) and the three parameter blocks, whose pointers the captured steps bake in.

Loop keys (``_key``): ``"step"``; ``"greedy"`` (the LM head's fused argmax, or torch's on a small
vocabulary) and ``"sample"`` (one batch-wide position, ``sample_logits``), each also as ``_lp`` (the
lse kernel before the pick), ``_proc`` (the process kernel after the LM head) and ``_proc_lp``, the
greedy ones on the ragged greedy pick (``_greedy_picked``); ``("ragged" | "ragged_lp" |
"ragged_proc" | "ragged_proc_lp", greedy)``; ``("beam", W)``; ``("spec", K)``.
"""
from __future__ import annotations

import gc
import os
import struct
from typing import Optional

import torch
import torch.nn.functional as F

from ..ops import reference as R
from ..ops.grads import before_use
from ..ops.quant import dequantize_rows, quantize_rows, snap_vectors


def _sample(logits, temperature, do_sample, top_k, top_p=None):
    if not do_sample:  # greedy: top-1 of softmax(logits / t) is the argmax of the logits
        return logits.argmax(dim=-1, keepdim=True)
    logits = logits.float() / temperature
    if top_k is not None:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits[logits < v[:, [-1]]] = -float("Inf")
    p = R.sample_top_p(top_p)
    if p is not None:  # the nucleus of what is left, ties at its boundary all kept (common.h)
        logits[~R.nucleus_keep(logits.double(), p)] = -float("Inf")
    probs = F.softmax(logits, dim=-1)
    return torch.multinomial(probs, num_samples=1)


# ------------------------------------------------------------------------------------ CPU
class _CpuCache:
    def __init__(self, model, idx, kv8=False, every=False):
        """``kv8``: the KV8 model (common.h) -- every K and V vector is snapped (``snap_vectors``) before
        any attention reads it, in the prompt pass and in ``step``.  ``every``: ``logits`` holds every
        position's, [B, T, V] (``score`` and the speculative verify rows), not the last one's."""
        self.model = model
        self.k, self.v = [], []
        self.snap = (lambda t: snap_vectors(t)[2]) if kv8 else (lambda t: t)
        tr = model.transformer

        def attend(i, q, k, v):  # the whole prompt at once: layer i's keys / values start here
            k, v = self.snap(k), self.snap(v)
            self.k.append(k)
            self.v.append(v)
            return R.causal_attention(q, k, v, 0.0, False)

        self.logits = self._body(tr.wte.weight[idx] + tr.wpe.weight[:idx.size(1)], attend, every)

    def _body(self, x, attend, every=False):
        """Last-position logits (``every``: all positions') of the blocks and the LM head on x [B, T, C];
        layer i's attention output is ``attend(i, q, k, v)`` ([B, H, T, hd] each)."""
        m = self.model
        tr = m.transformer
        B, T, C = x.shape
        H = m.config.n_head
        f = lambda t: t.view(B, T, H, C // H).transpose(1, 2)
        for i, blk in enumerate(tr.h):
            h = blk.ln_1(x)
            q, k, v = F.linear(h, blk.attn.c_attn.weight, blk.attn.c_attn.bias).split(C, dim=2)
            y = attend(i, f(q), f(k), f(v)).transpose(1, 2).reshape(B, T, C)
            x = x + F.linear(y, blk.attn.c_proj.weight, blk.attn.c_proj.bias)
            x = x + blk.mlp(blk.ln_2(x))
        return m.lm_head(tr.ln_f(x if every else x[:, -1]))

    def step(self, tok, pos):
        tr = self.model.transformer

        def attend(i, q, k, v):  # one new token against the layer's cached keys / values
            self.k[i] = torch.cat([self.k[i], self.snap(k)], dim=2)
            self.v[i] = torch.cat([self.v[i], self.snap(v)], dim=2)
            att = (q @ self.k[i].transpose(-1, -2)) / q.size(-1) ** 0.5
            return F.softmax(att, dim=-1) @ self.v[i]

        x = tr.wte.weight[tok[:, 0]] + tr.wpe.weight[pos]
        return self._body(x.unsqueeze(1), attend)


# ------------------------------------------------------------------------------------ GPU
def bf16_weights(model):
    """bf16 view of every weight the decode kernels read, converted ONCE and cached on the model.

    A model trained through the engine already holds bf16 compute weights (returned as is); an
    fp32 model (e.g. ``from_pretrained`` without ``.to(bfloat16)``) gets one bf16 copy per
    weight, reused across decode steps and ``generate`` calls, and refreshed only when the weight
    changes (storage pointer or in-place version).  The captured decode hipGraph therefore holds
    no conversion kernels: per-token traffic is the bf16 weights once."""
    cache = model.__dict__.setdefault("_mg_bf16_weights", {})

    def get(w: torch.Tensor) -> torch.Tensor:
        if w.dtype == torch.bfloat16:
            return w
        stamp = (w.data_ptr(), w._version)
        ent = cache.get(id(w))
        if ent is None or ent[0] != stamp:
            ent = (stamp, w.detach().to(torch.bfloat16).contiguous())
            cache[id(w)] = ent
        return ent[1]

    return get


def _w8_named_weights(model):
    """(name, weight) of every matrix the W8 path covers: the blocks' four projections and the LM head
    (the tied ``wte``)."""
    for i, blk in enumerate(model.transformer.h):
        for sub in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"):
            yield f"transformer.h.{i}.{sub}.weight", blk.get_submodule(sub).weight
    yield "lm_head.weight", model.lm_head.weight


def w8_weights(model):
    """int8 twins of the weights the skinny GEMM reads (the W8 rule in common.h), cached on the model.

    ``get(w)`` returns ``(q int8 [N, K], s float32 [N])`` or None.  A twin is built on first use and
    kept under the weight's (storage pointer, in-place version) stamp.  When the stamp changes the
    weight is quantized again, and the twin is kept only if the weight still equals its own
    dequantized twin exactly (a model snapped by ``quantize_int8_``); otherwise that weight takes the
    bf16 kernel from then on -- a later optimizer step or ``load_state_dict`` makes decode slower,
    never wrong (``quantize_int8_`` starts over).  K no multiple of 8: None."""
    cache = model.__dict__.setdefault("_mg_w8_weights", {})

    def get(w: torch.Tensor):
        if w.dim() != 2 or w.shape[1] % 8:
            return None
        stamp = (w.data_ptr(), w._version)
        ent = cache.get(id(w))
        if ent is not None and (ent[1] is None or ent[0] == stamp):
            return ent[1]
        twin = None
        try:
            q, s = quantize_rows(w)
            if torch.equal(dequantize_rows(q, s, w.dtype), w.detach()):
                twin = (q.contiguous(), s.contiguous())
        except ValueError:  # a non-finite weight or another dtype: the bf16 kernel's business
            pass
        cache[id(w)] = (stamp, twin)
        return twin

    return get


def w8_status(model):
    """Per covered weight name: True (an int8 twin is live), False (the weight left the W8 path: it no
    longer equals a dequantized twin) or None (no decode step has asked for it yet)."""
    cache = model.__dict__.get("_mg_w8_weights", {})
    out = {}
    for name, w in _w8_named_weights(model):
        ent = cache.get(id(w))
        out[name] = None if ent is None else ent[1] is not None
    return out


@torch.no_grad()
def quantize_int8_(model):
    """Snap ``model`` in place to int8-representable weights (the W8 rule in common.h,
    ``ops.quant.quantize_rows``): every block's ``c_attn``, attention ``c_proj``, ``mlp.c_fc`` and
    ``mlp.c_proj`` weight and ``lm_head.weight`` become s_n q[n, k], one power-of-two scale per output
    row.  ``lm_head.weight`` is the tied ``wte``, so the token embedding is snapped with it.  Biases,
    LayerNorms and ``wpe`` are untouched.  Every path (CPU, ``use_cache=False``, prefill, the rows and
    MFMA GEMMs) then computes the snapped model; GPU decode steps of up to 8 rows read the int8 twins
    (``gemv_w8``) and produce the same bits.  The model is marked (``_mg_w8``).  Idempotent.  Returns
    {weight name: the largest |W - s q| / a_n over its rows} (0.0 on a snapped model; < 1 / 127)."""
    report = {}
    for name, w in _w8_named_weights(model):
        q, s = quantize_rows(w)
        d = dequantize_rows(q, s, w.dtype)
        a = w.float().abs().amax(dim=1)
        err = (w.float() - d.float()).abs().amax(dim=1) / torch.where(a > 0, a, torch.ones_like(a))
        report[name] = float(err.max())
        if not torch.equal(d, w):
            w.copy_(d)
    model.__dict__.get("_mg_w8_weights", {}).clear()  # weights that had left the W8 path start over
    model.__dict__["_mg_w8"] = True
    return report


def _capture(fn):
    """(graph, fn()) with fn's launches captured into a new hipGraph.  Python's cyclic garbage is
    collected first and the collector stays off until the capture ends: a decode state and its
    model refer to each other, so a dropped model's graphs are freed by the collector, and a
    graph destroyed while a stream is capturing is a HIP error raised from a destructor (the
    process aborts).  ``torch.cuda.graph`` no longer collects on entry by itself."""
    gc.collect()
    on = gc.isenabled()
    gc.disable()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
    finally:
        if on:
            gc.enable()
    return graph, out


_GRAPH_DECODE = True  # set False to launch the decode step eagerly
# decode steps of 9..64 rows run their projections on the rows GEMM (gemm_rows.hip); False
# (MINGPT_ROWS_GEMM=0) sends them to the MFMA GEMM as more than 64 rows go
_ROWS_GEMM = os.environ.get("MINGPT_ROWS_GEMM", "1") != "0"
# a model marked by quantize_int8_ runs its skinny-GEMM projections on the int8 twins (gemv_w8: the
# same bits from half the weight bytes); False (MINGPT_W8_DECODE=0) keeps them on the bf16 kernel
_W8_DECODE = os.environ.get("MINGPT_W8_DECODE", "1") != "0"
# a kv_cache="int8" state keeps int8 caches and attends with attention_decode_kv8 (attention_kv8.hip);
# False (MINGPT_KV8_DECODE=0) runs the same KV8 model on the bf16 kernels: bf16 caches holding snapped
# rows, kv8_store on the step's row in place, then attention_decode -- the same bits
_KV8_DECODE = os.environ.get("MINGPT_KV8_DECODE", "1") != "0"
_KV_CACHES = ("bf16", "int8")


class _Loop:
    """One device-side token loop: ``step()`` launches one decode step on persistent device
    buffers (``state``, kept here for the loop's owner) that its own kernels advance, and returns
    the step's logits.  Decoding is launch-bound (B rows through ~5 kernels per layer), so the step
    is captured once as a hipGraph and the replays are queued back to back without a host round
    trip.  ``warm`` (default: ``step``) runs once, eagerly, when the loop is built: workspaces and
    lazy kernel attributes are set up outside the capture."""

    def __init__(self, step, state, warm=None):
        self.step, self.state = step, state
        self.graph = self.logits = None
        (warm or step)()

    def run(self, n):
        """n steps; ``logits`` is the last step's (a buffer the replays rewrite)."""
        if _GRAPH_DECODE and self.graph is None:
            self.graph, self.logits = _capture(self.step)
        for _ in range(n):
            if _GRAPH_DECODE:
                self.graph.replay()
            else:
                self.logits = self.step()


class _Params:
    """An 8-word int32 device parameter block (``dev``: captured steps bake its pointer in) and the
    words last uploaded to it."""

    def __init__(self, device):
        self.dev = torch.zeros(8, dtype=torch.int32, device=device)
        self.words = None

    def set(self, words, always=False):
        """Upload ``words`` unless they are the block's already -- a host-to-device copy waits for the
        queued replays to drain -- and return ``dev``.  ``always``: for a block that a kernel writes.
        The sampled step advances the draw counter in word 2 on the device, so the record here is
        stale after the first replay and every call has to upload."""
        if always or self.words != list(words):
            self.dev.copy_(torch.tensor(words, dtype=torch.int32))
            self.words = list(words)
        return self.dev


class _Body:
    """The step bodies' plumbing for one model (``_lin``, ``_blocks``, ``_head``, ``_prompt``) without
    KV caches, workspaces or loops: all that ``score`` needs, and the base of a decode state."""

    def __init__(self, model):
        from ..ops._ext import ext
        from ..ops import gemm as G

        model.config.check_gpu_support()
        self.C, self.G, self.bf, self.w8, self.model = ext(), G, bf16_weights(model), w8_weights(model), model

    def _w8_on(self):
        """The skinny-GEMM projections read int8 twins: the model is marked and the switch is on."""
        return _W8_DECODE and self.model.__dict__.get("_mg_w8", False)

    def _route(self, rows):
        """The GEMM a decode step of ``rows`` rows runs its projections on (``_lin``'s names).
        Up to 8 rows go through the skinny GEMM (gemv.hip): at M = rows the MFMA GEMM has one row
        tile and walks K latency-bound.  The widest row is the MLP output projection's, 4 D <=
        8192: every preset up to gpt2-xl (6400); the LayerNorm'ed projections and the LM head have
        K = D <= 2048, inside the kernel's 4096 for fused LayerNorm and wide outputs.  9..64 rows:
        the rows GEMM (gemm_rows.hip) streams each weight matrix once with the rows as MFMA
        operands; more rows, a wider model, or ``_ROWS_GEMM`` off: the MFMA GEMM."""
        K = 4 * self.model.config.n_embed
        if self.C.gemv_supported(rows, K):
            return "gemv"
        if _ROWS_GEMM and rows >= 9 and self.C.gemm_rows_supported(rows, K):
            return "rows"
        return "mfma"

    def _lin(self, route, inp, w, b, epi, resid=None, ld=0, ln=None, am=None):
        """epi(LN(inp) @ w^T + b) with ``ln`` = a LayerNorm module applied first, on the GEMM that
        ``route`` names: ``"gemv"`` the skinny GEMM (gemv.hip, up to 8 decode rows; the LayerNorm is
        fused into its staging, and ``am`` fuses the LM head's greedy argmax), ``"rows"`` the rows GEMM
        (gemm_rows.hip, 9..64 decode rows) and ``"mfma"`` the MFMA GEMM (gemm.hip), both behind a
        LayerNorm launch."""
        C, G, bf = self.C, self.G, self.bf
        eps = self.model.config.layer_norm_eps
        if route not in ("gemv", "rows", "mfma"):
            raise ValueError(f"unknown GEMM route {route!r}")
        if am is not None and route != "gemv":
            raise ValueError("the fused argmax is the skinny GEMM's")
        code = {"none": 0, "bias": 1, "gelu": 2, "resid": 3}[epi]
        if route == "gemv":
            lw, lb = (bf(ln.weight), bf(ln.bias)) if ln is not None else (None, None)
            tw = self.w8(w) if self._w8_on() else None  # (q, s): the int8 twin of a snapped weight
            kernel, wt = (C.gemv, (bf(w),)) if tw is None else (C.gemv_w8, tw)
            return kernel(inp, *wt, code, bf(b) if b is not None else None, resid, ld, lw, lb, eps, *(am or ()))
        if ln is not None:
            inp, _, _ = C.layernorm_fwd(inp, bf(ln.weight), bf(ln.bias), eps)
        if route == "rows":
            return C.gemm_rows(inp, bf(w), code, bf(b) if b is not None else None, resid, ld)
        if epi == "gelu":
            pre = torch.empty((inp.shape[0], w.shape[0]), dtype=torch.bfloat16, device=inp.device)
            return G.gemm_nt(inp, bf(w), bias=bf(b), epi="gelu", pre_out=pre)
        return G.gemm_nt(inp, bf(w), bias=bf(b) if b is not None else None, epi=epi, resid=resid,
                         ld=ld or None)

    def _blocks(self, x, attend, route):
        """The transformer blocks on rows x [M, D]; ``attend(i, qkv)`` is layer i's attention on its
        qkv projection [M, 3D], cache update included.  ``route``: the GEMM the projections go
        through (``_lin``)."""
        for i, blk in enumerate(self.model.transformer.h):
            a, mm = blk.attn, blk.mlp
            qkv = self._lin(route, x, a.c_attn.weight, a.c_attn.bias, "bias", ln=blk.ln_1)
            y = attend(i, qkv)
            x = self._lin(route, y, a.c_proj.weight, a.c_proj.bias, "resid", resid=x)
            u = self._lin(route, x, mm.c_fc.weight, mm.c_fc.bias, "gelu", ln=blk.ln_2)
            x = self._lin(route, u, mm.c_proj.weight, mm.c_proj.bias, "resid", resid=x)
        return x

    def _head(self, x_last, route, am=None):
        """ln_f and the LM head on x_last [B, D]: logits [B, ld], ld = V rounded up to 8 (the
        columns from V on are padding).  ``am`` = (part, pos): see ``_decode``."""
        m = self.model
        V = m.config.vocab_size
        return self._lin(route, x_last, m.lm_head.weight, None, "none", ld=(V + 7) // 8 * 8,
                         ln=m.transformer.ln_f, am=am)

    def _prompt(self, idx, keep=None):
        """The blocks' output [B, T, D] for the prompt idx [B, T] on the MFMA GEMM path; ``keep(i,
        qkv)`` is handed every layer's qkv rows [B, T, 3D] (a decode state's cache)."""
        C, bf = self.C, self.bf
        tr, cfg = self.model.transformer, self.model.config
        B, T = idx.shape
        D, H = cfg.n_embed, cfg.n_head
        x = C.embedding_fwd(idx.contiguous(), bf(tr.wte.weight), bf(tr.wpe.weight), 0.0, 0).view(B * T, D)

        def attend(i, qkv):
            if keep is not None:
                keep(i, qkv.view(B, T, 3 * D))
            return C.attention_fwd(qkv, B, T, H, 0.0, 0)[0]

        return self._blocks(x, attend, "mfma").view(B, T, D)


class _GpuCache(_Body):
    """One decode state: KV caches ([B, Tmax, 3D] qkv rows per layer) plus the captured decode steps
    (``_loops``) of one model at one batch size.  Kept on the model across calls (``_state_for``): a
    later ``generate`` with the same batch re-prefills into the same buffers and replays the same
    hipGraphs, unless a weight changed storage or version since the capture (then the graphs are
    re-captured)."""

    def __init__(self, model, idx, tmax, last=None, rows=None, kv8=False):
        """``rows`` (beam search, speculative decoding): a state of that many decode rows whose
        layers' caches are one stacked buffer ``kv`` [L, rows, Tmax, 3D] (the reorder kernel walks
        every layer in one launch), not prefilled here -- ``idx`` only names the device.
        ``kv8`` (``kv_cache="int8"``): a state of the KV8 model (common.h).  With ``_KV8_DECODE`` on its
        caches are ``kq`` int8 [B, 2, H, Tmax, hd] and ``ks`` float32 [B, 2, H, Tmax] per layer, off they
        are bf16 qkv rows holding snapped K/V (``_kv8_storage``); with ``rows`` either kind is one
        stacked buffer with a leading layer dimension (``kqs`` / ``kss``, or ``kv``)."""
        super().__init__(model)
        self.tmax, self.dev = tmax, idx.device
        B = idx.size(0) if rows is None else rows
        cfg = model.config
        D = cfg.n_embed
        self.B = B
        self.kv = self.kqs = self.kss = None
        self.kv8, self.stacked = bool(kv8), rows is not None
        self.caches, self.kq, self.ks = [], [], []
        if self.kv8:
            self._kv8_storage()
        elif rows is None:
            self.caches = [torch.empty(B, tmax, 3 * D, device=self.dev, dtype=torch.bfloat16)
                           for _ in range(cfg.n_layer)]
        else:
            self.kv = torch.empty(cfg.n_layer, B, tmax, 3 * D, device=self.dev, dtype=torch.bfloat16)
            self.caches = list(self.kv.unbind(0))
        # decode-attention workspace owned by this state (split partials + per-(b, h) counters
        # that the kernel leaves zero): the captured graphs bake these pointers in
        H = cfg.n_head
        self.dec_part = torch.empty(self.C.attention_decode_part_floats(B, H, D // H),
                                    device=self.dev, dtype=torch.float32)
        self.dec_cnt = torch.zeros(B * H, device=self.dev, dtype=torch.int32)
        self.stamp = self._stamp()
        self._loops = {}  # the device-side token loops (_Loop) by key, built on first use
        # what outlives the loops: the sample, ragged-pick and process kernels' parameter blocks, and
        # the ragged / beam (by W) / speculative (by K) states, allocated on first use
        self._sparams, self._rparams, self._pparams = (_Params(self.dev) for _ in range(3))
        self._rstate, self._bstate, self._sstate = None, {}, {}
        self.logits = None
        if rows is None:
            self.prefill(idx, last)

    def _kv8_on(self):
        """This state's decode attention is attention_decode_kv8 on int8 caches."""
        return self.kv8 and _KV8_DECODE

    def _kv8_storage(self):
        """A KV8 state's caches for the kernel ``_KV8_DECODE`` names now: the int8 pair, or bf16 qkv
        rows.  Called before every prefill and before a loop is looked up (``_fresh``: the beam and
        speculative loops are built, with a warm-up step, before their prefill), so a flip of the switch
        swaps the buffers (the other kind is freed) and the next prefill fills them; ``_stamp`` drops
        the loops captured on the old ones.  A ``rows`` state keeps each kind as one stacked buffer
        (``kqs`` [L, rows, 2, H, Tmax, hd] / ``kss`` [L, rows, 2, H, Tmax], or ``kv``) and the per-layer
        lists are views of it, so the reorder stays one launch."""
        cfg = self.model.config
        B, D, H, L = self.B, cfg.n_embed, cfg.n_head, cfg.n_layer
        new = lambda *shape, dtype: torch.empty(*shape, device=self.dev, dtype=dtype)
        if self._kv8_on():
            self.caches, self.kv = [], None
            if not self.kq and self.stacked:
                self.kqs = new(L, B, 2, H, self.tmax, D // H, dtype=torch.int8)
                self.kss = new(L, B, 2, H, self.tmax, dtype=torch.float32)
                self.kq, self.ks = list(self.kqs.unbind(0)), list(self.kss.unbind(0))
            elif not self.kq:
                self.kq = [new(B, 2, H, self.tmax, D // H, dtype=torch.int8) for _ in range(L)]
                self.ks = [new(B, 2, H, self.tmax, dtype=torch.float32) for _ in range(L)]
        else:
            self.kq, self.ks, self.kqs, self.kss = [], [], None, None
            if not self.caches and self.stacked:
                self.kv = new(L, B, self.tmax, 3 * D, dtype=torch.bfloat16)
                self.caches = list(self.kv.unbind(0))
            elif not self.caches:
                self.caches = [new(B, self.tmax, 3 * D, dtype=torch.bfloat16) for _ in range(L)]

    def cache_nbytes(self):
        """Bytes of this state's KV cache tensors."""
        ts = [self.kv] if self.kv is not None else self.caches + self.kq + self.ks
        return sum(t.numel() * t.element_size() for t in ts)

    def _keep(self, i, qkv):
        """Layer i's qkv rows [B, T, 3D] of a prompt into its cache.  A KV8 state snaps their K/V thirds
        in place first (``kv8_store``), so the prompt's own attention reads the snapped values."""
        B, T, D3 = qkv.shape
        if self.kv8:
            H = self.model.config.n_head
            if self._kv8_on():  # a beam state: one snap, the (q, s) stored to each of the prompt's beams
                self.C.kv8_store(qkv, H, self.kq[i], self.ks[i], self.kq[i].size(0) // B)
                return
            self.C.kv8_store(qkv, H)
        if self.caches[i].size(0) == B:
            self.caches[i][:, :T].copy_(qkv)
        else:  # a beam state: the prompt's rows go to each of its beams
            self.caches[i].view(B, -1, self.tmax, D3)[:, :, :T].copy_(qkv.view(B, 1, T, D3))

    def prefill(self, idx, last=None):
        """Run the prompt idx [B, T] on the MFMA GEMM path, keep every layer's qkv rows as the
        cache and set ``logits`` [B, V] to the last position's -- or, for a right-padded batch, to
        those of column ``last[b]`` (int64 [B]: the row's length - 1) of row b."""
        cfg = self.model.config
        B = idx.size(0)
        if self.kv8:
            self._kv8_storage()
        x = self._prompt(idx, self._keep)
        if last is not None:  # right-padded prefill: row b's hidden state at its own last token
            x = x[torch.arange(B, device=x.device), last]
        else:
            x = x[:, -1]
        self.logits = self._head(x.contiguous(), "mfma")[:, :cfg.vocab_size]
        return self.logits

    def _decode(self, tok, pos, hpos, pos_stride=0, am_part=None, seq=None):
        """One decode step, with nothing from the host: embed token ``tok`` [B, 1] (int64, on the
        device) at position ``pos`` (int32 on the device: [1], or with ``pos_stride`` 1 one per
        row, [B]), run the blocks -- each row appends its K/V at and attends up to its own cache
        row -- and return the LM head's padded logits [B, ld].  ``hpos``: a host-side position for
        the decode-attention binding's range check (the kernel reads ``pos``).

        ``am_part`` (int64 [B, G]; LM head on the skinny GEMM, V > 8192) fuses the greedy argmax:
        the LM-head kernel leaves one argmax key per (row, workgroup) in it and advances ``pos``,
        and the NEXT step's embedding kernel reduces the keys into its input token, which it also
        writes to ``tok`` and ``seq[:, pos]`` -- no cross-workgroup hand-off inside a kernel."""
        C, bf = self.C, self.bf
        tr, cfg = self.model.transformer, self.model.config
        B, D, H = tok.shape[0], cfg.n_embed, cfg.n_head
        route = self._route(B)
        x = C.embedding_fwd(tok, bf(tr.wte.weight), bf(tr.wpe.weight), 0.0, 0, pos, am_part, seq,
                            pos_stride).view(B, D)
        if self._kv8_on():
            attend = lambda i, qkv: C.attention_decode_kv8(qkv, self.kq[i], self.ks[i], H, hpos, pos, self.dec_part,
                                                           self.dec_cnt, pos_stride)
        elif self.kv8:  # the KV8 model on the bf16 kernel: snap the step's K/V in place, then attend

            def attend(i, qkv):
                C.kv8_store(qkv.view(B, 1, 3 * D), H)
                return C.attention_decode(qkv, self.caches[i], H, hpos, pos, self.dec_part, self.dec_cnt, pos_stride)
        else:
            attend = lambda i, qkv: C.attention_decode(qkv, self.caches[i], H, hpos, pos, self.dec_part,
                                                       self.dec_cnt, pos_stride)
        x = self._blocks(x, attend, route)
        return self._head(x, route, am=(am_part, pos) if am_part is not None else None)

    def _stamp(self):
        # the weights' stamp, which skinny GEMM and which decode attention the steps launch: a loop
        # captured for one kernel is never replayed for the other
        return _weight_stamp(self.model), self._w8_on(), self._kv8_on()

    def _fresh(self):
        if self.kv8:
            self._kv8_storage()
        st = self._stamp()
        if st != self.stamp:  # a weight moved or changed: captured pointers / bf16 copies are stale
            self.stamp = st
            self._loops.clear()

    def _loop(self, key, make):
        """The loop kept under ``key``; ``make()`` builds it on first use and again after a weight
        change, which drops every loop with its graph and buffers."""
        self._fresh()
        if key not in self._loops:
            self._loops[key] = make()
        return self._loops[key]

    @staticmethod
    def _key(base, proc, logprobs):
        """The key of a picked loop: ``base``, ``_proc`` with the process kernel in its step, ``_lp``
        with the lse kernel."""
        return base + ("_proc" if proc else "") + ("_lp" if logprobs else "")

    def _tok_state(self, per_row, cols, lp, tok=None, pos=0):
        """The device state of a token loop: ``tok`` int64 [B, 1] (the newest token, the next step's
        input), ``pos`` int32 (its position: [B] with ``per_row``, beside a finished flag ``done``
        int32 [B]; else [1] for the batch), ``seq`` int64 [B, cols] (the tokens by column) and with
        ``lp`` their log-probabilities ``lp`` float32 [B, cols]; ``hpos``: ``_decode``'s."""
        B = self.B if tok is None else tok.shape[0]
        zeros = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=self.dev)
        st = {"tok": zeros(B, 1, dtype=torch.long) if tok is None else tok.clone(),
              "pos": torch.full((B if per_row else 1,), pos, dtype=torch.int32, device=self.dev),
              "seq": zeros(B, cols, dtype=torch.long), "hpos": max(pos, 1)}
        if per_row:
            st["done"] = zeros(B, dtype=torch.int32)
        if lp:
            st["lp"] = zeros(B, cols, dtype=torch.float32)
        return st

    @staticmethod
    def _seed(st, tok, pos, ctx=None):
        """Point a rectangular loop's device state at token ``tok`` [B, 1] at position ``pos``.
        ``ctx`` [B, pos] (the processors are on), the window's context: ``seq`` holds it in columns
        0 .. pos - 1 and ``tok`` at column pos, since the process kernel reads the history from there."""
        st["tok"].copy_(tok)
        st["pos"].fill_(pos)
        st["hpos"] = max(pos, 1)
        if ctx is not None:
            st["seq"][:, :pos].copy_(ctx)
            st["seq"][:, pos:pos + 1].copy_(tok)

    @staticmethod
    def _picked(st, pos, n, logprobs):
        """What a run of n steps from position ``pos`` left in ``seq``: the new tokens [B, n], with
        ``logprobs`` (tokens, lp [B, n])."""
        toks = st["seq"][:, pos + 1:pos + 1 + n]
        return (toks, st["lp"][:, pos + 1:pos + 1 + n]) if logprobs else toks

    def step(self, tok, pos):
        """One decode step with token ``tok`` [B, 1] at position ``pos``, over static token /
        position buffers; the KV caches are persistent buffers the kernels append to.  Returns
        the logits [B, V]."""
        V = self.model.config.vocab_size

        def make():
            st = {"tok": tok.clone(), "pos": torch.full((1,), pos, dtype=torch.int32, device=tok.device),
                  "hpos": max(pos, 1)}
            return _Loop(lambda: self._decode(st["tok"], st["pos"], st["hpos"])[:, :V], st)

        lp = self._loop("step", make)
        self._seed(lp.state, tok, pos)
        lp.run(1)
        return lp.logits

    def with_logprob(self, tok):
        """(tok, lp): token ``tok`` [B] picked from the prefill logits, with its log-probability
        [B] from the lse kernel."""
        return tok, self.C.logits_lse(self.logits, self.model.config.vocab_size, tok.contiguous())[1]

    def _lp_args(self, logits, V, st, logprobs):
        """The trailing ``(lse, lp)`` arguments of a pick call on ``logits``: with ``logprobs`` the
        lse kernel's {m, lnz} of these logits and the state's ``lp`` buffer, else nothing -- no
        launch, and a state that owns an ``lp`` buffer from an earlier call does not pass it."""
        return (self.C.logits_lse(logits, V), st["lp"]) if logprobs else (None, None)

    def _process(self, logits, st, pos_stride, done=None):
        """The process kernel on a step's ``logits`` in place: row b's history is columns 0 ..
        pos[b] of the state's own ``seq``, which the step's pick kernel extends.  Its settings are
        this state's process block (``_proc_words``), set by the caller."""
        self.C.logits_process(logits, self.model.config.vocab_size, st["seq"][:, :self.tmax], st["pos"], pos_stride,
                              done, self._pparams.dev)

    def process_prefill(self, ctx, proc):
        """Edit the prefill logits in place with the processors ``proc`` (``_proc_words``) over the
        context ``ctx`` [B, L] they were computed from: one eager launch before a window's first pick."""
        pos = torch.full((1,), ctx.size(1) - 1, dtype=torch.int32, device=ctx.device)
        self.C.logits_process(self.logits, self.model.config.vocab_size, ctx, pos, 0, None, self._pparams.set(proc))

    def _ragged_step(self, st, greedy, logprobs, proc=False):
        """The decode step over per-row state ``st`` (``pos``, ``done``, ``tok``, ``seq``, ``params``,
        with ``logprobs`` also ``lp``): ``_decode`` with one position per row, then the ragged pick
        kernel, greedy or sampled.  ``proc``: the process kernel on the logits first (and before the
        lse kernel: the log-probability is the processed row's)."""
        V = self.model.config.vocab_size

        def step():
            logits = self._decode(st["tok"], st["pos"], 1, pos_stride=1)
            if proc:
                self._process(logits, st, 1, st["done"])
            self.C.pick_ragged(logits, V, st["params"], st["pos"], st["done"], st["tok"], st["seq"], greedy,
                               *self._lp_args(logits, V, st, logprobs))
            return logits[:, :V]

        return step

    def _greedy_picked(self, tok, pos, n, logprobs, proc, ctx):
        """``greedy`` with log-probabilities and / or the logits processors ``proc`` (``_proc_words``,
        with the window's context ``ctx``): loops ``"greedy_lp"``, ``"greedy_proc"``,
        ``"greedy_proc_lp"``.  Not the LM head's fused argmax, whose keys have no room for the number
        and which cannot see edited logits, but the ragged greedy step (``_ragged_step``) on equal
        positions over a state of its own, with no stop token.  Both rank the stored bf16 logits
        with the first index on ties.  ``seq`` / ``lp`` are one column longer than the ragged
        state's: the pick kernel keeps the position below the last column, and a window's last
        token sits at column tmax."""
        on = proc is not None
        if on:
            self._pparams.set(proc)

        def make():
            st = self._tok_state(True, self.tmax + 2, logprobs, tok, pos)
            st["params"] = torch.tensor(_ragged_words(0, 1.0, None, None), dtype=torch.int32, device=self.dev)
            return _Loop(self._ragged_step(st, True, logprobs, proc=on), st)

        lp = self._loop(self._key("greedy", on, logprobs), make)
        self._seed(lp.state, tok, pos, ctx if on else None)  # again: the warm-up step moved the state
        lp.run(n)
        return self._picked(lp.state, pos, n, logprobs)

    def greedy(self, tok, pos, n, logprobs=False, proc=None, ctx=None):
        """n greedy decode steps starting with token ``tok`` [B, 1] at position ``pos``: the step
        takes its input token and position from device buffers that its own kernels advance (the
        fused argmax of ``_decode`` when the rows fit the skinny GEMM -- B <= 8, 4 * n_embed <= 8192
        -- and V > 8192; otherwise the argmax in torch).  Returns the n
        new tokens [B, n] (positions pos + 1 .. pos + n); with ``logprobs`` also their
        log-probabilities [B, n], and with ``proc`` the argmax of the processed rows
        (``_greedy_picked``)."""
        assert pos + n <= self.tmax
        if logprobs or proc is not None:
            return self._greedy_picked(tok, pos, n, logprobs, proc, ctx)
        B = tok.shape[0]
        V = self.model.config.vocab_size

        def seed(st):
            self._seed(st, tok, pos)
            if st["part"] is not None:  # keys that every real logit loses to, argmax = tok
                st["part"].zero_()
                st["part"][:, :1].copy_(-1 - tok)  # bits 0xffffffff_(0xffffffff - tok)

        def make():
            fused = self._route(B) == "gemv" and V > 8192
            st = self._tok_state(False, self.tmax + 1, False, tok, pos)
            st["part"] = (torch.zeros(B, self.C.gemv_argmax_groups(V, B), dtype=torch.long, device=self.dev)
                          if fused else None)
            seed(st)
            if fused:
                return _Loop(lambda: self._decode(st["tok"], st["pos"], st["hpos"], am_part=st["part"],
                                                  seq=st["seq"])[:, :V], st)

            def step():  # small vocab (no fused argmax): the same in torch
                logits = self._decode(st["tok"], st["pos"], st["hpos"])[:, :V]
                nxt = logits.argmax(-1)
                st["tok"].view(B).copy_(nxt)
                st["seq"].index_copy_(1, st["pos"].long() + 1, nxt.view(B, 1))
                st["pos"].add_(1)
                return logits

            return _Loop(step, st)

        lp = self._loop("greedy", make)
        st = lp.state
        seed(st)  # again: the warm-up step moved the state
        lp.run(n)
        if st["part"] is None:
            return self._picked(st, pos, n, False)
        # the last step's token is still in its LM-head keys: reduce them here (unsigned max =
        # signed max after flipping the top bit; low word = 0xffffffff - column)
        k = (st["part"] ^ _I64_MIN).max(dim=1).values ^ _I64_MIN
        last = 0xFFFFFFFF - (k & 0xFFFFFFFF)
        return torch.cat([st["seq"][:, pos + 1:pos + n], last.view(B, 1)], dim=1)

    def sample_prefill(self, words):
        """The token [B] drawn from the prefill logits (the first token of a context window)."""
        return self.C.sample_logits(self.logits, self.model.config.vocab_size, self._sparams.set(words, always=True))

    def sample(self, tok, pos, n, words, logprobs=False, proc=None, ctx=None):
        """n sampled decode steps starting with token ``tok`` [B, 1] at position ``pos``: each step
        is the plain LM head followed by the sample kernel, which writes the next token into the
        buffer the next step's embedding reads and advances the device position and draw counter.
        Seed, temperature, top-k and top-p live in the device parameter block (``words``,
        ``_sample_words``), so the one captured step serves every call; the kernel advances the
        block's draw counter, so every call uploads it.  Returns the n new tokens [B, n] (positions
        pos + 1 .. pos + n).  ``logprobs``: a loop of its own (``"sample_lp"``) with the lse kernel
        between the LM head and the sampler, which writes each token's log-probability beside it;
        returns (tokens, lp [B, n]).  ``proc`` (``_proc_words``; with ``ctx`` [B, pos], the window's
        context): loops of their own again (``"sample_proc"`` / ``"sample_proc_lp"``) with the process
        kernel right after the LM head."""
        assert pos + n <= self.tmax
        V = self.model.config.vocab_size
        on = proc is not None
        if on:
            self._pparams.set(proc)

        def make():
            st = self._tok_state(False, self.tmax + 1, logprobs, tok, pos)
            params = self._sparams.set(words, always=True)

            def step():
                logits = self._decode(st["tok"], st["pos"], st["hpos"])
                if on:
                    self._process(logits, st, 0)
                self.C.sample_logits(logits, V, params, st["pos"], st["tok"], st["seq"],
                                     *self._lp_args(logits, V, st, logprobs))
                return logits[:, :V]

            return _Loop(step, st)

        lp = self._loop(self._key("sample", on, logprobs), make)
        self._seed(lp.state, tok, pos, ctx if on else None)
        self._sparams.set(words, always=True)
        lp.run(n)
        return self._picked(lp.state, pos, n, logprobs)

    # ----------------------------------------------------------------- ragged batches
    def ragged_state(self):
        """The per-row device state of the ragged loop, allocated once per decode state (the
        captured steps bake the pointers in, and it outlives them): ``pos`` int32 [B] (position of
        the row's newest token), ``done`` int32 [B], ``tok`` int64 [B, 1] (the newest token, the
        next step's input), ``seq`` int64 [B, tmax + 1] and the pick kernels' own parameter block
        ``params``."""
        if self._rstate is None:
            self._rstate = self._tok_state(True, self.tmax + 1, False)
            self._rstate["params"] = self._rparams.dev
        return self._rstate

    def ragged_start(self, idx, lengths, words, greedy, logprobs=False, proc=None):
        """Point the ragged state at a prefilled right-padded batch ``idx`` [B, Tp] with ``lengths``
        [B] (``self.logits`` = row b's logits at column lengths[b] - 1) and pick every row's first
        token with the loop's own pick kernel: pos = lengths - 1 and done = 0 going in.
        ``logprobs``: the state's ``lp`` buffer (float32, the shape of ``seq``; allocated on first
        use) is zeroed with ``seq`` and gets the first tokens' log-probabilities.  ``proc``
        (``_proc_words``): the prefill logits are edited by the process kernel over each row's own
        prompt first."""
        st = self.ragged_state()
        if logprobs:
            if "lp" not in st:
                st["lp"] = torch.zeros(st["seq"].shape, dtype=torch.float32, device=st["seq"].device)
            st["lp"].zero_()
        st["seq"].zero_()
        st["seq"][:, :idx.size(1)].copy_(idx)
        st["pos"].copy_(lengths - 1)
        st["done"].zero_()
        self._rparams.set(words)
        logits = self.logits  # [B, V] view of the padded [B, ld] buffer the LM head wrote
        if proc is not None:
            self._pparams.set(proc)
            self._process(logits, st, 1, st["done"])
        self.C.pick_ragged(logits, logits.size(1), st["params"], st["pos"], st["done"], st["tok"], st["seq"],
                           greedy, *self._lp_args(logits, logits.size(1), st, logprobs))
        return st

    def ragged(self, n, words, greedy, logprobs=False, proc=None):
        """n decode steps of a ragged batch on the current device state (``ragged_state``): embed
        ``tok[b]`` at ``pos[b]``, the blocks with per-row decode attention, the plain LM head, then
        the pick kernel -- greedy argmax or the seeded draw with counter ``pos[b] + 1`` -- which
        writes the row's next token and advances its position, or leaves a finished row alone.  A
        finished row keeps flowing through the step with its token and position frozen (it re-embeds
        the same token and rewrites the same cache row), so the launch shapes never change: one
        loop per mode (``_loops[("ragged", greedy)]``).  Resumable: n calls of one step equal one
        call of n steps.  ``words``: the parameter block (``_ragged_words``).  Returns the state;
        the last step's logits are the loop's ``logits``.  ``logprobs`` (after a ``ragged_start``
        with it): loops of their own (``("ragged_lp", greedy)``) with the lse kernel before the pick
        kernel, which writes ``lp[b, pos[b] + 1]`` with the token.  ``proc`` (``_proc_words``, after
        a ``ragged_start`` with it): loops of their own once more (``("ragged_proc", greedy)`` /
        ``("ragged_proc_lp", greedy)``) with the process kernel right after the LM head, reading each
        row's history from ``seq``."""
        st = self.ragged_state()
        self._rparams.set(words)
        on = proc is not None
        if on:
            self._pparams.set(proc)
        step = self._ragged_step(st, greedy, logprobs, proc=on)

        def warm():  # with every row marked finished the step is idempotent: the state the caller
            done = st["done"].clone()  # set up is left as it is
            st["done"].fill_(1)
            step()
            st["done"].copy_(done)

        self._loop((self._key("ragged", on, logprobs), greedy), lambda: _Loop(step, st, warm)).run(n)
        return st

    # ----------------------------------------------------------------- beam search
    def beam_state(self, W):
        """The device state of the beam loop with W beams per prompt on this state's B * W rows
        (row b * W + w = beam w of prompt b), allocated once (the captured step bakes the pointers
        in): ``tok`` int64 [R, 1] (the next step's input), ``pos`` int32 [1] (one position for the
        batch), ``ctl`` int32 [4] = {history column, stop token or -1, pad token, 0}, per beam
        ``score`` fp32, ``fin`` / ``len`` / ``parent`` int32 [R], the row kernel's candidates and
        ``lse``, and the per-step histories ``hparent`` / ``htok`` (int32 [B, W, tmax + 1]) and
        ``hscore`` (fp32), indexed by the column of the step's token in the sequence."""
        states = self._bstate
        if W not in states:
            dev, R = self.dev, self.B
            assert R % W == 0
            i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
            f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            start = torch.full((R // W, W), float("-inf"), dtype=torch.float32)
            start[:, 0] = 0.0  # only beam 0 is live going into the first step
            states[W] = {"tok": torch.zeros(R, 1, dtype=torch.long, device=dev), "pos": i32(1), "ctl": i32(4),
                         "score": f32(R), "fin": i32(R), "len": i32(R), "parent": i32(R),
                         "cand_tok": i32(R, W), "cand_c": f32(R, W), "lse": f32(R, 2),
                         "hparent": i32(R // W, W, self.tmax + 1), "htok": i32(R // W, W, self.tmax + 1),
                         "hscore": f32(R // W, W, self.tmax + 1), "score0": start.view(R).to(dev)}
        return states[W]

    def _beam_tail(self, st, W, logits):
        """The end of a beam step on the padded logits [R, ld]: the row kernel ({m, lnz} and W
        candidates per row), the merge (the prompt's W best become its beams; the position
        advances) and the in-place reorder of every layer's K / V rows by parent beam (the history
        column advances)."""
        C, V = self.C, self.model.config.vocab_size
        C.beam_rows(logits, V, W, st["score"], st["fin"], st["ctl"], st["cand_tok"], st["cand_c"], st["lse"])
        C.beam_merge(W, V, st["cand_tok"], st["cand_c"], st["score"], st["fin"], st["len"], st["tok"], st["parent"],
                     st["hparent"], st["htok"], st["hscore"], st["pos"], st["ctl"])
        if self._kv8_on():  # the int8 cache: (q, s) pairs move unchanged
            reorder = lambda sl, ctl: C.beam_reorder_kv8(self.kqs[sl], self.kss[sl], W, st["parent"], st["pos"], ctl)
        else:
            reorder = lambda sl, ctl: C.beam_reorder(self.kv[sl], W, st["parent"], st["pos"], ctl)
        if _BEAM_REORDER_PER_LAYER:
            for i in range(self.model.config.n_layer):
                reorder(slice(i, i + 1), st["ctl"] if i == 0 else None)
        else:
            reorder(slice(None), st["ctl"])

    def beam(self, W):
        """The beam loop of this state (``_loops[("beam", W)]``): ``_decode`` at one batch-wide
        position, then ``_beam_tail``.  A finished beam keeps flowing through the step with the pad
        token as its input and what it computes is ignored, so the launch shapes never change.
        Build it BEFORE the prefill: the warm-up step runs on whatever the state holds (all zeros
        the first time: position 0, token 0) and moves it."""
        st = self.beam_state(W)
        V = self.model.config.vocab_size

        def step():
            logits = self._decode(st["tok"], st["pos"], 1)
            self._beam_tail(st, W, logits)
            return logits[:, :V]

        return self._loop(("beam", W), lambda: _Loop(step, st))

    def beam_prefill(self, idx, W):
        """Prefill the B prompts idx [B, T] once: every layer's qkv rows go to the W beams of their
        prompt (``_prompt``), and the last position's padded logits [B, ld] come back W times over,
        [B * W, ld] -- the input of the first beam step."""
        x = self._prompt(idx, self._keep)[:, -1]
        full = self._head(x.contiguous(), "mfma")
        self.logits = full[:, :self.model.config.vocab_size]
        return full.repeat_interleave(W, dim=0)

    def beam_start(self, W, T, logits, eos_token, pad_token):
        """Point the beam state at prompts of T tokens whose (broadcast) last-position logits are
        ``logits`` and take the first step: the row and merge kernels with only beam 0 live."""
        st = self.beam_state(W)
        st["pos"].fill_(T - 1)
        st["ctl"].copy_(torch.tensor([T, -1 if eos_token is None else int(eos_token), int(pad_token), 0],
                                     dtype=torch.int32))
        st["score"].copy_(st["score0"])
        st["fin"].zero_()
        st["len"].fill_(T)
        self._beam_tail(st, W, logits)
        return st

    # ----------------------------------------------------------------- speculative decoding
    def spec_state(self, K):
        """The device state of the speculative loop with K rows per sequence on this state's B
        sequences (row b * K + r = row r of sequence b), allocated once (the captured step bakes the
        pointers in): ``seq`` int64 [B, tmax + 1] (the committed tokens), ``pos`` int32 [B] (the
        column of a sequence's newest token), ``ctl`` int32 [4] = {ngram, end, 0, 0}, the step's
        rows ``tok`` int64 [B * K, 1] / ``pos_rows`` int32 [B * K] / ``has`` int32 [B] / ``g`` int32
        [B * K], the statistics ``steps`` int32 [B] and ``hist`` int32 [B, K + 1], and the grouped
        decode attention's workspace for B * K rows."""
        states = self._sstate
        if K not in states:
            dev, B, cfg = self.dev, self.B, self.model.config
            H = cfg.n_head
            i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
            states[K] = {"seq": torch.zeros(B, self.tmax + 1, dtype=torch.long, device=dev), "pos": i32(B),
                         "ctl": i32(4), "tok": torch.zeros(B * K, 1, dtype=torch.long, device=dev),
                         "pos_rows": i32(B * K), "has": i32(B), "g": i32(B * K), "steps": i32(B),
                         "hist": i32(B, K + 1),
                         "part": torch.empty(self.C.attention_decode_part_floats(B * K, H, cfg.n_embed // H),
                                             device=dev, dtype=torch.float32),
                         "cnt": i32(B * K * H)}
        return states[K]

    def spec(self, K):
        """The speculative loop of this state (``_loops[("spec", K)]``; the rule in common.h): the
        draft kernel, the embedding with one position per row, the blocks on the skinny GEMM with the
        grouped decode attention (K rows share a sequence's cache), the plain LM head, the row argmax
        and the accept kernel, which writes the emitted tokens to ``seq`` and advances ``pos``.  A
        finished sequence (pos == end) keeps flowing through the step and the accept kernel leaves
        it alone, so the launch shapes never change.  Build it BEFORE the prefill: the warm-up step
        runs with end = 0 -- every sequence finished, no state moved -- but writes K/V rows."""
        st = self.spec_state(K)
        C, bf = self.C, self.bf
        tr, cfg = self.model.transformer, self.model.config
        D, H, V = cfg.n_embed, cfg.n_head, cfg.vocab_size
        R = self.B * K
        if self._route(R) != "gemv":  # R <= 8 rows of at most 8192 columns (gemv.hip)
            raise RuntimeError(f"speculative decoding: {R} rows of width {4 * D} do not fit the skinny GEMM")

        if self._kv8_on():
            attend = lambda i, qkv: C.attention_decode_kv8(qkv, self.kq[i], self.ks[i], H, 0, st["pos_rows"],
                                                           st["part"], st["cnt"], 1, K)
        elif self.kv8:  # the KV8 model on the bf16 kernel: snap the step's rows in place, then attend

            def attend(i, qkv):
                C.kv8_store(qkv.view(R, 1, 3 * D), H)
                return C.attention_decode(qkv, self.caches[i], H, 0, st["pos_rows"], st["part"], st["cnt"], 1, K)
        else:
            attend = lambda i, qkv: C.attention_decode(qkv, self.caches[i], H, 0, st["pos_rows"], st["part"],
                                                       st["cnt"], 1, K)

        def step():
            C.spec_draft(st["seq"], st["pos"], st["ctl"], K, st["tok"], st["pos_rows"], st["has"])
            x = C.embedding_fwd(st["tok"], bf(tr.wte.weight), bf(tr.wpe.weight), 0.0, 0, st["pos_rows"], None, None,
                                1).view(R, D)
            x = self._blocks(x, attend, "gemv")
            logits = self._head(x, "gemv")
            C.spec_argmax(logits, V, st["g"])
            C.spec_accept(st["g"], st["tok"], st["has"], K, st["pos"], st["ctl"], st["seq"], st["steps"], st["hist"])
            return logits[:, :V]

        def warm():
            st["ctl"].zero_()
            st["pos"].zero_()
            step()

        return self._loop(("spec", K), lambda: _Loop(step, st, warm))

    def spec_start(self, K, idx, first, n, ngram):
        """Point the speculative state at the prefilled prompts ``idx`` [B, T] with the first new
        token ``first`` [B] at column T: pos = T, end = T + n - 1, the statistics zeroed."""
        st = self.spec_state(K)
        T = idx.size(1)
        st["seq"].zero_()
        st["seq"][:, :T].copy_(idx)
        st["seq"][:, T].copy_(first)
        st["pos"].fill_(T)
        st["ctl"].copy_(torch.tensor([int(ngram), T + n - 1, 0, 0], dtype=torch.int32))
        st["steps"].zero_()
        st["hist"].zero_()
        return st


_I64_MIN = -(1 << 63)


def _f32_bits(v):
    """float32(v) as the int32 word of a parameter block."""
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _sample_words(seed, draw, temperature, top_k, top_p=None):
    """The sample kernel's parameter block as 8 int32: seed low / high word, draw counter,
    float32(1 / temperature) as bits, top_k (0: off), 0, float32(top_p) as bits (0: off), 0."""
    s32 = lambda x: ((x & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    p = R.sample_top_p(top_p)
    return [s32(seed), s32(seed >> 32), s32(draw), _f32_bits(1.0 / temperature), min(int(top_k or 0), 0x7FFFFFFF),
            0, 0 if p is None else _f32_bits(p), 0]


_PROC_HIST_MAX = 4096  # history entries the process kernel stages (kernels.h kProcHistMax)


def _proc_words(repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size):
    """The process kernel's parameter block as 8 int32 (the rule in common.h, 'Logits processors'):
    float32(repetition_penalty), float32(1 / repetition_penalty), float32(presence_penalty) and
    float32(frequency_penalty) as bits, no_repeat_ngram_size, 0, 0, 0."""
    vals = R.process_values(repetition_penalty, presence_penalty, frequency_penalty)
    return [_f32_bits(v) for v in vals] + [int(no_repeat_ngram_size), 0, 0, 0]


def _processors(who, model, kernel, repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size):
    """(args, words) of a call's logits processors -- the arguments as ``R.process_logits`` takes them
    and the device parameter block -- or (None, None) when every one is at its off value.
    ``kernel``: the call goes through the process kernel, whose history is bounded."""
    args = (repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size)
    if not R.check_process_args(*args):
        return None, None
    if kernel and model.block_size > _PROC_HIST_MAX:
        raise ValueError(f"{who}: the logits processors keep at most {_PROC_HIST_MAX} history tokens on the "
                         f"device, block_size is {model.block_size}")
    return args, _proc_words(*args)


def _weight_stamp(model):
    return tuple((p.data_ptr(), p._version) for p in model.parameters())


def _ragged_words(seed, temperature, top_k, eos_token, top_p=None):
    """The parameter block of the ragged pick kernels: ``_sample_words`` (the draw counter is not
    used: it is the row's position + 1) with the stop token in word 5, -1 for none."""
    w = _sample_words(seed, 0, temperature, top_k, top_p)
    w[5] = -1 if eos_token is None else int(eos_token)
    return w


_STATE_SLOTS = ("_mg_decode_cache", "_mg_kv8_cache", "_mg_beam_cache", "_mg_beam_kv8_cache", "_mg_spec_cache",
                "_mg_spec_kv8_cache")
# the bf16 slot of each kind of state and the KV8 slot kept beside it
_KV8_SLOTS = {"_mg_decode_cache": "_mg_kv8_cache", "_mg_beam_cache": "_mg_beam_kv8_cache",
              "_mg_spec_cache": "_mg_spec_kv8_cache"}


def _kv_slot(who, kv_cache, slot="_mg_decode_cache"):
    """(slot, kv8) of a ``kv_cache`` argument: ``"bf16"`` is the state ``slot`` (the plain one, or the
    beam / speculative state), ``"int8"`` the KV8 state kept beside it, so alternating calls rebuild
    neither and a KV8 call never touches a bf16 state or its graphs.  ValueError for anything else."""
    if kv_cache not in _KV_CACHES:
        raise ValueError(f"{who}: kv_cache must be one of {_KV_CACHES}, got {kv_cache!r}")
    return (_KV8_SLOTS[slot], True) if kv_cache == "int8" else (slot, False)


def kv_cache_nbytes(model):
    """{state slot: bytes of its KV cache tensors} for every decode state ``model`` keeps: ``_mg_decode_cache``
    (bf16 qkv rows, 6 D bytes per token and layer), ``_mg_kv8_cache`` (``kv_cache="int8"``: 2 D + 8 H bytes),
    ``_mg_beam_cache``, ``_mg_spec_cache`` and their KV8 states ``_mg_beam_kv8_cache``, ``_mg_spec_kv8_cache``."""
    return {slot: model.__dict__[slot].cache_nbytes() for slot in _STATE_SLOTS if model.__dict__.get(slot) is not None}


def _state_for(model, slot, idx, tmax, rows=None, last=None):
    """The decode state the model keeps under ``slot`` -- ``_mg_decode_cache``, beside it ``_mg_beam_cache`` /
    ``_mg_spec_cache`` of ``rows`` decode rows, so that beam and speculative calls leave the plain loops
    and their graphs alone, and the KV8 state of each (``_kv_slot``) -- or a new one when the device,
    the rows or ``tmax`` differ.  The
    plain state comes back prefilled with ``idx`` (``last``: ``_GpuCache.prefill``); the others are
    prefilled by their callers, after the loop is built."""
    c = model.__dict__.get(slot)
    if c is None or c.B != (rows or idx.size(0)) or c.tmax != tmax or c.dev != idx.device:
        c = model.__dict__[slot] = _GpuCache(model, idx, tmax, last, rows, kv8=slot in _KV8_SLOTS.values())
    elif rows is None:
        c.prefill(idx, last)
    return c


def _replay(run, n, flags, eos_token):
    """``run(k)`` for n captured steps in all; returns the steps taken.  With a stop token (without
    one nothing finishes early) and ``_EARLY_EXIT`` the device's finished ``flags`` are read every
    ``_EXIT_EVERY`` steps, and the rest is left out once every one is set."""
    check, left = _EARLY_EXIT and eos_token is not None, n
    while left > 0:
        k = min(left, _EXIT_EVERY) if check else left
        run(k)
        left -= k
        if check and left > 0 and bool(flags.all()):
            break
    return n - left


def _check_entry(who, model, max_new_tokens, idx=None, longest=None):
    """ValueError unless ``idx`` is a rectangular int64 prompt batch (or, for ragged prompts, given
    their ``longest``), ``max_new_tokens`` >= 0 and both fit ``block_size``; returns int(max_new_tokens)."""
    what, T = "longest prompt", longest
    if longest is None:
        if not (torch.is_tensor(idx) and idx.dim() == 2 and idx.dtype == torch.long and idx.size(0) >= 1
                and idx.size(1) >= 1):
            raise ValueError(f"{who}: idx must be an int64 [B, T] tensor with B, T >= 1")
        what, T = "prompt", idx.size(1)
    n, bs = int(max_new_tokens), model.block_size
    if n < 0:
        raise ValueError(f"{who}: max_new_tokens must be >= 0, got {max_new_tokens}")
    if T + n > bs:
        raise ValueError(f"{who}: {what} ({T}) + max_new_tokens ({n}) exceeds block_size ({bs}); this entry "
                         f"point has no sliding window")
    return n


@torch.no_grad()
def generate(model, idx, max_new_tokens: int, temperature: float = 1.0, do_sample: bool = False,
             top_k: Optional[int] = None, use_cache: bool = True, seed: Optional[int] = None,
             top_p: Optional[float] = None, return_logprobs: bool = False, repetition_penalty: float = 1.0,
             presence_penalty: float = 0.0, frequency_penalty: float = 0.0, no_repeat_ngram_size: int = 0,
             kv_cache: str = "bf16"):
    """``kv_cache``: ``"bf16"`` (default: every path as it is without the argument) or ``"int8"``, the KV8
    model (the rule in common.h, ``ops.quant.snap_vectors``): every K and V vector -- one per sequence,
    position, layer and head -- is snapped to int8 values times one power-of-two scale before any
    attention reads it, prompt and new tokens alike, on the GPU and the CPU; Q is untouched.  On the GPU
    the cache is then int8 with one fp32 scale per vector, 2 D + 8 H bytes per token and layer instead of
    6 D, read by ``attention_decode_kv8`` (``_mg_kv8_cache``, a state of its own).  Needs ``use_cache``;
    ValueError for any other string.

    ``repetition_penalty`` (finite, > 0; 1.0 off), ``presence_penalty``, ``frequency_penalty``
    (finite; 0.0 off), ``no_repeat_ngram_size`` (0 .. 8; 0 off): the logits processors (the rule in
    common.h, 'Logits processors'), applied to the stored logits before the temperature, top-k, top-p
    and the draw; greedy takes the argmax of the processed row.  A token seen c >= 1 times in the
    history has its logit x replaced by (x > 0 ? x / rp : x * rp) - (fp * c + pp), and with
    ``no_repeat_ngram_size = g`` every token that would complete a g-gram already in the history gets
    -inf.  The history of the token at column T is ``idx[b, max(0, T - block_size):T]`` -- exactly
    the context the model saw, NOT the whole sequence as in libraries that keep it all: past
    ``block_size`` the oldest tokens drop out of the penalties as they drop out of the attention,
    which bounds the history by ``block_size``.  With any processor on, ``return_logprobs`` reports
    the log-softmax of the processed row.  On the GPU (greedy or seeded) the process kernel runs
    inside the captured step, in loops of their own; with every argument at its off value every
    path is what it is without them.  ValueError for anything else.

    ``return_logprobs``: return ``(idx, logprobs)``, ``logprobs`` float32 of ``idx``'s shape --
    entry [b, j] is the model's log-probability of ``idx[b, j]`` given ``idx[b, :j]`` (the cropped
    window past ``block_size``, as for the token itself) at every generated position and 0.0 at the
    prompt's.  It is the log-softmax of the model's logits at temperature 1, before top-k and
    top-p, whatever the sampling settings (the rule in common.h): on the device loops from the lse
    kernel inside the captured step, on the host loops from ``ops.reference.token_logprob``.

    ``top_p`` (with ``do_sample``): nucleus filtering after the temperature and top-k -- keep the
    tokens whose probability mass strictly above them is below ``top_p`` of the total, ties kept
    together (the rule in common.h); None or 1.0 is off.  With a seed it is a word of the sample
    kernel's parameter block, so the captured loop serves any value.

    ``seed`` (with ``do_sample``): draw by the counter-based Gumbel-max rule (common.h,
    ``ops.reference.sample_gumbel``) instead of torch's global generator -- the tokens depend on
    (seed, column, batch row, logits) only, and on the GPU the whole token loop stays on the device
    (``_GpuCache.sample``).  ``seed=None`` leaves every path as it was."""
    bs = model.block_size
    slot, kv8 = _kv_slot("generate", kv_cache)
    if kv8 and not use_cache:
        raise ValueError("generate: kv_cache='int8' needs use_cache=True (without a cache there is nothing to "
                         "quantize)")
    seeded = do_sample and seed is not None
    if seeded or (do_sample and top_p is not None):
        R.check_sample_args(temperature, top_k, top_p)
    if seeded:
        seed = int(seed) & ((1 << 64) - 1)
    on_device = idx.is_cuda and use_cache and max_new_tokens > 0 and (seeded or not do_sample)  # the device loops
    proc, pwords = _processors("generate", model, on_device, repetition_penalty, presence_penalty,
                               frequency_penalty, no_repeat_ngram_size)

    def edit(logits, hist):  # host loops: the processors on the logits of the token after ``hist``
        return logits if proc is None else R.process_logits(logits, hist, *proc)

    def pick(logits, col):
        if seeded:
            return R.sample_gumbel(logits, temperature, top_k, seed, col, top_p=top_p)
        return _sample(logits, temperature, do_sample, top_k, top_p)

    lps = []  # host loops: one [B] per generated token

    def done(idx):
        if not return_logprobs:
            return idx
        lp = torch.zeros(idx.shape, dtype=torch.float32, device=idx.device)
        if lps:
            lp[:, idx.size(1) - len(lps):] = torch.stack(lps, dim=1)
        return idx, lp

    # ZeRO-1: the KV-cache path launches the kernels directly (never model.forward), so neither
    # the fused ops' per-bucket waits nor the engine's forward pre-hook run: wait here for every
    # in-flight parameter all-gather (stream-ordered) before any decode kernel reads the weights
    before_use(*model.parameters())
    if not use_cache:
        for _ in range(max_new_tokens):
            idx_cond = idx if idx.size(1) <= bs else idx[:, -bs:]
            logits, _ = model(idx_cond)
            last = edit(logits[:, -1, :], idx_cond)
            nxt = pick(last, idx.size(1))
            if return_logprobs:
                lps.append(R.token_logprob(last, nxt))
            idx = torch.cat((idx, nxt), dim=1)
        return done(idx)
    if on_device:
        if seeded:  # the draw counter of a token is its column T
            words = lambda T: _sample_words(seed, T, temperature, top_k, top_p)
            first = lambda c, T, ctx: c.sample_prefill(words(T))
            loop = lambda c, tok, L, n, T, ctx: c.sample(tok, L, n, words(T), logprobs=return_logprobs,
                                                         proc=pwords, ctx=ctx)
        else:
            first = lambda c, T, ctx: c.logits.argmax(-1)
            loop = lambda c, tok, L, n, T, ctx: c.greedy(tok, L, n, logprobs=return_logprobs, proc=pwords, ctx=ctx)
        return _generate_windowed_gpu(model, idx, max_new_tokens, first, loop, return_logprobs, pwords, slot)
    cache = None
    for _ in range(max_new_tokens):
        T = idx.size(1)
        if cache is None or T > bs:
            idx_cond = idx if T <= bs else idx[:, -bs:]
            cache = _state_for(model, slot, idx_cond, bs) if idx.is_cuda else _CpuCache(model, idx_cond, kv8)
            cache.pos = idx_cond.size(1)
            logits = cache.logits
        logits = edit(logits, idx[:, max(0, T - bs):])
        idx_next = pick(logits, T)
        if return_logprobs:
            lps.append(R.token_logprob(logits, idx_next))
        idx = torch.cat((idx, idx_next), dim=1)
        if idx.size(1) > bs:
            cache = None  # window slides: rebuild from the cropped context next step
            continue
        logits = cache.step(idx_next, cache.pos)
        cache.pos += 1
    return done(idx)


def _generate_windowed_gpu(model, idx, max_new_tokens, first, loop, logprobs=False, proc=None,
                           slot="_mg_decode_cache"):
    """Greedy or seeded decode on the GPU: one prefill per context window, whose logits give the
    window's first token ``first(cache, T, ctx)`` [B], then the device-side token loop ``loop(cache,
    tok, L, n, T, ctx)`` [B, n] (``_GpuCache.greedy`` / ``.sample``: n steps from token ``tok`` at
    position ``L``) for every position the window still has room for.  ``T`` is the column of the
    call's first token in the returned sequence, ``ctx`` the window's context.  ``proc``
    (``_proc_words``): the prefill logits are edited by the logits processors over ``ctx`` before
    the first pick (``process_prefill``).  Once the sequence outgrows block_size, each token
    is a fresh prefill of the last block_size tokens -- the reference's crop-every-step semantics
    (``/root/reference/mingpt/model.py:333``).  ``logprobs``: the first token gets its
    log-probability from the prefill logits (``with_logprob``), ``loop`` returns a (tokens,
    log-probabilities) pair, and so does this.  ``slot``: the decode state's (``_kv_slot``)."""
    bs = model.block_size
    B, T0 = idx.shape
    out = torch.empty(B, T0 + max_new_tokens, dtype=torch.long, device=idx.device)
    out[:, :T0] = idx
    outs = (out, torch.zeros(out.shape, dtype=torch.float32, device=idx.device)) if logprobs else (out,)

    def put(cols, vals):  # tokens, or with logprobs the (tokens, lp) pair, into columns ``cols``
        for dst, v in zip(outs, vals if logprobs else (vals,)):
            dst[:, cols] = v

    T, end = T0, T0 + max_new_tokens
    while T < end:
        ctx = out[:, max(0, T - bs):T]
        L = ctx.size(1)
        cache = _state_for(model, slot, ctx, bs)
        if proc is not None:
            cache.process_prefill(ctx, proc)
        tok = first(cache, T, ctx)
        put(T, cache.with_logprob(tok) if logprobs else tok)
        T += 1
        n = min(end - T, bs - L)
        if n > 0:
            put(slice(T, T + n), loop(cache, out[:, T - 1:T], L, n, T, ctx))
            T += n
    return outs if logprobs else out


# --------------------------------------------------------------------------- ragged batches
_EARLY_EXIT = True  # set False to replay every step even after every row has stopped
_EXIT_EVERY = 16    # replays between two reads of the finished flags


def _ragged_prompts(prompts, who="generate_batch"):
    """(rows, device): the unpadded int64 prompts of either input form, on the first one's device."""
    if isinstance(prompts, tuple) and len(prompts) == 2 and torch.is_tensor(prompts[0]) and prompts[0].dim() == 2:
        idx, lengths = prompts
        lengths = torch.as_tensor(lengths).to("cpu", torch.long).view(-1)
        if lengths.numel() != idx.size(0):
            raise ValueError(f"{who}: {idx.size(0)} rows, {lengths.numel()} lengths")
        if lengths.numel() and (int(lengths.min()) < 1 or int(lengths.max()) > idx.size(1)):
            raise ValueError(f"{who}: every length must be in 1..{idx.size(1)}, got {lengths.tolist()}")
        rows = [idx[b, :int(n)] for b, n in enumerate(lengths.tolist())]
    else:
        rows = [torch.as_tensor(p) for p in prompts]
        if any(r.dim() != 1 or r.numel() < 1 for r in rows):
            raise ValueError(f"{who}: every prompt must be a 1-D tensor of 1 or more tokens")
    if not rows:
        raise ValueError(f"{who}: no prompts")
    device = rows[0].device
    return [r.to(device=device, dtype=torch.long) for r in rows], device


def _check_token_ids(who, V, tokens, pad_token=None, eos_token=None, what="prompt token"):
    """ValueError unless ``pad_token`` and ``eos_token`` (None: not given) and every entry of
    ``tokens`` are token ids, 0 <= id < V."""
    if pad_token is not None and not 0 <= int(pad_token) < V:
        raise ValueError(f"{who}: pad_token {pad_token} is not a token id (vocab {V})")
    if eos_token is not None and not 0 <= int(eos_token) < V:
        raise ValueError(f"{who}: eos_token {eos_token} is not a token id (vocab {V})")
    lo, hi = tokens.aminmax()
    if int(lo) < 0 or int(hi) >= V:
        raise ValueError(f"{who}: {what} outside [0, {V})")


@torch.no_grad()
def generate_batch(model, prompts, max_new_tokens: int, temperature: float = 1.0, do_sample: bool = False,
                   top_k: Optional[int] = None, seed: Optional[int] = None, eos_token: Optional[int] = None,
                   pad_token: int = 0, top_p: Optional[float] = None, return_logprobs: bool = False,
                   repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                   no_repeat_ngram_size: int = 0, kv_cache: str = "bf16"):
    """Decode a batch of prompts of different lengths in one go; returns ``(tokens, lengths)``, or
    with ``return_logprobs`` ``(tokens, lengths, logprobs)``: float32 of ``tokens``' shape, entry
    [b, j] the model's log-probability of ``tokens[b, j]`` given ``tokens[b, :j]`` at every generated
    position (the stop token included) and 0.0 at prompt and padding positions -- the number
    ``generate(return_logprobs=True)`` gives for the row alone.

    ``prompts``: a sequence of 1-D int64 tensors (1 or more tokens each), or a pair ``(idx [B, Tp]
    right-padded, lengths [B])`` -- positions at or past a row's length are ignored, whatever they
    hold.  ``tokens`` is int64 [B, max(len) + max_new_tokens]: row b holds its prompt, its generated
    tokens directly after it (``eos_token``, if produced, is the row's last token) and ``pad_token``
    in the rest; ``lengths`` int64 [B] counts the valid tokens per row, prompt included.

    Every row is the single-prompt algorithm applied to that row alone: greedy takes the argmax of
    the row's last-position logits (first index on ties); sampling is the seeded Gumbel-max rule of
    ``generate(seed=...)`` with the draw counter = the column of the produced token in the row's
    own unpadded sequence and the batch row index b (``do_sample`` without a seed draws one seed
    from torch's global generator first), ``top_p`` included.  A row stops after ``eos_token`` or ``max_new_tokens``
    tokens.  There is no sliding window here: ``max(len) + max_new_tokens`` must fit ``block_size``
    (ValueError otherwise).

    ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty``, ``no_repeat_ngram_size``: the
    logits processors of ``generate`` (the rule in common.h), with the row's own unpadded sequence so
    far as its history -- never the padding, never another row.  With any of them on the reported
    log-probabilities are the processed rows'.

    ``kv_cache``: ``"bf16"`` or ``"int8"``, the KV8 model and the int8 cache of ``generate``.

    On the GPU the right-padded batch is prefilled once and the token loop is one captured step
    replayed back to back (``_GpuCache.ragged``): per-row positions and finished flags live in
    device memory.  On the CPU each row runs through the cache path on its own."""
    slot, kv8 = _kv_slot("generate_batch", kv_cache)
    rows, device = _ragged_prompts(prompts)
    V = model.config.vocab_size
    lens = [r.numel() for r in rows]
    B, Lmax = len(rows), max(lens)
    _check_entry("generate_batch", model, max_new_tokens, longest=Lmax)
    _check_token_ids("generate_batch", V, torch.cat(rows), pad_token, eos_token)
    R.check_sample_args(temperature, top_k, top_p)
    proc, pwords = _processors("generate_batch", model, device.type == "cuda", repetition_penalty, presence_penalty,
                               frequency_penalty, no_repeat_ngram_size)
    if do_sample and seed is None:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
    seed = int(seed or 0) & ((1 << 64) - 1)
    before_use(*model.parameters())
    lengths = torch.tensor(lens, dtype=torch.long, device=device)
    tokens = torch.full((B, Lmax + max_new_tokens), int(pad_token), dtype=torch.long, device=device)
    for b, r in enumerate(rows):
        tokens[b, :lens[b]] = r
    logprobs = torch.zeros(tokens.shape, dtype=torch.float32, device=device) if return_logprobs else None
    if max_new_tokens == 0:
        return (tokens, lengths, logprobs) if return_logprobs else (tokens, lengths)
    if device.type == "cuda":
        return _generate_batch_gpu(model, tokens[:, :Lmax].contiguous(), lengths, max_new_tokens, temperature,
                                   do_sample, top_k, seed, eos_token, int(pad_token), top_p, return_logprobs, pwords,
                                   slot)
    for b, r in enumerate(rows):  # the executable definition of the semantics
        cache = _CpuCache(model, r.view(1, -1), kv8)
        logits, n = cache.logits, lens[b]
        for _ in range(max_new_tokens):
            if proc is not None:  # the history is the row's own sequence so far
                logits = R.process_logits(logits, tokens[b:b + 1, :n], *proc)
            if do_sample:
                nxt = R.sample_gumbel(logits, temperature, top_k, seed, n, row0=b, top_p=top_p)
            else:
                nxt = logits.argmax(dim=-1, keepdim=True)
            tokens[b, n] = nxt.view(())
            if return_logprobs:
                logprobs[b, n] = R.token_logprob(logits, nxt).view(())
            n += 1
            if eos_token is not None and int(nxt) == int(eos_token):
                break
            if n < lens[b] + max_new_tokens:
                logits = cache.step(nxt, n - 1)
        lengths[b] = n
    return (tokens, lengths, logprobs) if return_logprobs else (tokens, lengths)


def _generate_batch_gpu(model, idx, lengths, max_new_tokens, temperature, do_sample, top_k, seed, eos_token,
                        pad_token, top_p=None, logprobs=False, proc=None, slot="_mg_decode_cache"):
    """The GPU half of ``generate_batch``: prefill the right-padded batch ``idx`` [B, Lmax] once --
    causal attention makes every position before a row's length exact -- take row b's logits at
    column lengths[b] - 1, pick the first token with the loop's own pick kernel, then replay the
    ragged step max_new_tokens - 1 times.  With a stop token the finished flags are read every
    ``_EXIT_EVERY`` replays; stopping early changes nothing, since a step leaves finished rows as
    they are.  ``logprobs``: the loops with the lse kernel, and the state's ``lp`` buffer (zero but
    at the generated positions) as a third result.  ``proc`` (``_proc_words``): the loops with the
    process kernel in front of the pick, the first pick included.  ``slot``: the decode state's."""
    B, Lmax = idx.shape
    cache = _state_for(model, slot, idx, model.block_size, last=lengths - 1)
    words = _ragged_words(seed, temperature, top_k, eos_token, top_p)
    greedy = not do_sample
    st = cache.ragged_start(idx, lengths, words, greedy, logprobs=logprobs, proc=proc)
    _replay(lambda k: cache.ragged(k, words, greedy, logprobs=logprobs, proc=proc), max_new_tokens - 1, st["done"],
            eos_token)
    out_len = st["pos"].long() + 1
    W = Lmax + max_new_tokens
    cols = torch.arange(W, device=idx.device).view(1, W)
    tokens = torch.where(cols < out_len.view(B, 1), st["seq"][:, :W], torch.full_like(cols, pad_token))
    if logprobs:
        return tokens, out_len, st["lp"][:, :W].clone()
    return tokens, out_len


# --------------------------------------------------------------------------- beam search
_BEAM_MAX = 8                     # beams per prompt the kernels take (kernels.h kBeamMax)
_BEAM_REORDER_PER_LAYER = False   # set True (before a state's first beam call) to launch the cache
#                                   reorder once per layer instead of once over all layers (PERF.md)


def _beam_backtrack(hparent, htok, pad_token, total):
    """The beams' generated tokens [B, W, total] from the per-step histories ``hparent`` / ``htok``
    [B, W, steps] (host tensors; column j: new beam r of step j came from old beam hparent[b, r, j]
    with token htok[b, r, j]), walked backwards from the last step's order.  Columns from ``steps``
    on -- every beam had finished and the loop stopped -- are ``pad_token``: more steps would have
    kept the order and offered only that."""
    B, W, steps = htok.shape
    out = torch.full((B, W, total), int(pad_token), dtype=torch.long)
    cur = torch.arange(W).expand(B, W)
    for j in range(steps - 1, -1, -1):
        out[:, :, j] = htok[:, :, j].long().gather(1, cur)
        cur = hparent[:, :, j].long().gather(1, cur)
    return out


@torch.no_grad()
def generate_beam(model, idx, max_new_tokens: int, num_beams: int, eos_token: Optional[int] = None,
                  pad_token: int = 0, length_penalty: float = 0.0, kv_cache: str = "bf16"):
    """Beam search over the model's log-probabilities (the rule in common.h, 'Beam search'): keep
    the ``num_beams`` continuations of every prompt with the largest summed log-probability, step
    by step.  Returns ``(tokens, lengths, scores)``, best beam first per prompt: ``tokens`` int64
    [B, W, T + max_new_tokens] -- the prompt, the beam's tokens (``eos_token``, if produced, is the
    beam's last) and ``pad_token`` in the rest; ``lengths`` int64 [B, W] counts the valid tokens,
    prompt included; ``scores`` float32 [B, W] is the beam's summed log-probability (the numbers of
    ``generate(return_logprobs=True)``, added in fp32 on the device).

    ``idx``: int64 [B, T], rectangular.  ``1 <= num_beams <= 8`` and at most the vocabulary size;
    ``T + max_new_tokens`` must fit ``block_size`` (no sliding window here); ValueError otherwise.
    A beam that produced ``eos_token`` is finished: it keeps its score, competes with the live
    beams' continuations for its place and is padded.  ``length_penalty = a`` re-ranks the final W
    beams by ``score / max(n_generated, 1) ** a`` (a stable sort: ties keep the search's order);
    ``scores`` stays the raw sum, and a = 0 returns the search's order untouched.

    On the GPU the prompt is prefilled once per prompt and the whole step -- decode, the row
    kernel, the merge, the in-place reorder of every layer's KV cache by parent beam -- is one
    captured graph replayed back to back on B * W rows (``_GpuCache.beam``); the sequences are
    rebuilt at the end from the per-step parent / token histories.  On the CPU the same loop runs
    ``ops.reference.beam_step`` on ``_CpuCache``.

    ``kv_cache``: ``"bf16"`` (default) or ``"int8"``, the KV8 model of ``generate`` (every K and V vector
    snapped to int8 times a power-of-two scale before any attention reads it).  On the GPU its B * W
    rows live in int8 caches -- (2 D + 8 H) / (6 D) of the bf16 beam state's bytes -- in a state of
    its own (``_mg_beam_kv8_cache``): the prompt is snapped once and stored to its W beams
    (``kv8_store(rep=W)``), the step attends with ``attention_decode_kv8`` and ends with
    ``beam_reorder_kv8``.  ValueError for any other string."""
    who = "generate_beam"
    slot, kv8 = _kv_slot(who, kv_cache, "_mg_beam_cache")
    n = _check_entry(who, model, max_new_tokens, idx)
    V, W = model.config.vocab_size, int(num_beams)
    B, T = idx.shape
    if not 1 <= W <= _BEAM_MAX:
        raise ValueError(f"{who}: num_beams must be in 1..{_BEAM_MAX}, got {num_beams}")
    if W > V:
        raise ValueError(f"{who}: num_beams ({W}) exceeds the vocabulary size ({V})")
    _check_token_ids(who, V, idx, pad_token, eos_token)
    a = float(length_penalty)
    device = idx.device
    before_use(*model.parameters())
    tokens = torch.full((B, W, T + n), int(pad_token), dtype=torch.long, device=device)
    tokens[:, :, :T] = idx.view(B, 1, T)
    lengths = torch.full((B, W), T, dtype=torch.long, device=device)
    scores = torch.zeros((B, W), dtype=torch.float32, device=device)
    if n == 0:
        return tokens, lengths, scores
    if device.type == "cuda":
        hparent, htok, lengths, scores = _generate_beam_gpu(model, idx.contiguous(), n, W, eos_token, int(pad_token),
                                                             slot)
    else:
        hparent, htok, lengths, scores = _generate_beam_cpu(model, idx, n, W, eos_token, int(pad_token), kv8)
    tokens[:, :, T:] = _beam_backtrack(hparent, htok, pad_token, n).to(device)
    if a != 0.0:
        key = scores.double() / (lengths - T).clamp(min=1).double() ** a
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        tokens = tokens.gather(1, order.view(B, W, 1).expand(B, W, T + n))
        lengths, scores = lengths.gather(1, order), scores.gather(1, order)
    return tokens, lengths, scores


def _generate_beam_cpu(model, idx, n, W, eos_token, pad_token, kv8=False):
    """The CPU half of ``generate_beam``, the executable definition of the semantics: one
    ``_CpuCache`` of B * W rows (the prompt prefilled once per prompt and broadcast), a step of
    ``ops.reference.beam_step`` per token, the caches' rows re-gathered by parent beam.  Returns the
    histories (``_beam_backtrack``), the lengths and the scores.  ``kv8``: the KV8 model."""
    B, T = idx.shape
    V = model.config.vocab_size
    cache = _CpuCache(model, idx, kv8)
    cache.k = [k.repeat_interleave(W, dim=0) for k in cache.k]
    cache.v = [v.repeat_interleave(W, dim=0) for v in cache.v]
    logits = cache.logits.repeat_interleave(W, dim=0)
    s = torch.full((B, W), float("-inf"), dtype=torch.float64)
    s[:, 0] = 0.0
    fin = torch.zeros((B, W), dtype=torch.bool)
    lens = torch.full((B, W), T, dtype=torch.long)
    base = torch.arange(B).view(B, 1) * W
    hparent, htok = [], []
    for j in range(n):
        par, tok, s, done = R.beam_step(s, fin, logits.view(B, W, V), eos_token, pad_token)
        lens = lens.gather(1, par) + (~fin.gather(1, par)).long()
        fin = done
        hparent.append(par)
        htok.append(tok)
        if j + 1 == n or bool(fin.all()):
            break
        rows = (base + par).view(-1)
        cache.k = [k.index_select(0, rows) for k in cache.k]
        cache.v = [v.index_select(0, rows) for v in cache.v]
        logits = cache.step(tok.view(B * W, 1), T + j)
    return torch.stack(hparent, dim=2), torch.stack(htok, dim=2), lens, s.float()


def _generate_beam_gpu(model, idx, n, W, eos_token, pad_token, slot="_mg_beam_cache"):
    """The GPU half of ``generate_beam``: build (once) the beam loop of the B * W-row state, prefill
    the B prompts, take the first beam step on the prefill's logits, then replay the captured step
    n - 1 times.  With a stop token the finished flags are read every ``_EXIT_EVERY`` replays and
    the loop ends once every beam has finished -- further steps would keep the order and append
    padding (``_beam_backtrack``), so stopping changes no result.  Returns the host histories of
    the steps taken, the lengths [B, W] and the scores [B, W].  ``slot``: the beam state's (``_kv_slot``)."""
    B, T = idx.shape
    cache = _state_for(model, slot, idx, model.block_size, rows=B * W)
    loop = cache.beam(W)  # before the prefill: building it runs a warm-up step
    st = cache.beam_start(W, T, cache.beam_prefill(idx, W), eos_token, pad_token)
    steps = 1 + _replay(loop.run, n - 1, st["fin"], eos_token)
    hparent, htok = st["hparent"][:, :, T:T + steps].cpu(), st["htok"][:, :, T:T + steps].cpu()
    return hparent, htok, st["len"].view(B, W).long(), st["score"].view(B, W).clone()


# --------------------------------------------------------------------------- speculative decoding
_SPEC_ROWS_MAX = 8   # rows of one verify step over the whole batch (the skinny GEMM's, kernels.h kSpecRowsMax)
_SPEC_NGRAM_MAX = 4  # kernels.h kSpecNgramMax


@torch.no_grad()
def generate_speculative(model, idx, max_new_tokens: int, draft_len: int = 3, ngram: int = 3,
                         return_stats: bool = False, kv_cache: str = "bf16"):
    """Greedy decoding, several tokens per step (the rule in common.h, 'Speculative greedy
    decoding'): every step guesses the next ``draft_len`` tokens of a sequence by prompt lookup --
    the continuation of the most recent earlier occurrence of its last up to ``ngram`` tokens -- runs
    the last committed token and the guesses as K = ``draft_len + 1`` rows at K consecutive
    positions of the same KV cache, and keeps the longest prefix of guesses that the model's own
    argmax confirms, plus the model's next token: 1 to K tokens per step.  The result is
    ``generate(model, idx, max_new_tokens)``'s greedy output: tokens int64 [B, T + max_new_tokens]
    (on the GPU bit for bit, every row of a step being computed from that row's inputs alone).

    Greedy only: no sampling, no log-probabilities and no stop token on this entry.  ``idx``: int64
    [B, T], rectangular.  ``1 <= draft_len <= 7`` with ``B * (draft_len + 1) <= 8`` (the rows of a step
    go through the skinny GEMM together), ``1 <= ngram <= 4``, and ``T + max_new_tokens`` must fit
    ``block_size`` (no sliding window here); ValueError otherwise.  On the GPU the model's widest
    projection input, ``4 * n_embed``, must fit the skinny GEMM's 8192 columns (every preset up to
    gpt2-xl); RuntimeError otherwise.

    ``return_stats``: also a dict with ``steps`` (int64 [B]: the verify steps in which the sequence
    was live) and ``emitted_hist`` (int64 [B, K + 1]: entry e counts the steps that emitted e
    tokens).  The first token comes from the prefill, so a row's histogram adds up to
    ``max_new_tokens - 1`` tokens.

    On the GPU the step -- draft kernel, embedding, blocks with the grouped decode attention, LM head,
    row argmax, accept kernel -- is one captured graph per (B, K) replayed back to back
    (``_GpuCache.spec``); the host reads the positions back once per round of replays.  On the CPU
    the same rule runs through ``ops.reference.ngram_draft`` / ``spec_accept`` and one model forward
    over the extended sequence per step.

    ``kv_cache``: ``"bf16"`` (default) or ``"int8"``, the KV8 model of ``generate``: the result is then
    ``generate(model, idx, max_new_tokens, kv_cache="int8")``'s.  On the GPU the verify rows attend with
    the grouped ``attention_decode_kv8`` on int8 caches, in a state of its own
    (``_mg_spec_kv8_cache``).  ValueError for any other string."""
    who = "generate_speculative"
    slot, kv8 = _kv_slot(who, kv_cache, "_mg_spec_cache")
    n = _check_entry(who, model, max_new_tokens, idx)
    B = idx.size(0)
    if int(draft_len) != draft_len or not 1 <= int(draft_len) <= _SPEC_ROWS_MAX - 1:
        raise ValueError(f"{who}: draft_len must be in 1..{_SPEC_ROWS_MAX - 1}, got {draft_len}")
    K = int(draft_len) + 1
    if B * K > _SPEC_ROWS_MAX:
        raise ValueError(f"{who}: draft_len {draft_len} at batch {B} needs {B * K} rows per step; a step takes "
                         f"at most {_SPEC_ROWS_MAX}")
    if int(ngram) != ngram or not 1 <= int(ngram) <= _SPEC_NGRAM_MAX:
        raise ValueError(f"{who}: ngram must be in 1..{_SPEC_NGRAM_MAX}, got {ngram}")
    _check_token_ids(who, model.config.vocab_size, idx)
    before_use(*model.parameters())
    if n == 0:
        out = idx.clone()
        steps = torch.zeros(B, dtype=torch.long, device=idx.device)
        hist = torch.zeros(B, K + 1, dtype=torch.long, device=idx.device)
    elif idx.is_cuda:
        out, steps, hist = _generate_speculative_gpu(model, idx.contiguous(), n, K, int(ngram), slot)
    else:
        out, steps, hist = _generate_speculative_cpu(model, idx, n, K, int(ngram), kv8)
    return (out, {"steps": steps, "emitted_hist": hist}) if return_stats else out


def _generate_speculative_cpu(model, idx, n, K, ngram, kv8=False):
    """The CPU half of ``generate_speculative``, the executable definition of the semantics: per
    sequence and step, ``ops.reference.ngram_draft``, one model forward over the committed tokens
    extended by the draft (only the min(K, end - p) rows that can still be emitted), the argmax of
    the rows' logits and ``ops.reference.spec_accept``.  Eval mode, as for ``score``.  ``kv8``: the
    forward is the KV8 model's (``_CpuCache`` with every position's logits)."""
    B, T = idx.shape
    out = torch.zeros(B, T + n, dtype=torch.long, device=idx.device)
    out[:, :T] = idx
    steps = torch.zeros(B, dtype=torch.long, device=idx.device)
    hist = torch.zeros(B, K + 1, dtype=torch.long, device=idx.device)
    end = T + n - 1
    forward = (lambda x: (_CpuCache(model, x, True, every=True).logits, None)) if kv8 else model
    was = model.training
    model.eval()
    try:
        for b in range(B):
            logits, _ = forward(idx[b:b + 1])
            out[b, T] = logits[0, -1].argmax()
            p = T
            while p < end:
                rows, has = R.ngram_draft(out[b], p, K, ngram)
                rows = rows[:min(K, end - p)]
                x = torch.cat([out[b, :p], torch.tensor(rows, dtype=torch.long, device=idx.device)])
                logits, _ = forward(x.view(1, -1))
                g = logits[0, p:].argmax(dim=-1)
                _, cnt = R.spec_accept(rows, g.tolist(), has, p, end)
                out[b, p + 1:p + 1 + cnt] = g[:cnt]
                p += cnt
                steps[b] += 1
                hist[b, cnt] += 1
    finally:
        model.train(was)
    return out, steps, hist


def _generate_speculative_gpu(model, idx, n, K, ngram, slot="_mg_spec_cache"):
    """The GPU half of ``generate_speculative``: build (once per (B, K)) the speculative loop, prefill
    the prompts and take the first token from the prefill logits as ``generate`` does, then replay
    the captured step in rounds of ceil((end - min p) / K) -- the fewest steps that could finish --
    reading the positions back after each round, until every sequence has reached ``end``.  ``slot``:
    the speculative state's (``_kv_slot``)."""
    B, T = idx.shape
    cache = _state_for(model, slot, idx, model.block_size, rows=B)
    loop = cache.spec(K)  # before the prefill: building it runs a warm-up step
    cache.prefill(idx)
    st = cache.spec_start(K, idx, cache.logits.argmax(-1), n, ngram)
    end, low = T + n - 1, T
    while low < end:
        loop.run(-(-(end - low) // K))
        low = int(st["pos"].min())
    return st["seq"][:, :T + n].clone(), st["steps"].long(), st["hist"].long()


# --------------------------------------------------------------------------- scoring
_SCORE_LOGITS_BYTES = 256 << 20  # cap on the transient bf16 logits of one LM-head chunk in score()


@torch.no_grad()
def score(model, idx, lengths=None, kv_cache: str = "bf16"):
    """Log-probabilities of given sequences: float32 [B, T], ``out[b, j]`` = the model's
    log-probability of ``idx[b, j]`` given ``idx[b, :j]`` (the rule in common.h: log-softmax at
    temperature 1) for 1 <= j < lengths[b], and 0.0 elsewhere, column 0 included.  A row's sum is
    its log-likelihood given its first token.

    ``idx``: a sequence of 1-D int64 tensors, or a right-padded [B, T] tensor with ``lengths`` [B]
    (None: every row is full) -- the input forms of ``generate_batch``; a pair ``(idx, lengths)`` is
    accepted too.  T must fit ``block_size`` and every token be in [0, V) (ValueError).  Runs in
    eval mode (no dropout) whatever ``model.training`` says, and leaves that flag as it was.

    GPU: one forward of the blocks on the MFMA path (the prefill's body), then the LM head in row
    chunks whose transient bf16 logits stay under ``_SCORE_LOGITS_BYTES`` (256 MiB; at least one
    row), each through the lse kernel with the next tokens as targets (``logits_lse``) -- the
    [B, T, V] logits never exist at once and nothing is read back in fp32.  CPU: the model's
    forward and ``ops.reference.token_logprob``.

    ``kv_cache``: ``"bf16"`` (default) or ``"int8"``: the log-probabilities the KV8 model of
    ``generate(kv_cache="int8")`` assigns -- every K and V vector snapped before any attention reads
    it (GPU: ``kv8_store`` in place on every layer's qkv rows of the prefill body, no cache kept; CPU:
    ``_CpuCache`` with every position's logits).  ValueError for any other string."""
    _, kv8 = _kv_slot("score", kv_cache)
    if isinstance(idx, tuple) and lengths is None:
        prompts = idx
    elif torch.is_tensor(idx) and idx.dim() == 2:
        prompts = (idx, torch.full((idx.size(0),), idx.size(1)) if lengths is None else lengths)
    elif lengths is not None:
        raise ValueError("score: lengths go with a 2-D idx")
    else:
        prompts = idx
    rows, device = _ragged_prompts(prompts, "score")
    V, bs = model.config.vocab_size, model.block_size
    lens = [r.numel() for r in rows]
    B = len(rows)
    T = prompts[0].size(1) if isinstance(prompts, tuple) else max(lens)
    if T > bs:
        raise ValueError(f"score: sequence length {T} exceeds block_size ({bs})")
    tokens = torch.zeros((B, T), dtype=torch.long, device=device)
    for b, r in enumerate(rows):
        tokens[b, :lens[b]] = r
    _check_token_ids("score", V, tokens, what="token")  # the padding is 0, a valid id
    before_use(*model.parameters())
    out = torch.zeros((B, T), dtype=torch.float32, device=device)
    if T == 1:
        return out
    cols = torch.arange(1, T, device=device).view(1, T - 1)
    valid = cols < torch.tensor(lens, device=device).view(B, 1)  # [B, T - 1]: column j has a target
    if device.type != "cuda":
        was = model.training
        model.eval()
        try:
            logits = _CpuCache(model, tokens, True, every=True).logits if kv8 else model(tokens)[0]
        finally:
            model.train(was)
        lp = R.token_logprob(logits[:, :-1], tokens[:, 1:])
        out[:, 1:] = torch.where(valid, lp, torch.zeros_like(lp))
        return out
    c = _Body(model)
    H = model.config.n_head
    keep = (lambda i, qkv: c.C.kv8_store(qkv, H)) if kv8 else None  # the KV8 model: snapped in place, no cache
    x = c._prompt(tokens, keep).view(B * T, model.config.n_embed)
    targets = torch.full((B, T), -1, dtype=torch.long, device=device)  # row (b, t) predicts column t + 1
    targets[:, :-1] = torch.where(valid, tokens[:, 1:], targets[:, 1:])
    targets = targets.view(B * T)
    lp = torch.zeros(B * T, dtype=torch.float32, device=device)
    step = max(1, _SCORE_LOGITS_BYTES // (2 * ((V + 7) // 8 * 8)))
    for r0 in range(0, B * T, step):
        r1 = min(B * T, r0 + step)
        c.C.logits_lse(c._head(x[r0:r1], "mfma"), V, targets[r0:r1], None, lp[r0:r1])
    out[:, 1:] = lp.view(B, T)[:, :-1]
    return out
