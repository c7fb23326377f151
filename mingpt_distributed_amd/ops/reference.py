"""Plain-PyTorch implementations of every fused op.

These serve two roles only: the CPU execution path (BASELINE config #1, gpt-nano on
SortDataset, and the multi-process ``gloo`` tests) and the fp32 numerics oracle that the
HIP kernels are tested against.  On a GPU tensor the framework never calls these (see
``ops/__init__.py``): the HIP kernels in ``csrc/kernels`` run instead.

Semantics are the *intended* ones of the reference (``/root/reference/mingpt/model.py``):
causal attention with a -inf mask (fixes D4), GELU between c_fc and c_proj (fixes D5),
tanh-approximate GELU (upstream ``NewGELU``, so OpenAI GPT-2 weights reproduce), and
cross-entropy with ``ignore_index=-1`` (``model.py:316-318``).
"""
from __future__ import annotations

import math
import numbers

import torch
import torch.nn.functional as F

GELU_K0 = math.sqrt(2.0 / math.pi)
GELU_K1 = 0.044715


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.tanh(GELU_K0 * (x + GELU_K1 * x * x * x)))


def embedding(idx, wte, wpe, p: float, training: bool):
    B, T = idx.shape
    x = wte[idx] + wpe[:T].unsqueeze(0)
    return F.dropout(x, p, training)


def layer_norm(x, w, b, eps: float = 1e-5):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def linear(x, w, b=None):
    return F.linear(x, w, b)


def causal_attention(q, k, v, p: float, training: bool):
    """q, k, v: [B, H, T, hd] -> [B, H, T, hd]. Explicit masked softmax (upstream minGPT)."""
    T = q.size(-2)
    att = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(k.size(-1)))
    mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
    att = att.masked_fill(~mask, float("-inf"))
    att = F.softmax(att, dim=-1)
    att = F.dropout(att, p, training)
    return att @ v


def self_attention(x, w_attn, b_attn, w_proj, b_proj, n_head: int, attn_p: float, resid_p: float,
                   training: bool):
    B, T, C = x.shape
    q, k, v = linear(x, w_attn, b_attn).split(C, dim=2)
    q = q.view(B, T, n_head, C // n_head).transpose(1, 2)
    k = k.view(B, T, n_head, C // n_head).transpose(1, 2)
    v = v.view(B, T, n_head, C // n_head).transpose(1, 2)
    y = causal_attention(q, k, v, attn_p, training)
    y = y.transpose(1, 2).contiguous().view(B, T, C)
    return F.dropout(linear(y, w_proj, b_proj), resid_p, training)


def mlp(x, w_fc, b_fc, w_proj, b_proj, resid_p: float, training: bool):
    return F.dropout(linear(gelu_tanh(linear(x, w_fc, b_fc)), w_proj, b_proj), resid_p, training)


SAMPLE_SALT = 0x5A3B1E97  # csrc/include/common.h kSampleSalt
_M32 = 0xFFFFFFFF


def _fmix32(h: torch.Tensor) -> torch.Tensor:
    """murmur3 finaliser on uint32 values held in int64 (a wrapped int64 product keeps its low 32 bits)."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def check_sample_args(temperature: float, top_k, top_p=None) -> None:
    if not temperature > 0:
        raise ValueError(f"sampling needs temperature > 0, got {temperature}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"sampling needs top_k >= 1 (or None), got {top_k}")
    if top_p is not None and not 0 < float(top_p) <= 1:  # NaN fails both comparisons
        raise ValueError(f"sampling needs 0 < top_p <= 1 (or None), got {top_p}")


PROC_NGRAM_MAX = 8  # kernels.h kProcNgramMax


def check_process_args(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                       no_repeat_ngram_size=0) -> bool:
    """ValueError unless the logits processors' arguments are valid (common.h, 'Logits processors');
    returns whether any processor is on (an argument differs from its off value)."""
    fin = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)
    if not (fin(repetition_penalty) and repetition_penalty > 0):
        raise ValueError(f"repetition_penalty must be finite and > 0 (1.0: off), got {repetition_penalty}")
    if not fin(presence_penalty):
        raise ValueError(f"presence_penalty must be finite (0.0: off), got {presence_penalty}")
    if not fin(frequency_penalty):
        raise ValueError(f"frequency_penalty must be finite (0.0: off), got {frequency_penalty}")
    g = no_repeat_ngram_size
    if isinstance(g, bool) or not isinstance(g, numbers.Integral) or not 0 <= g <= PROC_NGRAM_MAX:
        raise ValueError(f"no_repeat_ngram_size must be an integer in 0..{PROC_NGRAM_MAX} (0: off), got {g}")
    return repetition_penalty != 1.0 or presence_penalty != 0.0 or frequency_penalty != 0.0 or g != 0


def process_values(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """(rp, inv, pp, fp) of the rule as Python floats holding float32 values: the arguments rounded
    to float32 and inv = float32(1.0 / repetition_penalty), computed as ``sample_inv_t`` does."""
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32).item())
    return (f32(repetition_penalty), sample_inv_t(repetition_penalty), f32(presence_penalty),
            f32(frequency_penalty))


def process_logits(logits: torch.Tensor, hist: torch.Tensor, repetition_penalty=1.0, presence_penalty=0.0,
                   frequency_penalty=0.0, no_repeat_ngram_size=0) -> torch.Tensor:
    """The logits processors of ``csrc/include/common.h`` ('Logits processors'; the kernel is
    ``csrc/kernels/process.hip``) in torch: rows ``logits`` [B, V] (any floating dtype) edited from the
    histories ``hist`` [B, n] (int64, n >= 1) -- the penalties as single float32 operations rounded to
    the logits' dtype, then the no-repeat n-gram ban.  Returns a new tensor of ``logits``' dtype."""
    check_process_args(repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram_size)
    B, V = logits.shape
    n, dev = hist.size(1), logits.device
    hist = hist.to(dev)
    rp, inv, pp, fp = (torch.tensor(v, dtype=torch.float32, device=dev)
                       for v in process_values(repetition_penalty, presence_penalty, frequency_penalty))
    valid = (hist >= 0) & (hist < V)  # an id outside [0, V) counts for nothing
    safe = torch.where(valid, hist, torch.zeros_like(hist))
    c = torch.zeros(B, V, dtype=torch.long, device=dev).scatter_add_(1, safe, valid.long())
    x = logits.float()
    a = torch.where(x > 0, x * inv, x * rp)
    q = fp * c.float()
    q = q + pp
    y = (a - q).to(logits.dtype)
    out = torch.where((c > 0) & (x != float("-inf")), y, logits)
    g = int(no_repeat_ngram_size)
    if g >= 1 and n >= g:
        ok = torch.ones(B, n - g + 1, dtype=torch.bool, device=dev)  # column i: slot t = g - 1 + i
        for j in range(g - 1):  # h[t - 1 - j] == h[n - 1 - j], both real ids
            a_ = hist[:, g - 2 - j:n - 1 - j]
            ok &= (a_ == hist[:, n - 1 - j:n - j]) & valid[:, g - 2 - j:n - 1 - j]
        ok &= valid[:, g - 1:]
        ban = torch.zeros(B, V, dtype=torch.long, device=dev).scatter_add_(1, safe[:, g - 1:], ok.long())
        out = out.masked_fill(ban > 0, float("-inf"))
    return out


def sample_inv_t(temperature: float) -> float:
    """float32(1 / temperature), the factor both the kernel and this file multiply by."""
    return float(torch.tensor(1.0 / temperature, dtype=torch.float32).item())


def sample_top_p(top_p):
    """float32(top_p), the value the rule uses, or None when the nucleus is off (None or >= 1.0)."""
    if top_p is None:
        return None
    p = float(torch.tensor(float(top_p), dtype=torch.float32).item())
    return p if p < 1.0 else None


def nucleus_keep(x: torch.Tensor, top_p: float) -> torch.Tensor:
    """The nucleus of ``csrc/include/common.h`` on rows of log-weights ``x`` [B, V] (fp64; -inf =
    not in the set top-k kept): True where the mass strictly above the entry's value is below
    ``top_p`` times the row's mass.  Equal values share one answer; the row maximum is always kept."""
    xs, order = torch.sort(x, dim=-1, descending=True)
    w = torch.exp(xs - xs[:, :1])
    w = torch.where(torch.isfinite(xs), w, torch.zeros_like(w))
    cum = torch.cumsum(w, dim=-1)
    # the mass strictly above a value is the exclusive prefix at the first entry of its tie group
    first = torch.ones_like(xs, dtype=torch.bool)
    first[:, 1:] = xs[:, 1:] != xs[:, :-1]
    above = torch.cummax(torch.where(first, cum - w, torch.zeros_like(w)), dim=-1).values
    keep_sorted = (above < top_p * cum[:, -1:]) & torch.isfinite(xs)
    return torch.zeros_like(keep_sorted).scatter_(-1, order, keep_sorted)


def sample_gumbel(logits: torch.Tensor, temperature: float, top_k, seed: int, draw: int, row0: int = 0,
                  top_p=None):
    """One token per row of ``logits`` [B, V] by the Gumbel-max rule of ``csrc/include/common.h``
    ('Gumbel-max sampling'; the kernel is ``csrc/kernels/sample.hip``), in integer ops and fp64 on
    the logits' device.  ``draw`` is the column of the produced token in the returned sequence,
    row b of ``logits`` is batch row ``row0 + b``.  ``top_p``: the nucleus filter of the same rule,
    after the temperature and top-k (None or >= 1.0: off).  Returns [B, 1] int64."""
    check_sample_args(temperature, top_k, top_p)
    B, V = logits.shape
    dev = logits.device
    seed &= (1 << 64) - 1
    s = torch.tensor([(seed & _M32) ^ SAMPLE_SALT], dtype=torch.int64, device=dev)
    r1 = _fmix32((_fmix32(s) + (seed >> 32)) & _M32)
    r2 = _fmix32((r1 + (draw & _M32)) & _M32)
    rows = (torch.arange(B, dtype=torch.int64, device=dev) + row0) & _M32
    r3 = _fmix32(r2 ^ rows).view(B, 1)
    i = torch.arange(V, dtype=torch.int64, device=dev).view(1, V)
    h = _fmix32((r3 + ((i * 0x9E3779B1) & _M32)) & _M32)
    u = ((h >> 8).double() + 0.5) * 2.0 ** -24
    g = -torch.log(-torch.log(u))
    l = logits.double()
    score = (l - l.max(dim=-1, keepdim=True).values) * sample_inv_t(temperature) + g
    if top_k is not None:
        kth = torch.topk(l, min(int(top_k), V), dim=-1).values[:, -1:]
        score = score.masked_fill(l < kth, float("-inf"))
    score = score.masked_fill(l == float("-inf"), float("-inf"))
    p = sample_top_p(top_p)
    if p is not None:
        x = (l - l.max(dim=-1, keepdim=True).values) * sample_inv_t(temperature)
        x = x.masked_fill(score == float("-inf"), float("-inf"))  # outside top-k, or -inf itself
        score = score.masked_fill(~nucleus_keep(x, p), float("-inf"))
    return score.argmax(dim=-1, keepdim=True)


def token_logprob(logits: torch.Tensor, tok: torch.Tensor) -> torch.Tensor:
    """Log-probability of token ``tok[..., r]`` under row r of ``logits`` [..., V]: the rule of
    ``csrc/include/common.h`` ('Per-token log-probabilities') over the reals -- the model's
    log-softmax (temperature 1, before top-k / top-p), in fp64 on the logits as stored (bf16 values
    for a bf16 model), cast to float32.  ``tok``: int64 of the logits' leading shape (a trailing
    dimension of 1 is accepted).  Returns float32 of the leading shape."""
    lead = logits.shape[:-1]
    lp = F.log_softmax(logits.double(), dim=-1)
    return lp.gather(-1, tok.reshape(*lead, 1)).reshape(lead).float()


def beam_step(scores: torch.Tensor, finished: torch.Tensor, logits: torch.Tensor, eos_token=None,
              pad_token: int = 0):
    """One step of the beam-search rule of ``csrc/include/common.h`` ('Beam search'; the kernels are
    ``csrc/kernels/beam.hip``) over the reals, in fp64.  ``scores`` [B, W] (the running sums; -inf
    for a beam that does not exist yet), ``finished`` bool [B, W], ``logits`` [B, W, V] (the row of
    beam w of prompt b), W <= V.  A live beam offers (w, i) with c = s + log_softmax(logits)[i]; a
    finished one only (w, pad_token) with c = s.  The new beams are the W best candidates of the
    prompt: c descending, then the lower w, then the row's own order (logit descending, index
    ascending).  Returns ``(parents, tokens, scores, finished)``: int64, int64, fp64, bool, all
    [B, W], best first."""
    B, W, V = logits.shape
    if W > V:
        raise ValueError(f"beam_step: {W} beams need a vocabulary of at least {W}, got {V}")
    s = scores.double()
    l = logits.double()
    # a row can only contribute its first W entries in its own order (stable: the first index on ties)
    top, tok = torch.sort(l, dim=-1, descending=True, stable=True)
    top, tok = top[..., :W], tok[..., :W]
    lp = top - torch.logsumexp(l, dim=-1, keepdim=True)
    c = s.unsqueeze(-1) + lp  # [B, W, W]: beam w, rank k in its row
    fin = finished.bool().unsqueeze(-1)
    first = torch.arange(W, device=logits.device).view(1, 1, W) == 0
    c = torch.where(fin, torch.where(first, s.unsqueeze(-1), torch.full_like(c, float("-inf"))), c)
    tok = torch.where(fin, torch.full_like(tok, int(pad_token)), tok)
    offered = (~fin | first).reshape(B, W * W)
    c, tok = c.reshape(B, W * W), tok.reshape(B, W * W)
    # stable sorts, the last one the most significant: offered first, then c descending; what is left
    # of the flat (w, k) order breaks the ties
    order = torch.sort(c, dim=-1, descending=True, stable=True).indices
    order = order.gather(-1, torch.sort((~offered).gather(-1, order).long(), dim=-1, stable=True).indices)
    order = order[:, :W]
    parents = order // W
    tokens, new = tok.gather(-1, order), c.gather(-1, order)
    done = finished.bool().gather(-1, parents)
    if eos_token is not None:
        done = done | (tokens == int(eos_token))
    return parents, tokens, new, done


def ngram_draft(s, p: int, K: int, ngram: int):
    """The draft of the speculative rule of ``csrc/include/common.h`` ('Speculative greedy
    decoding'; the kernel is ``csrc/kernels/spec.hip``) for one sequence: ``s`` holds the committed
    tokens ``s[0 .. p]`` (a 1-D tensor or a sequence of ints; entries past ``p`` are ignored).  For
    every e in 0 .. p - 1, ml(e) is the largest m <= ngram with e - j >= 0 and s[e - j] == s[p - j]
    for every j < m; the e with the largest (ml, e) wins -- the longest suffix match, the most recent
    on ties -- and if its ml is 0 there is no draft.  Otherwise x = s[0 .. p] and for r = 1 .. K - 1:
    d_r = x[e + r], appended to x (a period below K drafts through itself).  Returns ``(rows,
    has_draft)``: the K tokens of the step's rows (row 0: s[p]; without a draft every row) at
    positions p .. p + K - 1, and the flag."""
    x = [int(t) for t in (s.tolist() if torch.is_tensor(s) else s)][:p + 1]
    if len(x) != p + 1 or p < 0:
        raise ValueError(f"ngram_draft: s must hold the tokens 0..{p}")
    best = (0, -1)
    for e in range(p):
        ml = 0
        while ml < ngram and e - ml >= 0 and x[e - ml] == x[p - ml]:
            ml += 1
        best = max(best, (ml, e))
    if best[0] == 0:
        return [x[p]] * K, False
    e = best[1]
    for r in range(1, K):
        x.append(x[e + r])
    return x[p:], True


def spec_accept(rows, g, has_draft: bool, p: int, end: int):
    """The accept half of the same rule: ``rows`` the step's input tokens (``ngram_draft``), ``g`` the
    argmax of each row's logits (first index on ties), as many as the step ran.  a is the largest
    value with rows[r] == g[r - 1] for all 1 <= r <= a (0 without a draft); the step emits
    min(a + 1, end - p) tokens g[0], g[1], ... at columns p + 1 ...  Returns ``(a, count)``; count is
    0 for a sequence with p == end, which is left alone."""
    if p >= end:
        return 0, 0
    a = 0
    if has_draft:
        while a + 1 < min(len(rows), len(g)) and int(rows[a + 1]) == int(g[a]):
            a += 1
    return a, min(a + 1, end - p)


def cross_entropy(logits, targets, ignore_index: int = -1):
    return F.cross_entropy(logits.reshape(-1, logits.size(-1)).float(), targets.reshape(-1),
                           ignore_index=ignore_index)
