// Host-side launch API of every gfx950 kernel in csrc/kernels.  Pure HIP: no torch headers,
// raw device pointers + an explicit stream, so the kernels can be driven by the torch binding
// (csrc/bindings.cpp), by native tools, or captured into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mg {
typedef uint16_t bf16_t;

// layernorm.hip
void layernorm_fwd(const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y, float* mean,
                   float* rstd, int M, int D, float eps, hipStream_t stream);
// dz (optional): also dz = residual-dropout backward of the stored dx (probability p, the forward's
// seed), its fp32 column sums added into dzb (the bias gradient of the branch that produced x)
void layernorm_bwd(const bf16_t* dy, const bf16_t* x, const bf16_t* w, const float* mean,
                   const float* rstd, const bf16_t* dres, bf16_t* dx, float* dw, float* db,
                   float* workspace, int M, int D, hipStream_t stream, bf16_t* dz = nullptr,
                   float* dzb = nullptr, float p = 0.f, uint64_t seed = 0);
size_t layernorm_bwd_workspace(int M, int D, bool drop);
// blocks layernorm_bwd launches for M rows: M / 32, at least 1, at most one resident wave of blocks
// of the instantiation (D, drop) selects; each block's waves stride over the rows
int ln_bwd_grid(int M, int D, bool drop);

// embedding.hip
void embedding_fwd(const int64_t* idx, const bf16_t* wte, const bf16_t* wpe, bf16_t* out, int M,
                   int T, int D, int V, float p, uint64_t seed, hipStream_t stream,
                   const int* pos_dev = nullptr,  // pos_dev: decode, position read on the device
                   const unsigned long long* am_part = nullptr,  // greedy decode: the token of row m
                   int am_groups = 0,             //   = argmax over the LM-head GEMV's keys
                   int64_t* tok = nullptr,        //   am_part[m][0 .. am_groups), written to tok[m]
                   int64_t* seq = nullptr,        //   and seq[m * seq_ld + *pos_dev]
                   long seq_ld = 0,
                   int pos_stride = 0,  // 1 (ragged batches): row m takes wpe row pos_dev[m], clamped
                   int pos_rows = 0);   //   to [0, pos_rows); 0: every row takes *pos_dev, as before
unsigned int debug_error_bits();  // MG_DEBUG builds: device range-check bits, cleared on read
void embedding_bwd(const int64_t* idx, const bf16_t* dout, float* dwte, float* dwpe, int M, int T,
                   int D, int V, float p, uint64_t seed, hipStream_t stream);

// xent.hip
void xent_fwd(const bf16_t* logits, const int64_t* targets, float* loss_row, float* lse, float* out,
              int M, int V, int ld, hipStream_t stream);
void xent_bwd(const bf16_t* logits, const int64_t* targets, const float* lse, const float* gscale,
              const float* inv_n, bf16_t* dlogits, int M, int V, int ld, hipStream_t stream);
int xent_fused_nv(int ld);
void xent_fused(const bf16_t* logits, const int64_t* targets, float* loss_row, float* out,
                bf16_t* dlogits, int M, int V, int ld, hipStream_t stream);
void xent_scale(bf16_t* dlogits, const float* gscale, long n, hipStream_t stream);

// adamw.hip (also holds the hipGraph-mode device state; see common.h eff_seed)
void set_graph_state(const uint64_t* seed_ofs, const float* opt_hp);
const uint64_t* graph_seed_ofs();
const float* graph_opt_hp();
size_t grad_norm_workspace();
void grad_sumsq(const float* grad, long n, float grad_scale, float* workspace, float* out,
                hipStream_t stream);
void grad_sumsq_chunks(const int64_t* chunk_start, const int* chunk_len, int n_chunks,
                       const void* grad, bool grad_bf16, float grad_scale, float* workspace,
                       float* out, hipStream_t stream);
void adamw_step(const int64_t* chunk_start, const int* chunk_len, const float* chunk_wd,
                const int64_t* moment_start, int n_chunks, float* master, bf16_t* param,
                const void* grad, bool grad_bf16, float* m, float* v, const float* norm, float lr,
                float b1, float b2, float eps, int step, float grad_scale, float clip,
                hipStream_t stream, float* zero_grad = nullptr);
void f32_to_bf16(const float* src, bf16_t* dst, long n, hipStream_t stream);
// one-GPU stand-in for a ring all-reduce's CU occupancy and duration (comm_proxy.hip)
void comm_proxy(const void* src, void* dst, long n16, long total16, int channels, double gbps,
                hipStream_t stream);

// gemv.hip (decode-time skinny GEMM, B <= 8 rows; epi 0 none, 1 bias, 2 bias+GELU, 3 bias+residual)
// gemv_supported: 1 <= B <= 8, K % 8 == 0, K <= 8192.  K > kGemvSegK (rows staged in two segments)
// only for N <= 8192 outputs and without fused LayerNorm (lnw / lnb null); the caller checks
// (bindings.cpp)
constexpr int kGemvSegK = 4096;  // B x kGemvSegK bf16 of x is the LDS staging buffer (64 KiB at B = 8)
bool gemv_supported(int B, int K);
// greedy-decode epilogue of the LM-head GEMV: each workgroup's best (ordered bf16 logit << 32 |
// ~index) key per row into part[b][workgroup]; workgroup 0 advances *pos.  The argmax over the
// workgroups (first index on ties) is taken by the next step's embedding kernel (embedding_fwd
// with am_part) or on the host after the last step.
struct GemvArgmax {
  unsigned long long* part;  // [B][gemv_grid(N, B)]
  int* pos;                  // device position of the step (+1)
};
int gemv_grid(int N, int B);  // workgroups of gemv() for N outputs at B rows (argmax key groups)
void gemv(const bf16_t* x, const bf16_t* W, bf16_t* y, int B, int N, int K, long ldy, const bf16_t* bias,
          const bf16_t* resid, int epi, hipStream_t stream, const bf16_t* lnw = nullptr,
          const bf16_t* lnb = nullptr, float eps = 1e-5f, const GemvArgmax* am = nullptr);
bool gemv_nt_weights();  // weight loads non-temporal (default) or cached (MINGPT_GEMV_NT=0); gemv.hip
// The same kernel body over int8 weight rows (the W8 rule in common.h): Wq int8 [N, K], 8-byte
// aligned, scale fp32 [N] (powers of two); y = epilogue(scale[n] * chain(x, float(Wq[n, :]))), bit
// for bit gemv's output on the bf16 matrix scale[n] * Wq[n, k].  Same paths, limits, fused
// LayerNorm, epilogues and argmax as gemv.
bool gemv_w8_supported(int B, int K);
void gemv_w8(const bf16_t* x, const int8_t* Wq, const float* scale, bf16_t* y, int B, int N, int K, long ldy,
             const bf16_t* bias, const bf16_t* resid, int epi, hipStream_t stream, const bf16_t* lnw = nullptr,
             const bf16_t* lnb = nullptr, float eps = 1e-5f, const GemvArgmax* am = nullptr);

// gemm_rows.hip (decode-time rows GEMM on MFMA: y[M, ldy] = epi(x[M, K] @ W[N, K]^T); the decode
// loops use it at 9..64 rows).  gemm_rows_supported: 1 <= M <= 64, K % 8 == 0, K <= 8192; any
// N >= 1, ldy >= N.  bf16 in and out, fp32 accumulation, one rounding to bf16 per element; epi as
// gemv's (0 none, 1 bias, 2 bias + GELU, 3 bias + residual; resid [M, ldy]), applied by the function
// gemv applies them with (proj_epilogue, common.h), without dropout.
// Contract: the bits of y[m, :] depend on x[m, :], W, bias, resid[m, :], epi, N
// and K only -- not on M, on which of the 64 slots the row sits in, or on the other rows' contents
// (NaN included); a pure function of the inputs, the same in a captured graph and eagerly.  Nothing
// is read past x + M * K or W + N * K; columns N .. ldy-1 of y are left untouched.
bool gemm_rows_supported(int M, int K);
void gemm_rows(const bf16_t* x, const bf16_t* W, bf16_t* y, int M, int N, int K, long ldy, const bf16_t* bias,
               const bf16_t* resid, int epi, hipStream_t stream);

// sample.hip -- one sampled token per row of bf16 logits [B, ld] (columns >= V never read; ld % 8
// == 0, rows 16-byte aligned): exact top-k + Gumbel-max, the rule in common.h.  params (device,
// 8 x u32): {seed lo, seed hi, draw counter, inv_t as fp32 bits, top_k (<= 0: off), stop token (ragged
// only), top_p as fp32 bits (0 or >= 1.0: off; the nucleus rule in common.h), 0} -- read by the
// kernel, so a captured launch replays with new values; only the draw counter is ever written.  Writes tok[b] (optional) and, with
// seq, seq[b * seq_ld + *pos_dev + 1]; then a trailing one-thread kernel advances params[2] and
// *pos_dev (when given) by one.
constexpr int kSampleParamWords = 8;
// lse, lp (optional, together, with seq): lse = the rows' {m, lnz} from logits_lse on the same logits,
// lp fp32 laid out as seq; lp[b * seq_ld + *pos_dev + 1] = the drawn token's log-probability,
// written exactly where and when the token is written to seq.
void sample_logits(const bf16_t* logits, long ld, int B, int V, uint32_t* params, int* pos_dev, int64_t* tok,
                   int64_t* seq, long seq_ld, hipStream_t stream, const float* lse = nullptr, float* lp = nullptr);
// The kept set of the same rule for the block's top_k / top_p / temperature, by the sampler's own
// kernel with the Gumbel pass replaced: out[2 b] = the bf16 bit pattern of row b's lowest kept
// value (-inf's when nothing is kept), out[2 b + 1] = the number of kept entries.  Writes only out.
void sample_kept(const bf16_t* logits, long ld, int B, int V, const uint32_t* params, int* out, hipStream_t stream);
// Ragged batches: per-row device state pos [B], done [B] (int32), tok [B], seq [B, seq_ld].  One
// kernel, one workgroup per row: a row with done[b] set is left alone; otherwise the token t -- the
// argmax of the row's V logits, first index on ties (greedy), or the Gumbel-max draw with counter
// pos[b] + 1 and batch row b -- is written to tok[b] and seq[b, pos[b] + 1], pos[b] advances by one
// and done[b] is set when t == (int)params[5] (the stop token; negative: none).  params[2] is not
// used and nothing is advanced after the launch.  A row whose pos[b] + 1 would reach seq_ld - 1 is
// left alone too.  lse, lp (optional, together): as for sample_logits -- lp[b, pos[b] + 1] is written
// with seq[b, pos[b] + 1], so a finished row or a row at capacity writes neither.
void pick_ragged(const bf16_t* logits, long ld, int B, int V, uint32_t* params, int* pos, int* done, int64_t* tok,
                 int64_t* seq, long seq_ld, bool greedy, hipStream_t stream, const float* lse = nullptr,
                 float* lp = nullptr);
// Per-token log-probabilities (the rule in common.h): lse[2 r] = the maximum m and lse[2 r + 1] =
// lnz of row r of logits [M, ld] (layout as for sample_logits; one workgroup per row, integer mass
// sum, no float atomics).  targets (optional, int64 [M]): lp[r] = the log-probability of token
// targets[r]; a negative target (or one >= V) leaves lp[r] as it is.
void logits_lse(const bf16_t* logits, long ld, int M, int V, const int64_t* targets, float* lse, float* lp,
                hipStream_t stream);

// process.hip -- the logits processors (the rule in common.h, 'Logits processors'): repetition /
// presence / frequency penalties and the no-repeat n-gram ban, applied in place to the first V
// columns of every row of logits [R, ld] (layout as for sample_logits; columns >= V are never read or
// written).  Row r's history is hist[r * hist_ld + 0 .. min(pos_r, hist_n - 1)] (int64; hist_n <=
// kProcHistMax), pos_r = pos[0] (pos_stride 0) or pos[r] (pos_stride 1), read on the device; a row
// with pos_r < 0 or with done[r] set (done optional, int32 [R]) is left alone.  params (device,
// kProcParamWords x int32): {rp, inv, pp, fp as fp32 bits, g, 0, 0, 0}.  Everything comes from device
// memory and nothing but the logits is written, so a captured launch serves every setting and a
// replay, a warm-up or a repeated launch cannot corrupt any state.
constexpr int kProcParamWords = 8;
constexpr int kProcHistMax = 4096;
constexpr int kProcNgramMax = 8;
void logits_process(bf16_t* logits, long ld, int R, int V, const int64_t* hist, long hist_ld, int hist_n,
                    const int* pos, int pos_stride, const int* done, const uint32_t* params, hipStream_t stream);

// beam.hip -- the tail of a beam decode step (the rule in common.h, 'Beam search'): B prompts, W <= 8
// beams each, R = B * W rows, row b * W + w = beam w of prompt b.  ctl (device, 4 x int32): {history
// column, stop token (negative: none), pad token, 0}.
constexpr int kBeamMax = 8;
constexpr int kBeamCtlWords = 4;
// Per row of logits [R, ld] (layout as for sample_logits, W <= V): lse[2 r], lse[2 r + 1] = {m, lnz}
// exactly as logits_lse writes them, and W candidates (cand_tok[r, k], cand_c[r, k]), k = the rank in
// the row's (logit descending, index ascending) order, c = score[r] + lp.  A row with fin[r] set
// writes (ctl[2], score[r]) and W - 1 empty candidates (token -1), which rank below everything.
void beam_rows(const bf16_t* logits, long ld, int R, int V, int W, const float* score, const int* fin, const int* ctl,
               int* cand_tok, float* cand_c, float* lse, hipStream_t stream);
// Per prompt: the W best of its W * W candidates become the new beams, best first.  Rewrites score,
// fin, len (int32 [R]; a finished parent's length does not grow), tok (int64 [R], the next step's
// input) and parent (int32 [R]), and writes column ctl[0] of hist_parent / hist_tok (int32 [R,
// hist_ld]) and hist_score (fp32, same shape).  Then *pos advances by one.
void beam_merge(int B, int W, int V, const int* cand_tok, const float* cand_c, float* score, int* fin, int* len,
                int64_t* tok, int* parent, int* hist_parent, int* hist_tok, float* hist_score, long hist_ld, int* pos,
                const int* ctl, hipStream_t stream);
// In place, for each of L layers of kv [L, R, Tmax, 3 D] (layer_stride elements apart): rows t <
// min(*pos, Tmax) of the K and V columns of beam r of every prompt become those of beam parent[r] of
// the same prompt.  Q columns, later rows and prompts whose parents are the identity are not
// touched.  ctl (optional): ctl[0] advances by one.  D % 8 == 0.
void beam_reorder(bf16_t* kv, int L, long layer_stride, int B, int W, int Tmax, int D, const int* parent,
                  const int* pos, int* ctl, hipStream_t stream);

// spec.hip -- the kernels around a speculative verify step (the rule in common.h, 'Speculative
// greedy decoding'): B sequences, K <= 8 rows each, row b * K + r = row r of sequence b.  ctl
// (device, 4 x int32): {ngram (clamped to 1 .. 4), end = the column of the last token, 0, 0}.
constexpr int kSpecRowsMax = 8;
constexpr int kSpecNgramMax = 4;
constexpr int kSpecCtlWords = 4;
// Per sequence b with committed tokens seq[b, 0 .. pos[b]] (seq int64 [B, seq_ld], pos clamped to
// [0, seq_ld)): the draft of the rule.  Writes tok[b * K + r] (row 0: seq[b, pos[b]]; without a
// draft every row), pos_rows[b * K + r] = pos[b] + r and has_draft[b] (1 / 0).
void spec_draft(const int64_t* seq, long seq_ld, int B, int K, const int* pos, const int* ctl, int64_t* tok,
                int* pos_rows, int* has_draft, hipStream_t stream);
// g[r] = the argmax of row r of logits [R, ld] (layout as for sample_logits) over its first V columns,
// first index on ties: the ragged greedy pick's ranking of the stored bf16 logits.
void spec_argmax(const bf16_t* logits, long ld, int R, int V, int* g, hipStream_t stream);
// Per sequence b with pos[b] < min(end, seq_ld - 1): a = the number of leading drafts with
// tok[b * K + r] == g[b * K + r - 1] (0 without a draft), cnt = min(a + 1, end - pos[b]);
// seq[b, pos[b] + 1 + i] = g[b * K + i] for i < cnt, pos[b] += cnt, steps[b] += 1 and
// hist[b, cnt] += 1 (hist int32 [B, K + 1]).  Any other sequence is left alone.
void spec_accept(const int* g, const int64_t* tok, const int* has_draft, int B, int K, int* pos, const int* ctl,
                 int64_t* seq, long seq_ld, int* steps, int* hist, hipStream_t stream);

// elementwise.hip
void bias_act_fwd(const bf16_t* x, const bf16_t* b, bf16_t* pre, bf16_t* y, long M, int N, int act,
                  hipStream_t stream);
void bias_dropout_residual(const bf16_t* x, const bf16_t* b, const bf16_t* r, bf16_t* y, long M,
                           int N, float p, uint64_t seed, hipStream_t stream);
void gelu_bwd(const bf16_t* dy, const bf16_t* pre, bf16_t* dx, long n, hipStream_t stream);
void dropout_bwd(const bf16_t* dy, bf16_t* dx, long M, int N, float p, uint64_t seed, hipStream_t stream);
void transpose(const bf16_t* src, bf16_t* dst, int R, int C, int ldd, hipStream_t stream);
void bias_grad(const bf16_t* dy, float* db, long M, int N, hipStream_t stream, long ld = 0);  // row stride ld (0: N)
void dropout_bias_grad(const bf16_t* dy, bf16_t* dx, float* db, long M, int N, float p, uint64_t seed,
                       hipStream_t stream);

// gemm.hip -- layout 0 NT (fwd), 1 NN (dgrad), 2 TN (wgrad, fp32 accumulate)
// epi: 0 none, 1 bias, 2 bias+gelu (gelu'(z) -> aux), 3 resid + dropout(acc + bias), 4 acc*gelu'(aux);
// 6 / 7: 2 / 4 with aux in the fragment order of the W4 256 x 256 tiles (gemm_frag_aux_elems)
void gemm(int layout, int epi, const bf16_t* A, const bf16_t* B, void* C, long lda, long ldb,
          long ldc, int M, int N, int K, int a_ext, int b_ext, int ka, int kb, const bf16_t* bias,
          bf16_t* aux, const bf16_t* resid, float p, uint64_t seed, hipStream_t stream,
          size_t a_bytes, size_t b_bytes,  // operand sizes in bytes (may exceed 4 GiB)
          float* dbias = nullptr);         // EPI 4 / 7: += column sums of C (bias gradient)
void gemm_set_variant(int v);  // tile config override: 0 auto (per shape), 1 T128, 5 W4, 6 W4-192
void gemm_set_debug_buffer(unsigned long long* p);  // MG_GEMM_STAMPS diagnostic builds
int gemm_get_variant();
int gemm_pick(int M, int N, int K, int layout);  // tile config the dispatcher picks (gemm_set_variant codes)

// attention_train.hip / attention.hip -- causal flash attention; qkv [B*T, 3D], out [B*T, D],
// lse [B*H*T]; dmask: dropout keep-bits generated by attention_fwd when p > 0
// (attention_dropout_mask_words u32), read by attention_bwd
size_t attention_dropout_mask_words(int B, int T, int H);
// 16-bit dropout keep threshold of probability p (keep iff a 16-bit uniform >= thr; 0: no dropout)
// and the matching keep scale 65536 / (65536 - thr)
int attention_dropout_threshold(float p);
float attention_dropout_scale(int thr);
void attention_fwd(const bf16_t* qkv, bf16_t* out, float* lse, uint32_t* dmask, int B, int T, int H,
                   int hd, float p, uint64_t seed, hipStream_t stream);
// delta [B*H*T] and dq [attention_bwd_workspace_floats] fp32 are workspaces; writes all three
// slots of dqkv
size_t attention_bwd_workspace_floats(int B, int T, int H, int hd);
// backward schedule (also MINGPT_ATTN_BWD_MODE): 0 auto; 1 persistent (b, h) workgroups, dQ summed
// in place; 2 key-block items with fp32 dQ partials and a finalize pass; 3 chained: a workgroup
// per (b, h) runs its key blocks in order with a running dQ sum and no finalize (hd = 64 with more
// than one key block and attention_set_bwd64 on; elsewhere 3 means 0).  Auto: 1 for a single key
// block, 3 where it exists and B*H fills the CUs in near-whole rounds, else 2.
void attention_set_bwd_mode(int mode);
// 1 (default): hd = 64 backward kernels attn_bwd64_kernel / attn_bwdchain_kernel; 0: the general kernel
void attention_set_bwd64(int on);
#ifdef MG_BWD64_STAMPS
void attention_bwd64_stamps(unsigned long long* host);  // diagnostic build only
#endif
// dbias (fp32 [3D] or null): += the column sums of dqkv (the qkv bias gradient), fused into the
// backward kernels where the schedule allows
void attention_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* dout, const float* lse,
                   const uint32_t* dmask, float* delta, float* dq, bf16_t* dqkv, int B, int T, int H,
                   int hd, float p, uint64_t seed, hipStream_t stream, float* dbias = nullptr);

// one decode step: appends K/V of qkv_new [B, 3D] at row pos of cache [B, Tmax, 3D]; out [B, D].
// part (attention_decode_part_floats(B, H, hd) floats) and counters (B * H, zero; the kernel leaves
// them zero) are the caller's workspace: one per decode state, so a captured hipGraph never sees
// another state's (possibly freed) buffers.  pos_dev: the position in device memory (clamped to
// [0, Tmax)), one for the batch (pos_stride 0) or one per row (pos_stride 1, ragged batches: row b
// appends at cache row pos_dev[b] and attends to keys 0..pos_dev[b], with its own split count).
// group = K > 1 (speculative decoding; needs pos_dev, one int per row): qkv_new [B * K, 3D] and out
// [B * K, D] hold K rows per sequence of cache [B, Tmax, 3D].  Row m = b * K + r sits at position
// base + r, base = pos_dev[b * K] clamped to [0, Tmax): it appends its K/V at cache row base + r of
// sequence b and attends to keys 0 .. base + r -- those at or past base from qkv_new rows b * K ..,
// the earlier ones from the cache -- with the split structure of a plain decode of B sequences at
// that position.  A row with base + r > Tmax - 1 appends nothing and gets a zero out row.  part and
// counters are then sized for B * K rows (attention_decode_part_floats(B * K, H, hd), B * K * H).
size_t attention_decode_part_floats(int B, int H, int hd);
void attention_decode(const bf16_t* qkv_new, bf16_t* cache, bf16_t* out, int B, int H, int hd,
                      long Tmax, int pos, hipStream_t stream, float* part, unsigned* counters,
                      const int* pos_dev = nullptr, int pos_stride = 0, int group = 1);

// Int8 KV cache (the KV8 rule in common.h; attention_kv8.hip).  Per layer: kq int8 [B, 2, H, Tmax, hd]
// (K then V, 16-byte aligned) and ks fp32 [B, 2, H, Tmax], one scale per (b, K | V, h, position).
// hd % 8 == 0, hd <= 128; hd / 8 need not be a power of two.
// kv8_store: snap the K and V thirds of qkv [B, T, 3D] in place per (b, t, head) -- the Q third is
// not touched -- and, with kq / ks given (both or neither), write the int8 values and scales of
// positions 0 .. T - 1 (T <= Tmax; later positions are left alone).  rep = W > 1 (the beam prefill): kq /
// ks have B * rep cache rows and prompt b's (q, s) go to rows b * rep .. b * rep + rep - 1 -- one snap,
// W stores.
void kv8_store(bf16_t* qkv, int8_t* kq, float* ks, int B, int T, int H, int hd, long Tmax, hipStream_t stream,
               int rep = 1);
// attention_decode on the int8 cache: appends the rule's (q, s) of qkv_new's K/V at position pos
// (qkv_new itself is not modified) and writes out [B, D] -- bit for bit what attention_decode writes
// for qkv_new with its K/V thirds snapped over a bf16 cache holding the dequantized rows.  part /
// counters / pos_dev / pos_stride and Tmax <= 4096: attention_decode's.
// group = K > 1 (needs pos_dev, one int per row): attention_decode's grouped form on kq / ks of B
// sequences, qkv_new [B * K, 3D], out [B * K, D], the workspace sized for B * K rows.  Row m = b * K + r
// sits at base + r, base = pos_dev[b * K] clamped to [0, Tmax): keys j < base come from sequence b's
// cache, keys j >= base from qkv_new row b * K + (j - base), snapped by the rule in the workgroup (rows
// 0 .. r of the head) and never read from the cache, so the group's appends cannot race its reads.
// Split 0 of row r appends the (q, s) of its own K/V at cache row base + r.  A row with base + r >
// Tmax - 1 appends nothing, touches no counter and gets a zero out row.  Se, CH, the key order, the
// rounding steps, the hand-off and the combine are the plain kernel's at that position (keys per
// split from B sequences): out and the final cache equal K plain calls at base + r, r = 0 .. K - 1,
// bit for bit, and out equals attention_decode(group = K) on the snapped rows over the dequantized cache.
void attention_decode_kv8(const bf16_t* qkv_new, int8_t* kq, float* ks, bf16_t* out, int B, int H, int hd,
                          long Tmax, int pos, hipStream_t stream, float* part, unsigned* counters,
                          const int* pos_dev = nullptr, int pos_stride = 0, int group = 1);
// beam_reorder on the int8 cache, in place over L layers (kq_layer / ks_layer elements apart): kq int8
// [L, R, 2, H, Tmax, hd], ks fp32 [L, R, 2, H, Tmax], R = B * W.  For every (K | V, head), positions t <
// min(*pos, Tmax) of beam r of a prompt become those of beam parent[r] of the same prompt, int8 bytes
// and scale words alike ((q, s) pairs move unchanged).  Later positions, identity prompts and every
// other byte are not touched; a parent outside [0, W) counts as identity.  ctl (optional): ctl[0]
// advances by one.
void beam_reorder_kv8(int8_t* kq, float* ks, int L, long kq_layer, long ks_layer, int B, int W, int H, int Tmax,
                      int hd, const int* parent, const int* pos, int* ctl, hipStream_t stream);

}  // namespace mg
