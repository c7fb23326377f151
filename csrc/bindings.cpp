// torch <-> gfx950 kernel bindings.  Every op validates shapes/dtypes on the host BEFORE
// launching (a mis-shaped launch can fault the GPU for the whole node), then launches on the
// caller's current HIP stream.  Built into mingpt_distributed_amd/_C.so by build_ext.py.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "comm.h"
#include "kernels.h"

namespace {

using mg::bf16_t;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }
using DevGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_BF16(t) \
  CHECK_DEV(t);       \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16")
#define CHECK_F32(t) \
  CHECK_DEV(t);      \
  TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be fp32")
#define CHECK_I64(t) \
  CHECK_DEV(t);      \
  TORCH_CHECK((t).scalar_type() == at::kLong, #t " must be int64")

inline bf16_t* bp(const at::Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
inline float* fp(const at::Tensor& t) { return t.data_ptr<float>(); }
inline float* fp_opt(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr<float>() : nullptr;
}
inline bf16_t* bp_opt(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? reinterpret_cast<bf16_t*>(t->data_ptr()) : nullptr;
}

// ------------------------------------------------------------------------------- layernorm
std::vector<at::Tensor> layernorm_fwd(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b,
                                      double eps) {
  CHECK_BF16(x); CHECK_BF16(w); CHECK_BF16(b); CHECK_CONTIG(x);
  const int64_t D = x.size(-1), M = x.numel() / D;
  TORCH_CHECK(D % 8 == 0 && D <= 4096, "layernorm: D must be a multiple of 8 and <= 4096");
  TORCH_CHECK(w.numel() == D && b.numel() == D, "layernorm: weight/bias size mismatch");
  DevGuard g(x.device());
  auto y = at::empty_like(x);
  auto mean = at::empty({M}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({M}, x.options().dtype(at::kFloat));
  mg::layernorm_fwd(bp(x), bp(w), bp(b), bp(y), fp(mean), fp(rstd), (int)M, (int)D, (float)eps,
                    cur_stream());
  return {y, mean, rstd};
}

// drop_p > 0 with dz_bias (fp32 [D]): returns (dx, dz), dz = the residual-dropout backward of dx
// (seed: the forward's) and dz's column sums added into dz_bias (layernorm.hip, fused)
std::vector<at::Tensor> layernorm_bwd(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& w,
                                      const at::Tensor& mean, const at::Tensor& rstd, const at::Tensor& dw,
                                      const at::Tensor& db, const c10::optional<at::Tensor>& dres,
                                      const c10::optional<at::Tensor>& dz_bias, double drop_p, int64_t drop_seed) {
  CHECK_BF16(dy); CHECK_BF16(x); CHECK_BF16(w); CHECK_F32(mean); CHECK_F32(rstd);
  CHECK_F32(dw); CHECK_F32(db); CHECK_CONTIG(dy); CHECK_CONTIG(x);
  const int64_t D = x.size(-1), M = x.numel() / D;
  TORCH_CHECK(dy.numel() == x.numel() && dw.numel() == D && db.numel() == D && mean.numel() == M,
              "layernorm_bwd: shape mismatch");
  TORCH_CHECK(D % 8 == 0 && D <= 4096, "layernorm_bwd: D must be a multiple of 8, at most 4096");
  DevGuard g(x.device());
  auto dx = at::empty_like(x);
  if (dres.has_value() && dres->defined()) {
    CHECK_BF16(*dres); CHECK_CONTIG(*dres);
    TORCH_CHECK(dres->numel() == x.numel(), "layernorm_bwd: dres shape");
  }
  const bool drop = dz_bias.has_value() && dz_bias->defined();
  at::Tensor dz;
  if (drop) {
    CHECK_F32(*dz_bias); CHECK_CONTIG(*dz_bias);
    TORCH_CHECK(dz_bias->numel() == D && D % 8 == 0, "layernorm_bwd: dz_bias must be fp32 [D]");
    dz = at::empty_like(x);
  }
  auto ws = at::empty({(int64_t)mg::layernorm_bwd_workspace((int)M, (int)D, drop)}, mean.options());
  mg::layernorm_bwd(bp(dy), bp(x), bp(w), fp(mean), fp(rstd), bp_opt(dres), bp(dx), fp(dw), fp(db), fp(ws),
                    (int)M, (int)D, cur_stream(), drop ? bp(dz) : nullptr, drop ? fp(*dz_bias) : nullptr,
                    (float)drop_p, (uint64_t)drop_seed);
  if (drop) return {dx, dz};
  return {dx};
}

at::Tensor layernorm_bwd_plain(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& w,
                               const at::Tensor& mean, const at::Tensor& rstd, const at::Tensor& dw,
                               const at::Tensor& db, const c10::optional<at::Tensor>& dres) {
  return layernorm_bwd(dy, x, w, mean, rstd, dw, db, dres, c10::nullopt, 0.0, 0)[0];
}

// ------------------------------------------------------------------------------- embedding
// pos_dev (int32 [1], optional; decode with T == 1): the position row of wpe is read on the device.
// pos_stride 1 (ragged batches): pos_dev is int32 [B] and row b takes wpe row pos_dev[b].
// am_part (int64 [B, G], optional, with pos_dev): greedy decode -- the token of row b is the argmax
// of the previous step's LM-head keys am_part[b] (gemv with am_part), written to tok[b] (idx may
// be that same buffer) and to seq[b, pos] when given.
at::Tensor embedding_fwd(const at::Tensor& idx, const at::Tensor& wte, const at::Tensor& wpe,
                         double p, int64_t seed, const c10::optional<at::Tensor>& pos_dev,
                         const c10::optional<at::Tensor>& am_part, const c10::optional<at::Tensor>& seq,
                         int64_t pos_stride) {
  CHECK_I64(idx); CHECK_BF16(wte); CHECK_BF16(wpe); CHECK_CONTIG(idx);
  CHECK_CONTIG(wte); CHECK_CONTIG(wpe);
  TORCH_CHECK(idx.dim() == 2, "idx must be [B, T]");
  const int64_t B = idx.size(0), T = idx.size(1), D = wte.size(1);
  TORCH_CHECK(D % 8 == 0 && wpe.size(1) == D && T <= wpe.size(0), "embedding: shape mismatch");
  const int* pd = nullptr;
  if (pos_dev.has_value()) {
    TORCH_CHECK(T == 1 && pos_dev->scalar_type() == at::kInt && pos_dev->is_cuda(),
                "embedding_fwd: pos_dev (int32 cuda) is for one-token decode steps");
    TORCH_CHECK((pos_stride == 0 || pos_stride == 1) && pos_dev->is_contiguous() &&
                pos_dev->numel() >= (pos_stride ? B : 1) && pos_dev->device() == idx.device(),
                "embedding_fwd: pos_dev int32 [1] (pos_stride 0) or [B] (pos_stride 1)");
    TORCH_CHECK(pos_stride == 0 || !am_part.has_value(), "embedding_fwd: am_part needs pos_stride 0");
    pd = pos_dev->data_ptr<int>();
  } else {
    TORCH_CHECK(pos_stride == 0, "embedding_fwd: pos_stride needs pos_dev");
  }
  const unsigned long long* ap = nullptr;
  int groups = 0;
  int64_t* seqp = nullptr;
  long seq_ld = 0;
  if (am_part.has_value()) {
    TORCH_CHECK(pd && am_part->scalar_type() == at::kLong && am_part->is_contiguous() && am_part->dim() == 2 &&
                am_part->size(0) == B, "embedding_fwd: am_part int64 [B, G] with pos_dev");
    ap = reinterpret_cast<const unsigned long long*>(am_part->data_ptr<int64_t>());
    groups = (int)am_part->size(1);
    if (seq.has_value()) {
      TORCH_CHECK(seq->scalar_type() == at::kLong && seq->is_contiguous() && seq->dim() == 2 && seq->size(0) == B,
                  "embedding_fwd: seq int64 [B, L]");
      seqp = seq->data_ptr<int64_t>();
      seq_ld = seq->size(1);
    }
  }
  DevGuard g(idx.device());
  auto out = at::empty({B, T, D}, wte.options());
  mg::embedding_fwd(idx.data_ptr<int64_t>(), bp(wte), bp(wpe), bp(out), (int)(B * T), (int)T,
                    (int)D, (int)wte.size(0), (float)p, (uint64_t)seed, cur_stream(), pd, ap, groups,
                    ap ? idx.data_ptr<int64_t>() : nullptr, seqp, seq_ld, (int)pos_stride, (int)wpe.size(0));
  return out;
}

void embedding_bwd(const at::Tensor& idx, const at::Tensor& dout,
                   const c10::optional<at::Tensor>& dwte, const c10::optional<at::Tensor>& dwpe,
                   double p, int64_t seed) {
  CHECK_I64(idx); CHECK_BF16(dout); CHECK_CONTIG(dout); CHECK_CONTIG(idx);
  const int64_t B = idx.size(0), T = idx.size(1), D = dout.size(-1);
  TORCH_CHECK(dout.numel() == B * T * D, "embedding_bwd: shape mismatch");
  if (dwte.has_value()) { CHECK_F32(*dwte); TORCH_CHECK(dwte->size(-1) == D); }
  if (dwpe.has_value()) { CHECK_F32(*dwpe); TORCH_CHECK(dwpe->size(-1) == D && dwpe->size(0) >= T); }
  DevGuard g(idx.device());
  mg::embedding_bwd(idx.data_ptr<int64_t>(), bp(dout), fp_opt(dwte), fp_opt(dwpe), (int)(B * T),
                    (int)T, (int)D, dwte.has_value() ? (int)(dwte->numel() / D) : 0, (float)p, (uint64_t)seed, cur_stream());
}

// ------------------------------------------------------------------------------- cross entropy
// logits [M, ld] with V valid columns; returns (out[2] = {loss, 1/n_valid}, lse[M])
std::vector<at::Tensor> xent_fwd(const at::Tensor& logits, const at::Tensor& targets, int64_t V) {
  CHECK_BF16(logits); CHECK_I64(targets); CHECK_CONTIG(logits); CHECK_CONTIG(targets);
  const int64_t ld = logits.size(-1), M = logits.numel() / ld;
  TORCH_CHECK(targets.numel() == M && V <= ld && ld % 8 == 0, "xent: shape mismatch");
  DevGuard g(logits.device());
  auto opts = logits.options().dtype(at::kFloat);
  auto loss_row = at::empty({M}, opts);
  auto lse = at::empty({M}, opts);
  auto out = at::empty({2}, opts);
  mg::xent_fwd(bp(logits), targets.data_ptr<int64_t>(), fp(loss_row), fp(lse), fp(out), (int)M,
               (int)V, (int)ld, cur_stream());
  return {out, lse};
}

at::Tensor xent_bwd(const at::Tensor& logits, const at::Tensor& targets, const at::Tensor& lse,
                    const at::Tensor& gscale, const at::Tensor& out, int64_t V) {
  CHECK_BF16(logits); CHECK_I64(targets); CHECK_F32(lse); CHECK_F32(gscale); CHECK_F32(out);
  const int64_t ld = logits.size(-1), M = logits.numel() / ld;
  TORCH_CHECK(targets.numel() == M && lse.numel() == M, "xent_bwd: shape mismatch");
  DevGuard g(logits.device());
  auto dl = at::empty_like(logits);
  mg::xent_bwd(bp(logits), targets.data_ptr<int64_t>(), fp(lse), fp(gscale), fp(out) + 1, bp(dl),
               (int)M, (int)V, (int)ld, cur_stream());
  return dl;
}

// one-pass training cross-entropy: returns (out[2] = {loss, 1/n_valid}, dlogits = (softmax -
// onehot) / n_valid); empty list when the row width is outside the fused kernel's range
std::vector<at::Tensor> xent_fused(const at::Tensor& logits, const at::Tensor& targets, int64_t V) {
  CHECK_BF16(logits); CHECK_I64(targets); CHECK_CONTIG(logits); CHECK_CONTIG(targets);
  const int64_t ld = logits.size(-1), M = logits.numel() / ld;
  TORCH_CHECK(targets.numel() == M && V <= ld && ld % 8 == 0, "xent_fused: shape mismatch");
  if (mg::xent_fused_nv((int)ld) == 0) return {};
  DevGuard g(logits.device());
  auto opts = logits.options().dtype(at::kFloat);
  auto loss_row = at::empty({M}, opts);
  auto out = at::empty({2}, opts);
  auto dl = at::empty_like(logits);
  mg::xent_fused(bp(logits), targets.data_ptr<int64_t>(), fp(loss_row), fp(out), bp(dl), (int)M,
                 (int)V, (int)ld, cur_stream());
  return {out, dl};
}

void xent_scale_(const at::Tensor& dlogits, const at::Tensor& gscale) {
  CHECK_BF16(dlogits); CHECK_CONTIG(dlogits); CHECK_F32(gscale);
  TORCH_CHECK(dlogits.numel() % 8 == 0, "xent_scale_: numel must be a multiple of 8");
  DevGuard g(dlogits.device());
  mg::xent_scale(bp(dlogits), fp(gscale), dlogits.numel(), cur_stream());
}

// ------------------------------------------------------------------------------- hipGraph mode
// While set, launches read dropout-seed offsets from seed_ofs[0] (uint64, bumped inside the graph
// each replay) and AdamW reads {lr, step} from opt_hp (fp32[2], written before each replay).
void set_graph_state(const c10::optional<at::Tensor>& seed_ofs, const c10::optional<at::Tensor>& opt_hp) {
  if (seed_ofs.has_value()) {
    TORCH_CHECK(seed_ofs->scalar_type() == at::kLong && seed_ofs->is_cuda() && seed_ofs->numel() >= 1);
  }
  if (opt_hp.has_value()) { CHECK_F32(*opt_hp); TORCH_CHECK(opt_hp->numel() >= 2); }
  mg::set_graph_state(seed_ofs.has_value() ? reinterpret_cast<const uint64_t*>(seed_ofs->data_ptr<int64_t>()) : nullptr,
                      opt_hp.has_value() ? fp(*opt_hp) : nullptr);
}

// ------------------------------------------------------------------------------- optimizer
void grad_sumsq(const at::Tensor& grad, double grad_scale, const at::Tensor& out) {
  CHECK_F32(grad); CHECK_F32(out); CHECK_CONTIG(grad);
  TORCH_CHECK(out.numel() >= 2);
  DevGuard g(grad.device());
  auto ws = at::empty({(int64_t)(mg::grad_norm_workspace() / 4)}, grad.options());
  mg::grad_sumsq(fp(grad), grad.numel(), (float)grad_scale, fp(ws), fp(out), cur_stream());
}

// The chunk tables are built and range-checked on the host by optim.make_chunk_table, which
// also returns the bounds it checked against (table_end: one past the last flat element any
// chunk touches; moment_end: the same for the packed moments).  The kernels index through the
// tables unchecked, so every buffer handed in here must cover those bounds: a table built for
// another store (e.g. before a re-layout) fails here instead of reading or writing out of bounds.
void grad_sumsq_chunks(const at::Tensor& chunk_start, const at::Tensor& chunk_len,
                       const at::Tensor& grad, double grad_scale, const at::Tensor& out,
                       int64_t table_end) {
  CHECK_I64(chunk_start); CHECK_DEV(chunk_len); CHECK_CONTIG(grad); CHECK_F32(out);
  TORCH_CHECK(chunk_len.scalar_type() == at::kInt, "chunk_len must be int32");
  TORCH_CHECK(grad.scalar_type() == at::kFloat || grad.scalar_type() == at::kBFloat16,
              "grad must be fp32 or bf16");
  TORCH_CHECK(chunk_start.numel() == chunk_len.numel() && out.numel() >= 2);
  TORCH_CHECK(table_end >= 0 && grad.numel() >= table_end, "grad_sumsq_chunks: chunk table reaches element ",
              table_end, " of a ", grad.numel(), "-element gradient buffer");
  const int64_t nc = chunk_len.numel();
  if (nc == 0) { out.zero_(); return; }
  DevGuard g(grad.device());
  auto ws = at::empty({nc}, out.options());
  mg::grad_sumsq_chunks(chunk_start.data_ptr<int64_t>(), chunk_len.data_ptr<int>(), (int)nc,
                        grad.data_ptr(), grad.scalar_type() == at::kBFloat16, (float)grad_scale,
                        fp(ws), fp(out), cur_stream());
}

void adamw_step(const at::Tensor& chunk_start, const at::Tensor& chunk_len,
                const at::Tensor& chunk_wd, const c10::optional<at::Tensor>& moment_start,
                const at::Tensor& master, const at::Tensor& param, const at::Tensor& grad,
                const at::Tensor& m, const at::Tensor& v, const at::Tensor& norm, double lr,
                double b1, double b2, double eps, int64_t step, double grad_scale, double clip,
                int64_t table_end, int64_t moment_end, const c10::optional<at::Tensor>& zero_grad) {
  CHECK_I64(chunk_start); CHECK_DEV(chunk_len); CHECK_F32(chunk_wd);
  TORCH_CHECK(chunk_len.scalar_type() == at::kInt, "chunk_len must be int32");
  CHECK_F32(master); CHECK_BF16(param); CHECK_F32(m); CHECK_F32(v); CHECK_F32(norm);
  CHECK_DEV(grad);
  TORCH_CHECK(grad.scalar_type() == at::kFloat || grad.scalar_type() == at::kBFloat16,
              "grad must be fp32 or bf16");
  const int64_t n = master.numel();
  TORCH_CHECK(param.numel() == n && grad.numel() == n, "adamw: flat buffer size mismatch");
  TORCH_CHECK(table_end >= 0 && n >= table_end, "adamw: chunk table reaches element ", table_end,
              " of ", n, "-element flat buffers");
  TORCH_CHECK(moment_end >= 0 && m.numel() >= moment_end && v.numel() >= moment_end,
              "adamw: chunk table reaches moment ", moment_end, " of ", m.numel());
  const int64_t* ms = nullptr;
  if (moment_start.has_value() && moment_start->defined()) {
    CHECK_I64(*moment_start);
    TORCH_CHECK(moment_start->numel() == chunk_start.numel(), "adamw: moment table length");
    TORCH_CHECK(m.numel() == v.numel(), "adamw: moment buffer size mismatch");
    ms = moment_start->data_ptr<int64_t>();
  } else {
    TORCH_CHECK(m.numel() == n && v.numel() == n, "adamw: moment buffer size mismatch");
  }
  TORCH_CHECK(chunk_start.numel() == chunk_len.numel() && chunk_wd.numel() == chunk_len.numel());
  float* zg = nullptr;  // fp32 main grads zeroed as they are consumed (same flat indexing)
  if (zero_grad.has_value() && zero_grad->defined()) {
    CHECK_F32(*zero_grad);
    TORCH_CHECK(zero_grad->numel() >= table_end, "adamw: zero_grad buffer shorter than the chunk table");
    zg = fp(*zero_grad);
  }
  if (chunk_len.numel() == 0) return;
  DevGuard g(master.device());
  mg::adamw_step(chunk_start.data_ptr<int64_t>(), chunk_len.data_ptr<int>(), fp(chunk_wd), ms,
                 (int)chunk_len.numel(), fp(master), bp(param), grad.data_ptr(),
                 grad.scalar_type() == at::kBFloat16, fp(m), fp(v), fp(norm), (float)lr, (float)b1,
                 (float)b2, (float)eps, (int)step, (float)grad_scale, (float)clip, cur_stream(),
                 zg);
}

void f32_to_bf16(const at::Tensor& src, const at::Tensor& dst) {
  CHECK_F32(src); CHECK_BF16(dst);
  TORCH_CHECK(src.numel() == dst.numel() && src.is_contiguous() && dst.is_contiguous());
  DevGuard g(src.device());
  mg::f32_to_bf16(fp(src), bp(dst), src.numel(), cur_stream());
}

void comm_proxy(const at::Tensor& src, const at::Tensor& scratch, double factor, int64_t channels,
                double gbps) {
  TORCH_CHECK(src.is_cuda() && scratch.is_cuda() && src.is_contiguous() && scratch.is_contiguous());
  const int64_t bytes = src.numel() * src.element_size();
  TORCH_CHECK(scratch.numel() * scratch.element_size() >= bytes, "comm_proxy: scratch too small");
  TORCH_CHECK(factor >= 0 && factor < 2 && channels > 0 && channels <= 1024 && gbps >= 0);
  // a timing model: the bucket's 16-byte-aligned interior is moved, < 32 edge bytes are not
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(src.data_ptr()), pa = (p0 + 15) & ~uintptr_t(15);
  const long n16 = bytes >= (int64_t)(pa - p0) ? (long)((bytes - (int64_t)(pa - p0)) / 16) : 0;
  DevGuard g(src.device());
  mg::comm_proxy(reinterpret_cast<const void*>(pa), scratch.data_ptr(), n16, (long)(factor * n16),
                 (int)channels, gbps, cur_stream());
}

// ------------------------------------------------------------------------------- elementwise
at::Tensor bias_act(const at::Tensor& x, const c10::optional<at::Tensor>& b,
                    const c10::optional<at::Tensor>& pre, int64_t act) {
  CHECK_BF16(x); CHECK_CONTIG(x);
  const int64_t N = x.size(-1), M = x.numel() / N;
  TORCH_CHECK(N % 8 == 0, "bias_act: N % 8 != 0");
  if (b.has_value()) { CHECK_BF16(*b); TORCH_CHECK(b->numel() == N); }
  if (pre.has_value()) { CHECK_BF16(*pre); TORCH_CHECK(pre->numel() == x.numel()); }
  DevGuard g(x.device());
  auto y = at::empty_like(x);
  mg::bias_act_fwd(bp(x), bp_opt(b), bp_opt(pre), bp(y), M, (int)N, (int)act, cur_stream());
  return y;
}

at::Tensor bias_dropout_residual(const at::Tensor& x, const c10::optional<at::Tensor>& b,
                                 const at::Tensor& r, double p, int64_t seed) {
  CHECK_BF16(x); CHECK_BF16(r); CHECK_CONTIG(x); CHECK_CONTIG(r);
  const int64_t N = x.size(-1), M = x.numel() / N;
  TORCH_CHECK(N % 8 == 0 && r.numel() == x.numel(), "bias_dropout_residual: shape mismatch");
  if (b.has_value()) { CHECK_BF16(*b); TORCH_CHECK(b->numel() == N); }
  DevGuard g(x.device());
  auto y = at::empty_like(x);
  mg::bias_dropout_residual(bp(x), bp_opt(b), bp(r), bp(y), M, (int)N, (float)p, (uint64_t)seed,
                            cur_stream());
  return y;
}

at::Tensor gelu_bwd(const at::Tensor& dy, const at::Tensor& pre) {
  CHECK_BF16(dy); CHECK_BF16(pre); CHECK_CONTIG(dy); CHECK_CONTIG(pre);
  TORCH_CHECK(dy.numel() == pre.numel() && dy.numel() % 8 == 0);
  DevGuard g(dy.device());
  auto dx = at::empty_like(dy);
  mg::gelu_bwd(bp(dy), bp(pre), bp(dx), dy.numel(), cur_stream());
  return dx;
}

// dst[C, ldd] = src[R, C]^T with columns R..ldd-1 zero (ldd = 0 -> R)
at::Tensor transpose(const at::Tensor& src, int64_t ldd) {
  CHECK_BF16(src); CHECK_CONTIG(src);
  TORCH_CHECK(src.dim() == 2, "transpose: 2-D input");
  const int64_t R = src.size(0), C = src.size(1);
  if (ldd <= 0) ldd = R;
  TORCH_CHECK(ldd >= R, "transpose: ldd < rows");
  DevGuard g(src.device());
  auto dst = at::empty({C, ldd}, src.options());
  mg::transpose(bp(src), bp(dst), (int)R, (int)C, (int)ldd, cur_stream());
  return dst;
}

// residual-stream dropout backward: the mask is keyed on (row, column) of the [.., N] tensor
at::Tensor dropout_bwd(const at::Tensor& dy, double p, int64_t seed) {
  CHECK_BF16(dy); CHECK_CONTIG(dy);
  const int64_t N = dy.size(-1), M = dy.numel() / N;
  TORCH_CHECK(N % 8 == 0, "dropout_bwd: last dim must be a multiple of 8");
  DevGuard g(dy.device());
  auto dx = at::empty_like(dy);
  mg::dropout_bwd(bp(dy), bp(dx), M, (int)N, (float)p, (uint64_t)seed, cur_stream());
  return dx;
}

// dx = dropout_bwd(dy) and db += colsum(dx) in one pass
at::Tensor dropout_bias_grad(const at::Tensor& dy, const at::Tensor& db, double p, int64_t seed) {
  CHECK_BF16(dy); CHECK_F32(db); CHECK_CONTIG(dy);
  const int64_t N = dy.size(-1), M = dy.numel() / N;
  TORCH_CHECK(N % 8 == 0 && db.numel() == N, "dropout_bias_grad: shape mismatch");
  DevGuard g(dy.device());
  auto dx = at::empty_like(dy);
  mg::dropout_bias_grad(bp(dy), bp(dx), fp(db), M, (int)N, (float)p, (uint64_t)seed, cur_stream());
  return dx;
}

void bias_grad(const at::Tensor& dy, const at::Tensor& db) {
  CHECK_BF16(dy); CHECK_F32(db); CHECK_CONTIG(dy);
  const int64_t N = dy.size(-1), M = dy.numel() / N;
  TORCH_CHECK(N % 8 == 0 && db.numel() == N, "bias_grad: shape mismatch");
  DevGuard g(dy.device());
  mg::bias_grad(bp(dy), fp(db), M, (int)N, cur_stream());
}

// ------------------------------------------------------------------------------- gemm
// layout 0 (NT): c[M, ldc] = a[M, K] @ b[N, K]^T           (+ epilogue)
// layout 1 (NN): c[M, N]   = a[M, K] @ b[Kb, N]            (b rows >= Kb read as zero)
// layout 2 (TN): c[M, N]  += a[K, Ma]^T @ b[K, N]   fp32 c (M <= Ma store rows)
void gemm(const at::Tensor& a, const at::Tensor& b, const at::Tensor& c, int64_t layout, int64_t epi,
          const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& aux,
          const c10::optional<at::Tensor>& resid, double p, int64_t seed, int64_t M, int64_t N,
          const c10::optional<at::Tensor>& dbias) {
  CHECK_BF16(a); CHECK_BF16(b); CHECK_DEV(c);
  CHECK_CONTIG(a); CHECK_CONTIG(b); CHECK_CONTIG(c);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "gemm: 2-D operands required");
  TORCH_CHECK(layout >= 0 && layout <= 2 && epi >= 0 && epi <= 7 && epi != 5, "gemm: bad layout/epilogue");
  TORCH_CHECK((epi != 6 || layout == 0) && (epi != 7 || layout == 1), "gemm: fragment-ordered GELU' epilogues: 6 NT, 7 NN");
  const int64_t lda = a.size(1), ldb = b.size(1), ldc = c.size(1);
  TORCH_CHECK(lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0, "gemm: row strides must be multiples of 8");
  TORCH_CHECK(M > 0 && N > 0 && M <= c.size(0) && N <= ldc, "gemm: output bounds");
  int64_t K, a_ext, b_ext, ka, kb;
  if (layout == 0) {
    K = lda; ka = lda; kb = ldb; a_ext = a.size(0); b_ext = b.size(0);
    TORCH_CHECK(lda == ldb, "gemm NT: K mismatch");
    TORCH_CHECK(M <= a_ext && N <= (epi == 0 ? ldc : b_ext), "gemm NT: shape mismatch");
    TORCH_CHECK(c.scalar_type() == at::kBFloat16, "gemm NT: bf16 output");
  } else if (layout == 1) {
    K = lda; ka = lda; kb = b.size(0); a_ext = a.size(0); b_ext = ldb;
    TORCH_CHECK(kb <= K && M <= a_ext && N <= ldb && (epi == 0 || epi == 4 || epi == 7), "gemm NN: shape mismatch");
    TORCH_CHECK(c.scalar_type() == at::kBFloat16, "gemm NN: bf16 output");
  } else {
    K = a.size(0); ka = K; kb = b.size(0); a_ext = lda; b_ext = ldb;
    TORCH_CHECK(kb == K && M <= lda && N <= ldb && epi == 0, "gemm TN: shape mismatch");
    TORCH_CHECK(c.scalar_type() == at::kFloat, "gemm TN: fp32 accumulate output");
  }
  TORCH_CHECK(K % 8 == 0, "gemm: K must be a multiple of 8");
  const bf16_t* bias_p = nullptr;
  if (bias.has_value() && bias->defined()) {
    CHECK_BF16(*bias);
    TORCH_CHECK(bias->numel() >= N, "gemm: bias too short");
    bias_p = bp(*bias);
  }
  bf16_t* aux_p = nullptr;
  if (epi == 2 || epi == 4 || epi == 6 || epi == 7) {
    TORCH_CHECK(aux.has_value() && aux->defined(), "gemm: epilogue needs aux");
    CHECK_BF16(*aux); CHECK_CONTIG(*aux);
    if (epi >= 6) {  // fragment order: whole 256 x 256 tiles
      TORCH_CHECK(aux->numel() == ((M + 255) / 256) * ((N + 255) / 256) * 65536 && ldc == N,
                  "gemm: fragment-ordered aux must hold ceil(M/256) * ceil(N/256) * 65536 elements");
    } else {
      TORCH_CHECK(aux->numel() == c.numel(), "gemm: aux shape");
    }
    aux_p = bp(*aux);
  }
  const bf16_t* res_p = nullptr;
  if (epi == 3) {
    TORCH_CHECK(resid.has_value() && resid->defined(), "gemm: epilogue needs resid");
    CHECK_BF16(*resid); CHECK_CONTIG(*resid);
    TORCH_CHECK(resid->numel() == c.numel() && ldc == N, "gemm: resid shape");
    res_p = bp(*resid);
  }
  // operands past 4 GiB are fine: every block's buffer descriptor starts at its own tile / split
  // origin (gemm.hip Stager::retarget; split-K ranges are capped below 4 GiB by set_split)
  float* dbias_p = nullptr;
  if (dbias.has_value() && dbias->defined()) {
    CHECK_F32(*dbias);
    TORCH_CHECK((epi == 4 || epi == 7) && dbias->numel() >= N, "gemm: dbias only with the gelu_bwd epilogue");
    dbias_p = fp(*dbias);
  }
  DevGuard g(a.device());
  mg::gemm((int)layout, (int)epi, bp(a), bp(b), c.data_ptr(), lda, ldb, ldc, (int)M, (int)N, (int)K,
           (int)a_ext, (int)b_ext, (int)ka, (int)kb, bias_p, aux_p, res_p, (float)p, (uint64_t)seed,
           cur_stream(), (size_t)a.numel() * 2, (size_t)b.numel() * 2, dbias_p);
}

// ------------------------------------------------------------------------------- attention
std::vector<at::Tensor> attention_fwd(const at::Tensor& qkv, int64_t B, int64_t T, int64_t H,
                                      double p, int64_t seed) {
  CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  const int64_t D3 = qkv.size(-1), D = D3 / 3, hd = D / H;
  TORCH_CHECK(D3 == 3 * D && D == H * hd && qkv.numel() == B * T * D3, "attention: qkv shape");
  TORCH_CHECK(hd % 8 == 0 && hd <= 128, "attention: head dim must be a multiple of 8 and <= 128");
  DevGuard g(qkv.device());
  auto out = at::empty({B * T, D}, qkv.options());
  auto lse = at::empty({B * H * T}, qkv.options().dtype(at::kFloat));
  at::Tensor mask = p > 0 ? at::empty({(int64_t)mg::attention_dropout_mask_words((int)B, (int)T, (int)H)},
                                      qkv.options().dtype(at::kInt))
                          : at::empty({0}, qkv.options().dtype(at::kInt));
  mg::attention_fwd(bp(qkv), bp(out), fp(lse),
                    p > 0 ? reinterpret_cast<uint32_t*>(mask.data_ptr<int>()) : nullptr, (int)B, (int)T,
                    (int)H, (int)hd, (float)p, (uint64_t)seed, cur_stream());
  return {out, lse, mask};
}

at::Tensor attention_bwd(const at::Tensor& qkv, const at::Tensor& out, const at::Tensor& dout,
                         const at::Tensor& lse, const at::Tensor& mask, int64_t B, int64_t T,
                         int64_t H, double p, int64_t seed, const c10::optional<at::Tensor>& dbias) {
  CHECK_BF16(qkv); CHECK_BF16(out); CHECK_BF16(dout); CHECK_F32(lse);
  CHECK_CONTIG(qkv); CHECK_CONTIG(out); CHECK_CONTIG(dout);
  const int64_t D3 = qkv.size(-1), D = D3 / 3, hd = D / H;
  TORCH_CHECK(qkv.numel() == B * T * D3 && out.numel() == B * T * D && dout.numel() == B * T * D &&
              lse.numel() == B * H * T && hd % 8 == 0 && hd <= 128 && D <= 4096, "attention_bwd: shape mismatch");
  TORCH_CHECK(B * T * H * 16 < (int64_t)1 << 31, "attention_bwd: B*T*H too large");
  DevGuard g(qkv.device());
  auto dqkv = at::empty_like(qkv);
  auto opts = qkv.options().dtype(at::kFloat);
  auto delta = at::empty({B * H * T}, opts);  // rowsum(dO * O) per (b, h, t), attn_bwd_pre_kernel
  // fp32 dQ accumulator (persistent mode) or per-key-block partials (attention_train.hip)
  auto dq = at::empty({(int64_t)mg::attention_bwd_workspace_floats((int)B, (int)T, (int)H, (int)hd)}, opts);
  const uint32_t* mp = nullptr;
  if (p > 0) {
    CHECK_DEV(mask);
    TORCH_CHECK(mask.scalar_type() == at::kInt &&
                    mask.numel() == (int64_t)mg::attention_dropout_mask_words((int)B, (int)T, (int)H),
                "attention_bwd: dropout mask from attention_fwd required when p > 0");
    mp = reinterpret_cast<const uint32_t*>(mask.data_ptr<int>());
  }
  float* db = nullptr;
  if (dbias.has_value() && dbias->defined()) {
    CHECK_F32(*dbias); CHECK_CONTIG(*dbias);
    TORCH_CHECK(dbias->numel() == D3, "attention_bwd: dbias must be fp32 [3D]");
    db = fp(*dbias);
  }
  mg::attention_bwd(bp(qkv), bp(out), bp(dout), fp(lse), mp, fp(delta), fp(dq), bp(dqkv), (int)B,
                    (int)T, (int)H, (int)hd, (float)p, (uint64_t)seed, cur_stream(), db);
  return dqkv;
}

// The shared arguments of the decode-time projections y[M, ldy] = epi(x[M, K] @ W[N, K]^T) (gemv.hip,
// gemm_rows.hip): x bf16 [..., K] and W bf16 [N, K], contiguous; ldy <= 0 means N, else ldy >= N;
// epi 0 none, 1 bias, 2 bias + GELU, 3 bias + residual, with bias bf16 [N] when given (null
// otherwise) and resid bf16 [M, ldy] for epi 3 (null otherwise).  How many rows and how long a row
// an op takes is that op's own check.  w8: W is int8 [N, K] instead (gemv_w8), 8-byte aligned.
struct ProjArgs {
  int64_t M, N, K, ldy;
  const bf16_t *bias, *resid;
};

ProjArgs proj_args(const char* op, const at::Tensor& x, const at::Tensor& W, int64_t epi,
                   const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& resid, int64_t ldy,
                   bool w8 = false) {
  CHECK_BF16(x); CHECK_CONTIG(x); CHECK_CONTIG(W);
  if (w8) {
    CHECK_DEV(W);
    TORCH_CHECK(W.scalar_type() == at::kChar, op, ": Wq must be int8");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(W.data_ptr()) % 8 == 0, op, ": Wq must be 8-byte aligned");
  } else {
    CHECK_BF16(W);
  }
  TORCH_CHECK(W.dim() == 2 && W.size(0) >= 1 && W.size(1) >= 1, op, ": W [N, K]");
  const int64_t K = W.size(1), N = W.size(0), M = x.numel() / K;
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) == K, op, ": x [..., K] against W [N, K]");
  if (ldy <= 0) ldy = N;
  TORCH_CHECK(ldy >= N && epi >= 0 && epi <= 3, op, ": ldy / epi");
  if (bias.has_value()) { CHECK_BF16(*bias); TORCH_CHECK(bias->numel() == N, op, ": bias size"); }
  if (epi == 3) {
    TORCH_CHECK(resid.has_value(), op, ": residual epilogue needs resid");
    CHECK_BF16(*resid); CHECK_CONTIG(*resid);
    TORCH_CHECK(resid->numel() == M * ldy, op, ": resid shape");
  }
  return {M, N, K, ldy, bias.has_value() ? bp(*bias) : nullptr, epi == 3 ? bp(*resid) : nullptr};
}

// y[B, ldy] (ldy >= N) = epi(x[B, K] @ W[N, K]^T): the decode-time projection (gemv.hip).  scale
// null: W bf16 (gemv); else W int8 with scale fp32 [N] (gemv_w8) -- one set of checks for both.
at::Tensor gemv_any(const char* op, const at::Tensor& x, const at::Tensor& W, const at::Tensor* scale, int64_t epi,
                    const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& resid, int64_t ldy,
                    const c10::optional<at::Tensor>& lnw, const c10::optional<at::Tensor>& lnb, double eps,
                    const c10::optional<at::Tensor>& am_part, const c10::optional<at::Tensor>& am_pos) {
  const ProjArgs p = proj_args(op, x, W, epi, bias, resid, ldy, scale != nullptr);
  const int64_t B = p.M, N = p.N, K = p.K;
  if (scale) {
    CHECK_F32(*scale); CHECK_CONTIG(*scale);
    TORCH_CHECK(scale->dim() == 1 && scale->numel() == N, op, ": scale fp32 [N]");
  }
  TORCH_CHECK(mg::gemv_supported((int)B, (int)K), "gemv: B <= 8, K % 8 == 0, K <= 8192");
  // rows staged in two segments: the one-row-per-wave path without fused LayerNorm only
  TORCH_CHECK(K <= mg::kGemvSegK || N <= 8192, "gemv: K > 4096 needs N <= 8192 (wide outputs take K <= 4096)");
  TORCH_CHECK(K <= mg::kGemvSegK || !(lnw.has_value() || lnb.has_value()),
              "gemv: K > 4096 cannot take LayerNorm weights (the fused LayerNorm takes K <= 4096)");
  TORCH_CHECK(lnw.has_value() == lnb.has_value(), "gemv: LayerNorm needs weight and bias");
  if (lnw.has_value()) {
    CHECK_BF16(*lnw); CHECK_BF16(*lnb);
    TORCH_CHECK(lnw->numel() == K && lnb->numel() == K, "gemv: LayerNorm size");
  }
  DevGuard g(x.device());
  mg::GemvArgmax am{};
  if (am_part.has_value()) {
    // greedy decode: the LM-head GEMV (N > 8192 rows) also leaves one argmax key per (row,
    // workgroup) in am_part [B, gemv_grid(N, B)] (int64 storage of the unsigned keys) and advances
    // *am_pos; the next step's embedding_fwd(am_part=...) reduces the keys into the token
    TORCH_CHECK(N > 8192 && epi == 0, "gemv argmax: LM-head shape (N > 8192, no epilogue)");
    TORCH_CHECK(am_part->scalar_type() == at::kLong && am_part->is_cuda() && am_part->is_contiguous() &&
                am_part->numel() == B * mg::gemv_grid((int)N, (int)B), "gemv argmax: am_part int64 [B, gemv_argmax_groups(N, B)]");
    TORCH_CHECK(am_pos.has_value() && am_pos->scalar_type() == at::kInt && am_pos->is_cuda(),
                "gemv argmax: am_pos int32 [1]");
    am.part = reinterpret_cast<unsigned long long*>(am_part->data_ptr<int64_t>());
    am.pos = am_pos->data_ptr<int>();
  }
  auto y = at::empty({B, p.ldy}, x.options());
  const mg::GemvArgmax* amp = am_part.has_value() ? &am : nullptr;
  if (scale)
    mg::gemv_w8(bp(x), W.data_ptr<int8_t>(), fp(*scale), bp(y), (int)B, (int)N, (int)K, p.ldy, p.bias, p.resid,
                (int)epi, cur_stream(), bp_opt(lnw), bp_opt(lnb), (float)eps, amp);
  else
    mg::gemv(bp(x), bp(W), bp(y), (int)B, (int)N, (int)K, p.ldy, p.bias, p.resid, (int)epi, cur_stream(), bp_opt(lnw),
             bp_opt(lnb), (float)eps, amp);
  return y;
}

at::Tensor gemv(const at::Tensor& x, const at::Tensor& W, int64_t epi, const c10::optional<at::Tensor>& bias,
                const c10::optional<at::Tensor>& resid, int64_t ldy, const c10::optional<at::Tensor>& lnw,
                const c10::optional<at::Tensor>& lnb, double eps, const c10::optional<at::Tensor>& am_part,
                const c10::optional<at::Tensor>& am_pos) {
  return gemv_any("gemv", x, W, nullptr, epi, bias, resid, ldy, lnw, lnb, eps, am_part, am_pos);
}

// the same on int8 weight rows Wq [N, K] with one power-of-two fp32 scale per row (the W8 rule, common.h)
at::Tensor gemv_w8(const at::Tensor& x, const at::Tensor& Wq, const at::Tensor& scale, int64_t epi,
                   const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& resid, int64_t ldy,
                   const c10::optional<at::Tensor>& lnw, const c10::optional<at::Tensor>& lnb, double eps,
                   const c10::optional<at::Tensor>& am_part, const c10::optional<at::Tensor>& am_pos) {
  return gemv_any("gemv_w8", x, Wq, &scale, epi, bias, resid, ldy, lnw, lnb, eps, am_part, am_pos);
}

// y[M, ldy] (ldy >= N) = epi(x[M, K] @ W[N, K]^T) at 1 <= M <= 64 rows: the decode-time projection
// past the skinny GEMM's 8 rows (gemm_rows.hip)
at::Tensor gemm_rows(const at::Tensor& x, const at::Tensor& W, int64_t epi, const c10::optional<at::Tensor>& bias,
                     const c10::optional<at::Tensor>& resid, int64_t ldy) {
  const ProjArgs p = proj_args("gemm_rows", x, W, epi, bias, resid, ldy);
  TORCH_CHECK(p.M <= 64 && mg::gemm_rows_supported((int)p.M, (int)p.K),
              "gemm_rows: 1 <= M <= 64, K % 8 == 0, K <= 8192");
  DevGuard g(x.device());
  auto y = at::empty({p.M, p.ldy}, x.options());
  mg::gemm_rows(bp(x), bp(W), bp(y), (int)p.M, (int)p.N, (int)p.K, p.ldy, p.bias, p.resid, (int)epi, cur_stream());
  return y;
}

// pos_dev (int32 [1] on the device, optional): the position is read by the kernel (hipGraph decode);
// with pos_stride 1 it is int32 [B], one position per row (ragged batches)
// part / counters (optional): the decode state's own workspace (kernels.h); without them a
// temporary pair is allocated for this call (tests; not for captured graphs)
// group = K > 1 (speculative decoding, kernels.h): K rows per cache row -- qkv_new [B * K, 3D], out
// [B * K, D], pos_dev int32 [B * K] with pos_stride 1 (row b * K holds the sequence's position), the
// workspace sized for B * K rows
at::Tensor attention_decode(const at::Tensor& qkv_new, const at::Tensor& cache, int64_t H,
                            int64_t pos, const c10::optional<at::Tensor>& pos_dev,
                            const c10::optional<at::Tensor>& part,
                            const c10::optional<at::Tensor>& counters, int64_t pos_stride, int64_t group) {
  CHECK_BF16(qkv_new); CHECK_BF16(cache); CHECK_CONTIG(qkv_new); CHECK_CONTIG(cache);
  TORCH_CHECK(cache.dim() == 3, "cache must be [B, Tmax, 3D]");
  TORCH_CHECK(group >= 1 && group <= mg::kSpecRowsMax, "attention_decode: group must be in 1..8");
  TORCH_CHECK(group == 1 || (pos_dev.has_value() && pos_stride == 1),
              "attention_decode: group > 1 needs pos_dev with pos_stride 1");
  const int64_t Bs = cache.size(0), B = Bs * group, Tmax = cache.size(1), D3 = cache.size(2), D = D3 / 3;
  TORCH_CHECK(qkv_new.numel() == B * D3 && D % H == 0, "attention_decode: shape mismatch");
  TORCH_CHECK(pos >= 0 && pos < Tmax && (D / H) % 8 == 0 && D / H <= 128, "attention_decode: pos / head dim");
  TORCH_CHECK(Tmax <= 4096, "attention_decode: KV cache longer than 4096 positions");
  DevGuard g(cache.device());
  auto out = at::empty({B, D}, cache.options());
  const int* pd = nullptr;
  if (pos_dev.has_value()) {
    TORCH_CHECK(pos_dev->scalar_type() == at::kInt && pos_dev->is_cuda(), "pos_dev must be int32 cuda");
    TORCH_CHECK((pos_stride == 0 || pos_stride == 1) && pos_dev->is_contiguous() &&
                pos_dev->numel() >= (pos_stride ? B : 1) && pos_dev->device() == cache.device(),
                "attention_decode: pos_dev int32 [1] (pos_stride 0) or [B] (pos_stride 1)");
    pd = pos_dev->data_ptr<int>();
  } else {
    TORCH_CHECK(pos_stride == 0, "attention_decode: pos_stride needs pos_dev");
  }
  const int64_t np = (int64_t)mg::attention_decode_part_floats((int)B, (int)H, (int)(D / H));
  at::Tensor pt, ct;
  if (part.has_value() && part->defined()) {
    TORCH_CHECK(counters.has_value() && counters->defined(), "attention_decode: part without counters");
    CHECK_F32(*part); CHECK_DEV(*counters);
    TORCH_CHECK(part->numel() >= np && part->device() == cache.device(), "attention_decode: part workspace too small");
    TORCH_CHECK(counters->scalar_type() == at::kInt && counters->numel() >= B * H &&
                counters->device() == cache.device(), "attention_decode: counters must be int32 [B * H]");
    pt = *part;
    ct = *counters;
  } else {
    pt = at::empty({np}, cache.options().dtype(at::kFloat));
    ct = at::zeros({B * H}, cache.options().dtype(at::kInt));
  }
  mg::attention_decode(bp(qkv_new), bp(cache), bp(out), (int)Bs, (int)H, (int)(D / H), Tmax, (int)pos,
                       cur_stream(), fp(pt), reinterpret_cast<unsigned*>(ct.data_ptr<int>()), pd,
                       (int)pos_stride, (int)group);
  return out;
}

// The int8 KV cache of one layer (kernels.h): kq int8 [B, 2, H, Tmax, hd], ks fp32 [B, 2, H, Tmax]
void kv8_cache_args(const char* op, const at::Tensor& kq, const at::Tensor& ks, int64_t B, int64_t H, int64_t hd) {
  CHECK_DEV(kq); CHECK_CONTIG(kq); CHECK_F32(ks); CHECK_CONTIG(ks);
  TORCH_CHECK(kq.scalar_type() == at::kChar, op, ": kq must be int8");
  TORCH_CHECK(kq.dim() == 5 && kq.size(0) == B && kq.size(1) == 2 && kq.size(2) == H && kq.size(4) == hd,
              op, ": kq must be [B, 2, H, Tmax, hd]");
  TORCH_CHECK(ks.dim() == 4 && ks.size(0) == B && ks.size(1) == 2 && ks.size(2) == H && ks.size(3) == kq.size(3),
              op, ": ks must be [B, 2, H, Tmax]");
  TORCH_CHECK(kq.device() == ks.device(), op, ": kq and ks on different devices");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(kq.data_ptr()) % 16 == 0, op, ": kq must be 16-byte aligned");
}

// Snap the K and V thirds of qkv [B, T, 3D] in place by the KV8 rule (common.h); with kq / ks also
// write the int8 cache's positions 0 .. T - 1; rep = W: the cache has B * rep rows, prompt b's go to rows
// b * rep .. b * rep + rep - 1 (the beam prefill)
void kv8_store(const at::Tensor& qkv, int64_t H, const c10::optional<at::Tensor>& kq,
               const c10::optional<at::Tensor>& ks, int64_t rep) {
  CHECK_BF16(qkv); CHECK_CONTIG(qkv);
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(2) % 3 == 0, "kv8_store: qkv must be [B, T, 3D]");
  const int64_t B = qkv.size(0), T = qkv.size(1), D = qkv.size(2) / 3;
  TORCH_CHECK(H >= 1 && D % H == 0 && (D / H) % 8 == 0 && D / H <= 128,
              "kv8_store: head dim must be a multiple of 8, at most 128");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, "kv8_store: qkv must be 16-byte aligned");
  const bool cache = kq.has_value() && kq->defined();
  TORCH_CHECK(cache == (ks.has_value() && ks->defined()), "kv8_store: kq and ks go together");
  TORCH_CHECK(rep >= 1 && rep <= mg::kBeamMax && (cache || rep == 1), "kv8_store: rep in 1..8, with kq / ks");
  int64_t Tmax = T;
  if (cache) {
    kv8_cache_args("kv8_store", *kq, *ks, B * rep, H, D / H);
    Tmax = kq->size(3);
    TORCH_CHECK(T <= Tmax && kq->device() == qkv.device(), "kv8_store: T exceeds the cache's Tmax");
  }
  if (B * T == 0) return;
  DevGuard g(qkv.device());
  mg::kv8_store(bp(qkv), cache ? kq->data_ptr<int8_t>() : nullptr, cache ? fp(*ks) : nullptr, (int)B, (int)T,
                (int)H, (int)(D / H), Tmax, cur_stream(), (int)rep);
}

// attention_decode on the int8 cache: pos / pos_dev / part / counters / pos_stride / group as there (group =
// K: kq / ks of B sequences, qkv_new [B * K, 3D], pos_dev int32 [B * K], the workspace for B * K rows)
at::Tensor attention_decode_kv8(const at::Tensor& qkv_new, const at::Tensor& kq, const at::Tensor& ks, int64_t H,
                                int64_t pos, const c10::optional<at::Tensor>& pos_dev,
                                const c10::optional<at::Tensor>& part, const c10::optional<at::Tensor>& counters,
                                int64_t pos_stride, int64_t group) {
  CHECK_BF16(qkv_new); CHECK_CONTIG(qkv_new);
  TORCH_CHECK(qkv_new.dim() == 2 && qkv_new.size(1) % 3 == 0, "attention_decode_kv8: qkv_new must be [B, 3D]");
  TORCH_CHECK(group >= 1 && group <= mg::kSpecRowsMax, "attention_decode_kv8: group must be in 1..8");
  TORCH_CHECK(group == 1 || (pos_dev.has_value() && pos_dev->defined() && pos_stride == 1),
              "attention_decode_kv8: group > 1 needs pos_dev with pos_stride 1");
  const int64_t B = qkv_new.size(0), D = qkv_new.size(1) / 3;
  TORCH_CHECK(B % group == 0, "attention_decode_kv8: qkv_new must hold group rows per sequence");
  TORCH_CHECK(B >= 1 && H >= 1 && D % H == 0 && (D / H) % 8 == 0 && D / H <= 128,
              "attention_decode_kv8: head dim must be a multiple of 8, at most 128");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv_new.data_ptr()) % 16 == 0,
              "attention_decode_kv8: qkv_new must be 16-byte aligned");
  const int64_t hd = D / H;
  kv8_cache_args("attention_decode_kv8", kq, ks, B / group, H, hd);
  TORCH_CHECK(kq.device() == qkv_new.device(), "attention_decode_kv8: the cache is on another device");
  const int64_t Tmax = kq.size(3);
  TORCH_CHECK(pos >= 0 && pos < Tmax, "attention_decode_kv8: pos outside the cache");
  TORCH_CHECK(Tmax <= 4096, "attention_decode_kv8: KV cache longer than 4096 positions");
  DevGuard g(qkv_new.device());
  auto out = at::empty({B, D}, qkv_new.options());
  const int* pd = nullptr;
  if (pos_dev.has_value() && pos_dev->defined()) {
    TORCH_CHECK(pos_dev->scalar_type() == at::kInt && pos_dev->is_cuda(), "pos_dev must be int32 cuda");
    TORCH_CHECK((pos_stride == 0 || pos_stride == 1) && pos_dev->is_contiguous() &&
                pos_dev->numel() >= (pos_stride ? B : 1) && pos_dev->device() == qkv_new.device(),
                "attention_decode_kv8: pos_dev int32 [1] (pos_stride 0) or [B] (pos_stride 1)");
    pd = pos_dev->data_ptr<int>();
  } else {
    TORCH_CHECK(pos_stride == 0, "attention_decode_kv8: pos_stride needs pos_dev");
  }
  const int64_t np = (int64_t)mg::attention_decode_part_floats((int)B, (int)H, (int)hd);
  at::Tensor pt, ct;
  if (part.has_value() && part->defined()) {
    TORCH_CHECK(counters.has_value() && counters->defined(), "attention_decode_kv8: part without counters");
    CHECK_F32(*part); CHECK_DEV(*counters); CHECK_CONTIG(*part); CHECK_CONTIG(*counters);
    TORCH_CHECK(part->numel() >= np && part->device() == qkv_new.device(),
                "attention_decode_kv8: part workspace too small");
    TORCH_CHECK(counters->scalar_type() == at::kInt && counters->numel() >= B * H &&
                counters->device() == qkv_new.device(), "attention_decode_kv8: counters must be int32 [B * H]");
    pt = *part;
    ct = *counters;
  } else {
    pt = at::empty({np}, qkv_new.options().dtype(at::kFloat));
    ct = at::zeros({B * H}, qkv_new.options().dtype(at::kInt));
  }
  mg::attention_decode_kv8(bp(qkv_new), kq.data_ptr<int8_t>(), fp(ks), bp(out), (int)(B / group), (int)H, (int)hd,
                           Tmax, (int)pos, cur_stream(), fp(pt), reinterpret_cast<unsigned*>(ct.data_ptr<int>()), pd,
                           (int)pos_stride, (int)group);
  return out;
}

// ------------------------------------------------------------------------------- logits-row ops
// The checks the one-workgroup-per-row ops (sample.hip, beam.hip) share, one per kind of argument.

// A contiguous int32 / fp32 device buffer of n elements on device dev, argument `name` of op `op`.
void dev_i32(const char* op, const char* name, const at::Tensor& t, int64_t n, const at::Device& dev) {
  TORCH_CHECK(t.scalar_type() == at::kInt && t.is_cuda() && t.is_contiguous() && t.numel() == n && t.device() == dev,
              op, ": ", name, " must be int32 with ", n, " elements on the operands' device");
}

void dev_f32(const char* op, const char* name, const at::Tensor& t, int64_t n, const at::Device& dev) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_cuda() && t.is_contiguous() && t.numel() == n && t.device() == dev,
              op, ": ", name, " must be float32 with ", n, " elements on the operands' device");
}

// The logits of op `op`: [rows, ld] bf16 with unit column stride, of which the kernel reads the
// first V columns of every row in 16-byte loads (columns >= V are padding, never read).  ld is the
// row stride in elements -- 0 for a single row, which has none to check.
struct LogitsRows {
  int64_t rows, ld;
  at::Device dev;
};

LogitsRows logits_rows(const char* op, const at::Tensor& logits, int64_t V) {
  CHECK_BF16(logits);
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) >= 1 && logits.stride(1) == 1, op,
              ": logits [rows, ld], unit column stride");
  const int64_t rows = logits.size(0), ld = rows > 1 ? logits.stride(0) : 0;
  TORCH_CHECK(V >= 1 && V <= logits.size(1) && (rows == 1 || ld >= logits.size(1)), op, ": 1 <= V <= ld");
  TORCH_CHECK(ld % 8 == 0 && reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0, op,
              ": rows must be 16-byte aligned (ld % 8 == 0)");
  return {rows, ld, logits.device()};
}

// The pick kernels' parameter block (kernels.h): int32 [8] on the logits' device.
uint32_t* sample_params(const char* op, const at::Tensor& params, const at::Device& dev) {
  CHECK_DEV(params);
  TORCH_CHECK(params.scalar_type() == at::kInt && params.is_contiguous() && params.numel() == mg::kSampleParamWords &&
              params.device() == dev, op, ": params int32 [8] on the logits' device");
  return reinterpret_cast<uint32_t*>(params.data_ptr<int>());
}

// The optional log-probability arguments of the pick kernels (kernels.h): lse fp32 with 2 B
// elements ({m, lnz} per row, from logits_lse on the same logits) and lp fp32 of seq's shape; both
// or neither.  Sets the two pointers (null without them).
void logprob_args(const char* op, const c10::optional<at::Tensor>& lse, const c10::optional<at::Tensor>& lp,
                  const LogitsRows& lr, const at::Tensor* seq, const float*& lsep, float*& lpp) {
  lsep = nullptr;
  lpp = nullptr;
  const bool has_lse = lse.has_value() && lse->defined(), has_lp = lp.has_value() && lp->defined();
  if (!has_lse && !has_lp) return;
  TORCH_CHECK(has_lse && has_lp && seq, op, ": lse and lp go together, with seq");
  dev_f32(op, "lse", *lse, 2 * lr.rows, lr.dev);
  dev_f32(op, "lp", *lp, seq->numel(), lr.dev);
  TORCH_CHECK(lp->sizes() == seq->sizes(), op, ": lp fp32 of seq's shape");
  lsep = lse->data_ptr<float>();
  lpp = lp->data_ptr<float>();
}

// One sampled token per row of logits [B, ld] bf16 (columns >= V are padding, never read): exact
// top-k + Gumbel-max (sample.hip, the rule in common.h).  params: int32 [8] on the device, {seed lo,
// seed hi, draw, inv_t fp32 bits, top_k (0: off), 0, top_p fp32 bits (0: off), 0}; the kernel advances params[2] and, when
// given, pos_dev[0] by one.  tok (int64, B elements) is written when given, else allocated; seq
// (int64 [B, L], needs pos_dev) gets seq[b, pos_dev[0] + 1].  lse / lp (optional, with seq): the
// drawn token's log-probability goes to lp[b, pos_dev[0] + 1] (logprob_args).  Returns tok.
at::Tensor sample_logits(const at::Tensor& logits, int64_t V, const at::Tensor& params,
                         const c10::optional<at::Tensor>& pos_dev, const c10::optional<at::Tensor>& tok,
                         const c10::optional<at::Tensor>& seq, const c10::optional<at::Tensor>& lse,
                         const c10::optional<at::Tensor>& lp) {
  const char* op = "sample_logits";
  const LogitsRows lr = logits_rows(op, logits, V);
  const int64_t B = lr.rows;
  uint32_t* pp = sample_params(op, params, lr.dev);
  int* pd = nullptr;
  if (pos_dev.has_value()) {
    dev_i32(op, "pos_dev", *pos_dev, 1, lr.dev);
    pd = pos_dev->data_ptr<int>();
  }
  DevGuard g(lr.dev);
  at::Tensor t;
  if (tok.has_value()) {
    CHECK_I64(*tok); CHECK_CONTIG(*tok);
    TORCH_CHECK(tok->numel() == B && tok->device() == lr.dev, "sample_logits: tok int64 with B elements");
    t = *tok;
  } else {
    t = at::empty({B}, logits.options().dtype(at::kLong));
  }
  int64_t* seqp = nullptr;
  long seq_ld = 0;
  if (seq.has_value()) {
    CHECK_I64(*seq); CHECK_CONTIG(*seq);
    TORCH_CHECK(pd && seq->dim() == 2 && seq->size(0) == B && seq->device() == lr.dev,
                "sample_logits: seq int64 [B, L] with pos_dev");
    seqp = seq->data_ptr<int64_t>();
    seq_ld = seq->size(1);
  }
  const float* lsep;
  float* lpp;
  logprob_args(op, lse, lp, lr, seq.has_value() ? &*seq : nullptr, lsep, lpp);
  mg::sample_logits(bp(logits), lr.ld, (int)B, (int)V, pp, pd, t.data_ptr<int64_t>(), seqp, seq_ld, cur_stream(),
                    lsep, lpp);
  return t;
}

// The kept set of the sampling rule per row of logits (as for sample_logits): int32 [B, 2], the bf16
// bit pattern of the lowest kept value and the number of kept entries under the block's top_k /
// top_p / temperature.  Runs the sampler's kernel up to its threshold; nothing but the result is
// written.
at::Tensor sample_kept(const at::Tensor& logits, int64_t V, const at::Tensor& params) {
  const LogitsRows lr = logits_rows("sample_kept", logits, V);
  const uint32_t* pp = sample_params("sample_kept", params, lr.dev);
  DevGuard g(lr.dev);
  at::Tensor out = at::empty({lr.rows, 2}, logits.options().dtype(at::kInt));
  mg::sample_kept(bp(logits), lr.ld, (int)lr.rows, (int)V, pp, out.data_ptr<int>(), cur_stream());
  return out;
}

// Ragged batches: the end of a decode step for every row that is not finished (kernels.h,
// pick_ragged).  logits [B, ld] bf16 as for sample_logits; params int32 [8] (word 5: the stop token,
// negative for none); pos, done int32 [B]; tok int64 with B elements; seq int64 [B, L].  All
// updated in place.  lse / lp (optional): the picked token's log-probability goes to
// lp[b, pos[b] + 1] of every row that advances (logprob_args).
void pick_ragged(const at::Tensor& logits, int64_t V, const at::Tensor& params, const at::Tensor& pos,
                 const at::Tensor& done, const at::Tensor& tok, const at::Tensor& seq, bool greedy,
                 const c10::optional<at::Tensor>& lse, const c10::optional<at::Tensor>& lp) {
  const char* op = "pick_ragged";
  const LogitsRows lr = logits_rows(op, logits, V);
  const int64_t B = lr.rows;
  uint32_t* pp = sample_params(op, params, lr.dev);
  dev_i32(op, "pos", pos, B, lr.dev);
  dev_i32(op, "done", done, B, lr.dev);
  CHECK_I64(tok); CHECK_CONTIG(tok); CHECK_I64(seq); CHECK_CONTIG(seq);
  TORCH_CHECK(tok.numel() == B && tok.device() == lr.dev, "pick_ragged: tok int64 with B elements");
  TORCH_CHECK(seq.dim() == 2 && seq.size(0) == B && seq.size(1) >= 2 && seq.device() == lr.dev,
              "pick_ragged: seq int64 [B, L]");
  const float* lsep;
  float* lpp;
  logprob_args(op, lse, lp, lr, &seq, lsep, lpp);
  DevGuard g(lr.dev);
  mg::pick_ragged(bp(logits), lr.ld, (int)B, (int)V, pp, pos.data_ptr<int>(), done.data_ptr<int>(),
                  tok.data_ptr<int64_t>(), seq.data_ptr<int64_t>(), seq.size(1), greedy, cur_stream(), lsep, lpp);
}

// Per-token log-probabilities of the rule in common.h for every row of logits [M, ld] bf16 (as for
// sample_logits: columns >= V never read).  Returns lse fp32 [M, 2] = {row maximum, lnz}; with
// targets (int64 [M] on the device) returns (lse, lp): lp fp32 [M], lp[r] = the log-probability of
// token targets[r] -- a negative target (or one >= V) leaves lp[r] as it is (0 in a buffer allocated
// here).  lse / lp: write into these instead of allocating.
py::object logits_lse(const at::Tensor& logits, int64_t V, const c10::optional<at::Tensor>& targets,
                      const c10::optional<at::Tensor>& lse, const c10::optional<at::Tensor>& lp) {
  const char* op = "logits_lse";
  const LogitsRows lr = logits_rows(op, logits, V);
  const int64_t M = lr.rows;
  TORCH_CHECK(M <= 0x7fffffff, "logits_lse: too many rows");
  DevGuard g(lr.dev);
  at::Tensor l, p;
  if (lse.has_value() && lse->defined()) {
    dev_f32(op, "lse", *lse, 2 * M, lr.dev);
    l = *lse;
  } else {
    l = at::empty({M, 2}, logits.options().dtype(at::kFloat));
  }
  const bool has_t = targets.has_value() && targets->defined();
  const int64_t* tp = nullptr;
  if (has_t) {
    CHECK_I64(*targets); CHECK_CONTIG(*targets);
    TORCH_CHECK(targets->numel() == M && targets->device() == lr.dev, "logits_lse: targets int64 [M]");
    tp = targets->data_ptr<int64_t>();
    if (lp.has_value() && lp->defined()) {
      dev_f32(op, "lp", *lp, M, lr.dev);
      p = *lp;
    } else {
      p = at::zeros({M}, logits.options().dtype(at::kFloat));
    }
  } else {
    TORCH_CHECK(!(lp.has_value() && lp->defined()), "logits_lse: lp needs targets");
  }
  mg::logits_lse(bp(logits), lr.ld, (int)M, (int)V, tp, fp(l), has_t ? fp(p) : nullptr, cur_stream());
  if (has_t) return py::make_tuple(l, p);
  return py::cast(l);
}

// The logits processors (process.hip, the rule in common.h) on logits [R, ld] bf16, in place: the
// first V columns of every row are edited from the row's history hist[r, 0 .. pos_r] (hist int64 [R,
// n] with unit column stride, n <= kProcHistMax; a view of a wider buffer is fine) under params (int32
// [kProcParamWords] on the device: rp, inv, pp, fp as fp32 bits, g, 0, 0, 0).  pos: int32 [1] with
// pos_stride 0 or [R] with pos_stride 1; done (optional): int32 [R], a finished row is left alone.
void logits_process(const at::Tensor& logits, int64_t V, const at::Tensor& hist, const at::Tensor& pos,
                    int64_t pos_stride, const c10::optional<at::Tensor>& done, const at::Tensor& params) {
  const char* op = "logits_process";
  const LogitsRows lr = logits_rows(op, logits, V);
  const int64_t R = lr.rows;
  TORCH_CHECK(R <= 0x7fffffff && V <= 0x7fffffff, op, ": too many rows or columns");
  CHECK_I64(hist); CHECK_DEV(hist);
  TORCH_CHECK(hist.dim() == 2 && hist.size(0) == R && hist.size(1) >= 1 && hist.stride(1) == 1 &&
              (R == 1 || hist.stride(0) >= hist.size(1)) && hist.device() == lr.dev,
              op, ": hist int64 [R, n] with unit column stride on the logits' device");
  TORCH_CHECK(hist.size(1) <= mg::kProcHistMax, op, ": at most ", mg::kProcHistMax, " history columns, got ",
              hist.size(1));
  TORCH_CHECK(pos_stride == 0 || pos_stride == 1, op, ": pos_stride 0 or 1");
  dev_i32(op, "pos", pos, pos_stride ? R : 1, lr.dev);
  const int* dp = nullptr;
  if (done.has_value() && done->defined()) {
    dev_i32(op, "done", *done, R, lr.dev);
    dp = done->data_ptr<int>();
  }
  CHECK_DEV(params);
  TORCH_CHECK(params.scalar_type() == at::kInt && params.is_contiguous() && params.numel() == mg::kProcParamWords &&
              params.device() == lr.dev, op, ": params int32 [8] on the logits' device");
  DevGuard g(lr.dev);
  mg::logits_process(bp(logits), lr.ld, (int)R, (int)V, hist.data_ptr<int64_t>(), R > 1 ? hist.stride(0) : 0,
                     (int)hist.size(1), pos.data_ptr<int>(), (int)pos_stride, dp,
                     reinterpret_cast<const uint32_t*>(params.data_ptr<int>()), cur_stream());
}

// ------------------------------------------------------------------------------- beam search
// beam.hip (kernels.h).  Every per-beam buffer has R = B * W elements, row b * W + w = beam w of
// prompt b; all of them live on the logits' / the cache's device and are updated in place.

// The row kernel on logits [R, ld] bf16 (columns >= V never read): writes cand_tok int32 [R, W],
// cand_c fp32 [R, W] and lse fp32 [R, 2] from score fp32 [R], fin int32 [R] and ctl int32 [4].
void beam_rows(const at::Tensor& logits, int64_t V, int64_t W, const at::Tensor& score, const at::Tensor& fin,
               const at::Tensor& ctl, const at::Tensor& cand_tok, const at::Tensor& cand_c, const at::Tensor& lse) {
  const LogitsRows lr = logits_rows("beam_rows", logits, V);
  const int64_t R = lr.rows;
  TORCH_CHECK(W >= 1 && W <= mg::kBeamMax && W <= V && R % W == 0 && R <= 0x7fffffff,
              "beam_rows: 1 <= W <= 8, W <= V, R a multiple of W");
  TORCH_CHECK(V <= (1 << 25), "beam_rows: V above 2^25 (a thread counts its elements in 16 bits)");
  const at::Device dev = lr.dev;
  dev_f32("beam_rows", "score", score, R, dev);
  dev_i32("beam_rows", "fin", fin, R, dev);
  dev_i32("beam_rows", "ctl", ctl, mg::kBeamCtlWords, dev);
  dev_i32("beam_rows", "cand_tok", cand_tok, R * W, dev);
  dev_f32("beam_rows", "cand_c", cand_c, R * W, dev);
  dev_f32("beam_rows", "lse", lse, 2 * R, dev);
  DevGuard g(dev);
  mg::beam_rows(bp(logits), lr.ld, (int)R, (int)V, (int)W, fp(score), fin.data_ptr<int>(), ctl.data_ptr<int>(),
                cand_tok.data_ptr<int>(), fp(cand_c), fp(lse), cur_stream());
}

// The merge kernel: cand_tok / cand_c [R, W] -> score, fin, len, tok (int64 [R]), parent and column
// ctl[0] of hist_parent / hist_tok (int32 [R, Lh]) / hist_score (fp32 [R, Lh]); pos int32 [1] advances.
void beam_merge(int64_t W, int64_t V, const at::Tensor& cand_tok, const at::Tensor& cand_c, const at::Tensor& score,
                const at::Tensor& fin, const at::Tensor& len, const at::Tensor& tok, const at::Tensor& parent,
                const at::Tensor& hist_parent, const at::Tensor& hist_tok, const at::Tensor& hist_score,
                const at::Tensor& pos, const at::Tensor& ctl) {
  CHECK_DEV(score);
  TORCH_CHECK(W >= 1 && W <= mg::kBeamMax && W <= V && V <= 0x7fffffff, "beam_merge: 1 <= W <= 8, W <= V");
  const int64_t R = score.numel();
  TORCH_CHECK(R >= W && R % W == 0 && R <= 0x7fffffff, "beam_merge: score with B * W elements");
  const at::Device dev = score.device();
  dev_f32("beam_merge", "score", score, R, dev);
  dev_i32("beam_merge", "cand_tok", cand_tok, R * W, dev);
  dev_f32("beam_merge", "cand_c", cand_c, R * W, dev);
  dev_i32("beam_merge", "fin", fin, R, dev);
  dev_i32("beam_merge", "len", len, R, dev);
  dev_i32("beam_merge", "parent", parent, R, dev);
  CHECK_I64(tok); CHECK_CONTIG(tok);
  TORCH_CHECK(tok.numel() == R && tok.device() == dev, "beam_merge: tok int64 with B * W elements");
  TORCH_CHECK(hist_parent.dim() >= 2 && hist_parent.size(-1) >= 1, "beam_merge: histories [B, W, Lh]");
  const int64_t Lh = hist_parent.size(-1);
  dev_i32("beam_merge", "hist_parent", hist_parent, R * Lh, dev);
  dev_i32("beam_merge", "hist_tok", hist_tok, R * Lh, dev);
  dev_f32("beam_merge", "hist_score", hist_score, R * Lh, dev);
  dev_i32("beam_merge", "pos", pos, 1, dev);
  dev_i32("beam_merge", "ctl", ctl, mg::kBeamCtlWords, dev);
  DevGuard g(dev);
  mg::beam_merge((int)(R / W), (int)W, (int)V, cand_tok.data_ptr<int>(), fp(cand_c), fp(score), fin.data_ptr<int>(),
                 len.data_ptr<int>(), tok.data_ptr<int64_t>(), parent.data_ptr<int>(), hist_parent.data_ptr<int>(),
                 hist_tok.data_ptr<int>(), fp(hist_score), Lh, pos.data_ptr<int>(), ctl.data_ptr<int>(), cur_stream());
}

// The cache reorder on kv [L, R, Tmax, 3 D] bf16 (one layer: [1, R, Tmax, 3 D]; layers may be a
// strided stack of contiguous [R, Tmax, 3 D] blocks), parent int32 [R], pos int32 [1]: rows t < pos.
// ctl (optional): its history column advances.
void beam_reorder(const at::Tensor& kv, int64_t W, const at::Tensor& parent, const at::Tensor& pos,
                  const c10::optional<at::Tensor>& ctl) {
  CHECK_BF16(kv);
  TORCH_CHECK(kv.dim() == 4 && kv.size(0) >= 1 && kv[0].is_contiguous() && kv.size(3) % 3 == 0,
              "beam_reorder: kv [L, R, Tmax, 3 D], every layer contiguous");
  const int64_t L = kv.size(0), R = kv.size(1), Tmax = kv.size(2), D = kv.size(3) / 3;
  const int64_t ls = L > 1 ? kv.stride(0) : 0;
  TORCH_CHECK(W >= 1 && W <= mg::kBeamMax && R >= W && R % W == 0, "beam_reorder: 1 <= W <= 8, R a multiple of W");
  TORCH_CHECK(D >= 8 && D % 8 == 0 && reinterpret_cast<uintptr_t>(kv.data_ptr()) % 16 == 0 && ls % 8 == 0 && ls >= 0,
              "beam_reorder: D % 8 == 0 and 16-byte aligned layers");
  TORCH_CHECK(Tmax >= 1 && Tmax * (D / 4) <= 0x7fffffff - 256 && R / W <= 65535 && L <= 65535,
              "beam_reorder: cache too large for one launch");
  const at::Device dev = kv.device();
  dev_i32("beam_reorder", "parent", parent, R, dev);
  dev_i32("beam_reorder", "pos", pos, 1, dev);
  int* cp = nullptr;
  if (ctl.has_value() && ctl->defined()) {
    dev_i32("beam_reorder", "ctl", *ctl, mg::kBeamCtlWords, dev);
    cp = ctl->data_ptr<int>();
  }
  DevGuard g(dev);
  mg::beam_reorder(bp(kv), (int)L, ls, (int)(R / W), (int)W, (int)Tmax, (int)D, parent.data_ptr<int>(),
                   pos.data_ptr<int>(), cp, cur_stream());
}

// The cache reorder on kq int8 [L, R, 2, H, Tmax, hd] and ks fp32 [L, R, 2, H, Tmax] (one layer: L = 1;
// layers may be a strided stack of contiguous blocks), parent int32 [R], pos int32 [1]: positions t < pos.
// ctl (optional): its history column advances.
void beam_reorder_kv8(const at::Tensor& kq, const at::Tensor& ks, int64_t W, const at::Tensor& parent,
                      const at::Tensor& pos, const c10::optional<at::Tensor>& ctl) {
  CHECK_DEV(kq); CHECK_F32(ks);
  TORCH_CHECK(kq.scalar_type() == at::kChar, "beam_reorder_kv8: kq must be int8");
  TORCH_CHECK(kq.dim() == 6 && kq.size(0) >= 1 && kq[0].is_contiguous() && kq.size(2) == 2,
              "beam_reorder_kv8: kq [L, R, 2, H, Tmax, hd], every layer contiguous");
  const int64_t L = kq.size(0), R = kq.size(1), H = kq.size(3), Tmax = kq.size(4), hd = kq.size(5);
  TORCH_CHECK(ks.dim() == 5 && ks.size(0) == L && ks.size(1) == R && ks.size(2) == 2 && ks.size(3) == H &&
              ks.size(4) == Tmax && ks[0].is_contiguous() && ks.device() == kq.device(),
              "beam_reorder_kv8: ks must be [L, R, 2, H, Tmax] beside kq, every layer contiguous");
  const int64_t lq = L > 1 ? kq.stride(0) : 0, lsc = L > 1 ? ks.stride(0) : 0;
  TORCH_CHECK(W >= 1 && W <= mg::kBeamMax && R >= W && R % W == 0,
              "beam_reorder_kv8: 1 <= W <= 8, R a multiple of W");
  TORCH_CHECK(H >= 1 && hd >= 8 && hd % 8 == 0 && hd <= 128 &&
              reinterpret_cast<uintptr_t>(kq.data_ptr()) % 16 == 0 && lq % 16 == 0 && lq >= 0 &&
              reinterpret_cast<uintptr_t>(ks.data_ptr()) % 4 == 0 && lsc >= 0,
              "beam_reorder_kv8: hd % 8 == 0, at most 128, and 16-byte aligned layers");
  TORCH_CHECK(Tmax >= 1 && 2 * H * Tmax * (hd / 8 + 1) <= 0x7fffffff - 256 && R / W <= 65535 && L <= 65535,
              "beam_reorder_kv8: cache too large for one launch");
  const at::Device dev = kq.device();
  dev_i32("beam_reorder_kv8", "parent", parent, R, dev);
  dev_i32("beam_reorder_kv8", "pos", pos, 1, dev);
  int* cp = nullptr;
  if (ctl.has_value() && ctl->defined()) {
    dev_i32("beam_reorder_kv8", "ctl", *ctl, mg::kBeamCtlWords, dev);
    cp = ctl->data_ptr<int>();
  }
  DevGuard g(dev);
  mg::beam_reorder_kv8(kq.data_ptr<int8_t>(), fp(ks), (int)L, lq, lsc, (int)(R / W), (int)W, (int)H, (int)Tmax,
                       (int)hd, parent.data_ptr<int>(), pos.data_ptr<int>(), cp, cur_stream());
}

// ------------------------------------------------------------------------------- speculative decoding
// spec.hip (kernels.h).  B sequences, K rows each; every buffer lives on seq's / the logits' device and
// is updated in place.

// seq int64 [B, L] with 1 <= L < 2^31 and 2 <= K <= 8: B, the device.
int64_t spec_seq(const char* op, const at::Tensor& seq, int64_t K) {
  CHECK_I64(seq); CHECK_CONTIG(seq); CHECK_DEV(seq);
  TORCH_CHECK(seq.dim() == 2 && seq.size(0) >= 1 && seq.size(1) >= 1 && seq.size(1) <= 0x7fffffff, op,
              ": seq int64 [B, L]");
  TORCH_CHECK(K >= 2 && K <= mg::kSpecRowsMax, op, ": K must be in 2..8");
  return seq.size(0);
}

// The draft kernel: seq int64 [B, L], pos int32 [B], ctl int32 [4] -> tok int64 [B * K], pos_rows
// int32 [B * K], has_draft int32 [B].
void spec_draft(const at::Tensor& seq, const at::Tensor& pos, const at::Tensor& ctl, int64_t K, const at::Tensor& tok,
                const at::Tensor& pos_rows, const at::Tensor& has_draft) {
  const char* op = "spec_draft";
  const int64_t B = spec_seq(op, seq, K);
  const at::Device dev = seq.device();
  dev_i32(op, "pos", pos, B, dev);
  dev_i32(op, "ctl", ctl, mg::kSpecCtlWords, dev);
  dev_i32(op, "pos_rows", pos_rows, B * K, dev);
  dev_i32(op, "has_draft", has_draft, B, dev);
  CHECK_I64(tok); CHECK_CONTIG(tok);
  TORCH_CHECK(tok.numel() == B * K && tok.device() == dev, op, ": tok int64 with B * K elements");
  DevGuard g(dev);
  mg::spec_draft(seq.data_ptr<int64_t>(), seq.size(1), (int)B, (int)K, pos.data_ptr<int>(), ctl.data_ptr<int>(),
                 tok.data_ptr<int64_t>(), pos_rows.data_ptr<int>(), has_draft.data_ptr<int>(), cur_stream());
}

// The row argmax: g int32 [R] (written when given, else allocated) of logits [R, ld] bf16.
at::Tensor spec_argmax(const at::Tensor& logits, int64_t V, const c10::optional<at::Tensor>& g) {
  const char* op = "spec_argmax";
  const LogitsRows lr = logits_rows(op, logits, V);
  TORCH_CHECK(lr.rows <= 0x7fffffff && V <= 0x7fffffff, op, ": too many rows");
  DevGuard guard(lr.dev);
  at::Tensor out;
  if (g.has_value() && g->defined()) {
    dev_i32(op, "g", *g, lr.rows, lr.dev);
    out = *g;
  } else {
    out = at::empty({lr.rows}, logits.options().dtype(at::kInt));
  }
  mg::spec_argmax(bp(logits), lr.ld, (int)lr.rows, (int)V, out.data_ptr<int>(), cur_stream());
  return out;
}

// The accept kernel: g int32 [B * K], tok int64 [B * K], has_draft int32 [B] -> seq int64 [B, L], pos,
// steps int32 [B], hist int32 [B, K + 1].
void spec_accept(const at::Tensor& g, const at::Tensor& tok, const at::Tensor& has_draft, int64_t K,
                 const at::Tensor& pos, const at::Tensor& ctl, const at::Tensor& seq, const at::Tensor& steps,
                 const at::Tensor& hist) {
  const char* op = "spec_accept";
  const int64_t B = spec_seq(op, seq, K);
  const at::Device dev = seq.device();
  dev_i32(op, "g", g, B * K, dev);
  dev_i32(op, "has_draft", has_draft, B, dev);
  dev_i32(op, "pos", pos, B, dev);
  dev_i32(op, "ctl", ctl, mg::kSpecCtlWords, dev);
  dev_i32(op, "steps", steps, B, dev);
  dev_i32(op, "hist", hist, B * (K + 1), dev);
  CHECK_I64(tok); CHECK_CONTIG(tok);
  TORCH_CHECK(tok.numel() == B * K && tok.device() == dev, op, ": tok int64 with B * K elements");
  DevGuard guard(dev);
  mg::spec_accept(g.data_ptr<int>(), tok.data_ptr<int64_t>(), has_draft.data_ptr<int>(), (int)B, (int)K,
                  pos.data_ptr<int>(), ctl.data_ptr<int>(), seq.data_ptr<int64_t>(), seq.size(1), steps.data_ptr<int>(),
                  hist.data_ptr<int>(), cur_stream());
}

// ------------------------------------------------------------------------------- native RCCL
// csrc/comm/rccl_comm.cpp. Every collective runs on the communicator's comm stream after the
// tensor's device's CURRENT stream (the producers); comm_wait makes that stream wait again.
mg::comm::DType comm_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return mg::comm::DType::F32;
    case at::kBFloat16: return mg::comm::DType::BF16;
    case at::kHalf: return mg::comm::DType::F16;
    case at::kLong: return mg::comm::DType::I64;
    case at::kByte: return mg::comm::DType::U8;
    default: TORCH_CHECK(false, "comm: unsupported dtype ", t.scalar_type());
  }
}

hipStream_t comm_cs(int64_t h, const at::Tensor& t) {
  CHECK_DEV(t);
  CHECK_CONTIG(t);
  TORCH_CHECK(t.device().index() == mg::comm::device(h), "comm: tensor on device ", t.device().index(),
              ", communicator on device ", mg::comm::device(h));
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

int64_t comm_all_reduce(int64_t h, const at::Tensor& t) {
  hipStream_t cs = comm_cs(h, t);
  return mg::comm::all_reduce(h, t.data_ptr(), (size_t)t.numel(), comm_dtype(t), cs);
}

int64_t comm_reduce_scatter(int64_t h, const at::Tensor& in, const at::Tensor& out) {
  hipStream_t cs = comm_cs(h, in);
  comm_cs(h, out);
  TORCH_CHECK(in.scalar_type() == out.scalar_type(), "comm_reduce_scatter: dtype mismatch");
  TORCH_CHECK(in.numel() == out.numel() * mg::comm::nranks(h), "comm_reduce_scatter: input must hold nranks x output");
  return mg::comm::reduce_scatter(h, in.data_ptr(), out.data_ptr(), (size_t)out.numel(), comm_dtype(in), cs);
}

int64_t comm_all_gather(int64_t h, const at::Tensor& in, const at::Tensor& out) {
  hipStream_t cs = comm_cs(h, in);
  comm_cs(h, out);
  TORCH_CHECK(in.scalar_type() == out.scalar_type(), "comm_all_gather: dtype mismatch");
  TORCH_CHECK(out.numel() == in.numel() * mg::comm::nranks(h), "comm_all_gather: output must hold nranks x input");
  return mg::comm::all_gather(h, in.data_ptr(), out.data_ptr(), (size_t)in.numel(), comm_dtype(in), cs);
}

int64_t comm_broadcast(int64_t h, const at::Tensor& t, int64_t root) {
  hipStream_t cs = comm_cs(h, t);
  TORCH_CHECK(root >= 0 && root < mg::comm::nranks(h), "comm_broadcast: bad root");
  return mg::comm::broadcast(h, t.data_ptr(), (size_t)t.numel(), comm_dtype(t), (int)root, cs);
}

void comm_wait(int64_t h, int64_t ticket) {
  const int d = mg::comm::device(h);
  mg::comm::wait(h, ticket, c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(d).stream());
}

}  // namespace


PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("comm_load", [](const std::string& path) {
    mg::comm::load_rccl(path);
    return (int64_t)mg::comm::rccl_version();
  }, py::arg("path") = std::string());
  m.def("comm_unique_id", []() { return py::bytes(mg::comm::unique_id()); });
  m.def("comm_create", [](const py::bytes& uid, int64_t nranks, int64_t rank, int64_t device) {
    return mg::comm::create(std::string(uid), (int)nranks, (int)rank, (int)device);
  });
  m.def("comm_destroy", &mg::comm::destroy);
  m.def("comm_stream_ptr", [](int64_t h) { return (int64_t)(intptr_t)mg::comm::comm_stream(h); });
  m.def("comm_all_reduce", &comm_all_reduce);
  m.def("comm_reduce_scatter", &comm_reduce_scatter);
  m.def("comm_all_gather", &comm_all_gather);
  m.def("comm_broadcast", &comm_broadcast);
  m.def("comm_wait", &comm_wait);
  m.def("comm_pending", &mg::comm::pending);
  m.def("comm_retire", &mg::comm::retire);
  m.def("comm_query", &mg::comm::query);
  m.doc() = "mingpt_distributed_amd gfx950 kernels";
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd_plain);
  m.def("layernorm_bwd_dropout", &layernorm_bwd, py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("mean"),
        py::arg("rstd"), py::arg("dw"), py::arg("db"), py::arg("dres"), py::arg("dz_bias"),
        py::arg("drop_p"), py::arg("drop_seed"));
  // read-only: the number of blocks layernorm_bwd launches (tests pick M past the capped grid with it)
  m.def("layernorm_bwd_grid", &mg::ln_bwd_grid, py::arg("M"), py::arg("D"), py::arg("drop"));
  m.def("embedding_fwd", &embedding_fwd, py::arg("idx"), py::arg("wte"), py::arg("wpe"), py::arg("p"),
        py::arg("seed"), py::arg("pos_dev") = py::none(), py::arg("am_part") = py::none(),
        py::arg("seq") = py::none(), py::arg("pos_stride") = 0);
  // debug builds: OR of the device error words (1/2 = token id out of range in embedding fwd/bwd,
  // 4 = cross-entropy target >= V), cleared on read; always 0 in release builds
  m.def("debug_error_bits", []() -> int64_t { return (int64_t)mg::debug_error_bits(); });
  m.def("debug_build", []() {
#ifdef MG_DEBUG
    return true;
#else
    return false;
#endif
  });
  m.def("embedding_bwd", &embedding_bwd);
  m.def("xent_fwd", &xent_fwd);
  m.def("xent_bwd", &xent_bwd);
  m.def("xent_fused", &xent_fused);
  m.def("xent_scale_", &xent_scale_);
  m.def("set_graph_state", &set_graph_state, py::arg("seed_ofs") = py::none(), py::arg("opt_hp") = py::none());
  m.def("grad_sumsq", &grad_sumsq);
  m.def("grad_sumsq_chunks", &grad_sumsq_chunks);
  m.def("adamw_step", &adamw_step, py::arg("chunk_start"), py::arg("chunk_len"), py::arg("chunk_wd"),
        py::arg("moment_start"), py::arg("master"), py::arg("param"), py::arg("grad"), py::arg("m"),
        py::arg("v"), py::arg("norm"), py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("step"), py::arg("grad_scale"), py::arg("clip"), py::arg("table_end"),
        py::arg("moment_end"), py::arg("zero_grad") = py::none());
  m.def("f32_to_bf16", &f32_to_bf16);
  m.def("comm_proxy", &comm_proxy);
  m.def("bias_act", &bias_act);
  m.def("bias_dropout_residual", &bias_dropout_residual);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("dropout_bwd", &dropout_bwd);
  m.def("transpose", &transpose);
  m.def("bias_grad", &bias_grad);
  m.def("dropout_bias_grad", &dropout_bias_grad);
  m.def("gemm", &gemm, py::arg("a"), py::arg("b"), py::arg("c"), py::arg("layout"), py::arg("epi"),
        py::arg("bias"), py::arg("aux"), py::arg("resid"), py::arg("p"), py::arg("seed"), py::arg("M"),
        py::arg("N"), py::arg("dbias") = py::none());
  m.def("gemm_set_variant", &mg::gemm_set_variant);
  m.def("gemm_get_variant", &mg::gemm_get_variant);
  m.def("gemm_pick", &mg::gemm_pick, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("layout"));
  m.def("attention_set_bwd_mode", &mg::attention_set_bwd_mode);
  m.def("attention_set_bwd64", &mg::attention_set_bwd64);
#ifdef MG_BWD64_STAMPS
  m.def("attention_bwd64_stamps", []() {
    auto t = at::empty({64 * 4 * 8 * 8 + 64 * 4 * 16}, at::kLong);
    mg::attention_bwd64_stamps(reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>()));
    return t;
  });
#endif
  m.def("attention_fwd", &attention_fwd);
  m.def("attention_bwd", &attention_bwd, py::arg("qkv"), py::arg("out"), py::arg("dout"), py::arg("lse"),
        py::arg("mask"), py::arg("B"), py::arg("T"), py::arg("H"), py::arg("p"), py::arg("seed"),
        py::arg("dbias") = py::none());
  m.def("gemv", &gemv, py::arg("x"), py::arg("W"), py::arg("epi"), py::arg("bias") = py::none(),
        py::arg("resid") = py::none(), py::arg("ldy") = 0, py::arg("lnw") = py::none(),
        py::arg("lnb") = py::none(), py::arg("eps") = 1e-5, py::arg("am_part") = py::none(),
        py::arg("am_pos") = py::none());
  m.def("gemv_argmax_groups", [](int64_t N, int64_t B) { return (int64_t)mg::gemv_grid((int)N, (int)B); },
        py::arg("N"), py::arg("B"));
  m.def("gemv_supported", &mg::gemv_supported);
  m.def("gemv_w8", &gemv_w8, py::arg("x"), py::arg("Wq"), py::arg("scale"), py::arg("epi"),
        py::arg("bias") = py::none(), py::arg("resid") = py::none(), py::arg("ldy") = 0, py::arg("lnw") = py::none(),
        py::arg("lnb") = py::none(), py::arg("eps") = 1e-5, py::arg("am_part") = py::none(),
        py::arg("am_pos") = py::none());
  m.def("gemv_w8_supported", &mg::gemv_w8_supported);
  m.def("gemm_rows", &gemm_rows, py::arg("x"), py::arg("W"), py::arg("epi"), py::arg("bias") = py::none(),
        py::arg("resid") = py::none(), py::arg("ldy") = 0);
  m.def("gemm_rows_supported", &mg::gemm_rows_supported);
  m.def("attention_decode", &attention_decode, py::arg("qkv_new"), py::arg("cache"), py::arg("H"),
        py::arg("pos"), py::arg("pos_dev") = py::none(), py::arg("part") = py::none(),
        py::arg("counters") = py::none(), py::arg("pos_stride") = 0, py::arg("group") = 1);
  m.def("kv8_store", &kv8_store, py::arg("qkv"), py::arg("H"), py::arg("kq") = py::none(),
        py::arg("ks") = py::none(), py::arg("rep") = 1);
  m.def("attention_decode_kv8", &attention_decode_kv8, py::arg("qkv_new"), py::arg("kq"), py::arg("ks"),
        py::arg("H"), py::arg("pos"), py::arg("pos_dev") = py::none(), py::arg("part") = py::none(),
        py::arg("counters") = py::none(), py::arg("pos_stride") = 0, py::arg("group") = 1);
  m.def("sample_logits", &sample_logits, py::arg("logits"), py::arg("V"), py::arg("params"),
        py::arg("pos_dev") = py::none(), py::arg("tok") = py::none(), py::arg("seq") = py::none(),
        py::arg("lse") = py::none(), py::arg("lp") = py::none());
  m.def("sample_kept", &sample_kept, py::arg("logits"), py::arg("V"), py::arg("params"));
  m.def("pick_ragged", &pick_ragged, py::arg("logits"), py::arg("V"), py::arg("params"), py::arg("pos"),
        py::arg("done"), py::arg("tok"), py::arg("seq"), py::arg("greedy"), py::arg("lse") = py::none(),
        py::arg("lp") = py::none());
  m.def("logits_lse", &logits_lse, py::arg("logits"), py::arg("V"), py::arg("targets") = py::none(),
        py::arg("lse") = py::none(), py::arg("lp") = py::none());
  m.def("logits_process", &logits_process, py::arg("logits"), py::arg("V"), py::arg("hist"), py::arg("pos"),
        py::arg("pos_stride"), py::arg("done"), py::arg("params"));
  m.attr("PROC_HIST_MAX") = (int64_t)mg::kProcHistMax;
  m.def("beam_rows", &beam_rows, py::arg("logits"), py::arg("V"), py::arg("W"), py::arg("score"), py::arg("fin"),
        py::arg("ctl"), py::arg("cand_tok"), py::arg("cand_c"), py::arg("lse"));
  m.def("beam_merge", &beam_merge, py::arg("W"), py::arg("V"), py::arg("cand_tok"), py::arg("cand_c"),
        py::arg("score"), py::arg("fin"), py::arg("len"), py::arg("tok"), py::arg("parent"), py::arg("hist_parent"),
        py::arg("hist_tok"), py::arg("hist_score"), py::arg("pos"), py::arg("ctl"));
  m.def("beam_reorder", &beam_reorder, py::arg("kv"), py::arg("W"), py::arg("parent"), py::arg("pos"),
        py::arg("ctl") = py::none());
  m.def("beam_reorder_kv8", &beam_reorder_kv8, py::arg("kq"), py::arg("ks"), py::arg("W"), py::arg("parent"),
        py::arg("pos"), py::arg("ctl") = py::none());
  m.def("spec_draft", &spec_draft, py::arg("seq"), py::arg("pos"), py::arg("ctl"), py::arg("K"), py::arg("tok"),
        py::arg("pos_rows"), py::arg("has_draft"));
  m.def("spec_argmax", &spec_argmax, py::arg("logits"), py::arg("V"), py::arg("g") = py::none());
  m.def("spec_accept", &spec_accept, py::arg("g"), py::arg("tok"), py::arg("has_draft"), py::arg("K"), py::arg("pos"),
        py::arg("ctl"), py::arg("seq"), py::arg("steps"), py::arg("hist"));
  m.def("attention_decode_part_floats", [](int64_t B, int64_t H, int64_t hd) {
    return (int64_t)mg::attention_decode_part_floats((int)B, (int)H, (int)hd);
  });
}
