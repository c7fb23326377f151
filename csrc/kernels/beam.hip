// Beam search on the device for gfx950: the three kernels that follow the LM head in a beam decode
// step (the rule in common.h, 'Beam search').  B prompts, W <= 8 beams each, R = B * W decode rows.
//
//   rows     one workgroup of 1024 threads per row, the row in registers as in sample.hip (Row,
//            row_common.h): {m, lnz} by the lse kernel's own row_max_mass, then the row's first W
//            entries in amax_key order -- every thread keeps its best key below the previous
//            winner, and only the thread that held the winner looks for its next one, so a round
//            costs one workgroup reduction -- written as W (token, c = s + lp) candidates.  A
//            finished row writes its one candidate (pad, s) and W - 1 empty ones.
//   merge    one wave per prompt ranks the W * W candidates (a count of the candidates that come
//            before each one), reads every old per-beam value, and after a barrier writes the new
//            beams: score, finished flag, length, the token the next step embeds, the parent, and
//            one column of the parent / token / score histories.
//   reorder  every layer's KV cache, in place: a thread owns one 16-byte chunk of the K / V columns
//            at (prompt, t), loads it from all W beams into registers and stores dst[r] =
//            src[parent[r]].  The permutation never leaves the thread: no second cache, no hand-off.
//
// Two device words move once per step, each in a launch none of whose workgroups reads it: the
// position `pos` (read by the decode step and the reorder) in the merge, the history column
// `ctl[0]` (read by the merge) in the reorder.  The stop token and the pad token are ctl[1], ctl[2],
// so one captured step serves every call.
#include "common.h"
#include "kernels.h"
#include "row_common.h"

using namespace mg;
using namespace mg::row;

namespace {

constexpr int kMergeThreads = 64;  // W * W <= 64 candidates, one per lane

__global__ __launch_bounds__(kThreads) void beam_row_kernel(const bf16_t* __restrict__ logits, long ld, int V, int W,
                                                            const float* __restrict__ score,
                                                            const int* __restrict__ fin, const int* __restrict__ ctl,
                                                            int* __restrict__ cand_tok, float* __restrict__ cand_c,
                                                            float* __restrict__ lse) {
  __shared__ float redf[kWaves];
  __shared__ unsigned long long redq[kWaves];
  __shared__ unsigned long long redk[2][kWaves];
  const long r = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const Row rw(logits + r * ld, V);
  const int nv = V >> 3, ti = nv * 8 + (int)threadIdx.x;
  // A thread ranks its own elements by a 32-bit key: the bf16 bits in amax_key's order (key16's, but
  // -0 stays below +0) above the inverted count e of the element within the thread (e grows with the
  // column: 8 j + c for column c of the thread's j-th vector, 0xffff for the tail element), so the
  // thread's maximum is its entry that comes first in amax_key order.  Only a thread's best is
  // widened to the 64-bit key.
  static_assert(kThreads == 1024, "the element count below takes the vector stride as 1 << 10");
  auto lkey = [&](int i, uint32_t bits) -> uint32_t {
    const uint32_t o = (bits & 0x8000u) ? (bits ^ 0xffffu) : (bits | 0x8000u);
    const uint32_t e = i >= nv * 8 ? 0xffffu : (uint32_t)(((((i >> 3) - (int)threadIdx.x) >> 10) << 3) | (i & 7));
    return (o << 16) | (0xffffu - e);
  };
  auto gkey = [&](uint32_t lk) -> unsigned long long {
    if (!lk) return 0ull;
    const uint32_t e = 0xffffu - (lk & 0xffffu);
    const int i = e == 0xffffu ? ti : ((((int)threadIdx.x + (int)(e >> 3) * kThreads) << 3) | (int)(e & 7u));
    return amax_key(bf2f(key16_bits(lk >> 16)), i);
  };
  // {m, lnz}: the lse kernel's (the thread's best key rides along in the first sweep)
  float m;
  unsigned long long z;
  uint32_t mine_l = 0u;
  row_max_mass(rw, redf, redq, m, z, [&](int i, uint32_t bits) {
    const uint32_t k = lkey(i, bits);
    mine_l = k > mine_l ? k : mine_l;
  });
  unsigned long long mine = gkey(mine_l);
  float lnz = 0.f;  // thread 0's: it writes the candidates
  if (threadIdx.x == 0) {
    lnz = logprob_lnz(z);
    lse[2 * r] = m;
    lse[2 * r + 1] = lnz;
  }
  const float s = score[r];
  if (fin[r]) {  // the whole workgroup: the frozen beam's one candidate, then W - 1 empty ones
    if ((int)threadIdx.x < W) {
      cand_tok[r * W + threadIdx.x] = threadIdx.x == 0 ? ctl[2] : -1;
      cand_c[r * W + threadIdx.x] = threadIdx.x == 0 ? s : -INFINITY;
    }
    return;
  }
  // the row's first W entries in amax_key order.  Keys are unique (the index is in them): after a
  // round only the thread that held the winner has lost its best key below it.
  unsigned long long prev = ~0ull;
  for (int k = 0; k < W; ++k) {
    if (k > 0 && mine == prev) {
      uint32_t nxt = 0u;
      rw.sweep([&](int i, uint32_t bits) {
        const uint32_t key = lkey(i, bits);
        nxt = (key < mine_l && key > nxt) ? key : nxt;
      });
      mine_l = nxt;
      mine = gkey(nxt);
    }
    unsigned long long best = wave_max_key(mine);
    // two buffers: a wave writes round k + 2 only after every wave has passed round k + 1's barrier,
    // i.e. has read round k
    if (lane == 0) redk[k & 1][wv] = best;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kWaves; ++i) best = redk[k & 1][i] > best ? redk[k & 1][i] : best;
    prev = best;
    if (threadIdx.x == 0) {
      // no entry left (never with W <= V) is still a valid id; the entry's bf16 bits are the top 16
      // of the key (amax_key undone): no dependent load of row[t]
      cand_tok[r * W + k] = (int)key_token(best, V);
      cand_c[r * W + k] = s + token_logprob(key16_bits((uint32_t)(best >> 48)), m, lnz);
    }
  }
}

// candidate a comes before candidate b (indices qa, qb = beam * W + rank in the beam's row): a real
// candidate before an empty one, the higher c (float compare: -0 == +0), then the lower index
MG_DEVICE bool beam_before(int va, float ca, int qa, int vb, float cb, int qb) {
  if (va != vb) return va > vb;
  if (ca != cb) return ca > cb;
  return qa < qb;
}

__global__ __launch_bounds__(kMergeThreads) void beam_merge_kernel(
    int W, int V, const int* __restrict__ cand_tok, const float* __restrict__ cand_c, float* __restrict__ score,
    int* __restrict__ fin, int* __restrict__ len, int64_t* __restrict__ tok, int* __restrict__ parent,
    int* __restrict__ hist_parent, int* __restrict__ hist_tok, float* __restrict__ hist_score, long hist_ld,
    int* pos, const int* __restrict__ ctl, unsigned* err) {
  __shared__ float sc[kMergeThreads];
  __shared__ int sv[kMergeThreads];
  const int b = blockIdx.x, j = threadIdx.x, n = W * W;
  const bool has = j < n;
  const int w = has ? j / W : 0;
  const long col = ctl[0];
  const int eos = ctl[1], pad = ctl[2];
  int t = -1, pfin = 0, plen = 0;
  float c = -INFINITY;
  if (has) {
    t = cand_tok[(long)b * n + j];
    c = cand_c[(long)b * n + j];
    if (c != c) c = -INFINITY;  // outside the rule (a row without a finite maximum): ranks last
    pfin = fin[b * W + w];
    plen = len[b * W + w];
  }
  const int valid = t >= 0;
  sc[j] = c;
  sv[j] = valid;
  __syncthreads();  // every old per-beam value has been read: the new ones may be written
  if (has) {
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += (q != j && beam_before(sv[q], sc[q], q, valid, c, j)) ? 1 : 0;
    if (rank < W) {
      MG_CHECK_INDEX(t, t >= 0 && t < V, pad, err, 8u);
      if (t < 0 || t >= V) t = 0;  // never embedded out of range, whatever came in
      const long o = (long)b * W + rank;
      score[o] = c;
      fin[o] = (pfin || (eos >= 0 && t == eos)) ? 1 : 0;
      len[o] = plen + (pfin ? 0 : 1);
      tok[o] = t;
      parent[o] = w;
      if (col >= 0 && col < hist_ld) {
        hist_parent[o * hist_ld + col] = w;
        hist_tok[o * hist_ld + col] = t;
        hist_score[o * hist_ld + col] = c;
      }
    }
  }
  if (b == 0 && j == 0) pos[0] += 1;  // nobody in this launch reads it
}

// kv [L, B * W, Tmax, 3 D]: rows t < *pos of the K / V columns (D .. 3 D) of prompt blockIdx.y in
// layer blockIdx.z.  A prompt whose parents are the identity returns at once (uniform per workgroup).
template <int W>
__global__ __launch_bounds__(256) void beam_reorder_kernel(bf16_t* __restrict__ kv, long layer_stride, int Tmax, int D,
                                                           const int* __restrict__ parent,
                                                           const int* __restrict__ pos, int* ctl, unsigned* err) {
  if (ctl && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) ctl[0] += 1;
  const int b = blockIdx.y;
  int par[W];
  bool ident = true;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    int p = parent[b * W + r];
    MG_CHECK_INDEX(p, p >= 0 && p < W, r, err, 16u);
    if (p < 0 || p >= W) p = r;
    par[r] = p;
    ident = ident && p == r;
  }
#ifndef MG_BEAM_NO_IDENT_SKIP  // A/B switch (MG_EXTRA_FLAGS): what the skip buys, PERF.md
  if (ident) return;
#endif
  int n = pos[0];
  n = n < Tmax ? n : Tmax;
  const int chunks = D >> 2;  // 16-byte chunks in the 2 D bf16 of K and V
  const int idx = blockIdx.x * 256 + (int)threadIdx.x;
  const int t = idx / chunks, ch = idx - t * chunks;
  if (t >= n) return;
  const long beam_stride = (long)Tmax * 3 * D;
  bf16_t* base = kv + blockIdx.z * layer_stride + (long)b * W * beam_stride + (long)t * 3 * D + D + ch * 8;
  uint4 v[W];
#pragma unroll
  for (int r = 0; r < W; ++r) v[r] = ld16(base + r * beam_stride);
#pragma unroll
  for (int r = 0; r < W; ++r) {
    // uniform branches over constant register indices (a select chain on v[] is turned into an
    // indexed private array); a beam that keeps its own rows stores nothing
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if (q != r && par[r] == q) st16(base + r * beam_stride, v[q]);
    }
  }
}

}  // namespace

namespace mg {

void beam_rows(const bf16_t* logits, long ld, int R, int V, int W, const float* score, const int* fin, const int* ctl,
               int* cand_tok, float* cand_c, float* lse, hipStream_t stream) {
  beam_row_kernel<<<R, kThreads, 0, stream>>>(logits, ld, V, W, score, fin, ctl, cand_tok, cand_c, lse);
}

void beam_merge(int B, int W, int V, const int* cand_tok, const float* cand_c, float* score, int* fin, int* len,
                int64_t* tok, int* parent, int* hist_parent, int* hist_tok, float* hist_score, long hist_ld, int* pos,
                const int* ctl, hipStream_t stream) {
  beam_merge_kernel<<<B, kMergeThreads, 0, stream>>>(W, V, cand_tok, cand_c, score, fin, len, tok, parent,
                                                     hist_parent, hist_tok, hist_score, hist_ld, pos, ctl,
                                                     debug_err_word());
}

void beam_reorder(bf16_t* kv, int L, long layer_stride, int B, int W, int Tmax, int D, const int* parent,
                  const int* pos, int* ctl, hipStream_t stream) {
  const dim3 grid(cdiv((long)Tmax * (D >> 2), 256), B, L);
#define MG_BEAM_REORDER(w) \
  case w: beam_reorder_kernel<w><<<grid, 256, 0, stream>>>(kv, layer_stride, Tmax, D, parent, pos, ctl, debug_err_word()); break;
  switch (W) {
    MG_BEAM_REORDER(1) MG_BEAM_REORDER(2) MG_BEAM_REORDER(3) MG_BEAM_REORDER(4)
    MG_BEAM_REORDER(5) MG_BEAM_REORDER(6) MG_BEAM_REORDER(7) MG_BEAM_REORDER(8)
    default: break;  // the binding admits 1 .. 8
  }
#undef MG_BEAM_REORDER
}

}  // namespace mg
