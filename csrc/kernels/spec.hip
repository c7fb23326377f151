// Speculative greedy decoding on the device for gfx950: the kernels around the K-row verify step
// (the rule in common.h, 'Speculative greedy decoding').  B sequences, K = draft_len + 1 <= 8 rows
// each, row b * K + r = row r of sequence b.
//
//   draft    one workgroup per sequence: the threads scan the candidate ends e < p in parallel, each
//            with at most ngram compares against the committed suffix, the workgroup max-reduces the
//            key (ml << 32) | e, and one thread walks the self-extension (at most K - 1 serial
//            reads) and writes the K input tokens, their positions and the "has a draft" flag.
//   argmax   one workgroup of 1024 threads per logits row (Row, row_common.h): the ragged greedy
//            pick's own ranking -- amax_key over the stored bf16 logits, first index on ties --
//            written as g[row].
//   accept   one wave per sequence applies the accept rule to the sequence's K picks: the emitted
//            tokens go to seq, the position advances by their count, the statistics are bumped.
//
// Each kernel's inputs were written by an earlier launch and nothing one workgroup writes is read
// by another of the same launch: the launch boundary is the only hand-off, there are no atomics.
// ngram and end live in the control block ctl (device, 4 x int32: {ngram, end, 0, 0}), so one
// captured step serves any max_new_tokens and any ngram.
#include "common.h"
#include "kernels.h"
#include "row_common.h"

using namespace mg;
using namespace mg::row;

namespace {

constexpr int kDraftThreads = 256;
constexpr int kDraftWaves = kDraftThreads / 64;

__global__ __launch_bounds__(kDraftThreads) void spec_draft_kernel(const int64_t* __restrict__ seq, long seq_ld,
                                                                   const int* __restrict__ pos,
                                                                   const int* __restrict__ ctl, int K,
                                                                   int64_t* __restrict__ tok,
                                                                   int* __restrict__ pos_rows,
                                                                   int* __restrict__ has_draft) {
  __shared__ unsigned long long redk[kDraftWaves];
  const int b = blockIdx.x;
  const int64_t* s = seq + (long)b * seq_ld;
  const int p = min(max(pos[b], 0), (int)seq_ld - 1);
  const int ngram = min(max(ctl[0], 1), kSpecNgramMax);
  // the committed suffix s[p], s[p - 1], ... (entries before the sequence's start are never compared)
  int64_t suf[kSpecNgramMax];
#pragma unroll
  for (int j = 0; j < kSpecNgramMax; ++j) suf[j] = s[max(p - j, 0)];
  unsigned long long best = 0ull;  // ml = 0: no candidate
  for (int e = threadIdx.x; e < p; e += kDraftThreads) {
    int ml = 0;
#pragma unroll
    for (int j = 0; j < kSpecNgramMax; ++j) {
      if (j < ngram && ml == j && e - j >= 0 && s[max(e - j, 0)] == suf[j]) ml = j + 1;
    }
    const unsigned long long k = ((unsigned long long)ml << 32) | (uint32_t)e;
    best = (ml && k > best) ? k : best;
  }
  best = wave_max_key(best);
  if ((threadIdx.x & 63) == 0) redk[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 1; i < kDraftWaves; ++i) best = redk[i] > best ? redk[i] : best;
  const bool has = (best >> 32) != 0ull;
  const int e = (int)(uint32_t)best;
  int64_t d[kSpecRowsMax];  // d[r] = x[p + r], x the committed tokens extended by the draft itself
#pragma unroll
  for (int r = 0; r < kSpecRowsMax; ++r) d[r] = s[p];  // without a draft every row carries s[p]
  if (has) {
#pragma unroll
    for (int r = 1; r < kSpecRowsMax; ++r) {
      if (r < K) {
        const int i = e + r;  // <= p + r - 1: committed, or an earlier draft token
        int64_t v = s[min(i, p)];
#pragma unroll
        for (int q = 1; q < r; ++q) v = (i - p == q) ? d[q] : v;  // constant register indices
        d[r] = v;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kSpecRowsMax; ++r) {
    if (r < K) {
      tok[(long)b * K + r] = d[r];
      pos_rows[(long)b * K + r] = p + r;
    }
  }
  has_draft[b] = has ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void spec_argmax_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                               int* __restrict__ g) {
  __shared__ unsigned long long redk[kWaves];
  const long r = blockIdx.x;
  unsigned long long best = 0ull;
  Row(logits + r * ld, V).sweep([&](int i, uint32_t bits) {
    const unsigned long long k = amax_key(bf2f(bits), i);
    best = k > best ? k : best;
  });
  best = block_max_key(best, redk);
  if (threadIdx.x == 0) g[r] = (int)key_token(best, V);
}

__global__ __launch_bounds__(64) void spec_accept_kernel(const int* __restrict__ g, const int64_t* __restrict__ tok,
                                                         const int* __restrict__ has_draft, int K, int* pos,
                                                         const int* __restrict__ ctl, int64_t* __restrict__ seq,
                                                         long seq_ld, int* steps, int* hist) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int p = pos[b];
  const int end = min(ctl[1], (int)seq_ld - 1);
  if (p < 0 || p >= end) return;  // the whole wave: a finished sequence changes nothing
  const bool row = lane < K;
  const int gr = row ? g[(long)b * K + lane] : 0;
  const int gprev = __shfl_up(gr, 1, 64);
  const bool ok = row && lane >= 1 && has_draft[b] != 0 && tok[(long)b * K + lane] == (int64_t)gprev;
  // bit r - 1 of m: draft r confirmed; the accepted count is the run of ones from bit 0 (bit K - 1 is 0)
  const unsigned long long m = __ballot(ok) >> 1;
  const int a = __builtin_ctzll(~m);
  const int cnt = min(a + 1, end - p);
  if (lane < cnt) seq[(long)b * seq_ld + p + 1 + lane] = gr;
  if (lane == 0) {
    pos[b] = p + cnt;
    steps[b] += 1;
    hist[(long)b * (K + 1) + cnt] += 1;
  }
}

}  // namespace

namespace mg {

void spec_draft(const int64_t* seq, long seq_ld, int B, int K, const int* pos, const int* ctl, int64_t* tok,
                int* pos_rows, int* has_draft, hipStream_t stream) {
  spec_draft_kernel<<<B, kDraftThreads, 0, stream>>>(seq, seq_ld, pos, ctl, K, tok, pos_rows, has_draft);
}

void spec_argmax(const bf16_t* logits, long ld, int R, int V, int* g, hipStream_t stream) {
  spec_argmax_kernel<<<R, kThreads, 0, stream>>>(logits, ld, V, g);
}

void spec_accept(const int* g, const int64_t* tok, const int* has_draft, int B, int K, int* pos, const int* ctl,
                 int64_t* seq, long seq_ld, int* steps, int* hist, hipStream_t stream) {
  spec_accept_kernel<<<B, 64, 0, stream>>>(g, tok, has_draft, K, pos, ctl, seq, seq_ld, steps, hist);
}

}  // namespace mg
