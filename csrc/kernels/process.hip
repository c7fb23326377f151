// Logits processors for gfx950: repetition / presence / frequency penalties and the no-repeat n-gram
// ban, applied in place to the bf16 logits the LM head wrote, inside the captured decode step (the
// rule in common.h, 'Logits processors').
//
// Other stacks run these on the host between the model and the sampler: one round trip per token and
// no graph replay.  Here the step's own kernels keep the token history in device memory (the seq
// buffer the pick kernels write), the position is read on the device and the settings come from a
// device parameter block, so one captured launch serves every value.
//
// One workgroup of 1024 threads per row.  The history (at most kProcHistMax ids) is staged once in
// LDS as int32, ids outside [0, V) as -1.  Thread t owns the history slots t, t + 1024, ...:
//   penalties  the counts c_i come from an open-addressing table in LDS (a power of two of at least 2 n
//              slots, so at most half full): the owner of a slot inserts its token with a compare-
//              and-swap on the key and adds 1 to the slot's count.  Integer adds: the counts do not
//              depend on the order of the inserts.  After a barrier the threads walk the table, and
//              the thread that finds a key rewrites that logit -- a token has one table slot, so one
//              writer per element, at most n of the V entries touched, O(n) work.  (Every owner
//              comparing its token with the whole staged history, 16 bytes per LDS read, was measured
//              first: 32 us per launch at n = 1024 and 465 us at n = 4096, against 2.8 us at n = 32;
//              PERF.md.)
//   n-gram     after a workgroup barrier (which also orders the global stores: a ban lands after the
//              penalty on the same element), the owner of slot t compares the g - 1 ids before it with
//              the history's last g - 1 and stores the -inf pattern to the logit of h[t] on a match.
//              Duplicate stores carry the same value.
// Nothing but the first V columns of the row is written, and nothing is kept between launches.
#include "common.h"
#include "kernels.h"
#include "row_common.h"

using namespace mg;
using namespace mg::row;

namespace {

constexpr int kSlots = kProcHistMax / kThreads;
static_assert(kSlots * kThreads == kProcHistMax, "every history slot has an owner");
constexpr int kTable = 2 * kProcHistMax;  // slots of the count table: a power of two, never more than half full
static_assert((kTable & (kTable - 1)) == 0, "the table index is a mask");

__global__ __launch_bounds__(kThreads) void process_kernel(bf16_t* __restrict__ logits, long ld, int V,
                                                           const int64_t* __restrict__ hist, long hist_ld,
                                                           int hist_n, const int* __restrict__ pos, int pos_stride,
                                                           const int* __restrict__ done,
                                                           const uint32_t* __restrict__ params, unsigned* err) {
  __shared__ int h[kProcHistMax];
  __shared__ int key[kTable];
  __shared__ int cnt[kTable];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (done && done[r]) return;  // the whole workgroup: a finished row changes nothing
  const int p = pos[pos_stride ? r : 0];
  if (p < 0) return;
  const int n = p + 1 < hist_n ? p + 1 : hist_n;  // hist_n <= kProcHistMax (the launcher)
  const float rp = __uint_as_float(params[0]), inv = __uint_as_float(params[1]);
  const float pp = __uint_as_float(params[2]), fp = __uint_as_float(params[3]);
  int g = (int)params[4];
  g = g < 0 ? 0 : (g > kProcNgramMax ? kProcNgramMax : g);
  bf16_t* row = logits + (long)r * ld;
  const int64_t* hr = hist + (long)r * hist_ld;

  // ---- stage the history and clear the table: 2^lg slots, 2 n <= 2^lg <= kTable
  int lg = 6;
  while ((1 << lg) < 2 * n) ++lg;
  const int size = 1 << lg;
  for (int i = tid; i < size; i += kThreads) {
    key[i] = -1;
    cnt[i] = 0;
  }
  for (int i = tid; i < n; i += kThreads) {
    long t = hr[i];
    MG_CHECK_INDEX(t, (unsigned long)t < (unsigned long)V, -1, err, 32u)
    h[i] = (unsigned long)t < (unsigned long)V ? (int)t : -1;
  }
  __syncthreads();

  // ---- penalties: count every token in the table ...
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    const int j = tid + k * kThreads;
    const int t = j < n ? h[j] : -1;
    if (t < 0) continue;
    int s = (int)(((uint32_t)t * 0x9E3779B1u) >> (32 - lg));
    for (int probe = 0; probe < size; ++probe) {  // ends at a free slot or the token's own: the table is never full
      const int old = atomicCAS(&key[s], -1, t);
      if (old == -1 || old == t) {
        atomicAdd(&cnt[s], 1);
        break;
      }
      s = (s + 1) & (size - 1);
    }
  }
  __syncthreads();
  // ... and rewrite the logit of every key once
  for (int i = tid; i < size; i += kThreads) {
    const int t = key[i];
    if (t < 0) continue;
    const uint32_t bits = row[t];
    if (bits != 0xff80u) row[t] = proc_penalty(bits, cnt[i], rp, inv, pp, fp);  // -inf stays -inf
  }
  if (g < 1 || n < g) return;  // uniform
  __syncthreads();             // every penalty store is done before any ban store

  // ---- no-repeat n-gram: slot t is banned when the g - 1 ids before it are the last g - 1
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    const int t = tid + k * kThreads;
    if (t < g - 1 || t >= n) continue;
    bool ok = true;
    for (int j = 0; j < g - 1; ++j) {
      const int a = h[t - 1 - j];
      ok = ok && a >= 0 && a == h[n - 1 - j];
    }
    const int tok = h[t];
    if (ok && tok >= 0) row[tok] = (bf16_t)0xff80u;
  }
}

}  // namespace

namespace mg {

void logits_process(bf16_t* logits, long ld, int R, int V, const int64_t* hist, long hist_ld, int hist_n,
                    const int* pos, int pos_stride, const int* done, const uint32_t* params, hipStream_t stream) {
  if (hist_n > kProcHistMax) hist_n = kProcHistMax;
  process_kernel<<<R, kThreads, 0, stream>>>(logits, ld, V, hist, hist_ld, hist_n, pos, pos_stride, done, params,
                                             debug_err_word());
}

}  // namespace mg
