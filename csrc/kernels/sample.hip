// Sampled decode for gfx950: exact top-k + Gumbel-max sampling of one token per logits row.
//
// Replaces the reference's per-token host sequence (/root/reference/mingpt/model.py:341-352:
// divide by the temperature, torch.topk, masked fill, softmax, torch.multinomial) with one kernel
// that reads the bf16 logits the LM head wrote and leaves the token in device memory, so a decode
// step needs nothing from the host.  The rule (common.h, 'Gumbel-max sampling') is counter-based:
// the token depends on (seed, draw, row, logits) only -- not on the block size, the reduction
// order, or whether the launch is replayed from a hipGraph.
//
// One workgroup of 1024 threads per row; the row (100 KB at V = 50257) is loaded once into
// registers (Row, row_common.h; rows past 65536 columns are streamed by every pass instead):
//   pass A  row maximum, and (top-k on) a 256-bin histogram of the high byte of the 16-bit key;
//   pass B  (top-k on) histogram of the low byte among the keys in the bin that holds the k-th;
//           -> the exact k-th largest key, ties included, no sort and no tolerance;
//   nucleus (top_p on) the same two-level select with 64-bit integer masses in place of counts,
//           over the elements top-k kept: the lowest key whose mass strictly above is below
//           ceil(top_p * Z); the final threshold is the larger of the two keys;
//   pass C  score (l - max) * inv_t + gumbel of every kept element, argmax as one 64-bit key
//           (ordered score << 32 | ~index: the lowest index wins an exact tie).
// Histograms are kept 32 times over (one copy per lane mod 32, the copy picks the LDS bank):
// logits of one row share a few exponents, and 64 lanes adding to one LDS word serialise.  The mass
// histograms reuse the same 32 KiB as 256 x 16 copies of 64 bits; integer adds commute, so the
// threshold is a function of the row's values alone.
//
// Everything that changes between generate() calls is read from a device parameter block (and the
// position from pos_dev), so a captured launch replays with a new seed, temperature or k.  The
// draw counter and the position advance in a one-thread kernel launched after the sampler: the
// stream order is the "every row has read them" guarantee, with no cross-workgroup hand-off.
//
// Ragged batches (pick_ragged): every row has its own position, draw counter (position + 1) and
// finished flag in device memory, read and written by the row's own workgroup only -- the sampler
// in its RAGGED form or the greedy pick kernel, both ending in ragged_finish.  No advance kernel.
//
// Log-probabilities (logits_lse; the rule in common.h, 'Per-token log-probabilities'): one more
// one-workgroup-per-row kernel over the same row in registers -- the maximum, then the 64-bit
// integer sum of the sampler's own masses at temperature 1 by wave shuffle and LDS (row_max_mass)
// -- leaves {m, lnz} per row, and with targets the log-probability of one given token per row
// (score).  The pick kernels take that pair and write the picked token's log-probability beside the
// token, under the conditions of the token's own store.
//
// The row itself (Row and its sweeps), key16 and its inverse, key_token, the workgroup reductions
// and row_max_mass live in row_common.h, shared with beam.hip; amax_key in common.h.
#include "common.h"
#include "kernels.h"
#include "row_common.h"

using namespace mg;
using namespace mg::row;

namespace {

constexpr int kCopies = 32;
constexpr int kMassCopies = kCopies / 2;  // 64-bit bins in the same array

MG_DEVICE uint32_t ordered_f32(float s) {
  if (s == 0.f) s = 0.f;  // -0 -> +0
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

MG_DEVICE unsigned long long shfl_up_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_up((unsigned)v, o, 64), hi = __shfl_up((unsigned)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

MG_DEVICE void hist_clear(uint32_t* hist) {
  for (int i = threadIdx.x; i < 256 * kCopies; i += kThreads) hist[i] = 0u;
}

// The bin (counted from the top) in which the cumulative count reaches `want`, and how many of
// that bin's elements are still wanted.  hist: 256 x kCopies counts; scan: kWaves + 2 words.
// Needs 1 <= want <= sum of all counts.  Result broadcast to the block.
MG_DEVICE void hist_select(const uint32_t* hist, uint32_t* scan, uint32_t want, uint32_t& bin, uint32_t& rest) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  __syncthreads();  // the histogram is complete
  uint32_t c = 0u;
  if (t < 256) {  // thread t owns bin 255 - t; rotated start: the copies of one bin share no bank
#pragma unroll 8
    for (int j = 0; j < kCopies; ++j) c += hist[(255 - t) * kCopies + ((j + t) & (kCopies - 1))];
  }
  uint32_t inc = c;  // inclusive scan over descending bins
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (t < 256 && lane == 63) scan[w] = inc;
  __syncthreads();
  if (t < 256) {
    uint32_t before = inc - c;
    for (int i = 0; i < w; ++i) before += scan[i];
    if (before < want && want <= before + c) {  // exactly one thread
      scan[kWaves] = 255u - (uint32_t)t;
      scan[kWaves + 1] = want - before;
    }
  }
  __syncthreads();
  bin = scan[kWaves];
  rest = scan[kWaves + 1];
  __syncthreads();  // scan and hist may be rewritten
}

// hist_select on masses.  hist: 256 x kMassCopies 64-bit sums; scan: 6 words.  The bin (counted
// from the top) in which the cumulative mass reaches want = target(sum of all bins), and how much of
// that bin's mass is still wanted; bin 0 and rest 0 when there is no such bin (want = 0 or above
// the sum).  Result broadcast to the block.
template <class T>
MG_DEVICE void mass_select(const unsigned long long* hist, unsigned long long* scan, T target, uint32_t& bin,
                           unsigned long long& rest) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  __syncthreads();  // the histogram is complete
  unsigned long long c = 0ull;
  if (t < 256) {
#pragma unroll 8
    for (int j = 0; j < kMassCopies; ++j) c += hist[(255 - t) * kMassCopies + ((j + t) & (kMassCopies - 1))];
  }
  unsigned long long inc = c;  // inclusive scan over descending bins
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long v = shfl_up_u64(inc, o);
    if (lane >= o) inc += v;
  }
  if (t < 256 && lane == 63) scan[w] = inc;
  if (t == 0) scan[4] = scan[5] = 0ull;
  __syncthreads();
  if (t < 256) {
    const unsigned long long want = target(scan[0] + scan[1] + scan[2] + scan[3]);
    unsigned long long before = inc - c;
    for (int i = 0; i < w; ++i) before += scan[i];
    if (before < want && want <= before + c) {  // at most one thread
      scan[4] = 255ull - (unsigned long long)t;
      scan[5] = want - before;
    }
  }
  __syncthreads();
  bin = (uint32_t)scan[4];
  rest = scan[5];
  __syncthreads();  // scan and hist may be rewritten
}

// Ragged decode: the end of row b's step, by one thread of the row's own workgroup.  p is the
// row's position as the workgroup read it (pos[b]); the picked token t goes to tok[b] and
// seq[b, p + 1], the position moves on, and the row is finished once t is the stop token
// (params[5], negative: none).  Nobody else reads or writes pos[b], done[b], tok[b] or row b of
// seq in this launch, so there is no hand-off and no trailing advance kernel.  The position never
// reaches seq_ld - 1 = Tmax (the cache's and wpe's row count): a row that would is left as it is.
// lp (optional, laid out as seq) gets the token's log-probability where seq gets the token: lse =
// {m, lnz} of every row (logits_lse), row = the logits of row b.
MG_DEVICE void ragged_finish(long t, int b, int p, int eos, int* pos, int* done, int64_t* tok, int64_t* seq,
                             long seq_ld, const bf16_t* row, const float* lse, float* lp) {
  if (p < 0 || (long)p + 1 >= seq_ld - 1) return;
  tok[b] = t;
  seq[(long)b * seq_ld + p + 1] = t;
  if (lp) lp[(long)b * seq_ld + p + 1] = token_logprob(row[t], lse[2 * b], lse[2 * b + 1]);
  pos[b] = p + 1;
  if (eos >= 0 && t == (long)eos) done[b] = 1;
}

// params: {seed_lo, seed_hi, draw, inv_t (fp32 bits), top_k (<= 0: off), eos (ragged),
//          top_p (fp32 bits; 0 or >= 1.0: off), 0}
// RAGGED: per-row state -- the draw counter is pos_dev[b] + 1 (the column of the produced token in
// the row's own sequence), a row whose done[b] is set is skipped, and ragged_finish ends the row.
// KEPT (sample_kept): the same thresholds, then instead of the Gumbel pass the kept set itself --
// kept_out[2 b] = the bf16 bits of the lowest kept value (-inf when nothing is kept),
// kept_out[2 b + 1] = the number of kept entries; nothing else is written.
// lse, lp (optional, together; lp needs seq): the drawn token's log-probability goes to lp where the
// token goes to seq.
template <bool RAGGED, bool KEPT>
__global__ __launch_bounds__(kThreads) void sample_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                          const uint32_t* params, int* pos_dev, int* done,
                                                          int64_t* __restrict__ tok, int64_t* __restrict__ seq,
                                                          long seq_ld, int* __restrict__ kept_out,
                                                          const float* __restrict__ lse, float* __restrict__ lp) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[256 * kCopies];  // or 256 x kMassCopies x 64 bits
  __shared__ uint32_t scan[kWaves + 2];
  __shared__ unsigned long long mscan[6];
  __shared__ float redf[kWaves];
  __shared__ unsigned long long redk[kWaves];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bf16_t* row = logits + (long)b * ld;
  int rpos = 0;
  if constexpr (RAGGED) {
    if (done[b]) return;  // the whole workgroup: a finished row changes nothing
    rpos = pos_dev[b];
  }
  const uint32_t seed_lo = params[0], seed_hi = params[1], draw = RAGGED ? (uint32_t)(rpos + 1) : params[2];
  const float inv_t = __uint_as_float(params[3]);
  const int top_k = (int)params[4];
  const bool select = top_k > 0 && top_k < V;  // k >= V keeps every element
  const uint32_t top_p = params[6];
  const bool nucleus = top_p - 1u < 0x3f7fffffu;  // fp32 bits of a value in (0, 1)

  const Row rw(row, V);  // in registers when it fits
  const int nv = V >> 3, ti = nv * 8 + (int)threadIdx.x;

  // ---- pass A: row maximum (+ high-byte histogram)
  uint32_t* my = hist + (lane & (kCopies - 1));
  if (select) hist_clear(hist);
  __syncthreads();
  float m = -INFINITY;
  if (select) {
    rw.sweep([&](int, uint32_t bits) {
      m = fmaxf(m, bf2f(bits));
      atomicAdd(my + (key16(bits) >> 8) * kCopies, 1u);
    });
  } else {
    rw.sweep([&](int, uint32_t bits) { m = fmaxf(m, bf2f(bits)); });
  }
  m = block_max<kWaves>(m, redf);

  // ---- pass B: the exact k-th largest key
  uint32_t thr = 0u;
  if (select) {
    uint32_t hi, rest, lo, unused;
    hist_select(hist, scan, (uint32_t)top_k, hi, rest);
    hist_clear(hist);
    __syncthreads();
    rw.sweep([&](int, uint32_t bits) {
      const uint32_t k = key16(bits);
      if ((k >> 8) == hi) atomicAdd(my + (k & 0xffu) * kCopies, 1u);
    });
    hist_select(hist, scan, rest, lo, unused);
    thr = (hi << 8) | lo;
  }

  // A row in registers whose threshold keeps a few elements per thread: mark them in a sweep over
  // the registers (bit 8 j + e = element e of register j), then visit the marked ones one by one
  // -- one copy of an expensive body (the ~100 instructions of Gumbel noise) in the code, not one
  // per register element.  The body checks the threshold itself (the tail is always visited).
  auto mark = [&](uint32_t t) {
    unsigned long long kept = 0ull;
#pragma unroll
    for (int j = 0; j < kRegVec; ++j) {
      if ((int)threadIdx.x + j * kThreads < nv)
        for_vec(rw.regs[j], j * 8, [&](int e, uint32_t bits) { kept |= key16(bits) >= t ? 1ull << e : 0ull; });
    }
    return kept;
  };
  auto for_marked = [&](unsigned long long kept, auto f) {
    while (kept) {
      const int e = __builtin_ctzll(kept);
      kept &= kept - 1ull;
      const int i = (((int)threadIdx.x + (e >> 3) * kThreads) << 3) + (e & 7);
      f(i, (uint32_t)row[i]);
    }
    if (threadIdx.x < 8 && ti < V) f(ti, rw.tail);
  };

  // ---- nucleus: the lowest key whose mass strictly above is below ceil(top_p * Z), by the same
  // two-level select on integer masses (common.h); only what top-k kept carries mass
  if (nucleus) {
    unsigned long long* mhist = reinterpret_cast<unsigned long long*>(hist);
    unsigned long long* mine = mhist + (lane & (kMassCopies - 1));
    const bool few = select && rw.cached;
    const unsigned long long kept = few ? mark(thr) : 0ull;
    auto pass = [&](auto f) {
      if (few) for_marked(kept, f);
      else rw.sweep(f);
    };
    uint32_t hi, lo;
    unsigned long long rest, unused;
    hist_clear(hist);
    __syncthreads();
    pass([&](int, uint32_t bits) {
      const uint32_t k = key16(bits);
      if (k < thr || bits == 0xff80u) return;
      const unsigned long long q = sample_mass(bits, m, inv_t);
      if (q) atomicAdd(mine + (k >> 8) * kMassCopies, q);
    });
    mass_select(mhist, mscan, [&](unsigned long long Z) { return sample_nucleus_target(top_p, Z); }, hi, rest);
    hist_clear(hist);
    __syncthreads();
    pass([&](int, uint32_t bits) {
      const uint32_t k = key16(bits);
      if ((k >> 8) != hi || k < thr || bits == 0xff80u) return;
      const unsigned long long q = sample_mass(bits, m, inv_t);
      if (q) atomicAdd(mine + (k & 0xffu) * kMassCopies, q);
    });
    mass_select(mhist, mscan, [&](unsigned long long) { return rest; }, lo, unused);
    const uint32_t pt = (hi << 8) | lo;
    thr = pt > thr ? pt : thr;
  }

  if constexpr (KEPT) {  // the kept set itself: its lowest value and its size
    uint32_t cnt = 0u, lowest = 0xffffffffu;
    rw.sweep([&](int, uint32_t bits) {
      const uint32_t k = key16(bits);
      if (k < thr || bits == 0xff80u) return;
      ++cnt;
      lowest = k < lowest ? k : lowest;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      const uint32_t k = __shfl_xor(lowest, o, 64);
      lowest = k < lowest ? k : lowest;
    }
    if (lane == 0) {
      scan[w] = cnt;
      redk[w] = lowest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 1; i < kWaves; ++i) {
        cnt += scan[i];
        lowest = (uint32_t)redk[i] < lowest ? (uint32_t)redk[i] : lowest;
      }
      kept_out[2 * b] = cnt ? (int)key16_bits(lowest) : 0xff80;
      kept_out[2 * b + 1] = (int)cnt;
    }
    return;
  }

  // ---- pass C: Gumbel-max over the kept set
  const uint32_t r0 = fmix32(seed_lo ^ kSampleSalt);
  const uint32_t r1 = fmix32(r0 + seed_hi);
  const uint32_t r2 = fmix32(r1 + draw);
  const uint32_t r3 = fmix32(r2 ^ (uint32_t)b);
  unsigned long long best = 0ull;
  auto score = [&](int i, uint32_t bits) {
    if (key16(bits) < thr || bits == 0xff80u) return;  // below the threshold, or -inf
    const float s = (bf2f(bits) - m) * inv_t + sample_gumbel(r3, (uint32_t)i);
    const unsigned long long k = ((unsigned long long)ordered_f32(s) << 32) | (0xffffffffu - (uint32_t)i);
    best = k > best ? k : best;
  };
  if ((select || nucleus) && rw.cached) {  // top-k and the nucleus keep a few elements per row
    for_marked(mark(thr), score);
  } else {
    for_row(row, V, score);
  }
  best = block_max_key(best, redk);
  if (threadIdx.x == 0) {
    const long t = key_token(best, V);
    if constexpr (RAGGED) {
      ragged_finish(t, b, rpos, (int)params[5], pos_dev, done, tok, seq, seq_ld, row, lse, lp);
    } else {
      if (tok) tok[b] = t;
      if (seq) {
        const long p = (long)pos_dev[0] + 1;
        if (p >= 0 && p < seq_ld) {
          seq[(long)b * seq_ld + p] = t;
          if (lp) lp[(long)b * seq_ld + p] = token_logprob(row[t], lse[2 * b], lse[2 * b + 1]);
        }
      }
    }
  }
}

// Ragged greedy pick: one workgroup per logits row, the argmax over the first V bf16 columns
// (16-byte loads, first index on ties), then ragged_finish (lse, lp: as for the sampler).
__global__ __launch_bounds__(kThreads) void pick_greedy_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                               const uint32_t* params, int* pos, int* done,
                                                               int64_t* __restrict__ tok,
                                                               int64_t* __restrict__ seq, long seq_ld,
                                                               const float* __restrict__ lse,
                                                               float* __restrict__ lp) {
  __shared__ unsigned long long redk[kWaves];
  const int b = blockIdx.x;
  if (done[b]) return;  // the whole workgroup: a finished row changes nothing
  const int p = pos[b];
  const bf16_t* row = logits + (long)b * ld;
  unsigned long long best = 0ull;
  Row(row, V).sweep([&](int i, uint32_t bits) {
    const unsigned long long k = amax_key(bf2f(bits), i);
    best = k > best ? k : best;
  });
  best = block_max_key(best, redk);
  if (threadIdx.x == 0)
    ragged_finish(key_token(best, V), b, p, (int)params[5], pos, done, tok, seq, seq_ld, row, lse, lp);
}

// {m, lnz} of the log-probability rule (common.h) for every row of logits [M, ld], and with targets
// (int64 [M]; negative or >= V: the row's lp is not written) lp[r] of the target.  The row is loaded
// once into registers when it fits, as in the sampler; both passes stream a longer one.
__global__ __launch_bounds__(kThreads) void lse_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                       const int64_t* __restrict__ targets,
                                                       float* __restrict__ lse, float* __restrict__ lp) {
  __shared__ float redf[kWaves];
  __shared__ unsigned long long redq[kWaves];
  const long r = blockIdx.x;
  const bf16_t* row = logits + r * ld;
  float m;
  unsigned long long z;
  row_max_mass(Row(row, V), redf, redq, m, z, [](int, uint32_t) {});
  if (threadIdx.x == 0) {
    const float lnz = logprob_lnz(z);
    lse[2 * r] = m;
    lse[2 * r + 1] = lnz;
    if (targets) {
      const long t = targets[r];
      if (t >= 0 && t < V) lp[r] = token_logprob(row[t], m, lnz);
    }
  }
}

// after every row of sample_kernel has read them (stream order): next draw, next position
__global__ __launch_bounds__(64) void sample_advance_kernel(uint32_t* params, int* pos_dev) {
  if (threadIdx.x == 0) {
    params[2] += 1u;
    if (pos_dev) pos_dev[0] += 1;
  }
}

}  // namespace

namespace mg {

void sample_logits(const bf16_t* logits, long ld, int B, int V, uint32_t* params, int* pos_dev, int64_t* tok,
                   int64_t* seq, long seq_ld, hipStream_t stream, const float* lse, float* lp) {
  sample_kernel<false, false><<<B, kThreads, 0, stream>>>(logits, ld, V, params, pos_dev, nullptr, tok, seq, seq_ld,
                                                          nullptr, lse, lp);
  sample_advance_kernel<<<1, 64, 0, stream>>>(params, pos_dev);
}

void pick_ragged(const bf16_t* logits, long ld, int B, int V, uint32_t* params, int* pos, int* done, int64_t* tok,
                 int64_t* seq, long seq_ld, bool greedy, hipStream_t stream, const float* lse, float* lp) {
  if (greedy)
    pick_greedy_kernel<<<B, kThreads, 0, stream>>>(logits, ld, V, params, pos, done, tok, seq, seq_ld, lse, lp);
  else sample_kernel<true, false><<<B, kThreads, 0, stream>>>(logits, ld, V, params, pos, done, tok, seq, seq_ld,
                                                              nullptr, lse, lp);
}

void logits_lse(const bf16_t* logits, long ld, int M, int V, const int64_t* targets, float* lse, float* lp,
                hipStream_t stream) {
  lse_kernel<<<M, kThreads, 0, stream>>>(logits, ld, V, targets, lse, lp);
}

void sample_kept(const bf16_t* logits, long ld, int B, int V, const uint32_t* params, int* out, hipStream_t stream) {
  sample_kernel<false, true><<<B, kThreads, 0, stream>>>(logits, ld, V, params, nullptr, nullptr, nullptr, nullptr, 0,
                                                         out, nullptr, nullptr);
}

}  // namespace mg
