// The row of the one-workgroup-per-logits-row kernels (sample.hip, beam.hip): 1024 threads walk a
// row of bf16 logits 8 columns per 16-byte load, keep it in registers when it fits (Row), rank it by
// 16-bit (key16) and 64-bit (amax_key, common.h) keys and reduce keys / integer masses over the
// workgroup.  Shared so that every kernel that ranks or sums a row does it with the same code: the
// lse kernel's {m, lnz} and the beam row kernel's are one function, row_max_mass.
#pragma once
#include "common.h"

namespace mg {
namespace row {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

MG_DEVICE unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

template <class F>
MG_DEVICE void for_vec(const uint4& u, int i, F f) {
  f(i + 0, u.x & 0xffffu); f(i + 1, u.x >> 16);
  f(i + 2, u.y & 0xffffu); f(i + 3, u.y >> 16);
  f(i + 4, u.z & 0xffffu); f(i + 5, u.z >> 16);
  f(i + 6, u.w & 0xffffu); f(i + 7, u.w >> 16);
}

// f(i, bits) for every element i < V of the row, 8 per 16-byte load; the V % 8 tail one by one
// (columns >= V are never loaded)
template <class F>
MG_DEVICE void for_row(const bf16_t* __restrict__ row, int V, F f) {
  const int nv = V >> 3;
  for (int v = threadIdx.x; v < nv; v += kThreads) for_vec(ld16(row + (long)v * 8), v * 8, f);
  const int i = nv * 8 + (int)threadIdx.x;
  if (threadIdx.x < 8 && i < V) f(i, (uint32_t)row[i]);
}

// A row of up to kRegVec * kThreads * 8 = 65536 columns is loaded ONCE, every load in flight
// together (thread t holds vectors t, t + 1024, ...): the row was written by the LM head's
// workgroups on every XCD, so a load pays the trip past this XCD's L2, and a pass that walks the
// row with a loop pays it once per iteration (measured at V = 50257, top_k 40: 21.0 us per call
// with three streaming passes, 18.8 us from registers; the rest is the one CU's VALU rate over
// ~15 instructions per element and pass, PERF.md).  Unrolled over the registers, so only for
// cheap per-element bodies.
constexpr int kRegVec = 8;

template <class F>
MG_DEVICE void for_regs(const uint4 (&regs)[kRegVec], uint32_t tail, int V, F f) {
  const int nv = V >> 3;
#pragma unroll
  for (int j = 0; j < kRegVec; ++j) {
    const int v = (int)threadIdx.x + j * kThreads;
    if (v < nv) for_vec(regs[j], v * 8, f);
  }
  const int i = nv * 8 + (int)threadIdx.x;
  if (threadIdx.x < 8 && i < V) f(i, tail);
}

// The first V columns of one logits row as its workgroup holds it: in registers when it fits
// (`cached`: regs and tail are loaded here; thread t < 8 holds tail element (V & ~7) + t), else
// streamed again by every sweep.
struct Row {
  const bf16_t* row;
  int V;
  bool cached;
  uint4 regs[kRegVec];
  uint32_t tail = 0u;

  MG_DEVICE Row(const bf16_t* row_, int V_) : row(row_), V(V_), cached((V_ >> 3) <= kRegVec * kThreads) {
    const int nv = V >> 3, ti = nv * 8 + (int)threadIdx.x;
    if (cached) {
#pragma unroll
      for (int j = 0; j < kRegVec; ++j) {
        const int v = (int)threadIdx.x + j * kThreads;
        regs[j] = v < nv ? ld16(row + (long)v * 8) : make_uint4(0u, 0u, 0u, 0u);
      }
      if (threadIdx.x < 8 && ti < V) tail = row[ti];
    }
  }

  // f(i, bits) for every element i < V
  template <class F>
  MG_DEVICE void sweep(F f) const {
    if (cached) for_regs(regs, tail, V, f);
    else for_row(row, V, f);
  }
};

// order-preserving 16-bit key of a bf16 bit pattern (-0 counts as +0, as in a float compare), and
// the bit pattern of a key (of +0 for the key the two zeros share).  key16_bits also undoes the high
// half of amax_key's 32-bit float key, which orders the same 16 bits but keeps -0 below +0.
MG_DEVICE uint32_t key16(uint32_t bits) {
  if (bits == 0x8000u) bits = 0u;
  return (bits & 0x8000u) ? (bits ^ 0xffffu) : (bits | 0x8000u);
}
MG_DEVICE uint32_t key16_bits(uint32_t key) { return (key & 0x8000u) ? (key ^ 0x8000u) : (key ^ 0xffffu); }

// the token of a winning amax_key-style key (index inverted in the low word) of a row of V
// columns; no candidate (key 0: a row without a finite maximum) still gives a valid id
MG_DEVICE long key_token(unsigned long long best, int V) {
  const long t = amax_index(best);
  return t >= V ? V - 1 : t;
}

// max of one key per lane over the wave, in every lane
MG_DEVICE unsigned long long wave_max_key(unsigned long long best) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = shfl_xor_u64(best, o);
    best = k > best ? k : best;
  }
  return best;
}

// max of one key per thread over the workgroup, valid in thread 0
MG_DEVICE unsigned long long block_max_key(unsigned long long best, unsigned long long* redk) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  best = wave_max_key(best);
  if (lane == 0) redk[w] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kWaves; ++i) best = redk[i] > best ? redk[i] : best;
  }
  return best;
}

// sum of one 64-bit integer per thread over the workgroup, broadcast (integer adds: any order)
MG_DEVICE unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
  if (lane == 0) red[w] = v;
  __syncthreads();
  unsigned long long t = 0ull;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) t += red[i];
  return t;
}

// {m, z} of the log-probability rule (common.h) for a row, in every thread: the maximum, then the
// integer sum of the masses at temperature 1 (lnz = logprob_lnz(z)).  redf, redq: kWaves words of
// LDS each.  rider(i, bits) runs for every element inside the first sweep (the beam row kernel forms
// its keys there).
template <class F>
MG_DEVICE void row_max_mass(const Row& r, float* redf, unsigned long long* redq, float& m, unsigned long long& z,
                            F rider) {
  m = -INFINITY;
  r.sweep([&](int i, uint32_t bits) {
    m = fmaxf(m, bf2f(bits));
    rider(i, bits);
  });
  m = block_max<kWaves>(m, redf);
  z = 0ull;
  r.sweep([&](int, uint32_t bits) { z += sample_mass(bits, m, 1.0f); });
  z = block_sum_u64(z, redq);
}

}  // namespace row
}  // namespace mg
