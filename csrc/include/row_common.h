// Row helpers of the one-workgroup-per-logits-row kernels (sample.hip, beam.hip): 1024 threads walk
// a row of bf16 logits 8 columns per 16-byte load, keep it in registers when it fits, and reduce
// 64-bit keys / integer masses over the workgroup.  Shared so that every kernel that ranks or sums a
// row does it with the same code: the lse kernel's {m, lnz} and the beam row kernel's are one
// instruction sequence.
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

// order-preserving key of a float with the index inverted in the low half: the max key is the
// FIRST index among equal values (the amax_key of gemv.hip, whose fused argmax ranks the same
// stored bf16 logits)
MG_DEVICE unsigned long long amax_key(float v, int n) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)k << 32) | (uint32_t)(0xffffffffu - (uint32_t)n);
}

// max of one key per thread over the workgroup, valid in thread 0
MG_DEVICE unsigned long long block_max_key(unsigned long long best, unsigned long long* redk) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = shfl_xor_u64(best, o);
    best = k > best ? k : best;
  }
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

}  // namespace row
}  // namespace mg
