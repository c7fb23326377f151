// Int8 KV cache for gfx950 (CDNA4, MI355X): the KV8 rule of common.h on the device.
//
//   kv8_store             snaps the K and V thirds of a prompt's qkv rows in place (the prefill's own
//                         attention then sees the snapped values) and writes the int8 cache.
//   attention_decode_kv8  attention.hip's split-key decode kernel with the loads swapped: keys and
//                         values come as 8 / 16 bytes of int8 plus one fp32 scale per key, the new
//                         token's K/V are snapped into LDS by every workgroup of the head and stored
//                         by split 0.  GROUPED (group = K rows per sequence): attention.hip's grouped
//                         form -- row r of a group sits at base + r, snaps rows 0 .. r of its group
//                         into LDS (keys j >= base never come from the cache) and appends its own.
//   beam_reorder_kv8      beam.hip's in-place reorder on the int8 layout: (q, s) pairs move unchanged.
//
// Cache layout per layer: kq int8 [B, 2, H, Tmax, hd] (K then V; the rows of a (b, h) are contiguous)
// and ks fp32 [B, 2, H, Tmax].  A dequantized element float(q) * s is exact (7 bits times a power of
// two >= 2^-126) and is the bf16 value the snapped row holds, and every score / PV chain below is
// the bf16 kernel's -- the same element order, the same split rule, fold, hand-off and combine -- so
// the output equals attention_decode on the dequantized cache bit for bit.  No scale is folded out of
// a sum.
//
// Rounding steps.  attention.hip leaves mul + add to -ffp-contract=fast, and what the compiler makes of
// it is part of that kernel's behaviour: the plain instantiation rounds every score product before the
// add (v_pk_mul_f32 + v_add_f32), fuses the PV updates (v_pk_fma_f32) -- except dims 6 and 7 of a lane
// in the 4-keys-at-a-time loop, which are v_mul + v_pk_add -- and fuses the one-key tail loop.  This
// kernel states the same steps explicitly (score_step / pv_fused / pv_split), so nothing here is left
// to contraction; tests/test_kv8_kernel_gpu.py holds the two kernels to each other bit for bit.
#include "attn_common.h"
#include "kernels.h"

using namespace mg;
using mg::attn::fexp2;

namespace {

constexpr int kDecSplitsMax = 16;  // attention.hip's: the workspace layout is shared

// ------------------------------------------------------------------------------ the rule
// Integer form of the KV8 rule for bf16 inputs (no fp32 operation sees a subnormal): a15 = the
// largest |u| of the vector as bf16 bits without the sign.  Returns the scale; ex = its exponent;
// live = the vector has non-zero q's (finite, non-zero).
MG_DEVICE float kv8_scale(uint32_t a15, int& ex, bool& live) {
  ex = 0;
  live = false;
  if (a15 >= 0x7f80u) return __uint_as_float(0x7fc00000u);  // inf or NaN in the vector: s = NaN, q = 0
  if (a15 == 0u) return 1.f;
  const int E = (int)(a15 >> 7), m7 = (int)(a15 & 0x7fu);
  // a = (1 + m7 / 128) 2^(E - 127): frexp gives m = (128 + m7) / 256, e = E - 126, and m > 127 / 128
  // only for m7 == 127.  A subnormal a (E == 0) lands far below the floor.
  ex = max(m7 == 127 ? E - 132 : E - 133, -126);
  live = true;
  return __uint_as_float((uint32_t)(ex + 127) << 23);
}

// q of one element (bf16 bits) under scale 2^ex: |u| = mag 2^(max(E, 1) - 134), so |u| / s = mag >> sh
// with sh = ex - max(E, 1) + 134 >= 1 for every |u| <= a; rounded to nearest, halves to even
MG_DEVICE int kv8_quant(uint32_t bits, int ex) {
  const int E = (int)((bits >> 7) & 0xffu), m7 = (int)(bits & 0x7fu);
  const int mag = E ? (128 | m7) : m7;
  const int sh = min(ex - max(E, 1) + 134, 16);
  const int q = min((mag + (1 << (sh - 1)) - 1 + ((mag >> sh) & 1)) >> sh, 127);
  return (bits & 0x8000u) ? -q : q;
}

MG_DEVICE uint32_t max_abs8(const uint4& u) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m = max(m, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
  return m;
}

// 8 elements (one 16-byte chunk of bf16) under the vector's scale: the int8 values packed low byte
// first, and the dequantized floats
MG_DEVICE uint2 kv8_quant8(const uint4& u, int ex, bool live, float s, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
  uint32_t pk[2] = {0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t bits = (w[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
    const int q = live ? kv8_quant(bits, ex) : 0;
    pk[e >> 2] |= ((uint32_t)q & 0xffu) << ((e & 3) * 8);
    f[e] = (float)q * s;  // NaN scale: 0 * NaN = NaN
  }
  return make_uint2(pk[0], pk[1]);
}

// the bf16 kernel's rounding steps (see the top of the file).  A product the compiler cannot see into
// has nothing to contract with (__fmul_rn is a plain multiply here): proc_penalty's device, common.h
MG_DEVICE float mul_rounded(float x, float y) {
  float m = x * y;
  asm volatile("" : "+v"(m));
  return m;
}
MG_DEVICE float score_step(float a, float q, float k) { return a + mul_rounded(q, k); }
MG_DEVICE float pv_fused(float o, float p, float v) { return __builtin_fmaf(p, v, o); }
MG_DEVICE float pv_split(float o, float p, float v) { return o + mul_rounded(p, v); }

MG_DEVICE uint2 ld8(const void* p) { return *reinterpret_cast<const uint2*>(p); }
MG_DEVICE void st8(void* p, const uint2& v) { *reinterpret_cast<uint2*>(p) = v; }

MG_DEVICE float deq(uint32_t w, int byte, float s) { return (float)((int)(w << (24 - 8 * byte)) >> 24) * s; }
MG_DEVICE void dequant8(const uint2& u, float s, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = deq(u.x, e, s);
    f[4 + e] = deq(u.y, e, s);
  }
}

// ------------------------------------------------------------------------------ kv8_store
// One thread per 16-byte chunk; the dch = hd / 8 chunks of a vector sit in consecutive threads of one
// workgroup (256 / dch whole vectors per workgroup) and meet through LDS.  Vector v = ((b * T + t) * 2
// + w) * H + h, so consecutive threads walk consecutive addresses of the K and V thirds.
// rep > 1 (beam prefill): the cache has B * rep rows and prompt b's (q, s) go to rows b * rep .. b * rep + rep - 1.
__global__ __launch_bounds__(256) void kv8_store_kernel(bf16_t* __restrict__ qkv, int8_t* __restrict__ kq,
                                                        float* __restrict__ ks, long NV, int T, int H, int hd,
                                                        long Tmax, int rep) {
  __shared__ uint32_t cm[256];
  const int dch = hd >> 3, vpb = 256 / dch;
  const int lv = threadIdx.x / dch, c = threadIdx.x % dch;
  const long v = (long)blockIdx.x * vpb + lv;
  const bool on = lv < vpb && v < NV;
  const int D = H * hd;
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  bf16_t* src = nullptr;
  int h = 0, w = 0;
  long bt = 0;
  if (on) {
    h = (int)(v % H);
    w = (int)((v / H) % 2);
    bt = v / (2L * H);
    src = qkv + bt * 3L * D + (long)(1 + w) * D + h * hd + c * 8;
    raw = ld16(src);
  }
  cm[threadIdx.x] = max_abs8(raw);
  __syncthreads();
  if (!on) return;
  uint32_t a15 = 0;
  for (int i = 0; i < dch; ++i) a15 = max(a15, cm[lv * dch + i]);
  int ex;
  bool live;
  const float s = kv8_scale(a15, ex, live);
  float f[8];
  const uint2 q8 = kv8_quant8(raw, ex, live, s, f);
  st16(src, pack8(f));  // s * q is a bf16 value: the conversion is exact
  if (kq) {
    const long b = bt / T, t = bt % T;
    for (int i = 0; i < rep; ++i) {
      const long row = (((b * rep + i) * 2 + w) * H + h) * Tmax + t;
      st8(kq + row * hd + c * 8, q8);
      if (c == 0) ks[row] = s;
    }
  }
}

// ------------------------------------------------------------------------------ decode
// attention.hip's attn_decode_kernel<GROUPED> on the int8 cache; what differs is marked KV8.  GROUPED:
// blockIdx.x / (H * S) is the row m = b * group + r; the row's group is snapped into nkv[g * 256 ..],
// g = 0 .. r (at most 8 * 2 * hd / 8 = 256 chunk-threads: the workgroup), and keys j >= base are
// nkv[(j - base) * 256 ..].  The plain instantiation is the code as it was.
template <bool GROUPED>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const bf16_t* __restrict__ qkv_new,
                                                              int8_t* __restrict__ kq, float* __restrict__ ks,
                                                              bf16_t* __restrict__ out, int H, int hd, int D,
                                                              long Tmax, int pos, const int* __restrict__ pos_dev,
                                                              float scale_log2, int S, int KPS,
                                                              float* __restrict__ part,
                                                              unsigned* __restrict__ counters, int pos_stride,
                                                              int group) {
  __shared__ float qs[128];
  __shared__ float sc[256];
  __shared__ float vs[256];   // KV8: the V scale of the split's key t
  // KV8: the new token's snapped K [0, 128) and V [128, 256) of this head; GROUPED: of group row g at g * 256
  __shared__ float nkv[GROUPED ? 8 * 256 : 256];
  __shared__ uint32_t cm[GROUPED ? 256 : 32];
  __shared__ float red[16];
  __shared__ float acc[256 * 8];
  __shared__ int last_flag;
  const int bh = blockIdx.x / S, sp = blockIdx.x % S;
  const int b = bh / H, hh = bh % H;
  int base = 0, m0 = b, cb = b;  // GROUPED: the group's first position and first row; the sequence (cache row)
  if constexpr (GROUPED) {
    m0 = (b / group) * group;
    cb = b / group;
    base = min(max(pos_dev[m0], 0), (int)Tmax - 1);
    pos = base + (b - m0);
    if (pos > (int)Tmax - 1) {  // the whole workgroup: no room for this row
      if (sp == 0 && threadIdx.x < hd) out[(long)b * D + hh * hd + threadIdx.x] = 0;
      return;
    }
  } else {
    if (pos_dev) pos = min(max(pos_dev[(long)b * pos_stride], 0), (int)Tmax - 1);
  }
  const int L = pos + 1;
  const int Se = min(S, (L + KPS - 1) / KPS);
  if (sp >= Se) return;  // never counted: the last arrival is the Se-th (split 0, which appends, stays)
  const long ld = 3L * D;
  const bf16_t* qrow = qkv_new + (long)b * ld + hh * hd;
  const int dch = hd >> 3;
  const long rowk = ((long)(cb * 2) * H + hh) * Tmax, rowv = ((long)(cb * 2 + 1) * H + hh) * Tmax;
  // KV8: snap this step's K/V of the head into LDS (every split: row pos is never read from the
  // cache in the launch that writes it); split 0 appends the int8 row and its scale
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  const int nv = threadIdx.x / dch, nc = threadIdx.x % dch;  // vector and chunk
  const int ng = GROUPED ? nv >> 1 : 0, nw = GROUPED ? nv & 1 : nv;  // group row; 0: K, 1: V
  const int nsnap = (GROUPED ? 2 * (pos - base + 1) : 2) * dch;      // GROUPED: rows 0 .. r of the group
  if (threadIdx.x < nsnap) {
    raw = ld16(qkv_new + (long)(m0 + ng) * ld + hh * hd + (long)D * (1 + nw) + nc * 8);
    cm[threadIdx.x] = max_abs8(raw);
  }
  for (int d = threadIdx.x; d < hd; d += 256) qs[d] = bf2f(qrow[d]);
  __syncthreads();
  if (threadIdx.x < nsnap) {
    uint32_t a15 = 0;
    for (int i = 0; i < dch; ++i) a15 = max(a15, cm[nv * dch + i]);
    int ex;
    bool live;
    const float s = kv8_scale(a15, ex, live);
    float f[8];
    const uint2 q8 = kv8_quant8(raw, ex, live, s, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) nkv[ng * 256 + nw * 128 + nc * 8 + e] = f[e];
    if (sp == 0 && m0 + ng == b) {  // its own row
      const long row = (nw ? rowv : rowk) + pos;
      st8(kq + row * hd + nc * 8, q8);
      if (nc == 0) ks[row] = s;
    }
  }
  __syncthreads();
  const int CH = (L + Se - 1) / Se;
  const int k0 = sp * CH, k1 = min(k0 + CH, L);
  const int nk = max(k1 - k0, 0);
  // scores: one key per thread (CH <= 256), d ascending
  float s = -INFINITY;
  if (threadIdx.x < nk) {
    const int j = k0 + threadIdx.x;
    float a = 0.f;
    if (GROUPED ? j >= base : j == pos) {
      const float* nk_ = nkv + (GROUPED ? (j - base) * 256 : 0);
      for (int d = 0; d < hd; ++d) a = score_step(a, qs[d], nk_[d]);
      vs[threadIdx.x] = 0.f;
    } else {
      const float sk = ks[rowk + j];
      vs[threadIdx.x] = ks[rowv + j];
      const int8_t* kr = kq + (rowk + j) * hd;
      if ((hd & 15) == 0) {
        for (int d = 0; d < hd; d += 16) {
          const uint4 u = ld16(kr + d);
          float k8[8];
          dequant8(make_uint2(u.x, u.y), sk, k8);
#pragma unroll
          for (int e = 0; e < 8; ++e) a = score_step(a, qs[d + e], k8[e]);
          dequant8(make_uint2(u.z, u.w), sk, k8);
#pragma unroll
          for (int e = 0; e < 8; ++e) a = score_step(a, qs[d + 8 + e], k8[e]);
        }
      } else {
        for (int d = 0; d < hd; d += 8) {
          float k8[8];
          dequant8(ld8(kr + d), sk, k8);
#pragma unroll
          for (int e = 0; e < 8; ++e) a = score_step(a, qs[d + e], k8[e]);
        }
      }
    }
    s = a * scale_log2;
  }
  const float mx = block_max<4>(s, red);
  const float p = threadIdx.x < nk ? fexp2(s - mx) : 0.f;
  sc[threadIdx.x] = p;
  const float sm = block_sum<4>(p, red + 4);
  __syncthreads();
  // P V: DCH = hd/8 lanes of 8 dims per key group, 256/DCH key groups, loads issued 4 at a time
  const int ngrp = 256 / dch;
  const int grp = threadIdx.x / dch, d8 = (threadIdx.x % dch) * 8;
  const int8_t* vb = kq + rowv * hd + d8;
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (grp < ngrp) {
    int jj = grp;
    for (; jj + 3 * ngrp < nk; jj += 4 * ngrp) {
      uint2 vv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = k0 + jj + u * ngrp;
        vv[u] = (GROUPED ? j >= base : j == pos) ? make_uint2(0u, 0u) : ld8(vb + (long)j * hd);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = jj + u * ngrp;
        float v8[8];
        dequant8(vv[u], vs[t], v8);
        if (GROUPED ? k0 + t >= base : k0 + t == pos) {
          const float* nv_ = nkv + (GROUPED ? (k0 + t - base) * 256 : 0) + 128 + d8;
#pragma unroll
          for (int e = 0; e < 8; ++e) v8[e] = nv_[e];
        }
        const float pj = sc[t];
#pragma unroll
        for (int e = 0; e < 6; ++e) o[e] = pv_fused(o[e], pj, v8[e]);
        o[6] = pv_split(o[6], pj, v8[6]);
        o[7] = pv_split(o[7], pj, v8[7]);
      }
    }
    for (; jj < nk; jj += ngrp) {
      const int j = k0 + jj;
      float v8[8];
      if (GROUPED ? j >= base : j == pos) {
        const float* nv_ = nkv + (GROUPED ? (j - base) * 256 : 0) + 128 + d8;
#pragma unroll
        for (int e = 0; e < 8; ++e) v8[e] = nv_[e];
      } else {
        dequant8(ld8(vb + (long)j * hd), vs[jj], v8);
      }
      const float pj = sc[jj];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = pv_fused(o[e], pj, v8[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[threadIdx.x * 8 + e] = o[e];
  __syncthreads();
  if (Se == 1) {  // the whole context in this workgroup: normalise and write
    if (threadIdx.x < hd) {
      const int c = threadIdx.x / 8, e = threadIdx.x % 8;
      float v = 0.f;
      for (int g = 0; g < ngrp; ++g) v += acc[(g * dch + c) * 8 + e];
      out[(long)b * D + hh * hd + threadIdx.x] = f2bf(v / sm);
    }
    return;
  }
  // partial state of this split: {max, sum, o[hd]} (fp32)
  float* mine = part + (long)blockIdx.x * (hd + 2);
  if (threadIdx.x < hd) {
    const int c = threadIdx.x / 8, e = threadIdx.x % 8;
    float v = 0.f;
    for (int g = 0; g < ngrp; ++g) v += acc[(g * dch + c) * 8 + e];
    __hip_atomic_store(mine + 2 + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(mine, nk ? mx : -INFINITY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 1, sm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's partial stores have landed
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(counters + bh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_flag = prev == (unsigned)(Se - 1);
  }
  __syncthreads();
  if (!last_flag) return;
  // last split of (b, h): combine the partial states (agent-scope loads: never a stale line)
  const float* pb = part + (long)bh * S * (hd + 2);
  if (threadIdx.x < Se) {
    red[threadIdx.x] = __hip_atomic_load(pb + threadIdx.x * (hd + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sc[threadIdx.x] = __hip_atomic_load(pb + threadIdx.x * (hd + 2) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (threadIdx.x < hd) {
    float ov[kDecSplitsMax];
#pragma unroll
    for (int t = 0; t < kDecSplitsMax; ++t)
      ov[t] = t < Se ? __hip_atomic_load(pb + t * (hd + 2) + 2 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    float M = -INFINITY;
    for (int t = 0; t < Se; ++t) M = fmaxf(M, red[t]);
    float Ls = 0.f, Os = 0.f;
#pragma unroll
    for (int t = 0; t < kDecSplitsMax; ++t) {
      if (t < Se && red[t] != -INFINITY) {
        const float w = fexp2(red[t] - M);
        Ls += w * sc[t];
        Os += w * ov[t];
      }
    }
    out[(long)b * D + hh * hd + threadIdx.x] = f2bf(Os / Ls);
  }
  if (threadIdx.x == 0) __hip_atomic_store(counters + bh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------ beam reorder
// beam.hip's reorder on kq int8 [L, R, 2, H, Tmax, hd] and ks fp32 [L, R, 2, H, Tmax], R = B * W: for
// prompt blockIdx.y in layer blockIdx.z, positions t < min(*pos, Tmax) of every (K | V, head) block of
// beam r become those of beam parent[r].  A thread owns one chunk of the int8 bytes at (K | V, head, t)
// -- CT = 16 bytes where hd % 16 == 0, else 8: a block starts at a multiple of Tmax * hd bytes, which
// is only 8-byte aligned for hd % 16 == 8 with odd Tmax -- or one scale word (rows of Tmax words are
// only 4-byte aligned for odd Tmax), loads it from all W beams and stores the permutation; a beam
// that keeps its rows stores nothing.  Per (K | V, head) the items are the Tmax * cpv chunks, then the
// Tmax scale words.
typedef unsigned kv8_u4 __attribute__((ext_vector_type(4)));
typedef unsigned kv8_u2 __attribute__((ext_vector_type(2)));

template <int W, typename T>
MG_DEVICE void reorder_item(T* p, long beam_stride, const int (&par)[W]) {
  T v[W];
#pragma unroll
  for (int r = 0; r < W; ++r) v[r] = p[r * beam_stride];
#pragma unroll
  for (int r = 0; r < W; ++r) {
    // uniform branches over constant register indices, as in beam.hip
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if (q != r && par[r] == q) p[r * beam_stride] = v[q];
    }
  }
}

template <int W, typename CT>
__global__ __launch_bounds__(256) void beam_reorder_kv8_kernel(int8_t* __restrict__ kq, float* __restrict__ ks,
                                                               long kq_layer, long ks_layer, int H2, int Tmax,
                                                               int hd, const int* __restrict__ parent,
                                                               const int* __restrict__ pos, int* ctl,
                                                               unsigned* err) {
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
  if (ident) return;
  int n = pos[0];
  n = n < Tmax ? n : Tmax;
  constexpr int CB = (int)sizeof(CT);
  const int cpv = hd / CB;            // chunks per vector
  const int per = Tmax * (cpv + 1);   // items per (K | V, head): chunks, then scale words
  const int idx = blockIdx.x * 256 + (int)threadIdx.x;
  const int wh = idx / per, rem = idx - wh * per;
  if (wh >= H2) return;
  const long blk = (long)b * W * H2 + wh;  // beam 0's (row, K | V, head) block
  if (rem < Tmax * cpv) {
    const int t = rem / cpv, c = rem - t * cpv;
    if (t >= n) return;
    int8_t* p = kq + blockIdx.z * kq_layer + (blk * Tmax + t) * hd + c * CB;
    reorder_item<W>(reinterpret_cast<CT*>(p), (long)H2 * Tmax * hd / CB, par);
  } else {
    const int t = rem - Tmax * cpv;
    if (t >= n) return;
    reorder_item<W>(ks + blockIdx.z * ks_layer + blk * Tmax + t, (long)H2 * Tmax, par);
  }
}


}  // namespace

namespace mg {

void kv8_store(bf16_t* qkv, int8_t* kq, float* ks, int B, int T, int H, int hd, long Tmax, hipStream_t stream,
               int rep) {
  const long NV = (long)B * T * 2 * H;
  const int vpb = 256 / (hd >> 3);
  kv8_store_kernel<<<cdiv(NV, vpb), 256, 0, stream>>>(qkv, kq, ks, NV, T, H, hd, Tmax, rep);
}

void attention_decode_kv8(const bf16_t* qkv_new, int8_t* kq, float* ks, bf16_t* out, int B, int H, int hd,
                          long Tmax, int pos, hipStream_t stream, float* part, unsigned* counters,
                          const int* pos_dev, int pos_stride, int group) {
  // the grid, the split count and the keys per split are attention_decode's (B: sequences)
  const int S = kDecSplitsMax;
  const int kps = B * H <= 32 ? 256 : 128;
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)hd);
  if (group > 1) {
    attn_decode_kv8_kernel<true><<<B * group * H * S, 256, 0, stream>>>(
        qkv_new, kq, ks, out, H, hd, H * hd, Tmax, pos, pos_dev, scale_log2, S, kps, part, counters, pos_stride, group);
    return;
  }
  attn_decode_kv8_kernel<false><<<B * H * S, 256, 0, stream>>>(qkv_new, kq, ks, out, H, hd, H * hd, Tmax, pos, pos_dev,
                                                               scale_log2, S, kps, part, counters, pos_stride, group);
}

void beam_reorder_kv8(int8_t* kq, float* ks, int L, long kq_layer, long ks_layer, int B, int W, int H, int Tmax,
                      int hd, const int* parent, const int* pos, int* ctl, hipStream_t stream) {
  const bool wide = hd % 16 == 0;
  const long items = 2L * H * Tmax * (hd / (wide ? 16 : 8) + 1);
  const dim3 grid(cdiv(items, 256), B, L);
#define MG_BEAM_REORDER_KV8(w)                                                                                \
  case w:                                                                                                     \
    if (wide)                                                                                                 \
      beam_reorder_kv8_kernel<w, kv8_u4><<<grid, 256, 0, stream>>>(kq, ks, kq_layer, ks_layer, 2 * H, Tmax, hd, \
                                                                  parent, pos, ctl, debug_err_word());        \
    else                                                                                                      \
      beam_reorder_kv8_kernel<w, kv8_u2><<<grid, 256, 0, stream>>>(kq, ks, kq_layer, ks_layer, 2 * H, Tmax, hd, \
                                                                  parent, pos, ctl, debug_err_word());        \
    break;
  switch (W) {
    MG_BEAM_REORDER_KV8(1) MG_BEAM_REORDER_KV8(2) MG_BEAM_REORDER_KV8(3) MG_BEAM_REORDER_KV8(4)
    MG_BEAM_REORDER_KV8(5) MG_BEAM_REORDER_KV8(6) MG_BEAM_REORDER_KV8(7) MG_BEAM_REORDER_KV8(8)
    default: break;  // the binding admits 1 .. 8
  }
#undef MG_BEAM_REORDER_KV8
}

}  // namespace mg
