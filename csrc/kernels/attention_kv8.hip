// Int8 KV cache for gfx950 (CDNA4, MI355X): the KV8 rule of common.h on the device.
//
//   kv8_store             snaps the K and V thirds of a prompt's qkv rows in place (the prefill's own
//                         attention then sees the snapped values) and writes the int8 cache.
//   attention_decode_kv8  attention.hip's split-key decode kernel with the loads swapped: keys and
//                         values come as 8 / 16 bytes of int8 plus one fp32 scale per key, the new
//                         token's K/V are snapped into LDS by every workgroup of the head and stored
//                         by split 0.
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
__global__ __launch_bounds__(256) void kv8_store_kernel(bf16_t* __restrict__ qkv, int8_t* __restrict__ kq,
                                                        float* __restrict__ ks, long NV, int T, int H, int hd,
                                                        long Tmax) {
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
    const long row = ((b * 2 + w) * H + h) * Tmax + t;
    st8(kq + row * hd + c * 8, q8);
    if (c == 0) ks[row] = s;
  }
}

// ------------------------------------------------------------------------------ decode
// attention.hip's attn_decode_kernel<false> on the int8 cache; what differs is marked KV8.
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const bf16_t* __restrict__ qkv_new,
                                                              int8_t* __restrict__ kq, float* __restrict__ ks,
                                                              bf16_t* __restrict__ out, int H, int hd, int D,
                                                              long Tmax, int pos, const int* __restrict__ pos_dev,
                                                              float scale_log2, int S, int KPS,
                                                              float* __restrict__ part,
                                                              unsigned* __restrict__ counters, int pos_stride) {
  __shared__ float qs[128];
  __shared__ float sc[256];
  __shared__ float vs[256];   // KV8: the V scale of the split's key t
  __shared__ float nkv[256];  // KV8: the new token's snapped K [0, 128) and V [128, 256) of this head
  __shared__ uint32_t cm[32];
  __shared__ float red[16];
  __shared__ float acc[256 * 8];
  __shared__ int last_flag;
  const int bh = blockIdx.x / S, sp = blockIdx.x % S;
  const int b = bh / H, hh = bh % H;
  if (pos_dev) pos = min(max(pos_dev[(long)b * pos_stride], 0), (int)Tmax - 1);
  const int L = pos + 1;
  const int Se = min(S, (L + KPS - 1) / KPS);
  if (sp >= Se) return;  // never counted: the last arrival is the Se-th (split 0, which appends, stays)
  const long ld = 3L * D;
  const bf16_t* qrow = qkv_new + (long)b * ld + hh * hd;
  const int dch = hd >> 3;
  const long rowk = ((long)(b * 2) * H + hh) * Tmax, rowv = ((long)(b * 2 + 1) * H + hh) * Tmax;
  // KV8: snap this step's K/V of the head into LDS (every split: row pos is never read from the
  // cache in the launch that writes it); split 0 appends the int8 row and its scale
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  const int nw = threadIdx.x / dch, nc = threadIdx.x % dch;  // vector (0: K, 1: V) and chunk
  if (threadIdx.x < 2 * dch) {
    raw = ld16(qrow + (long)D * (1 + nw) + nc * 8);
    cm[threadIdx.x] = max_abs8(raw);
  }
  for (int d = threadIdx.x; d < hd; d += 256) qs[d] = bf2f(qrow[d]);
  __syncthreads();
  if (threadIdx.x < 2 * dch) {
    uint32_t a15 = 0;
    for (int i = 0; i < dch; ++i) a15 = max(a15, cm[nw * dch + i]);
    int ex;
    bool live;
    const float s = kv8_scale(a15, ex, live);
    float f[8];
    const uint2 q8 = kv8_quant8(raw, ex, live, s, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) nkv[nw * 128 + nc * 8 + e] = f[e];
    if (sp == 0) {
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
    if (j == pos) {
      for (int d = 0; d < hd; ++d) a = score_step(a, qs[d], nkv[d]);
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
        vv[u] = j == pos ? make_uint2(0u, 0u) : ld8(vb + (long)j * hd);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = jj + u * ngrp;
        float v8[8];
        dequant8(vv[u], vs[t], v8);
        if (k0 + t == pos) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v8[e] = nkv[128 + d8 + e];
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
      if (j == pos) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v8[e] = nkv[128 + d8 + e];
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

}  // namespace

namespace mg {

void kv8_store(bf16_t* qkv, int8_t* kq, float* ks, int B, int T, int H, int hd, long Tmax, hipStream_t stream) {
  const long NV = (long)B * T * 2 * H;
  const int vpb = 256 / (hd >> 3);
  kv8_store_kernel<<<cdiv(NV, vpb), 256, 0, stream>>>(qkv, kq, ks, NV, T, H, hd, Tmax);
}

void attention_decode_kv8(const bf16_t* qkv_new, int8_t* kq, float* ks, bf16_t* out, int B, int H, int hd,
                          long Tmax, int pos, hipStream_t stream, float* part, unsigned* counters,
                          const int* pos_dev, int pos_stride) {
  // the grid, the split count and the keys per split are attention_decode's
  const int S = kDecSplitsMax;
  const int kps = B * H <= 32 ? 256 : 128;
  attn_decode_kv8_kernel<<<B * H * S, 256, 0, stream>>>(qkv_new, kq, ks, out, H, hd, H * hd, Tmax, pos, pos_dev,
                                                        1.4426950408889634f / sqrtf((float)hd), S, kps, part,
                                                        counters, pos_stride);
}

}  // namespace mg
