// The KV8 rule (common.h) on the device, shared by the kernels that read or append the int8 KV cache
// (attention_kv8.hip, attention_shared.hip): the scale and the int8 values of one vector, and the
// dequantized floats of 8 stored bytes.
#pragma once
#include "common.h"

namespace mg {
namespace kv8 {

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

// 8 stored int8 values times their vector's scale: exact, and the bf16 value the snapped row holds
MG_DEVICE float deq(uint32_t w, int byte, float s) { return (float)((int)(w << (24 - 8 * byte)) >> 24) * s; }
MG_DEVICE void dequant8(const uint2& u, float s, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = deq(u.x, e, s);
    f[4 + e] = deq(u.y, e, s);
  }
}

}  // namespace kv8
}  // namespace mg
