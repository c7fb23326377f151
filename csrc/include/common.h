// Shared device helpers for the gfx950 (CDNA4, MI355X) kernels.
//
// Conventions used by every kernel in csrc/kernels:
//  * bf16 tensors travel as raw uint16_t bit patterns; they are loaded 8 at a time
//    (16 B per lane, the coalescing sweet spot on CDNA) and widened to fp32 with a shift.
//  * a wave is 64 lanes; block sizes are multiples of 64.
//  * every launch takes an explicit hipStream_t (the caller's current torch stream), so a
//    whole step can be captured into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#define MG_DEVICE __device__ __forceinline__

namespace mg {

constexpr int kWave = 64;

typedef uint16_t bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

MG_DEVICE float bf2f(uint32_t v) { return __uint_as_float(v << 16); }

MG_DEVICE bf16_t f2bf(float f) {
  __bf16 h = (__bf16)f;  // gfx950: v_cvt_pk_bf16_f32, round-to-nearest-even, NaN-preserving
  return __builtin_bit_cast(bf16_t, h);
}

// ONE v_cvt_pk_bf16_f32 (two scalar converts + shift + or when written element-wise)
MG_DEVICE uint32_t pack2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// 8 x bf16 <-> 8 x f32 through one 16-byte vector.
MG_DEVICE void unpack8(const uint4& u, float (&f)[8]) {
  f[0] = bf2f(u.x & 0xffffu); f[1] = bf2f(u.x >> 16);
  f[2] = bf2f(u.y & 0xffffu); f[3] = bf2f(u.y >> 16);
  f[4] = bf2f(u.z & 0xffffu); f[5] = bf2f(u.z >> 16);
  f[6] = bf2f(u.w & 0xffffu); f[7] = bf2f(u.w >> 16);
}

MG_DEVICE uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}

MG_DEVICE uint4 ld16(const void* p) { return *reinterpret_cast<const uint4*>(p); }
// non-temporal 16-byte load (streamed-once weights: decode GEMV)
MG_DEVICE uint4 ld16_nt(const void* p) {
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// hipGraph mode: a captured kernel's seed argument is an offset into a per-replay stream whose
// counter lives in device memory (incremented inside the graph), so every replay draws new
// dropout masks; nullptr = eager launch, the argument is the seed itself.
MG_DEVICE uint64_t eff_seed(uint64_t s, const uint64_t* ofs) {
  return ofs ? s + ofs[0] * 0x9E3779B97F4A7C15ull : s;
}

// Opaque to the optimiser: values derived from v before the fence are recomputed after it
// instead of being kept live (keeps packed bf16 packed across a reduction; see layernorm.hip).
MG_DEVICE void reg_fence(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
MG_DEVICE void st16(void* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }
// non-temporal 16-byte store (a large output consumed by a later kernel: keep L2 / MALL for inputs)
MG_DEVICE void st16_nt(void* p, const uint4& v) {
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(v4u{v.x, v.y, v.z, v.w}, reinterpret_cast<v4u*>(p));
}

// ---------------------------------------------------------------- wave / block reductions
MG_DEVICE float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

MG_DEVICE float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum over a block of NW waves; `red` must hold NW floats of LDS. Result broadcast to all.
template <int NW>
MG_DEVICE float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) t += red[i];
  return t;
}

template <int NW>
MG_DEVICE float block_max(float v, float* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = -INFINITY;
#pragma unroll
  for (int i = 0; i < NW; ++i) t = fmaxf(t, red[i]);
  return t;
}

// ---------------------------------------------------------------- argmax keys
// order-preserving key of a float (larger float -> larger key) with the index inverted in the low
// half: the max key is the FIRST index among equal values (torch.argmax).  One definition for the
// LM head's fused argmax (gemv.hip), the embedding kernel that reduces its keys, and the row kernels
// (row_common.h), which all rank the same stored bf16 logits.
MG_DEVICE unsigned long long amax_key(float v, int n) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)k << 32) | (uint32_t)(0xffffffffu - (uint32_t)n);
}
// the index in a key (key 0, "no candidate", gives 0xffffffff)
MG_DEVICE long amax_index(unsigned long long key) { return (long)(0xffffffffu - (uint32_t)key); }

// ---------------------------------------------------------------- residual-stream dropout mask
// Exact nn.Dropout(p) decisions to 1/65536: keep iff a 16-bit uniform >= thr16 = round(65536 p),
// scale 65536 / (65536 - thr16) (p = 0.1 -> 0.100006; the 8-bit decisions of rounds 1-3 ran
// p = 0.1 as 26/256 = 0.1016).  Element (m, n) of a row-major [M, N] tensor takes half (n & 1) of
// the word  fmix32(m * ceil(N / 2) + (n >> 1) + key(seed))  (32-bit index arithmetic: exact below
// 2^32 words, i.e. 8 G elements per tensor).  One word per 2 consecutive elements: a GEMM epilogue
// lane holding C[m][n..n+3] draws two, a thread owning 8 consecutive elements four.  The murmur3
// finaliser is 2 multiplies per word (a Philox-4x32-10 generator, used in round 1, cost 40
// quarter-rate multiplies per 16 decisions and made the standalone dropout-backward kernels
// RNG-bound).  Counter-based: backward regenerates the mask, nothing is stored.
constexpr uint32_t kRowDropSalt = 0x0d0f0d0fu;

inline uint32_t dropout_threshold16(float p) {
  const double t = (double)p * 65536.0 + 0.5;
  return (uint32_t)(t < 0.0 ? 0.0 : (t > 65536.0 ? 65536.0 : t));
}
inline float dropout_scale16(uint32_t thr16) { return thr16 >= 65536u ? 0.f : 65536.f / (float)(65536u - thr16); }

MG_DEVICE uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// per-seed key (wave-uniform: scalar work)
MG_DEVICE uint32_t rowdrop_key(uint64_t seed) {
  return fmix32((uint32_t)seed ^ kRowDropSalt) ^ ((uint32_t)(seed >> 32) * 0x9E3779B1u);
}

// decision word of elements (m, n), (m, n + 1), n % 2 == 0
MG_DEVICE uint32_t rowdrop_word(uint32_t key, long m, int n, int N) {
  return fmix32((uint32_t)m * (uint32_t)((N + 1) >> 1) + (uint32_t)(n >> 1) + key);
}

// apply the mask to 2 consecutive elements whose decisions are the two halves of `word`
MG_DEVICE void rowdrop2(float* v, uint32_t word, uint32_t thr16, float scale) {
  v[0] = (word & 0xffffu) >= thr16 ? v[0] * scale : 0.f;
  v[1] = (word >> 16) >= thr16 ? v[1] * scale : 0.f;
}

// 4 consecutive elements (m, n..n+3), n % 4 == 0
MG_DEVICE void rowdrop4(float* v, uint32_t key, long m, int n, int N, uint32_t thr16, float scale) {
  rowdrop2(v, rowdrop_word(key, m, n, N), thr16, scale);
  rowdrop2(v + 2, rowdrop_word(key, m, n + 2, N), thr16, scale);
}

// 8 consecutive elements (m, n..n+7), n % 8 == 0
MG_DEVICE void rowdrop8(float (&v)[8], uint64_t seed, long m, int n, int N, uint32_t thr16, float scale) {
  const uint32_t key = rowdrop_key(seed);
  rowdrop4(v, key, m, n, N, thr16, scale);
  rowdrop4(v + 4, key, m, n + 4, N, thr16, scale);
}

// ---------------------------------------------------------------- Gumbel-max sampling
// One token per logits row, exactly distributed as softmax(l / T) over the kept set, from a
// counter-based hash: the token depends on (seed, draw, row, logits) alone, not on a reduction
// order, a workgroup size or graph / eager mode.  For batch row b, draw counter d (the column of
// the produced token in the returned sequence), vocabulary index i < V and a 64-bit seed:
//   r0 = fmix32(lo32(seed) ^ kSampleSalt)     r1 = fmix32(r0 + hi32(seed))
//   r2 = fmix32(r1 + d)                       r3 = fmix32(r2 ^ b)
//   h  = fmix32(r3 + i * 0x9E3779B1)          (all mod 2^32)
//   u  = ((h >> 8) + 0.5) * 2^-24             (24 bits: never 0 or 1)
//   g  = -ln(-ln(u))
// Kept set: { i : l_i >= the min(top_k, V)-th largest logit of the row } on the bf16 logits, ties
// at the threshold all kept (the reference's `logits[logits < v[:, [-1]]] = -inf`); every i when
// top-k is off.  Score of a kept element: s_i = (l_i - m) * inv_t + g_i, m the row maximum,
// inv_t = float32(1 / temperature).  The token is the kept index with the largest s_i, the lowest
// index on an exact tie.  -inf logits never win; the row maximum must be finite.
// fp32 evaluation: x = h >> 8 below 2^23 gives u = (x + 0.5) 2^-24 exactly; from 2^23 on u has 25
// significant bits, so its complement y = ((2^24 - x) - 0.5) 2^-24 is formed instead (exact) and
// -ln(u) = -log1p(-y).  Accurate logf / log1pf, not the fast intrinsics: g is good to ~1e-6, the
// score of any contender within 25 of the top to ~1e-5.
//
// Nucleus (top-p) filtering, after the temperature and top-k, before the Gumbel pass.  K is the
// set top-k keeps (every finite entry when top-k is off; -inf is never kept), and for i in K
//   w_i = exp((l_i - m) * inv_t)      Z = sum_K w_i      A(v) = sum_{i in K, l_i > v} w_i
// (A(v): the mass strictly above the value v).  Kept: every i in K with A(l_i) < top_p * Z.  Equal
// logits have the same A, so they are kept or dropped together (ties at the threshold all kept, as
// for top-k); A(m) = 0, so the row maximum is always kept; A grows as the value falls, so the kept
// set is an upper set of the bf16 values -- a threshold on the 16-bit key, and the final threshold
// is the larger of the top-k and the nucleus keys.  top_p is a float32 in (0, 1]; params word 6
// holds its bits, and 0 or anything >= 1.0 means off (the stage is skipped by a uniform branch).
// Device arithmetic, independent of the order of the additions: the mass of an element is the
// integer q_i = floor(w^_i * 2^32), w^_i = exp2(((l_i - m) * inv_t) * float32(log2 e)) in fp32
// (sample_mass: subtract, two multiplies, v_exp_f32, a scale by 2^32, truncation -- one fixed
// sequence, nothing to contract or reassociate), added as a 64-bit integer into LDS histograms
// over the key's high, then low byte (V * 2^32 fits 64 bits for any V the binding accepts).  With
// top_p = f * 2^-s exactly (f its 24-bit significand), the target is the integer
//   T = ceil(f * Z^ / 2^s),  Z^ = sum q_i   (a 128-bit product),
// and A^ < top_p * Z^ over the reals is exactly A^ < T over the integers.  The threshold is the
// lowest key whose mass strictly above is below T.
// Error of A^/Z^ against the real A/Z: an element's weight is off by at most eps_w * w_i + 2^-32,
//   eps_w = 22.2 * (3 * 2^-24 + 1.2e-8) + 2^-23 = 4.4e-6
// (three fp32 roundings and the rounded constant on an exponent of at most 32 ln 2 = 22.2 in
// magnitude -- smaller weights truncate to 0 and are covered by the 2^-32 -- and 1 ulp of
// v_exp_f32).  Z >= 1 (the maximum weighs 1), so |A^/Z^ - A/Z| <= 2 eps_w * A/Z + V * 2^-32: at the
// boundary A/Z ~ top_p this is a relative shift of top_p by at most 8.8e-6 + V * 2^-32 / top_p
// (2.2e-5 at V = 50257, top_p = 0.9; 4.8e-5 at top_p = 0.3).  The tests bracket the kernel's
// threshold between the fp64 rule at top_p (1 +- delta), delta = 4 x that bound.
constexpr uint32_t kSampleSalt = 0x5a3b1e97u;

// q_i of the nucleus rule above: floor(2^32 exp((l - m) * inv_t)) for l <= m, 0 for l = -inf
MG_DEVICE unsigned long long sample_mass(uint32_t bits, float m, float inv_t) {
  const float y = ((bf2f(bits) - m) * inv_t) * 1.44269504f;
  return (unsigned long long)(__builtin_amdgcn_exp2f(y) * 0x1p32f);
}

// T of the nucleus rule: ceil(top_p * Z) for top_p in (0, 1) given as fp32 bits, exactly
MG_DEVICE unsigned long long sample_nucleus_target(uint32_t top_p_bits, unsigned long long Z) {
  const uint32_t e = top_p_bits >> 23, frac = top_p_bits & 0x7fffffu;
  const uint32_t f = e ? (frac | 0x800000u) : frac, s = e ? 150u - e : 149u;  // top_p = f * 2^-s, s >= 24
  const unsigned __int128 prod = (unsigned __int128)f * Z;                    // < 2^88
  if (s >= 96u) return prod ? 1ull : 0ull;
  return (unsigned long long)((prod + (((unsigned __int128)1 << s) - 1)) >> s);
}

MG_DEVICE float sample_gumbel(uint32_t r3, uint32_t i) {
  const uint32_t x = fmix32(r3 + i * 0x9E3779B1u) >> 8;
  const float t = x < (1u << 23) ? -logf(((float)x + 0.5f) * 0x1p-24f)
                                 : -log1pf(-(((float)((1u << 24) - x) - 0.5f) * 0x1p-24f));
  return -logf(t);
}

// ---------------------------------------------------------------- Per-token log-probabilities
// The log-probability of token t for a row of bf16 logits l_0 .. l_{V-1} is the MODEL's
// log-softmax: temperature 1, before top-k and top-p, natural log -- so greedy, sampled, ragged and
// scored paths give one number for one (row, token), and the numbers of a sequence add up to its
// log-likelihood.  With m the row maximum:
//   q_i   = sample_mass(bits_i, m, 1.0f)      (the nucleus rule's fixed fp32 sequence; -inf weighs 0)
//   Z^    = sum q_i                           (a 64-bit integer: the adds commute, V * 2^32 fits)
//   lnz   = logf((float)Z^ * 2^-32)
//   lp(t) = (float(l_t) - m) - lnz            (a greedy token has l_t = m: lp = -lnz)
// {m, lnz} is a function of the row's values alone -- not of a reduction order, a workgroup size or
// graph / eager launch -- and so is lp.  A target whose logit is -inf gets -inf.  A row without a
// finite maximum is outside the rule (any value may come out, nothing faults).
// Error against the real log-softmax of the same bf16 logits: Z^ / 2^32 is off from Z by at most
// eps_w * Z + V * 2^-32 (above), and Z >= 1, so ln is off by at most eps_w + V * 2^-32 = 4.4e-6 +
// V * 2^-32; the integer-to-float conversion (2^-24 relative) and an accurate logf (1 ulp of a
// result in [0, ln V]) add at most 2^-23 * (ln V + 1); l_t - m is exact while the two bf16 exponents
// are within 16 of each other and rounds to 2^-24 * |l_t - m| otherwise; the last subtraction adds
// half an ulp, 2^-24 * |lp|.  |l_t - m| <= |lp|, so in all
//   |lp^ - lp| <= 4.4e-6 + V * 2^-32 + 2^-23 * (ln V + 1) + 2^-23 * |lp|
// (2.5e-5 at V = 50257, |lp| <= 64).  The tests take four times this, as the nucleus tests do.
MG_DEVICE float logprob_lnz(unsigned long long Z) { return logf((float)Z * 0x1p-32f); }

MG_DEVICE float token_logprob(uint32_t bits, float m, float lnz) { return (bf2f(bits) - m) - lnz; }

// ---------------------------------------------------------------- Beam search
// W <= 8 beams per prompt over the log-probabilities above.  State per prompt b and beam w: a score
// s[b, w] in fp32 (the running sum of the beam's lp numbers) and a finished flag.  Start: s[b, 0] = 0,
// s[b, w > 0] = -inf, nothing finished; the W rows of a prompt hold the same prompt.
// One step, from the bf16 logits row of each (b, w):
//   a live beam offers the candidates (w, i), i < V, with  c = s[b, w] + lp_i,  lp_i =
//     token_logprob(bits_i, m, lnz) on the row's own {m, lnz} -- one fp32 add; a -inf logit gives -inf;
//   a finished beam offers the single candidate (w, pad_token) with c = s[b, w]: it stays finished
//     and its length does not grow.
// The new beams are the W best candidates of the prompt: c descending (a float compare: -0 equals
// +0), among equal c the lower w first, then the row's own order -- logit descending, index
// ascending (amax_key's order; for equal logits of one row that is the lower i).  -inf candidates
// rank last by the same tie-break.  New beam r is the rank-r candidate with parent w, token i and
// score c; it is finished if its parent was or if i is the stop token.  fp32 adds and subtractions
// are monotone, so within a row c never rises along the row's order: a row can only contribute its
// first W entries, and W * W candidates per prompt suffice.
// Error against the rule over the reals (the fp64 step of ops/reference.py) given the same scores
// going in: |c^ - c| <= (the lp bound above) + 2^-24 * |c| for the one add; the tests allow
// d = 4 x the lp bound + 2^-23 * |c| and check that no unchosen candidate beats a chosen one by more
// than the two candidates' d.
// {m, lnz} is the lse kernel's, bit for bit (row_common.h holds the shared row code); the result
// depends on the rows' values and the scores alone, not on a reduction order or graph / eager launch.

// ---------------------------------------------------------------- Speculative greedy decoding
// K = draft_len + 1 <= 8 rows per sequence and step: the last committed token and K - 1 guessed ones
// run at K consecutive positions of one KV cache, and the longest prefix of guesses that the model's
// own argmax confirms is kept.  Integers only; the output is the greedy output.  Per sequence, with
// tokens s[0 .. p] committed (p the device position) and end = T + n - 1 the column of the last token:
// Draft (prompt lookup).  For every e in 0 .. p - 1, ml(e) is the largest m <= ngram (1 .. 4) with
//   e - j >= 0 and s[e - j] == s[p - j] for every j < m.  Take the e with the largest (ml, e): the
//   longest suffix match, the most recent on ties.  If the best ml is 0 there is no draft.
//   Otherwise extend: x = s[0 .. p], and for r = 1 .. K - 1: d_r = x[e + r], then append d_r to x
//   (e + r <= p + r - 1, so the value exists: a repetition with a period below K drafts through
//   itself).  Row r carries token d_r (row 0: s[p]) at position p + r; without a draft rows
//   1 .. K - 1 carry s[p] and a flag says "no draft".
// Accept.  g_r is the argmax of row r's stored bf16 logits, first index on ties (amax_key's order,
//   the ragged greedy pick's).  a is the largest value with d_r == g_{r-1} for all 1 <= r <= a; 0
//   without a draft.  The step emits min(a + 1, end - p) tokens g_0, g_1, ... into s[p + 1 ...],
//   advances p by that count and bumps steps and emitted_hist[count].  A sequence with p == end is
//   left alone: no token, no position change, no statistics.
// Row r <= a saw exactly the committed tokens s[0 .. p + r] (its drafts were confirmed), and every
// kernel of the step computes a row from that row's inputs alone, so g_r is what plain greedy
// decoding picks at position p + r: the emitted tokens are generate()'s, bit for bit.

// ---------------------------------------------------------------- Logits processors
// Repetition, presence and frequency penalties and the no-repeat n-gram ban: an edit of one row of
// stored logits l_0 .. l_{V-1} (bf16 on the device, the tensor's own dtype on host paths) from a
// history h[0 .. n-1] of token ids, n >= 1, BEFORE anything else looks at the row.  Temperature,
// top-k, top-p and the Gumbel pass see the edited row; greedy is its argmax (first index on ties);
// a log-probability reported with a processor on is the rule above applied to the edited row.
// History: generate() -- for the token at column T of the returned sequence, h = idx[b, max(0, T -
// block_size) : T], exactly the context the model saw (n <= block_size); generate_batch() -- the row's
// own unpadded sequence s[0 .. pos].  An id outside [0, V) counts for nothing: it has no c, is never
// banned and equals nothing in an n-gram comparison, not even itself.
// Parameters (a device block of kProcParamWords int32: rp, inv, pp, fp as fp32 bits, g, 0, 0, 0):
//   rp = float32(repetition_penalty) (> 0; 1: off)       inv = float32(1.0 / repetition_penalty)
//   pp = float32(presence_penalty), fp = float32(frequency_penalty) (0: off)
//   g  = no_repeat_ngram_size (0 .. 8; 0: off)
// Penalties.  c_i = the number of j with h[j] == i.  Every i with c_i >= 1 whose logit is not -inf is
// rewritten by one fixed sequence of single correctly rounded fp32 operations (proc_penalty: no step
// may fuse with another, whatever -ffp-contract says):
//   x = float(l_i)    a = x > 0 ? x (*) inv : x (*) rp    q = fp (*) float(c_i)    q = q (+) pp
//   y = a (-) q       l_i' = y rounded to the row's dtype (bf16: round-to-nearest-even, f2bf)
// A -inf logit stays -inf; entries with c_i == 0 keep their bits; with every parameter off the
// sequence is the identity on every non-NaN value.
// No-repeat n-gram, after the penalties, if g >= 1: for every e in g-2 .. n-2 with h[e-j] == h[n-1-j]
// for all j < g-1, the logit of h[e+1] becomes -inf.  g = 1 bans every history token; n < g bans
// nothing.
// The edited row must keep a finite maximum; otherwise it is outside the rule (any token, no fault).
// The result is a function of (row, history, parameters) alone: one writer per element and phase,
// nothing accumulated in floating point, nothing kept between launches -- a replay, a warm-up or a
// repeated launch on fresh logits gives the same bits.
MG_DEVICE bf16_t proc_penalty(uint32_t bits, int c, float rp, float inv, float pp, float fp) {
  const float x = bf2f(bits);
  float a = x > 0.f ? __fmul_rn(x, inv) : __fmul_rn(x, rp);
  asm volatile("" : "+v"(a));  // a product the compiler cannot see into: nothing to contract with
  float q = __fmul_rn(fp, (float)c);
  asm volatile("" : "+v"(q));
  q = __fadd_rn(q, pp);
  return f2bf(__fsub_rn(a, q));
}

// ---------------------------------------------------------------- GELU (tanh approximation)
constexpr float kGeluK0 = 0.7978845608028654f;  // sqrt(2/pi)
constexpr float kGeluK1 = 0.044715f;

// 0.5 x (1 + tanh(u)) == x * sigmoid(2u), u = K0 (x + K1 x^3): one v_exp_f32 and one v_rcp_f32
// instead of the libm tanhf (range reduction + branches), ~4x fewer instructions in the GEMM
// epilogues.  exp2 overflows to +inf for very negative x -> rcp(inf) = 0 -> gelu -> -0, as it should.
constexpr float kGeluE0 = -2.f * kGeluK0 * 1.4426950408889634f;  // -2 K0 log2(e)
constexpr float kGeluE1 = kGeluE0 * kGeluK1;

MG_DEVICE float gelu_sigmoid(float x) {  // sigmoid(2u)
  const float x2 = x * x;
  const float e = __builtin_amdgcn_exp2f(x * __builtin_fmaf(kGeluE1, x2, kGeluE0));
  return __builtin_amdgcn_rcpf(1.f + e);
}

MG_DEVICE float gelu_f(float x) { return x * gelu_sigmoid(x); }

// d/dx [x s(x)], s = sigmoid(2u): s + 2 x s (1 - s) K0 (1 + 3 K1 x^2)
MG_DEVICE float gelu_grad_from(float x, float sg) {
  return __builtin_fmaf(2.f * kGeluK0 * x * sg * (1.f - sg), __builtin_fmaf(3.f * kGeluK1, x * x, 1.f), sg);
}
MG_DEVICE float gelu_grad(float x) { return gelu_grad_from(x, gelu_sigmoid(x)); }

// GELU and GELU' of two values with packed fp32 math (v_pk_mul_f32 / v_pk_fma_f32: two lanes'
// worth per instruction; only exp2 and rcp stay per element).  Same formulas and rounding steps as
// gelu_sigmoid / gelu_grad_from; used by the GEMM epilogue, where one wave per SIMD runs ~12 VALU
// ops per element with nothing to overlap them.
MG_DEVICE void gelu2(f32x2 x, f32x2& y, f32x2& g) {
  const f32x2 x2 = x * x;
  const f32x2 t = x * (kGeluE1 * x2 + kGeluE0);
  const f32x2 d = f32x2{1.f, 1.f} + f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
  const f32x2 sg = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  y = x * sg;
  g = (2.f * kGeluK0) * x * sg * (f32x2{1.f, 1.f} - sg) * ((3.f * kGeluK1) * x2 + 1.f) + sg;
}

// ---------------------------------------------------------------- decode projection epilogue
// One output element of the decode-time projections (gemv.hip, gemm_rows.hip; kernels.h epi codes):
// add the bias (0.f without one), GELU for epi 2, add the residual element for epi 3 (resid_elem is
// read for epi 3 only), one rounding to bf16 -- in this order, for both kernels.
MG_DEVICE bf16_t proj_epilogue(float acc, float bias, int epi, const bf16_t* resid_elem) {
  float v = acc + bias;
  if (epi == 2) v = gelu_f(v);
  if (epi == 3) v += bf2f(*resid_elem);
  return f2bf(v);
}

// ---------------------------------------------------------------- W8: int8 weight rows, power-of-two scales
// Weight-only 8-bit decode (gemv_w8, gemv.hip; ops/quant.py is the rule in torch ops).  For a weight
// matrix W [N, K] (row n = output column n) and a_n = max_k |W[n, k]|:
//   a_n == 0: s_n = 1, q[n, :] = 0;
//   else s_n = the smallest power of two with a_n / s_n <= 127, from the exponent of a_n alone: with
//     a_n = m * 2^e, m in [0.5, 1) (frexp), s_n = 2^(e - 7) if m <= 127 / 128, else 2^(e - 6) -- no log2
//     of a rounded quotient;
//   q[n, k] = clamp(rne(W[n, k] / s_n), -127, 127) as int8: the division is exact (a power of two),
//     the rounding is to nearest, halves to even.
// A non-finite weight is outside the rule (ValueError on the host).  s_n is never below 2^-126 (a
// normal fp32): a row with 0 < a_n < 2^-119 keeps |W - s q| <= s_n / 2, the exactness and the fixed point
// below, not the two bounds that need a_n / s_n > 63.5.  Consequences:
//   |W - s q| <= s_n / 2 < a_n / 127            (a_n / s_n > 63.5, and the clamp never acts: |W / s| <= 127)
//   max_k |q[n, k]| >= 64 for a non-zero row    (rne of a value above 63.5)
//   s q is exact in bf16                        (7 significant bits times a power of two)
//   quantize(s q) == (q, s)                     (max |q| in [64, 127] gives the same s; q / 1 rounds to itself)
// One output of gemv_w8 is  y[b, n] = proj_epilogue(s_n * sum[b, n]),  sum the bf16 kernel's chain with
// float(q[n, k]) in place of the bf16 weight: the same lanes (64, or 16 on the wide path), the same
// columns per lane c = 8 j + 8 L u, the same element order, the same xor fold.  Every product
// float(q) * x is exact (at most 7 significant bits times 8).  Scaling by a power of two commutes with
// every fp32 rounding, so s_n * sum equals the chain run on the bf16 values s_n * q[n, k], bit for
// bit: gemv_w8(x, q, s) == gemv(x, s q).  Precondition: no fp32 intermediate of either chain (a lane
// sum, a fold sum, s_n * sum) is subnormal or overflows -- there the two roundings differ.
// (s_n * sum + bias may contract to one fma: the product is exact, so the result is the same.)

// ---------------------------------------------------------------- KV8: int8 K / V vectors, power-of-two scales
// The int8 KV cache (kv_cache="int8" on every entry point that keeps or reads K / V; attention_kv8.hip;
// ops/quant.py snap_vectors is the rule in torch ops).  A vector u[0 .. hd-1] is the K, or separately
// the V, of one (sequence, position, layer, head): bf16 as c_attn wrote it on the GPU, the model's dtype
// on the CPU.  With a = max |u|:
//   a not finite (a NaN or an inf anywhere in u): s = NaN, q = 0 -- every dequantized element of the
//     vector is NaN, so a blown-up activation stays visible and stays in its own (sequence, head);
//   a == 0: s = 1, q = 0;
//   otherwise the W8 rule unchanged: s from frexp of a (2^(e-7), or 2^(e-6) when m > 127/128), never
//     below 2^-126, and q = clamp(rne(u / s), -127, 127).
// snap(u) = s * q is exact in bf16, and snapping it again returns (q, s).  The W8 consequences hold per
// vector (|u - s q| <= s / 2 < a / 127 and max |q| >= 64 when a >= 2^-119).
// The KV8 model: every attention uses snap(K) and snap(V) in place of K and V -- prefill and decode, GPU
// and CPU; Q is untouched, and a new token's own K / V are snapped for its own query too.  One model on
// every path: the prefill snaps the prompt's K / V thirds in place before its attention (kv8_store), a
// decode step snaps the new row (attention_decode_kv8 in LDS, or kv8_store in place with the switch
// off).  Storage per layer: kq int8 [B, 2, H, Tmax, hd] and ks fp32 [B, 2, H, Tmax], 2 D + 8 H bytes per
// token against the bf16 cache's 6 D (whole qkv rows).
// float(q) * s is exact and equals the snapped bf16 value, and attention_decode_kv8 runs the bf16 kernel's
// fma chains on it -- no scale is folded out of a sum, so there is no precondition: it equals
// attention_decode on the snapped row over a bf16 cache of the dequantized rows bit for bit.
// The rows of a group (speculative verify rows) are snapped before any row of the group reads them, and a
// beam reorder moves (q, s) pairs unchanged.
// Limits: use_cache=False has no cache and is a ValueError; one scale per vector, no per-channel or
// grouped scales; int8 only, no fp8 or 4-bit; hd % 8 == 0, hd <= 128, Tmax <= 4096; the quality of
// the KV8 model on pretrained weights is not measured.

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Host: f(std::true_type{}) or f(std::false_type{}) for a run-time flag that is a template argument
// of the kernel f launches (the decode projections' weight-load policy)
template <class F>
inline void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace mg

// Debug builds (build_ext.py --debug => -DMG_DEBUG, loaded with MINGPT_EXT_SO): data-dependent
// indices (token ids, targets) are range-checked on the device.  A bad index is clamped to a safe
// value (no out-of-bounds access, no GPU fault) and recorded with a vector atomic in a device
// error word (hipMalloc'd, mg::debug_err_word(); nullptr in release builds, where the check
// compiles away).  The host reads and clears it after each op (mg::debug_error_bits,
// ops/_ext.py MINGPT_DEBUG_CHECKS=1) and raises naming the op.
namespace mg {
unsigned int* debug_err_word();
}
#ifdef MG_DEBUG
#define MG_CHECK_INDEX(var, ok, safe, err, bit) \
  if (!(ok)) {                                  \
    atomicOr((err), (bit));                     \
    (var) = (safe);                             \
  }
#else
#define MG_CHECK_INDEX(var, ok, safe, err, bit)
#endif
