// Chunk attention over the KV cache for gfx950 (CDNA4, MI355X): Tq new tokens per sequence, at
// positions base .. base + Tq - 1, attend to the `base` cached keys plus the chunk itself, and their
// K/V rows are appended to the cache.  (Square-causal training forward: attention_fwd.hip; one query
// per sequence: attention.hip.)  models/generation.py extends a cache that already holds a prompt's
// prefix with it instead of prefilling from row 0 (`_GpuCache.extend`).
//
// Append and reads: TWO stream-ordered launches.  attn_extend_append_kernel copies the K and V thirds
// of qkv_new to cache rows [base, base + Tq) bit for bit (the Q third of a cache row is never
// written); the attention launch after it reads every key and value from the cache and writes no
// cache byte, so no workgroup reads a row that another workgroup of its launch writes.  The other
// way -- keys >= base from qkv_new, one designated workgroup per (b, h) appending, as the grouped
// decode kernel does -- was not taken: `base` is not tile-aligned, so the tile that straddles it
// would stage rows from two tensors with a per-row source select, and every tile would carry the
// second descriptor; here a tile has one source and one descriptor, and the append is one small
// copy per layer in front of a launch that is never captured per token.
//
// Stale rows: the cache comes from torch.empty, rows at or past base + Tq may hold NaN / inf bits.
// Every K / V load goes through a buffer descriptor over the sequence's rows [0, base + Tq) only
// (kv_rsrc): a row past it reads as zeros, and its scores are masked as well.  A 16-byte chunk whose
// columns lie at or past hd (LDS images are 64 columns wide) is staged as zeros too: it would
// otherwise read the next head, the next third or the next row's -- stale -- Q third, and 0 x NaN in
// an MFMA is NaN.
//
// Attention kernel (FA2 structure of the training forward, no dropout):
//  * grid (query block, b * h, key split); workgroup = 4 waves = 128 queries of one (b, h), each
//    wave 32 of them; a wave whose queries are all past Tq issues no MFMA but stages tiles.
//  * Q fragments (from qkv_new) live in VGPRs, pre-multiplied by log2(e) / sqrt(hd).
//  * 64-key K / V tiles double-buffered through LDS (register staging: tile t + 1's loads are in
//    flight during tile t's MFMAs), one barrier per tile.
//  * S^T = K Q^T with v_mfma_f32_32x32x16_bf16: the query is on the lane, the softmax statistics are
//    lane-local; the running max rides in as the MFMA's C operand and moves only when a tile's row
//    sum leaves [2^-60, 2^60] (ext_tile).  P goes to bf16 in registers as the B operand of
//    O^T = V^T P^T; V^T fragments come from LDS with ds_read_b64_tr_b16.
//  * the causal limit of query r is key base + r: tiles wholly below base + (the wave's first query)
//    run unmasked, tiles that straddle the diagonal take the masked body (a per-lane `lim`), tiles
//    past the wave's last query are skipped per wave.
//  * key splits: the shape that matters is few queries against many keys (Tq 1..64, base in the
//    hundreds), where a workgroup per (query block, b, h) leaves most of the chip idle.  Split s
//    takes `tps` whole 64-key tiles; with S > 1 every split writes its unnormalised fp32 state
//    (m, l, O) of the rows below Tq to a workspace and attn_extend_combine_kernel -- a launch of its
//    own: a launch boundary cannot hang, and this op is not captured per token -- rescales, sums in
//    split order and stores bf16.  S = 1 stores `out` directly.  S depends on the shapes and the CU
//    count only (attention_extend_splits), so equal calls give equal bits, and a row's bits depend
//    on its own sequence only.
//  * instantiated per number of 16-column MFMA k-steps, nks_for(hd).
//
// KV8 (attention_extend_kv8): the same three launches on the int8 cache of kernels.h, kq [B, 2, H, Tmax,
// hd] and ks [B, 2, H, Tmax].  Only the append and the tile staging differ.
//  * attn_extend_snap_kernel appends the KV8 rule's (q, s) of the chunk's K and V vectors at positions
//    base .. base + Tq - 1 and leaves qkv_new alone.  A kernel of its own beside kv8_store's, not that
//    kernel with an offset and a flag: this one writes no qkv byte and never replicates rows, and it
//    stays in this file with this file's flags; the rule itself is kv8_common.h's one copy.
//  * attn_extend_kernel<NKS, KV>, KV = 16 (hd % 16 == 0) or 8 bytes per load.  A 64-key tile of one
//    (b, K | V, h) plane is 64 * hd contiguous bytes and 64 scale words: half the bf16 tile's bytes and no
//    strided rows.  Thread i of the workgroup loads bytes [(i + 256 c) * KV, + KV) of the tile, so every
//    load instruction of a wave covers one contiguous 64 * KV bytes, and the scale word of that chunk's
//    key with a 4-byte load of its own (at most 16 lanes share a word: served by one cache line; a
//    cross-wave exchange of 64 scale words through LDS would cost a barrier per tile).  Both planes go
//    through descriptors that end at key base + Tq, so a key past it reads q = 0, s = 0 and stages 0.
//    The chunk is dequantized in registers -- float(q) * s is exact, it IS the bf16 value of the
//    snapped row, and a NaN scale makes the vector NaN -- at store time, after the current tile's
//    MFMAs, so what waits in registers under them is the raw int8 chunk and its scale: (KV / 4 + 1)
//    registers per load against the bf16 staging's 4 per 8 columns.  The stores write the swizzled
//    images the bf16 staging writes; fragment offsets, ext_tile, mask, partials and combine are the
//    one copy above, and the key split is the same function, so out equals attention_extend on the
//    snapped chunk over the dequantized cache bit for bit.  Image columns at or past hd are covered by
//    no load: both buffers are zeroed once before the first tile when hd < 32 NO.
//
// Ragged (attention_extend_ragged; the contract and the plan tables: kernels.h): every sequence has its
// own (base_b, Tq_b), the new rows are packed, and the shape that matters is a chat turn -- 5 to 50 new
// rows behind hundreds of cached ones, another amount of each per sequence (generate_batch(reuse_cache=
// True), `_GpuCache.extend_ragged`).  attn_extend_kernel's workgroup is 128 queries of one (b, h), a wave
// per 32: three of its four waves would only stage tiles there, and its grid and split count know one
// (base, Tq).  So the same three launches, but
//  * a flat work list: a 1-D grid over items (sequence, 32-query block, key split) x heads from a plan the
//    host builds once per call; no workgroup exists for padding, and a sequence's split count S_b comes
//    from its own key count, so a long history beside short ones is split and they are not.  An output
//    block owns as many partial slots as it has splits (no max-S padding); one with a single split stores
//    `out` directly and takes no part in the combine, which walks each block's own count in split order.
//  * the four waves split the KEYS: all hold the same 32 queries (Q fragments in VGPRs) and wave w runs
//    tiles t0 + w, t0 + w + 4, ... of the item's key range through ext_tile, staging its own tiles into
//    its own K / V image (LDS: 4 waves x 2 images, 128 KiB at hd = 128), masked body only from the tile
//    that reaches past the block's first query.  The four (m, l, O) states are folded through LDS in wave
//    order (attention_shared.hip's arrangement on a causal chunk), so with 1 to 32 queries per block every
//    wave issues MFMAs.  A row below a wave's first key has weight zero in the fold.
//  * the append reads the per-row (sequence, position) tables the packed embedding needs anyway.
#include "attn_common.h"
#include "kernels.h"
#include "kv8_common.h"

using namespace mg;
using namespace mg::attn;
using namespace mg::kv8;

namespace {

constexpr int kExtSplitsMax = 16;

struct ExtArgs {
  const bf16_t* qkv_new;  // [B * Tq, 3D]
  const bf16_t* cache;    // [B, Tmax, 3D], rows [base, base + Tq) already appended
  // KV8 (attention_extend_kv8): the int8 cache in place of `cache`, positions [base, base + Tq) appended
  const int8_t* kq;       // [B, 2, H, Tmax, hd]
  const float* ks;        // [B, 2, H, Tmax]
  bf16_t* out;            // [B * Tq, D]
  float* part_ml;         // S > 1: [nqb][B * H][S][128][2] {m, l}
  float* part_o;          // S > 1: [nqb][B * H][S][128][hd]
  int B, Tq, H, hd, D, base;
  long Tmax;
  int S, tps;             // key splits and whole 64-key tiles per split
  float scale_log2;       // log2(e) / sqrt(hd)
};

// K and V thirds of qkv_new row b * Tq + r -> cache row base + r of sequence b, 16 bytes a thread
__global__ __launch_bounds__(256) void attn_extend_append_kernel(const bf16_t* __restrict__ qkv_new,
                                                                 bf16_t* __restrict__ cache, int B, int Tq,
                                                                 int D, long Tmax, int base) {
  const int cpr = D >> 2;  // 16-byte chunks of a row's K and V thirds (2 D elements)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Tq * cpr) return;
  const long m = i / cpr;
  const int c = (int)(i % cpr);
  const long b = m / Tq, r = m % Tq;
  const long ld = 3L * D;
  st16(cache + (b * Tmax + base + r) * ld + D + 8 * c, ld16(qkv_new + m * ld + D + 8 * c));
}

// KV8 append: the rule's (q, s) of the K and V vectors of qkv_new row b * Tq + r -> position base + r of
// the (b, K | V, h) planes.  One thread per 16-byte chunk; the dch = hd / 8 chunks of a vector sit in
// consecutive threads of one workgroup (256 / dch whole vectors per workgroup) and meet through LDS.
// Vector v = ((b * Tq + r) * 2 + w) * H + h walks consecutive addresses of the K and V thirds.
__global__ __launch_bounds__(256) void attn_extend_snap_kernel(const bf16_t* __restrict__ qkv_new,
                                                               int8_t* __restrict__ kq, float* __restrict__ ks,
                                                               long NV, int Tq, int H, int hd, long Tmax, int base) {
  __shared__ uint32_t cm[256];
  const int dch = hd >> 3, vpb = 256 / dch;
  const int lv = threadIdx.x / dch, c = threadIdx.x % dch;
  const long v = (long)blockIdx.x * vpb + lv;
  const bool on = lv < vpb && v < NV;
  const int h = (int)(v % H), w = (int)((v / H) % 2);
  const long m = v / (2L * H);
  const uint4 raw = on ? ld16(qkv_new + (m * 3 + 1 + w) * H * hd + h * hd + c * 8) : make_uint4(0u, 0u, 0u, 0u);
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
  const long b = m / Tq, r = m % Tq;
  const long row = ((b * 2 + w) * H + h) * Tmax + base + r;
  *reinterpret_cast<uint2*>(kq + row * hd + c * 8) = q8;
  if (c == 0) ks[row] = s;
}

// One 64-key tile for one wave's 32 queries: S'^T = K Q^T - m, p = exp2(S'), O^T += V^T P^T.  m moves
// only when a tile's row sum leaves [lo, 2^60] (lo = 2^-60 on a split's first tile, where m starts
// at 0, else 0); the tile is then recomputed against its row max (K is still in LDS).
template <int NKS, bool MASK>
MG_DEVICE void ext_tile(const char* sk, const char* sv, const int (&ko)[NKS], const bf16x8 (&qf)[NKS],
                        f32x16 (&o)[(NKS + 1) / 2], f32x16& negm, float& m, float& l, bool first, int lim,
                        int ta0, int tb0, int ta1, int tb1) {
  constexpr int NO = (NKS + 1) / 2;
  constexpr int HALF = 64 * ROWB;
  f32x16 s[2];
  auto scores = [&](int lim) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_row_at(sk + sub * 32 * ROWB, ko[0]), qf[0], negm, 0, 0, 0);
#pragma unroll
      for (int ks = 1; ks < NKS; ++ks)
        s[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_row_at(sk + sub * 32 * ROWB, ko[ks]), qf[ks],
                                                         s[sub], 0, 0, 0);
    }
    if constexpr (MASK) {  // key = k0 + c(sub, r) + 4 h32, c a constant: one compare per score
      asm volatile("" : "+v"(lim));  // the compares stay below the MFMAs (SGPR pressure otherwise)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          s[sub][r] = (sub * 32 + (r & 3) + 8 * (r >> 2) > lim) ? kNegBig : s[sub][r];
    }
  };
  auto expsum = [&]() {
    float rs = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = fexp2(s[sub][r]);
        rs += p;
        s[sub][r] = p;
      }
    return rs;
  };
  scores(lim);
  float rs = expsum();
  const float lo = first ? 8.673617379884035e-19f : 0.f;  // 2^-60
  if (__builtin_expect(__any(!(rs <= 1.152921504606847e18f && rs >= lo)), 0)) {  // 2^60; inf / nan
    int lim2 = lim;
    asm volatile("" : "+v"(lim2));
    scores(lim2);
    float mx = s[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[1][r]);
    mx = max_xor32(mx);
    // a split's first tile may move m down as well (nothing accumulated yet); later tiles up only
    const float d = first ? mx : fmaxf(mx, 0.f);
    const float alpha = first ? 1.f : fexp2(-d);
    l *= alpha;
#pragma unroll
    for (int n = 0; n < NO; ++n) o[n] *= alpha;
    m += d;
#pragma unroll
    for (int r = 0; r < 16; ++r) negm[r] = -m;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[sub][r] -= d;
    rs = expsum();
  }
  l += rs;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const bf16x8 pf = pack_frag(s[sub], st);
      const int rb = (sub * 32 + 16 * st) * ROWB;  // 16-row aligned: an immediate
#pragma unroll
      for (int n = 0; n < NO; ++n) {
        const char* vb = sv + (n >> 1) * HALF + rb;
        o[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            (n & 1) ? lds_tr_at(vb, ta1, tb1) : lds_tr_at(vb, ta0, tb0), pf, o[n], 0, 0, 0);
      }
    }
}

// what a thread holds of tile t + 1 under tile t's MFMAs
template <int NC>
struct ExtRegs {  // bf16 rows: 16-byte chunks of K and V
  uint4 k[NC], v[NC];
};
template <int NL, int CB>
struct ExtRegsKv8 {  // int8 planes: CB-byte chunks and the scale of each chunk's key
  typedef uint32_t chunk __attribute__((ext_vector_type(CB / 4)));
  chunk k[NL], v[NL];
  float sk[NL], sv[NL];
};

// KV = 0: bf16 cache rows.  KV = 16 / 8: the int8 cache (kq / ks), staged with 16-byte loads (hd % 16 ==
// 0) or 8-byte loads -- the KV8 staging in the file header.
template <int NKS, int KV>
__global__ __launch_bounds__(256, NKS > 4 ? 1 : 2) void attn_extend_kernel(const ExtArgs a) {
  constexpr int NH = (NKS + 3) / 4;   // 64-column halves of the LDS images
  constexpr int NO = (NKS + 1) / 2;   // 32-column O^T accumulator tiles
  constexpr int HALF = 64 * ROWB;     // one 64-row, 64-column image
  constexpr int TILE = NH * HALF;     // one K or V tile
  constexpr int NC = 2 * NH;          // 16-byte chunks per thread per tile per matrix
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE];  // K0 V0 K1 V1
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h32 = lane >> 5, l32 = lane & 31;
  const int qb = blockIdx.x, bh = blockIdx.y, sp = blockIdx.z;
  const int b = bh / a.H, hh = bh % a.H;
  const long ld = 3L * a.D;
  const int q0 = qb * 128;
  const int qend = min(a.Tq, q0 + 128);            // the block's queries are rows [q0, qend)
  const int ntb = (a.base + qend + 63) / 64;       // key tiles the block's last query sees
  const int t0 = sp * a.tps, t1 = min(t0 + a.tps, ntb);  // this split's tiles [t0, t1)

  // tile staging: chunk c of this thread -> (half, row, 16-byte column chunk).  Buffer loads through
  // a per-tile descriptor whose range ends at the sequence's row base + Tq (file header); a chunk
  // whose columns are at or past hd is staged as zeros.
  uint32_t voff[NC], sdst[NC];
  bool cok[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int idx = threadIdx.x + 256 * c;
    const int hf = idx >> 9, rem = idx & 511;
    voff[c] = (uint32_t)(((rem >> 3) * ld + hf * 64 + (rem & 7) * 8) * 2);
    sdst[c] = hf * HALF + lds_off(rem >> 3, rem & 7);
    cok[c] = hf * 64 + (rem & 7) * 8 < a.hd;
  }
  const bf16_t* seq = a.cache + (long)b * a.Tmax * ld;
  const uint64_t seq_bytes = (uint64_t)(a.base + a.Tq) * ld * 2;  // rows [0, base + Tq) of this sequence
  const uint64_t kcol = (uint64_t)(a.D + hh * a.hd) * 2;
  auto load_tile = [&](auto& rg, int k0) {
    uint4 (&rk)[NC] = rg.k;
    uint4 (&rv)[NC] = rg.v;
    const uint64_t off = kcol + (uint64_t)k0 * ld * 2;
    const __amdgpu_buffer_rsrc_t dk = kv_rsrc(seq, seq_bytes, off);
    const __amdgpu_buffer_rsrc_t dv = kv_rsrc(seq, seq_bytes, off + (uint64_t)a.D * 2);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const uint4 k = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(dk, voff[c], 0, 0));
      const uint4 v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(dv, voff[c], 0, 0));
      rk[c] = cok[c] ? k : make_uint4(0, 0, 0, 0);
      rv[c] = cok[c] ? v : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&](char* dst, const auto& rg) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      *reinterpret_cast<uint4*>(dst + sdst[c]) = rg.k[c];
      *reinterpret_cast<uint4*>(dst + TILE + sdst[c]) = rg.v[c];
    }
  };

  // KV8 staging (file header).  Load c of a thread is chunk idx = thread + 256 c of the tile's 64 * cpr
  // chunks, cpr = hd / CB per key: key row idx / cpr, columns (idx % cpr) * CB.  qok: the chunk exists.
  constexpr int CB = KV ? KV : 16;              // bytes per load
  constexpr int NL = (NKS * 4 + CB - 1) / CB;   // loads per thread and matrix at most: 64 * 16 NKS / CB / 256
  const int cpr = max(a.hd / CB, 1);
  uint32_t qdst[NL], qkey[NL];                  // image offset of the chunk's first 8 columns; its key row
  bool qok[NL];
#pragma unroll
  for (int c = 0; c < NL; ++c) {
    const int idx = threadIdx.x + 256 * c, row = min(idx / cpr, 63), col = (idx % cpr) * CB;
    qok[c] = idx < 64 * cpr;
    qkey[c] = row;
    qdst[c] = (col >> 6) * HALF + lds_off(row, (col >> 3) & 7);
  }
  const long plane = ((long)b * 2 * a.H + hh) * a.Tmax;  // K; V is H * Tmax keys behind it
  const long vplane = (long)a.H * a.Tmax;
  auto load_kv8 = [&](auto& rg, int k0) {
    const uint64_t qbytes = (uint64_t)(a.base + a.Tq) * a.hd, qoff = (uint64_t)k0 * a.hd;
    const uint64_t sbytes = (uint64_t)(a.base + a.Tq) * 4, soff = (uint64_t)k0 * 4;
    const __amdgpu_buffer_rsrc_t dk = kv_rsrc(a.kq + plane * a.hd, qbytes, qoff);
    const __amdgpu_buffer_rsrc_t dv = kv_rsrc(a.kq + (plane + vplane) * a.hd, qbytes, qoff);
    const __amdgpu_buffer_rsrc_t dsk = kv_rsrc(a.ks + plane, sbytes, soff);
    const __amdgpu_buffer_rsrc_t dsv = kv_rsrc(a.ks + plane + vplane, sbytes, soff);
    typedef typename ExtRegsKv8<NL, CB>::chunk chunk;
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      if (qok[c]) {
        const uint32_t off = (uint32_t)(threadIdx.x + 256 * c) * CB;
        if constexpr (CB == 16) {
          rg.k[c] = __builtin_bit_cast(chunk, __builtin_amdgcn_raw_buffer_load_b128(dk, off, 0, 0));
          rg.v[c] = __builtin_bit_cast(chunk, __builtin_amdgcn_raw_buffer_load_b128(dv, off, 0, 0));
        } else {
          rg.k[c] = __builtin_bit_cast(chunk, __builtin_amdgcn_raw_buffer_load_b64(dk, off, 0, 0));
          rg.v[c] = __builtin_bit_cast(chunk, __builtin_amdgcn_raw_buffer_load_b64(dv, off, 0, 0));
        }
        rg.sk[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dsk, qkey[c] * 4, 0, 0));
        rg.sv[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dsv, qkey[c] * 4, 0, 0));
      }
    }
  };
  auto store_chunk = [&](char* img, uint32_t dst, const auto& u, float sc) {
    float f[8];
    dequant8(make_uint2(u[0], u[1]), sc, f);
    *reinterpret_cast<uint4*>(img + dst) = pack8(f);
    if constexpr (CB == 16) {  // columns 8 .. 15 of the chunk: the neighbouring image chunk
      dequant8(make_uint2(u[2], u[3]), sc, f);
      *reinterpret_cast<uint4*>(img + (dst ^ 16)) = pack8(f);
    }
  };
  auto store_kv8 = [&](char* dst, const auto& rg) {
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      if (qok[c]) {
        store_chunk(dst, qdst[c], rg.k[c], rg.sk[c]);
        store_chunk(dst + TILE, qdst[c], rg.v[c], rg.sv[c]);
      }
    }
  };
  using Regs = std::conditional_t<KV != 0, ExtRegsKv8<NL, CB>, ExtRegs<NC>>;
  auto load = [&](Regs& rg, int k0) {
    if constexpr (KV != 0) load_kv8(rg, k0);
    else load_tile(rg, k0);
  };
  auto store = [&](char* dst, const Regs& rg) {
    if constexpr (KV != 0) store_kv8(dst, rg);
    else store_tile(dst, rg);
  };

  // per-lane fragment offsets: K rows l32 (+32 per sub: an immediate), chunk 2 ks + h32;
  // V^T transposed reads rows 4 h32 + q (+8), columns (n & 1) * 32 + cb + 4 p
  int ko[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) ko[ks] = (ks >> 2) * HALF + lds_off(l32, (2 * ks + h32) & 7);
  const int trq = (lane & 15) >> 2, trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const int ta0 = tr_off(4 * h32 + trq, trc), tb0 = tr_off(8 + 4 * h32 + trq, trc);
  const int ta1 = tr_off(4 * h32 + trq, 32 + trc), tb1 = tr_off(8 + 4 * h32 + trq, 32 + trc);

  // this lane's query: row myr of the chunk, position base + myr; a lane past Tq holds a zero query
  // under the last row's limit and stores nothing
  const int wave_r = q0 + 32 * w;
  const int myr = wave_r + l32;
  const bool live = myr < a.Tq;
  const int wave_first = a.base + wave_r;                    // position of the wave's first query
  const int wave_last = a.base + min(wave_r + 31, a.Tq - 1);  // ... and of its last one
  const int mypos = a.base + min(myr, a.Tq - 1);
  const bf16_t* qrow = a.qkv_new + ((long)b * a.Tq + min(myr, a.Tq - 1)) * ld + hh * a.hd;
  bf16x8 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int d = ks * 16 + 8 * h32;
    const uint4 u = (live && d < a.hd) ? ld16(qrow + d) : make_uint4(0, 0, 0, 0);
    float f[8];
    unpack8(u, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= a.scale_log2;
    qf[ks] = __builtin_bit_cast(bf16x8, pack8(f));
  }
  f32x16 o[NO], negm = f32x16{0};
#pragma unroll
  for (int n = 0; n < NO; ++n) o[n] = f32x16{0};
  float m = 0.f, l = 0.f;

  if (t0 < t1) {  // (an empty split of a short block stages nothing and writes neutral partials)
    if constexpr (KV != 0) {
      // image columns hd .. 32 NO - 1 (K fragments read below 16 NKS, V^T fragments below 32 NO) are
      // never staged: zero both buffers once
      if (a.hd < 32 * NO) {
        for (int i = threadIdx.x * 16; i < 4 * TILE; i += 256 * 16) *reinterpret_cast<uint4*>(smem + i) = make_uint4(0, 0, 0, 0);
        __syncthreads();
      }
    }
    {
      Regs rg;
      load(rg, t0 * 64);
      store(smem, rg);
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
      const int it = t - t0;
      const char* sk = smem + (it & 1) * 2 * TILE;
      const char* sv = sk + TILE;
      const bool more = t + 1 < t1;
      Regs rg;
      if (more) load(rg, (t + 1) * 64);
      const int k0 = t * 64;
      if (k0 <= wave_last && wave_r < a.Tq) {
        const int lim = mypos - k0 - 4 * h32;
        // the causal mask only on the tiles that straddle the diagonal (separate bodies)
        if (k0 + 63 > wave_first) ext_tile<NKS, true>(sk, sv, ko, qf, o, negm, m, l, t == t0, lim, ta0, tb0, ta1, tb1);
        else ext_tile<NKS, false>(sk, sv, ko, qf, o, negm, m, l, t == t0, lim, ta0, tb0, ta1, tb1);
      }
      if (more) store(smem + ((it + 1) & 1) * 2 * TILE, rg);
      __syncthreads();
    }
  }

  const float lt = sum_xor32(l);
  if (!live) return;
  if (a.S == 1) {  // the whole key range: normalise and store
    const float inv = 1.f / lt;
    bf16_t* orow = a.out + ((long)b * a.Tq + myr) * a.D + hh * a.hd;
#pragma unroll
    for (int n = 0; n < NO; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = n * 32 + 8 * g + 4 * h32;
        if (d < a.hd)
          *reinterpret_cast<uint2*>(orow + d) = make_uint2(pack2(o[n][4 * g] * inv, o[n][4 * g + 1] * inv),
                                                           pack2(o[n][4 * g + 2] * inv, o[n][4 * g + 3] * inv));
      }
    return;
  }
  // this split's state of row myr: {m, l} and the unnormalised O.  A row that saw no key of the
  // split (no tile, or its position lies below the split's first key) has weight zero: m = -big
  const bool seen = t0 < t1 && mypos >= t0 * 64;
  const long slot = (((long)qb * gridDim.y + bh) * a.S + sp) * 128 + (myr - q0);
  if (h32 == 0) *reinterpret_cast<float2*>(a.part_ml + 2 * slot) = make_float2(seen ? m : kNegBig, seen ? lt : 0.f);
  float* prow = a.part_o + slot * a.hd;
#pragma unroll
  for (int n = 0; n < NO; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = n * 32 + 8 * g + 4 * h32;
      if (d < a.hd)
        *reinterpret_cast<float4*>(prow + d) = seen ? make_float4(o[n][4 * g], o[n][4 * g + 1], o[n][4 * g + 2], o[n][4 * g + 3])
                                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// out row = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s, M = max_s m_s, in split order: a thread
// per (row, 4 columns).  Split 0 holds key 0, which every row sees, so M is a real max.
__global__ __launch_bounds__(256) void attn_extend_combine_kernel(const ExtArgs a) {
  const int qb = blockIdx.y, bh = blockIdx.z;
  const int q0 = qb * 128, rows = min(a.Tq - q0, 128), hd4 = a.hd >> 2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * hd4) return;
  const int r = i / hd4, d = (i % hd4) * 4;
  const long slot0 = ((long)qb * gridDim.z + bh) * a.S * 128 + r;
  float ms[kExtSplitsMax], M = kNegBig;
#pragma unroll
  for (int s = 0; s < kExtSplitsMax; ++s) {
    ms[s] = s < a.S ? a.part_ml[2 * (slot0 + 128L * s)] : kNegBig;
    M = fmaxf(M, ms[s]);
  }
  float L = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int s = 0; s < kExtSplitsMax; ++s) {
    if (s < a.S) {
      const float wgt = fexp2(ms[s] - M);
      const float4 v = *reinterpret_cast<const float4*>(a.part_o + (slot0 + 128L * s) * a.hd + d);
      L += wgt * a.part_ml[2 * (slot0 + 128L * s) + 1];
      acc.x += wgt * v.x;
      acc.y += wgt * v.y;
      acc.z += wgt * v.z;
      acc.w += wgt * v.w;
    }
  }
  const float inv = 1.f / L;
  const int b = bh / a.H, hh = bh % a.H;
  bf16_t* orow = a.out + ((long)b * a.Tq + q0 + r) * a.D + hh * a.hd + d;
  *reinterpret_cast<uint2*>(orow) = make_uint2(pack2(acc.x * inv, acc.y * inv), pack2(acc.z * inv, acc.w * inv));
}

// ------------------------------------------------------------------------------- ragged (file header)
struct RagArgs {
  const bf16_t* qkv_new;  // [M, 3D] packed rows
  const bf16_t* cache;    // [B, Tmax, 3D], every sequence's new rows already appended
  bf16_t* out;            // [M, D]
  float* part_ml;         // [slots * H][32][2] {m, l}
  float* part_o;          // [slots * H][32][hd]
  const int* seq;         // plan tables (kernels.h): [B][8], [items][4], [combs][4]
  const int* items;
  const int* combs;
  int B, M, H, hd, D, slots;
  long Tmax;
  float scale_log2;
};

// One sequence's row of the plan, checked against the tensors: the plan is the caller's tensor, and a plan
// of other lists must not send a load or a store outside them (the workgroup then does nothing).
struct RagSeq {
  int cu, base, Tq, tps;
  bool ok;
};
MG_DEVICE RagSeq rag_seq(const RagArgs& a, int b, int qb, int cnt, int pbase) {
  RagSeq s{0, 0, 1, 1, false};
  if ((unsigned)b >= (unsigned)a.B) return s;
  const int* sq = a.seq + 8 * b;
  s.cu = sq[0]; s.base = sq[1]; s.Tq = sq[2]; s.tps = sq[4];
  s.ok = s.cu >= 0 && s.base >= 0 && s.Tq >= 1 && (long)s.cu + s.Tq <= a.M && (long)s.base + s.Tq <= a.Tmax &&
         qb >= 0 && (long)qb * 32 < s.Tq && s.tps >= 1 && cnt >= 1 && cnt <= kExtSplitsMax &&
         (cnt == 1 || (pbase >= 0 && (long)pbase + cnt <= a.slots));
  return s;
}

// K and V thirds of packed row m -> cache row row_pos[m] of sequence row_seq[m], 16 bytes a thread
__global__ __launch_bounds__(256) void attn_extend_ragged_append_kernel(const bf16_t* __restrict__ qkv_new,
                                                                        bf16_t* __restrict__ cache,
                                                                        const int* __restrict__ row_seq,
                                                                        const int* __restrict__ row_pos, int M, int B,
                                                                        int D, long Tmax) {
  const int cpr = D >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * cpr) return;
  const long m = i / cpr;
  const int c = (int)(i % cpr);
  const int b = row_seq[m], p = row_pos[m];
  if ((unsigned)b >= (unsigned)B || p < 0 || p >= Tmax) return;
  const long ld = 3L * D;
  st16(cache + ((long)b * Tmax + p) * ld + D + 8 * c, ld16(qkv_new + m * ld + D + 8 * c));
}

// One item (sequence, 32-query block, key split) of the plan and one head: the four waves hold the same
// 32 queries and take the split's 64-key tiles t0 + w, t0 + w + 4, ..., each wave staging its own tiles
// into its own K / V image; the four states are folded through LDS in wave order and wave 0 stores `out`
// (one split) or the split's partial.  PF: how much of the wave's next tile waits in registers under the
// current one's MFMAs -- 2: K and V, 1: K (V is loaded once the image is free), 0: nothing -- the most each
// instantiation holds without scratch (launch_ragged's callers).
template <int NKS, int PF>
__global__ __launch_bounds__(256, NKS > 4 ? 1 : 2) void attn_extend_ragged_kernel(const RagArgs a) {
  constexpr int NH = (NKS + 3) / 4;   // 64-column halves of the LDS images
  constexpr int NO = (NKS + 1) / 2;   // 32-column O^T accumulator tiles
  constexpr int HALF = 64 * ROWB;     // one 64-row, 64-column image
  constexpr int TILE = NH * HALF;     // one K or V tile
  constexpr int NC = 8 * NH;          // 16-byte chunks per lane per tile per matrix (a wave stages its own tile)
  constexpr int FOLD_O = NO * 8 * 32 * 16;  // one wave's O for the fold: [NO * 8 float4 columns][32 queries]
  static_assert(3 * (FOLD_O + 32 * 8) <= 8 * TILE, "the fold reuses the tile regions");
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];  // per wave: K, V
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h32 = lane >> 5, l32 = lane & 31;
  const int item = blockIdx.x / a.H, hh = blockIdx.x % a.H;
  const int* it = a.items + 4 * item;
  const int b = it[0], qb = it[1], sp = it[2] & 0xffff, cnt = it[2] >> 16, pbase = it[3];
  const RagSeq sq = rag_seq(a, b, qb, cnt, pbase);
  if (!sq.ok || sp >= cnt) return;  // uniform: before any barrier
  const int base = sq.base, Tq = sq.Tq;
  const long ld = 3L * a.D;
  const int q0 = qb * 32;
  const int qend = min(Tq, q0 + 32);            // the block's queries are rows [q0, qend) of the sequence
  const int ntb = (base + qend + 63) / 64;      // key tiles the block's last query sees
  const int t0 = sp * sq.tps, t1 = min(t0 + sq.tps, ntb);  // this split's tiles [t0, t1)

  // tile staging: chunk c of this lane -> (half, row, 16-byte column chunk), through a per-tile descriptor
  // that ends at the sequence's row base + Tq (file header); columns at or past hd are staged as zeros
  // Chunk c = 8 hf + cc of a lane is row (lane >> 3) + 8 cc, 16-byte column chunk lane & 7 of half hf: one
  // per-lane offset plus a wave-uniform step (added into the VGPR offset: the descriptor's range check
  // must see it), and the swizzle of row r + 8 cc depends on cc's parity only -- two image offsets
  const int r0 = lane >> 3, ch = lane & 7;
  const uint32_t voff = (uint32_t)((r0 * ld + ch * 8) * 2);
  const uint32_t sd[2] = {(uint32_t)lds_off(r0, ch), (uint32_t)(lds_off(r0 + 8, ch) - 8 * ROWB)};
  const bool cok[2] = {ch * 8 < a.hd, 64 + ch * 8 < a.hd};
  const bf16_t* seq = a.cache + (long)b * a.Tmax * ld;
  const uint64_t seq_bytes = (uint64_t)(base + Tq) * ld * 2;  // rows [0, base + Tq) of this sequence
  const uint64_t kcol = (uint64_t)(a.D + hh * a.hd) * 2;
  auto load_mat = [&](uint4 (&r)[NC], int k0, bool vmat) {  // K or V of the tile at key k0
    const __amdgpu_buffer_rsrc_t d = kv_rsrc(seq, seq_bytes, kcol + (uint64_t)k0 * ld * 2 + (vmat ? (uint64_t)a.D * 2 : 0));
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const uint32_t vo = voff + (uint32_t)(((c & 7) * 8 * ld + (c >> 3) * 64) * 2);
      const uint4 u = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(d, vo, 0, 0));
      r[c] = cok[c >> 3] ? u : make_uint4(0, 0, 0, 0);
    }
  };
  char* mine = smem + w * 2 * TILE;
  auto store_mat = [&](const uint4 (&r)[NC], char* img) {
#pragma unroll
    for (int c = 0; c < NC; ++c) *reinterpret_cast<uint4*>(img + (c >> 3) * HALF + (c & 7) * 8 * ROWB + sd[c & 1]) = r[c];
  };

  // per-lane fragment offsets, as in attn_extend_kernel
  int ko[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) ko[ks] = (ks >> 2) * HALF + lds_off(l32, (2 * ks + h32) & 7);
  const int trq = (lane & 15) >> 2, trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const int ta0 = tr_off(4 * h32 + trq, trc), tb0 = tr_off(8 + 4 * h32 + trq, trc);
  const int ta1 = tr_off(4 * h32 + trq, 32 + trc), tb1 = tr_off(8 + 4 * h32 + trq, 32 + trc);

  // this lane's query: row myr of the sequence's chunk, position base + myr; a lane past Tq holds a zero
  // query under the last row's limit and stores nothing
  const int myr = q0 + l32;
  const bool live = myr < Tq;
  const int mypos = base + min(myr, Tq - 1);
  const bf16_t* qrow = a.qkv_new + ((long)sq.cu + min(myr, Tq - 1)) * ld + hh * a.hd;
  bf16x8 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int d = ks * 16 + 8 * h32;
    const uint4 u = (live && d < a.hd) ? ld16(qrow + d) : make_uint4(0, 0, 0, 0);
    float f[8];
    unpack8(u, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= a.scale_log2;
    qf[ks] = __builtin_bit_cast(bf16x8, pack8(f));
  }
  f32x16 o[NO], negm = f32x16{0};
#pragma unroll
  for (int n = 0; n < NO; ++n) o[n] = f32x16{0};
  float m = 0.f, l = 0.f;

  // the trip count is the same for the four waves: the barriers are uniform
  const int niter = (t1 - t0 + 3) >> 2;
  const int tw = t0 + w;  // this wave's first tile
  {
    uint4 rk[PF >= 1 ? NC : 1], rv[PF >= 2 ? NC : 1];  // what waits in registers under the MFMAs
    int t = tw;
    if (t < t1) {
      if constexpr (PF >= 1) load_mat(rk, t * 64, false);
      if constexpr (PF >= 2) load_mat(rv, t * 64, true);
    }
    for (int i = 0; i < niter; ++i, t += 4) {
      const bool have = t < t1;
      const int k0 = t * 64;
      if (have) {
        if constexpr (PF >= 1) {
          store_mat(rk, mine);
        } else {
          uint4 r[NC];
          load_mat(r, k0, false);
          store_mat(r, mine);
        }
        if constexpr (PF >= 2) {
          store_mat(rv, mine + TILE);
        } else {
          uint4 r[NC];
          load_mat(r, k0, true);
          store_mat(r, mine + TILE);
        }
      }
      __syncthreads();
      if (t + 4 < t1) {
        if constexpr (PF >= 1) load_mat(rk, k0 + 256, false);
        if constexpr (PF >= 2) load_mat(rv, k0 + 256, true);
      }
      if (have) {
        const int lim = mypos - k0 - 4 * h32;
        // the causal mask only on the tiles that reach past the block's first query (separate bodies)
        if (k0 + 63 > base + q0) ext_tile<NKS, true>(mine, mine + TILE, ko, qf, o, negm, m, l, i == 0, lim, ta0, tb0, ta1, tb1);
        else ext_tile<NKS, false>(mine, mine + TILE, ko, qf, o, negm, m, l, i == 0, lim, ta0, tb0, ta1, tb1);
      }
      __syncthreads();
    }
  }

  // A row that saw no key of this wave's tiles (no tile, or its position lies below the first one's first
  // key: the wave's tiles ascend) has weight zero, whatever the masked bodies left in its registers
  const bool seen = tw < t1 && mypos >= tw * 64;
  float lt = sum_xor32(l);
  if (!seen) {
    m = kNegBig;
    lt = 0.f;
  }
#pragma unroll
  for (int n = 0; n < NO; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[n][r] = seen ? o[n][r] : 0.f;

  // fold in wave order: waves 1..3 -> LDS, wave 0 merges 1, 2, 3 into its own state
  float4* fo = reinterpret_cast<float4*>(smem);
  float2* fml = reinterpret_cast<float2*>(smem + 3 * FOLD_O);
  if (w > 0) {
#pragma unroll
    for (int n = 0; n < NO; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        fo[((w - 1) * NO * 8 + n * 8 + 2 * g + h32) * 32 + l32] =
            make_float4(o[n][4 * g], o[n][4 * g + 1], o[n][4 * g + 2], o[n][4 * g + 3]);
    if (h32 == 0) fml[(w - 1) * 32 + l32] = make_float2(m, lt);
  }
  __syncthreads();
  if (w != 0 || !live) return;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const float2 ml = fml[u * 32 + l32];
    const float Mx = fmaxf(m, ml.x);
    const float ca = fexp2(m - Mx), cb = fexp2(ml.x - Mx);
    lt = ca * lt + cb * ml.y;
    m = Mx;
#pragma unroll
    for (int n = 0; n < NO; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = fo[(u * NO * 8 + n * 8 + 2 * g + h32) * 32 + l32];
        o[n][4 * g] = ca * o[n][4 * g] + cb * v.x;
        o[n][4 * g + 1] = ca * o[n][4 * g + 1] + cb * v.y;
        o[n][4 * g + 2] = ca * o[n][4 * g + 2] + cb * v.z;
        o[n][4 * g + 3] = ca * o[n][4 * g + 3] + cb * v.w;
      }
  }
  if (cnt == 1) {  // the block's whole key range (key 0 is in it: lt > 0): normalise and store
    const float inv = 1.f / lt;
    bf16_t* orow = a.out + ((long)sq.cu + myr) * a.D + hh * a.hd;
#pragma unroll
    for (int n = 0; n < NO; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = n * 32 + 8 * g + 4 * h32;
        if (d < a.hd)
          *reinterpret_cast<uint2*>(orow + d) = make_uint2(pack2(o[n][4 * g] * inv, o[n][4 * g + 1] * inv),
                                                           pack2(o[n][4 * g + 2] * inv, o[n][4 * g + 3] * inv));
      }
    return;
  }
  // this split's state of row myr: {m, l} and the unnormalised O (neutral where the row saw none of it)
  const long slot = (((long)pbase * a.H + (long)hh * cnt + sp) << 5) + l32;
  if (h32 == 0) *reinterpret_cast<float2*>(a.part_ml + 2 * slot) = make_float2(m, lt);
  float* prow = a.part_o + slot * a.hd;
#pragma unroll
  for (int n = 0; n < NO; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = n * 32 + 8 * g + 4 * h32;
      if (d < a.hd)
        *reinterpret_cast<float4*>(prow + d) = make_float4(o[n][4 * g], o[n][4 * g + 1], o[n][4 * g + 2], o[n][4 * g + 3]);
    }
}

// The combine of one output block (sequence, 32-query block) with cnt > 1 splits and one head, as
// attn_extend_combine_kernel: a thread per (row, 4 columns), the block's own count of splits in split
// order.  Split 0 holds key 0, which every row sees, so M is a real max.
__global__ __launch_bounds__(256) void attn_extend_ragged_combine_kernel(const RagArgs a) {
  const int e = blockIdx.x / a.H, hh = blockIdx.x % a.H;
  const int* cb = a.combs + 4 * e;
  const int b = cb[0], qb = cb[1], cnt = cb[2], pbase = cb[3];
  const RagSeq sq = rag_seq(a, b, qb, cnt, pbase);
  if (!sq.ok || cnt < 2) return;
  const int q0 = qb * 32, rows = min(sq.Tq - q0, 32), hd4 = a.hd >> 2;
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i >= rows * hd4) return;
  const int r = i / hd4, d = (i % hd4) * 4;
  const long slot0 = (((long)pbase * a.H + (long)hh * cnt) << 5) + r;
  float ms[kExtSplitsMax], M = kNegBig;
#pragma unroll
  for (int s = 0; s < kExtSplitsMax; ++s) {
    ms[s] = s < cnt ? a.part_ml[2 * (slot0 + 32L * s)] : kNegBig;
    M = fmaxf(M, ms[s]);
  }
  float L = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int s = 0; s < kExtSplitsMax; ++s) {
    if (s < cnt) {
      const float wgt = fexp2(ms[s] - M);
      const float4 v = *reinterpret_cast<const float4*>(a.part_o + (slot0 + 32L * s) * a.hd + d);
      L += wgt * a.part_ml[2 * (slot0 + 32L * s) + 1];
      acc.x += wgt * v.x;
      acc.y += wgt * v.y;
      acc.z += wgt * v.z;
      acc.w += wgt * v.w;
    }
  }
  const float inv = 1.f / L;
  bf16_t* orow = a.out + ((long)sq.cu + q0 + r) * a.D + hh * a.hd + d;
  *reinterpret_cast<uint2*>(orow) = make_uint2(pack2(acc.x * inv, acc.y * inv), pack2(acc.z * inv, acc.w * inv));
}

int ext_cu_count() {
  static int ncu[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (!ncu[dev]) {
    int n = 0;
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    ncu[dev] = n > 0 ? n : 256;
  }
  return ncu[dev];
}

// whole 64-key tiles per split: enough splits to put two workgroups on every CU, at least two tiles
// each (a split's partial state is about a tile's worth of traffic), at most kExtSplitsMax splits
int ext_tiles_per_split(int B, int Tq, int H, int base) {
  const int nt = cdiv(base + Tq, 64);
  const long wgs = (long)cdiv(Tq, 128) * B * H;
  long S = 2L * ext_cu_count() / wgs;
  S = std::min<long>(S, std::min(kExtSplitsMax, nt / 2));
  return cdiv(nt, std::max<long>(S, 1));
}

template <int NKS, int KV>
void launch_extend(const ExtArgs& a, hipStream_t stream) {
  attn_extend_kernel<NKS, KV><<<dim3(cdiv(a.Tq, 128), a.B * a.H, a.S), 256, 0, stream>>>(a);
}

// the attention launch and, with split keys, the combine; kv: 0 (bf16 rows), 16 / 8 (int8 planes by the
// staging's load width)
template <int KV>
void launch_attend(const ExtArgs& a, hipStream_t stream) {
  switch (nks_for(a.hd)) {
    case 1: launch_extend<1, KV>(a, stream); break;
    case 2: launch_extend<2, KV>(a, stream); break;
    case 3: launch_extend<3, KV>(a, stream); break;
    case 4: launch_extend<4, KV>(a, stream); break;
    case 6: launch_extend<6, KV>(a, stream); break;
    default: launch_extend<8, KV>(a, stream); break;
  }
  if (a.S > 1)
    attn_extend_combine_kernel<<<dim3(cdiv(std::min(a.Tq, 128) * (a.hd >> 2), 256), cdiv(a.Tq, 128), a.B * a.H), 256, 0,
                                 stream>>>(a);
}

// the shapes, the split plan and the workspace layout: the same for both storage kinds
ExtArgs ext_plan(const bf16_t* qkv_new, bf16_t* out, float* part, int B, int Tq, int H, int hd, long Tmax, int base) {
  ExtArgs a{};
  a.qkv_new = qkv_new; a.out = out;
  a.B = B; a.Tq = Tq; a.H = H; a.hd = hd; a.D = H * hd; a.base = base; a.Tmax = Tmax;
  a.tps = ext_tiles_per_split(B, Tq, H, base);
  a.S = mg::attention_extend_splits(B, Tq, H, base);
  a.scale_log2 = 1.4426950408889634f / sqrtf((float)hd);
  a.part_ml = part;
  a.part_o = part ? part + (size_t)cdiv(Tq, 128) * B * H * a.S * 128 * 2 : nullptr;
  return a;
}

template <int NKS, int PF>
void launch_ragged(const RagArgs& a, int items, hipStream_t stream) {
  attn_extend_ragged_kernel<NKS, PF><<<items * a.H, 256, 0, stream>>>(a);
}

// Sequence b's key split of the ragged plan: enough splits to put two workgroups on every CU were every
// output block (32 queries, one head) split alike, capped by the sequence's own tiles -- at least two
// 64-key tiles per split, as ext_tiles_per_split reasons -- and by kExtSplitsMax.  A long history beside
// short ones is split; the short ones are not.
int rag_tiles_per_split(int tq, int base, long blocks) {
  const int nt = cdiv(base + tq, 64);
  long S = 2L * ext_cu_count() / std::max<long>(blocks, 1);
  S = std::min<long>(S, std::min(kExtSplitsMax, nt / 2));
  return cdiv(nt, std::max<long>(S, 1));
}

// walks the plan in table order: f(b, qb, cnt, pbase) per output block (pbase: the first partial slot
// of a block with cnt > 1 splits)
template <class F>
void rag_walk(const int* tq, const int* base, int B, int H, F f) {
  long blocks = 0;
  for (int b = 0; b < B; ++b) blocks += (long)cdiv(tq[b], 32) * H;
  int pbase = 0;
  for (int b = 0; b < B; ++b) {
    const int tps = rag_tiles_per_split(tq[b], base[b], blocks);
    for (int qb = 0; qb * 32 < tq[b]; ++qb) {
      const int ntb = cdiv(base[b] + std::min(tq[b], qb * 32 + 32), 64);
      const int cnt = cdiv(ntb, tps);
      f(b, qb, cnt, tps, pbase);
      if (cnt > 1) pbase += cnt;
    }
  }
}

}  // namespace

namespace mg {

int attention_extend_splits(int B, int Tq, int H, int base) {
  return cdiv(cdiv(base + Tq, 64), ext_tiles_per_split(B, Tq, H, base));
}

size_t attention_extend_part_floats(int B, int Tq, int H, int hd, int base) {
  const int S = attention_extend_splits(B, Tq, H, base);
  return S > 1 ? (size_t)cdiv(Tq, 128) * B * H * S * 128 * (hd + 2) : 0;
}

void attention_extend(const bf16_t* qkv_new, bf16_t* cache, bf16_t* out, float* part, int B, int Tq, int H,
                      int hd, long Tmax, int base, hipStream_t stream) {
  ExtArgs a = ext_plan(qkv_new, out, part, B, Tq, H, hd, Tmax, base);
  a.cache = cache;
  attn_extend_append_kernel<<<cdiv((long)B * Tq * (a.D >> 2), 256), 256, 0, stream>>>(qkv_new, cache, B, Tq, a.D,
                                                                                     Tmax, base);
  launch_attend<0>(a, stream);
}

void attention_extend_kv8(const bf16_t* qkv_new, int8_t* kq, float* ks, bf16_t* out, float* part, int B, int Tq,
                          int H, int hd, long Tmax, int base, hipStream_t stream) {
  ExtArgs a = ext_plan(qkv_new, out, part, B, Tq, H, hd, Tmax, base);
  a.kq = kq; a.ks = ks;
  const long NV = (long)B * Tq * 2 * H;
  attn_extend_snap_kernel<<<cdiv(NV, 256 / (hd >> 3)), 256, 0, stream>>>(qkv_new, kq, ks, NV, Tq, H, hd, Tmax, base);
  if (hd % 16 == 0) launch_attend<16>(a, stream);
  else launch_attend<8>(a, stream);
}

ExtRaggedShape attention_extend_ragged_shape(const int* tq, const int* base, int B, int H) {
  ExtRaggedShape sh{B, 0, 0, 0, 0};
  for (int b = 0; b < B; ++b) sh.M += tq[b];
  rag_walk(tq, base, B, H, [&](int, int, int cnt, int, int) {
    sh.items += cnt;
    if (cnt > 1) {
      sh.combs += 1;
      sh.slots += cnt;
    }
  });
  return sh;
}

void attention_extend_ragged_plan(const int* tq, const int* base, int B, int H, int* plan, int* splits) {
  const ExtRaggedShape sh = attention_extend_ragged_shape(tq, base, B, H);
  if (plan) {
    const int hdr[8] = {sh.B, sh.M, sh.items, sh.combs, sh.slots, H, 0, 0};
    std::copy(hdr, hdr + 8, plan);
    int* row_seq = plan + sh.row_seq();
    int* row_pos = plan + sh.row_pos();
    int* last = plan + sh.last();
    int* seq = plan + sh.seq();
    for (int b = 0, m = 0; b < B; ++b) {
      seq[8 * b] = m;
      seq[8 * b + 1] = base[b];
      seq[8 * b + 2] = tq[b];
      for (int r = 0; r < tq[b]; ++r, ++m) {
        row_seq[m] = b;
        row_pos[m] = base[b] + r;
      }
      last[b] = m - 1;
      for (int j = 5; j < 8; ++j) seq[8 * b + j] = 0;
    }
    int* item = plan + sh.item();
    int* comb = plan + sh.comb();
    rag_walk(tq, base, B, H, [&](int b, int qb, int cnt, int tps, int pbase) {
      seq[8 * b + 4] = tps;
      for (int s = 0; s < cnt; ++s, item += 4) {
        item[0] = b; item[1] = qb; item[2] = s | (cnt << 16); item[3] = pbase;
      }
      if (cnt > 1) {
        comb[0] = b; comb[1] = qb; comb[2] = cnt; comb[3] = pbase;
        comb += 4;
      }
    });
    for (int b = 0; b < B; ++b) seq[8 * b + 3] = cdiv(cdiv(base[b] + tq[b], 64), seq[8 * b + 4]);
  }
  if (splits) {
    long blocks = 0;
    for (int b = 0; b < B; ++b) blocks += (long)cdiv(tq[b], 32) * H;
    for (int b = 0; b < B; ++b)
      splits[b] = cdiv(cdiv(base[b] + tq[b], 64), rag_tiles_per_split(tq[b], base[b], blocks));
  }
}

void attention_extend_ragged(const bf16_t* qkv_new, bf16_t* cache, bf16_t* out, float* part, const int* plan,
                             const ExtRaggedShape& sh, int H, int hd, long Tmax, hipStream_t stream) {
  RagArgs a{};
  a.qkv_new = qkv_new; a.cache = cache; a.out = out;
  a.part_ml = part;
  a.part_o = part ? part + (size_t)sh.slots * H * 32 * 2 : nullptr;
  a.seq = plan + sh.seq(); a.items = plan + sh.item(); a.combs = plan + sh.comb();
  a.B = sh.B; a.M = sh.M; a.H = H; a.hd = hd; a.D = H * hd; a.slots = part ? sh.slots : 0; a.Tmax = Tmax;
  a.scale_log2 = 1.4426950408889634f / sqrtf((float)hd);
  attn_extend_ragged_append_kernel<<<cdiv((long)sh.M * (a.D >> 2), 256), 256, 0, stream>>>(
      qkv_new, cache, plan + sh.row_seq(), plan + sh.row_pos(), sh.M, sh.B, a.D, Tmax);
  switch (nks_for(hd)) {
    case 1: launch_ragged<1, 2>(a, sh.items, stream); break;
    case 2: launch_ragged<2, 2>(a, sh.items, stream); break;
    case 3: launch_ragged<3, 0>(a, sh.items, stream); break;
    case 4: launch_ragged<4, 1>(a, sh.items, stream); break;
    case 6: launch_ragged<6, 2>(a, sh.items, stream); break;
    default: launch_ragged<8, 1>(a, sh.items, stream); break;
  }
  if (sh.combs > 0 && part)
    attn_extend_ragged_combine_kernel<<<dim3(sh.combs * H, cdiv(32 * (hd >> 2), 256)), 256, 0, stream>>>(a);
}

}  // namespace mg
