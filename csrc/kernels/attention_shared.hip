// Shared-prefix decode attention for gfx950 (CDNA4, MI355X): R = B * N decode rows, the N rows of
// prompt b share that prompt's K/V (`pre` [B, Tpre, 3D], keys 0 .. P - 1, written by the prefill and
// never here) and each keeps only what it generated itself (`own` [R, Town, 3D], keys P .. pos - 1);
// key pos is the step's own row of qkv_new.  (One query against one cache: attention.hip; a chunk
// of one sequence against its cache: attention_extend.hip.)  models/generation.py decodes
// generate(num_return_sequences=N) on it.
//
// N rows against one set of keys is a matrix product, so the prefix part runs on MFMA and reads a
// prompt's K/V tiles once per (b, h) and launch, however large N is; the plain decode kernel streams
// them once per row through scalar FMAs.
//
// Three stream-ordered launches; each split writes an unnormalised fp32 state (m, l, O) per row
// to the caller's workspace and the last launch sums them.  Launch boundaries, not a last-arrival
// hand-off inside a kernel: a boundary cannot hang.
//  1. attn_shared_prefix_kernel<NKS, NF>, grid (b * h, prefix split).  A split is `tps` whole 64-key
//     tiles.  The work split is by KEYS: the extend kernel gives each of its four waves 32 queries,
//     but here there are at most 64 queries, often 2 to 16, and that would idle three waves.  Wave w
//     of split s walks tiles s * tps + w, + 4, ... -- each staged by that wave into its own LDS
//     region; with up to 16 splits a wave has one tile at Tpre <= 4096 unless B * H fills the chip,
//     so no tile is prefetched under another (it cost 64 to 128 staging VGPRs) -- against ALL N queries, held
//     as NF = 1 or 2 fragments of 32 queries in VGPRs, pre-multiplied by log2(e) / sqrt(hd), and
//     keeps its own (m, l, O) per fragment.  S^T = K Q^T with v_mfma_f32_32x32x16_bf16: the query
//     is on the lane, the softmax statistics are lane-local; O^T += V^T P^T with V^T fragments from
//     ds_read_b64_tr_b16 (shr_tile: the extend kernel's tile body, but the rare re-centring of the
//     running max is decided and applied per query, so a row's bits never depend on its neighbours'
//     queries).  No causal mask: every prefix key is visible to every row; the tail tile is masked
//     by key index.  At the end waves 1..3 put their state in LDS (the tile regions are free by
//     then) and wave 0 folds them in wave order and writes the split's partial.
//  2. attn_shared_own_kernel, grid (row * h, own split of 256 keys): the row's private keys P .. pos
//     as the plain decode kernel's vector body, one query per workgroup; the workgroup of a row's
//     first own split appends the row's K/V at own[m, pos - P] bit for bit (nobody reads that row
//     in this launch: key pos comes from qkv_new).  The first own split always holds key pos, so
//     the maximum over a row's partials is always real.
//  3. attn_shared_combine_kernel: out = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s in the fixed
//     order prefix splits ascending, then own splits ascending, over ALL splits of the grid.
//
// Both lengths come from device memory (pos_dev, plen_dev), so one captured hipGraph serves every
// step and every prompt length: the grids depend on Tpre, Town, B, N, H and the CU count only, and a
// split with no key at this (P, pos) writes the neutral partial (m = -big, l = 0, O = 0).  A row's
// bits depend on its own query, its own rows of `own` and qkv_new and its prompt's `pre` rows: not
// on the other rows, not on its slot in the group (an MFMA column is computed from that column's
// B operand alone), not on graph or eager launch.
//
// Stale rows: `pre` rows at or past P and `own` rows at or past pos - P come from torch.empty and
// may hold NaN.  Prefix tiles are loaded through a buffer descriptor that ends at row P (kv_rsrc:
// rows past it read as zeros) and the tail tile's scores are masked; a 16-byte chunk whose columns
// lie at or past hd is staged as zeros (it would read the next head or third, and 0 x NaN in an
// MFMA is NaN); the own part indexes keys below pos - P only.
//
// Out of range (pos < P or pos - P >= Town): nothing is appended, every split is neutral and the
// combine writes zero rows.
//
// KV8 (attention_decode_shared_kv8): the same launches on the int8 cache of kernels.h, pre_q / pre_s
// [B, 2, H, Tpre, (hd)] and own_q / own_s [R, 2, H, Town, (hd)].  Only the loads differ.  Prefix: a 64-key
// tile of one (b, K | V, h) plane is 64 * hd contiguous bytes plus 64 scale words (half the bf16 tile's
// bytes, no strided rows); a wave loads them with 16-byte loads (hd % 16 == 0; KV = 16) or 8-byte loads
// (KV = 8), dequantizes float(q) * s in registers -- exact, the bf16 value the snapped row holds -- and
// writes the LDS images the bf16 staging writes, so shr_tile, the key walk, the fold and the partials
// are this file's one copy.  No tile is prefetched under another here either: not measured.  With hd >
// 64 and N > 32 the two query fragments run as two workgroups (no instantiation uses scratch).  Own:
// attention_decode_kv8's loads and its snap of the step's K/V in LDS; the first own split appends the
// rule's (q, s).  out equals the bf16 kernels on the dequantized rows bit for bit.
#include "attn_common.h"
#include "kernels.h"
#include "kv8_common.h"

using namespace mg;
using namespace mg::attn;
using namespace mg::kv8;

namespace {

constexpr int kShrSplitsMax = 16;  // prefix splits per (b, h)
constexpr int kShrOwnKeys = 256;   // keys per own split (one per thread)

struct ShrArgs {
  const bf16_t* qkv_new;  // [R, 3D]
  const bf16_t* pre;      // [B, Tpre, 3D]
  bf16_t* own;            // [R, Town, 3D]
  // KV8 (attention_decode_shared_kv8): the int8 caches in place of pre / own
  const int8_t* pre_q;    // [B, 2, H, Tpre, hd]
  const float* pre_s;     // [B, 2, H, Tpre]
  int8_t* own_q;          // [R, 2, H, Town, hd]
  float* own_s;           // [R, 2, H, Town]
  bf16_t* out;            // [R, D]
  float* part_ml;         // [B * H][St][N][2] {m, l}
  float* part_o;          // [B * H][St][N][hd]
  const int* pos_dev;
  const int* plen_dev;
  int B, N, H, hd, D, Tpre, Town;
  int Sp, tps, So, St;    // prefix splits, whole 64-key tiles per prefix split, own splits, Sp + So
  float scale_log2;       // log2(e) / sqrt(hd)
};

// P (clamped to [1, Tpre]) and pos from device memory; false: the step has no room
MG_DEVICE bool shr_lengths(const ShrArgs& a, int& P, int& pos) {
  P = min(max(*a.plen_dev, 1), a.Tpre);
  pos = *a.pos_dev;
  return pos >= P && pos - P < a.Town;
}

// One 64-key tile for one fragment of 32 queries: S'^T = K Q^T - m, p = exp2(S'), O^T += V^T P^T.
// m moves only when a tile's row sum leaves [lo, 2^60] (lo = 2^-60 on the wave's first tile, where m
// starts at 0, else 0).  The wave then recomputes the tile, but only the queries whose own sum left
// the range move their m (d = 0 for the others: alpha = 1, the same scores, the same bits).
template <int NKS, bool MASK>
MG_DEVICE void shr_tile(const char* sk, const char* sv, const int (&ko)[NKS], const bf16x8 (&qf)[NKS],
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
      asm volatile("" : "+v"(lim));
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
  // this query's sum -- either half of it -- left the range (inf / nan included)
  const bool need = max_xor32(!(rs <= 1.152921504606847e18f && rs >= lo) ? 1.f : 0.f) > 0.f;  // 2^60
  if (__builtin_expect(__any(need), 0)) {
    int lim2 = lim;
    asm volatile("" : "+v"(lim2));
    scores(lim2);
    float mx = s[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[1][r]);
    mx = max_xor32(mx);
    // the wave's first tile may move m down as well (nothing accumulated yet); later tiles up only
    const float d = need ? (first ? mx : fmaxf(mx, 0.f)) : 0.f;
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

// KV = 0: bf16 qkv rows (pre).  KV = 16 / 8: the int8 cache (pre_q / pre_s), staged with 16-byte loads
// (hd % 16 == 0) or 8-byte loads -- the KV8 staging in the file header.
template <int NKS, int NF, int KV>
__global__ __launch_bounds__(256, (NKS > 4 || NF > 1) ? 1 : 2) void attn_shared_prefix_kernel(const ShrArgs a) {
  constexpr int NH = (NKS + 3) / 4;   // 64-column halves of the LDS images
  constexpr int NO = (NKS + 1) / 2;   // 32-column O^T accumulator tiles
  constexpr int HALF = 64 * ROWB;     // one 64-row, 64-column image
  constexpr int TILE = NH * HALF;     // one K or V tile
  constexpr int NC = 8 * NH;          // 16-byte chunks per lane per tile per matrix (a wave stages its own tile)
  constexpr int FOLD_O = NO * 8 * 64 * 16;  // one wave's O for the fold: [NO * 8 float4 columns][64 queries]
  static_assert(3 * (FOLD_O + 64 * 8) <= 8 * TILE, "the fold reuses the tile regions");
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];  // per wave: K, V
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h32 = lane >> 5, l32 = lane & 31;
  const int bh = blockIdx.x, sp = blockIdx.y;
  const int b = bh / a.H, hh = bh % a.H;
  const long ld = 3L * a.D;
  int P, pos;
  const bool ok = shr_lengths(a, P, pos);
  const int ntp = ok ? (P + 63) / 64 : 0;               // prefix tiles at this length
  const int t0 = sp * a.tps, t1 = min(t0 + a.tps, ntp);  // this split's tiles [t0, t1); wave w: t0 + w, + 4, ...

  // tile staging: chunk c of this lane -> (half, row, 16-byte column chunk), through a per-tile
  // descriptor that ends at the prompt's row P (file header)
  uint32_t voff[NC], sdst[NC];
  bool cok[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int idx = lane + 64 * c;
    const int hf = idx >> 9, rem = idx & 511;
    voff[c] = (uint32_t)(((rem >> 3) * ld + hf * 64 + (rem & 7) * 8) * 2);
    sdst[c] = hf * HALF + lds_off(rem >> 3, rem & 7);
    cok[c] = hf * 64 + (rem & 7) * 8 < a.hd;
  }
  const bf16_t* seq = a.pre + (long)b * a.Tpre * ld;
  const uint64_t seq_bytes = (uint64_t)P * ld * 2;  // rows [0, P) of this prompt
  const uint64_t kcol = (uint64_t)(a.D + hh * a.hd) * 2;
  auto load_tile = [&](uint4 (&rk)[NC], uint4 (&rv)[NC], int k0) {
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
  char* mine = smem + w * 2 * TILE;
  auto store_tile = [&](const uint4 (&rk)[NC], const uint4 (&rv)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      *reinterpret_cast<uint4*>(mine + sdst[c]) = rk[c];
      *reinterpret_cast<uint4*>(mine + TILE + sdst[c]) = rv[c];
    }
  };

  // KV8 staging.  The 64 keys of a tile of one (b, K | V, h) plane are 64 * hd contiguous int8 bytes and
  // 64 contiguous scale words.  Load c of a lane is the plane's bytes [(lane + 64 c) * CB, + CB) of the
  // tile: cpr = hd / CB loads per lane and matrix, the same count in every lane, each instruction one
  // contiguous 64 * CB bytes.  Lane l also loads the scale of key l, and the scale of a chunk's key row
  // comes from that lane (ds_bpermute).  The chunk is dequantized in registers -- float(q) * s is exact
  // and IS the bf16 value of the snapped row, a NaN scale makes the vector NaN -- packed to bf16 and
  // written as the one or two 16-byte chunks of the swizzled image the bf16 staging writes.  Both planes
  // are read through descriptors that end at key P: past it bytes and scale read as 0 and 0 x 0 = 0.
  // The loads never touch columns at or past hd, so those image columns are zeroed once, before the
  // first tile (zero_pad).
  constexpr int CB = KV ? KV : 16;     // bytes per load
  constexpr int NL = NKS * 16 / CB;    // loads per lane and matrix at most
  typedef uint32_t kv8_chunk __attribute__((ext_vector_type(CB / 4)));
  const int cpr = a.hd / CB;
  uint32_t qdst[NL];                   // image offset of the chunk's first 8 columns; key row = bits 7..12
#pragma unroll
  for (int c = 0; c < NL; ++c) {
    const int idx = lane + 64 * c, row = min(idx / max(cpr, 1), 63), col = (idx % max(cpr, 1)) * CB;
    qdst[c] = (col >> 6) * HALF + lds_off(row, (col >> 3) & 7);
  }
  const long plane = ((long)b * 2 * a.H + hh) * a.Tpre;   // K; V is H * Tpre keys behind it
  const long vplane = (long)a.H * a.Tpre;
  auto kv8_chunk_store = [&](char* img, uint32_t dst, const kv8_chunk& u, float sc) {
    float f[8];
    dequant8(make_uint2(u[0], u[1]), sc, f);
    *reinterpret_cast<uint4*>(img + dst) = pack8(f);
    if constexpr (CB == 16) {  // columns 8 .. 15 of the chunk: the neighbouring image chunk
      dequant8(make_uint2(u[2], u[3]), sc, f);
      *reinterpret_cast<uint4*>(img + (dst ^ 16)) = pack8(f);
    }
  };
  auto stage_kv8 = [&](int k0) {
    const uint64_t qbytes = (uint64_t)P * a.hd, qoff = (uint64_t)k0 * a.hd;
    const __amdgpu_buffer_rsrc_t dk = kv_rsrc(a.pre_q + plane * a.hd, qbytes, qoff);
    const __amdgpu_buffer_rsrc_t dv = kv_rsrc(a.pre_q + (plane + vplane) * a.hd, qbytes, qoff);
    const __amdgpu_buffer_rsrc_t dsk = kv_rsrc(a.pre_s + plane, (uint64_t)P * 4, (uint64_t)k0 * 4);
    const __amdgpu_buffer_rsrc_t dsv = kv_rsrc(a.pre_s + plane + vplane, (uint64_t)P * 4, (uint64_t)k0 * 4);
    kv8_chunk rk[NL], rv[NL];
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      if (c < cpr) {
        const uint32_t off = (uint32_t)(lane + 64 * c) * CB;
        if constexpr (CB == 16) {
          rk[c] = __builtin_bit_cast(kv8_chunk, __builtin_amdgcn_raw_buffer_load_b128(dk, off, 0, 0));
          rv[c] = __builtin_bit_cast(kv8_chunk, __builtin_amdgcn_raw_buffer_load_b128(dv, off, 0, 0));
        } else {
          rk[c] = __builtin_bit_cast(kv8_chunk, __builtin_amdgcn_raw_buffer_load_b64(dk, off, 0, 0));
          rv[c] = __builtin_bit_cast(kv8_chunk, __builtin_amdgcn_raw_buffer_load_b64(dv, off, 0, 0));
        }
      }
    }
    const float sk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dsk, lane * 4, 0, 0));
    const float sv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dsv, lane * 4, 0, 0));
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      if (c < cpr) {
        const int row = (qdst[c] >> 7) & 63;
        kv8_chunk_store(mine, qdst[c], rk[c], __shfl(sk, row, 64));
        kv8_chunk_store(mine + TILE, qdst[c], rv[c], __shfl(sv, row, 64));
      }
    }
  };
  if constexpr (KV != 0) {
    // image columns hd .. 32 NO - 1 (K fragments read below 16 NKS, V^T fragments below 32 NO): never
    // staged, so zero this wave's two images once
    if (a.hd < 32 * NO) {
      for (int i = lane * 16; i < 2 * TILE; i += 64 * 16) *reinterpret_cast<uint4*>(mine + i) = make_uint4(0, 0, 0, 0);
    }
  }

  // per-lane fragment offsets (as in the extend kernel): K rows l32 (+32 per sub), chunk 2 ks + h32;
  // V^T transposed reads rows 4 h32 + q (+8), columns (n & 1) * 32 + cb + 4 p
  int ko[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) ko[ks] = (ks >> 2) * HALF + lds_off(l32, (2 * ks + h32) & 7);
  const int trq = (lane & 15) >> 2, trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const int ta0 = tr_off(4 * h32 + trq, trc), tb0 = tr_off(8 + 4 * h32 + trq, trc);
  const int ta1 = tr_off(4 * h32 + trq, 32 + trc), tb1 = tr_off(8 + 4 * h32 + trq, 32 + trc);

  // this lane's queries: slot 32 f + l32 of the group, row b * N + slot; a lane past N holds a zero
  // query and stores nothing
  // KV8 with hd > 64 and N > 32 runs its two fragments as two workgroups of one (blockIdx.z; launch_prefix)
  const int f0 = KV != 0 ? blockIdx.z : 0;
  bf16x8 qf[NF][NKS];
  f32x16 o[NF][NO], negm[NF];
  float m[NF], l[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int j = 32 * (f + f0) + l32;
    const bf16_t* qrow = a.qkv_new + ((long)b * a.N + min(j, a.N - 1)) * ld + hh * a.hd;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int d = ks * 16 + 8 * h32;
      const uint4 u = (j < a.N && d < a.hd) ? ld16(qrow + d) : make_uint4(0, 0, 0, 0);
      float q8[8];
      unpack8(u, q8);
#pragma unroll
      for (int e = 0; e < 8; ++e) q8[e] *= a.scale_log2;
      qf[f][ks] = __builtin_bit_cast(bf16x8, pack8(q8));
    }
#pragma unroll
    for (int n = 0; n < NO; ++n) o[f][n] = f32x16{0};
    negm[f] = f32x16{0};
    m[f] = 0.f;
    l[f] = 0.f;
  }

  // the trip count is the same for every wave and every (P, pos): the barriers are uniform
  const int niter = (a.tps + 3) >> 2;
  bool seen = false;
  int t = t0 + w;
  for (int it = 0; it < niter; ++it, t += 4) {
    const bool have = t < t1;
    if (have) {
      if constexpr (KV != 0) {
        stage_kv8(t * 64);
      } else {
        uint4 rk[NC], rv[NC];
        load_tile(rk, rv, t * 64);
        store_tile(rk, rv);
      }
    }
    __syncthreads();
    if (have) {
      const int k0 = t * 64;
      const int lim = P - 1 - k0 - 4 * h32;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (k0 + 63 > P - 1) shr_tile<NKS, true>(mine, mine + TILE, ko, qf[f], o[f], negm[f], m[f], l[f], !seen, lim, ta0, tb0, ta1, tb1);
        else shr_tile<NKS, false>(mine, mine + TILE, ko, qf[f], o[f], negm[f], m[f], l[f], !seen, lim, ta0, tb0, ta1, tb1);
      }
      seen = true;
    }
    __syncthreads();
  }

  // fold in wave order: waves 1..3 -> LDS, wave 0 merges 1, 2, 3 into its own state.  A wave that
  // saw no tile has weight zero
  float lt[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    lt[f] = sum_xor32(l[f]);
    if (!seen) m[f] = kNegBig;
  }
  float4* fo = reinterpret_cast<float4*>(smem);
  float2* fml = reinterpret_cast<float2*>(smem + 3 * FOLD_O);
  if (w > 0) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
#pragma unroll
      for (int n = 0; n < NO; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          fo[((w - 1) * NO * 8 + n * 8 + 2 * g + h32) * 64 + 32 * f + l32] =
              make_float4(o[f][n][4 * g], o[f][n][4 * g + 1], o[f][n][4 * g + 2], o[f][n][4 * g + 3]);
      if (h32 == 0) fml[(w - 1) * 64 + 32 * f + l32] = make_float2(m[f], lt[f]);
    }
  }
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const float2 ml = fml[u * 64 + 32 * f + l32];
      const float M = fmaxf(m[f], ml.x);
      const float ca = fexp2(m[f] - M), cb = fexp2(ml.x - M);
      lt[f] = ca * lt[f] + cb * ml.y;
      m[f] = M;
#pragma unroll
      for (int n = 0; n < NO; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 v = fo[(u * NO * 8 + n * 8 + 2 * g + h32) * 64 + 32 * f + l32];
          o[f][n][4 * g] = ca * o[f][n][4 * g] + cb * v.x;
          o[f][n][4 * g + 1] = ca * o[f][n][4 * g + 1] + cb * v.y;
          o[f][n][4 * g + 2] = ca * o[f][n][4 * g + 2] + cb * v.z;
          o[f][n][4 * g + 3] = ca * o[f][n][4 * g + 3] + cb * v.w;
        }
    }
  // the split's partial of every row of the group (neutral when the split has no tile: m = -big)
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int j = 32 * (f + f0) + l32;
    if (j >= a.N) continue;
    const long slot = ((long)bh * a.St + sp) * a.N + j;
    if (h32 == 0) *reinterpret_cast<float2*>(a.part_ml + 2 * slot) = make_float2(m[f], lt[f]);
    float* prow = a.part_o + slot * a.hd;
#pragma unroll
    for (int n = 0; n < NO; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = n * 32 + 8 * g + 4 * h32;
        if (d < a.hd)
          *reinterpret_cast<float4*>(prow + d) =
              make_float4(o[f][n][4 * g], o[f][n][4 * g + 1], o[f][n][4 * g + 2], o[f][n][4 * g + 3]);
      }
  }
}

// The private keys of row m, head hh, own split so: indices [so * 256, ..) of the row's `no` =
// pos - P + 1 own keys, the last of which (key pos) is qkv_new's.  The plain decode kernel's body: a
// key per thread for the scores, then P V over key groups of hd / 8 lanes.
// KV8: the own keys come from own_q / own_s through attention_decode_kv8's loads (8 or 16 bytes of int8
// and one scale per key, dequantized to the floats the bf16 row holds); the step's K/V are snapped by
// the KV8 rule into LDS by every own split (key pos is read from there, never from the cache) and their
// (q, s) are appended at own row pos - P by the row's first own split.  The sums are the bf16
// instantiation's statements, element for element.
template <bool KV8>
__global__ __launch_bounds__(256) void attn_shared_own_kernel(const ShrArgs a) {
  __shared__ float qs[128];
  __shared__ float sc[256];
  __shared__ float red[16];
  __shared__ float acc[256 * 8];
  __shared__ float vs[KV8 ? 256 : 1];     // KV8: the V scale of the split's key t
  __shared__ float nkv[KV8 ? 256 : 1];    // KV8: the step's snapped K [0, 128) and V [128, 256) of this head
  __shared__ uint32_t cm[KV8 ? 32 : 1];
  const int row = blockIdx.x / a.H, hh = blockIdx.x % a.H, so = blockIdx.y;
  const int b = row / a.N, j = row % a.N;
  const int hd = a.hd, D = a.D;
  const long ld = 3L * D;
  int P, pos;
  const bool ok = shr_lengths(a, P, pos);
  const long slot = ((long)(b * a.H + hh) * a.St + a.Sp + so) * a.N + j;
  float* pml = a.part_ml + 2 * slot;
  float* po = a.part_o + slot * hd;
  const int no = ok ? pos - P + 1 : 0;
  const int k0 = so * kShrOwnKeys;
  const int nk = max(min(no - k0, kShrOwnKeys), 0);
  if (nk == 0) {  // the whole workgroup: no own key in this split at this (P, pos)
    if (threadIdx.x < hd) po[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) *reinterpret_cast<float2*>(pml) = make_float2(kNegBig, 0.f);
    return;
  }
  const bf16_t* qrow = a.qkv_new + (long)row * ld + hh * hd;
  bf16_t* orows = KV8 ? nullptr : a.own + (long)row * a.Town * ld;
  const int dch = hd >> 3;
  // KV8: this row's K and V planes of the head in own_q (bytes: * hd) and own_s
  const long rowk = ((long)row * 2 * a.H + hh) * a.Town, rowv = rowk + (long)a.H * a.Town;
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  const int which = threadIdx.x / dch, c8 = threadIdx.x % dch;  // threads below 2 dch: K | V, 16-byte chunk
  if constexpr (KV8) {
    if (threadIdx.x < 2 * dch) {
      raw = ld16(qrow + (long)D * (1 + which) + 8 * c8);
      cm[threadIdx.x] = max_abs8(raw);
    }
  } else {
    if (so == 0 && threadIdx.x < (hd >> 2)) {  // append K and V at own row pos - P, 16 bytes a thread
      st16(orows + (long)(pos - P) * ld + (long)D * (1 + which) + hh * hd + 8 * c8, ld16(qrow + (long)D * (1 + which) + 8 * c8));
    }
  }
  for (int d = threadIdx.x; d < hd; d += 256) qs[d] = bf2f(qrow[d]);
  __syncthreads();
  if constexpr (KV8) {
    if (threadIdx.x < 2 * dch) {  // snap the step's K/V into LDS; the first own split appends their (q, s)
      uint32_t a15 = 0;
      for (int i = 0; i < dch; ++i) a15 = max(a15, cm[which * dch + i]);
      int ex;
      bool live;
      const float sn = kv8_scale(a15, ex, live);
      float f[8];
      const uint2 q8 = kv8_quant8(raw, ex, live, sn, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) nkv[which * 128 + c8 * 8 + e] = f[e];
      if (so == 0) {
        const long r = (which ? rowv : rowk) + (pos - P);
        *reinterpret_cast<uint2*>(a.own_q + r * hd + c8 * 8) = q8;
        if (c8 == 0) a.own_s[r] = sn;
      }
    }
    __syncthreads();
  }
  auto kv_row = [&](int i) {  // K columns of own key i of this head (V: + D)
    return i == no - 1 ? qrow + D : orows + (long)i * ld + D + hh * hd;
  };
  float s = -INFINITY;
  if (threadIdx.x < nk) {
    float dot = 0.f;
    auto dot8 = [&](int d, const float (&k8)[8]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) dot += qs[d + e] * k8[e];
    };
    if constexpr (KV8) {
      const int i = k0 + threadIdx.x;
      float k8[8];
      if (i == no - 1) {
        vs[threadIdx.x] = 0.f;
        for (int d = 0; d < hd; d += 8) {
#pragma unroll
          for (int e = 0; e < 8; ++e) k8[e] = nkv[d + e];
          dot8(d, k8);
        }
      } else {
        const float sk = a.own_s[rowk + i];
        vs[threadIdx.x] = a.own_s[rowv + i];
        const int8_t* kr = a.own_q + (rowk + i) * hd;
        if ((hd & 15) == 0) {
          for (int d = 0; d < hd; d += 16) {
            const uint4 u = ld16(kr + d);
            dequant8(make_uint2(u.x, u.y), sk, k8);
            dot8(d, k8);
            dequant8(make_uint2(u.z, u.w), sk, k8);
            dot8(d + 8, k8);
          }
        } else {
          for (int d = 0; d < hd; d += 8) {
            dequant8(*reinterpret_cast<const uint2*>(kr + d), sk, k8);
            dot8(d, k8);
          }
        }
      }
    } else {
      const bf16_t* kr = kv_row(k0 + threadIdx.x);
      for (int d = 0; d < hd; d += 8) {
        float k8[8];
        unpack8(ld16(kr + d), k8);
        dot8(d, k8);
      }
    }
    s = dot * a.scale_log2;
  }
  const float mx = block_max<4>(s, red);
  const float p = threadIdx.x < nk ? fexp2(s - mx) : 0.f;
  sc[threadIdx.x] = p;
  const float sm = block_sum<4>(p, red + 4);
  __syncthreads();
  const int ngrp = 256 / dch;
  const int grp = threadIdx.x / dch, d8 = (threadIdx.x % dch) * 8;
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (grp < ngrp) {
    for (int jj = grp; jj < nk; jj += ngrp) {
      float v8[8];
      if constexpr (KV8) {
        if (k0 + jj == no - 1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v8[e] = nkv[128 + d8 + e];
        } else {
          dequant8(*reinterpret_cast<const uint2*>(a.own_q + (rowv + k0 + jj) * hd + d8), vs[jj], v8);
        }
      } else {
        unpack8(ld16(kv_row(k0 + jj) + D + d8), v8);
      }
      const float pj = sc[jj];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += pj * v8[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[threadIdx.x * 8 + e] = o[e];
  __syncthreads();
  if (threadIdx.x < hd) {
    const int c = threadIdx.x / 8, e = threadIdx.x % 8;
    float v = 0.f;
    for (int g = 0; g < ngrp; ++g) v += acc[(g * dch + c) * 8 + e];
    po[threadIdx.x] = v;
  }
  if (threadIdx.x == 0) *reinterpret_cast<float2*>(pml) = make_float2(mx, sm);
}

// out row = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s over all St partials in order, M = max_s
// m_s (real: the first own split holds key pos): a thread per (row, head, 4 columns)
__global__ __launch_bounds__(256) void attn_shared_combine_kernel(const ShrArgs a) {
  const int hd4 = a.hd >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)a.B * a.N * a.H * hd4) return;
  const int row = (int)(i / (a.H * hd4)), rem = (int)(i % (a.H * hd4));
  const int hh = rem / hd4, d = (rem % hd4) * 4;
  const int b = row / a.N, j = row % a.N;
  bf16_t* orow = a.out + (long)row * a.D + hh * a.hd + d;
  int P, pos;
  if (!shr_lengths(a, P, pos)) {
    *reinterpret_cast<uint2*>(orow) = make_uint2(0, 0);
    return;
  }
  const long slot0 = (long)(b * a.H + hh) * a.St * a.N + j;
  float M = kNegBig;
  for (int s = 0; s < a.St; ++s) M = fmaxf(M, a.part_ml[2 * (slot0 + (long)s * a.N)]);
  float L = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < a.St; ++s) {
    const long slot = slot0 + (long)s * a.N;
    const float2 ml = *reinterpret_cast<const float2*>(a.part_ml + 2 * slot);
    const float wgt = fexp2(ml.x - M);
    const float4 v = *reinterpret_cast<const float4*>(a.part_o + slot * a.hd + d);
    L += wgt * ml.y;
    acc.x += wgt * v.x;
    acc.y += wgt * v.y;
    acc.z += wgt * v.z;
    acc.w += wgt * v.w;
  }
  const float inv = 1.f / L;
  *reinterpret_cast<uint2*>(orow) = make_uint2(pack2(acc.x * inv, acc.y * inv), pack2(acc.z * inv, acc.w * inv));
}

int shr_cu_count() {
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

// prefix splits: enough to put two workgroups on every CU, at least four tiles each while there
// are that many (one per wave), at most kShrSplitsMax
int shr_prefix_splits(int B, int H, int Tpre) {
  const int nt = cdiv(Tpre, 64);
  long S = 2L * shr_cu_count() / ((long)B * H);
  S = std::min<long>(S, std::min(kShrSplitsMax, cdiv(nt, 4)));
  return (int)std::max<long>(S, 1);
}

// floats of the {m, l} region, rounded so that the O region behind it stays 16-byte aligned
size_t shr_ml_floats(int B, int N, int H, int St) { return ((size_t)B * H * St * N * 2 + 3) & ~(size_t)3; }

template <int NKS, int KV>
void launch_prefix(const ShrArgs& a, hipStream_t stream) {
  const dim3 grid(a.B * a.H, a.Sp);
  if (a.N <= 32) {
    attn_shared_prefix_kernel<NKS, 1, KV><<<grid, 256, 0, stream>>>(a);
  } else if constexpr (KV != 0 && NKS > 4) {
    // two query fragments at hd > 64 need more than the 512 registers (the bf16 <8, 2> spills): one
    // workgroup per fragment instead.  A row's bits do not depend on which fragment slot computes it
    attn_shared_prefix_kernel<NKS, 1, KV><<<dim3(a.B * a.H, a.Sp, 2), 256, 0, stream>>>(a);
  } else {
    attn_shared_prefix_kernel<NKS, 2, KV><<<grid, 256, 0, stream>>>(a);
  }
}

// the three launches of one call; kv: 0 (bf16 rows), 16 / 8 (int8 planes by the staging's load width)
template <int KV>
void launch_shared(const ShrArgs& a, hipStream_t stream) {
  switch (nks_for(a.hd)) {
    case 1: launch_prefix<1, KV>(a, stream); break;
    case 2: launch_prefix<2, KV>(a, stream); break;
    case 3: launch_prefix<3, KV>(a, stream); break;
    case 4: launch_prefix<4, KV>(a, stream); break;
    case 6: launch_prefix<6, KV>(a, stream); break;
    default: launch_prefix<8, KV>(a, stream); break;
  }
  const int R = a.B * a.N;
  attn_shared_own_kernel<KV != 0><<<dim3(R * a.H, a.So), 256, 0, stream>>>(a);
  attn_shared_combine_kernel<<<cdiv((long)R * a.H * (a.hd >> 2), 256), 256, 0, stream>>>(a);
}

// the shapes, the split plan and the workspace layout: the same for both storage kinds
ShrArgs shr_plan(const bf16_t* qkv_new, bf16_t* out, float* part, int R, int N, int H, int hd, int Tpre, int Town,
                 const int* pos_dev, const int* plen_dev) {
  ShrArgs a{};
  a.qkv_new = qkv_new; a.out = out;
  a.pos_dev = pos_dev; a.plen_dev = plen_dev;
  a.B = R / N; a.N = N; a.H = H; a.hd = hd; a.D = H * hd; a.Tpre = Tpre; a.Town = Town;
  a.Sp = mg::attention_decode_shared_splits(a.B, H, Tpre);
  a.tps = cdiv(cdiv(Tpre, 64), a.Sp);
  a.So = cdiv(Town, kShrOwnKeys);
  a.St = a.Sp + a.So;
  a.scale_log2 = 1.4426950408889634f / sqrtf((float)hd);
  a.part_ml = part;
  a.part_o = part + shr_ml_floats(a.B, N, H, a.St);
  return a;
}

}  // namespace

namespace mg {

int attention_decode_shared_splits(int B, int H, int Tpre) {
  const int S = shr_prefix_splits(B, H, Tpre);
  return cdiv(cdiv(Tpre, 64), cdiv(cdiv(Tpre, 64), S));  // no empty trailing split
}

size_t attention_decode_shared_part_floats(int B, int N, int H, int hd, int Tpre, int Town) {
  const int St = attention_decode_shared_splits(B, H, Tpre) + cdiv(Town, kShrOwnKeys);
  return shr_ml_floats(B, N, H, St) + (size_t)B * H * St * N * hd;
}

void attention_decode_shared(const bf16_t* qkv_new, const bf16_t* pre, bf16_t* own, bf16_t* out, float* part,
                             int R, int N, int H, int hd, int Tpre, int Town, const int* pos_dev,
                             const int* plen_dev, hipStream_t stream) {
  ShrArgs a = shr_plan(qkv_new, out, part, R, N, H, hd, Tpre, Town, pos_dev, plen_dev);
  a.pre = pre; a.own = own;
  launch_shared<0>(a, stream);
}

void attention_decode_shared_kv8(const bf16_t* qkv_new, const int8_t* pre_q, const float* pre_s, int8_t* own_q,
                                 float* own_s, bf16_t* out, float* part, int R, int N, int H, int hd, int Tpre,
                                 int Town, const int* pos_dev, const int* plen_dev, hipStream_t stream) {
  ShrArgs a = shr_plan(qkv_new, out, part, R, N, H, hd, Tpre, Town, pos_dev, plen_dev);
  a.pre_q = pre_q; a.pre_s = pre_s; a.own_q = own_q; a.own_s = own_s;
  if (hd % 16 == 0) launch_shared<16>(a, stream);
  else launch_shared<8>(a, stream);
}

}  // namespace mg
