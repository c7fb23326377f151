// Skinny GEMM ("GEMV") for autoregressive decode on gfx950.
//
// One decode step pushes B <= 8 rows through every projection of the model (the reference's
// generate() re-runs the whole prefix instead; the KV-cache path in models/generation.py needs only
// the new token's rows).  At M = B the MFMA GEMM has 1 row tile:
// 6-24 workgroups walk a K loop one tile at a time and the projection is latency-bound
// (26 us for the 3072 -> 768 MLP projection at B = 1).  The work is a stream of the weight
// matrix (K x N bf16, read once) against B vectors that fit in LDS, so here:
//   * x [B, K] is staged once per workgroup in LDS -- optionally LayerNorm'ed on the way in (the
//     LN that precedes every decode projection but the residual ones; one kernel instead of two);
//     rows of 4096 < K <= 8192 (the MLP output projection of gpt2-large / -xl) go through the
//     same 64 KiB buffer in two segments;
//   * a wave owns one output column n (outputs <= 8k: every block projection) or 4 (the LM head):
//     its 64 (or 16) lanes read row n = W[n, :] in 16-byte chunks, 4 loads in flight per lane,
//     FMA against the B vectors from LDS (gemv_fma: the one chain every path runs);
//   * the lanes of a row fold with xor-shuffles; the row's first lane writes y[b, n] with the same
//     fused epilogues as gemm.hip's forward (bias | bias + GELU | residual + bias), no dropout
//     (inference): proj_epilogue, common.h;
//   * weights are read non-temporally (streamed once per token; MI355X_MICROARCH launches-baseline:
//     nt weight loads ~11 % faster per decode layer);
//   * greedy decode (LM head): the argmax of the logits is fused -- each workgroup publishes its
//     best (value, index) key and the next decode step's embedding kernel reduces them into the
//     token (and advances the device position), so a captured decode step can be replayed back
//     to back with no host round trip per token.
// gemv_kernel<B, LPR, NTW, KMAX> is one of three paths, each a block of the kernel's body:
//   LPR 64, KMAX kGemvSegK  one column per wave          N <= 8192, K <= 4096
//   LPR 64, KMAX kGemvMaxK  long rows in segments        N <= 8192, 4096 < K <= 8192
//   LPR 16                  wide, grid-strided + argmax  N > 8192 (K <= 4096)
// The weight element type WT is a template argument of the one body: bf16_t (gemv) or int8_t
// (gemv_w8: int8 rows with a power-of-two fp32 scale per row -- the W8 rule in common.h).  A lane's
// 8-column chunk is then 8 bytes instead of 16, float(q) takes the bf16 weight's place in the same
// chain, and the folded sum is multiplied by the row's scale (exact) before the epilogue, so the
// output bits are the bf16 kernel's on the dequantized matrix.
#include "common.h"
#include "kernels.h"

using namespace mg;

namespace {

constexpr int kGemvMaxB = 8;
constexpr int kGemvMaxK = 2 * kGemvSegK;  // narrow outputs: two segments of x (kernels.h kGemvSegK)

MG_DEVICE unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// Fused greedy argmax, first half: every workgroup publishes its best (value, index) key per row
// to part[b][workgroup] with plain stores, and workgroup 0 advances the device position.  The
// cross-workgroup reduction is the NEXT kernel's (the decode step's embedding kernel, at a launch
// boundary: no atomics, no hand-off).  A last-arrival reduction inside this kernel cost ~5 us per
// token (store drain + returning atomics on counters; MI355X_MICROARCH 'dequeue').
template <int B>
MG_DEVICE void gemv_argmax(const GemvArgmax& am, const unsigned long long (&key)[B], bool mine, int row) {
  __shared__ unsigned long long kk[B][16];
  if (mine) {  // this lane's best over the rows it produced (0: none)
#pragma unroll
    for (int b = 0; b < B; ++b) kk[b][row] = key[b];
  }
  __syncthreads();
  if (threadIdx.x < B) {
    unsigned long long best = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) best = umax64(best, kk[threadIdx.x][r]);
    am.part[(long)threadIdx.x * gridDim.x + blockIdx.x] = best;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *am.pos += 1;  // nothing else in this kernel reads it
}

// A lane's 8-column chunk of a weight row: 16 bytes of bf16 or 8 bytes of int8, read with the
// default or the non-temporal policy; a chunk past K is zero.
template <class WT>
struct WChunk;
template <>
struct WChunk<bf16_t> {
  typedef uint4 type;
  static MG_DEVICE uint4 zero() { return make_uint4(0, 0, 0, 0); }
  template <bool NT>
  static MG_DEVICE uint4 ld(const bf16_t* p) { return NT ? ld16_nt(p) : ld16(p); }
  static MG_DEVICE void unpack(const uint4& u, float (&f)[8]) { unpack8(u, f); }
};
template <>
struct WChunk<int8_t> {
  typedef uint2 type;
  static MG_DEVICE uint2 zero() { return make_uint2(0, 0); }
  template <bool NT>
  static MG_DEVICE uint2 ld(const int8_t* p) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    const v2u v = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p)) : *reinterpret_cast<const v2u*>(p);
    return make_uint2(v[0], v[1]);
  }
  // 8 x int8 -> 8 x f32 (exact), column order = byte order
  static MG_DEVICE void unpack(const uint2& u, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[e] = (float)(int8_t)(u.x >> (8 * e));
      f[4 + e] = (float)(int8_t)(u.y >> (8 * e));
    }
  }
};

// The FMA chain of one 8-column chunk: weight chunk w against the B staged rows' chunks at xcol,
// xcol + ldx, ...  A lane's sum is this chain over its chunks in ascending column order (e = 0..7
// within a chunk, rows inner), whichever path runs it: tests/_gemv_oracle.py restates it.
template <int B, class WT>
MG_DEVICE void gemv_fma(const typename WChunk<WT>::type& w, const bf16_t* xcol, int ldx, float (&acc)[B]) {
  float wf[8];
  WChunk<WT>::unpack(w, wf);
#pragma unroll
  for (int b = 0; b < B; ++b) {
    float xf[8];
    unpack8(ld16(xcol + b * ldx), xf);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[b] = __builtin_fmaf(wf[e], xf[e], acc[b]);
  }
}

// KMAX: the longest row an instantiation takes (kGemvMaxK: one column per wave only); LPR: lanes per
// output row.  The body is: request the weight row (one column per wave), stage x, then one of
// the three paths.  The paths are blocks of this body and the LayerNorm passes a lambda in it, not
// device functions beside gemv_fma: -ffp-contract leaves to the compiler which of the LayerNorm's
// squares fuse with their add, and that choice -- the staged bits -- changed for some B whenever
// this code was compiled from inside another function (PERF.md 'Decode projections refactor').
// scale: one fp32 per output column for int8 weights (the folded sum times it is the dot product
// with the dequantized row); not read for bf16 weights.
template <int B, int LPR, bool NTW, int KMAX = kGemvSegK, class WT = bf16_t>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16_t* __restrict__ x,
                                                   const WT* __restrict__ W,
                                                   bf16_t* __restrict__ y, int N, int K, long ldy,
                                                   const bf16_t* __restrict__ bias,
                                                   const bf16_t* __restrict__ resid, int epi,
                                                   const bf16_t* __restrict__ lnw,
                                                   const bf16_t* __restrict__ lnb, float eps,
                                                   const GemvArgmax am,
                                                   const float* __restrict__ scale) {
  typedef WChunk<WT> WC;
  typedef typename WC::type wchunk_t;
  constexpr bool W8 = std::is_same<WT, int8_t>::value;
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];  // [B][K]; long rows: [B][kGemvSegK]
  constexpr bool LONGK = KMAX > kGemvSegK;
  static_assert(!LONGK || LPR == 64, "rows longer than kGemvSegK: one row per wave only");
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  constexpr int RPW = 64 / LPR;  // rows per wave
  const int g = lane / LPR, j = lane % LPR;
  const int n = (blockIdx.x * 4 + wid) * RPW + g;
  constexpr int STRIDE = LPR * 8;  // elements per load round of a row
  // one row per wave: the whole row (K <= 4096: <= 8 loads per lane; LONGK: <= 16) is requested
  // before x is staged and normalised, so the weight stream's memory latency overlaps the LayerNorm's
  constexpr int NPF = LPR == 64 ? KMAX / STRIDE : 1;
  wchunk_t wpf[NPF];
  if constexpr (LPR == 64) {
    const WT* wr = W + (long)min(n, N - 1) * K;
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
      const int c = j * 8 + u * STRIDE;
      wpf[u] = c < K ? WC::template ld<NTW>(wr + c) : WC::zero();
    }
  }
  if (!LONGK && lnw) {  // (LONGK: no fused LayerNorm -- a LayerNorm'ed row is at most 4096 wide)
    // fused LayerNorm of the B input rows (wave w normalises rows w, w+4): the same lane/chunk
    // order and wave reduction as ln_fwd_kernel, so the staged bf16 rows equal its output.  Three
    // passes over a lane's chunks c = 8 lane + 512 u (sum, sum of squares, write), written once
    // over how a chunk is obtained.  HELD = 2 (K <= 1024: GPT-2 small / medium): the row, gamma and
    // beta chunks are loaded once into registers (one memory round trip instead of three dependent
    // L2 reads), zero past K; HELD = 0 (wider rows): every pass re-reads its chunks
    auto stage_ln = [&](auto held) {
      constexpr int HELD = decltype(held)::value;
      for (int b = wid; b < B; b += 4) {
        const bf16_t* xr = x + (long)b * K;
        constexpr int NH = HELD ? HELD : 1;
        uint4 xv[NH], wv[NH], bv[NH];
        if constexpr (HELD > 0) {
#pragma unroll
          for (int u = 0; u < HELD; ++u) {
            const int c = lane * 8 + u * 512;
            const bool ok = c < K;
            xv[u] = ok ? ld16(xr + c) : make_uint4(0, 0, 0, 0);
            wv[u] = ok ? ld16(lnw + c) : make_uint4(0, 0, 0, 0);
            bv[u] = ok ? ld16(lnb + c) : make_uint4(0, 0, 0, 0);
          }
        }
        auto each = [&](auto&& f) {  // f(u, c) for the lane's chunks; HELD: the zero ones past K too
          if constexpr (HELD > 0) {
#pragma unroll
            for (int u = 0; u < HELD; ++u) f(u, lane * 8 + u * 512);
          } else {
            for (int c = lane * 8; c < K; c += 512) f(0, c);
          }
        };
        float s = 0.f;
        each([&](int u, int c) {
          float v[8];
          unpack8(HELD ? xv[u] : ld16(xr + c), v);
#pragma unroll
          for (int e = 0; e < 8; ++e) s += v[e];  // zero chunks past K add nothing
        });
        const float mu = wave_sum(s) / K;
        float ss = 0.f;
        each([&](int u, int c) {
          if (c < K) {
            float v[8];
            unpack8(HELD ? xv[u] : ld16(xr + c), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float d = v[e] - mu;
              ss += d * d;
            }
          }
        });
        const float rs = rsqrtf(wave_sum(ss) / K + eps);
        each([&](int u, int c) {
          if (c < K) {
            float v[8], wf[8], bf[8], o[8];
            unpack8(HELD ? xv[u] : ld16(xr + c), v);
            unpack8(HELD ? wv[u] : ld16(lnw + c), wf);
            unpack8(HELD ? bv[u] : ld16(lnb + c), bf);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[e] - mu) * rs * wf[e] + bf[e];
            st16(xs + b * K + c, pack8(o));
          }
        });
      }
    };
    if (K <= 1024) stage_ln(std::integral_constant<int, 2>{});
    else stage_ln(std::integral_constant<int, 0>{});
  } else if constexpr (!LONGK) {
    for (int i = threadIdx.x * 8; i < B * K; i += 256 * 8) st16(xs + i, ld16(x + i));
  }
  if constexpr (!LONGK) __syncthreads();
  // a row's LPR lanes fold with xor-shuffles; lane j == 0 applies the epilogue and writes y[b, n]
  auto epilogue = [&](float (&acc)[B], int n) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
      for (int o = 1; o < LPR; o <<= 1) acc[b] += __shfl_xor(acc[b], o, 64);
    }
    if (n < N && j == 0) {
      const float bv = bias ? bf2f(bias[n]) : 0.f;
      float sc = 1.f;
      if constexpr (W8) sc = scale[n];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if constexpr (W8) acc[b] *= sc;  // a power of two: exact
        const bf16_t o = proj_epilogue(acc[b], bv, epi, resid + (long)b * ldy + n);
        y[(long)b * ldy + n] = o;
        acc[b] = bf2f(o);  // the argmax ranks the stored (bf16) logits
      }
    }
  };
  float acc[B];
#pragma unroll
  for (int b = 0; b < B; ++b) acc[b] = 0.f;
  if constexpr (LONGK) {
    // ---- long rows in segments: kGemvSegK < K <= kGemvMaxK, one column per wave.  The whole weight
    // row was requested up front (16 chunks per lane); x goes through the LDS buffer in segments of
    // kGemvSegK columns, [B][kGemvSegK], with a workgroup barrier between segments -- segment s + 1's
    // weight chunks and its x chunks are in flight (or already in registers) while segment s is
    // multiplied.  Chosen over whole-row staging (B x 8192 x 2 B = 128 KiB: an opt-in above the
    // 64 KiB dynamic-LDS default and one workgroup per CU): 64 KiB keeps two workgroups on a CU, so
    // the 320 / 400 workgroups of the gpt2-large / -xl MLP projection are all resident on the 256
    // CUs at once instead of running as one full round and a part-filled second.  A lane's sum is
    // the same chain either way: chunks u = 0, 1, ... in order, 8 fmas each, then the xor fold.
    constexpr int UPS = kGemvSegK / STRIDE;  // weight chunks per lane and segment
    constexpr int CPT = kGemvSegK / (256 * 8);  // x chunks per thread, row and segment
    constexpr int NSEG = KMAX / kGemvSegK;
    uint4 xv[B][CPT];  // a segment of x on its way to LDS: requested one segment ahead
    auto load_x = [&](int s0) {
#pragma unroll
      for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int h = 0; h < CPT; ++h) {
          const int c = s0 + (threadIdx.x + h * 256) * 8;
          xv[b][h] = c < K ? ld16(x + (long)b * K + c) : make_uint4(0, 0, 0, 0);
        }
      }
    };
    load_x(0);
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
      const int s0 = s * kGemvSegK;
      if (s0 < K) {  // K is uniform over the workgroup: so are the barriers
        if (s > 0) __syncthreads();  // every wave is done reading the previous segment
#pragma unroll
        for (int b = 0; b < B; ++b) {
#pragma unroll
          for (int h = 0; h < CPT; ++h) {
            const int c = (threadIdx.x + h * 256) * 8;
            if (s0 + c < K) st16(xs + b * kGemvSegK + c, xv[b][h]);
          }
        }
        __syncthreads();
        if (s + 1 < NSEG) load_x(s0 + kGemvSegK);
#pragma unroll
        for (int u = s * UPS; u < (s + 1) * UPS; ++u) {
          const int c = j * 8 + u * STRIDE;
          if (c < K) gemv_fma<B, WT>(wpf[u], xs + c - s0, kGemvSegK, acc);
        }
      }
    }
    epilogue(acc, n);
  } else if constexpr (LPR == 64) {
    // ---- one column per wave: the block projections (N <= 8192, K <= kGemvSegK), N / 4 workgroups,
    // a wave's 64 lanes on one column with the whole row's loads in flight at once.  (16 lanes per
    // row, the wide path's layout, left most of the chip idle at these 48-192 workgroups and the
    // HBM latency exposed.)
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
      const int c = j * 8 + u * STRIDE;
      if (c < K) gemv_fma<B, WT>(wpf[u], xs + c, K, acc);
    }
    epilogue(acc, n);
  } else {
    // ---- wide, grid-strided, with the fused argmax: N > 8192 (the LM head), 16 lanes per output
    // row and 4 rows per wave; a grid of a few hundred workgroups (gemv_grid) strides over the
    // 16-row blocks, each staging x once, and the fused argmax pays its cross-workgroup hand-off
    // once per workgroup
    unsigned long long best[B];
#pragma unroll
    for (int b = 0; b < B; ++b) best[b] = 0ull;
    // work items = (16-row block, 1024-column segment); the next item's 8 chunks per lane are
    // requested before the current item's FMAs, so every lane keeps a full item in flight
    const int nrb = (N + 15) / 16;
    const int nseg = (K + 16 * 8 * 8 - 1) / (16 * 8 * 8);
    const int nit = (blockIdx.x < nrb ? (nrb - 1 - blockIdx.x) / gridDim.x + 1 : 0) * nseg;
    auto load_item = [&](int it, wchunk_t (&r)[8]) {
      const int rb = blockIdx.x + (it / nseg) * gridDim.x, seg = it % nseg;
      const int nr = min((rb * 4 + wid) * RPW + g, N - 1);
      const WT* wr = W + (long)nr * K + seg * 1024;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = seg * 1024 + j * 8 + u * STRIDE;
        r[u] = c < K ? WC::template ld<NTW>(wr + j * 8 + u * STRIDE) : WC::zero();
      }
    };
    wchunk_t cur[8], nxt[8];
    if (nit > 0) load_item(0, cur);
    for (int it = 0; it < nit; ++it) {
      if (it + 1 < nit) load_item(it + 1, nxt);
      const int rb = blockIdx.x + (it / nseg) * gridDim.x, seg = it % nseg;
      const int nr = (rb * 4 + wid) * RPW + g;
      if (seg == 0) {
#pragma unroll
        for (int b = 0; b < B; ++b) acc[b] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = seg * 1024 + j * 8 + u * STRIDE;
        if (c < K) gemv_fma<B, WT>(cur[u], xs + c, K, acc);
      }
      if (seg == nseg - 1) {
        epilogue(acc, nr);
        if (am.part && nr < N && j == 0) {
#pragma unroll
          for (int b = 0; b < B; ++b) best[b] = umax64(best[b], amax_key(acc[b], nr));
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) cur[u] = nxt[u];
    }
    if (am.part) gemv_argmax<B>(am, best, j == 0, wid * RPW + g);
  }
}

}  // namespace

namespace mg {

// K > kGemvSegK: narrow outputs (N <= 8192) without fused LayerNorm only (the bindings check)
bool gemv_supported(int B, int K) { return B >= 1 && B <= kGemvMaxB && K % 8 == 0 && K <= kGemvMaxK; }

// wide outputs: a few workgroups per CU, grid-striding over the 16-row blocks -- at most
// MINGPT_GEMV_WIDE_GRID (default 512) of them when the variable is set or B > 2, else 1024
// (B <= 2: twice the workgroups -- the LM head's 16-row blocks are then latency-, not
// bandwidth-bound: 3,359 / 3,335 vs 3,319 / 3,302 tok/s at B = 1, equal at B = 8;
// profiles/round2_s8_decode_gemv_policy_ab.jsonl)
int gemv_grid(int N, int B) {
  if (N <= 8192) return cdiv(N, 4);
  static const char* const env = getenv("MINGPT_GEMV_WIDE_GRID");
  static const int cap = env && atoi(env) > 0 ? atoi(env) : 512;
  return min(cdiv(N, 16), (env || B > 2) ? cap : 1024);
}
// weight loads non-temporal (default) or default cache policy (MINGPT_GEMV_NT=0): the decode step
// re-reads the same ~250 MB of GPT-2 weights every token, about the Infinity Cache's size
bool gemv_nt_weights() {
  static int nt = -1;
  if (nt < 0) {
    const char* e = getenv("MINGPT_GEMV_NT");
    nt = e ? atoi(e) != 0 : 1;
  }
  return nt != 0;
}

namespace {
// the launch of gemv (WT bf16_t, scale null) and gemv_w8 (WT int8_t)
template <class WT>
void gemv_launch(const bf16_t* x, const WT* W, const float* scale, bf16_t* y, int B, int N, int K, long ldy,
                 const bf16_t* bias, const bf16_t* resid, int epi, hipStream_t stream, const bf16_t* lnw,
                 const bf16_t* lnb, float eps, const GemvArgmax* am) {
  const bool longk = K > kGemvSegK;  // x staged in segments of kGemvSegK columns
  const size_t smem = sizeof(bf16_t) * (size_t)B * (longk ? kGemvSegK : K);
  // one row per wave (N / 4 workgroups) up to ~8k outputs; 4 rows per wave beyond (the LM head
  // already launches thousands of workgroups and re-stages x in each)
  const bool wide = N > 8192;
  const int grid = gemv_grid(N, B);
  const GemvArgmax amv = am ? *am : GemvArgmax{nullptr, nullptr};
  // the one launch: B, the path (LPR, KMAX) and the weight-load policy pick the instantiation
  auto launch = [&](auto b, auto lpr, auto kmax) {
    dispatch_bool(gemv_nt_weights(), [&](auto nt) {
      gemv_kernel<decltype(b)::value, decltype(lpr)::value, decltype(nt)::value, decltype(kmax)::value, WT>
          <<<grid, 256, smem, stream>>>(x, W, y, N, K, ldy, bias, resid, epi, lnw, lnb, eps, amv, scale);
    });
  };
  auto rows = [&](auto b) {
    if (longk) launch(b, std::integral_constant<int, 64>{}, std::integral_constant<int, kGemvMaxK>{});
    else if (wide) launch(b, std::integral_constant<int, 16>{}, std::integral_constant<int, kGemvSegK>{});
    else launch(b, std::integral_constant<int, 64>{}, std::integral_constant<int, kGemvSegK>{});
  };
  switch (B) {  // exact row counts: the kernel stages and writes exactly B rows
    case 1: rows(std::integral_constant<int, 1>{}); break;
    case 2: rows(std::integral_constant<int, 2>{}); break;
    case 3: rows(std::integral_constant<int, 3>{}); break;
    case 4: rows(std::integral_constant<int, 4>{}); break;
    case 5: rows(std::integral_constant<int, 5>{}); break;
    case 6: rows(std::integral_constant<int, 6>{}); break;
    case 7: rows(std::integral_constant<int, 7>{}); break;
    case 8: rows(std::integral_constant<int, 8>{}); break;
    default: break;
  }
}
}  // namespace

void gemv(const bf16_t* x, const bf16_t* W, bf16_t* y, int B, int N, int K, long ldy, const bf16_t* bias,
          const bf16_t* resid, int epi, hipStream_t stream, const bf16_t* lnw, const bf16_t* lnb,
          float eps, const GemvArgmax* am) {
  gemv_launch<bf16_t>(x, W, nullptr, y, B, N, K, ldy, bias, resid, epi, stream, lnw, lnb, eps, am);
}

bool gemv_w8_supported(int B, int K) { return gemv_supported(B, K); }

void gemv_w8(const bf16_t* x, const int8_t* Wq, const float* scale, bf16_t* y, int B, int N, int K, long ldy,
             const bf16_t* bias, const bf16_t* resid, int epi, hipStream_t stream, const bf16_t* lnw,
             const bf16_t* lnb, float eps, const GemvArgmax* am) {
  gemv_launch<int8_t>(x, Wq, scale, y, B, N, K, ldy, bias, resid, epi, stream, lnw, lnb, eps, am);
}

}  // namespace mg
