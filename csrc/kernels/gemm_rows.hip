// Rows GEMM for batched decode on gfx950: y[M, ldy] = epi(x[M, K] @ W[N, K]^T), 1 <= M <= 64.
//
// A decode step at 9..64 rows is past the skinny GEMM (gemv.hip: per-lane FMA chains, 8 rows at the
// most) and far below the training GEMM's tiles (gemm.hip at M = B: one row tile, 6-24 workgroups
// walking K one tile at a time).  The work is still one stream of the weight matrix, read once,
// with the rows of x riding along -- here as MFMA operands (v_mfma_f32_16x16x32_bf16):
//   * a workgroup (4 waves) owns 16 output columns n0 .. n0+15; N / 16 workgroups;
//   * W is the B operand: lane l holds B[k = 8 (l >> 4) + j][col l & 15] = W[n0 + (l & 15)][k0 + 8
//     (l >> 4) + j], 16 contiguous bytes of one weight row, loaded from global memory straight into
//     the fragment registers (non-temporal under gemv_nt_weights()); nothing of W passes LDS;
//   * x is the A operand, RT = ceil(M / 16) row tiles (a compile-time parameter) sharing every
//     weight fragment: lane l holds x[16 rt + (l & 15)][k0 + 8 (l >> 4) + j], read from L2 (x is at
//     most 1 MiB and every workgroup reads all of it; a workgroup's waves read disjoint k, so an
//     LDS image would be written and read once -- no reuse to stage for).  Rows from M on and
//     columns of k from K on are zero in the operand and never read;
//   * K is split over the 4 waves in 32-column steps, interleaved: wave w takes steps w, w + 4, ...
//     (at any moment the workgroup reads 256 contiguous bytes of each weight row), kRowsU (4) steps of
//     loads requested one group ahead of the MFMAs that use them;
//   * the 4 partial accumulators meet in LDS and are added in wave order, ((p0 + p1) + p2) + p3,
//     then gemv.hip's epilogue (proj_epilogue, common.h): bias | bias + GELU | bias + residual, no
//     dropout, one rounding to bf16.
// The split and the step order are functions of K alone and an MFMA computes each output row from
// that row's operand alone, so the bits of y[m, :] depend on x[m, :], W, bias, resid[m, :], epi, N
// and K -- not on M, the row's slot, the other rows' contents (NaN included), or graph / eager
// launch.  No atomics, no cross-workgroup hand-off; columns N .. ldy-1 of y are left untouched.
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "kernels.h"

using namespace mg;

namespace {

constexpr int kRowsMaxM = 64;
constexpr int kRowsMaxK = 8192;
// k-steps per load group; two groups (cur / nxt) in flight per lane.  MG_ROWS_U_NARROW (a build
// switch for A/B runs, PERF.md 'Rows GEMM') is the group of 1 and 2 row tiles; 3 and 4 row tiles keep
// 4 steps (8 would take 2 x (32 + 128) registers for the fragments alone)
#ifndef MG_ROWS_U_NARROW
#define MG_ROWS_U_NARROW 4
#endif
template <int RT>
constexpr int kRowsU = RT <= 2 ? MG_ROWS_U_NARROW : 4;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

MG_DEVICE f32x4 rows_mfma(const uint4& a, const uint4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                 c, 0, 0, 0);
}

template <int RT>
struct RowsFrag {
  uint4 w[kRowsU<RT>];
  uint4 x[kRowsU<RT>][RT];
};

template <int RT, bool NTW>
__global__ __launch_bounds__(256) void gemm_rows_kernel(const bf16_t* __restrict__ x,
                                                        const bf16_t* __restrict__ W,
                                                        bf16_t* __restrict__ y, int M, int N, int K, long ldy,
                                                        const bf16_t* __restrict__ bias,
                                                        const bf16_t* __restrict__ resid, int epi) {
  __shared__ f32x4 part[4][RT][64];  // [wave][row tile][lane]: 4 KiB per row tile
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  constexpr int U = kRowsU<RT>;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const bf16_t* wr = W + (long)min(n0 + r, N - 1) * K;  // columns past N: a valid row, never stored
  const bf16_t* xr[RT];
  bool xok[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int m = t * 16 + r;
    xok[t] = m < M;
    xr[t] = x + (long)min(m, M - 1) * K;
  }
  const int nstep = (K + 31) >> 5;                                   // 32-column k-steps of the row
  const int mine = wid < nstep ? (nstep - 1 - wid) / 4 + 1 : 0;      // steps w, w + 4, ...
  const int ngrp = (mine + U - 1) / U;
  auto load_group = [&](int g, RowsFrag<RT>& f) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = ((g * U + u) * 4 + wid) * 32 + q * 8;  // steps past the wave's last: c >= K
      const bool ok = c < K;
      f.w[u] = ok ? (NTW ? ld16_nt(wr + c) : ld16(wr + c)) : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < RT; ++t) f.x[u][t] = ok && xok[t] ? ld16(xr[t] + c) : make_uint4(0, 0, 0, 0);
    }
  };
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  RowsFrag<RT> cur, nxt;
  if (ngrp > 0) load_group(0, cur);
  for (int g = 0; g < ngrp; ++g) {
    if (g + 1 < ngrp) load_group(g + 1, nxt);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // a step past K multiplies zero fragments: +0 into the accumulator, the bits unchanged
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = rows_mfma(cur.x[u][t], cur.w[u], acc[t]);
    }
    if (g + 1 < ngrp) cur = nxt;
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) part[wid][t][lane] = acc[t];
  __syncthreads();
  // wave t finishes row tile t: C/D lane l, register i is row 4 (l >> 4) + i, column l & 15
  if (wid < RT) {
    const f32x4 s = ((part[0][wid][lane] + part[1][wid][lane]) + part[2][wid][lane]) + part[3][wid][lane];
    const int n = n0 + r;
    if (n < N) {
      const float bv = bias ? bf2f(bias[n]) : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = wid * 16 + q * 4 + i;
        if (m < M) y[(long)m * ldy + n] = proj_epilogue(s[i], bv, epi, resid + (long)m * ldy + n);
      }
    }
  }
}

}  // namespace

namespace mg {

bool gemm_rows_supported(int M, int K) {
  return M >= 1 && M <= kRowsMaxM && K >= 8 && K % 8 == 0 && K <= kRowsMaxK;
}

void gemm_rows(const bf16_t* x, const bf16_t* W, bf16_t* y, int M, int N, int K, long ldy, const bf16_t* bias,
               const bf16_t* resid, int epi, hipStream_t stream) {
  const int grid = cdiv(N, 16);
  const bool ntw = gemv_nt_weights();
  // the one launch: the row tiles and the weight-load policy pick the instantiation
  auto launch = [&](auto rt) {
    dispatch_bool(ntw, [&](auto nt) {
      gemm_rows_kernel<decltype(rt)::value, decltype(nt)::value><<<grid, 256, 0, stream>>>(x, W, y, M, N, K, ldy,
                                                                                           bias, resid, epi);
    });
  };
  switch (cdiv(M, 16)) {  // row tiles: rows past M are zero operands, never stored
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default:  // the caller checks gemm_rows_supported: nothing is launched, y is left as it was
#ifdef MG_DEBUG
      fprintf(stderr, "gemm_rows: M = %d outside 1..%d\n", M, kRowsMaxM);
      abort();
#endif
      break;
  }
}

}  // namespace mg
