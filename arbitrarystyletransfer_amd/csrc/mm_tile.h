// The 64x64 centred fp32-MFMA product tile shared by wct.hip (covariance, Newton-Schulz, apply) and
// moment.hip (covariance, sign GEMM), and the pixel split of a covariance. Device code and the
// split rule only, no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "match_tile.h"

namespace ast_mm {

using ast_tile::f32x16;
constexpr int kT = 256;                 // threads per workgroup of every kernel that calls tile_mm
constexpr int WT = 64, WK = 32, WP = WT + 1, WL = WK * WT / kT;
constexpr int kMaxSplits = 8;           // covariance K splits per sample

namespace {

// ------------------------------------------------------------------------------------------------
// One 64x64 tile of (A - amu) . (B - bmu) over k in [kbeg, kend), as this wave's 32x32 accumulator.
// A is k-contiguous: A(m, k) = A[m * lda + k]. B is either k-contiguous as well (BKFAST, B(k, n) =
// B[n * ldb + k]: the covariance, whose second operand is the first one transposed) or
// n-contiguous (B(k, n) = B[k * ldb + n]). amu / bmu (null: none) are indexed by the operand's row
// in memory -- m for A, n for a k-contiguous B, k for an n-contiguous one -- and are subtracted while
// staging; elements past M, N or kend are staged as 0, not as -mu.
// Accumulator element i of a lane is row wm * 32 + (i & 3) + 8 (i >> 2) + 4 h, column wn * 32 + r.
// GATHER (the regional kernels): the pixel axis of the map -- k of both operands when BKFAST, else the
// n of B -- is read through idx, so logical pixel j is element idx[j] of its plane; kbeg, kend, n0 and
// N then count logical pixels. Without it idx is unused and the code is the ungathered one.
// TA: the storage type of A, converted to fp32 while staging (moment.hip's int8 sign matrix).
// ------------------------------------------------------------------------------------------------
template <bool BKFAST, bool GATHER = false, typename TA = float>
__device__ __forceinline__ f32x16 tile_mm(const TA* __restrict__ A, int64_t lda, const float* __restrict__ amu,
                                          const float* __restrict__ B, int64_t ldb, const float* __restrict__ bmu,
                                          int M, int N, int m0, int n0, int kbeg, int kend, float* As, float* Bs,
                                          const int* __restrict__ idx = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int k_f = tid & 31, r_f = tid >> 5;  // k-contiguous operand: k = k_f, row = r_f + 8 i
  const int n_f = tid & 63, k_s = tid >> 6;  // n-contiguous B: column n_f, k = k_s + 4 i
  float ra[WL], rb[WL], am[WL], bm[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    const int gm = m0 + r_f + 8 * i, gn = n0 + r_f + 8 * i;
    am[i] = (amu && gm < M) ? amu[gm] : 0.f;
    bm[i] = (BKFAST && bmu && gn < N) ? bmu[gn] : 0.f;
  }
  int pn = n0 + n_f;  // the n-contiguous B's column in memory
  if constexpr (GATHER && !BKFAST) pn = pn < N ? idx[pn] : 0;
  auto load = [&](int k0) {
    const int gk = k0 + k_f;
    int pk = gk;        // the k-contiguous operands' k in memory
    if constexpr (GATHER && BKFAST) pk = gk < kend ? idx[gk] : 0;
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int gm = m0 + r_f + 8 * i;
      ra[i] = (gk < kend && gm < M) ? (float)A[(int64_t)gm * lda + pk] - am[i] : 0.f;
    }
    if (BKFAST) {
#pragma unroll
      for (int i = 0; i < WL; ++i) {
        const int gn = n0 + r_f + 8 * i;
        rb[i] = (gk < kend && gn < N) ? B[(int64_t)gn * ldb + pk] - bm[i] : 0.f;
      }
    } else {
      const int gn = n0 + n_f;
#pragma unroll
      for (int i = 0; i < WL; ++i) {
        const int gk2 = k0 + k_s + 4 * i;
        rb[i] = (gk2 < kend && gn < N) ? B[(int64_t)gk2 * ldb + pn] - (bmu ? bmu[gk2] : 0.f) : 0.f;
      }
    }
  };
  f32x16 acc = (f32x16){0.f};
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += WK) {
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      As[k_f * WP + r_f + 8 * i] = ra[i];
      if (BKFAST) Bs[k_f * WP + r_f + 8 * i] = rb[i];
      else Bs[(k_s + 4 * i) * WP + n_f] = rb[i];
    }
    __syncthreads();
    if (k0 + WK < kend) load(k0 + WK);
#pragma unroll
    for (int kp = 0; kp < WK / 2; ++kp)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * kp + h) * WP + wm * 32 + r], Bs[(2 * kp + h) * WP + wn * 32 + r],
                                                 acc, 0, 0, 0);
    __syncthreads();
  }
  return acc;
}

// (ti, tj), ti <= tj, of upper-triangle tile pair p of a C x C matrix, rows first
__device__ __forceinline__ void tri_tile(int p, int C, int& ti, int& tj) {
  int rowlen = (C + WT - 1) / WT;
  ti = 0;
  while (p >= rowlen) {
    p -= rowlen;
    ++ti;
    --rowlen;
  }
  tj = ti + p;
}

}  // namespace

// K split of a covariance: chunks of at least 64 pixels (a multiple of 32), at most kMaxSplits. The
// host sizes the unmasked launch with it; a regional workgroup evaluates it for its region's size.
__host__ __device__ inline int cov_splits(int64_t m, int* kchunk) {
  int64_t s = (m + 63) / 64;
  if (s > kMaxSplits) s = kMaxSplits;
  const int64_t kc = (((m + s - 1) / s) + 31) / 32 * 32;
  if (kchunk) *kchunk = (int)kc;
  return (int)((m + kc - 1) / kc);
}

}  // namespace ast_mm
