// Whitening and colouring transform (WCT; Li et al., NeurIPS 2017) for gfx950, fp32 storage. The
// definition is in include/ast_hip.h; tests/wct_ref.py restates it. Three stages, each a C-ABI entry
// of its own, and ast_wct_f32 is exactly their composition:
//   covariance    plane means (shifted one-pass sum, exact for a constant plane), then the centred
//                 product (x - mu)(x - mu)^T over the upper-triangle tiles only, split along the
//                 pixels; the partial tiles meet in a workspace and are summed in split order, scaled
//                 by 1/(M - 1), mirrored into the lower triangle, and the ridge goes on the diagonal
//   roots         coupled Newton-Schulz: per iteration P = 1.5 I - 0.5 Z Y (epilogue fused), then
//                 [Y; Z] <- [Y P; P Z] as one launch of 2 * batch products between two buffers
//   apply         T = S^(1/2)_style . S^(-1/2)_content, then out = alpha (T (x - mu_c) + mu_s) +
//                 (1 - alpha) x as one GEMM with the centring staged into the operand and the bias
//                 and blend in the epilogue
// The regional form (ast_wct_regions_f32 and its stages, further down) bins the pixels of a label map
// by region once and runs the same covariance and apply products through that permutation.
// Every product is v_mfma_f32_32x32x2_f32 on fp32 operands (the tile of mbtrain.hip's gemm_kernel:
// 64x64 per workgroup, 4 waves x 32x32, K in chunks of 32 through LDS with the next chunk's loads in
// flight). Tiles past a matrix edge are zero-filled while staging, so any C in 1..1024 and any
// plane size run the same code. No atomics, no host synchronisation, no allocation: every sample is
// indexed by a grid dimension, so a non-finite value stays inside its own sample.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "match_tile.h"
#include "mm_tile.h"
#include "wave.h"
#include "ws.h"

namespace {

using ast_mm::cov_splits;
using ast_mm::f32x16;
using ast_mm::kMaxSplits;
using ast_mm::kT;  // threads per workgroup everywhere in this file
using ast_mm::tile_mm;  // the 64x64 centred product tile (mm_tile.h)
using ast_mm::WK;
using ast_mm::WP;
using ast_mm::WT;
constexpr int kMaxC = 1024;
constexpr float kTraceFloor = 1e-20f;

// Sum (order A) / max of v over the workgroup in a fixed order; every thread receives the result.
using ast_wave::block_max;
using ast_wave::block_sum;

// ------------------------------------------------------------------------------------------------
// Covariance
// ------------------------------------------------------------------------------------------------

// mean[p] of plane p: x0 + sum(x - x0) / M with x0 the plane's first element, so a constant plane
// has exactly its value as mean (its centred values, trace and covariance are then exactly 0).
__global__ __launch_bounds__(kT) void wct_mean_kernel(const float* __restrict__ x, float* __restrict__ mean, int64_t M) {
  __shared__ float sh[kT / 64];
  const float* p = x + (int64_t)blockIdx.x * M;
  const float x0 = p[0];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < M; i += kT) s += p[i] - x0;
  s = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) mean[blockIdx.x] = x0 + s / (float)M;
}

// grid (upper-triangle tile pairs, K splits, samples): one dense 64x64 partial tile each.
__global__ __launch_bounds__(kT) void wct_cov_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                    float* __restrict__ part, int C, int64_t M, int kchunk) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  int p = blockIdx.x, ti = 0, rowlen = (C + WT - 1) / WT;
  while (p >= rowlen) {
    p -= rowlen;
    ++ti;
    --rowlen;
  }
  const int tj = ti + p;
  const int b = blockIdx.z, ks = blockIdx.y;
  const int kbeg = ks * kchunk, kend = (int)min((int64_t)kbeg + kchunk, M);
  const float* X = x + (int64_t)b * C * M;
  const float* mu = mean + (int64_t)b * C;
  const f32x16 acc = tile_mm<true>(X, M, mu, X, M, mu, C, C, ti * WT, tj * WT, kbeg, kend, As, Bs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  float* P = part + (((int64_t)b * gridDim.y + ks) * gridDim.x + blockIdx.x) * (WT * WT) + wn * 32 + r;
#pragma unroll
  for (int i = 0; i < 16; ++i) P[(wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * WT] = acc[i];
}

// grid (tile pairs, samples): the splits of every element in split order, / (M - 1), written to
// (i, j) and (j, i) from the same register; a diagonal tile keeps its i <= j half.
__global__ __launch_bounds__(kT) void wct_cov_reduce_kernel(const float* __restrict__ part, float* __restrict__ cov,
                                                           int C, int splits, float denom) {
  int p = blockIdx.x, ti = 0, rowlen = (C + WT - 1) / WT;
  while (p >= rowlen) {
    p -= rowlen;
    ++ti;
    --rowlen;
  }
  const int tj = ti + p, b = blockIdx.y;
  const int64_t tile = WT * WT, sstride = (int64_t)gridDim.x * tile;
  const float* P = part + (int64_t)b * splits * sstride + (int64_t)blockIdx.x * tile;
  float* S = cov + (int64_t)b * C * C;
  for (int e = threadIdx.x; e < WT * WT; e += kT) {
    const int i = ti * WT + e / WT, j = tj * WT + e % WT;
    if (i >= C || j >= C || (ti == tj && i > j)) continue;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += P[k * sstride + e];
    s /= denom;
    S[(int64_t)i * C + j] = s;
    S[(int64_t)j * C + i] = s;
  }
}

// grid (samples): eps = eps_rel * max(tr / C, floor) on the C real diagonal entries.
__global__ __launch_bounds__(kT) void wct_ridge_kernel(float* __restrict__ cov, int C, float eps_rel) {
  __shared__ float sh[kT / 64];
  float* S = cov + (int64_t)blockIdx.x * C * C;
  float t = 0.f;
  for (int i = threadIdx.x; i < C; i += kT) t += S[(int64_t)i * C + i];
  t = block_sum<kT / 64>(t, sh);
  const float eps = eps_rel * fmaxf(t / (float)C, kTraceFloor);
  for (int i = threadIdx.x; i < C; i += kT) S[(int64_t)i * C + i] += eps;
}

// ------------------------------------------------------------------------------------------------
// Newton-Schulz
// ------------------------------------------------------------------------------------------------

// grid (matrices): norm[b] = ||S||_F as max|s| * sqrt(sum (s / max|s|)^2), so neither a tiny matrix
// (the 1e-23 ridge of a constant map) nor a huge one leaves the fp32 range under the square.
__global__ __launch_bounds__(kT) void wct_norm_kernel(const float* __restrict__ cov, float* __restrict__ norm, int C) {
  __shared__ float sh[kT / 64];
  const int64_t cc = (int64_t)C * C;
  const float* S = cov + (int64_t)blockIdx.x * cc;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < cc; i += kT) m = fmaxf(m, fabsf(S[i]));
  m = block_max<kT / 64>(m, sh);
  __syncthreads();
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < cc; i += kT) {
    const float v = S[i] / m;
    s += v * v;
  }
  s = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) norm[blockIdx.x] = m * sqrtf(s);
}

// grid (elements / 256, matrices): Y0 = S / ||S||_F, Z0 = I.
__global__ __launch_bounds__(kT) void wct_ns_init_kernel(const float* __restrict__ cov, const float* __restrict__ norm,
                                                        float* __restrict__ Y, float* __restrict__ Z, int C) {
  const int64_t cc = (int64_t)C * C, e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= cc) return;
  const int64_t o = (int64_t)blockIdx.y * cc + e;
  Y[o] = cov[o] / norm[blockIdx.y];
  Z[o] = (e / C == e % C) ? 1.f : 0.f;
}

// grid (elements / 256, matrices): S^(1/2) = Y sqrt(||S||_F), S^(-1/2) = Z / sqrt(||S||_F).
__global__ __launch_bounds__(kT) void wct_ns_final_kernel(const float* __restrict__ Y, const float* __restrict__ Z,
                                                         const float* __restrict__ norm, float* __restrict__ root,
                                                         float* __restrict__ iroot, int C) {
  const int64_t cc = (int64_t)C * C, e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e >= cc) return;
  const int64_t o = (int64_t)blockIdx.y * cc + e;
  const float q = sqrtf(norm[blockIdx.y]);
  if (root) root[o] = Y[o] * q;
  if (iroot) iroot[o] = Z[o] / q;
}

// Batched square products of C x C row-major matrices, grid (tiles, tiles, products).
//   kStepP   P[z] = 1.5 I - 0.5 Z[z] Y[z]                        (yz = [Y; Z], `batch` of each)
//   kStepYZ  z < batch: Yn[z] = Y[z] P[z];  else Zn[z'] = P[z'] Z[z'], z' = z - batch
//   kPlain   out[z] = A[z * sA] B[z * sB]                         (T = S^(1/2)_style S^(-1/2)_content)
enum { kStepP = 0, kStepYZ = 1, kPlain = 2 };

template <int MODE>
__global__ __launch_bounds__(kT) void wct_sq_gemm_kernel(const float* __restrict__ a0, const float* __restrict__ b0,
                                                        float* __restrict__ out, int64_t sA, int64_t sB, int C,
                                                        int batch) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  const int64_t cc = (int64_t)C * C;
  const int z = blockIdx.z;
  const float *A, *B;
  if (MODE == kStepP) {          // a0 = [Y; Z]
    A = a0 + (int64_t)(batch + z) * cc;
    B = a0 + (int64_t)z * cc;
  } else if (MODE == kStepYZ) {  // a0 = [Y; Z], b0 = P
    if (z < batch) {
      A = a0 + (int64_t)z * cc;
      B = b0 + (int64_t)z * cc;
    } else {
      A = b0 + (int64_t)(z - batch) * cc;
      B = a0 + (int64_t)z * cc;
    }
  } else {
    A = a0 + (int64_t)z * sA;
    B = b0 + (int64_t)z * sB;
  }
  const int m0 = blockIdx.y * WT, n0 = blockIdx.x * WT;
  const f32x16 acc = tile_mm<false>(A, C, nullptr, B, C, nullptr, C, C, m0, n0, 0, C, As, Bs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int n = n0 + (wave >> 1) * 32 + r;
  if (n >= C) return;
  float* O = out + (int64_t)z * cc + n;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = m0 + (wave & 1) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (m >= C) continue;
    O[(int64_t)m * C] = MODE == kStepP ? (m == n ? 1.5f : 0.f) - 0.5f * acc[i] : acc[i];
  }
}

// ------------------------------------------------------------------------------------------------
// Apply: out[b] = alpha (T[b] (x[b] - mu_c[b]) + mu_s[b']) + (1 - alpha) x[b], grid (pixel tiles,
// channel tiles, samples); b' = b, or 0 for a shared style (smu_stride = 0).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void wct_apply_kernel(const float* __restrict__ T, const float* __restrict__ x,
                                                      const float* __restrict__ cmu, const float* __restrict__ smu,
                                                      float* __restrict__ out, int C, int64_t M, int64_t smu_stride,
                                                      float alpha) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  const int b = blockIdx.z;
  const float* X = x + (int64_t)b * C * M;
  const float* Tb = T + (int64_t)b * C * C;
  const int m0 = blockIdx.y * WT, n0 = blockIdx.x * WT;
  const f32x16 acc = tile_mm<false>(Tb, C, nullptr, X, M, cmu + (int64_t)b * C, C, (int)M, m0, n0, 0, C, As, Bs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t n = n0 + (wave >> 1) * 32 + r;
  if (n >= M) return;
  const float* ms = smu + (int64_t)b * smu_stride;
  float* O = out + (int64_t)b * C * M + n;
  const float beta = 1.f - alpha;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = m0 + (wave & 1) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (m >= C) continue;
    const float t = acc[i] + ms[m];
    O[(int64_t)m * M] = alpha * t + beta * X[(int64_t)m * M + n];
  }
}

// ------------------------------------------------------------------------------------------------
// Regional WCT: the pixels of a sample are binned by region once (a permutation of the pixel indices
// and K counts); every later kernel reads its pixel axis through that permutation and so does the
// MFMA work of the unmasked transform, whatever K. Bin K holds the pass-through pixels (label >= K).
// No grid size depends on the labels: a workgroup that finds nothing to do in the counts exits
// before its first barrier (the counts are uniform over a workgroup, so all its threads leave).
// ------------------------------------------------------------------------------------------------

constexpr int kBins = AST_MAX_REGIONS + 1;
constexpr int64_t kMaxRegionM = (int64_t)1 << 24;  // pixels per plane: one workgroup bins a sample

// grid (samples): perm[b] = the pixel indices of sample b ordered by (min(label, K), pixel index),
// count[b, k] = the pixels labelled k. Thread t owns the contiguous chunk [t * chunk, (t + 1) * chunk)
// of the pixels: it counts its chunk per bin, the kBins * 256 counts are scanned in (bin, thread)
// order through LDS, and it then writes its pixels at its offsets. Integer sums, no atomics.
__global__ __launch_bounds__(kT) void wct_bin_kernel(const unsigned char* __restrict__ labels, int* __restrict__ perm,
                                                    int* __restrict__ count, int M, int K) {
  __shared__ int sc[kBins * kT];
  __shared__ int wtot[kT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned char* L = labels + (int64_t)blockIdx.x * M;
  int* P = perm + (int64_t)blockIdx.x * M;
  const int chunk = (M + kT - 1) / kT;
  const int beg = min(tid * chunk, M), end = min(beg + chunk, M);
  int c[kBins];
#pragma unroll
  for (int j = 0; j < kBins; ++j) c[j] = 0;
  for (int i = beg; i < end; ++i) {
    const int l = min((int)L[i], K);
#pragma unroll
    for (int j = 0; j < kBins; ++j) c[j] += l == j;
  }
#pragma unroll
  for (int j = 0; j < kBins; ++j) sc[j * kT + tid] = c[j];
  __syncthreads();
  // exclusive scan of sc[0 .. kBins * kT): thread t takes entries [t * kBins, (t + 1) * kBins)
  int loc[kBins], tot = 0;
#pragma unroll
  for (int j = 0; j < kBins; ++j) {
    loc[j] = tot;
    tot += sc[tid * kBins + j];
  }
  int inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int base = inc - tot;
  for (int i = 0; i < wave; ++i) base += wtot[i];
#pragma unroll
  for (int j = 0; j < kBins; ++j) sc[tid * kBins + j] = base + loc[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kBins; ++j) c[j] = sc[j * kT + tid];
  for (int i = beg; i < end; ++i) {
    const int l = min((int)L[i], K);
    int pos = 0;
#pragma unroll
    for (int j = 0; j < kBins; ++j) {
      pos = l == j ? c[j] : pos;
      c[j] += l == j;
    }
    P[pos] = i;
  }
  if (tid < K) count[blockIdx.x * K + tid] = sc[(tid + 1) * kT] - sc[tid * kT];
}

// The first pixel of region k in the permutation of its sample.
__device__ __forceinline__ int bin_offset(const int* __restrict__ cnt, int k) {
  int off = 0;
  for (int j = 0; j < k; ++j) off += cnt[j];
  return off;
}

// grid (channels, samples * K): wct_mean_kernel on the region's pixels in ascending pixel index; 0 for a
// region of fewer than 2 pixels.
__global__ __launch_bounds__(kT) void wct_region_mean_kernel(const float* __restrict__ x, const int* __restrict__ perm,
                                                            const int* __restrict__ count, float* __restrict__ mean,
                                                            int C, int M, int K) {
  __shared__ float sh[kT / 64];
  const int z = blockIdx.y, b = z / K, k = z % K;
  const int* cnt = count + b * K;
  const int mk = cnt[k];
  float* out = mean + (int64_t)z * C + blockIdx.x;
  if (mk < 2) {
    if (threadIdx.x == 0) *out = 0.f;
    return;
  }
  const int* idx = perm + (int64_t)b * M + bin_offset(cnt, k);
  const float* p = x + ((int64_t)b * C + blockIdx.x) * M;
  const float x0 = p[idx[0]];
  float s = 0.f;
  for (int i = threadIdx.x; i < mk; i += kT) s += p[idx[i]] - x0;
  s = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) *out = x0 + s / (float)mk;
}

// grid (upper-triangle tile pairs, region_slots(M), samples * K): wct_cov_kernel on the region's gathered
// map, with the split count and chunk that cov_splits gives for the region's own size (never more than
// region_slots(M), the bound over every region size up to M).
__global__ __launch_bounds__(kT) void wct_region_cov_kernel(const float* __restrict__ x, const int* __restrict__ perm,
                                                           const int* __restrict__ count, const float* __restrict__ mean,
                                                           float* __restrict__ part, int C, int M, int K) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  const int z = blockIdx.z, b = z / K, k = z % K, ks = blockIdx.y;
  const int* cnt = count + b * K;
  const int mk = cnt[k];
  if (mk < 2) return;
  int kchunk = 0;
  if (ks >= cov_splits(mk, &kchunk)) return;
  int p = blockIdx.x, ti = 0, rowlen = (C + WT - 1) / WT;
  while (p >= rowlen) {
    p -= rowlen;
    ++ti;
    --rowlen;
  }
  const int tj = ti + p;
  const int kbeg = ks * kchunk, kend = min(kbeg + kchunk, mk);
  const float* X = x + (int64_t)b * C * M;
  const float* mu = mean + (int64_t)z * C;
  const f32x16 acc = tile_mm<true, true>(X, M, mu, X, M, mu, C, C, ti * WT, tj * WT, kbeg, kend, As, Bs,
                                         perm + (int64_t)b * M + bin_offset(cnt, k));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  float* P = part + (((int64_t)z * gridDim.y + ks) * gridDim.x + blockIdx.x) * (WT * WT) + wn * 32 + r;
#pragma unroll
  for (int i = 0; i < 16; ++i) P[(wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * WT] = acc[i];
}

// grid (tile pairs, samples * K): wct_cov_reduce_kernel over the region's own splits (`slots` per region
// in the workspace); the identity for a region of fewer than 2 pixels.
__global__ __launch_bounds__(kT) void wct_region_reduce_kernel(const float* __restrict__ part,
                                                              const int* __restrict__ count, float* __restrict__ cov,
                                                              int C, int slots) {
  int p = blockIdx.x, ti = 0, rowlen = (C + WT - 1) / WT;
  while (p >= rowlen) {
    p -= rowlen;
    ++ti;
    --rowlen;
  }
  const int tj = ti + p, z = blockIdx.y, mk = count[z];
  const int splits = mk < 2 ? 0 : cov_splits(mk, nullptr);
  const float denom = (float)(mk - 1);
  const int64_t tile = WT * WT, sstride = (int64_t)gridDim.x * tile;
  const float* P = part + (int64_t)z * slots * sstride + (int64_t)blockIdx.x * tile;
  float* S = cov + (int64_t)z * C * C;
  for (int e = threadIdx.x; e < WT * WT; e += kT) {
    const int i = ti * WT + e / WT, j = tj * WT + e % WT;
    if (i >= C || j >= C || (ti == tj && i > j)) continue;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += P[k * sstride + e];
    s = splits ? s / denom : (i == j ? 1.f : 0.f);
    S[(int64_t)i * C + j] = s;
    S[(int64_t)j * C + i] = s;
  }
}

// grid (samples * K): wct_ridge_kernel; the identity of an invalid region stays as it is.
__global__ __launch_bounds__(kT) void wct_region_ridge_kernel(float* __restrict__ cov, const int* __restrict__ count,
                                                             int C, float eps_rel) {
  __shared__ float sh[kT / 64];
  if (count[blockIdx.x] < 2) return;
  float* S = cov + (int64_t)blockIdx.x * C * C;
  float t = 0.f;
  for (int i = threadIdx.x; i < C; i += kT) t += S[(int64_t)i * C + i];
  t = block_sum<kT / 64>(t, sh);
  const float eps = eps_rel * fmaxf(t / (float)C, kTraceFloor);
  for (int i = threadIdx.x; i < C; i += kT) S[(int64_t)i * C + i] += eps;
}

// grid (ceil((C * C + C) / 256), samples * K): the colouring matrix cmix[b, k] = sum_s w_s sroot[s] and
// the target mean mmix[b, k] = sum_s w_s smean[s] over the styles of non-zero weight in ascending s (the
// first term a product, the later ones fmaf), and valid[b, k]: the content region has 2 pixels or more,
// some weight is non-zero, and (scount given) so has region k of every style used. A style row is s, or
// s * K + k with `regional` statistics.
__global__ __launch_bounds__(kT) void wct_region_mix_kernel(const float* __restrict__ sroot, const float* __restrict__ smean,
                                                           const float* __restrict__ mix, const int* __restrict__ ccount,
                                                           const int* __restrict__ scount, float* __restrict__ cmix,
                                                           float* __restrict__ mmix, int* __restrict__ valid, int C, int K,
                                                           int S, int mix_stride, int regional) {
  const int z = blockIdx.y, b = z / K, k = z % K;
  const float* w = mix + (int64_t)b * mix_stride + k * S;
  const int64_t cc = (int64_t)C * C, e = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (e == 0) {
    int ok = ccount[z] >= 2, used = 0;
    for (int s = 0; s < S; ++s) {
      if (w[s] == 0.f) continue;
      used = 1;
      if (scount && scount[s * K + k] < 2) ok = 0;
    }
    valid[z] = ok & used;
  }
  if (e >= cc + C) return;
  const bool mat = e < cc;
  const float* src = mat ? sroot : smean;
  const int64_t stride = mat ? cc : C, el = mat ? e : e - cc;
  float acc = 0.f;
  bool first = true;
  for (int s = 0; s < S; ++s) {
    const float ws = w[s];
    if (ws == 0.f) continue;
    const float y = src[(int64_t)(regional ? s * K + k : s) * stride + el];
    acc = first ? ws * y : __fmaf_rn(ws, y, acc);
    first = false;
  }
  (mat ? cmix + (int64_t)z * cc : mmix + (int64_t)z * C)[el] = acc;
}

// grid (ceil(M / 64) + K + 1 column tiles, channel tiles, samples). A column tile is 64 consecutive
// entries of one bin of the permutation, found from the counts; tiles past the last bin exit. A tile of
// a valid region is wct_apply_kernel's on the gathered columns, scattered back through the
// permutation; a tile of the pass-through bin or of an invalid region copies its pixels. Every output
// element is written exactly once.
__global__ __launch_bounds__(kT) void wct_region_apply_kernel(const float* __restrict__ T, const float* __restrict__ x,
                                                             const int* __restrict__ perm, const int* __restrict__ count,
                                                             const int* __restrict__ valid, const float* __restrict__ cmu,
                                                             const float* __restrict__ mmix, float* __restrict__ out,
                                                             int C, int M, int K, float alpha) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  const int b = blockIdx.z;
  const int* cnt = count + b * K;
  int rest = M;
  for (int j = 0; j < K; ++j) rest -= cnt[j];
  int t = blockIdx.x, bin = 0, off = 0, nb = 0;
  for (; bin <= K; ++bin) {
    nb = bin < K ? cnt[bin] : rest;
    const int nt = (nb + WT - 1) / WT;
    if (t < nt) break;
    t -= nt;
    off += nb;
  }
  if (bin > K) return;
  const int z = b * K + bin, m0 = blockIdx.y * WT, n0 = t * WT;
  const int* idx = perm + (int64_t)b * M + off;
  const float* X = x + (int64_t)b * C * M;
  float* O = out + (int64_t)b * C * M;
  if (bin == K || valid[z] == 0) {
    const int j = n0 + (threadIdx.x & 63);
    if (j >= nb) return;
    const int64_t pix = idx[j];
#pragma unroll
    for (int i = 0; i < WT / (kT / 64); ++i) {
      const int m = m0 + (threadIdx.x >> 6) + (kT / 64) * i;
      if (m < C) O[(int64_t)m * M + pix] = X[(int64_t)m * M + pix];
    }
    return;
  }
  const f32x16 acc = tile_mm<false, true>(T + (int64_t)z * C * C, C, nullptr, X, M, cmu + (int64_t)z * C, C, nb, m0, n0,
                                          0, C, As, Bs, idx);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int j = n0 + (wave >> 1) * 32 + r;
  if (j >= nb) return;
  const int64_t n = idx[j];
  const float* ms = mmix + (int64_t)z * C;
  O += n;
  const float beta = 1.f - alpha;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = m0 + (wave & 1) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (m >= C) continue;
    const float v = acc[i] + ms[m];
    O[(int64_t)m * M] = alpha * v + beta * X[(int64_t)m * M + n];
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layouts, launch sequences
// ------------------------------------------------------------------------------------------------

using ast_ws::al256;
using ast_tile::tiles_of;  // WT = 64
inline bool eps_ok(float e) { return e >= 1e-4f && e <= 1.f; }

inline int default_iters(int c, float eps_rel) {
  return (int)ceil(log((double)c / (double)eps_rel) / log(2.25)) + 5;
}

// AST_OK, or the code that rejects (samples, channels, pixels per plane)
inline int cov_shape(int n, int c, int64_t m) {
  if (n <= 0 || c <= 0 || m < 2 || m > 0x7fffffffLL || n > 32767) return AST_E_SHAPE;
  if (c > kMaxC) return AST_E_UNSUPPORTED;
  return AST_OK;
}

// A workspace of one region is its size. Covariance partials, of the plain and of the regional stage:
// [slots x tile pairs x 64 x 64 per matrix]; the apply stage's: [T]
inline int64_t part_ws(int matrices, int c, int slots) {
  const int t = tiles_of(c);
  return al256((int64_t)4 * matrices * slots * (t * (t + 1) / 2) * (WT * WT));
}
inline int64_t cov_ws(int n, int c, int64_t m) { return part_ws(n, c, cov_splits(m, nullptr)); }
inline int64_t apply_ws(int n, int c) { return al256((int64_t)4 * n * c * c); }

// The Newton-Schulz iteration's workspace: [norm | Y, Z | Y, Z | P], the pairs ping-pong
struct SqrtWs {
  float *norm, *yz[2], *P;
  int64_t bytes;
};

inline SqrtWs sqrt_ws(void* base, int b, int c) {
  ast_ws::Walk wk(base);
  const int64_t mb = al256((int64_t)4 * b * c * c);  // one matrix per sample
  return {wk.take<float>((int64_t)4 * b), {wk.take<float>(2 * mb), wk.take<float>(2 * mb)}, wk.take<float>(mb), wk.off};
}

int cov_launch(const float* x, float* mean, float* cov, int n, int c, int64_t m, float eps_rel, float* part,
               hipStream_t st) {
  int kchunk = 0;
  const int splits = cov_splits(m, &kchunk), t = tiles_of(c), pairs = t * (t + 1) / 2;
  hipLaunchKernelGGL(wct_mean_kernel, dim3((unsigned)(n * c)), dim3(kT), 0, st, x, mean, m);
  hipLaunchKernelGGL(wct_cov_kernel, dim3(pairs, splits, n), dim3(kT), 0, st, x, (const float*)mean, part, c, m, kchunk);
  hipLaunchKernelGGL(wct_cov_reduce_kernel, dim3(pairs, n), dim3(kT), 0, st, (const float*)part, cov, c, splits,
                     (float)(m - 1));
  hipLaunchKernelGGL(wct_ridge_kernel, dim3(n), dim3(kT), 0, st, cov, c, eps_rel);
  return (int)hipGetLastError();
}

int sqrt_launch(const float* cov, float* root, float* iroot, int b, int c, int iters, void* wsp,
                hipStream_t st) {
  const SqrtWs ws = sqrt_ws(wsp, b, c);
  float *norm = ws.norm, *const *yz = ws.yz, *P = ws.P;
  const int64_t cc = (int64_t)c * c;
  const int t = tiles_of(c);
  const dim3 eg((unsigned)((cc + kT - 1) / kT), b);
  hipLaunchKernelGGL(wct_norm_kernel, dim3(b), dim3(kT), 0, st, cov, norm, c);
  hipLaunchKernelGGL(wct_ns_init_kernel, eg, dim3(kT), 0, st, cov, (const float*)norm, yz[0], yz[0] + b * cc, c);
  int cur = 0;
  for (int it = 0; it < iters; ++it, cur ^= 1) {
    hipLaunchKernelGGL(wct_sq_gemm_kernel<kStepP>, dim3(t, t, b), dim3(kT), 0, st, (const float*)yz[cur],
                       (const float*)nullptr, P, (int64_t)0, (int64_t)0, c, b);
    hipLaunchKernelGGL(wct_sq_gemm_kernel<kStepYZ>, dim3(t, t, 2 * b), dim3(kT), 0, st, (const float*)yz[cur],
                       (const float*)P, yz[cur ^ 1], (int64_t)0, (int64_t)0, c, b);
  }
  hipLaunchKernelGGL(wct_ns_final_kernel, eg, dim3(kT), 0, st, (const float*)yz[cur], (const float*)(yz[cur] + b * cc),
                     (const float*)norm, root, iroot, c);
  return (int)hipGetLastError();
}

int apply_launch(const float* content, const float* cmu, const float* smu, const float* sroot, const float* ciroot,
                 float* out, int n, int ns, int c, int64_t mc, float alpha, float* T, hipStream_t st) {
  const int64_t cc = (int64_t)c * c;
  const int t = tiles_of(c);
  hipLaunchKernelGGL(wct_sq_gemm_kernel<kPlain>, dim3(t, t, n), dim3(kT), 0, st, sroot, ciroot, T,
                     ns == 1 ? (int64_t)0 : cc, cc, c, n);
  hipLaunchKernelGGL(wct_apply_kernel, dim3((unsigned)((mc + WT - 1) / WT), t, n), dim3(kT), 0, st, (const float*)T,
                     content, cmu, smu, out, c, mc, ns == 1 ? (int64_t)0 : (int64_t)c, alpha);
  return (int)hipGetLastError();
}

int pair_shape(int n, int ns, int c, int64_t mc, int64_t ms) {
  if (n <= 0 || ns <= 0 || (ns != n && ns != 1)) return AST_E_SHAPE;
  int e = cov_shape(n, c, mc);
  if (e) return e;
  e = cov_shape(ns, c, ms);
  if (e) return e;
  return n + ns > 32767 ? AST_E_SHAPE : AST_OK;
}

// The matrices of a compound op: [mean | cov | sqrt | isqrt], b of each
struct MatWs {
  float *mean, *cov, *root, *iroot;
};

inline MatWs mat_ws(ast_ws::Walk& wk, int b, int c) {
  const int64_t mat = (int64_t)4 * b * c * c;
  return {wk.take<float>((int64_t)4 * b * c), wk.take<float>(mat), wk.take<float>(mat), wk.take<float>(mat)};
}

// The whole op's workspace: [mean | cov | sqrt | isqrt | scratch], content samples first, then the
// style's; the scratch is the covariance partials, then the iteration's buffers, then T, each laid
// out by its stage: stream order keeps them apart
struct WctWs {
  MatWs mat;
  void* scratch;
  int64_t bytes;
};

inline WctWs wct_ws(void* base, int n, int ns, int c, int64_t mc, int64_t ms) {
  ast_ws::Walk wk(base);
  return {mat_ws(wk, n + ns, c),
          wk.take<void>(std::max({cov_ws(n, c, mc), cov_ws(ns, c, ms), sqrt_ws(nullptr, n + ns, c).bytes, apply_ws(n, c)})),
          wk.off};
}

// ---- regional WCT ----

// AST_OK, or the code that rejects (samples, channels, plane, regions) of a labelled map
inline int region_shape(int n, int c, int h, int w, int regions) {
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || (int64_t)h * w > kMaxRegionM || regions < 1 ||
      regions > AST_MAX_REGIONS || (int64_t)n * regions > 32767)
    return AST_E_SHAPE;
  return c > kMaxC ? AST_E_UNSUPPORTED : AST_OK;
}

// The most splits that a region of a plane of m pixels can take: max of cov_splits(mk) over mk <= m.
// cov_splits is ceil(mk / 64) up to 448 pixels and kMaxSplits from 449 to 512, but dips below that
// beyond (6 at 513: chunks of 96), so cov_splits(m) itself is no bound.
inline int region_slots(int64_t m) { return m >= 64 * (kMaxSplits - 1) + 1 ? kMaxSplits : cov_splits(m, nullptr); }

inline int64_t region_part_ws(int n, int c, int64_t m, int k) { return part_ws(n * k, c, region_slots(m)); }

// The regional covariance stage's workspace: [permutation | partials]
struct RegionCovWs {
  int* perm;
  float* part;
  int64_t bytes;
};

inline RegionCovWs region_cov_ws(void* base, int n, int c, int64_t m, int k) {
  ast_ws::Walk wk(base);
  return {wk.take<int>((int64_t)4 * n * m), wk.take<float>(region_part_ws(n, c, m, k)), wk.off};
}

// The mixing and apply launches' workspace: [valid | mmix | cmix | T]
struct RegionMixWs {
  int* valid;
  float *mmix, *cmix, *T;
  int64_t bytes;
};

inline RegionMixWs region_mix_ws(void* base, int n, int c, int k) {
  ast_ws::Walk wk(base);
  const int64_t nk = (int64_t)4 * n * k;
  return {wk.take<int>(nk), wk.take<float>(nk * c), wk.take<float>(nk * c * c), wk.take<float>(nk * c * c), wk.off};
}

// The regional apply stage's workspace: [permutation | counts | the mixing and apply launches']
struct RegionApplyWs {
  int *perm, *count;
  void* mix;
  int64_t bytes;
};

inline RegionApplyWs region_apply_ws(void* base, int n, int c, int64_t m, int k) {
  ast_ws::Walk wk(base);
  return {wk.take<int>((int64_t)4 * n * m), wk.take<int>((int64_t)4 * n * k),
          wk.take<void>(region_mix_ws(nullptr, n, c, k).bytes), wk.off};
}

int bin_launch(const unsigned char* labels, int* perm, int* count, int n, int64_t m, int k, hipStream_t st) {
  hipLaunchKernelGGL(wct_bin_kernel, dim3(n), dim3(kT), 0, st, labels, perm, count, (int)m, k);
  return (int)hipGetLastError();
}

// mean [n, k, c] and cov [n, k, c, c] from a binned map
int region_cov_launch(const float* x, const int* perm, const int* count, float* mean, float* cov, int n, int c,
                      int64_t m, int k, float eps_rel, float* part, hipStream_t st) {
  const int slots = region_slots(m), t = tiles_of(c), pairs = t * (t + 1) / 2;
  hipLaunchKernelGGL(wct_region_mean_kernel, dim3(c, n * k), dim3(kT), 0, st, x, perm, count, mean, c, (int)m, k);
  hipLaunchKernelGGL(wct_region_cov_kernel, dim3(pairs, slots, n * k), dim3(kT), 0, st, x, perm, count,
                     (const float*)mean, part, c, (int)m, k);
  hipLaunchKernelGGL(wct_region_reduce_kernel, dim3(pairs, n * k), dim3(kT), 0, st, (const float*)part, count, cov, c,
                     slots);
  hipLaunchKernelGGL(wct_region_ridge_kernel, dim3(n * k), dim3(kT), 0, st, cov, count, c, eps_rel);
  return (int)hipGetLastError();
}

// out from a binned content map and the parts
int region_apply_launch(const float* content, const int* perm, const int* count, const float* cmean, const float* ciroot,
                        const float* smean, const float* sroot, const float* mix, const int* scount, float* out, int n,
                        int c, int64_t m, int k, int s, int mix_n, int regional, float alpha, void* wsp,
                        hipStream_t st) {
  const int64_t cc = (int64_t)c * c;
  const int t = tiles_of(c);
  const RegionMixWs ws = region_mix_ws(wsp, n, c, k);
  int* valid = ws.valid;
  float *mmix = ws.mmix, *cmix = ws.cmix, *T = ws.T;
  hipLaunchKernelGGL(wct_region_mix_kernel, dim3((unsigned)((cc + c + kT - 1) / kT), n * k), dim3(kT), 0, st, sroot, smean,
                     mix, count, scount, cmix, mmix, valid, c, k, s, mix_n == 1 ? 0 : k * s, regional);
  hipLaunchKernelGGL(wct_sq_gemm_kernel<kPlain>, dim3(t, t, n * k), dim3(kT), 0, st, (const float*)cmix, ciroot, T, cc,
                     cc, c, n * k);
  hipLaunchKernelGGL(wct_region_apply_kernel, dim3((unsigned)((m + WT - 1) / WT + k + 1), t, n), dim3(kT), 0, st,
                     (const float*)T, content, perm, count, (const int*)valid, cmean, (const float*)mmix, out, c, (int)m,
                     k, alpha);
  return (int)hipGetLastError();
}

inline int mix_shape(int n, int styles, int mix_n) {
  return (styles < 1 || styles > AST_MAX_STYLE_ROWS || (mix_n != 1 && mix_n != n)) ? AST_E_SHAPE : AST_OK;
}

// the checks of the whole op, in the order of the stages
int regions_shape(int n, int c, int hc, int wc, int regions, int styles, int hs, int ws, int style_regional, int mix_n) {
  int e = region_shape(n, c, hc, wc, regions);
  if (e) return e;
  e = mix_shape(n, styles, mix_n);
  if (e) return e;
  if (hs <= 0 || ws <= 0) return AST_E_SHAPE;
  e = style_regional ? region_shape(styles, c, hs, ws, regions) : cov_shape(styles, c, (int64_t)hs * ws);
  if (e) return e;
  return n * regions + styles * (style_regional ? regions : 1) > 32767 ? AST_E_SHAPE : AST_OK;
}

// The whole regional op's workspace: [mean | cov | sqrt | isqrt | content perm, counts | style perm,
// counts | scratch]: the n * regions content matrices first, then the styles'; the scratch is the
// covariance partials (the content's, then the styles', regional or plain), then the iteration's
// buffers, then the apply stage's, each laid out by its stage: stream order keeps them apart
struct RegionsWs {
  MatWs mat;
  int *cperm, *ccount, *sperm, *scount;
  void* scratch;
  int64_t bytes;
};

inline RegionsWs regions_ws(void* base, int n, int c, int64_t mc, int k, int s, int64_t ms, int style_regional) {
  ast_ws::Walk wk(base);
  const int b = n * k + s * (style_regional ? k : 1);
  const int64_t spart = style_regional ? region_part_ws(s, c, ms, k) : cov_ws(s, c, ms);
  return {mat_ws(wk, b, c), wk.take<int>((int64_t)4 * n * mc), wk.take<int>((int64_t)4 * n * k),
          wk.take<int>((int64_t)4 * s * ms), wk.take<int>((int64_t)4 * s * k),
          wk.take<void>(std::max({region_part_ws(n, c, mc, k), spart, sqrt_ws(nullptr, b, c).bytes,
                                  region_mix_ws(nullptr, n, c, k).bytes})),
          wk.off};
}

}  // namespace

extern "C" {

int ast_wct_default_iters(int c, float eps_rel) {
  if (c <= 0) return AST_E_SHAPE;
  if (c > kMaxC || !eps_ok(eps_rel)) return AST_E_UNSUPPORTED;
  return default_iters(c, eps_rel);
}

long long ast_wct_cov_workspace_bytes(int n, int c, long long m) {
  const int e = cov_shape(n, c, m);
  return e ? e : cov_ws(n, c, m);
}

int ast_wct_cov_f32(const float* x, float* mean, float* cov, int n, int c, long long m, float eps_rel, void* workspace,
                    long long workspace_bytes, void* stream) {
  if (!x || !mean || !cov || !workspace) return AST_E_NULLPTR;
  const int e = cov_shape(n, c, m);
  if (e) return e;
  if (!eps_ok(eps_rel)) return AST_E_UNSUPPORTED;
  if (workspace_bytes < cov_ws(n, c, m)) return AST_E_SHAPE;
  return cov_launch(x, mean, cov, n, c, m, eps_rel, (float*)workspace, (hipStream_t)stream);
}

long long ast_wct_sqrt_workspace_bytes(int b, int c) {
  if (b <= 0 || c <= 0 || b > 32767) return AST_E_SHAPE;
  if (c > kMaxC) return AST_E_UNSUPPORTED;
  return sqrt_ws(nullptr, b, c).bytes;
}

int ast_wct_sqrt_f32(const float* cov, float* sqrt_or_null, float* isqrt_or_null, int b, int c, int iters,
                     void* workspace, long long workspace_bytes, void* stream) {
  if (!cov || !workspace || (!sqrt_or_null && !isqrt_or_null)) return AST_E_NULLPTR;
  if (b <= 0 || c <= 0 || b > 32767) return AST_E_SHAPE;
  if (c > kMaxC || iters < 0) return AST_E_UNSUPPORTED;
  if (workspace_bytes < sqrt_ws(nullptr, b, c).bytes) return AST_E_SHAPE;
  if (iters == 0) iters = default_iters(c, 1e-3f);
  return sqrt_launch(cov, sqrt_or_null, isqrt_or_null, b, c, iters, workspace, (hipStream_t)stream);
}

long long ast_wct_apply_workspace_bytes(int n, int c) {
  if (n <= 0 || c <= 0 || n > 32767) return AST_E_SHAPE;
  if (c > kMaxC) return AST_E_UNSUPPORTED;
  return apply_ws(n, c);
}

int ast_wct_apply_f32(const float* content, const float* content_mean, const float* style_mean,
                      const float* style_sqrt, const float* content_isqrt, float* out, int n, int ns, int c,
                      long long mc, double alpha, void* workspace, long long workspace_bytes, void* stream) {
  if (!content || !content_mean || !style_mean || !style_sqrt || !content_isqrt || !out || !workspace)
    return AST_E_NULLPTR;
  if (ns <= 0 || (ns != n && ns != 1)) return AST_E_SHAPE;
  const int e = cov_shape(n, c, mc);
  if (e) return e;
  if (workspace_bytes < apply_ws(n, c)) return AST_E_SHAPE;
  return apply_launch(content, content_mean, style_mean, style_sqrt, content_isqrt, out, n, ns, c, mc, (float)alpha,
                      (float*)workspace, (hipStream_t)stream);
}

long long ast_wct_workspace_bytes(int n, int ns, int c, long long mc, long long ms) {
  const int e = pair_shape(n, ns, c, mc, ms);
  return e ? e : wct_ws(nullptr, n, ns, c, mc, ms).bytes;
}

int ast_wct_f32(const float* content, const float* style, float* out, int n, int ns, int c, int hc, int wc, int hs,
                int ws, double alpha, float eps_rel, int iters, void* workspace, long long workspace_bytes,
                void* stream) {
  if (!content || !style || !out || !workspace) return AST_E_NULLPTR;
  if (hc <= 0 || wc <= 0 || hs <= 0 || ws <= 0) return AST_E_SHAPE;
  const int64_t mc = (int64_t)hc * wc, ms = (int64_t)hs * ws;
  int e = pair_shape(n, ns, c, mc, ms);
  if (e) return e;
  if (!eps_ok(eps_rel) || iters < 0) return AST_E_UNSUPPORTED;
  const WctWs w = wct_ws(workspace, n, ns, c, mc, ms);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  if (iters == 0) iters = default_iters(c, eps_rel);
  hipStream_t st = (hipStream_t)stream;
  const int b = n + ns;
  const int64_t cc = (int64_t)c * c;
  float *mean = w.mat.mean, *cov = w.mat.cov, *root = w.mat.root, *iroot = w.mat.iroot;
  e = cov_launch(content, mean, cov, n, c, mc, eps_rel, (float*)w.scratch, st);
  if (e) return e;
  e = cov_launch(style, mean + (int64_t)n * c, cov + n * cc, ns, c, ms, eps_rel, (float*)w.scratch, st);
  if (e) return e;
  e = sqrt_launch(cov, root, iroot, b, c, iters, w.scratch, st);
  if (e) return e;
  return apply_launch(content, mean, mean + (int64_t)n * c, root + n * cc, iroot, out, n, ns, c, mc, (float)alpha,
                      (float*)w.scratch, st);
}

// ---- regional WCT ----

long long ast_wct_region_cov_workspace_bytes(int n, int c, int h, int w, int regions) {
  const int e = region_shape(n, c, h, w, regions);
  return e ? e : region_cov_ws(nullptr, n, c, (int64_t)h * w, regions).bytes;
}

int ast_wct_region_cov_f32(const float* x, const unsigned char* labels, float* mean, float* cov, int* count, int n,
                           int c, int h, int w, int regions, float eps_rel, void* workspace,
                           long long workspace_bytes, void* stream) {
  if (!x || !labels || !mean || !cov || !count || !workspace) return AST_E_NULLPTR;
  int e = region_shape(n, c, h, w, regions);
  if (e) return e;
  if (!eps_ok(eps_rel)) return AST_E_UNSUPPORTED;
  const int64_t m = (int64_t)h * w;
  const RegionCovWs s = region_cov_ws(workspace, n, c, m, regions);
  if (workspace_bytes < s.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  e = bin_launch(labels, s.perm, count, n, m, regions, st);
  if (e) return e;
  return region_cov_launch(x, s.perm, count, mean, cov, n, c, m, regions, eps_rel, s.part, st);
}

long long ast_wct_region_apply_workspace_bytes(int n, int c, int h, int w, int regions) {
  const int e = region_shape(n, c, h, w, regions);
  return e ? e : region_apply_ws(nullptr, n, c, (int64_t)h * w, regions).bytes;
}

int ast_wct_region_apply_f32(const float* content, const unsigned char* labels, const float* content_mean,
                             const float* content_isqrt, const float* style_mean, const float* style_sqrt,
                             const float* mix, const int* style_count_or_null, float* out, int n, int c, int h, int w,
                             int regions, int styles, int mix_n, int style_regional, double alpha, void* workspace,
                             long long workspace_bytes, void* stream) {
  if (!content || !labels || !content_mean || !content_isqrt || !style_mean || !style_sqrt || !mix || !out || !workspace)
    return AST_E_NULLPTR;
  int e = region_shape(n, c, h, w, regions);
  if (e) return e;
  e = mix_shape(n, styles, mix_n);
  if (e) return e;
  const int64_t m = (int64_t)h * w;
  const RegionApplyWs s = region_apply_ws(workspace, n, c, m, regions);
  if (workspace_bytes < s.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  e = bin_launch(labels, s.perm, s.count, n, m, regions, st);
  if (e) return e;
  return region_apply_launch(content, s.perm, s.count, content_mean, content_isqrt, style_mean, style_sqrt, mix,
                             style_regional ? style_count_or_null : nullptr, out, n, c, m, regions, styles, mix_n,
                             style_regional ? 1 : 0, (float)alpha, s.mix, st);
}

long long ast_wct_regions_workspace_bytes(int n, int c, int hc, int wc, int regions, int styles, int hs, int ws,
                                          int style_regional) {
  const int e = regions_shape(n, c, hc, wc, regions, styles, hs, ws, style_regional, 1);
  return e ? e : regions_ws(nullptr, n, c, (int64_t)hc * wc, regions, styles, (int64_t)hs * ws, style_regional).bytes;
}

int ast_wct_regions_f32(const float* content, const unsigned char* labels, const float* styles,
                        const unsigned char* style_labels_or_null, const float* mix, float* out, int n, int c, int hc,
                        int wc, int regions, int s, int hs, int ws, int mix_n, double alpha, float eps_rel, int iters,
                        void* workspace, long long workspace_bytes, void* stream) {
  if (!content || !labels || !styles || !mix || !out || !workspace) return AST_E_NULLPTR;
  const int reg = style_labels_or_null ? 1 : 0;
  int e = regions_shape(n, c, hc, wc, regions, s, hs, ws, reg, mix_n);
  if (e) return e;
  if (!eps_ok(eps_rel) || iters < 0) return AST_E_UNSUPPORTED;
  const int64_t mc = (int64_t)hc * wc, ms = (int64_t)hs * ws, cc = (int64_t)c * c;
  const RegionsWs w = regions_ws(workspace, n, c, mc, regions, s, ms, reg);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  if (iters == 0) iters = default_iters(c, eps_rel);
  hipStream_t st = (hipStream_t)stream;
  const int nk = n * regions, b = nk + s * (reg ? regions : 1);
  float *mean = w.mat.mean, *cov = w.mat.cov, *root = w.mat.root, *iroot = w.mat.iroot;
  int *cperm = w.cperm, *ccount = w.ccount, *sperm = w.sperm, *scount = w.scount;
  e = bin_launch(labels, cperm, ccount, n, mc, regions, st);
  if (e) return e;
  e = region_cov_launch(content, cperm, ccount, mean, cov, n, c, mc, regions, eps_rel, (float*)w.scratch, st);
  if (e) return e;
  float* smean = mean + (int64_t)nk * c;
  if (reg) {
    e = bin_launch(style_labels_or_null, sperm, scount, s, ms, regions, st);
    if (e) return e;
    e = region_cov_launch(styles, sperm, scount, smean, cov + nk * cc, s, c, ms, regions, eps_rel, (float*)w.scratch, st);
  } else {
    e = cov_launch(styles, smean, cov + nk * cc, s, c, ms, eps_rel, (float*)w.scratch, st);
  }
  if (e) return e;
  e = sqrt_launch(cov, root, iroot, b, c, iters, w.scratch, st);
  if (e) return e;
  return region_apply_launch(content, cperm, ccount, mean, iroot, smean, root + nk * cc, mix, reg ? scount : nullptr, out,
                             n, c, mc, regions, s, mix_n, reg, (float)alpha, w.scratch, st);
}

}  // extern "C"
