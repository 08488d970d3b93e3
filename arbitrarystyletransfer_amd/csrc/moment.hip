// Moment-matching style loss (the l_m of STROTSS; Kolkin et al., CVPR 2019) for gfx950, fp32 storage:
// L1 distance between the channel means and between the channel covariances of two feature maps,
// with a backward to the first map. The definition is in include/ast_hip.h; tests/moment_ref.py
// restates it.
//   statistics   plane means (shifted one-pass sum, exact for a constant plane), then the centred
//                product (x - mu)(x - mu)^T over the upper-triangle tiles only, split along the
//                pixels (the tile and the split rule of mm_tile.h, shared with wct.hip); the partial
//                tiles meet in a workspace and are summed in split order and scaled by 1 / (M - 1).
//                For the target (ast_moment_stats_f32) the tile is mirrored into cov; the style's
//                statistics are computed once and reused across iterations.
//   forward      the same product for x; its reduce epilogue subtracts the target tile, writes the
//                sign of the difference as int8 to (i, j) and (j, i) from one register and sums
//                |d| per tile pair in a fixed order (an off-diagonal element counts twice).
//                Cov(x) is never stored. One workgroup per sample then forms the sample's term
//                (and sign_mu), and one workgroup adds weight / n * their sum into the accumulator.
//   backward     one GEMM S . (X - mu_x), C x C by C x M per sample: S staged from int8, the centring
//                staged into the second operand, the mean term, scale and accumulate in the epilogue.
// Every product is v_mfma_f32_32x32x2_f32 on fp32 operands. No floating-point atomics, no host
// synchronisation, no allocation; every sample is indexed by a grid dimension, so a non-finite value
// stays inside its own sample; every sum has a fixed order, so two runs agree in bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "det.h"
#include "match_tile.h"
#include "mm_tile.h"
#include "wave.h"
#include "ws.h"

namespace {

using ast_mm::f32x16;
using ast_mm::kT;
using ast_mm::tile_mm;
using ast_mm::tri_tile;
using ast_mm::WK;
using ast_mm::WP;
using ast_mm::WT;
using ast_wave::block_sum;

// +1 / -1 / 0 for d > 0 / d < 0 / otherwise (zero and NaN)
__device__ __forceinline__ signed char sign_of(float d) { return d > 0.f ? 1 : (d < 0.f ? -1 : 0); }

// mean[p] of plane p: x0 + sum(x - x0) / M with x0 the plane's first element, so a constant plane
// has exactly its value as mean (its centred values and its covariance row are then exactly 0).
__global__ __launch_bounds__(kT) void moment_mean_kernel(const float* __restrict__ x, float* __restrict__ mean,
                                                        int64_t M) {
  __shared__ float sh[kT / 64];
  const float* p = x + (int64_t)blockIdx.x * M;
  const float x0 = p[0];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < M; i += kT) s += p[i] - x0;
  s = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) mean[blockIdx.x] = x0 + s / (float)M;
}

// grid (upper-triangle tile pairs, K splits, samples): one dense 64x64 partial tile each.
__global__ __launch_bounds__(kT) void moment_cov_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                       float* __restrict__ part, int C, int64_t M, int kchunk) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  int ti, tj;
  tri_tile(blockIdx.x, C, ti, tj);
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

// grid (tile pairs, samples): the splits of every element in split order, / (M - 1). A diagonal tile
// keeps its i <= j half. LOSS false: the value goes to cov (i, j) and (j, i). LOSS true: d = value -
// ycov (i, j); its sign goes to (i, j) and (j, i) of sign_cov, and lpart[b, pair] = sum |d| over the
// tile's elements (twice off the diagonal), per thread in element order, then over the workgroup.
template <bool LOSS>
__global__ __launch_bounds__(kT) void moment_reduce_kernel(const float* __restrict__ part, float* __restrict__ cov,
                                                          const float* __restrict__ ycov, int64_t ystride,
                                                          signed char* __restrict__ sign_cov,
                                                          float* __restrict__ lpart, int C, int splits, float denom) {
  __shared__ float sh[kT / 64];
  int ti, tj;
  tri_tile(blockIdx.x, C, ti, tj);
  const int b = blockIdx.y;
  const int64_t tile = WT * WT, sstride = (int64_t)gridDim.x * tile, cc = (int64_t)C * C;
  const float* P = part + (int64_t)b * splits * sstride + (int64_t)blockIdx.x * tile;
  float total = 0.f;
  for (int e = threadIdx.x; e < WT * WT; e += kT) {
    const int i = ti * WT + e / WT, j = tj * WT + e % WT;
    if (i >= C || j >= C || (ti == tj && i > j)) continue;
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += P[k * sstride + e];
    s /= denom;
    if (LOSS) {
      const float d = s - ycov[b * ystride + (int64_t)i * C + j];
      const signed char sg = sign_of(d);
      signed char* S = sign_cov + b * cc;
      S[(int64_t)i * C + j] = sg;
      S[(int64_t)j * C + i] = sg;
      const float a = fabsf(d);
      total += i == j ? a : a + a;
    } else {
      float* S = cov + b * cc;
      S[(int64_t)i * C + j] = s;
      S[(int64_t)j * C + i] = s;
    }
  }
  if (LOSS) {
    total = block_sum<kT / 64>(total, sh);
    if (threadIdx.x == 0) lpart[(int64_t)b * gridDim.x + blockIdx.x] = total;
  }
}

// grid (samples): sign_mu and sums[b] = (1/C) sum_c |mu_x - mu_y| + (1/C^2) sum over the tile pairs
__global__ __launch_bounds__(kT) void moment_sample_kernel(const float* __restrict__ mean_x,
                                                          const float* __restrict__ mean_y, int64_t ystride,
                                                          const float* __restrict__ lpart,
                                                          signed char* __restrict__ sign_mu,
                                                          float* __restrict__ sums, int C, int pairs) {
  __shared__ float sh[kT / 64];
  const int b = blockIdx.x;
  const float* mx = mean_x + (int64_t)b * C;
  const float* my = mean_y + b * ystride;
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += kT) {
    const float d = mx[c] - my[c];
    sign_mu[(int64_t)b * C + c] = sign_of(d);
    s += fabsf(d);
  }
  const float smu = block_sum<kT / 64>(s, sh);
  s = 0.f;
  for (int k = threadIdx.x; k < pairs; k += kT) s += lpart[(int64_t)b * pairs + k];
  const float scov = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) sums[b] = smu / (float)C + scov / ((float)C * (float)C);
}

// one workgroup: *loss += w_over_n * sum over the samples, in sample order per thread
__global__ __launch_bounds__(kT) void moment_total_kernel(const float* __restrict__ sums, float* loss, int n,
                                                         float w_over_n) {
  __shared__ float sh[kT / 64];
  float s = 0.f;
  for (int b = threadIdx.x; b < n; b += kT) s += sums[b];
  const float t = block_sum<kT / 64>(s, sh);
  ast_det::loss_acc_commit(loss, w_over_n * t);
}

// grid (pixel tiles, channel tiles, samples):
//   dx[b, c, m] (+)= g (amu sign_mu[c] + acov sum_k S[c, k] (x[k, m] - mu_x[k]))
template <bool ACC>
__global__ __launch_bounds__(kT) void moment_backward_kernel(const float* __restrict__ x,
                                                            const float* __restrict__ mean_x,
                                                            const signed char* __restrict__ sign_mu,
                                                            const signed char* __restrict__ sign_cov,
                                                            const float* __restrict__ gscale, float* __restrict__ dx,
                                                            int C, int64_t M, float amu, float acov) {
  __shared__ float As[WK * WP];
  __shared__ float Bs[WK * WP];
  const int b = blockIdx.z, m0 = blockIdx.y * WT, n0 = blockIdx.x * WT;
  const float* X = x + (int64_t)b * C * M;
  const signed char* S = sign_cov + (int64_t)b * C * C;
  const f32x16 acc = tile_mm<false, false, signed char>(S, C, nullptr, X, M, mean_x + (int64_t)b * C, C, (int)M, m0,
                                                        n0, 0, C, As, Bs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int n = n0 + (wave >> 1) * 32 + r;
  if (n >= M) return;
  const float g = gscale ? *gscale : 1.f;
  const signed char* sm = sign_mu + (int64_t)b * C;
  float* O = dx + (int64_t)b * C * M + n;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = m0 + (wave & 1) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (m >= C) continue;
    const float v = g * (amu * (float)sm[m] + acov * acc[i]);
    O[(int64_t)m * M] = ACC ? O[(int64_t)m * M] + v : v;
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layouts, launch sequences
// ------------------------------------------------------------------------------------------------

using ast_tile::tiles_of;  // WT = 64

// AST_OK, or the code that rejects (samples, channels, pixels per plane)
inline int stats_shape(int n, int c, int64_t m) {
  if (n <= 0 || c <= 0 || m < 2 || m > 0x7fffffffLL || n > 32767) return AST_E_SHAPE;
  if (c > AST_MOMENT_MAX_C) return AST_E_UNSUPPORTED;
  return AST_OK;
}

// The pixel splits and the pixels per split (a multiple of 32): the library's rule (mm_tile.h) for
// forced == 0, else `forced` splits, clamped so that every split has pixels (the test hook).
inline int moment_splits(int64_t m, int forced, int* kchunk) {
  if (forced <= 0) return ast_mm::cov_splits(m, kchunk);
  const int64_t s = std::min<int64_t>(forced, (m + 31) / 32);
  const int64_t kc = (((m + s - 1) / s) + 31) / 32 * 32;
  if (kchunk) *kchunk = (int)kc;
  return (int)((m + kc - 1) / kc);
}

inline int pairs_of(int c) {
  const int t = tiles_of(c);
  return t * (t + 1) / 2;
}

// Statistics: [partial tiles: samples x splits x tile pairs x 64 x 64]
struct StatsWs {
  float* part;
  int64_t bytes;
};

inline StatsWs stats_ws(void* base, int n, int c, int64_t m, int forced) {
  ast_ws::Walk wk(base);
  const int splits = moment_splits(m, forced, nullptr);
  return {wk.take<float>((int64_t)4 * n * splits * pairs_of(c) * (WT * WT)), wk.off};
}

// Forward: [partial tiles | |d| sums: samples x tile pairs]
struct LossWs {
  float *part, *lpart;
  int64_t bytes;
};

inline LossWs loss_ws(void* base, int n, int c, int64_t m, int forced) {
  ast_ws::Walk wk(base);
  const int splits = moment_splits(m, forced, nullptr);
  return {wk.take<float>((int64_t)4 * n * splits * pairs_of(c) * (WT * WT)), wk.take<float>((int64_t)4 * n * pairs_of(c)),
          wk.off};
}

// mean, then the partial tiles of the centred product; returns the split count
int product_launch(const float* x, float* mean, float* part, int n, int c, int64_t m, int forced, hipStream_t st) {
  int kchunk = 0;
  const int splits = moment_splits(m, forced, &kchunk);
  hipLaunchKernelGGL(moment_mean_kernel, dim3((unsigned)(n * c)), dim3(kT), 0, st, x, mean, m);
  hipLaunchKernelGGL(moment_cov_kernel, dim3(pairs_of(c), splits, n), dim3(kT), 0, st, x, (const float*)mean, part, c, m,
                     kchunk);
  return splits;
}

}  // namespace

extern "C" {

long long ast_moment_stats_workspace_bytes(int n, int c, long long m, int splits) {
  const int e = stats_shape(n, c, m);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  return stats_ws(nullptr, n, c, m, splits).bytes;
}

int ast_moment_stats_f32(const float* y, float* mean, float* cov, int n, int c, long long m, int splits,
                         void* workspace, long long workspace_bytes, void* stream) {
  if (!y || !mean || !cov || !workspace) return AST_E_NULLPTR;
  const int e = stats_shape(n, c, m);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  const StatsWs ws = stats_ws(workspace, n, c, m, splits);
  if (workspace_bytes < ws.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int ns = product_launch(y, mean, ws.part, n, c, m, splits, st);
  hipLaunchKernelGGL((moment_reduce_kernel<false>), dim3(pairs_of(c), n), dim3(kT), 0, st, (const float*)ws.part, cov,
                     (const float*)nullptr, (int64_t)0, (signed char*)nullptr, (float*)nullptr, c, ns, (float)(m - 1));
  return (int)hipGetLastError();
}

long long ast_moment_loss_workspace_bytes(int n, int c, long long m, int splits) {
  const int e = stats_shape(n, c, m);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  return loss_ws(nullptr, n, c, m, splits).bytes;
}

int ast_moment_loss_f32(const float* x, const float* y_mean, const float* y_cov, float* mean_x,
                        signed char* sign_mu, signed char* sign_cov, float* sums, float* loss, int n, int ns, int c,
                        long long m, float weight, int splits, void* workspace, long long workspace_bytes,
                        void* stream) {
  if (!x || !y_mean || !y_cov || !mean_x || !sign_mu || !sign_cov || !sums || !loss || !workspace)
    return AST_E_NULLPTR;
  const int e = stats_shape(n, c, m);
  if (e) return e;
  if (ns != n && ns != 1) return AST_E_SHAPE;
  if (splits < 0) return AST_E_UNSUPPORTED;
  const LossWs ws = loss_ws(workspace, n, c, m, splits);
  if (workspace_bytes < ws.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int pairs = pairs_of(c);
  const int nsplit = product_launch(x, mean_x, ws.part, n, c, m, splits, st);
  hipLaunchKernelGGL((moment_reduce_kernel<true>), dim3(pairs, n), dim3(kT), 0, st, (const float*)ws.part,
                     (float*)nullptr, y_cov, ns == 1 ? (int64_t)0 : (int64_t)c * c, sign_cov, ws.lpart, c, nsplit,
                     (float)(m - 1));
  hipLaunchKernelGGL(moment_sample_kernel, dim3(n), dim3(kT), 0, st, (const float*)mean_x, y_mean,
                     ns == 1 ? (int64_t)0 : (int64_t)c, (const float*)ws.lpart, sign_mu, sums, c, pairs);
  hipLaunchKernelGGL(moment_total_kernel, dim3(1), dim3(kT), 0, st, (const float*)sums, loss, n, weight / (float)n);
  return (int)hipGetLastError();
}

int ast_moment_loss_backward_f32(const float* x, const float* mean_x, const signed char* sign_mu,
                                 const signed char* sign_cov, const float* gscale, float* dx, int n, int c,
                                 long long m, float weight, int accumulate, void* stream) {
  if (!x || !mean_x || !sign_mu || !sign_cov || !dx) return AST_E_NULLPTR;
  const int e = stats_shape(n, c, m);
  if (e) return e;
  hipStream_t st = (hipStream_t)stream;
  const double wn = (double)weight / (double)n;
  const float amu = (float)(wn / ((double)c * (double)m));
  const float acov = (float)(2.0 * wn / ((double)c * (double)c * (double)(m - 1)));
  const dim3 grid((unsigned)((m + WT - 1) / WT), tiles_of(c), n);
  if (accumulate)
    hipLaunchKernelGGL((moment_backward_kernel<true>), grid, dim3(kT), 0, st, x, mean_x, sign_mu, sign_cov, gscale, dx,
                       c, (int64_t)m, amu, acov);
  else
    hipLaunchKernelGGL((moment_backward_kernel<false>), grid, dim3(kT), 0, st, x, mean_x, sign_mu, sign_cov, gscale, dx,
                       c, (int64_t)m, amu, acov);
  return (int)hipGetLastError();
}

}  // extern "C"
