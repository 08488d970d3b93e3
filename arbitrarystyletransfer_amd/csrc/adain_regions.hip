// Regional multi-style AdaIN for gfx950: per-region content statistics, a per-region mix of style
// statistics and the normalise-affine-blend write, in one launch (an extension of AdaIN.forward,
// models.py:43-51; the reference has no counterpart).
//
// A uint8 label map [n, h, w], shared by the C planes of a sample, assigns every pixel to a region
// k < K or, with any label >= K, to "pass through". One workgroup per (n, c) plane, as adain.hip:
//   pass 1  per-region sum and pixel count             (plane from HBM, labels from HBM / L2)
//   pass 2  per-region sum of squared deviations       (plane and labels from L1 / L2)
//   pass 3  out = alpha*((c - mu_k)/sd_k*scale_k + shift_k) + beta*c, labels >= K copied bit for bit
// with (scale_k, shift_k) the region's weighted mix of the rows of a style-statistics table. Each
// thread keeps K partial sums in registers, selected by label compare (a pixel adds 0 to the regions
// it is not in, so a NaN never crosses regions); partials meet through 64-lane shuffles and LDS in a
// fixed order, so results are bitwise reproducible. Labels are compared and range-checked before
// they select anything: no address is ever formed from a label.
// Algorithmic bytes per plane: read hw floats + hw label bytes, write hw floats.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = AST_MAX_REGIONS;

using ast_wave::wave_sum;

// Sums of KT values over the 256-thread block (order A of wave.h, KT values at once); every thread
// gets the totals. `sh` holds kWaves rows.
template <int KT>
__device__ __forceinline__ void block_sum_k(float (&v)[KT], float (*sh)[kMaxK]) {
#pragma unroll
  for (int k = 0; k < KT; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k) sh[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) t += sh[i][k];
    v[k] = t;
  }
}

// f(value, label) over the plane: four pixels per 128-bit load with their labels in one 32-bit word
// (shifts and masks: no byte-vector unpacking) when VEC, else the same runs with scalar loads.
template <bool VEC, typename F>
__device__ __forceinline__ void for_pixels(const float* __restrict__ x, const unsigned char* __restrict__ lab,
                                           int64_t hw, F f) {
  if (VEC) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const uint32_t* l4 = reinterpret_cast<const uint32_t*>(lab);
    for (int64_t i = threadIdx.x; i < hw / 4; i += kThreads) {
      const float4 v = x4[i];
      const uint32_t l = l4[i];
      f(v.x, (int)(l & 255u));
      f(v.y, (int)((l >> 8) & 255u));
      f(v.z, (int)((l >> 16) & 255u));
      f(v.w, (int)(l >> 24));
    }
  } else {
    // the same pixels per thread in the same order (runs of four, a short last run), so a thread's
    // partial sums, and with them the results, have the bits of the vector path
    for (int64_t i = threadIdx.x; i < (hw + 3) / 4; i += kThreads) {
      const int64_t e = i * 4 + 4 < hw ? i * 4 + 4 : hw;
      for (int64_t j = i * 4; j < e; ++j) f(x[j], (int)lab[j]);
    }
  }
}

// Two-pass statistics of the regions k < KT of one plane: count, mean, and sd = sqrt(sum of squared
// deviations / (count - 1)) with no eps, as plane_stats of adain.hip (an empty region gives NaN
// mean and sd, a one-pixel region 0/0 = NaN sd). Every thread gets all of them.
// `shm` (kMaxK floats of LDS) holds the means for pass 2's lookup by range-checked label. Pixel
// counts are wave-uniform: the popcount of the label compare's lane mask, on the scalar unit.
template <int KT, bool VEC>
__device__ __forceinline__ void region_plane_stats(const float* __restrict__ x, const unsigned char* __restrict__ lab,
                                                   int64_t hw, float (*shf)[kMaxK], int (*shi)[kMaxK], float* shm,
                                                   int (&cnt)[KT], float (&mean)[KT], float (&sd)[KT]) {
  float s[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) s[k] = 0.f, cnt[k] = 0;
  for_pixels<VEC>(x, lab, hw, [&](float v, int l) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const bool hit = l == k;
      s[k] += hit ? v : 0.f;
      cnt[k] += __popcll(__ballot(hit));
    }
  });
  block_sum_k<KT>(s, shf);
  // cnt is already the wave's total
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k) shi[threadIdx.x >> 6][k] = cnt[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    cnt[k] = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) cnt[k] += shi[i][k];
    mean[k] = s[k] / (float)cnt[k];
    s[k] = 0.f;
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k) shm[k] = mean[k];
  }
  __syncthreads();
  for_pixels<VEC>(x, lab, hw, [&](float v, int l) {
    const float d = v - shm[l < KT ? l : 0];
    const float dd = d * d;
#pragma unroll
    for (int k = 0; k < KT; ++k) s[k] += l == k ? dd : 0.f;
  });
  block_sum_k<KT>(s, shf);
#pragma unroll
  for (int k = 0; k < KT; ++k) sd[k] = cnt[k] > 0 ? sqrtf(s[k] / (float)(cnt[k] - 1)) : __builtin_nanf("");
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Per-region (mu, sd, scale, shift), looked up by a range-checked label in pass 3.
__device__ __forceinline__ float blend(float v, const float4& p, float alpha, float beta) {
  return alpha * ((v - p.x) / p.y * p.z + p.w) + beta * v;
}

template <int KT>
__global__ __launch_bounds__(kThreads) void adain_regions_kernel(
    const float* __restrict__ content, const unsigned char* __restrict__ labels, const float* __restrict__ smean,
    const float* __restrict__ sstd, const float* __restrict__ mix, float* __restrict__ out, int64_t hw, int c,
    int regions, int rows, int mix_stride_n, float alpha, float beta, int swap) {
  __shared__ float shf[kWaves][kMaxK];
  __shared__ int shi[kWaves][kMaxK];
  __shared__ float shm[kMaxK];
  __shared__ float4 prm[kMaxK];
  const int64_t p = blockIdx.x;
  const int64_t n = p / c;
  const int ch = (int)(p % c);
  const float* x = content + p * hw;
  const unsigned char* lab = labels + n * hw;
  float* o = out + p * hw;

  // style mix: 32 lanes per region, rows t = lane, lane + 32; zero weights skipped (their rows may be NaN)
  {
    const int k = threadIdx.x >> 5, lane = threadIdx.x & 31;
    float am = 0.f, as = 0.f;
    if (k < regions) {
      const float* w = mix + n * mix_stride_n + (int64_t)k * rows;
      for (int t = lane; t < rows; t += 32) {
        const float wt = w[t];
        if (wt != 0.f) {
          am += wt * smean[(int64_t)t * c + ch];
          as += wt * sstd[(int64_t)t * c + ch];
        }
      }
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      am += __shfl_xor(am, off, 64);
      as += __shfl_xor(as, off, 64);
    }
    if (lane == 0 && k < kMaxK) prm[k] = make_float4(0.f, 0.f, swap ? am : as, swap ? as : am);
  }

  const bool vec = (hw & 3) == 0 && aligned16(x) && aligned16(o) && ((uintptr_t)lab & 3) == 0;
  int cnt[KT];
  float mean[KT], sd[KT];
  if (vec)
    region_plane_stats<KT, true>(x, lab, hw, shf, shi, shm, cnt, mean, sd);
  else
    region_plane_stats<KT, false>(x, lab, hw, shf, shi, shm, cnt, mean, sd);
  // (the block sums above put barriers between the prm writes of the mix and this update)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k) prm[k].x = mean[k], prm[k].y = sd[k];
  }
  __syncthreads();

  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const uint32_t* l4 = reinterpret_cast<const uint32_t*>(lab);
    float4* o4 = reinterpret_cast<float4*>(o);
    for (int64_t i = threadIdx.x; i < hw / 4; i += kThreads) {
      const float4 v = x4[i];
      const uint32_t l = l4[i];
      const int l0 = (int)(l & 255u), l1 = (int)((l >> 8) & 255u), l2 = (int)((l >> 16) & 255u), l3 = (int)(l >> 24);
      float4 r;
      r.x = l0 < regions ? blend(v.x, prm[l0 < regions ? l0 : 0], alpha, beta) : v.x;
      r.y = l1 < regions ? blend(v.y, prm[l1 < regions ? l1 : 0], alpha, beta) : v.y;
      r.z = l2 < regions ? blend(v.z, prm[l2 < regions ? l2 : 0], alpha, beta) : v.z;
      r.w = l3 < regions ? blend(v.w, prm[l3 < regions ? l3 : 0], alpha, beta) : v.w;
      o4[i] = r;
    }
  } else {
    for (int64_t i = threadIdx.x; i < hw; i += kThreads) {
      const float v = x[i];
      const int l = (int)lab[i];
      o[i] = l < regions ? blend(v, prm[l < regions ? l : 0], alpha, beta) : v;
    }
  }
}

// mean, std [n, regions, c] and count [n, regions] (written by the workgroup of channel 0).
template <int KT>
__global__ __launch_bounds__(kThreads) void region_stats_kernel(const float* __restrict__ x,
                                                                const unsigned char* __restrict__ labels,
                                                                float* __restrict__ mean_out,
                                                                float* __restrict__ std_out, int* __restrict__ count_out,
                                                                int64_t hw, int c, int regions) {
  __shared__ float shf[kWaves][kMaxK];
  __shared__ int shi[kWaves][kMaxK];
  __shared__ float shm[kMaxK];
  const int64_t p = blockIdx.x;
  const int64_t n = p / c;
  const int ch = (int)(p % c);
  const float* xp = x + p * hw;
  const unsigned char* lab = labels + n * hw;
  int cnt[KT];
  float mean[KT], sd[KT];
  if ((hw & 3) == 0 && aligned16(xp) && ((uintptr_t)lab & 3) == 0)
    region_plane_stats<KT, true>(xp, lab, hw, shf, shi, shm, cnt, mean, sd);
  else
    region_plane_stats<KT, false>(xp, lab, hw, shf, shi, shm, cnt, mean, sd);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < regions) {
        const int64_t at = (n * regions + k) * c + ch;
        mean_out[at] = mean[k];
        std_out[at] = sd[k];
        if (ch == 0) count_out[n * regions + k] = cnt[k];
      }
    }
  }
}

// Nearest-neighbour resize of uint8 label maps: src = (dst * in) / out per axis, in integers.
__global__ __launch_bounds__(kThreads) void resize_labels_kernel(const unsigned char* __restrict__ src,
                                                                 unsigned char* __restrict__ dst, int64_t n, int hs,
                                                                 int ws, int hd, int wd) {
  const int64_t total = n * hd * wd;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int xd = (int)(i % wd);
    const int yd = (int)((i / wd) % hd);
    const int64_t img = i / ((int64_t)wd * hd);
    const int ys = (int)(((int64_t)yd * hs) / hd), xs = (int)(((int64_t)xd * ws) / wd);
    dst[i] = src[(img * hs + ys) * ws + xs];
  }
}

}  // namespace

extern "C" {

int ast_resize_labels_u8(const unsigned char* src, unsigned char* dst, long long n, int hs, int ws, int hd, int wd,
                         void* stream) {
  if (!src || !dst) return AST_E_NULLPTR;
  if (n <= 0 || hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0) return AST_E_SHAPE;
  const int64_t total = (int64_t)n * hd * wd;
  const int blocks = (int)((total + kThreads - 1) / kThreads < 8192 ? (total + kThreads - 1) / kThreads : 8192);
  hipLaunchKernelGGL(resize_labels_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, src, dst,
                     (int64_t)n, hs, ws, hd, wd);
  return (int)hipGetLastError();
}

int ast_region_stats_f32(const float* x, const unsigned char* labels, float* mean, float* std, int* count, int n,
                         int c, int h, int w, int regions, void* stream) {
  if (!x || !labels || !mean || !std || !count) return AST_E_NULLPTR;
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || regions < 1 || regions > AST_MAX_REGIONS) return AST_E_SHAPE;
  if ((int64_t)n * c > 0x7fffffffLL) return AST_E_SHAPE;
  const dim3 grid((unsigned)((int64_t)n * c));
  const int64_t hw = (int64_t)h * w;
  hipStream_t st = (hipStream_t)stream;
#define AST_RS(KT) \
  hipLaunchKernelGGL(region_stats_kernel<KT>, grid, dim3(kThreads), 0, st, x, labels, mean, std, count, hw, c, regions)
  if (regions == 1) AST_RS(1);
  else if (regions == 2) AST_RS(2);
  else if (regions <= 4) AST_RS(4);
  else AST_RS(8);
#undef AST_RS
  return (int)hipGetLastError();
}

int ast_adain_regions_f32(const float* content, const unsigned char* labels, const float* style_mean,
                          const float* style_std, const float* mix, float* out, int n, int c, int h, int w,
                          int regions, int rows, int mix_stride_n, double alpha, int swap_style_stats, void* stream) {
  if (!content || !labels || !style_mean || !style_std || !mix || !out) return AST_E_NULLPTR;
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return AST_E_SHAPE;
  if (regions < 1 || regions > AST_MAX_REGIONS || rows < 1 || rows > AST_MAX_STYLE_ROWS) return AST_E_SHAPE;
  if (mix_stride_n != 0 && mix_stride_n != regions * rows) return AST_E_SHAPE;
  if ((int64_t)n * c > 0x7fffffffLL) return AST_E_SHAPE;
  // torch: `alpha * t + (1 - alpha) * c` with Python-float scalars applied in fp32 (as ast_adain_f32)
  const float a = (float)alpha, b = (float)(1.0 - alpha);
  const dim3 grid((unsigned)((int64_t)n * c));
  const int64_t hw = (int64_t)h * w;
  const int swap = swap_style_stats ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
#define AST_AR(KT)                                                                                               \
  hipLaunchKernelGGL(adain_regions_kernel<KT>, grid, dim3(kThreads), 0, st, content, labels, style_mean, style_std, \
                     mix, out, hw, c, regions, rows, mix_stride_n, a, b, swap)
  if (regions == 1) AST_AR(1);
  else if (regions == 2) AST_AR(2);
  else if (regions <= 4) AST_AR(4);
  else AST_AR(8);
#undef AST_AR
  return (int)hipGetLastError();
}

}  // extern "C"
