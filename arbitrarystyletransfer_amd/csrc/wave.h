// The one place a full-wave or workgroup reduction is written. Device code only, no kernels.
// A wave reduction is the xor butterfly over all 64 lanes (offsets 32, 16, ..., 1). A workgroup
// reduction is that butterfly, then lane 0 of every wave stores to LDS, then every thread adds the
// waves' values in one of three orders, which differ in bits (0.f + -0.f is +0.f; (a + b) + (c + d)
// and ((a + b) + c) + d round differently):
//   A  t = 0.f; t += sh[0], sh[1], ...    block_sum<NW>: adain, adaattn, wct, mbtrain, hist; det.h's
//                                         block_sum_fixed is A with a runtime wave count
//   B  (sh[0] + sh[1]) + (sh[2] + sh[3])  block_sum_pairs: optim; losses.hip's block_sum
//   C  sh[0] + sh[1] + sh[2] + sh[3]      mobilenet.hip's block_sum256 only
// A kernel's order is part of its numerical contract (determinism): do not "unify" them.
//
// The block reductions write their butterfly out and do not call wave_sum / wave_max: a callee is
// optimised on its own before it is inlined, and the kernels then come out scheduled differently.
// For the same reason a butterfly written inline in a kernel (det.h, augment, hist's emd_kernel,
// kmeans, wgrad_co3, mbt_dw, mb_ed5, conv3x3_bwd) equals wave_sum in value but not in the code the
// compiler makes of it: replacing one changes that kernel's code object and is to be measured as such.
#pragma once
#include <hip/hip_runtime.h>

namespace ast_wave {
namespace {

// Reductions over the 64 lanes of a wave; every lane receives the result.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Reductions over a workgroup of NW waves (blockDim.x == 64 * NW); `sh` holds NW floats and every
// thread receives the result. No trailing barrier: the caller may not overwrite sh before its next
// barrier (a second block_* call on the same sh is fine, it starts with one).
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* sh) {  // order A
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) t += sh[i];
  return t;
}

template <int NW>
__device__ __forceinline__ float block_max(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = sh[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t = fmaxf(t, sh[i]);
  return t;
}

__device__ __forceinline__ float block_sum_pairs(float v, float* sh) {  // order B, four waves
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

}  // namespace
}  // namespace ast_wave
