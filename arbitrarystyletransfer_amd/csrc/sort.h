// The LDS bitonic sort that the EFDM kernels share (efdm.hip, efdm_regions.hip). Device code only, no
// kernels.
// Floats are ordered by IEEE-754 totalOrder of their bits: key = bits ^ (sign ? 0xffffffff : 0x80000000),
// an unsigned compare, so -0 < +0, negative NaNs first, positive NaNs last, equal keys = equal bits.
// lds_sort is a bitonic network over a power-of-two length P >= 512, keys as 32-bit words and (IDX)
// indices as 16-bit words in two arrays; the pairs (key, index) are unique per element, so the
// (unstable) network gives the stable result. Padding has key 0xffffffff and an index past the real
// ones, so it sorts after every real element (a real all-ones NaN included). A wave owns tiles of 512
// consecutive elements, 8 per lane in registers: every stage of stride < 512 runs there -- strides
// 8..256 across lanes (lane ^ 1..8 as DPP moves, lane ^ 16 and 32 through ds_bpermute), strides 4, 2, 1
// inside the lane -- without a barrier, so the first 45 stages (k = 2..512) are one register pass.
// Strides >= 512 are compare-exchanges in LDS, every lane on one pair per step, a barrier per stage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ast_sort {
namespace {

constexpr int kE = 8;                // elements per lane in a register pass
constexpr int kTile = 64 * kE;       // elements per wave tile
constexpr int kMaxThreads = 1024;
constexpr uint32_t kPadKey = 0xffffffffu;

__device__ __forceinline__ uint32_t to_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}

__device__ __forceinline__ float from_key(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

template <bool IDX>
__device__ __forceinline__ bool gt(uint32_t ka, uint32_t ia, uint32_t kb, uint32_t ib) {
  if (IDX) return (((uint64_t)ka << 32) | ia) > (((uint64_t)kb << 32) | ib);   // one 64-bit compare
  return ka > kb;
}

// stride J < kE inside the lane, for the merge step k of the network
template <bool IDX, int J>
__device__ __forceinline__ void ce_lane(uint32_t (&kk)[kE], uint32_t (&ii)[kE], int base, int k) {
#pragma unroll
  for (int q = 0; q < kE; ++q) {
    if (q & J) continue;
    const bool up = ((base + q) & k) == 0;
    if (gt<IDX>(kk[q], ii[q], kk[q | J], ii[q | J]) == up) {
      const uint32_t tk = kk[q], ti = ii[q];
      kk[q] = kk[q | J], ii[q] = ii[q | J];
      kk[q | J] = tk, ii[q | J] = ti;
    }
  }
}

// v of lane ^ M. Masks 1..8 are DPP moves on the VALU (quad permutes; xor 4 = half-row mirror, i.e.
// xor 7, after xor 3; xor 8 = row mirror, i.e. xor 15, after xor 7), which leaves the LDS crossbar
// to masks 16 and 32.
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
  constexpr int kQuad1032 = 0xB1, kQuad2301 = 0x4E, kQuad3210 = 0x1B, kRowMirror = 0x140, kRowHalfMirror = 0x141;
  if (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, kQuad1032, 0xf, 0xf, true);
  if (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, kQuad2301, 0xf, 0xf, true);
  if (M == 4)
    return (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)v, kQuad3210, 0xf, 0xf, true),
                                              kRowHalfMirror, 0xf, 0xf, true);
  if (M == 8)
    return (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)v, kRowHalfMirror, 0xf, 0xf, true),
                                              kRowMirror, 0xf, 0xf, true);
  return __shfl_xor(v, M, 64);
}

// stride M * kE across lanes (partner lane = lane ^ M, same register), for the merge step k
template <bool IDX, int M>
__device__ __forceinline__ void ce_lanes(uint32_t (&kk)[kE], uint32_t (&ii)[kE], int lane, int base, int k) {
  const bool want_min = ((lane & M) == 0) == ((base & k) == 0);   // k > stride >= kE: q does not reach bit k
#pragma unroll
  for (int q = 0; q < kE; ++q) {
    const uint32_t ok = lane_xor<M>(kk[q]);
    uint32_t oi = 0u;
    if (IDX) oi = lane_xor<M>(ii[q]);
    const bool take = gt<IDX>(kk[q], ii[q], ok, oi) == want_min;
    kk[q] = take ? ok : kk[q];
    if (IDX) ii[q] = take ? oi : ii[q];
  }
}

// Every stage of stride < kTile of the merge steps k_lo..k_hi, on the tiles of this wave, in
// registers. key (and idx) hold P elements, P a multiple of kTile; the caller puts barriers around.
template <bool IDX>
__device__ __forceinline__ void reg_pass(uint32_t* key, uint16_t* idx, int P, int k_lo, int k_hi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  for (int tile = wave; tile < P / kTile; tile += waves) {
    const int base = tile * kTile + lane * kE;
    uint32_t kk[kE], ii[kE];
    {
      const uint4 a = *reinterpret_cast<const uint4*>(key + base);
      const uint4 b = *reinterpret_cast<const uint4*>(key + base + 4);
      kk[0] = a.x, kk[1] = a.y, kk[2] = a.z, kk[3] = a.w, kk[4] = b.x, kk[5] = b.y, kk[6] = b.z, kk[7] = b.w;
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      if (IDX) c = *reinterpret_cast<const uint4*>(idx + base);
      ii[0] = c.x & 0xffffu, ii[1] = c.x >> 16, ii[2] = c.y & 0xffffu, ii[3] = c.y >> 16;
      ii[4] = c.z & 0xffffu, ii[5] = c.z >> 16, ii[6] = c.w & 0xffffu, ii[7] = c.w >> 16;
    }
    for (int k = k_lo; k <= k_hi; k <<= 1) {
      const int j0 = (k >> 1) < (kTile >> 1) ? (k >> 1) : (kTile >> 1);
      if (j0 >= 32 * kE) ce_lanes<IDX, 32>(kk, ii, lane, base, k);
      if (j0 >= 16 * kE) ce_lanes<IDX, 16>(kk, ii, lane, base, k);
      if (j0 >= 8 * kE) ce_lanes<IDX, 8>(kk, ii, lane, base, k);
      if (j0 >= 4 * kE) ce_lanes<IDX, 4>(kk, ii, lane, base, k);
      if (j0 >= 2 * kE) ce_lanes<IDX, 2>(kk, ii, lane, base, k);
      if (j0 >= kE) ce_lanes<IDX, 1>(kk, ii, lane, base, k);
      if (k >= 8) ce_lane<IDX, 4>(kk, ii, base, k);
      if (k >= 4) ce_lane<IDX, 2>(kk, ii, base, k);
      ce_lane<IDX, 1>(kk, ii, base, k);
    }
    *reinterpret_cast<uint4*>(key + base) = make_uint4(kk[0], kk[1], kk[2], kk[3]);
    *reinterpret_cast<uint4*>(key + base + 4) = make_uint4(kk[4], kk[5], kk[6], kk[7]);
    if (IDX)
      *reinterpret_cast<uint4*>(idx + base) = make_uint4(ii[0] | (ii[1] << 16), ii[2] | (ii[3] << 16),
                                                         ii[4] | (ii[5] << 16), ii[6] | (ii[7] << 16));
  }
}

// Ascending sort of key[0..P) (IDX: of the pairs (key, idx)) in LDS; P a power of two >= kTile,
// blockDim.x a multiple of 64. The data is in place and visible (a barrier passed) on entry and on return.
template <bool IDX>
__device__ __forceinline__ void lds_sort(uint32_t* key, uint16_t* idx, int P) {
  reg_pass<IDX>(key, idx, P, 2, kTile);
  __syncthreads();
  for (int k = 2 * kTile; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= kTile; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;   // i has bit j clear: every lane owns one pair
        const bool up = (i & k) == 0;
        const uint32_t ka = key[i], kb = key[l];
        uint32_t ia = 0u, ib = 0u;
        if (IDX) ia = idx[i], ib = idx[l];
        if (gt<IDX>(ka, ia, kb, ib) == up) {
          key[i] = kb, key[l] = ka;
          if (IDX) idx[i] = (uint16_t)ib, idx[l] = (uint16_t)ia;
        }
      }
      __syncthreads();
    }
    reg_pass<IDX>(key, idx, P, k, k);
    __syncthreads();
  }
}

// keys of x[0..m) and padding up to P into LDS, local indices 0..P-1
template <bool IDX>
__device__ __forceinline__ void lds_fill(const float* __restrict__ x, int m, uint32_t* key, uint16_t* idx, int P) {
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    key[i] = i < m ? to_key(x[i]) : kPadKey;
    if (IDX) idx[i] = (uint16_t)i;
  }
  __syncthreads();
}

}  // namespace
}  // namespace ast_sort
