// The fp32 MFMA match tile that swap.hip, remd.hip and selfsim.hip share: 64 x 64 outputs per
// workgroup, four waves of one v_mfma_f32_32x32x2_f32 block each (wave = 2 wn + wm, the block's rows at
// wm * 32, its columns at wn * 32), a lane holding 16 rows of one column. Device helpers, no kernels,
// then the host helpers of the same ops. As for wave.h, a helper is used only where the device assembly
// of the file that takes it stays what it was; what is not listed keeps its own code.
//   f32x16                     swap, remd, selfsim, wct
//   acc_row                    swap, remd, selfsim
//   stage_load / stage_store   remd, selfsim (pixel chunks of 4 RT channels; swap stages patch rows
//                              by a Plan of its own and keeps that)
//   fold_arg                   swap (MAX), remd (min), kmeans (MAX)
//   quarter_sum                swap, remd, selfsim, kmeans
//   quarter_sqsum              swap_sqnorm_kernel, remd_invnorm_kernel (the `p < hw` test stays in the kernel:
//                              inside the helper it changes remd_invnorm_kernel's compares)
//   merge_slots                swap_merge_kernel (MAX), remd_merge_kernel (min)
// Sites that keep their own code, because taking the helper changes their assembly
// (profiles/ws_match_tile_asm.txt has the first differing lines):
//   wct.hip, the accumulator rows `... * 32 + (i & 3) + 8 * (i >> 2) + 4 * h` of its cov, gemm and
//     apply kernels: with acc_row(i, h), or with a helper that adds the base first, some 2500 lines
//     of its assembly differ from wct_cov_kernel on (registers renumbered, code rescheduled).
//   The row arg-reduction that ends swap_match_kernel and remd_match_kernel (butterfly over the 32
//     lanes of a half, LDS exchange between the two waves of a row, store): as one
//     template <bool MAX> function remd's registers are renumbered and swap's code grows by some
//     320 lines. Both stay inline in their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"

namespace ast_tile {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the lane's accumulator row k of a 32 x 32 MFMA block: rows 4 h .. 4 h + 3, then every 8
__device__ __forceinline__ int acc_row(int k, int h) { return (k & 3) + 8 * (k >> 2) + 4 * h; }

// The chunk of KC = 4 RT channels whose first channel plane is `chunk` (`cleft` >= 1 channels are left
// from there) into registers: wave w takes channels w, w + 4, ... of the chunk, lane l pixel p0 + l.
// Buffer loads whose descriptor ends with the chunk's last real channel: a channel past C reads as 0
// (the hardware's range check), and so does anything past the sample. A pixel past the map reads the
// next channel's first pixels; such a row or column of the tile is never folded.
template <int RT>
__device__ __forceinline__ void stage_load(float (&reg)[RT], const float* chunk, int cleft, int hw, int p0, int wave,
                                           int lane) {
  constexpr int KC = 4 * RT;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(chunk), 0, 4 * min(cleft, KC) * hw, 0x00020000);
#pragma unroll
  for (int t = 0; t < RT; ++t)
    reg[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, 4 * ((wave + 4 * t) * hw + p0 + lane), 0, 0));
}

// and into the LDS image S [KC channels][64 pixels]
template <int RT>
__device__ __forceinline__ void stage_store(const float (&reg)[RT], float* S, int wave, int lane) {
#pragma unroll
  for (int t = 0; t < RT; ++t) S[(wave + 4 * t) * 64 + lane] = reg[t];
}

// (ov, oi) wins over the running pair: better (greater for MAX, else less), or equal with the lower index
template <bool MAX>
__device__ __forceinline__ void fold_arg(float& v, int& ix, float ov, int oi) {
  if ((MAX ? ov > v : ov < v) || (ov == v && oi < ix)) {
    v = ov;
    ix = oi;
  }
}

// the four channel quarters of a pixel, added in quarter order
__device__ __forceinline__ float quarter_sum(const float (&sh)[4][64], int lane) {
  return ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// quarter g of pixel p's squared norm: channels g, g + 4, ... of X [C, hw] in order (p < hw)
__device__ __forceinline__ float quarter_sqsum(const float* X, int C, int hw, int g, int p) {
  float s = 0.f;
  for (int c = g; c < C; c += 4) {
    const float v = X[(int64_t)c * hw + p];
    s = fmaf(v, v, s);
  }
  return s;
}

// The body of a merge kernel of T threads, grid (elements / T, samples): the `slots` partial pairs of an
// element, [(b * slots + s) * count + e], in slot order. A later slot holds higher indices only, so
// strictly better keeps the lowest index of equal values; `none` is the index of an element for which
// no slot has a winner.
template <bool MAX, int T>
__device__ __forceinline__ void merge_slots(const float* __restrict__ pval, const int* __restrict__ pidx,
                                            float* __restrict__ oval, int* __restrict__ oidx, int count, int slots,
                                            int none) {
  const int e = blockIdx.x * T + threadIdx.x, b = blockIdx.y;
  if (e >= count) return;
  float v = MAX ? -INFINITY : INFINITY;
  int ix = none;
  for (int s = 0; s < slots; ++s) {
    const int64_t o = ((int64_t)b * slots + s) * count + e;
    const float ov = pval[o];
    if (MAX ? ov > v : ov < v) {
      v = ov;
      ix = pidx[o];
    }
  }
  oval[(int64_t)b * count + e] = v;
  oidx[(int64_t)b * count + e] = ix;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------

// 64-wide tiles over p pixels, patches or channels
inline int tiles_of(int64_t p) { return (int)((p + 63) / 64); }

// AST_OK, or the code that rejects a channel count
inline int chan_shape(int c, int max_c) { return c <= 0 ? AST_E_SHAPE : c > max_c ? AST_E_UNSUPPORTED : AST_OK; }

// AST_OK, or the code that rejects n maps of `pixels` flattened pixels (a sample is a grid index)
inline int map_shape(int n, int pixels, int max_pixels) {
  return (n <= 0 || n > 65535 || pixels <= 0 || pixels > max_pixels) ? AST_E_SHAPE : AST_OK;
}

// Splits of the `ntiles` tiles that a workgroup streams, for a grid of `wgs` workgroups per split: as
// asked (`want` > 0, clamped to the tiles and to 64), or, for 0, as many as bring the grid to
// `target_wgs` workgroups while a split keeps at least `min_tiles_per_split` tiles; then rounded so
// that no split is empty. Returns the splits; their length goes to *tiles_per_split.
inline int split_tiles(int64_t wgs, int ntiles, int want, int target_wgs, int min_tiles_per_split,
                       int* tiles_per_split) {
  constexpr int kMaxSplits = 64;
  int64_t s = want > 0 ? want : (target_wgs + wgs - 1) / wgs;
  if (want <= 0 && s > ntiles / min_tiles_per_split) s = ntiles / min_tiles_per_split;
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > ntiles) s = ntiles;
  if (s < 1) s = 1;
  const int tps = (int)((ntiles + s - 1) / s);
  if (tiles_per_split) *tiles_per_split = tps;
  return (ntiles + tps - 1) / tps;
}

}  // namespace ast_tile
