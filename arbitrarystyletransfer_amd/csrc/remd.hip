// Relaxed earth mover's distance style loss (Kolkin et al., STROTSS, CVPR 2019; the matching of Neural
// Neighbor Style Transfer; a relative of the contextual loss, Mechrez et al. 2018) for gfx950, fp32
// storage, exact: every pixel of both maps takes part, nothing is sampled. The definition is in
// include/ast_hip.h; tests/remd_ref.py restates it. Inputs: x [n, C, M pixels], the differentiable
// side, and y [ns, C, P pixels] (ns = n, or 1 for a style shared by the batch), both dense NCHW with
// the spatial sides flattened; pixel i of x and pixel j of y are C-vectors.
//   u_i = 1 / ||x_i||, v_j = 1 / ||y_j||   (0 unless the squared norm is positive)
//   D(i, j) = 1 - (<x_i, y_j> u_i) v_j
//   r_i = min_j D(i, j), a_i its arg-min;  c_j = min_i D(i, j), b_j its arg-min: the lowest index on
//         equal values; a NaN never wins; a value replaces the running (+inf, 0) only when strictly less
//   L = weight / n * sum_b (row branch ? mean_i r_i : mean_j c_j), row branch when mean r >= mean c
// Three stages, each a C-ABI entry of its own; ast_remd_loss_f32 is exactly norms, norms, match, means:
//   inverse norms  one launch per side: four interleaved channel quarters per pixel, summed in quarter
//                  order, 1 / sqrt; the same order at every position, so equal vectors have equal
//                  norms in bits
//   match          an implicit GEMM, M = content pixels, N = style pixels, K = C, both operands read
//                  straight from NCHW (a chunk of 64 channels x 64 pixels is 64 contiguous runs). A
//                  workgroup owns 64 content pixels and streams 64-pixel style tiles; the next chunk's
//                  buffer loads (a descriptor per chunk: channels past C read as 0) are in flight while
//                  this one is multiplied. Products are v_mfma_f32_32x32x2_f32 (4 waves x 32x32, the
//                  tile of swap.hip); a distance is one fma chain over the channels in an order that
//                  does not depend on where either pixel sits. After a style tile every lane holds 16
//                  rows of one column: the rows fold into a running (min, index) pair per content pixel
//                  in registers, the column folds over the lane's rows, the other lane half and the
//                  other wave of the column, and goes out as this content tile's partial (min, index)
//                  for that style pixel. A merge launch reduces the partials in content-tile order
//                  (strictly less: the lowest index stays). Splits of the style tiles for small grids
//                  as in swap.hip, the row pairs of the splits merged in split order. The distances
//                  are never stored.
//   means          per sample the two means in a fixed order (wave.h), the branch chosen on the
//                  device; a one-workgroup launch sums the samples' values in sample order into a
//                  loss accumulator.
// Backward (to x only): the column branch needs, for each content pixel, the ascending list of the
// style pixels that chose it. One workgroup per sample builds it with integer work alone and no
// atomics: a count, a scan and a stable fill, all three walking the style pixels in chunks of 256 in
// ascending order; within a chunk a thread's rank among equal keys comes from comparing the chunk's
// keys in LDS. Then one gather launch per branch; a launch returns at once for a sample of the other
// branch, so every element of dx is written exactly once.
// No floating-point atomics, no host synchronisation, no allocation: every sample is indexed by a grid
// dimension, so a non-finite value stays inside its own sample.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "det.h"
#include "match_tile.h"
#include "wave.h"
#include "ws.h"

namespace {

using ast_tile::acc_row;
using ast_tile::f32x16;
using ast_tile::fold_arg;
using ast_tile::stage_load;
using ast_tile::stage_store;
using ast_wave::block_sum;

constexpr int kT = 256;   // threads per workgroup everywhere in this file
constexpr int MT = 64;    // pixels per tile side (4 waves x 32 x 32)
constexpr int KC = 64;    // channels per staged chunk
constexpr int RT = KC / 4;  // channel runs per wave and chunk
constexpr int kMaxC = AST_REMD_MAX_C;
constexpr int kMaxPixels = AST_REMD_MAX_PIXELS;  // 4 * KC * pixels stays below 2^31: the buffer offsets are int32
constexpr int kTargetWGs = 8 * 256;
constexpr int kMinSplitTiles = 4;  // a split of fewer style tiles does not amortise its content tile's loads
constexpr int GC = 32;    // channels per workgroup of the row gather
constexpr int GCC = 8;    // and of the column gather, whose threads walk lists of unequal length
constexpr int AST_ROW = 1, AST_COL = 2;

// ------------------------------------------------------------------------------------------------
// Inverse norms: grid (pixels / 64, samples); thread (p, g) sums channels g, g + 4, ... and the four
// partials are added in g order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void remd_invnorm_kernel(const float* __restrict__ x, float* __restrict__ inv, int C,
                                                         int hw) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, p = blockIdx.x * 64 + lane;
  const float* X = x + (int64_t)blockIdx.y * C * hw;
  float s = 0.f;
  if (p < hw) s = ast_tile::quarter_sqsum(X, C, hw, g, p);
  sh[g][lane] = s;
  __syncthreads();
  if (g == 0 && p < hw) {
    const float t = ast_tile::quarter_sum(sh, lane);
    const float q = 1.0f / sqrtf(t);
    inv[(int64_t)blockIdx.y * hw + p] = (t > 0.f && q > 0.f) ? q : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// Match
// ------------------------------------------------------------------------------------------------

// stage_load / stage_store (match_tile.h): a chunk of KC channels x 64 pixels into registers, then LDS.

// grid (content tiles, splits, samples). Row pairs of sample b and split s at [(b * splits + s) * M + i]:
// the outputs themselves when splits == 1. Column pairs of content tile t at [(b * tiles + t) * P + j];
// a style pixel is visited by exactly one split.
__global__ __launch_bounds__(kT) void remd_match_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ u, const float* __restrict__ v,
                                                       float* __restrict__ orow, int* __restrict__ oridx,
                                                       float* __restrict__ pcol, int* __restrict__ pcidx, int C, int M,
                                                       int P, int style_batch, int tiles_per_split) {
  __shared__ float As[KC * MT];
  __shared__ float Bs[KC * MT];
  __shared__ float colv[2][32];
  __shared__ int coli[2][32];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave & 1, wn = wave >> 1;
  const int b = blockIdx.z, bs = style_batch == 1 ? 0 : b, split = blockIdx.y;
  const int ptiles = (P + MT - 1) / MT, m0 = blockIdx.x * MT;
  const int jt_beg = split * tiles_per_split, jt_end = min(jt_beg + tiles_per_split, ptiles);
  const float* Ab = x + (int64_t)b * C * M;
  const float* Bb = y + (int64_t)bs * C * P;
  const float* ub = u + (int64_t)b * M;
  const float* vb = v + (int64_t)bs * P;
  const float* Ar = As + h * MT + wm * 32 + r;
  const float* Br = Bs + h * MT + wn * 32 + r;

  // the lane's 16 accumulator rows: content pixel m0 + wm * 32 + acc_row(i, h)
  float ur[16], best[16];
  int bidx[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int gi = m0 + wm * 32 + acc_row(i, h);
    ur[i] = gi < M ? ub[gi] : 0.f;
    best[i] = INFINITY;
    bidx[i] = 0;
  }

  float ra[RT], rb[RT];
  if (jt_beg < jt_end) {
    stage_load(ra, Ab, C, M, m0, wave, lane);
    stage_load(rb, Bb, C, P, jt_beg * MT, wave, lane);
  }
  // every branch that encloses a barrier depends on block indices and kernel arguments alone
  for (int jt = jt_beg; jt < jt_end; ++jt) {
    const int jl = jt * MT + wn * 32 + r;  // the lane's style pixel
    const bool jvalid = jl < P;
    f32x16 acc = (f32x16){0.f};
    for (int c0 = 0; c0 < C; c0 += KC) {
      stage_store(ra, As, wave, lane);
      stage_store(rb, Bs, wave, lane);
      __syncthreads();
      // the next chunk -- the next style tile's first one after this tile's last -- is in flight while
      // this one is multiplied; the workgroup's last step loads a chunk again that nobody uses
      const bool wrap = c0 + KC >= C;
      const int nc0 = wrap ? 0 : c0 + KC;
      const int nj0 = (wrap && jt + 1 < jt_end ? jt + 1 : jt) * MT;
      stage_load(ra, Ab + (int64_t)nc0 * M, C - nc0, M, m0, wave, lane);
      stage_load(rb, Bb + (int64_t)nc0 * P, C - nc0, P, nj0, wave, lane);
      __builtin_amdgcn_sched_barrier(0);  // the loads are issued here, ahead of the products
      // k order of every distance: ascending channel pairs; lane half h takes the pair's channel h
#pragma unroll
      for (int cp = 0; cp < KC / 2; ++cp)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ar[2 * cp * MT], Br[2 * cp * MT], acc, 0, 0, 0);
      __syncthreads();
    }
    const float vj = jvalid ? vb[jl] : 0.f;
    float cmin = INFINITY;
    int cix = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int gi = m0 + wm * 32 + acc_row(i, h);
      const float d = 1.0f - (acc[i] * ur[i]) * vj;
      if (jvalid && d < best[i]) {  // j grows from tile to tile: the lowest j of equal distances stays
        best[i] = d;
        bidx[i] = jl;
      }
      if (gi < M && d < cmin) {  // the lane's rows ascend with i
        cmin = d;
        cix = gi;
      }
    }
    // the column: the other lane half holds the rows in between, the wm = 1 wave the 32 rows after
    fold_arg<false>(cmin, cix, __shfl_xor(cmin, 32, 64), __shfl_xor(cix, 32, 64));
    if (wm == 1 && h == 0) {
      colv[wn][r] = cmin;
      coli[wn][r] = cix;
    }
    __syncthreads();  // the wm = 1 waves write colv again only after the next tile's chunk barriers
    if (wm == 0 && h == 0 && jvalid) {
      if (colv[wn][r] < cmin) {
        cmin = colv[wn][r];
        cix = coli[wn][r];
      }
      const int64_t o = ((int64_t)b * gridDim.x + blockIdx.x) * P + jl;
      pcol[o] = cmin;
      pcidx[o] = cix;
    }
  }

  // the 32 lanes of a half hold the same 16 rows over different columns; then the two waves of a row
  float* redv = As;  // [2 wm][32 rows] of the wn = 1 waves; As is free after the loop's last barrier
  int* redi = (int*)(As + 64);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float bv = best[i];
    int ix = bidx[i];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(ix, o, 64);
      fold_arg<false>(bv, ix, ov, oi);
    }
    best[i] = bv;
    bidx[i] = ix;
  }
  if (wn == 1 && r == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, h);
      redv[wm * 32 + row] = best[i];
      redi[wm * 32 + row] = bidx[i];
    }
  }
  __syncthreads();
  if (wn == 0 && r == 0) {
    const int64_t ob = ((int64_t)b * gridDim.y + split) * M;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, h), gi = m0 + wm * 32 + row;
      if (gi >= M) continue;
      float bv = best[i];
      int ix = bidx[i];
      fold_arg<false>(bv, ix, redv[wm * 32 + row], redi[wm * 32 + row]);
      orow[ob + gi] = bv;
      oridx[ob + gi] = ix;
    }
  }
}

// grid (elements / 256, samples): the `slots` partial pairs of an element, [(b * slots + s) * count + e],
// in slot order; a later slot holds higher indices only, so strictly less keeps the lowest index of
// equal values. Rows: the slots are the splits. Columns: the slots are the content tiles.
__global__ __launch_bounds__(kT) void remd_merge_kernel(const float* __restrict__ pmin, const int* __restrict__ pidx,
                                                       float* __restrict__ omin, int* __restrict__ oidx, int count,
                                                       int slots) {
  ast_tile::merge_slots<false, kT>(pmin, pidx, omin, oidx, count, slots, 0);
}

// ------------------------------------------------------------------------------------------------
// Means, branch, loss
// ------------------------------------------------------------------------------------------------

// grid (samples): thread t sums elements t, t + 256, ... in order, then order A of wave.h.
__global__ __launch_bounds__(kT) void remd_means_kernel(const float* __restrict__ rmin, const float* __restrict__ cmin,
                                                       float* __restrict__ rmean, float* __restrict__ cmean,
                                                       unsigned char* __restrict__ branch, int M, int P, int force) {
  __shared__ float sh[kT / 64];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int i = threadIdx.x; i < M; i += kT) s += rmin[(int64_t)b * M + i];
  const float rm = block_sum<kT / 64>(s, sh) / (float)M;
  s = 0.f;
  for (int j = threadIdx.x; j < P; j += kT) s += cmin[(int64_t)b * P + j];
  const float cm = block_sum<kT / 64>(s, sh) / (float)P;
  if (threadIdx.x == 0) {
    rmean[b] = rm;
    cmean[b] = cm;
    branch[b] = (unsigned char)(force ? force : (rm >= cm ? AST_ROW : AST_COL));
  }
}

// one workgroup: *loss += w_over_n * sum over the samples, in sample order per thread, of the mean of
// the sample's branch
__global__ __launch_bounds__(kT) void remd_total_kernel(const float* __restrict__ rmean, const float* __restrict__ cmean,
                                                       const unsigned char* __restrict__ branch, float* loss, int n,
                                                       float w_over_n) {
  __shared__ float sh[kT / 64];
  float s = 0.f;
  for (int b = threadIdx.x; b < n; b += kT) s += branch[b] == AST_ROW ? rmean[b] : cmean[b];
  const float t = block_sum<kT / 64>(s, sh);
  ast_det::loss_acc_commit(loss, w_over_n * t);
}

// ------------------------------------------------------------------------------------------------
// Backward
// ------------------------------------------------------------------------------------------------

// The rank of thread t's key among the equal keys of the chunk before it, and whether an equal key
// follows it. keys: 256 ints in LDS, visible.
__device__ __forceinline__ void chunk_rank(const int* keys, int t, int key, int& rank, bool& later) {
  rank = 0;
  later = false;
  const int4* k4 = reinterpret_cast<const int4*>(keys);
  for (int q = 0; q < kT / 4; ++q) {
    const int4 k = k4[q];
    const int t0 = 4 * q;
    rank += (k.x == key && t0 < t) + (k.y == key && t0 + 1 < t) + (k.z == key && t0 + 2 < t) + (k.w == key && t0 + 3 < t);
    later |= (k.x == key && t0 > t) || (k.y == key && t0 + 1 > t) || (k.z == key && t0 + 2 > t) ||
             (k.w == key && t0 + 3 > t);
  }
}

// grid (samples), for the samples of the column branch: start[b, i] .. start[b, i + 1] delimit, in
// list[b, .], the ascending style pixels j with cidx[b, j] == i (an index outside 0 .. M - 1 is clamped).
// start [n, M + 1], cursor [n, M], list [n, P]. Integer work only, no atomics: the style pixels are
// walked in chunks of 256 in ascending order, one thread per pixel; of the threads of a chunk with
// the same key the last one updates the key's counter, so no two threads touch one word between two
// barriers.
__global__ __launch_bounds__(kT) void remd_invert_kernel(const int* __restrict__ cidx,
                                                        const unsigned char* __restrict__ branch, int* start,
                                                        int* cursor, int* __restrict__ list, int M, int P) {
  __shared__ __attribute__((aligned(16))) int keys[kT];
  __shared__ int scan[kT];
  __shared__ int carry;
  const int b = blockIdx.x, t = threadIdx.x;
  if (branch[b] != AST_COL) return;
  const int* B = cidx + (int64_t)b * P;
  int* S = start + (int64_t)b * (M + 1);
  int* Cu = cursor + (int64_t)b * M;
  int* Ls = list + (int64_t)b * P;
  // count: S[i + 1] = the number of style pixels that chose i
  for (int i = t; i <= M; i += kT) S[i] = 0;
  __syncthreads();
  for (int j0 = 0; j0 < P; j0 += kT) {
    const int j = j0 + t;
    const int key = j < P ? min(max(B[j], 0), M - 1) : -1 - t;  // a key of its own past the map
    keys[t] = key;
    __syncthreads();
    int rank;
    bool later;
    chunk_rank(keys, t, key, rank, later);
    if (j < P && !later) S[key + 1] += rank + 1;
    __syncthreads();
  }
  // scan: S[i] = the number of style pixels that chose a pixel below i; cursor[i] = S[i]
  if (t == 0) carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < M; i0 += kT) {
    const int i = i0 + t;
    const int cnt = i < M ? S[i + 1] : 0;
    scan[t] = cnt;
    __syncthreads();
    for (int o = 1; o < kT; o <<= 1) {
      const int add = t >= o ? scan[t - o] : 0;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    const int incl = carry + scan[t];
    if (i < M) {
      S[i + 1] = incl;
      Cu[i] = incl - cnt;
    }
    __syncthreads();
    if (t == kT - 1) carry = incl;
    __syncthreads();
  }
  // stable fill
  for (int j0 = 0; j0 < P; j0 += kT) {
    const int j = j0 + t;
    const int key = j < P ? min(max(B[j], 0), M - 1) : -1 - t;
    keys[t] = key;
    __syncthreads();
    int rank;
    bool later;
    chunk_rank(keys, t, key, rank, later);
    int pos = 0;
    if (j < P) {
      pos = Cu[key] + rank;
      Ls[pos] = j;
    }
    __syncthreads();
    if (j < P && !later) Cu[key] = pos + 1;
    __syncthreads();
  }
}

// Row branch, grid (pixels / 256, channels / GC, samples):
//   dx_i = -(g w / (n M)) u_i (v_a y_a - (1 - r_i) (u_i x_i)),  a = ridx[i] (clamped into the map)
__global__ __launch_bounds__(kT) void remd_bwd_row_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ u, const float* __restrict__ v,
                                                         const float* __restrict__ rmin, const int* __restrict__ ridx,
                                                         const unsigned char* __restrict__ branch,
                                                         const float* __restrict__ g, float* __restrict__ dx, int C,
                                                         int M, int P, int style_batch, float w_over_nm) {
  const int i = blockIdx.x * kT + threadIdx.x, b = blockIdx.z, bs = style_batch == 1 ? 0 : b;
  if (branch[b] != AST_ROW || i >= M) return;
  const float ui = u[(int64_t)b * M + i];
  const int a = min(max(ridx[(int64_t)b * M + i], 0), P - 1);
  const float va = v[(int64_t)bs * P + a], s = 1.0f - rmin[(int64_t)b * M + i];
  const float k = -(g[0] * w_over_nm) * ui;
  const int c_beg = blockIdx.y * GC, c_end = min(c_beg + GC, C);
  const float* X = x + (int64_t)b * C * M + i;
  const float* Y = y + (int64_t)bs * C * P + a;
  float* D = dx + (int64_t)b * C * M + i;
  for (int c = c_beg; c < c_end; ++c) {
    const float t = va * Y[(int64_t)c * P] - s * (ui * X[(int64_t)c * M]);
    D[(int64_t)c * M] = ui == 0.f ? 0.f : k * t;
  }
}

// Column branch, grid (pixels / 256, channels / GCC, samples):
//   dx_i = -(g w / (n P)) u_i sum over the j of i's list, ascending, of (v_j y_j - (1 - c_j) (u_i x_i))
__global__ __launch_bounds__(kT) void remd_bwd_col_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ u, const float* __restrict__ v,
                                                         const float* __restrict__ cmin, const int* __restrict__ start,
                                                         const int* __restrict__ list,
                                                         const unsigned char* __restrict__ branch,
                                                         const float* __restrict__ g, float* __restrict__ dx, int C,
                                                         int M, int P, int style_batch, float w_over_np) {
  const int i = blockIdx.x * kT + threadIdx.x, b = blockIdx.z, bs = style_batch == 1 ? 0 : b;
  if (branch[b] != AST_COL || i >= M) return;
  const float ui = u[(int64_t)b * M + i];
  const int beg = start[(int64_t)b * (M + 1) + i], end = start[(int64_t)b * (M + 1) + i + 1];
  const float k = -(g[0] * w_over_np) * ui;
  const int c_beg = blockIdx.y * GCC, c_end = min(c_beg + GCC, C);
  const float* X = x + (int64_t)b * C * M + i;
  const float* Y = y + (int64_t)bs * C * P;
  const float* V = v + (int64_t)bs * P;
  const float* Cm = cmin + (int64_t)b * P;
  const int* Ls = list + (int64_t)b * P;
  float* D = dx + (int64_t)b * C * M + i;
  for (int c = c_beg; c < c_end; ++c) {
    const float xh = ui * X[(int64_t)c * M];
    const float* Yc = Y + (int64_t)c * P;
    float s = 0.f;
    for (int q = beg; q < end; ++q) {
      const int j = Ls[q];
      s += V[j] * Yc[j] - (1.0f - Cm[j]) * xh;
    }
    D[(int64_t)c * M] = (ui == 0.f || beg == end) ? 0.f : k * s;
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layouts, launch sequences
// ------------------------------------------------------------------------------------------------

using ast_tile::tiles_of;

inline int map_shape(int n, int pixels) { return ast_tile::map_shape(n, pixels, kMaxPixels); }

inline int pair_shape(int n, int ns, int m, int p) {
  if (n <= 0 || ns <= 0 || (ns != n && ns != 1)) return AST_E_SHAPE;
  const int e = map_shape(n, m);
  return e ? e : map_shape(ns, p);
}

inline int chan_shape(int c) { return ast_tile::chan_shape(c, kMaxC); }

// The match's workspace: [column partial minima | column partial indices | row partial minima | row
// partial indices], the column partials per content tile, the row partials per split and only when
// there is more than one. Splits of the style tiles (ast_tile::split_tiles): as asked, or, for 0, as
// many as bring the grid to about 8 workgroups per CU while a split keeps at least 4 tiles (measured at
// C = 512, n = 16: 2 splits at 64 x 64, 4 at 32 x 32).
struct MatchWs {
  int splits, tiles_per_split;
  float* pcol;
  int* pcidx;
  float* prow;  // null for one split: the rows go straight to the outputs
  int* pridx;
  int64_t bytes;
};

inline MatchWs match_ws(void* base, int n, int m, int p, int want) {
  ast_ws::Walk wk(base);
  int tps = 0;
  const int s = ast_tile::split_tiles((int64_t)n * tiles_of(m), tiles_of(p), want, kTargetWGs, kMinSplitTiles, &tps);
  const int64_t col = (int64_t)4 * n * tiles_of(m) * p, row = (int64_t)4 * n * s * m;
  return {s, tps, wk.take<float>(col), wk.take<int>(col), s > 1 ? wk.take<float>(row) : nullptr,
          s > 1 ? wk.take<int>(row) : nullptr, wk.off};
}

// The backward's workspace: [start | cursor | list]
struct BwdWs {
  int *start, *cursor, *list;
  int64_t bytes;
};

inline BwdWs bwd_ws(void* base, int n, int m, int p) {
  ast_ws::Walk wk(base);
  return {wk.take<int>((int64_t)4 * n * (m + 1)), wk.take<int>((int64_t)4 * n * m), wk.take<int>((int64_t)4 * n * p),
          wk.off};
}

int norms_launch(const float* x, float* inv, int n, int c, int hw, hipStream_t st) {
  hipLaunchKernelGGL(remd_invnorm_kernel, dim3((hw + 63) / 64, n), dim3(kT), 0, st, x, inv, c, hw);
  return (int)hipGetLastError();
}

int match_launch(const float* x, const float* y, const float* u, const float* v, float* rmin, int* ridx, float* cmin,
                 int* cidx, int n, int ns, int c, int m, int p, int want, void* wsp, hipStream_t st) {
  const MatchWs w = match_ws(wsp, n, m, p, want);
  const int splits = w.splits, tps = w.tiles_per_split, ct = tiles_of(m);
  float* pc = w.pcol;
  int* pci = w.pcidx;
  float* pr = splits > 1 ? w.prow : rmin;
  int* pri = splits > 1 ? w.pridx : ridx;
  hipLaunchKernelGGL(remd_match_kernel, dim3(ct, splits, n), dim3(kT), 0, st, x, y, u, v, pr, pri, pc, pci, c, m, p, ns,
                     tps);
  if (splits > 1)
    hipLaunchKernelGGL(remd_merge_kernel, dim3((m + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)pr, (const int*)pri,
                       rmin, ridx, m, splits);
  hipLaunchKernelGGL(remd_merge_kernel, dim3((p + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)pc, (const int*)pci,
                     cmin, cidx, p, ct);
  return (int)hipGetLastError();
}

int means_launch(const float* rmin, const float* cmin, float* rmean, float* cmean, unsigned char* branch, float* loss,
                 int n, int m, int p, float weight, int force, hipStream_t st) {
  hipLaunchKernelGGL(remd_means_kernel, dim3(n), dim3(kT), 0, st, rmin, cmin, rmean, cmean, branch, m, p, force);
  hipLaunchKernelGGL(remd_total_kernel, dim3(1), dim3(kT), 0, st, (const float*)rmean, (const float*)cmean,
                     (const unsigned char*)branch, loss, n, weight / (float)n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ast_cosine_norms_f32(const float* x, float* inv_norm, int n, int c, int pixels, void* stream) {
  if (!x || !inv_norm) return AST_E_NULLPTR;
  int e = map_shape(n, pixels);
  if (!e) e = chan_shape(c);
  if (e) return e;
  return norms_launch(x, inv_norm, n, c, pixels, (hipStream_t)stream);
}

long long ast_cosine_match_workspace_bytes(int n, int ns, int m, int p, int splits) {
  const int e = pair_shape(n, ns, m, p);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  return match_ws(nullptr, n, m, p, splits).bytes;
}

int ast_cosine_match_f32(const float* x, const float* y, const float* inv_x, const float* inv_y, float* row_min,
                         int* row_index, float* col_min, int* col_index, int n, int ns, int c, int m, int p, int splits,
                         void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !y || !inv_x || !inv_y || !row_min || !row_index || !col_min || !col_index || !workspace)
    return AST_E_NULLPTR;
  int e = pair_shape(n, ns, m, p);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  if (workspace_bytes < match_ws(nullptr, n, m, p, splits).bytes) return AST_E_SHAPE;
  return match_launch(x, y, inv_x, inv_y, row_min, row_index, col_min, col_index, n, ns, c, m, p, splits, workspace,
                      (hipStream_t)stream);
}

int ast_remd_means_f32(const float* row_min, const float* col_min, float* row_mean, float* col_mean,
                       unsigned char* branch, float* loss, int n, int m, int p, float weight, int force_branch,
                       void* stream) {
  if (!row_min || !col_min || !row_mean || !col_mean || !branch || !loss) return AST_E_NULLPTR;
  const int e = pair_shape(n, n, m, p);
  if (e) return e;
  if (force_branch < 0 || force_branch > 2) return AST_E_UNSUPPORTED;
  return means_launch(row_min, col_min, row_mean, col_mean, branch, loss, n, m, p, weight, force_branch,
                      (hipStream_t)stream);
}

long long ast_remd_loss_workspace_bytes(int n, int ns, int m, int p) {
  const int e = pair_shape(n, ns, m, p);
  return e ? e : match_ws(nullptr, n, m, p, 0).bytes;
}

int ast_remd_loss_f32(const float* x, const float* y, float* inv_x, float* inv_y, float* row_min, int* row_index,
                      float* col_min, int* col_index, float* row_mean, float* col_mean, unsigned char* branch,
                      float* loss, int n, int ns, int c, int m, int p, float weight, int force_branch, void* workspace,
                      long long workspace_bytes, void* stream) {
  if (!x || !y || !inv_x || !inv_y || !row_min || !row_index || !col_min || !col_index || !row_mean || !col_mean ||
      !branch || !loss || !workspace)
    return AST_E_NULLPTR;
  int e = pair_shape(n, ns, m, p);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (force_branch < 0 || force_branch > 2) return AST_E_UNSUPPORTED;
  if (workspace_bytes < match_ws(nullptr, n, m, p, 0).bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  e = norms_launch(x, inv_x, n, c, m, st);
  if (e) return e;
  e = norms_launch(y, inv_y, ns, c, p, st);
  if (e) return e;
  e = match_launch(x, y, inv_x, inv_y, row_min, row_index, col_min, col_index, n, ns, c, m, p, 0, workspace, st);
  if (e) return e;
  return means_launch(row_min, col_min, row_mean, col_mean, branch, loss, n, m, p, weight, force_branch, st);
}

long long ast_remd_loss_backward_workspace_bytes(int n, int m, int p) {
  const int e = pair_shape(n, n, m, p);
  return e ? e : bwd_ws(nullptr, n, m, p).bytes;
}

int ast_remd_loss_backward_f32(const float* x, const float* y, const float* inv_x, const float* inv_y,
                               const float* row_min, const int* row_index, const float* col_min, const int* col_index,
                               const unsigned char* branch, const float* grad_scale, float* dx, int n, int ns, int c,
                               int m, int p, float weight, void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !y || !inv_x || !inv_y || !row_min || !row_index || !col_min || !col_index || !branch || !grad_scale ||
      !dx || !workspace)
    return AST_E_NULLPTR;
  int e = pair_shape(n, ns, m, p);
  if (!e) e = chan_shape(c);
  if (e) return e;
  const BwdWs w = bwd_ws(workspace, n, m, p);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(remd_invert_kernel, dim3(n), dim3(kT), 0, st, col_index, branch, w.start, w.cursor, w.list, m, p);
  const dim3 grid((m + kT - 1) / kT, (c + GC - 1) / GC, n);
  hipLaunchKernelGGL(remd_bwd_row_kernel, grid, dim3(kT), 0, st, x, y, inv_x, inv_y, row_min, row_index, branch,
                     grad_scale, dx, c, m, p, ns, weight / ((float)n * (float)m));
  const dim3 cgrid((m + kT - 1) / kT, (c + GCC - 1) / GCC, n);
  hipLaunchKernelGGL(remd_bwd_col_kernel, cgrid, dim3(kT), 0, st, x, y, inv_x, inv_y, col_min, (const int*)w.start,
                     (const int*)w.list, branch, grad_scale, dx, c, m, p, ns, weight / ((float)n * (float)p));
  return (int)hipGetLastError();
}

}  // extern "C"
