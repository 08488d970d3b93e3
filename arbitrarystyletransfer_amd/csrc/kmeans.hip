// Feature k-means for the regional transforms (the clustering stage of Multimodal Style Transfer,
// Zhang et al. ICCV 2019) for gfx950, fp32 storage, and a 3x3 mode filter for the label maps it makes.
// The definition is in include/ast_hip.h; tests/kmeans_ref.py restates it. A bank x [B, C, H, W] is
// B HW points, point g = b HW + p the C-vector at pixel p of map b; centroids c [K, C], K <= 8;
//   d(g, k)  = sum over ch of (x - c)^2, one fp32 chain per (thread, k) over the thread's channels and
//              the partial chains of a point added in a fixed order
//   label(g) = the k of least d; the lowest k on equal d; a candidate replaces the running (+inf, 255)
//              only when strictly smaller, so a NaN never wins and a point without a winner gets 255
//   update   = c_k <- (sum of the points labelled k) / count_k; an empty cluster keeps its centroid
//   seeds    = maximin: the point farthest from the mean, then repeatedly the point farthest from the
//              seeds so far (ties to the lowest g)
// One tile kernel does all the per-point work, in four modes. A workgroup (256 threads) takes tiles of
// TP consecutive pixels of one map (a tile never straddles two maps), tile t, t + grid, ...:
//   stage    thread (pixel p = tid % TP, channel group tid / TP) walks its channels: a coalesced load of
//            x (TP * 4 bytes per channel row), a store into the LDS image of the tile, and NK
//            sub-and-fma against the centroids held in LDS (read as a broadcast)
//   label    the 256 / TP partial distances of a point meet in LDS and are added in group order by one
//            thread per pixel, which picks the label and stores it (LDS and, as a byte, global)
//   add      thread = channel now: it walks the tile's pixels in the LDS image (row stride TP + 1, so
//            neither phase has a bank conflict) and adds each value to the register accumulator of the
//            pixel's label, a workgroup-uniform branch; the accumulators live across the workgroup's
//            tiles and go out once, as its partial sums [workgroup][K][C] and counts [workgroup][K]
// so an iteration reads the bank from memory once. A second, small kernel adds the workgroups' partials
// in a fixed order (four runs of workgroups per channel, then the four), divides and writes the
// centroids. No floating-point atomics, no host synchronisation, no allocation, no cooperative launch:
// Lloyd's iterations are a fixed number of launches on the stream.
// The modes: ASSIGN (stage without the image, label), UPDATE (stage without distances, labels read
// from memory, add), FUSED (all three), DIST (one centroid -- the mean, or a point named by an index in
// device memory --: the running least distance per point and the workgroup's farthest point). UPDATE
// and FUSED run the same add code on the same tiles, so ast_kmeans_f32 equals its stages in bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "match_tile.h"
#include "ws.h"

namespace {

using ast_tile::fold_arg;

constexpr int kT = 256;            // threads per workgroup everywhere in this file
constexpr int kMaxK = AST_KMEANS_MAX_K;
constexpr int kMaxC = AST_KMEANS_MAX_C;
constexpr int kMaxPoints = AST_KMEANS_MAX_POINTS;
constexpr int kMaxWGs = 512;       // workgroups of the tile kernel: two per CU, and the bound of the partials
constexpr int kMaxWideWGs = 4096;  // ASSIGN and DIST leave no partial sums behind: a grid bounded for their few words per workgroup
constexpr int kCPT = kMaxC / kT;   // channels per thread of the add phase
constexpr int kLdsMax = 160 * 1024;

enum Mode { ASSIGN = 0, UPDATE = 1, FUSED = 2, DIST = 3 };

struct TileArgs {
  const float* x;          // [B, C, hw]
  const float* cen;        // [K, C]; DIST: the one centroid when seed is null
  const int* seed;         // DIST: the centroid is the point *seed (clamped into the bank)
  const uint8_t* lin;      // UPDATE: labels [B, hw], null for "all 0"
  uint8_t* lout;           // ASSIGN, FUSED: labels [B, hw]
  float* part;             // UPDATE, FUSED: [grid, K, C]
  int* pcnt;               // [grid, K]; ASSIGN: null for none
  float* dmin;             // DIST: [B hw], overwritten when first, else lowered
  float* pval;             // DIST: [grid] the workgroup's largest dmin
  int* pidx;               //       and its point
  int C, hw, K, tiles_per_map, ntiles, npoints, first;
};

__host__ __device__ constexpr bool scores(int mode) { return mode != UPDATE; }
__host__ __device__ constexpr bool adds(int mode) { return mode == UPDATE || mode == FUSED; }

// floats of dynamic LDS: [centroids C x NK | tile image C x (TP + 1) | partial distances (256 / TP) x NK x TP | labels TP]
__host__ __device__ constexpr int64_t lds_floats(int mode, int tp, int nk, int c) {
  return (scores(mode) ? (int64_t)nk * c + (int64_t)kT * nk : 0) + (adds(mode) ? (int64_t)c * (tp + 1) : 0) + tp;
}

extern __shared__ __attribute__((aligned(16))) float km_smem[];

template <int TP, int NK, int MODE>
__global__ __launch_bounds__(kT) void kmeans_tile_kernel(const TileArgs a) {
  constexpr int GRP = kT / TP;            // channel groups of the stage phase
  constexpr int TS = TP + 1;              // row stride of the tile image
  constexpr bool SCORE = scores(MODE), ADD = adds(MODE);
  const int tid = threadIdx.x, p = tid % TP, grp = tid / TP;
  const int C = a.C, hw = a.hw, K = a.K;
  float* cs = km_smem;                                   // [C][NK]
  float* red = cs + (SCORE ? NK * C : 0);                // [GRP][NK][TP]
  float* tile = red + (SCORE ? kT * NK : 0);             // [C][TS]
  int* labs = (int*)(tile + (ADD ? C * TS : 0));         // [TP]

  if constexpr (SCORE) {
    const float* src = a.cen;
    int64_t stride = 1;
    if constexpr (MODE == DIST) {
      if (a.seed) {
        const int g = min(max(*a.seed, 0), a.npoints - 1), b = g / hw;
        src = a.x + (int64_t)b * C * hw + (g - b * hw);
        stride = hw;
      }
    }
    for (int i = tid; i < NK * C; i += kT) {
      const int k = i / C, ch = i - k * C;
      cs[ch * NK + k] = k < K ? src[((int64_t)k * C + ch) * stride] : 0.f;
    }
  }

  float acc[kCPT][NK];
#pragma unroll
  for (int j = 0; j < kCPT; ++j)
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[j][k] = 0.f;
  int cnt = 0;                       // thread k < K: the points of this workgroup labelled k
  float bestv = -INFINITY;           // DIST, thread 0: the workgroup's farthest point so far
  int besti = INT_MAX;
  __syncthreads();

  // the loop's bounds are workgroup-uniform, so all 256 threads meet at every barrier
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int b = t / a.tiles_per_map, p0 = (t - b * a.tiles_per_map) * TP, np = min(TP, hw - p0);
    const float* X = a.x + (int64_t)b * C * hw + min(p0 + p, hw - 1);  // a pixel past the map reads the last one
    float d[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) d[k] = 0.f;
#pragma unroll 8
    for (int ch = grp; ch < C; ch += GRP) {
      const float v = X[(int64_t)ch * hw];
      if constexpr (ADD) tile[ch * TS + p] = v;
      if constexpr (SCORE) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const float e = v - cs[ch * NK + k];
          d[k] = fmaf(e, e, d[k]);
        }
      }
    }
    if constexpr (SCORE) {
#pragma unroll
      for (int k = 0; k < NK; ++k) red[(grp * NK + k) * TP + p] = d[k];
      __syncthreads();
    }
    if (tid < 64) {                  // wave 0; its first TP lanes own a pixel each
      const bool valid = tid < np;
      const int64_t g = (int64_t)b * hw + p0 + tid;
      int lab = 255;
      float dm = -INFINITY;
      if constexpr (SCORE) {
        if (tid < TP) {
          float best = INFINITY;
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < GRP; ++q) s += red[(q * NK + k) * TP + tid];
            if (MODE == DIST) dm = s;
            if (k < K && s < best) {   // k ascends: the lowest k of equal distances stays; a NaN is never smaller
              best = s;
              lab = k;
            }
          }
        }
      } else {
        if (valid) lab = a.lin ? a.lin[g] : 0;
      }
      if constexpr (MODE == DIST) {
        if (valid) {
          if (!a.first) {
            const float o = a.dmin[g];
            dm = (dm < o || dm != dm) ? dm : o;   // a NaN on either side stays a NaN: such a point is never a seed
          }
          a.dmin[g] = dm;
        }
        float v = (valid && dm == dm) ? dm : -INFINITY;
        int ix = (valid && dm == dm) ? (int)g : INT_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(v, o, 64);
          const int oi = __shfl_xor(ix, o, 64);
          fold_arg<true>(v, ix, ov, oi);
        }
        fold_arg<true>(bestv, besti, v, ix);
      } else {
        if (tid < TP) labs[tid] = valid ? lab : 255;
        if constexpr (MODE != UPDATE)
          if (valid) a.lout[g] = (uint8_t)lab;
      }
    }
    if constexpr (MODE != DIST) {
      __syncthreads();
      if (tid < K)
        for (int q = 0; q < np; ++q) cnt += labs[q] == tid;
      if constexpr (ADD) {
        for (int q = 0; q < np; ++q) {
          const int l = __builtin_amdgcn_readfirstlane(labs[q]);
          if (l >= K) continue;
          float v[kCPT];
#pragma unroll
          for (int j = 0; j < kCPT; ++j) v[j] = tid + kT * j < C ? tile[(tid + kT * j) * TS + q] : 0.f;
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (l == k) {
#pragma unroll
              for (int j = 0; j < kCPT; ++j) acc[j][k] += v[j];
            }
        }
      }
    }
    __syncthreads();   // the next tile's stage overwrites the image, the distances and the labels
  }

  if constexpr (MODE == DIST) {
    if (tid == 0) {
      a.pval[blockIdx.x] = bestv;
      a.pidx[blockIdx.x] = besti;
    }
  } else {
    if (a.pcnt && tid < K) a.pcnt[blockIdx.x * K + tid] = cnt;
    if constexpr (ADD) {
#pragma unroll
      for (int j = 0; j < kCPT; ++j) {
        const int ch = tid + kT * j;
        if (ch < C) {
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (k < K) a.part[((int64_t)blockIdx.x * K + k) * C + ch] = acc[j][k];
        }
      }
    }
  }
}

// The sum over the tile kernel's workgroups of their counts of cluster k; every thread returns it.
__device__ __forceinline__ int count_sum(const int* __restrict__ pcnt, int nwg, int K, int k, int* sh) {
  int s = 0;
  for (int w = threadIdx.x; w < nwg; w += kT) s += pcnt[w * K + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// grid (channels / 64, K): the workgroups' partial sums of 64 channels of cluster k in four runs of
// consecutive workgroups, each added in workgroup order, then the four in run order; the mean, or the
// previous centroid (in bits) for an empty cluster. `prev` may be `cen`: a thread reads what it writes.
__global__ __launch_bounds__(kT) void kmeans_reduce_kernel(const float* __restrict__ part, const int* __restrict__ pcnt,
                                                          const float* prev, float* cen, int* __restrict__ counts,
                                                          int nwg, int K, int C) {
  __shared__ float sh[4][64];
  __shared__ int shc[4];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, k = blockIdx.y, ch = blockIdx.x * 64 + lane;
  const int per = (nwg + 3) / 4, w0 = q * per, w1 = min(w0 + per, nwg);
  float s = 0.f;
  if (ch < C) {
#pragma unroll 8
    for (int w = w0; w < w1; ++w) s += part[((int64_t)w * K + k) * C + ch];   // the loads of eight in flight, the adds in order
  }
  sh[q][lane] = s;
  const int n = count_sum(pcnt, nwg, K, k, shc);   // its barrier covers sh too
  if (q == 0 && ch < C) {
    const float tot = ast_tile::quarter_sum(sh, lane);
    const int64_t o = (int64_t)k * C + ch;
    cen[o] = n > 0 ? tot / (float)n : prev[o];
  }
  if (counts && blockIdx.x == 0 && threadIdx.x == 0) counts[k] = n;
}

// grid (K): counts alone, after the last assignment
__global__ __launch_bounds__(kT) void kmeans_count_kernel(const int* __restrict__ pcnt, int* __restrict__ counts, int nwg,
                                                         int K) {
  __shared__ int shc[4];
  const int n = count_sum(pcnt, nwg, K, blockIdx.x, shc);
  if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// one workgroup: the farthest point over the DIST workgroups' partials, the lowest g of equal distances;
// 0 where no point has a distance that compares (all NaN)
__global__ __launch_bounds__(kT) void kmeans_argmax_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                          int* __restrict__ seed, int nwg) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  float v = -INFINITY;
  int ix = INT_MAX;
  for (int w = threadIdx.x; w < nwg; w += kT) fold_arg<true>(v, ix, pval[w], pidx[w]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(ix, o, 64);
    fold_arg<true>(v, ix, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) {
    shv[threadIdx.x >> 6] = v;
    shi[threadIdx.x >> 6] = ix;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; ++q) fold_arg<true>(v, ix, shv[q], shi[q]);
    *seed = ix == INT_MAX ? 0 : ix;
  }
}

// grid (channels / 256, K): cen[k] = the point seeds[k] (clamped into the bank), or init[k], in bits
__global__ __launch_bounds__(kT) void kmeans_gather_kernel(const float* __restrict__ x, const int* __restrict__ seeds,
                                                          const float* __restrict__ init, float* __restrict__ cen, int C,
                                                          int hw, int npoints) {
  const int ch = blockIdx.x * kT + threadIdx.x, k = blockIdx.y;
  if (ch >= C) return;
  if (init) {
    cen[(int64_t)k * C + ch] = init[(int64_t)k * C + ch];
    return;
  }
  const int g = min(max(seeds[k], 0), npoints - 1), b = g / hw;
  cen[(int64_t)k * C + ch] = x[((int64_t)b * C + ch) * hw + (g - b * hw)];
}

// grid (pixels / 256, maps): one pass of the 3x3 majority vote. The votes of the up-to-nine labels
// below K in the clipped window are nibbles of one word (a count is at most 9); the most frequent
// label wins, the lowest on a tie unless the centre's own label is among the tied. A centre >= K
// passes through.
__global__ __launch_bounds__(kT) void label_mode_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int h,
                                                       int w, int K) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= h * w) return;
  const int y = p / w, x = p - y * w;
  const uint8_t* I = in + (int64_t)blockIdx.y * h * w;
  const unsigned own = I[p];
  unsigned res = own;
  if ((int)own < K) {
    unsigned votes = 0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        const unsigned l = I[yy * w + xx];
        if ((int)l < K) votes += 1u << (4 * l);
      }
    unsigned bestc = 0;
    for (int k = 0; k < K; ++k) {
      const unsigned c = (votes >> (4 * k)) & 15u;
      if (c > bestc) {
        bestc = c;
        res = (unsigned)k;
      }
    }
    if (((votes >> (4 * own)) & 15u) == bestc) res = own;
  }
  out[(int64_t)blockIdx.y * h * w + p] = (uint8_t)res;
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layout, launch sequences
// ------------------------------------------------------------------------------------------------

// AST_OK, or the code that rejects a bank [b, c, h, w] and k clusters
inline int bank_shape(int b, int c, int h, int w, int k) {
  if (b <= 0 || c <= 0 || h <= 0 || w <= 0 || k <= 0) return AST_E_SHAPE;
  if ((int64_t)h * w > kMaxPoints || (int64_t)b * h * w > kMaxPoints) return AST_E_SHAPE;
  if (c > kMaxC || k > kMaxK) return AST_E_UNSUPPORTED;
  return AST_OK;
}

// centroid slots per channel of the instantiation that serves k clusters
inline int nk_of(int k) { return k == 1 ? 1 : k <= 4 ? 4 : 8; }

// Pixels per tile: 32 where two workgroups of the fused kernel fit a CU's LDS, else 16 (at C = 512 that
// is 32 up to K = 4 and 16 above; with one workgroup per CU too few loads are in flight: measured,
// DESIGN.md section 3). Every mode takes the fused mode's choice, so the stages and their composition
// cut the bank into the same tiles.
inline int tp_of(int c, int nk) { return 2 * 4 * lds_floats(FUSED, 32, nk, c) <= kLdsMax ? 32 : 16; }

struct Plan {
  int tp, nk, tiles_per_map, ntiles, grid, wide_grid;
};

inline Plan plan_of(int b, int c, int h, int w, int k) {
  Plan p;
  p.nk = nk_of(k);
  p.tp = tp_of(c, p.nk);
  p.tiles_per_map = (h * w + p.tp - 1) / p.tp;
  p.ntiles = b * p.tiles_per_map;   // <= 2^24 / 16 + b
  p.grid = p.ntiles < kMaxWGs ? p.ntiles : kMaxWGs;
  p.wide_grid = p.ntiles < kMaxWideWGs ? p.ntiles : kMaxWideWGs;
  return p;
}

template <int TP, int NK, int MODE>
int launch_tile(const TileArgs& a, int grid, hipStream_t st) {
  const size_t lds = (size_t)(4 * lds_floats(MODE, TP, NK, a.C));
  auto kern = kmeans_tile_kernel<TP, NK, MODE>;
  if (lds > 64 * 1024) {   // dynamic LDS above 64 KB has to be allowed per kernel (as efdm.hip does)
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kT), lds, st, a);
  return (int)hipGetLastError();
}

template <int MODE>
int launch_mode(const TileArgs& a, const Plan& p, hipStream_t st) {
  const int grid = (MODE == ASSIGN || MODE == DIST) ? p.wide_grid : p.grid;
  if (p.tp == 32) {
    if (p.nk == 1) return launch_tile<32, 1, MODE>(a, grid, st);
    if (p.nk == 4) return launch_tile<32, 4, MODE>(a, grid, st);
    return launch_tile<32, 8, MODE>(a, grid, st);
  }
  if (p.nk == 1) return launch_tile<16, 1, MODE>(a, grid, st);
  if (p.nk == 4) return launch_tile<16, 4, MODE>(a, grid, st);
  return launch_tile<16, 8, MODE>(a, grid, st);
}

inline TileArgs base_args(const float* x, const Plan& p, int b, int c, int h, int w, int k) {
  TileArgs a{};
  a.x = x;
  a.C = c;
  a.hw = h * w;
  a.K = k;
  a.tiles_per_map = p.tiles_per_map;
  a.ntiles = p.ntiles;
  a.npoints = b * h * w;
  return a;
}

// The workspace of every entry: [partial sums grid x K x C | partial counts wide grid x K | dmin B HW |
// partial maxima wide grid | their points wide grid | mean C | seeds K]
struct Ws {
  float* part;
  int* pcnt;
  float* dmin;
  float* pval;
  int* pidx;
  float* mean;
  int* seeds;
  int64_t bytes;
};

inline Ws ws_of(unsigned char* base, int b, int c, int h, int w, int k) {
  // the seeding runs with one centroid, so with a plan of its own: size for the larger grid
  const Plan pk = plan_of(b, c, h, w, k), p1 = plan_of(b, c, h, w, 1);
  const int64_t g = pk.grid > p1.grid ? pk.grid : p1.grid;
  ast_ws::Walk wk(base);
  Ws s;
  s.part = wk.take<float>(4 * g * k * c);
  s.pcnt = wk.take<int>((int64_t)4 * pk.wide_grid * k);   // wide_grid >= grid
  s.dmin = wk.take<float>((int64_t)4 * b * h * w);
  s.pval = wk.take<float>((int64_t)4 * p1.wide_grid);
  s.pidx = wk.take<int>((int64_t)4 * p1.wide_grid);
  s.mean = wk.take<float>(4 * c);
  s.seeds = wk.take<int>(4 * kMaxK);
  s.bytes = wk.off;
  return s;
}

int assign_launch(const float* x, const float* cen, uint8_t* labels, int* pcnt, int b, int c, int h, int w, int k,
                  hipStream_t st) {
  const Plan p = plan_of(b, c, h, w, k);
  TileArgs a = base_args(x, p, b, c, h, w, k);
  a.cen = cen;
  a.lout = labels;
  a.pcnt = pcnt;
  return launch_mode<ASSIGN>(a, p, st);
}

int reduce_launch(const Ws& s, const float* prev, float* cen, int* counts, int grid, int c, int k, hipStream_t st) {
  hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((c + 63) / 64, k), dim3(kT), 0, st, (const float*)s.part,
                     (const int*)s.pcnt, prev, cen, counts, grid, k, c);
  return (int)hipGetLastError();
}

// UPDATE (labels given) or FUSED (labels written), then the reduction
int update_launch(const float* x, const uint8_t* lin, uint8_t* lout, const float* prev, float* cen, int* counts, int b,
                  int c, int h, int w, int k, const Ws& s, bool fused, hipStream_t st) {
  const Plan p = plan_of(b, c, h, w, k);
  TileArgs a = base_args(x, p, b, c, h, w, k);
  a.cen = prev;
  a.lin = lin;
  a.lout = lout;
  a.part = s.part;
  a.pcnt = s.pcnt;
  const int e = fused ? launch_mode<FUSED>(a, p, st) : launch_mode<UPDATE>(a, p, st);
  if (e) return e;
  return reduce_launch(s, prev, cen, counts, p.grid, c, k, st);
}

int seed_launch(const float* x, int* seeds, int b, int c, int h, int w, int k, const Ws& s, hipStream_t st) {
  const Plan p = plan_of(b, c, h, w, 1);
  // the mean: an update of one cluster that holds every point
  TileArgs a = base_args(x, p, b, c, h, w, 1);
  a.part = s.part;
  a.pcnt = s.pcnt;
  int e = launch_mode<UPDATE>(a, p, st);
  if (e) return e;
  e = reduce_launch(s, s.mean, s.mean, nullptr, p.grid, c, 1, st);   // the count is B HW > 0: prev is never read
  if (e) return e;
  for (int j = 0; j < k; ++j) {
    TileArgs d = base_args(x, p, b, c, h, w, 1);
    d.cen = s.mean;
    d.seed = j ? seeds + j - 1 : nullptr;
    d.first = j <= 1;   // the distance to the mean picks seed 0 only: dmin runs over the seeds
    d.dmin = s.dmin;
    d.pval = s.pval;
    d.pidx = s.pidx;
    e = launch_mode<DIST>(d, p, st);
    if (e) return e;
    hipLaunchKernelGGL(kmeans_argmax_kernel, dim3(1), dim3(kT), 0, st, (const float*)s.pval, (const int*)s.pidx,
                       seeds + j, p.wide_grid);
    e = (int)hipGetLastError();
    if (e) return e;
  }
  return 0;
}

int gather_launch(const float* x, const int* seeds, const float* init, float* cen, int b, int c, int h, int w, int k,
                  hipStream_t st) {
  hipLaunchKernelGGL(kmeans_gather_kernel, dim3((c + kT - 1) / kT, k), dim3(kT), 0, st, x, seeds, init, cen, c, h * w,
                     b * h * w);
  return (int)hipGetLastError();
}

inline int map_shape(int n, int h, int w) {
  if (n <= 0 || n > 65535 || h <= 0 || w <= 0 || (int64_t)h * w > kMaxPoints) return AST_E_SHAPE;
  return AST_OK;
}

}  // namespace

extern "C" {

long long ast_kmeans_workspace_bytes(int b, int c, int h, int w, int k) {
  const int e = bank_shape(b, c, h, w, k);
  return e ? e : ws_of(nullptr, b, c, h, w, k).bytes;
}

int ast_kmeans_seed_f32(const float* x, int* seeds, int b, int c, int h, int w, int k, void* workspace,
                        long long workspace_bytes, void* stream) {
  if (!x || !seeds || !workspace) return AST_E_NULLPTR;
  const int e = bank_shape(b, c, h, w, k);
  if (e) return e;
  const Ws s = ws_of((unsigned char*)workspace, b, c, h, w, k);
  if (workspace_bytes < s.bytes) return AST_E_SHAPE;
  return seed_launch(x, seeds, b, c, h, w, k, s, (hipStream_t)stream);
}

int ast_kmeans_assign_f32(const float* x, const float* centroids, unsigned char* labels, int b, int c, int h, int w,
                          int k, void* stream) {
  if (!x || !centroids || !labels) return AST_E_NULLPTR;
  const int e = bank_shape(b, c, h, w, k);
  if (e) return e;
  return assign_launch(x, centroids, labels, nullptr, b, c, h, w, k, (hipStream_t)stream);
}

int ast_kmeans_update_f32(const float* x, const unsigned char* labels, const float* prev_centroids, float* centroids,
                          int* counts, int b, int c, int h, int w, int k, void* workspace, long long workspace_bytes,
                          void* stream) {
  if (!x || !labels || !prev_centroids || !centroids || !counts || !workspace) return AST_E_NULLPTR;
  const int e = bank_shape(b, c, h, w, k);
  if (e) return e;
  const Ws s = ws_of((unsigned char*)workspace, b, c, h, w, k);
  if (workspace_bytes < s.bytes) return AST_E_SHAPE;
  return update_launch(x, labels, nullptr, prev_centroids, centroids, counts, b, c, h, w, k, s, false,
                       (hipStream_t)stream);
}

int ast_kmeans_f32(const float* x, const float* init_or_null, float* centroids, unsigned char* labels, int* counts,
                   int* seeds_or_null, int b, int c, int h, int w, int k, int iters, void* workspace,
                   long long workspace_bytes, void* stream) {
  if (!x || !centroids || !labels || !counts || !workspace) return AST_E_NULLPTR;
  int e = bank_shape(b, c, h, w, k);
  if (e) return e;
  if (iters < 0) return AST_E_UNSUPPORTED;
  const Ws s = ws_of((unsigned char*)workspace, b, c, h, w, k);
  if (workspace_bytes < s.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  int* seeds = seeds_or_null ? seeds_or_null : s.seeds;
  if (!init_or_null) {
    e = seed_launch(x, seeds, b, c, h, w, k, s, st);
    if (e) return e;
  }
  e = gather_launch(x, seeds, init_or_null, centroids, b, c, h, w, k, st);
  if (e) return e;
  for (int it = 0; it < iters; ++it) {
    e = update_launch(x, nullptr, labels, centroids, centroids, counts, b, c, h, w, k, s, true, st);
    if (e) return e;
  }
  e = assign_launch(x, centroids, labels, s.pcnt, b, c, h, w, k, st);
  if (e) return e;
  hipLaunchKernelGGL(kmeans_count_kernel, dim3(k), dim3(kT), 0, st, (const int*)s.pcnt, counts,
                     plan_of(b, c, h, w, k).wide_grid, k);
  return (int)hipGetLastError();
}

long long ast_label_mode_filter_workspace_bytes(int n, int h, int w, int passes) {
  const int e = map_shape(n, h, w);
  if (e) return e;
  if (passes < 0) return AST_E_UNSUPPORTED;
  return passes > 1 ? ast_ws::al256((int64_t)n * h * w) : 0;
}

int ast_label_mode_filter_u8(const unsigned char* labels, unsigned char* out, int n, int h, int w, int regions,
                             int passes, void* workspace, long long workspace_bytes, void* stream) {
  if (!labels || !out || labels == out) return AST_E_NULLPTR;
  const int e = map_shape(n, h, w);
  if (e) return e;
  if (regions < 1 || regions > AST_MAX_REGIONS || passes < 0) return AST_E_UNSUPPORTED;
  if (passes > 1 && !workspace) return AST_E_NULLPTR;
  if (workspace_bytes < ast_label_mode_filter_workspace_bytes(n, h, w, passes)) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((h * w + kT - 1) / kT, n);
  if (passes == 0) {   // a vote among no labels: every pixel passes through
    hipLaunchKernelGGL(label_mode_kernel, grid, dim3(kT), 0, st, labels, out, h, w, 0);
    return (int)hipGetLastError();
  }
  // the passes alternate between out and the workspace so that the last one writes out
  const unsigned char* src = labels;
  for (int i = 0; i < passes; ++i) {
    unsigned char* dst = (passes - 1 - i) % 2 == 0 ? out : (unsigned char*)workspace;
    hipLaunchKernelGGL(label_mode_kernel, grid, dim3(kT), 0, st, src, dst, h, w, regions);
    src = dst;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
