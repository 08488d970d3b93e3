// Contextual loss (Mechrez, Talmi, Zelnik-Manor, ECCV 2018) for gfx950, fp32 storage, exact: every pixel
// pair takes part, nothing is sampled, and no M x P tensor is ever stored. The soft counterpart of the
// relaxed EMD of remd.hip, on the same match tile. The definition is in include/ast_hip.h;
// tests/cx_ref.py restates it. Inputs: x [n, C, M pixels], the differentiable side, and y [ns, C, P pixels]
// (ns = n, or 1 for a target shared by the batch), dense NCHW with the spatial sides flattened.
//   mu[c] = mean_j y[c, j];  xc = x - mu, yc = y - mu   (centring, optional)
//   u_i, v_j, D(i, j)   those of ast_cosine_norms_f32 / ast_cosine_match_f32 on (xc, yc), bit for bit
//   r_i = min_j D(i, j), m_i its arg-min (ast_cosine_match_f32 as it is);  k_i = 1 / (r_i + eps)
//   w(i, j) = exp((1 - D(i, j) k_i) / h);  S_i = sum_j w(i, j);  E_i = sum_j w(i, j) D(i, j)
//   CX(i, j) = w(i, j) / S_i;  c_j = max_i CX(i, j), a_j its arg-max (lowest index on equal values, a NaN
//   never wins, (-inf, 0) without a winner);  CX_b = (1 / P) sum_j c_j;  L = weight / n * sum_b -log CX_b
// Stages, each a C-ABI entry of its own; ast_cx_loss_f32 is exactly centre, norms, norms, match, rowsum,
// colmax, value:
//   centre  one launch sums every channel of y over the pixels in a fixed order (the launch of
//           selfsim.hip's channel sums), one launch per map subtracts.
//   rowsum  the loop of remd.hip's match: a workgroup owns 64 content pixels and streams 64-pixel style
//           tiles, both operands from NCHW by stage_load / stage_store, 32 v_mfma_f32_32x32x2_f32 per wave
//           and chunk with the next chunk's loads in flight. D comes from the match's expression
//           (cx_dist), so D(i, m_i) is row_min in bits; w from cx_w, the one function all three passes
//           share. A lane keeps a running (S, E) per accumulator row over the tiles in ascending order;
//           then a butterfly over the 32 lanes of a half, the other wave of the row, and a merge of the
//           splits in split order.
//   colmax  the same loop with S_i and k_i of the workgroup's rows resident: a column folds over the lane's
//           16 rows, the other lane half and the other wave and goes out as this content tile's partial
//           (value, index, distance at the winner); a merge in content-tile order follows (strictly
//           greater: the lowest index stays). Nothing depends on the splits.
//   value   per sample CX_b in a fixed order, then a one-workgroup launch adds the loss into the accumulator.
// Backward (to x only), an attention-like pass that recomputes the weights instead of reading them:
//   invert  the ascending lists J_i = { j : a_j = i }: count, scan, stable fill, integer work alone. This
//           is a copy of remd_invert_kernel without its branch test: shared through a header, remd.hip's
//           device assembly changes (the branch argument goes), so each file keeps its own.
//   rows    A_i, B_i over the list from col_dist and cx_w; alpha_i = k_i / (h S_i), beta_i = A_i / S_i,
//           tau_i = k_i^2 T_i / h, an active flag per row and per 64-row tile.
//   dense   a workgroup owns 64 rows and up to 512 channels and walks the style tiles: it recomputes the
//           64 x 64 block of D (K = C) as the forward does, builds
//             c'(i, j) = (alpha_i w(i, j) ([a_j = i] - beta_i) - tau_i [j = m_i]) v_j
//           on the VALU into LDS and multiplies it by the raw yc tile on the same MFMA (self-similarity's
//           form), one block of 128 channels after the other into 32 accumulators per block: 4 M P C FLOP
//           for C <= 512. A tile without an active row writes zeros and computes nothing. G goes to the
//           workspace.
//   finish  dx_i = -(g weight / (n P CX_b)) u_i (G_i - xh_i <xh_i, G_i>), every element written once.
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
using ast_tile::quarter_sum;
using ast_tile::stage_load;
using ast_tile::stage_store;
using ast_wave::block_sum;

constexpr int kT = 256;     // threads per workgroup everywhere in this file
constexpr int MT = 64;      // pixels per tile side (4 waves x 32 x 32)
constexpr int KC = 64;      // channels per staged chunk of the forward passes
constexpr int RT = KC / 4;  // channel runs per wave and chunk
constexpr int BKC = 32;     // and of the backward's distance block, whose LDS also holds c' and the yc tile
constexpr int BRT = BKC / 4;
constexpr int kMaxC = AST_CX_MAX_C;
constexpr int kMaxPixels = AST_CX_MAX_PIXELS;
constexpr int kTargetWGs = 8 * 256;  // the match's split rule (remd.hip)
constexpr int kMinSplitTiles = 4;
constexpr int CH = 128;     // channels per block of the backward GEMM: 32 accumulators per lane and block
constexpr int XP = MT + 1;  // padded row of the backward's yc tile in LDS
// channel blocks per workgroup of the backward's dense pass, at most; -DCX_DENSE_BLOCKS=1 builds the form that
// recomputes the distance block for every block of CH channels (the A/B of scripts/bench_cx.py)
#ifndef CX_DENSE_BLOCKS
#define CX_DENSE_BLOCKS 4
#endif
constexpr int kDenseBlocks = CX_DENSE_BLOCKS < 1 ? 1 : CX_DENSE_BLOCKS > 4 ? 4 : CX_DENSE_BLOCKS;

// The match's distance (remd_match_kernel): the same expression, contracted the same way.
__device__ __forceinline__ float cx_dist(float acc, float u, float v) { return 1.0f - (acc * u) * v; }

__device__ __forceinline__ float cx_k(float rmin) { return 1.0f / (rmin + AST_CX_EPS); }

// w(i, j): one function for the row pass, the column pass and the backward; every operation rounds on
// its own, so the three get the same bits from the same (d, k, h).
__device__ __forceinline__ float cx_w(float d, float k, float h) {
#pragma clang fp contract(off)
  const float t = d * k;
  const float a = 1.0f - t;
  return expf(a / h);
}

// ------------------------------------------------------------------------------------------------
// Centring
// ------------------------------------------------------------------------------------------------

// grid (channels, style samples): mu[b, ch] = (sum_p y[ch, p]) / P; thread t sums pixels t, t + 256, ... in
// order, then order A of wave.h.
__global__ __launch_bounds__(kT) void cx_mean_kernel(const float* __restrict__ y, float* __restrict__ mu, int C, int P) {
  __shared__ float sh[kT / 64];
  const int ch = blockIdx.x, b = blockIdx.y;
  const float* Y = y + ((int64_t)b * C + ch) * P;
  float s = 0.f;
  for (int p = threadIdx.x; p < P; p += kT) s += Y[p];
  const float t = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) mu[(int64_t)b * C + ch] = t / (float)P;
}

// grid (pixels / 256, channels, samples): out = in - mu[style sample, ch]
__global__ __launch_bounds__(kT) void cx_sub_kernel(const float* __restrict__ in, const float* __restrict__ mu,
                                                   float* __restrict__ out, int C, int hw, int style_batch) {
  const int p = blockIdx.x * kT + threadIdx.x, ch = blockIdx.y, b = blockIdx.z, bs = style_batch == 1 ? 0 : b;
  if (p >= hw) return;
  const int64_t o = ((int64_t)b * C + ch) * hw + p;
  out[o] = in[o] - mu[(int64_t)bs * C + ch];
}

// ------------------------------------------------------------------------------------------------
// The two soft passes
// ------------------------------------------------------------------------------------------------

// grid (content tiles, splits, samples). COL = false, the row sums: (S, E) of sample b and split s at
// [(b * splits + s) * M + i], the outputs themselves when splits == 1. COL = true, the column maxima: the
// triple of content tile t at [(b * tiles + t) * P + j]; a style pixel is visited by exactly one split.
template <bool COL>
__global__ __launch_bounds__(kT) void cx_pass_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ u, const float* __restrict__ v,
                                                    const float* __restrict__ rmin, const float* __restrict__ rsum,
                                                    float* __restrict__ o0, float* __restrict__ o1,
                                                    int* __restrict__ oi, int C, int M, int P, int style_batch,
                                                    int tiles_per_split, float h) {
  __shared__ float As[KC * MT];
  __shared__ float Bs[KC * MT];
  __shared__ float colv[2][32];
  __shared__ float cold[2][32];
  __shared__ int coli[2][32];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave & 1, wn = wave >> 1;
  const int b = blockIdx.z, bs = style_batch == 1 ? 0 : b, split = blockIdx.y;
  const int ptiles = (P + MT - 1) / MT, m0 = blockIdx.x * MT;
  const int jt_beg = split * tiles_per_split, jt_end = min(jt_beg + tiles_per_split, ptiles);
  const float* Ab = x + (int64_t)b * C * M;
  const float* Bb = y + (int64_t)bs * C * P;
  const float* vb = v + (int64_t)bs * P;
  const float* Ar = As + hh * MT + wm * 32 + r;
  const float* Br = Bs + hh * MT + wn * 32 + r;

  // the lane's 16 accumulator rows: content pixel m0 + wm * 32 + acc_row(i, hh)
  float ur[16], kr[16], sr[16], er[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int gi = m0 + wm * 32 + acc_row(i, hh);
    const int64_t o = (int64_t)b * M + gi;
    ur[i] = gi < M ? u[o] : 0.f;
    kr[i] = gi < M ? cx_k(rmin[o]) : 0.f;
    sr[i] = COL ? (gi < M ? rsum[o] : 1.f) : 0.f;  // COL: S_i; else the running S
    er[i] = 0.f;
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
      // k order of every distance: ascending channel pairs, as in the match
#pragma unroll
      for (int cp = 0; cp < KC / 2; ++cp)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ar[2 * cp * MT], Br[2 * cp * MT], acc, 0, 0, 0);
      __syncthreads();
    }
    const float vj = jvalid ? vb[jl] : 0.f;
    if (!COL) {
#pragma clang fp contract(off)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = cx_dist(acc[i], ur[i], vj);
        const float w = jvalid ? cx_w(d, kr[i], h) : 0.f;
        sr[i] += w;
        er[i] += jvalid ? w * d : 0.f;
      }
    } else {
      float cmax = -INFINITY, cd = 0.f;
      int cix = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int gi = m0 + wm * 32 + acc_row(i, hh);
        const float d = cx_dist(acc[i], ur[i], vj);
        const float cx = cx_w(d, kr[i], h) / sr[i];
        if (gi < M && cx > cmax) {  // the lane's rows ascend with i
          cmax = cx;
          cix = gi;
          cd = d;
        }
      }
      // the column: the other lane half holds the rows in between, the wm = 1 wave the 32 rows after
      {
        const float ov = __shfl_xor(cmax, 32, 64), od = __shfl_xor(cd, 32, 64);
        const int ox = __shfl_xor(cix, 32, 64);
        if (ov > cmax || (ov == cmax && ox < cix)) {
          cmax = ov;
          cix = ox;
          cd = od;
        }
      }
      if (wm == 1 && hh == 0) {
        colv[wn][r] = cmax;
        coli[wn][r] = cix;
        cold[wn][r] = cd;
      }
      __syncthreads();  // the wm = 1 waves write colv again only after the next tile's chunk barriers
      if (wm == 0 && hh == 0 && jvalid) {
        if (colv[wn][r] > cmax) {
          cmax = colv[wn][r];
          cix = coli[wn][r];
          cd = cold[wn][r];
        }
        const int64_t o = ((int64_t)b * gridDim.x + blockIdx.x) * P + jl;
        o0[o] = cmax;
        oi[o] = cix;
        o1[o] = cd;
      }
    }
  }

  if (!COL) {
    // the 32 lanes of a half hold the same 16 rows over different columns; then the two waves of a row
    float* reds = As;  // [2 wm][32 rows] of the wn = 1 waves; As is free after the loop's last barrier
    float* rede = As + 64;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float s = sr[i], e = er[i];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        e += __shfl_xor(e, o, 64);
      }
      sr[i] = s;
      er[i] = e;
    }
    if (wn == 1 && r == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hh);
        reds[wm * 32 + row] = sr[i];
        rede[wm * 32 + row] = er[i];
      }
    }
    __syncthreads();
    if (wn == 0 && r == 0) {
      const int64_t ob = ((int64_t)b * gridDim.y + split) * M;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hh), gi = m0 + wm * 32 + row;
        if (gi >= M) continue;
        o0[ob + gi] = sr[i] + reds[wm * 32 + row];
        o1[ob + gi] = er[i] + rede[wm * 32 + row];
      }
    }
  }
}

// grid (pixels / 256, samples): the splits' (S, E) partials of a row, added in split order
__global__ __launch_bounds__(kT) void cx_rowmerge_kernel(const float* __restrict__ ps, const float* __restrict__ pe,
                                                        float* __restrict__ S, float* __restrict__ E, int M,
                                                        int splits) {
  const int i = blockIdx.x * kT + threadIdx.x, b = blockIdx.y;
  if (i >= M) return;
  float s = 0.f, e = 0.f;
  for (int k = 0; k < splits; ++k) {
    s += ps[((int64_t)b * splits + k) * M + i];
    e += pe[((int64_t)b * splits + k) * M + i];
  }
  S[(int64_t)b * M + i] = s;
  E[(int64_t)b * M + i] = e;
}

// grid (pixels / 256, samples): the content tiles' triples of a column in tile order. A later tile holds
// higher indices only, so strictly greater keeps the lowest index of equal values: merge_slots<true> of
// match_tile.h with the distance at the winner as a payload.
__global__ __launch_bounds__(kT) void cx_colmerge_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                        const float* __restrict__ pdist, float* __restrict__ oval,
                                                        int* __restrict__ oidx, float* __restrict__ odist, int P,
                                                        int slots) {
  const int j = blockIdx.x * kT + threadIdx.x, b = blockIdx.y;
  if (j >= P) return;
  float v = -INFINITY, d = 0.f;
  int ix = 0;
  for (int s = 0; s < slots; ++s) {
    const int64_t o = ((int64_t)b * slots + s) * P + j;
    const float ov = pval[o];
    if (ov > v) {
      v = ov;
      ix = pidx[o];
      d = pdist[o];
    }
  }
  oval[(int64_t)b * P + j] = v;
  oidx[(int64_t)b * P + j] = ix;
  odist[(int64_t)b * P + j] = d;
}

// ------------------------------------------------------------------------------------------------
// Value
// ------------------------------------------------------------------------------------------------

// grid (samples): CX_b = (thread t sums columns t, t + 256, ... in order, then order A of wave.h) / P
__global__ __launch_bounds__(kT) void cx_sample_kernel(const float* __restrict__ ccx, float* __restrict__ cxb, int P) {
  __shared__ float sh[kT / 64];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int j = threadIdx.x; j < P; j += kT) s += ccx[(int64_t)b * P + j];
  const float t = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) cxb[b] = t / (float)P;
}

// one workgroup: *loss += w_over_n * sum over the samples, in sample order per thread, of -log CX_b
__global__ __launch_bounds__(kT) void cx_total_kernel(const float* __restrict__ cxb, float* loss, int n, float w_over_n) {
  __shared__ float sh[kT / 64];
  float s = 0.f;
  for (int b = threadIdx.x; b < n; b += kT) s += -logf(cxb[b]);
  const float t = block_sum<kT / 64>(s, sh);
  ast_det::loss_acc_commit(loss, w_over_n * t);
}

// ------------------------------------------------------------------------------------------------
// Backward
// ------------------------------------------------------------------------------------------------

// The rank of thread t's key among the equal keys of the chunk before it, and whether an equal key
// follows it. keys: 256 ints in LDS, visible. (remd.hip's chunk_rank.)
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

// grid (samples): start[b, i] .. start[b, i + 1] delimit, in list[b, .], the ascending style pixels j with
// cidx[b, j] == i (an index outside 0 .. M - 1 is clamped). start [n, M + 1], cursor [n, M], list [n, P].
// Integer work only, no atomics: remd_invert_kernel without its branch test.
__global__ __launch_bounds__(kT) void cx_invert_kernel(const int* __restrict__ cidx, int* start, int* cursor,
                                                      int* __restrict__ list, int M, int P) {
  __shared__ __attribute__((aligned(16))) int keys[kT];
  __shared__ int scan[kT];
  __shared__ int carry;
  const int b = blockIdx.x, t = threadIdx.x;
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

// grid (pixels / 256, samples): the row scalars from the lists, in ascending j. rs [n, 3, M]: alpha, beta,
// tau; act [n, M]; tact [n, tiles]: whether the 64-row tile (one wave here) holds an active row.
__global__ __launch_bounds__(kT) void cx_rows_kernel(const float* __restrict__ u, const float* __restrict__ rmin,
                                                    const float* __restrict__ S, const float* __restrict__ E,
                                                    const float* __restrict__ cdist, const int* __restrict__ start,
                                                    const int* __restrict__ list, float* __restrict__ rs,
                                                    int* __restrict__ act, int* __restrict__ tact, int M, int P,
                                                    int tiles, float h) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kT + threadIdx.x, b = blockIdx.y;
  bool active = false;
  if (i < M) {
    const int64_t o = (int64_t)b * M + i;
    const int beg = start[(int64_t)b * (M + 1) + i], end = start[(int64_t)b * (M + 1) + i + 1];
    const float k = cx_k(rmin[o]), s = S[o], e = E[o];
    const float* Cd = cdist + (int64_t)b * P;
    const int* Ls = list + (int64_t)b * P;
    float A = 0.f, B = 0.f;
    for (int q = beg; q < end; ++q) {
      const float d = Cd[Ls[q]];
      const float w = cx_w(d, k, h);
      A += w;
      B += w * d;
    }
    active = beg < end && u[o] != 0.f;
    const float T = B / s - (A * e) / (s * s);
    float* R = rs + (int64_t)b * 3 * M + i;
    R[0] = active ? k / (h * s) : 0.f;
    R[M] = active ? A / s : 0.f;
    R[2 * (int64_t)M] = active ? (k * k) * T / h : 0.f;
    act[o] = active ? 1 : 0;
  }
  const bool any = __ballot(active) != 0;
  const int tile = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && tile < tiles) tact[(int64_t)b * tiles + tile] = any ? 1 : 0;
}

// grid (content tiles, channels / (NB CH), samples): G[b, ch, i] = sum_j c'(i, j) yc[b, ch, j], the style
// tiles in ascending order, inside a tile ascending j pairs on the MFMA. Per style tile: the distance block
// as in the forward (lane = column j, 16 rows), once; c' into LDS; then, for each of the workgroup's NB
// blocks of CH channels in turn, the raw yc tile of the block into LDS and wave w multiplies channels
// 32 w .. 32 w + 31 of it into the block's own 32 accumulators (32 NB per lane), the next block's loads in
// flight. The sum of a G element runs in the same order for every NB.
template <int NB>
__global__ __launch_bounds__(kT) void cx_dense_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                     const float* __restrict__ u, const float* __restrict__ v,
                                                     const float* __restrict__ rmin, const int* __restrict__ ridx,
                                                     const int* __restrict__ cidx, const float* __restrict__ rs,
                                                     const int* __restrict__ act, const int* __restrict__ tact,
                                                     float* __restrict__ G, int C, int M, int P, int style_batch,
                                                     float h) {
  __shared__ float Sab[2 * BKC * MT];  // the chunk of x and of y; then c' [j][i], the row swizzled by j
  __shared__ float Ys[CH * XP];        // [channel][j], a row padded to 65
  __shared__ float rowf[5][MT];        // u, k, alpha, beta, tau of the workgroup's rows
  __shared__ int rowi[2][MT];          // m_i, active
  float* As = Sab;
  float* Bs = Sab + BKC * MT;
  float* Ws = Sab;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave & 1, wn = wave >> 1;
  const int tile = blockIdx.x, m0 = tile * MT, ch0 = blockIdx.y * (NB * CH), b = blockIdx.z;
  const int bs = style_batch == 1 ? 0 : b;
  const int ctiles = gridDim.x, ptiles = (P + MT - 1) / MT;

  if (!tact[(int64_t)b * ctiles + tile]) {  // uniform over the workgroup, before any barrier
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int ch = ch0 + q * CH + wave * 32 + r;
      if (ch < C) {
        float* Gc = G + ((int64_t)b * C + ch) * M;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int ma = m0 + acc_row(k, hh), mb = ma + 32;
          if (ma < M) Gc[ma] = 0.f;
          if (mb < M) Gc[mb] = 0.f;
        }
      }
    }
    return;
  }

  const float* Ab = x + (int64_t)b * C * M;
  const float* Bb = y + (int64_t)bs * C * P;
  const float* vb = v + (int64_t)bs * P;
  const int* cb = cidx + (int64_t)b * P;
  if (tid < MT) {
    const int gi = m0 + tid;
    const bool ok = gi < M;
    const int64_t o = (int64_t)b * M + gi;
    const float* R = rs + (int64_t)b * 3 * M + gi;
    rowf[0][tid] = ok ? u[o] : 0.f;
    rowf[1][tid] = ok ? cx_k(rmin[o]) : 0.f;
    rowf[2][tid] = ok ? R[0] : 0.f;
    rowf[3][tid] = ok ? R[M] : 0.f;
    rowf[4][tid] = ok ? R[2 * (int64_t)M] : 0.f;
    rowi[0][tid] = ok ? ridx[o] : -1;
    rowi[1][tid] = ok ? act[o] : 0;
  }
  const float* Ar = As + hh * MT + wm * 32 + r;
  const float* Br = Bs + hh * MT + wn * 32 + r;

  // channel block q of the raw yc tile at j0: wave w takes channels w, w + 4, ... of the block, lane l pixel j0 + l
  float ra[BRT], rb[BRT], yr[CH / 4];
  auto load_y = [&](int q, int j0) {
#pragma unroll
    for (int k = 0; k < CH / 4; ++k) {
      const int ch = ch0 + q * CH + wave + 4 * k, jj = j0 + lane;
      yr[k] = (ch < C && jj < P) ? Bb[(int64_t)ch * P + jj] : 0.f;
    }
  };
  stage_load(ra, Ab, C, M, m0, wave, lane);
  stage_load(rb, Bb, C, P, 0, wave, lane);
  f32x16 g[NB][2];
#pragma unroll
  for (int q = 0; q < NB; ++q) g[q][0] = g[q][1] = (f32x16){0.f};
  // every branch that encloses a barrier depends on block indices and kernel arguments alone
  for (int jt = 0; jt < ptiles; ++jt) {
    const int j0 = jt * MT, jl = wn * 32 + r, j = j0 + jl;
    const bool jvalid = j < P;
    load_y(0, j0);  // in flight while the distances are multiplied
    f32x16 acc = (f32x16){0.f};
    for (int c0 = 0; c0 < C; c0 += BKC) {
      stage_store(ra, As, wave, lane);
      stage_store(rb, Bs, wave, lane);
      __syncthreads();
      const bool wrap = c0 + BKC >= C;
      const int nc0 = wrap ? 0 : c0 + BKC;
      const int nj0 = (wrap && jt + 1 < ptiles ? jt + 1 : jt) * MT;
      stage_load(ra, Ab + (int64_t)nc0 * M, C - nc0, M, m0, wave, lane);
      stage_load(rb, Bb + (int64_t)nc0 * P, C - nc0, P, nj0, wave, lane);
      __builtin_amdgcn_sched_barrier(0);  // the loads are issued here, ahead of the products
#pragma unroll
      for (int cp = 0; cp < BKC / 2; ++cp)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ar[2 * cp * MT], Br[2 * cp * MT], acc, 0, 0, 0);
      __syncthreads();
    }
    const float vj = jvalid ? vb[j] : 0.f;
    const int aj = jvalid ? min(max(cb[j], 0), M - 1) : -1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int il = wm * 32 + acc_row(i, hh), gi = m0 + il;
      const float d = cx_dist(acc[i], rowf[0][il], vj);
      const float w = cx_w(d, rowf[1][il], h);
      const float ind = aj == gi ? 1.f : 0.f;
      const float hit = j == rowi[0][il] ? rowf[4][il] : 0.f;
      const float cv = (rowf[2][il] * w * (ind - rowf[3][il]) - hit) * vj;
      Ws[jl * MT + (il ^ r)] = (jvalid && rowi[1][il]) ? cv : 0.f;
    }
    const float* Yr = Ys + (wave * 32 + r) * XP + hh;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
#pragma unroll
      for (int k = 0; k < CH / 4; ++k) Ys[(wave + 4 * k) * XP + lane] = yr[k];
      __syncthreads();  // c' and this block's yc tile are visible
      if (q + 1 < NB) load_y(q + 1, j0);
#pragma unroll
      for (int kp = 0; kp < MT / 2; ++kp) {
        const int jj = 2 * kp + hh;
        const float bv = Yr[2 * kp];
        const float* Wr = Ws + jj * MT + (r ^ (jj & 31));
        g[q][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wr[0], bv, g[q][0], 0, 0, 0);
        g[q][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Wr[32], bv, g[q][1], 0, 0, 0);
      }
      __syncthreads();  // Ys and, after the last block, c' may be overwritten
    }
  }
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int ch = ch0 + q * CH + wave * 32 + r;
    if (ch < C) {
      float* Gc = G + ((int64_t)b * C + ch) * M;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int ma = m0 + acc_row(k, hh), mb = ma + 32;
        if (ma < M) Gc[ma] = g[q][0][k];
        if (mb < M) Gc[mb] = g[q][1][k];
      }
    }
  }
}

// grid (pixels / 64, samples): with q = -(g w / (n P CX_b)),
//   dx_i = u_i q (G_i - xh_i <xh_i, G_i>), 0 where u_i = 0 or no column chose i;
// thread (p, g) takes channels g, g + 4, ...; the four partials of the inner product are added in g order.
__global__ __launch_bounds__(kT) void cx_finish_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                      const float* __restrict__ G, const int* __restrict__ act,
                                                      const float* __restrict__ cxb, const float* __restrict__ g,
                                                      float* __restrict__ dx, int C, int M, float w_over_np) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.x * 64 + lane, b = blockIdx.y;
  const int64_t base = (int64_t)b * C * M + p;
  const float up = p < M ? u[(int64_t)b * M + p] : 0.f;
  const bool on = p < M && act[(int64_t)b * M + p] != 0;
  float d = 0.f;
  if (on)
    for (int ch = q; ch < C; ch += 4) d = fmaf(up * x[base + (int64_t)ch * M], G[base + (int64_t)ch * M], d);
  sh[q][lane] = d;
  __syncthreads();
  if (p >= M) return;
  const float dot = quarter_sum(sh, lane);
  const float k = -((g[0] * w_over_np) / cxb[b]) * up;
  for (int ch = q; ch < C; ch += 4) {
    const int64_t o = base + (int64_t)ch * M;
    dx[o] = on ? k * (G[o] - (up * x[o]) * dot) : 0.f;
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

inline int all_shape(int n, int ns, int c, int m, int p) {
  const int e = pair_shape(n, ns, m, p);
  return e ? e : chan_shape(c);
}

inline bool bad_h(float h) { return !(h > 0.f) || !(h < INFINITY); }

inline int splits_of(int n, int m, int p, int want, int* tps) {
  return ast_tile::split_tiles((int64_t)n * tiles_of(m), tiles_of(p), want, kTargetWGs, kMinSplitTiles, tps);
}

// The row sums' workspace: [S partials | E partials] per split (unused for one split: the sums go
// straight to the outputs)
struct RowWs {
  int splits, tiles_per_split;
  float *ps, *pe;
  int64_t bytes;
};

inline RowWs row_ws(void* base, int n, int m, int p, int want) {
  ast_ws::Walk wk(base);
  int tps = 0;
  const int s = splits_of(n, m, p, want, &tps);
  const int64_t row = (int64_t)4 * n * s * m;
  return {s, tps, wk.take<float>(row), wk.take<float>(row), wk.off};
}

// The column maxima's workspace: [partial values | partial indices | partial distances] per content tile
struct ColWs {
  float* pval;
  int* pidx;
  float* pdist;
  int64_t bytes;
};

inline ColWs col_ws(void* base, int n, int m, int p) {
  ast_ws::Walk wk(base);
  const int64_t col = (int64_t)4 * n * tiles_of(m) * p;
  return {wk.take<float>(col), wk.take<int>(col), wk.take<float>(col), wk.off};
}

// The whole loss's workspace: [the match's unused column minima | their indices | the stage in flight]
struct LossWs {
  float* cmin;
  int* cidx;
  void* stage;
  int64_t bytes;
};

inline LossWs loss_ws(void* base, int n, int ns, int m, int p) {
  ast_ws::Walk wk(base);
  const int64_t match = ast_cosine_match_workspace_bytes(n, ns, m, p, 0);
  const int64_t stage = std::max(std::max(match, row_ws(nullptr, n, m, p, 0).bytes), col_ws(nullptr, n, m, p).bytes);
  return {wk.take<float>((int64_t)4 * n * p), wk.take<int>((int64_t)4 * n * p), wk.take<void>(stage), wk.off};
}

// The backward's workspace: [start | cursor | list | row scalars | row flags | tile flags | G]
struct BwdWs {
  int *start, *cursor, *list;
  float* rs;
  int *act, *tact;
  float* G;
  int64_t bytes;
};

inline BwdWs bwd_ws(void* base, int n, int c, int m, int p) {
  ast_ws::Walk wk(base);
  return {wk.take<int>((int64_t)4 * n * (m + 1)), wk.take<int>((int64_t)4 * n * m), wk.take<int>((int64_t)4 * n * p),
          wk.take<float>((int64_t)12 * n * m), wk.take<int>((int64_t)4 * n * m),
          wk.take<int>((int64_t)4 * n * tiles_of(m)), wk.take<float>((int64_t)4 * n * c * m), wk.off};
}

int center_launch(const float* x, const float* y, float* mu, float* xc, float* yc, int n, int ns, int c, int m, int p,
                  hipStream_t st) {
  hipLaunchKernelGGL(cx_mean_kernel, dim3(c, ns), dim3(kT), 0, st, y, mu, c, p);
  hipLaunchKernelGGL(cx_sub_kernel, dim3((m + kT - 1) / kT, c, n), dim3(kT), 0, st, x, (const float*)mu, xc, c, m, ns);
  hipLaunchKernelGGL(cx_sub_kernel, dim3((p + kT - 1) / kT, c, ns), dim3(kT), 0, st, y, (const float*)mu, yc, c, p, ns);
  return (int)hipGetLastError();
}

int rowsum_launch(const float* x, const float* y, const float* u, const float* v, const float* rmin, float* S, float* E,
                  int n, int ns, int c, int m, int p, float h, int want, void* wsp, hipStream_t st) {
  const RowWs w = row_ws(wsp, n, m, p, want);
  float* ps = w.splits > 1 ? w.ps : S;
  float* pe = w.splits > 1 ? w.pe : E;
  hipLaunchKernelGGL(cx_pass_kernel<false>, dim3(tiles_of(m), w.splits, n), dim3(kT), 0, st, x, y, u, v, rmin,
                     (const float*)nullptr, ps, pe, (int*)nullptr, c, m, p, ns, w.tiles_per_split, h);
  if (w.splits > 1)
    hipLaunchKernelGGL(cx_rowmerge_kernel, dim3((m + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)ps,
                       (const float*)pe, S, E, m, w.splits);
  return (int)hipGetLastError();
}

int colmax_launch(const float* x, const float* y, const float* u, const float* v, const float* rmin, const float* S,
                  float* ccx, int* cidx, float* cdist, int n, int ns, int c, int m, int p, float h, int want, void* wsp,
                  hipStream_t st) {
  const ColWs w = col_ws(wsp, n, m, p);
  int tps = 0;
  const int splits = splits_of(n, m, p, want, &tps), ct = tiles_of(m);
  hipLaunchKernelGGL(cx_pass_kernel<true>, dim3(ct, splits, n), dim3(kT), 0, st, x, y, u, v, rmin, S, w.pval, w.pdist,
                     w.pidx, c, m, p, ns, tps, h);
  hipLaunchKernelGGL(cx_colmerge_kernel, dim3((p + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)w.pval,
                     (const int*)w.pidx, (const float*)w.pdist, ccx, cidx, cdist, p, ct);
  return (int)hipGetLastError();
}

// The dense pass of the backward: a workgroup takes as many blocks of CH channels as cover C, up to
// kDenseBlocks of them (32 accumulators per lane and block); past that the channel groups are grid
// entries and each recomputes the distance block.
template <int NB>
void dense_launch_nb(const float* xc, const float* yc, const float* u, const float* v, const float* rmin, const int* ridx,
                     const int* cidx, const float* rs, const int* act, const int* tact, float* G, int n, int ns, int c,
                     int m, int p, float h, hipStream_t st) {
  hipLaunchKernelGGL(cx_dense_kernel<NB>, dim3(tiles_of(m), (c + NB * CH - 1) / (NB * CH), n), dim3(kT), 0, st, xc, yc, u,
                     v, rmin, ridx, cidx, rs, act, tact, G, c, m, p, ns, h);
}

void dense_launch(const float* xc, const float* yc, const float* u, const float* v, const float* rmin, const int* ridx,
                  const int* cidx, const float* rs, const int* act, const int* tact, float* G, int n, int ns, int c,
                  int m, int p, float h, hipStream_t st) {
  const int nb = std::min((c + CH - 1) / CH, kDenseBlocks);
  (nb >= 4   ? dense_launch_nb<4>
   : nb == 3 ? dense_launch_nb<3>
   : nb == 2 ? dense_launch_nb<2>
             : dense_launch_nb<1>)(xc, yc, u, v, rmin, ridx, cidx, rs, act, tact, G, n, ns, c, m, p, h, st);
}

int value_launch(const float* ccx, float* cxb, float* loss, int n, int p, float weight, hipStream_t st) {
  hipLaunchKernelGGL(cx_sample_kernel, dim3(n), dim3(kT), 0, st, ccx, cxb, p);
  hipLaunchKernelGGL(cx_total_kernel, dim3(1), dim3(kT), 0, st, (const float*)cxb, loss, n, weight / (float)n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ast_cx_center_f32(const float* x, const float* y, float* mu, float* xc, float* yc, int n, int ns, int c, int m,
                      int p, void* stream) {
  if (!x || !y || !mu || !xc || !yc) return AST_E_NULLPTR;
  const int e = all_shape(n, ns, c, m, p);
  if (e) return e;
  return center_launch(x, y, mu, xc, yc, n, ns, c, m, p, (hipStream_t)stream);
}

long long ast_cx_rowsum_workspace_bytes(int n, int ns, int m, int p, int splits) {
  const int e = pair_shape(n, ns, m, p);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  return row_ws(nullptr, n, m, p, splits).bytes;
}

int ast_cx_rowsum_f32(const float* xc, const float* yc, const float* inv_x, const float* inv_y, const float* row_min,
                      float* row_sum, float* row_dsum, int n, int ns, int c, int m, int p, float h, int splits,
                      void* workspace, long long workspace_bytes, void* stream) {
  if (!xc || !yc || !inv_x || !inv_y || !row_min || !row_sum || !row_dsum || !workspace) return AST_E_NULLPTR;
  const int e = all_shape(n, ns, c, m, p);
  if (e) return e;
  if (splits < 0 || bad_h(h)) return AST_E_UNSUPPORTED;
  if (workspace_bytes < row_ws(nullptr, n, m, p, splits).bytes) return AST_E_SHAPE;
  return rowsum_launch(xc, yc, inv_x, inv_y, row_min, row_sum, row_dsum, n, ns, c, m, p, h, splits, workspace,
                       (hipStream_t)stream);
}

long long ast_cx_colmax_workspace_bytes(int n, int ns, int m, int p) {
  const int e = pair_shape(n, ns, m, p);
  return e ? e : col_ws(nullptr, n, m, p).bytes;
}

int ast_cx_colmax_f32(const float* xc, const float* yc, const float* inv_x, const float* inv_y, const float* row_min,
                      const float* row_sum, float* col_cx, int* col_index, float* col_dist, int n, int ns, int c, int m,
                      int p, float h, int splits, void* workspace, long long workspace_bytes, void* stream) {
  if (!xc || !yc || !inv_x || !inv_y || !row_min || !row_sum || !col_cx || !col_index || !col_dist || !workspace)
    return AST_E_NULLPTR;
  const int e = all_shape(n, ns, c, m, p);
  if (e) return e;
  if (splits < 0 || bad_h(h)) return AST_E_UNSUPPORTED;
  if (workspace_bytes < col_ws(nullptr, n, m, p).bytes) return AST_E_SHAPE;
  return colmax_launch(xc, yc, inv_x, inv_y, row_min, row_sum, col_cx, col_index, col_dist, n, ns, c, m, p, h, splits,
                       workspace, (hipStream_t)stream);
}

int ast_cx_value_f32(const float* col_cx, float* sample_cx, float* loss, int n, int p, float weight, void* stream) {
  if (!col_cx || !sample_cx || !loss) return AST_E_NULLPTR;
  const int e = map_shape(n, p);
  if (e) return e;
  return value_launch(col_cx, sample_cx, loss, n, p, weight, (hipStream_t)stream);
}

long long ast_cx_loss_workspace_bytes(int n, int ns, int m, int p) {
  const int e = pair_shape(n, ns, m, p);
  return e ? e : loss_ws(nullptr, n, ns, m, p).bytes;
}

int ast_cx_loss_f32(const float* x, const float* y, float* mu, float* xc, float* yc, float* inv_x, float* inv_y,
                    float* row_min, int* row_index, float* row_sum, float* row_dsum, float* col_cx, int* col_index,
                    float* col_dist, float* sample_cx, float* loss, int n, int ns, int c, int m, int p, float weight,
                    float h, int center, void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !y || !inv_x || !inv_y || !row_min || !row_index || !row_sum || !row_dsum || !col_cx || !col_index ||
      !col_dist || !sample_cx || !loss || !workspace)
    return AST_E_NULLPTR;
  if (center && (!mu || !xc || !yc)) return AST_E_NULLPTR;
  int e = all_shape(n, ns, c, m, p);
  if (e) return e;
  if (bad_h(h)) return AST_E_UNSUPPORTED;
  const LossWs w = loss_ws(workspace, n, ns, m, p);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const float *xs = x, *ys = y;
  if (center) {
    e = center_launch(x, y, mu, xc, yc, n, ns, c, m, p, st);
    if (e) return e;
    xs = xc;
    ys = yc;
  }
  e = ast_cosine_norms_f32(xs, inv_x, n, c, m, stream);
  if (e) return e;
  e = ast_cosine_norms_f32(ys, inv_y, ns, c, p, stream);
  if (e) return e;
  const long long match = ast_cosine_match_workspace_bytes(n, ns, m, p, 0);
  e = ast_cosine_match_f32(xs, ys, inv_x, inv_y, row_min, row_index, w.cmin, w.cidx, n, ns, c, m, p, 0, w.stage, match,
                           stream);
  if (e) return e;
  e = rowsum_launch(xs, ys, inv_x, inv_y, row_min, row_sum, row_dsum, n, ns, c, m, p, h, 0, w.stage, st);
  if (e) return e;
  e = colmax_launch(xs, ys, inv_x, inv_y, row_min, row_sum, col_cx, col_index, col_dist, n, ns, c, m, p, h, 0, w.stage,
                    st);
  if (e) return e;
  return value_launch(col_cx, sample_cx, loss, n, p, weight, st);
}

long long ast_cx_loss_backward_workspace_bytes(int n, int c, int m, int p) {
  const int e = all_shape(n, n, c, m, p);
  return e ? e : bwd_ws(nullptr, n, c, m, p).bytes;
}

int ast_cx_loss_backward_f32(const float* xc, const float* yc, const float* inv_x, const float* inv_y,
                             const float* row_min, const int* row_index, const float* row_sum, const float* row_dsum,
                             const int* col_index, const float* col_dist, const float* sample_cx,
                             const float* grad_scale, float* dx, int n, int ns, int c, int m, int p, float weight,
                             float h, void* workspace, long long workspace_bytes, void* stream) {
  if (!xc || !yc || !inv_x || !inv_y || !row_min || !row_index || !row_sum || !row_dsum || !col_index || !col_dist ||
      !sample_cx || !grad_scale || !dx || !workspace)
    return AST_E_NULLPTR;
  const int e = all_shape(n, ns, c, m, p);
  if (e) return e;
  if (bad_h(h)) return AST_E_UNSUPPORTED;
  const BwdWs w = bwd_ws(workspace, n, c, m, p);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int ct = tiles_of(m);
  hipLaunchKernelGGL(cx_invert_kernel, dim3(n), dim3(kT), 0, st, col_index, w.start, w.cursor, w.list, m, p);
  hipLaunchKernelGGL(cx_rows_kernel, dim3((m + kT - 1) / kT, n), dim3(kT), 0, st, inv_x, row_min, row_sum, row_dsum,
                     col_dist, (const int*)w.start, (const int*)w.list, w.rs, w.act, w.tact, m, p, ct, h);
  dense_launch(xc, yc, inv_x, inv_y, row_min, row_index, col_index, w.rs, w.act, w.tact, w.G, n, ns, c, m, p, h, st);
  hipLaunchKernelGGL(cx_finish_kernel, dim3((m + 63) / 64, n), dim3(kT), 0, st, xc, inv_x, (const float*)w.G,
                     (const int*)w.act, sample_cx, grad_scale, dx, c, m, weight / ((float)n * (float)p));
  return (int)hipGetLastError();
}

}  // extern "C"
