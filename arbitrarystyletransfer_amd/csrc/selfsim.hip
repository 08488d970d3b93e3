// Self-similarity content loss (Kolkin et al., STROTSS, CVPR 2019) for gfx950, fp32 storage, exact:
// every pixel pair of both maps takes part, nothing is sampled. The definition is in include/ast_hip.h;
// tests/selfsim_ref.py restates it. Inputs: x [n, C, N pixels], the stylised map and the differentiable
// side, and c, the content map of the same shape, both dense NCHW with the spatial sides flattened.
//   u_i = 1 / ||f_i|| (ast_cosine_norms_f32 of remd.hip, unchanged), for either map f
//   D_f(i, j) = 1 - <f_i, f_j> (u_i u_j) for i != j, 0 on the diagonal
//   r_f(j) = sum_i D_f(i, j),  q_f(j) = 1 / r_f(j) when that is positive and finite, else 0
//   e(i, j) = D_x(i, j) q_x(j) - D_c(i, j) q_c(j),  s = sign(e) (0 for 0, NaN and the diagonal)
//   L_b = (1 / N) sum_{i != j} |e(i, j)|,  L = weight / n * sum_b L_b
//   t(j) = q_x(j) sum_{k != j} s(k, j) D_x(k, j)
// Stages, each a C-ABI entry of its own; ast_selfsim_loss_f32 is exactly norms, norms, colsum, colsum,
// pairs, total:
//   colsum  r_f(j) = (N - 1) - (<fh_j, S> - ||fh_j||^2) with S = sum_i fh_i: one launch sums every channel
//           over the pixels in a fixed order, one walks the pixels. O(N C): no pass over pairs.
//   pairs   one workgroup per upper-triangle pair (I <= J) of 64-pixel tiles: the implicit GEMM of
//           remd.hip's match (v_mfma_f32_32x32x2_f32, both operands straight from NCHW, the next chunk's
//           buffer loads in flight while this one is multiplied) with two K = C products, x_I . x_J and
//           c_I . c_J. The 64 x 64 block of distances serves e(i, j), the tile's columns normalised (the
//           column role), and e(j, i), its rows normalised (the row role); a diagonal tile pair has the
//           column role alone and masks i = j. |e| goes into one partial per tile pair; the signed sums
//           of t into one partial per (other tile, pixel): slot (I, p in J) in the column role, slot
//           (J, p in I) in the row role, every slot written exactly once and merged in tile order by a
//           second launch; the signs into two bit planes, 32-bit halves of the int64 words written by
//           the wave that holds them. A third launch sums a sample's partials in pair order.
//   total   a one-workgroup launch adds weight / n * sum_b L_b, in sample order, into a loss accumulator.
// Backward (to x only): a second GEMM that recomputes no cosine. A workgroup owns 64 rows m and 128
// channels and walks the tiles J in ascending order: W(m, j) u_j is built in LDS from q_x, t and the
// two planes -- word (m, J) for s(m, j), the words (j, M) of tile J's rows, staged in LDS, for s(j, m)
// -- and multiplied on the MFMA by the raw x tile, G[m, ch] = sum_j W'(m, j) x[ch, j]. G goes to the
// workspace; a finishing pass takes <xh_m, G_m> over all channels and writes every element of dx once.
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
constexpr int KC = 64;      // channels per staged chunk of the pairs kernel
constexpr int RT = KC / 4;  // channel runs per wave and chunk
constexpr int kMaxC = AST_REMD_MAX_C;
constexpr int kMaxPixels = AST_SELFSIM_MAX_PIXELS;  // 4 * KC * pixels stays far below 2^31: the buffer offsets are int32
constexpr int CH = 128;     // channels per workgroup of the backward GEMM: 32 accumulators per lane
constexpr int XP = MT + 1;  // padded row of the backward's x tile in LDS

__device__ __forceinline__ float inv_colsum(float r) { return (r > 0.f && r < INFINITY) ? 1.0f / r : 0.f; }

// ------------------------------------------------------------------------------------------------
// Column sums
// ------------------------------------------------------------------------------------------------

// grid (channels, samples): S[b, ch] = sum_p u_p x[ch, p]; thread t sums pixels t, t + 256, ... in order,
// then order A of wave.h.
__global__ __launch_bounds__(kT) void selfsim_chsum_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                          float* __restrict__ S, int C, int N) {
  __shared__ float sh[kT / 64];
  const int ch = blockIdx.x, b = blockIdx.y;
  const float* X = x + ((int64_t)b * C + ch) * N;
  const float* U = u + (int64_t)b * N;
  float s = 0.f;
  for (int p = threadIdx.x; p < N; p += kT) s = fmaf(U[p], X[p], s);
  const float t = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) S[(int64_t)b * C + ch] = t;
}

// grid (pixels / 64, samples); thread (p, g) takes channels g, g + 4, ...; the four partials are added in
// g order. One pixel: <fh, S> and ||fh||^2 are the same chain, r is exactly 0.
__global__ __launch_bounds__(kT) void selfsim_colsum_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                           const float* __restrict__ S, float* __restrict__ rsum,
                                                           int C, int N) {
  __shared__ float shd[4][64];
  __shared__ float shq[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, p = blockIdx.x * 64 + lane, b = blockIdx.y;
  const float* X = x + (int64_t)b * C * N;
  const float* Sb = S + (int64_t)b * C;
  float d = 0.f, q = 0.f;
  if (p < N) {
    const float up = u[(int64_t)b * N + p];
    for (int ch = g; ch < C; ch += 4) {
      const float v = up * X[(int64_t)ch * N + p];
      d = fmaf(v, Sb[ch], d);
      q = fmaf(v, v, q);
    }
  }
  shd[g][lane] = d;
  shq[g][lane] = q;
  __syncthreads();
  if (g == 0 && p < N) {
    const float dot = quarter_sum(shd, lane);
    const float sq = quarter_sum(shq, lane);
    rsum[(int64_t)b * N + p] = (float)(N - 1) - (dot - sq);
  }
}

// ------------------------------------------------------------------------------------------------
// Pairs
// ------------------------------------------------------------------------------------------------

// stage_load / stage_store (match_tile.h): a chunk of KC channels x 64 pixels into registers, then LDS. A
// pixel past the map reads the next channel's first pixels; such a row or column of the tile is masked.

// the first pair of tile row I in the list (0, 0), (0, 1), ..., (0, T - 1), (1, 1), ...
__device__ __host__ inline int tri_start(int I, int T) { return I * T - I * (I - 1) / 2; }

// grid (tile pairs, samples). lpart [n, pairs]; tpart [n, T, N]; pos, neg: the int64 planes [n, N, T] as
// 32-bit halves. Two workgroups per CU (64 KiB of LDS each): one multiplies while the other loads or folds.
__global__ __launch_bounds__(kT, 2) void selfsim_pairs_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                          const float* __restrict__ ux, const float* __restrict__ uc,
                                                          const float* __restrict__ rx, const float* __restrict__ rc,
                                                          float* __restrict__ lpart, float* __restrict__ tpart,
                                                          uint32_t* __restrict__ pos, uint32_t* __restrict__ neg, int C,
                                                          int N, int T) {
  __shared__ float S[4 * KC * MT];
  float* XI = S;
  float* XJ = S + KC * MT;
  float* CI = S + 2 * KC * MT;
  float* CJ = S + 3 * KC * MT;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave & 1, wn = wave >> 1;
  const int b = blockIdx.y, pair = blockIdx.x;
  int I = (int)(0.5f * ((float)(2 * T + 1) - sqrtf((float)((2 * T + 1) * (2 * T + 1) - 8 * pair))));
  I = min(max(I, 0), T - 1);
  while (I + 1 < T && tri_start(I + 1, T) <= pair) ++I;
  while (I > 0 && tri_start(I, T) > pair) --I;
  I = __builtin_amdgcn_readfirstlane(I);
  const int J = I + pair - tri_start(I, T);
  const bool diag = I == J;
  const int i0 = I * MT, j0 = J * MT;
  const float* Xb = x + (int64_t)b * C * N;
  const float* Cb = c + (int64_t)b * C * N;
  const int ao = h * MT + wm * 32 + r, bo = h * MT + wn * 32 + r;

  float xa[RT], xb[RT], ca[RT], cb[RT];
  stage_load(xa, Xb, C, N, i0, wave, lane);
  stage_load(xb, Xb, C, N, j0, wave, lane);
  stage_load(ca, Cb, C, N, i0, wave, lane);
  stage_load(cb, Cb, C, N, j0, wave, lane);
  f32x16 ax = (f32x16){0.f}, ac = (f32x16){0.f};
  // every branch that encloses a barrier depends on block indices and kernel arguments alone
  for (int c0 = 0; c0 < C; c0 += KC) {
    stage_store(xa, XI, wave, lane);
    stage_store(xb, XJ, wave, lane);
    stage_store(ca, CI, wave, lane);
    stage_store(cb, CJ, wave, lane);
    __syncthreads();
    const int nc0 = c0 + KC;
    if (nc0 < C) {  // the next chunk is in flight while this one is multiplied
      stage_load(xa, Xb + (int64_t)nc0 * N, C - nc0, N, i0, wave, lane);
      stage_load(xb, Xb + (int64_t)nc0 * N, C - nc0, N, j0, wave, lane);
      stage_load(ca, Cb + (int64_t)nc0 * N, C - nc0, N, i0, wave, lane);
      stage_load(cb, Cb + (int64_t)nc0 * N, C - nc0, N, j0, wave, lane);
    }
    __builtin_amdgcn_sched_barrier(0);  // the loads are issued here, ahead of the products
    // k order of every inner product: ascending channel pairs; lane half h takes the pair's channel h
#pragma unroll
    for (int cp = 0; cp < KC / 2; ++cp) {
      ax = __builtin_amdgcn_mfma_f32_32x32x2f32(XI[2 * cp * MT + ao], XJ[2 * cp * MT + bo], ax, 0, 0, 0);
      ac = __builtin_amdgcn_mfma_f32_32x32x2f32(CI[2 * cp * MT + ao], CJ[2 * cp * MT + bo], ac, 0, 0, 0);
    }
    __syncthreads();
  }

  // S is free after the loop's last barrier: the tiles' vectors, then the scratch of the reductions
  float* vI = S;            // [4][64]: u_x, u_c, q_x, q_c of tile I's pixels
  float* vJ = S + 4 * MT;   // the same of tile J's
  float* shs = S + 8 * MT;  // block_sum
  float* colred = shs + 64;     // [2 wn][32]: the column sums of the wm = 1 waves
  float* rowred = colred + 64;  // [2 wm][32]: the row sums of the wn = 1 waves
  if (tid < 2 * MT) {
    const int l = tid & 63, p = (tid < MT ? i0 : j0) + l;
    float* v = tid < MT ? vI : vJ;
    const bool ok = p < N;
    const int64_t o = (int64_t)b * N + p;
    v[l] = ok ? ux[o] : 0.f;
    v[MT + l] = ok ? uc[o] : 0.f;
    v[2 * MT + l] = ok ? inv_colsum(rx[o]) : 0.f;
    v[3 * MT + l] = ok ? inv_colsum(rc[o]) : 0.f;
  }
  __syncthreads();

  const int jl = wn * 32 + r, j = j0 + jl;
  const bool jvalid = j < N;
  const float uxj = vJ[jl], ucj = vJ[MT + jl], qxj = vJ[2 * MT + jl], qcj = vJ[3 * MT + jl];
  // the lane of the wave's first half that stores local row `lane` of the column role's plane words
  const int kL = (lane & 3) + 4 * ((lane >> 3) & 3), hL = (lane >> 2) & 1;
  float lsum = 0.f, tcol = 0.f, trow[16];
  uint32_t pcol = 0, ncol = 0, prow = 0, nrow = 0;
  {
    // x == c must give e == 0 exactly: the two products round on their own, no fused multiply-add
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int il = wm * 32 + acc_row(k, h), i = i0 + il;
      const float dx = 1.0f - ax[k] * (vI[il] * uxj);
      const float dc = 1.0f - ac[k] * (vI[MT + il] * ucj);
      const bool ok = jvalid && i < N && i != j;
      // column role: e(i, j), column j of tile J
      const float e1 = dx * qxj - dc * qcj;
      const bool p1 = ok && e1 > 0.f, n1 = ok && e1 < 0.f;
      lsum += ok ? fabsf(e1) : 0.f;
      tcol += p1 ? dx : n1 ? -dx : 0.f;
      // the ballot's low half: row acc_row(k, 0) over the wave's 32 columns; its high half: row acc_row(k, 1)
      const uint64_t bp = __ballot(p1), bn = __ballot(n1);
      if (kL == k) {
        pcol = hL ? (uint32_t)(bp >> 32) : (uint32_t)bp;
        ncol = hL ? (uint32_t)(bn >> 32) : (uint32_t)bn;
      }
      trow[k] = 0.f;
      if (!diag) {  // row role: e(j, i), column i of tile I
        const float e2 = dx * vI[2 * MT + il] - dc * vI[3 * MT + il];
        const bool p2 = ok && e2 > 0.f, n2 = ok && e2 < 0.f;
        lsum += ok ? fabsf(e2) : 0.f;
        trow[k] = p2 ? dx : n2 ? -dx : 0.f;
        prow |= (uint32_t)p2 << acc_row(k, h);
        nrow |= (uint32_t)n2 << acc_row(k, h);
      }
    }
  }

  const float tot = block_sum<kT / 64>(lsum, shs);
  if (tid == 0) lpart[(int64_t)b * gridDim.x + pair] = tot;

  // column role: the other lane half holds the rows in between, the wm = 1 wave the 32 rows after
  tcol += __shfl_xor(tcol, 32, 64);
  if (wm == 1 && h == 0) colred[jl] = tcol;
  if (!diag) {
    // row role: the 32 lanes of a half hold the same 16 rows over different columns
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float v = trow[k];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      trow[k] = v;
    }
    if (wn == 1 && r == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) rowred[wm * 32 + acc_row(k, h)] = trow[k];
    }
    prow |= __shfl_xor(prow, 32, 64);
    nrow |= __shfl_xor(nrow, 32, 64);
  }
  __syncthreads();
  if (wm == 0 && h == 0 && jvalid) tpart[((int64_t)b * T + I) * N + j] = tcol + colred[jl];
  if (lane < 32) {
    const int i = i0 + wm * 32 + lane;
    if (i < N) {
      const int64_t o = (((int64_t)b * N + i) * T + J) * 2 + wn;
      pos[o] = pcol;
      neg[o] = ncol;
    }
  }
  if (!diag) {
    if (wn == 0 && r == 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int il = wm * 32 + acc_row(k, h), i = i0 + il;
        if (i < N) tpart[((int64_t)b * T + J) * N + i] = trow[k] + rowred[il];
      }
    }
    if (h == 0 && jvalid) {
      const int64_t o = (((int64_t)b * N + j) * T + I) * 2 + wm;
      pos[o] = prow;
      neg[o] = nrow;
    }
  }
}

// grid (pixels / 256, samples): t[b, p] = q_x(p) * the partials of p in ascending tile order
__global__ __launch_bounds__(kT) void selfsim_tmerge_kernel(const float* __restrict__ tpart, const float* __restrict__ rx,
                                                           float* __restrict__ t, int N, int T) {
  const int p = blockIdx.x * kT + threadIdx.x, b = blockIdx.y;
  if (p >= N) return;
  float s = 0.f;
  for (int k = 0; k < T; ++k) s += tpart[((int64_t)b * T + k) * N + p];
  t[(int64_t)b * N + p] = inv_colsum(rx[(int64_t)b * N + p]) * s;
}

// grid (samples): sums[b] = (the sample's tile-pair partials in pair order per thread, then order A) / N
__global__ __launch_bounds__(kT) void selfsim_sums_kernel(const float* __restrict__ lpart, float* __restrict__ sums,
                                                         int pairs, int N) {
  __shared__ float sh[kT / 64];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < pairs; k += kT) s += lpart[(int64_t)b * pairs + k];
  const float t = block_sum<kT / 64>(s, sh);
  if (threadIdx.x == 0) sums[b] = t / (float)N;
}

// one workgroup: *loss += w_over_n * sum over the samples, in sample order per thread
__global__ __launch_bounds__(kT) void selfsim_total_kernel(const float* __restrict__ sums, float* loss, int n,
                                                          float w_over_n) {
  __shared__ float sh[kT / 64];
  float s = 0.f;
  for (int b = threadIdx.x; b < n; b += kT) s += sums[b];
  const float t = block_sum<kT / 64>(s, sh);
  ast_det::loss_acc_commit(loss, w_over_n * t);
}

// ------------------------------------------------------------------------------------------------
// Backward
// ------------------------------------------------------------------------------------------------

// grid (tiles, channels / CH, samples): G[b, ch, m] = sum_{j != m} W(m, j) u_j x[b, ch, j],
//   W(m, j) = (s(m, j) - t_j) q_j + (s(j, m) - t_m) q_m,
// the tiles J in ascending order, inside a tile ascending j pairs on the MFMA. Wave w builds the 16
// columns j = 16 w .. 16 w + 15 of W' (lane = row m), then multiplies channels 32 w .. 32 w + 31.
__global__ __launch_bounds__(kT) void selfsim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ ux,
                                                        const float* __restrict__ rx, const float* __restrict__ t,
                                                        const uint64_t* __restrict__ pos,
                                                        const uint64_t* __restrict__ neg, float* __restrict__ G, int C,
                                                        int N, int T) {
  __shared__ float Xs[CH * XP];   // [channel][j], a row padded to 65
  __shared__ float Ws[MT * MT];   // [j][m]
  __shared__ uint64_t wp[MT], wq[MT];  // the words (j, M) of tile J's rows: bit m - m0 is s(j, m)
  __shared__ float vt[MT], vq[MT], vu[MT];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Mt = blockIdx.x, m0 = Mt * MT, ch0 = blockIdx.y * CH, b = blockIdx.z;
  const int m = m0 + lane;
  const bool mvalid = m < N;
  const int64_t bn = (int64_t)b * N;
  const float tm = mvalid ? t[bn + m] : 0.f, qm = mvalid ? inv_colsum(rx[bn + m]) : 0.f;
  const float* Xb = x + (int64_t)b * C * N;

  float xr[CH / 4];
#pragma unroll
  for (int k = 0; k < CH / 4; ++k) {
    const int ch = ch0 + wave + 4 * k;
    xr[k] = (ch < C && lane < N) ? Xb[(int64_t)ch * N + lane] : 0.f;
  }
  f32x16 acc0 = (f32x16){0.f}, acc1 = (f32x16){0.f};
  for (int J = 0; J < T; ++J) {
    const int j0 = J * MT;
#pragma unroll
    for (int k = 0; k < CH / 4; ++k) Xs[(wave + 4 * k) * XP + lane] = xr[k];
    if (tid < MT) {
      const int j = j0 + tid;
      const bool ok = j < N;
      vt[tid] = ok ? t[bn + j] : 0.f;
      vq[tid] = ok ? inv_colsum(rx[bn + j]) : 0.f;
      vu[tid] = ok ? ux[bn + j] : 0.f;
      wp[tid] = ok ? pos[(bn + j) * T + Mt] : 0;
      wq[tid] = ok ? neg[(bn + j) * T + Mt] : 0;
    }
    const uint64_t pm = mvalid ? pos[(bn + m) * T + J] : 0, nm = mvalid ? neg[(bn + m) * T + J] : 0;
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int jl = wave * 16 + jj, j = j0 + jl;
      const float s1 = (float)((int)((pm >> jl) & 1) - (int)((nm >> jl) & 1));
      const float s2 = (float)((int)((wp[jl] >> lane) & 1) - (int)((wq[jl] >> lane) & 1));
      const float w = (s1 - vt[jl]) * vq[jl] + (s2 - tm) * qm;
      Ws[jl * MT + lane] = (j < N && j != m) ? w * vu[jl] : 0.f;
    }
    if (J + 1 < T) {  // the next x tile is in flight while this one is multiplied
#pragma unroll
      for (int k = 0; k < CH / 4; ++k) {
        const int ch = ch0 + wave + 4 * k, j = j0 + MT + lane;
        xr[k] = (ch < C && j < N) ? Xb[(int64_t)ch * N + j] : 0.f;
      }
    }
    __syncthreads();
    const float* Br = Xs + (wave * 32 + r) * XP + h;
    const float* Ar = Ws + h * MT + r;
#pragma unroll
    for (int kp = 0; kp < MT / 2; ++kp) {
      const float bv = Br[2 * kp];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ar[2 * kp * MT], bv, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ar[2 * kp * MT + 32], bv, acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  const int ch = ch0 + wave * 32 + r;
  if (ch < C) {
    float* Gc = G + ((int64_t)b * C + ch) * N;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int ma = m0 + acc_row(k, h), mb = ma + 32;
      if (ma < N) Gc[ma] = acc0[k];
      if (mb < N) Gc[mb] = acc1[k];
    }
  }
}

// grid (pixels / 64, samples): with k = -(g w / (n N)), dxh_m = k G_m,
//   dx_m = u_m (dxh_m - xh_m <xh_m, dxh_m>) = u_m k (G_m - xh_m <xh_m, G_m>), 0 where u_m = 0;
// thread (p, g) takes channels g, g + 4, ...; the four partials of the inner product are added in g order.
__global__ __launch_bounds__(kT) void selfsim_finish_kernel(const float* __restrict__ x, const float* __restrict__ ux,
                                                           const float* __restrict__ G, const float* __restrict__ g,
                                                           float* __restrict__ dx, int C, int N, float w_over_nn) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.x * 64 + lane, b = blockIdx.y;
  const int64_t base = (int64_t)b * C * N + p;
  const float up = p < N ? ux[(int64_t)b * N + p] : 0.f;
  float d = 0.f;
  if (p < N)
    for (int ch = q; ch < C; ch += 4) d = fmaf(up * x[base + (int64_t)ch * N], G[base + (int64_t)ch * N], d);
  sh[q][lane] = d;
  __syncthreads();
  if (p >= N) return;
  const float dot = quarter_sum(sh, lane);
  const float k = -(g[0] * w_over_nn) * up;
  for (int ch = q; ch < C; ch += 4) {
    const int64_t o = base + (int64_t)ch * N;
    dx[o] = up == 0.f ? 0.f : k * (G[o] - (up * x[o]) * dot);
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layouts, launch sequences
// ------------------------------------------------------------------------------------------------

using ast_tile::tiles_of;
inline int pairs_of(int pixels) { return tiles_of(pixels) * (tiles_of(pixels) + 1) / 2; }

inline int map_shape(int n, int pixels) { return ast_tile::map_shape(n, pixels, kMaxPixels); }
inline int chan_shape(int c) { return ast_tile::chan_shape(c, kMaxC); }
inline int all_shape(int n, int c, int pixels) {
  const int e = map_shape(n, pixels);
  return e ? e : chan_shape(c);
}

// A workspace of one region is its size: the column sums' [channel sums] and the backward's [G]
inline int64_t colsum_ws(int n, int c) { return ast_ws::al256((int64_t)4 * n * c); }
inline int64_t bwd_ws(int n, int c, int pixels) { return ast_ws::al256((int64_t)4 * n * c * pixels); }

// The pairs' workspace: [t partials | loss partials]
struct PairsWs {
  float *tpart, *lpart;
  int64_t bytes;
};

inline PairsWs pairs_ws(void* base, int n, int pixels) {
  ast_ws::Walk wk(base);
  return {wk.take<float>((int64_t)4 * n * tiles_of(pixels) * pixels), wk.take<float>((int64_t)4 * n * pairs_of(pixels)),
          wk.off};
}

// The whole loss's workspace: [the column sums' | the pairs']
struct LossWs {
  float* S;
  void* pairs;
  int64_t bytes;
};

inline LossWs loss_ws(void* base, int n, int c, int pixels) {
  ast_ws::Walk wk(base);
  return {wk.take<float>(colsum_ws(n, c)), wk.take<void>(pairs_ws(nullptr, n, pixels).bytes), wk.off};
}

int colsum_launch(const float* x, const float* u, float* r, int n, int c, int pixels, float* S, hipStream_t st) {
  hipLaunchKernelGGL(selfsim_chsum_kernel, dim3(c, n), dim3(kT), 0, st, x, u, S, c, pixels);
  hipLaunchKernelGGL(selfsim_colsum_kernel, dim3((pixels + 63) / 64, n), dim3(kT), 0, st, x, u, (const float*)S, r, c,
                     pixels);
  return (int)hipGetLastError();
}

int pairs_launch(const float* x, const float* c, const float* ux, const float* uc, const float* rx, const float* rc,
                 float* sums, float* t, long long* pos, long long* neg, int n, int ch, int pixels, void* wsp,
                 hipStream_t st) {
  const int T = tiles_of(pixels), pairs = pairs_of(pixels);
  const PairsWs w = pairs_ws(wsp, n, pixels);
  float *tpart = w.tpart, *lpart = w.lpart;
  hipLaunchKernelGGL(selfsim_pairs_kernel, dim3(pairs, n), dim3(kT), 0, st, x, c, ux, uc, rx, rc, lpart, tpart,
                     (uint32_t*)pos, (uint32_t*)neg, ch, pixels, T);
  hipLaunchKernelGGL(selfsim_tmerge_kernel, dim3((pixels + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)tpart, rx, t,
                     pixels, T);
  hipLaunchKernelGGL(selfsim_sums_kernel, dim3(n), dim3(kT), 0, st, (const float*)lpart, sums, pairs, pixels);
  return (int)hipGetLastError();
}

int total_launch(const float* sums, float* loss, int n, float weight, hipStream_t st) {
  hipLaunchKernelGGL(selfsim_total_kernel, dim3(1), dim3(kT), 0, st, sums, loss, n, weight / (float)n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

long long ast_selfsim_colsum_workspace_bytes(int n, int c) {
  if (n <= 0 || n > 65535) return AST_E_SHAPE;
  const int e = chan_shape(c);
  return e ? e : colsum_ws(n, c);
}

int ast_selfsim_colsum_f32(const float* x, const float* inv_norm, float* col_sum, int n, int c, int pixels,
                           void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !inv_norm || !col_sum || !workspace) return AST_E_NULLPTR;
  const int e = all_shape(n, c, pixels);
  if (e) return e;
  if (workspace_bytes < colsum_ws(n, c)) return AST_E_SHAPE;
  return colsum_launch(x, inv_norm, col_sum, n, c, pixels, (float*)workspace, (hipStream_t)stream);
}

long long ast_selfsim_pairs_workspace_bytes(int n, int pixels) {
  const int e = map_shape(n, pixels);
  return e ? e : pairs_ws(nullptr, n, pixels).bytes;
}

int ast_selfsim_pairs_f32(const float* x, const float* c, const float* inv_x, const float* inv_c, const float* r_x,
                          const float* r_c, float* sums, float* t, long long* pos, long long* neg, int n, int ch,
                          int pixels, void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !c || !inv_x || !inv_c || !r_x || !r_c || !sums || !t || !pos || !neg || !workspace) return AST_E_NULLPTR;
  const int e = all_shape(n, ch, pixels);
  if (e) return e;
  if (workspace_bytes < pairs_ws(nullptr, n, pixels).bytes) return AST_E_SHAPE;
  return pairs_launch(x, c, inv_x, inv_c, r_x, r_c, sums, t, pos, neg, n, ch, pixels, workspace, (hipStream_t)stream);
}

int ast_selfsim_total_f32(const float* sums, float* loss, int n, float weight, void* stream) {
  if (!sums || !loss) return AST_E_NULLPTR;
  if (n <= 0 || n > 65535) return AST_E_SHAPE;
  return total_launch(sums, loss, n, weight, (hipStream_t)stream);
}

long long ast_selfsim_loss_workspace_bytes(int n, int c, int pixels) {
  const int e = all_shape(n, c, pixels);
  return e ? e : loss_ws(nullptr, n, c, pixels).bytes;
}

int ast_selfsim_loss_f32(const float* x, const float* c, float* inv_x, float* inv_c, float* r_x, float* r_c, float* t,
                         long long* pos, long long* neg, float* sums, float* loss, int n, int ch, int pixels,
                         float weight, void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !c || !inv_x || !inv_c || !r_x || !r_c || !t || !pos || !neg || !sums || !loss || !workspace)
    return AST_E_NULLPTR;
  int e = all_shape(n, ch, pixels);
  if (e) return e;
  const LossWs w = loss_ws(workspace, n, ch, pixels);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  e = ast_cosine_norms_f32(x, inv_x, n, ch, pixels, stream);
  if (e) return e;
  e = ast_cosine_norms_f32(c, inv_c, n, ch, pixels, stream);
  if (e) return e;
  e = colsum_launch(x, inv_x, r_x, n, ch, pixels, w.S, st);
  if (e) return e;
  e = colsum_launch(c, inv_c, r_c, n, ch, pixels, w.S, st);
  if (e) return e;
  e = pairs_launch(x, c, inv_x, inv_c, r_x, r_c, sums, t, pos, neg, n, ch, pixels, w.pairs, st);
  if (e) return e;
  return total_launch(sums, loss, n, weight, st);
}

long long ast_selfsim_loss_backward_workspace_bytes(int n, int c, int pixels) {
  const int e = all_shape(n, c, pixels);
  return e ? e : bwd_ws(n, c, pixels);
}

int ast_selfsim_loss_backward_f32(const float* x, const float* inv_x, const float* r_x, const float* t,
                                  const long long* pos, const long long* neg, const float* grad_scale, float* dx, int n,
                                  int c, int pixels, float weight, void* workspace, long long workspace_bytes,
                                  void* stream) {
  if (!x || !inv_x || !r_x || !t || !pos || !neg || !grad_scale || !dx || !workspace) return AST_E_NULLPTR;
  const int e = all_shape(n, c, pixels);
  if (e) return e;
  if (workspace_bytes < bwd_ws(n, c, pixels)) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  float* G = (float*)workspace;
  const int T = tiles_of(pixels);
  hipLaunchKernelGGL(selfsim_bwd_kernel, dim3(T, (c + CH - 1) / CH, n), dim3(kT), 0, st, x, inv_x, r_x, t,
                     (const uint64_t*)pos, (const uint64_t*)neg, G, c, pixels, T);
  hipLaunchKernelGGL(selfsim_finish_kernel, dim3((pixels + 63) / 64, n), dim3(kT), 0, st, x, inv_x, (const float*)G,
                     grad_scale, dx, c, pixels, weight / ((float)n * (float)pixels));
  return (int)hipGetLastError();
}

}  // extern "C"
