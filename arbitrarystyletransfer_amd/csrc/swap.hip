// Style swap (Chen & Schmidt 2016; the "style decorator" of Avatar-Net, Sheng et al. CVPR 2018, on
// normalised keys) for gfx950, fp32 storage: every 3x3 patch of the content map is replaced by the most
// similar patch of the style map and the overlaps are averaged. The definition is in
// include/ast_hip.h; tests/swap_ref.py restates it. Inputs: content key ck [n, C, H, W], style key sk
// and style value sv [ns, C, Hs, Ws] (ns = n, or 1 for a style shared by the batch), content c
// [n, C, H, W]; content patch i = y (W - 2) + x and style patch j = jy (Ws - 2) + jx are the C x 3 x 3
// blocks with their top-left corner there.
//   score(i, j) = <ck patch i, sk patch j> / ||sk patch j||_2   (0 for a style patch of zero norm)
//   index(i)    = the j of maximal score; the lowest j on equal scores; a NaN never wins; a score
//                 replaces the running (-inf, 0) only when strictly greater, so (score -inf, index 0)
//                 is what a patch without any winner returns
//   out[y, x]   = (1 - alpha) c[y, x] + alpha / cnt(y, x) * sum over (dy, dx) ascending, content patch
//                 (y - dy, x - dx) existing, of sv[jy + dy, jx + dx] with (jy, jx) = index(y - dy, x - dx)
// Three stages, each a C-ABI entry of its own, and ast_style_swap_f32 is exactly their composition:
//   inverse norms  per-pixel squared norm over the channels (four interleaved channel quarters, summed
//                  in quarter order), a 3x3 box sum in (dy, dx) order, 1 / sqrt; the same order at
//                  every position, so equal style patches have equal norms in bits
//   match          an implicit GEMM, M = content patches, N = style patches, K = 9 C as channel chunk x
//                  channel pair x tap. A workgroup owns 64 consecutive content patches and streams
//                  64-patch style tiles; per chunk of 8 channels each side stages, for each of the 3
//                  patch rows, the contiguous run of pixels its 64 patches touch (70 at W = 64; at
//                  most 128 when the map is 5 wide or more, 192 below that: two instantiations), so
//                  the nine taps are shifted reads of one LDS image and no unfolded matrix exists
//                  anywhere. The next chunk's buffer loads (a descriptor per chunk: channels past C
//                  read as 0) are in flight while this one is multiplied. Products are
//                  v_mfma_f32_32x32x2_f32 (4 waves x 32x32, the tile of wct.hip's tile_mm); a score
//                  is one fma chain over k in an order that does not depend on where its style
//                  patch sits. After a style tile the accumulator columns are scaled by the inverse
//                  norms and folded into a running (max, index) pair per content patch in
//                  registers; lanes, waves and workgroups over splits of the style tiles (the grid
//                  is brought to about 16 workgroups per CU) meet once at the end, the partial
//                  pairs of the splits in a workspace, merged in split order. The scores are never
//                  stored.
//   gather         the overlap average with the alpha blend fused, one launch: a thread decodes the
//                  up-to-nine source positions of its pixel once and walks the channels.
// No atomics, no host synchronisation, no allocation: every sample is indexed by a grid dimension, so
// a non-finite value stays inside its own sample.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kT = 256;            // threads per workgroup everywhere in this file
constexpr int MT = 64;             // patches per tile side (4 waves x 32 x 32)
constexpr int KC = 8;              // channels per staged chunk: K = 72 per chunk
constexpr int ROWS = KC * 3;       // staged runs per chunk and side: (channel, patch row)
constexpr int RT = ROWS / 4;       // runs per wave
constexpr int kMaxC = 1024;
constexpr int kMaxSplits = 64;
constexpr int kMaxPlane = 1 << 24; // pixels per map
constexpr int kTargetWGs = 16 * 256;
constexpr int GC = 32;             // channels per workgroup of the gather

// pixel index (in a plane of width w = pw + 2) of the top-left corner of patch i
__device__ __forceinline__ int pix_of(int i, int pw) { return i + 2 * (i / pw); }

// ------------------------------------------------------------------------------------------------
// Inverse norms of the style patches
// ------------------------------------------------------------------------------------------------

// grid (pixels / 64, samples): pix[b, p] = sum over channels of x^2; thread (p, g) sums channels
// g, g + 4, ... and the four partials are added in g order.
__global__ __launch_bounds__(kT) void swap_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ pix, int C,
                                                        int hw) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, p = blockIdx.x * 64 + lane;
  const float* X = x + (int64_t)blockIdx.y * C * hw;
  float s = 0.f;
  if (p < hw)
    for (int c = g; c < C; c += 4) {
      const float v = X[(int64_t)c * hw + p];
      s = fmaf(v, v, s);
    }
  sh[g][lane] = s;
  __syncthreads();
  if (g == 0 && p < hw) pix[(int64_t)blockIdx.y * hw + p] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// grid (patches / 256, samples): inv[b, j] = 1 / sqrt(box sum), 0 unless the sum is positive.
__global__ __launch_bounds__(kT) void swap_invnorm_kernel(const float* __restrict__ pix, float* __restrict__ inv, int hs,
                                                         int ws) {
  const int pw = ws - 2, cnt = (hs - 2) * pw, j = blockIdx.x * kT + threadIdx.x;
  if (j >= cnt) return;
  const float* P = pix + (int64_t)blockIdx.y * hs * ws + pix_of(j, pw);
  float s = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) s += P[dy * ws + dx];
  const float q = 1.0f / sqrtf(s);
  inv[(int64_t)blockIdx.y * cnt + j] = (s > 0.f && q > 0.f) ? q : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Match
// ------------------------------------------------------------------------------------------------

// Where a thread's part of one side's runs lies: wave w takes runs w, w + 4, ...; run rr is channel
// rr / 3 of the chunk, patch row rr % 3; lane l takes pixels l, l + 64, ... of the run. off[t] is the
// byte offset of the lane's first pixel of run t from the chunk's first channel plane. Fixed for a
// tile.
struct Plan {
  int off[RT];
};

__device__ __forceinline__ Plan stage_plan(int hw, int w, int p0, int wave, int lane) {
  Plan p;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int rr = wave + 4 * t, ch = rr / 3, dy = rr - 3 * ch;
    p.off[t] = 4 * (ch * hw + p0 + dy * w + lane);
  }
  return p;
}

// The chunk whose first channel plane is `chunk` (`cleft` >= 1 channels are left from there) into
// registers, NP pixels per lane and run, as buffer loads whose descriptor ends with the chunk's last
// real channel: a channel past C reads as 0 (the hardware's range check), and so does anything past
// the tensor. A pixel past the run is never read by a real patch (a patch past the map's last reads
// the run's first pixels), so what such a load returns -- the next plane's pixels -- does not matter.
// No load is predicated, so all of them are in flight together.
template <int NP>
__device__ __forceinline__ void stage_load(float (&reg)[RT][NP], const float* chunk, int cleft, int hw, const Plan& p) {
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(chunk), 0, 4 * min(cleft, KC) * hw, 0x00020000);
#pragma unroll
  for (int ps = 0; ps < NP; ++ps)
#pragma unroll
    for (int t = 0; t < RT; ++t)
      reg[t][ps] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, p.off[t] + 256 * ps, 0, 0));
}

template <int NP>
__device__ __forceinline__ void stage_store(const float (&reg)[RT][NP], float* S, int wave, int lane) {
#pragma unroll
  for (int ps = 0; ps < NP; ++ps)
#pragma unroll
    for (int t = 0; t < RT; ++t) S[(wave + 4 * t) * (64 * NP) + lane + 64 * ps] = reg[t][ps];
}

// b wins over a: greater, or equal with the lower index
__device__ __forceinline__ void fold(float& v, int& ix, float ov, int oi) {
  if (ov > v || (ov == v && oi < ix)) {
    v = ov;
    ix = oi;
  }
}

// grid (content tiles, splits, samples). Writes (score, index) of content patch i of sample b and
// split s at [(b * splits + s) * M + i]: the outputs themselves when splits == 1. NP = 2 (runs of up to
// 128 pixels) covers every map at least 5 wide on both sides; NP = 3 the narrower ones.
template <int NP>
__global__ __launch_bounds__(kT) void swap_match_kernel(const float* __restrict__ ck, const float* __restrict__ sk,
                                                       const float* __restrict__ inv, float* __restrict__ oscore,
                                                       int* __restrict__ oindex, int C, int H, int W, int Hs, int Ws,
                                                       int style_batch, int tiles_per_split) {
  constexpr int SEG = 64 * NP;  // floats per run
  __shared__ float As[ROWS * SEG];
  __shared__ float Bs[ROWS * SEG];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave & 1, wn = wave >> 1;
  const int pw = W - 2, M = (H - 2) * pw, pws = Ws - 2, N = (Hs - 2) * pws, hw = H * W, hws = Hs * Ws;
  const int b = blockIdx.z, bs = style_batch == 1 ? 0 : b, split = blockIdx.y;
  const int m0 = blockIdx.x * MT, ntiles = (N + MT - 1) / MT;
  const int jt_beg = split * tiles_per_split, jt_end = min(jt_beg + tiles_per_split, ntiles);
  const float* Ab = ck + (int64_t)b * C * hw;
  const float* Bb = sk + (int64_t)bs * C * hws;
  const float* invb = inv + (int64_t)bs * N;

  const int pa0 = pix_of(m0, pw);  // first pixel of the content tile's runs
  const int ia = m0 + wm * 32 + r;
  const float* Ar = As + h * 3 * SEG + (ia < M ? pix_of(ia, pw) - pa0 : 0);

  float best[16];
  int bidx[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    best[i] = -INFINITY;
    bidx[i] = 0;
  }

  float ra[RT][NP], rb[RT][NP];
  int pb0 = pix_of(jt_beg * MT, pws), pn0 = pb0;  // and of the style tile's, this one and the next
  const Plan pa = stage_plan(hw, W, pa0, wave, lane);
  Plan pb = stage_plan(hws, Ws, pb0, wave, lane);
  if (jt_beg < jt_end) {
    stage_load<NP>(ra, Ab, C, hw, pa);
    stage_load<NP>(rb, Bb, C, hws, pb);
  }
  for (int jt = jt_beg; jt < jt_end; ++jt) {
    const int j = jt * MT + wn * 32 + r;
    const bool jvalid = j < N;
    const float* Br = Bs + h * 3 * SEG + (jvalid ? pix_of(j, pws) - pb0 : 0);
    f32x16 acc = (f32x16){0.f};
    for (int c0 = 0; c0 < C; c0 += KC) {
      stage_store<NP>(ra, As, wave, lane);
      stage_store<NP>(rb, Bs, wave, lane);
      __syncthreads();
      // the next chunk -- the next style tile's first one after this tile's last -- is in flight
      // while this one is multiplied; the workgroup's last step loads a chunk again that nobody uses
      const bool wrap = c0 + KC >= C;
      const int nc0 = wrap ? 0 : c0 + KC;
      if (wrap && jt + 1 < jt_end) {
        pn0 = pix_of((jt + 1) * MT, pws);
        pb = stage_plan(hws, Ws, pn0, wave, lane);
      }
      stage_load<NP>(ra, Ab + (int64_t)nc0 * hw, C - nc0, hw, pa);
      stage_load<NP>(rb, Bb + (int64_t)nc0 * hws, C - nc0, hws, pb);
      __builtin_amdgcn_sched_barrier(0);  // the loads are issued here, ahead of the products, not after them
      // k order of every score: channel pair, patch row, patch column; lane half h takes the pair's
      // channel h
#pragma unroll
      for (int cp = 0; cp < KC / 2; ++cp)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int o = (2 * cp * 3 + dy) * SEG + dx;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ar[o], Br[o], acc, 0, 0, 0);
          }
      __syncthreads();
    }
    const float iv = jvalid ? invb[j] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float s = acc[i] * iv;
      if (jvalid && s > best[i]) {  // j grows from tile to tile: the lowest j of equal scores stays
        best[i] = s;
        bidx[i] = j;
      }
    }
    pb0 = pn0;
  }

  // the 32 lanes of a half hold the same 16 rows over different columns; then the two waves of a row
  float* redv = As;              // [2 wm][32 rows] of the wn = 1 waves
  int* redi = (int*)(As + 64);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float v = best[i];
    int ix = bidx[i];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(ix, o, 64);
      fold(v, ix, ov, oi);
    }
    best[i] = v;
    bidx[i] = ix;
  }
  if (wn == 1 && r == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
      redv[wm * 32 + row] = best[i];
      redi[wm * 32 + row] = bidx[i];
    }
  }
  __syncthreads();
  if (wn == 0 && r == 0) {
    const int64_t ob = ((int64_t)b * gridDim.y + split) * M;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * h, gi = m0 + wm * 32 + row;
      if (gi >= M) continue;
      float v = best[i];
      int ix = bidx[i];
      fold(v, ix, redv[wm * 32 + row], redi[wm * 32 + row]);
      oscore[ob + gi] = v;
      oindex[ob + gi] = ix;
    }
  }
}

// grid (patches / 256, samples): the splits of a content patch in split order; a later split holds
// higher j only, so strictly greater keeps the lowest j of equal scores.
__global__ __launch_bounds__(kT) void swap_merge_kernel(const float* __restrict__ pscore, const int* __restrict__ pindex,
                                                       float* __restrict__ score, int* __restrict__ index, int M,
                                                       int splits) {
  const int i = blockIdx.x * kT + threadIdx.x, b = blockIdx.y;
  if (i >= M) return;
  float v = -INFINITY;
  int ix = 0;
  for (int s = 0; s < splits; ++s) {
    const int64_t o = ((int64_t)b * splits + s) * M + i;
    const float ov = pscore[o];
    if (ov > v) {
      v = ov;
      ix = pindex[o];
    }
  }
  score[(int64_t)b * M + i] = v;
  index[(int64_t)b * M + i] = ix;
}

// ------------------------------------------------------------------------------------------------
// Gather: grid (pixels / 256, channels / GC, samples)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void swap_gather_kernel(const float* __restrict__ sv, const int* __restrict__ index,
                                                        const float* __restrict__ content, float* __restrict__ out,
                                                        int C, int H, int W, int Hs, int Ws, int style_batch,
                                                        float alpha) {
  const int hw = H * W, hws = Hs * Ws, pw = W - 2, pws = Ws - 2, N = (Hs - 2) * pws;
  const int p = blockIdx.x * kT + threadIdx.x, b = blockIdx.z;
  if (p >= hw) return;
  const int y = p / W, x = p - y * W;
  const int* idx = index + (int64_t)b * (H - 2) * pw;
  int src[9], cnt = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int py = y - dy, px = x - dx;
      int s = -1;
      if (py >= 0 && py <= H - 3 && px >= 0 && px <= W - 3) {
        const int j = min(max(idx[py * pw + px], 0), N - 1);  // a caller's index outside the map is clamped
        s = pix_of(j, pws) + dy * Ws + dx;
        ++cnt;
      }
      src[dy * 3 + dx] = s;
    }
  const float rc = 1.0f / (float)cnt, beta = 1.f - alpha;
  const int c_beg = blockIdx.y * GC, c_end = min(c_beg + GC, C);
  const float* V = sv + (int64_t)(style_batch == 1 ? 0 : b) * C * hws;
  const int64_t ob = (int64_t)b * C * hw + p;
  for (int c = c_beg; c < c_end; ++c) {
    const float* Vc = V + (int64_t)c * hws;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (src[k] >= 0) s += Vc[src[k]];
    const int64_t o = ob + (int64_t)c * hw;
    out[o] = beta * content[o] + alpha * (s * rc);
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layouts, launch sequences
// ------------------------------------------------------------------------------------------------

inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }
inline int64_t patches(int h, int w) { return (int64_t)(h - 2) * (w - 2); }
inline int tiles_of(int64_t p) { return (int)((p + MT - 1) / MT); }

// AST_OK, or the code that rejects a map of `n` samples and sides h x w
inline int map_shape(int n, int h, int w) {
  if (n <= 0 || n > 65535 || h < 3 || w < 3 || (int64_t)h * w > kMaxPlane) return AST_E_SHAPE;
  return AST_OK;
}

inline int pair_shape(int n, int ns, int hc, int wc, int hs, int ws) {
  if (n <= 0 || ns <= 0 || (ns != n && ns != 1)) return AST_E_SHAPE;
  const int e = map_shape(n, hc, wc);
  return e ? e : map_shape(ns, hs, ws);
}

inline int chan_shape(int c) { return c <= 0 ? AST_E_SHAPE : c > kMaxC ? AST_E_UNSUPPORTED : AST_OK; }

// Splits of the style tiles: as asked (clamped to the tiles), or, for 0, as many as bring the grid to
// kTargetWGs workgroups -- about 16 per CU: three are resident per CU and short ones even out the tail
// (measured at C = 512, 64 x 64: 61 splits at n = 1, 9 at n = 8) --; then rounded so that no split is empty.
inline int match_splits(int n, int hc, int wc, int hs, int ws, int want, int* tiles_per_split) {
  const int ntiles = tiles_of(patches(hs, ws));
  const int64_t wgs = (int64_t)n * tiles_of(patches(hc, wc));
  int64_t s = want > 0 ? want : (kTargetWGs + wgs - 1) / wgs;
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > ntiles) s = ntiles;
  if (s < 1) s = 1;
  const int tps = (int)((ntiles + s - 1) / s);
  if (tiles_per_split) *tiles_per_split = tps;
  return (ntiles + tps - 1) / tps;
}

inline int64_t norms_ws(int ns, int hs, int ws) { return al256((int64_t)4 * ns * hs * ws); }

// [score scratch | partial scores | partial indices]
inline int64_t match_ws(int n, int hc, int wc, int hs, int ws, int want) {
  const int s = match_splits(n, hc, wc, hs, ws, want, nullptr);
  const int64_t one = al256((int64_t)4 * n * patches(hc, wc));
  return one + (s > 1 ? 2 * al256((int64_t)4 * n * s * patches(hc, wc)) : 0);
}

int norms_launch(const float* sk, float* inv, int ns, int c, int hs, int ws, float* pix, hipStream_t st) {
  const int hw = hs * ws;
  hipLaunchKernelGGL(swap_sqnorm_kernel, dim3((hw + 63) / 64, ns), dim3(kT), 0, st, sk, pix, c, hw);
  hipLaunchKernelGGL(swap_invnorm_kernel, dim3((unsigned)((patches(hs, ws) + kT - 1) / kT), ns), dim3(kT), 0, st,
                     (const float*)pix, inv, hs, ws);
  return (int)hipGetLastError();
}

int match_launch(const float* ck, const float* sk, const float* inv, int* index, float* score, int n, int ns, int c,
                 int hc, int wc, int hs, int ws, int want, unsigned char* wsp, hipStream_t st) {
  int tps = 0;
  const int splits = match_splits(n, hc, wc, hs, ws, want, &tps);
  const int m = (int)patches(hc, wc);
  const int64_t one = al256((int64_t)4 * n * m);
  if (!score) score = (float*)wsp;
  const dim3 grid(tiles_of(m), splits, n);
  // a tile's run is 63 patches + 2 pixels per image row crossed + 3: within 128 when a row has 3 patches or more
  auto kern = (wc >= 5 && ws >= 5) ? swap_match_kernel<2> : swap_match_kernel<3>;
  if (splits == 1) {
    hipLaunchKernelGGL(kern, grid, dim3(kT), 0, st, ck, sk, inv, score, index, c, hc, wc, hs, ws, ns, tps);
  } else {
    float* ps = (float*)(wsp + one);
    int* pi = (int*)(wsp + one + al256((int64_t)4 * n * splits * m));
    hipLaunchKernelGGL(kern, grid, dim3(kT), 0, st, ck, sk, inv, ps, pi, c, hc, wc, hs, ws, ns, tps);
    hipLaunchKernelGGL(swap_merge_kernel, dim3((m + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)ps, (const int*)pi,
                       score, index, m, splits);
  }
  return (int)hipGetLastError();
}

int gather_launch(const float* sv, const int* index, const float* content, float* out, int n, int ns, int c, int hc,
                  int wc, int hs, int ws, float alpha, hipStream_t st) {
  hipLaunchKernelGGL(swap_gather_kernel, dim3((hc * wc + kT - 1) / kT, (c + GC - 1) / GC, n), dim3(kT), 0, st, sv, index,
                     content, out, c, hc, wc, hs, ws, ns, alpha);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

long long ast_patch_norms_workspace_bytes(int ns, int hs, int ws) {
  const int e = map_shape(ns, hs, ws);
  return e ? e : norms_ws(ns, hs, ws);
}

int ast_patch_norms_f32(const float* style_key, float* inv_norm, int ns, int c, int hs, int ws, void* workspace,
                        long long workspace_bytes, void* stream) {
  if (!style_key || !inv_norm || !workspace) return AST_E_NULLPTR;
  int e = map_shape(ns, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (workspace_bytes < norms_ws(ns, hs, ws)) return AST_E_SHAPE;
  return norms_launch(style_key, inv_norm, ns, c, hs, ws, (float*)workspace, (hipStream_t)stream);
}

long long ast_patch_match_workspace_bytes(int n, int ns, int hc, int wc, int hs, int ws, int splits) {
  const int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  return match_ws(n, hc, wc, hs, ws, splits);
}

int ast_patch_match_ex_f32(const float* content_key, const float* style_key, const float* inv_norm, int* index,
                           float* score_or_null, int n, int ns, int c, int hc, int wc, int hs, int ws, int splits,
                           void* workspace, long long workspace_bytes, void* stream) {
  if (!content_key || !style_key || !inv_norm || !index || !workspace) return AST_E_NULLPTR;
  int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  if (workspace_bytes < match_ws(n, hc, wc, hs, ws, splits)) return AST_E_SHAPE;
  return match_launch(content_key, style_key, inv_norm, index, score_or_null, n, ns, c, hc, wc, hs, ws, splits,
                      (unsigned char*)workspace, (hipStream_t)stream);
}

int ast_patch_match_f32(const float* content_key, const float* style_key, const float* inv_norm, int* index,
                        float* score_or_null, int n, int ns, int c, int hc, int wc, int hs, int ws, void* workspace,
                        long long workspace_bytes, void* stream) {
  return ast_patch_match_ex_f32(content_key, style_key, inv_norm, index, score_or_null, n, ns, c, hc, wc, hs, ws, 0,
                                workspace, workspace_bytes, stream);
}

int ast_patch_gather_f32(const float* style_value, const int* index, const float* content, float* out, int n, int ns,
                         int c, int hc, int wc, int hs, int ws, double alpha, void* stream) {
  if (!style_value || !index || !content || !out) return AST_E_NULLPTR;
  int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  return gather_launch(style_value, index, content, out, n, ns, c, hc, wc, hs, ws, (float)alpha, (hipStream_t)stream);
}

// [inverse norms | index | the larger of the norms' and the match's scratch]
long long ast_style_swap_workspace_bytes(int n, int ns, int hc, int wc, int hs, int ws) {
  const int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (e) return e;
  const int64_t a = norms_ws(ns, hs, ws), b = match_ws(n, hc, wc, hs, ws, 0);
  return al256((int64_t)4 * ns * patches(hs, ws)) + al256((int64_t)4 * n * patches(hc, wc)) + (a > b ? a : b);
}

int ast_style_swap_f32(const float* content_key, const float* style_key, const float* style_value, const float* content,
                       float* out, int* index_or_null, float* score_or_null, int n, int ns, int c, int hc, int wc,
                       int hs, int ws, double alpha, void* workspace, long long workspace_bytes, void* stream) {
  if (!content_key || !style_key || !style_value || !content || !out || !workspace) return AST_E_NULLPTR;
  int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (workspace_bytes < ast_style_swap_workspace_bytes(n, ns, hc, wc, hs, ws)) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* w = (unsigned char*)workspace;
  float* inv = (float*)w;
  int* index = (int*)(w + al256((int64_t)4 * ns * patches(hs, ws)));
  unsigned char* scratch = (unsigned char*)index + al256((int64_t)4 * n * patches(hc, wc));
  if (index_or_null) index = index_or_null;
  e = norms_launch(style_key, inv, ns, c, hs, ws, (float*)scratch, st);
  if (e) return e;
  e = match_launch(content_key, style_key, inv, index, score_or_null, n, ns, c, hc, wc, hs, ws, 0, scratch, st);
  if (e) return e;
  return gather_launch(style_value, index, content, out, n, ns, c, hc, wc, hs, ws, (float)alpha, st);
}

}  // extern "C"
