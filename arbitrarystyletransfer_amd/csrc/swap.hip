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
// Guided style swap (semantic patch transfer) is the same three stages over a bank of S styles shared
// by the batch, with one uint8 class per content patch and per style patch: a content patch is matched
// only against the style patches of its own class (a class >= AST_SWAP_MAX_CLASSES takes no part), the
// index is global over the bank, j = s Ns + local, and -1 where nothing is admissible. The match is the
// guided instantiation of the same kernel, scores bit-equal to the unguided one's; a pre-kernel writes
// one 64-bit class-presence mask per 64-patch tile and a workgroup visits only the bank tiles whose
// mask meets its content tile's. The gather skips negative indices and copies the content where no
// covering patch has a match. ast_style_swap_guided_f32 is norms, masks, match, gather.
// No atomics, no host synchronisation, no allocation: every sample is indexed by a grid dimension, so
// a non-finite value stays inside its own sample.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "match_tile.h"
#include "ws.h"

namespace {

using ast_tile::acc_row;
using ast_tile::f32x16;
using ast_tile::fold_arg;

constexpr int kT = 256;            // threads per workgroup everywhere in this file
constexpr int MT = 64;             // patches per tile side (4 waves x 32 x 32)
constexpr int KC = 8;              // channels per staged chunk: K = 72 per chunk
constexpr int ROWS = KC * 3;       // staged runs per chunk and side: (channel, patch row)
constexpr int RT = ROWS / 4;       // runs per wave
constexpr int kMaxC = 1024;
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
  if (p < hw) s = ast_tile::quarter_sqsum(X, C, hw, g, p);
  sh[g][lane] = s;
  __syncthreads();
  if (g == 0 && p < hw) pix[(int64_t)blockIdx.y * hw + p] = ast_tile::quarter_sum(sh, lane);
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

// What the guided match reads beside the unguided one's inputs: one class
// per content patch [n, M] and per style patch of the bank [S, Ns], and the class-presence masks of
// the 64-patch tiles, bit k = "some patch of the tile has class k", content [n, content tiles] and
// bank [S * tiles per style].
struct Guide {
  const uint8_t* cc;
  const uint8_t* sc;
  const unsigned long long* cmask;
  const unsigned long long* bmask;
  int flags;
};

// The guided instantiation of the match kernel has one more argument, a Guide; the unguided one none,
// so its signature is what it was.
template <class... G>
__device__ __forceinline__ Guide guide_of(G... g) {
  if constexpr (sizeof...(G) == 1)
    return (g, ...);
  else
    return Guide{};
}

// A 64-bit value that every lane holds equal, moved to scalar registers: what a branch around a
// barrier may depend on.
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// The first bank tile in [t, end) whose classes meet the content tile's `cm` -- every tile when `all`
// (AST_SWAP_NO_SKIP) --, or `end`. Workgroup-uniform by construction: t, end and cm are scalars of the
// workgroup (block indices, kernel arguments and readfirstlane results), every thread reads the same
// mask words in the same order, and the result passes through readfirstlane again.
__device__ __forceinline__ int next_visited(const unsigned long long* __restrict__ bmask, unsigned long long cm, int t,
                                            int end, bool all) {
  if (!all)
    while (t < end && !(uniform64(bmask[t]) & cm)) ++t;
  return __builtin_amdgcn_readfirstlane(min(t, end));
}

// The match of one workgroup: grid (content tiles, splits, samples). Writes (score, index) of content
// patch i of sample b and split s at [(b * splits + s) * M + i]: the outputs themselves when
// splits == 1. NP = 2 (runs of up to 128 pixels) covers every map at least 5 wide on both sides; NP = 3
// the narrower ones. GUIDED: the style maps are a bank of `style_batch` styles shared by the batch,
// bank tile t = (style t / tiles per style, local tile t % tiles per style) so that no tile straddles
// two styles, the index is the global s Ns + local one, a style patch is admitted for an accumulator
// row only where the row's content class equals its own, a bank tile is visited only if its class mask
// meets the content tile's, and a patch without a winner returns index -1.
template <int NP, class... G>
__global__ __launch_bounds__(kT) void swap_match_kernel(const float* __restrict__ ck, const float* __restrict__ sk,
                                                       const float* __restrict__ inv, float* __restrict__ oscore,
                                                       int* __restrict__ oindex, int C, int H, int W, int Hs, int Ws,
                                                       int style_batch, int tiles_per_split, G... guide) {
  constexpr bool GUIDED = sizeof...(G) == 1;
  const Guide g = guide_of(guide...);
  constexpr int SEG = 64 * NP;  // floats per run
  __shared__ float As[ROWS * SEG];
  __shared__ float Bs[ROWS * SEG];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave & 1, wn = wave >> 1;
  const int pw = W - 2, M = (H - 2) * pw, pws = Ws - 2, N = (Hs - 2) * pws, hw = H * W, hws = Hs * Ws;
  const int b = blockIdx.z, bs = GUIDED ? 0 : style_batch == 1 ? 0 : b, split = blockIdx.y;
  const int tps = (N + MT - 1) / MT;  // 64-patch tiles of one style map
  const int m0 = blockIdx.x * MT, ntiles = GUIDED ? style_batch * tps : tps;
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
    bidx[i] = GUIDED ? -1 : 0;
  }

  // GUIDED: the classes of the lane's 16 accumulator rows, four to a register (rows 4 q .. 4 q + 3 are
  // consecutive content patches), 0xff for "takes no part"; the content tile's class mask; the first
  // tile to visit and the style it lies in.
  unsigned ccls[4] = {0u, 0u, 0u, 0u};
  unsigned long long cm = 0;
  bool all = true;
  int jt0 = jt_beg, sty = 0;
  if constexpr (GUIDED) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int gi = m0 + wm * 32 + 8 * q + 4 * h + k;
        const unsigned v = gi < M ? g.cc[(int64_t)b * M + gi] : 0xffu;
        ccls[q] |= (v < AST_SWAP_MAX_CLASSES ? v : 0xffu) << (8 * k);
      }
    cm = uniform64(g.cmask[(int64_t)b * gridDim.x + blockIdx.x]);
    all = (g.flags & AST_SWAP_NO_SKIP) != 0;
    jt0 = next_visited(g.bmask, cm, jt_beg, jt_end, all);
    sty = jt0 / tps;
    Bb += (int64_t)sty * C * hws;
  }

  float ra[RT][NP], rb[RT][NP];
  int pb0 = pix_of((jt0 - sty * tps) * MT, pws), pn0 = pb0;  // and of the style tile's, this one and the next
  const Plan pa = stage_plan(hw, W, pa0, wave, lane);
  Plan pb = stage_plan(hws, Ws, pb0, wave, lane);
  if (jt0 < jt_end) {
    stage_load<NP>(ra, Ab, C, hw, pa);
    stage_load<NP>(rb, Bb, C, hws, pb);
  }
  // Every branch below that encloses a barrier depends on jt, jn and jt_end alone, and these are
  // workgroup-uniform: jt_end comes from block indices and kernel arguments, jt and jn from
  // next_visited (see there). So all 256 threads visit the same tiles and meet at every barrier.
  // GUIDED: jn is the tile visited after jt (jt_end: none); Bb, sty and pb describe tile jt at the top
  // of the body and are moved on to jn at its last chunk. Unguided, the next tile is jt + 1.
  for (int jt = GUIDED ? jt0 : jt_beg, jn = 0; jt < jt_end; GUIDED ? (jt = jn) : ++jt) {
    if constexpr (GUIDED) jn = next_visited(g.bmask, cm, jt + 1, jt_end, all);
    const int st = sty, jl = (jt - st * tps) * MT + wn * 32 + r;  // this tile's style, the lane's patch in it
    const int j = st * N + jl;
    const bool jvalid = jl < N;
    const float* Br = Bs + h * 3 * SEG + (jvalid ? pix_of(jl, pws) - pb0 : 0);
    f32x16 acc = (f32x16){0.f};
    for (int c0 = 0; c0 < C; c0 += KC) {
      stage_store<NP>(ra, As, wave, lane);
      stage_store<NP>(rb, Bs, wave, lane);
      __syncthreads();
      // the next chunk -- the next visited style tile's first one after this tile's last -- is in flight
      // while this one is multiplied; the workgroup's last step loads a chunk again that nobody uses
      const bool wrap = c0 + KC >= C;
      const int nc0 = wrap ? 0 : c0 + KC;
      if (wrap && (GUIDED ? jn : jt + 1) < jt_end) {
        if constexpr (GUIDED) {
          const int sn = jn / tps;
          Bb += (int64_t)(sn - sty) * C * hws;
          sty = sn;
          pn0 = pix_of((jn - sn * tps) * MT, pws);
        } else {
          pn0 = pix_of((jt + 1) * MT, pws);
        }
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
    if constexpr (GUIDED) {
      // the lane's column is one style patch with one class, loaded beside its inverse norm; 0xfe
      // ("never a candidate") equals no content class
      const unsigned v = jvalid ? g.sc[j] : 0xfeu;
      const unsigned scls = v < AST_SWAP_MAX_CLASSES ? v : 0xfeu;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float s = acc[i] * iv;
        if (((ccls[i >> 2] >> (8 * (i & 3))) & 0xffu) == scls && s > best[i]) {
          best[i] = s;
          bidx[i] = j;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float s = acc[i] * iv;
        if (jvalid && s > best[i]) {  // j grows from tile to tile: the lowest j of equal scores stays
          best[i] = s;
          bidx[i] = j;
        }
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
      fold_arg<true>(v, ix, ov, oi);
    }
    best[i] = v;
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
      float v = best[i];
      int ix = bidx[i];
      fold_arg<true>(v, ix, redv[wm * 32 + row], redi[wm * 32 + row]);
      oscore[ob + gi] = v;
      oindex[ob + gi] = ix;
    }
  }
}

// grid (tiles, maps), one wave per 64-patch tile: mask[map, tile] = OR over the tile's patches of
// 1 << class, a class >= AST_SWAP_MAX_CLASSES or a patch past the map giving no bit; an OR-reduction
// across the wave's lanes.
__global__ __launch_bounds__(64) void swap_class_mask_kernel(const uint8_t* __restrict__ cls,
                                                            unsigned long long* __restrict__ mask, int P) {
  const int lane = threadIdx.x, i = blockIdx.x * MT + lane;
  const unsigned v = i < P ? cls[(int64_t)blockIdx.y * P + i] : 0xffu;
  unsigned lo = v < 32 ? 1u << v : 0u, hi = (v >= 32 && v < AST_SWAP_MAX_CLASSES) ? 1u << (v - 32) : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo |= (unsigned)__shfl_xor((int)lo, o, 64);
    hi |= (unsigned)__shfl_xor((int)hi, o, 64);
  }
  if (lane == 0) mask[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((unsigned long long)hi << 32) | lo;
}

// grid (patches / 256, samples): the splits of a content patch in split order; a later split holds
// higher j only, so strictly greater keeps the lowest j of equal scores. NONE is the index of a patch
// for which no split has a winner: 0, or -1 for the guided match.
template <int NONE>
__global__ __launch_bounds__(kT) void swap_merge_kernel(const float* __restrict__ pscore, const int* __restrict__ pindex,
                                                       float* __restrict__ score, int* __restrict__ index, int M,
                                                       int splits) {
  ast_tile::merge_slots<true, kT>(pscore, pindex, score, index, M, splits, NONE);
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

// The guided gather, same grid: the index is global over a bank of `styles` maps, j = s Ns + local; a
// negative index is "no match" and adds no term; a pixel none of whose covering patches has a match
// is a copy of the content.
__global__ __launch_bounds__(kT) void swap_gather_guided_kernel(const float* __restrict__ sv,
                                                               const int* __restrict__ index,
                                                               const float* __restrict__ content,
                                                               float* __restrict__ out, int C, int H, int W, int Hs,
                                                               int Ws, int styles, float alpha) {
  const int hw = H * W, hws = Hs * Ws, pw = W - 2, pws = Ws - 2, N = (Hs - 2) * pws;
  const int p = blockIdx.x * kT + threadIdx.x, b = blockIdx.z;
  if (p >= hw) return;
  const int y = p / W, x = p - y * W;
  const int* idx = index + (int64_t)b * (H - 2) * pw;
  const int last = styles * N - 1;  // < 2^31: checked on the host
  int64_t src[9];                   // the source pixel's offset in its style's channel 0, or -1
  int cnt = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int py = y - dy, px = x - dx;
      int64_t s = -1;
      if (py >= 0 && py <= H - 3 && px >= 0 && px <= W - 3) {
        const int j = min(idx[py * pw + px], last);  // a caller's index past the bank is clamped
        if (j >= 0) {
          const int st = j / N;
          s = (int64_t)st * C * hws + pix_of(j - st * N, pws) + dy * Ws + dx;
          ++cnt;
        }
      }
      src[dy * 3 + dx] = s;
    }
  const float rc = 1.0f / (float)cnt, beta = 1.f - alpha;
  const int c_beg = blockIdx.y * GC, c_end = min(c_beg + GC, C);
  const int64_t ob = (int64_t)b * C * hw + p;
  for (int c = c_beg; c < c_end; ++c) {
    const float* Vc = sv + (int64_t)c * hws;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (src[k] >= 0) s += Vc[src[k]];
    const int64_t o = ob + (int64_t)c * hw;
    const float x0 = content[o];
    out[o] = cnt ? beta * x0 + alpha * (s * rc) : x0;
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: argument checks, workspace layouts, launch sequences
// ------------------------------------------------------------------------------------------------

using ast_tile::tiles_of;
inline int64_t patches(int h, int w) { return (int64_t)(h - 2) * (w - 2); }

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

inline int chan_shape(int c) { return ast_tile::chan_shape(c, kMaxC); }

// A workspace of one region is its size: the norms' [squared pixel norms]
inline int64_t norms_ws(int ns, int hs, int ws) { return ast_ws::al256((int64_t)4 * ns * hs * ws); }

// The match's workspace: [score scratch | content tile masks | bank tile masks | partial scores |
// partial indices]; the masks only for the guided match (S > 0 styles in the bank), the partials only
// when there is more than one split. Splits of the style tiles (ast_tile::split_tiles), of the bank
// tiles when guided, whatever the classes are (the count must not depend on device data; under
// skipping the runs do unequal work, which the many workgroups per CU even out): as asked (clamped to
// the tiles), or, for 0, as many as bring the grid to kTargetWGs workgroups -- about 16 per CU: three
// are resident per CU and short ones even out the tail (measured at C = 512, 64 x 64: 61 splits at
// n = 1, 9 at n = 8).
struct MatchWs {
  int splits, tiles_per_split;
  float* score;
  unsigned long long *cmask, *bmask;
  float* pscore;
  int* pindex;
  int64_t bytes;
};

inline MatchWs match_ws(void* base, int n, int S, int hc, int wc, int hs, int ws, int want) {
  ast_ws::Walk wk(base);
  const int64_t m = patches(hc, wc);
  const int ct = tiles_of(m), bt = (S > 0 ? S : 1) * tiles_of(patches(hs, ws));
  int tps = 0;
  const int s = ast_tile::split_tiles((int64_t)n * ct, bt, want, kTargetWGs, 1, &tps);
  using u64 = unsigned long long;
  return {s, tps, wk.take<float>(4 * n * m), S > 0 ? wk.take<u64>((int64_t)8 * n * ct) : nullptr,
          S > 0 ? wk.take<u64>((int64_t)8 * bt) : nullptr, s > 1 ? wk.take<float>(4 * n * s * m) : nullptr,
          s > 1 ? wk.take<int>(4 * n * s * m) : nullptr, wk.off};
}

// The whole op's workspace: [inverse norms | index | scratch], the scratch the norms' workspace, then
// the match's (the guided match's for a bank of S > 0 styles): stream order keeps them apart
struct SwapWs {
  float* inv;
  int* index;
  void* scratch;
  int64_t bytes;
};

inline SwapWs swap_ws(void* base, int n, int ns, int S, int hc, int wc, int hs, int ws) {
  ast_ws::Walk wk(base);
  return {wk.take<float>(4 * ns * patches(hs, ws)), wk.take<int>(4 * n * patches(hc, wc)),
          wk.take<void>(std::max<int64_t>(norms_ws(ns, hs, ws), match_ws(nullptr, n, S, hc, wc, hs, ws, 0).bytes)), wk.off};
}

int norms_launch(const float* sk, float* inv, int ns, int c, int hs, int ws, float* pix, hipStream_t st) {
  const int hw = hs * ws;
  hipLaunchKernelGGL(swap_sqnorm_kernel, dim3((hw + 63) / 64, ns), dim3(kT), 0, st, sk, pix, c, hw);
  hipLaunchKernelGGL(swap_invnorm_kernel, dim3((unsigned)((patches(hs, ws) + kT - 1) / kT), ns), dim3(kT), 0, st,
                     (const float*)pix, inv, hs, ws);
  return (int)hipGetLastError();
}

int match_launch(const float* ck, const float* sk, const float* inv, int* index, float* score, int n, int ns, int c,
                 int hc, int wc, int hs, int ws, int want, void* wsp, hipStream_t st) {
  const MatchWs w = match_ws(wsp, n, 0, hc, wc, hs, ws, want);
  const int splits = w.splits, tps = w.tiles_per_split;
  const int m = (int)patches(hc, wc);
  if (!score) score = w.score;
  const dim3 grid(tiles_of(m), splits, n);
  // a tile's run is 63 patches + 2 pixels per image row crossed + 3: within 128 when a row has 3 patches or more
  auto kern = (wc >= 5 && ws >= 5) ? swap_match_kernel<2> : swap_match_kernel<3>;
  if (splits == 1) {
    hipLaunchKernelGGL(kern, grid, dim3(kT), 0, st, ck, sk, inv, score, index, c, hc, wc, hs, ws, ns, tps);
  } else {
    float* ps = w.pscore;
    int* pi = w.pindex;
    hipLaunchKernelGGL(kern, grid, dim3(kT), 0, st, ck, sk, inv, ps, pi, c, hc, wc, hs, ws, ns, tps);
    hipLaunchKernelGGL(swap_merge_kernel<0>, dim3((m + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)ps, (const int*)pi,
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

// ---- guided: a bank of S styles shared by the batch, one class per patch ------------------------------

// AST_OK, or the code that rejects n content maps hc x wc against a bank of S maps hs x ws
inline int bank_shape(int n, int S, int hc, int wc, int hs, int ws) {
  if (n <= 0 || S <= 0) return AST_E_SHAPE;
  int e = map_shape(n, hc, wc);
  if (!e) e = map_shape(S, hs, ws);
  if (!e && (int64_t)S * patches(hs, ws) > INT32_MAX) e = AST_E_SHAPE;  // the global style patch index is an int32
  return e;
}

int guided_match_launch(const float* ck, const float* sk, const float* inv, const uint8_t* cc, const uint8_t* sc,
                        int* index, float* score, int n, int S, int c, int hc, int wc, int hs, int ws, int want,
                        int flags, void* wsp, hipStream_t st) {
  const MatchWs w = match_ws(wsp, n, S, hc, wc, hs, ws, want);
  const int splits = w.splits, tps = w.tiles_per_split;
  const int m = (int)patches(hc, wc), ns = (int)patches(hs, ws), ct = tiles_of(m), bt = tiles_of(ns);
  if (!score) score = w.score;
  unsigned long long *cmask = w.cmask, *bmask = w.bmask;
  hipLaunchKernelGGL(swap_class_mask_kernel, dim3(ct, n), dim3(64), 0, st, cc, cmask, m);
  hipLaunchKernelGGL(swap_class_mask_kernel, dim3(bt, S), dim3(64), 0, st, sc, bmask, ns);
  const Guide g{cc, sc, cmask, bmask, flags};
  const dim3 grid(ct, splits, n);
  auto kern = (wc >= 5 && ws >= 5) ? swap_match_kernel<2, Guide> : swap_match_kernel<3, Guide>;
  if (splits == 1) {
    hipLaunchKernelGGL(kern, grid, dim3(kT), 0, st, ck, sk, inv, score, index, c, hc, wc, hs, ws, S, tps, g);
  } else {
    float* ps = w.pscore;
    int* pi = w.pindex;
    hipLaunchKernelGGL(kern, grid, dim3(kT), 0, st, ck, sk, inv, ps, pi, c, hc, wc, hs, ws, S, tps, g);
    hipLaunchKernelGGL(swap_merge_kernel<-1>, dim3((m + kT - 1) / kT, n), dim3(kT), 0, st, (const float*)ps,
                       (const int*)pi, score, index, m, splits);
  }
  return (int)hipGetLastError();
}

int guided_gather_launch(const float* sv, const int* index, const float* content, float* out, int n, int S, int c,
                         int hc, int wc, int hs, int ws, float alpha, hipStream_t st) {
  hipLaunchKernelGGL(swap_gather_guided_kernel, dim3((hc * wc + kT - 1) / kT, (c + GC - 1) / GC, n), dim3(kT), 0, st, sv,
                     index, content, out, c, hc, wc, hs, ws, S, alpha);
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
  return match_ws(nullptr, n, 0, hc, wc, hs, ws, splits).bytes;
}

int ast_patch_match_ex_f32(const float* content_key, const float* style_key, const float* inv_norm, int* index,
                           float* score_or_null, int n, int ns, int c, int hc, int wc, int hs, int ws, int splits,
                           void* workspace, long long workspace_bytes, void* stream) {
  if (!content_key || !style_key || !inv_norm || !index || !workspace) return AST_E_NULLPTR;
  int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  if (workspace_bytes < match_ws(nullptr, n, 0, hc, wc, hs, ws, splits).bytes) return AST_E_SHAPE;
  return match_launch(content_key, style_key, inv_norm, index, score_or_null, n, ns, c, hc, wc, hs, ws, splits, workspace,
                      (hipStream_t)stream);
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

long long ast_style_swap_workspace_bytes(int n, int ns, int hc, int wc, int hs, int ws) {
  const int e = pair_shape(n, ns, hc, wc, hs, ws);
  return e ? e : swap_ws(nullptr, n, ns, 0, hc, wc, hs, ws).bytes;
}

int ast_style_swap_f32(const float* content_key, const float* style_key, const float* style_value, const float* content,
                       float* out, int* index_or_null, float* score_or_null, int n, int ns, int c, int hc, int wc,
                       int hs, int ws, double alpha, void* workspace, long long workspace_bytes, void* stream) {
  if (!content_key || !style_key || !style_value || !content || !out || !workspace) return AST_E_NULLPTR;
  int e = pair_shape(n, ns, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  const SwapWs w = swap_ws(workspace, n, ns, 0, hc, wc, hs, ws);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  int* index = index_or_null ? index_or_null : w.index;
  e = norms_launch(style_key, w.inv, ns, c, hs, ws, (float*)w.scratch, st);
  if (e) return e;
  e = match_launch(content_key, style_key, w.inv, index, score_or_null, n, ns, c, hc, wc, hs, ws, 0, w.scratch, st);
  if (e) return e;
  return gather_launch(style_value, index, content, out, n, ns, c, hc, wc, hs, ws, (float)alpha, st);
}

// ---- guided ----

long long ast_patch_match_guided_workspace_bytes(int n, int s, int hc, int wc, int hs, int ws, int splits) {
  const int e = bank_shape(n, s, hc, wc, hs, ws);
  if (e) return e;
  if (splits < 0) return AST_E_UNSUPPORTED;
  return match_ws(nullptr, n, s, hc, wc, hs, ws, splits).bytes;
}

int ast_patch_match_guided_ex_f32(const float* content_key, const float* style_keys, const float* inv_norm,
                                  const unsigned char* content_class, const unsigned char* style_class, int* index,
                                  float* score_or_null, int n, int s, int c, int hc, int wc, int hs, int ws, int splits,
                                  int flags, void* workspace, long long workspace_bytes, void* stream) {
  if (!content_key || !style_keys || !inv_norm || !content_class || !style_class || !index || !workspace)
    return AST_E_NULLPTR;
  int e = bank_shape(n, s, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  if (splits < 0 || (flags & ~AST_SWAP_NO_SKIP)) return AST_E_UNSUPPORTED;
  if (workspace_bytes < match_ws(nullptr, n, s, hc, wc, hs, ws, splits).bytes) return AST_E_SHAPE;
  return guided_match_launch(content_key, style_keys, inv_norm, content_class, style_class, index, score_or_null, n, s,
                             c, hc, wc, hs, ws, splits, flags, workspace, (hipStream_t)stream);
}

int ast_patch_gather_guided_f32(const float* style_values, const int* index, const float* content, float* out, int n,
                                int s, int c, int hc, int wc, int hs, int ws, double alpha, void* stream) {
  if (!style_values || !index || !content || !out) return AST_E_NULLPTR;
  int e = bank_shape(n, s, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  return guided_gather_launch(style_values, index, content, out, n, s, c, hc, wc, hs, ws, (float)alpha,
                              (hipStream_t)stream);
}

long long ast_style_swap_guided_workspace_bytes(int n, int s, int hc, int wc, int hs, int ws) {
  const int e = bank_shape(n, s, hc, wc, hs, ws);
  return e ? e : swap_ws(nullptr, n, s, s, hc, wc, hs, ws).bytes;
}

int ast_style_swap_guided_f32(const float* content_key, const float* style_keys, const float* style_values,
                              const float* content, const unsigned char* content_class,
                              const unsigned char* style_class, float* out, int* index_or_null, float* score_or_null,
                              int n, int s, int c, int hc, int wc, int hs, int ws, double alpha, void* workspace,
                              long long workspace_bytes, void* stream) {
  if (!content_key || !style_keys || !style_values || !content || !content_class || !style_class || !out || !workspace)
    return AST_E_NULLPTR;
  int e = bank_shape(n, s, hc, wc, hs, ws);
  if (!e) e = chan_shape(c);
  if (e) return e;
  const SwapWs w = swap_ws(workspace, n, s, s, hc, wc, hs, ws);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  int* index = index_or_null ? index_or_null : w.index;
  e = norms_launch(style_keys, w.inv, s, c, hs, ws, (float*)w.scratch, st);
  if (e) return e;
  e = guided_match_launch(content_key, style_keys, w.inv, content_class, style_class, index, score_or_null, n, s, c, hc,
                          wc, hs, ws, 0, 0, w.scratch, st);
  if (e) return e;
  return guided_gather_launch(style_values, index, content, out, n, s, c, hc, wc, hs, ws, (float)alpha, st);
}

}  // extern "C"
