// Exact feature distribution matching (EFDM; Zhang et al., CVPR 2022) and the segmented plane sort
// it is built on, for gfx950. The reference has no counterpart (its train.py:265 keeps a
// commented-out histogram_match).
//
// Per (n, c) plane: the content element of stable ascending rank r takes the style plane's sorted
// value S[j(r)], j(r) = ((2r + 1) * Ms) / (2 * Mc) (the identity for equal sizes). Floats are
// ordered by IEEE-754 totalOrder of their bits: key = bits ^ (sign ? 0xffffffff : 0x80000000), an
// unsigned compare, so -0 < +0, negative NaNs first, positive NaNs last, equal keys = equal bits.
// Ties keep index order: the content sort compares (key, index), which is unique per element, so
// the (unstable) bitonic network gives the stable result; the style sort needs keys only.
//
// Sort in LDS: lds_sort of sort.h, a bitonic network over a power-of-two length P >= 512 (P = 4096:
// 6 LDS stages and 4 register passes for the 78 stages of the network).
//
// Fused path (both planes <= AST_EFDM_FUSED_MAX): one workgroup per plane sorts the content
// (key, index) pairs, inverts the permutation into a 16-bit rank array, sorts the style keys in the
// space of the content keys, and writes out[i] = blend(c[i], S[j(rank[i])]) with coalesced loads
// and stores. LDS: 4 * max(Pc, Ps) + 4 * Pc bytes (32 KB at 4096, 128 KB at 16384).
// General path: chunks of `chunk` elements sorted in LDS into a workspace, log2(M / chunk) merge
// passes (merge path: every thread finds its split of the two runs by binary search and merges 8
// outputs; the left run wins ties, which keeps index order), then a rank-walk / scatter kernel.
// No atomics, no host synchronisation, no allocation: capturable in a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "sort.h"
#include "ws.h"

using namespace ast_sort;

namespace {

constexpr int kAutoChunk = 4096;     // general path: LDS chunk when the caller leaves it to us
constexpr int kMergeE = 8;           // outputs per thread of a merge pass
constexpr int kMergeThreads = 256;

__device__ __forceinline__ float blend(float c, float t, float alpha) { return c + alpha * (t - c); }

extern __shared__ __align__(16) unsigned char efdm_smem[];

__global__ __launch_bounds__(kMaxThreads) void efdm_fused_kernel(const float* __restrict__ content,
                                                                 const float* __restrict__ style,
                                                                 float* __restrict__ out, int c, int style_shared,
                                                                 int mc, int ms, int pc, int ps, float alpha,
                                                                 int copy) {
  uint32_t* key = reinterpret_cast<uint32_t*>(efdm_smem);
  uint16_t* idx = reinterpret_cast<uint16_t*>(key + (pc > ps ? pc : ps));
  uint16_t* rank = idx + pc;
  const int64_t p = blockIdx.x;
  const int64_t sp = style_shared ? p % c : p;
  const float* x = content + p * mc;
  const float* s = style + sp * ms;
  float* o = out + p * mc;

  lds_fill<true>(x, mc, key, idx, pc);
  lds_sort<true>(key, idx, pc);
  // the real elements come first (padding sorts last): idx[r] < mc for r < mc
  for (int r = threadIdx.x; r < mc; r += blockDim.x) rank[idx[r]] = (uint16_t)r;
  lds_fill<false>(s, ms, key, nullptr, ps);   // nobody reads the content keys any more
  lds_sort<false>(key, nullptr, ps);
  for (int i = threadIdx.x; i < mc; i += blockDim.x) {
    const uint32_t r = rank[i];
    // (2r + 1) * ms < 2^30 for planes <= AST_EFDM_FUSED_MAX: 32-bit arithmetic is exact here
    const uint32_t j = ms == mc ? r : ((2u * r + 1u) * (uint32_t)ms) / (2u * (uint32_t)mc);
    const float t = from_key(key[j]);
    o[i] = copy ? t : blend(x[i], t, alpha);
  }
}

template <bool IDX>
__global__ __launch_bounds__(kMaxThreads) void plane_sort_fused_kernel(const float* __restrict__ x,
                                                                       float* __restrict__ sorted,
                                                                       int* __restrict__ index, int m, int P) {
  uint32_t* key = reinterpret_cast<uint32_t*>(efdm_smem);
  uint16_t* idx = reinterpret_cast<uint16_t*>(key + P);
  const int64_t p = blockIdx.x;
  lds_fill<IDX>(x + p * m, m, key, idx, P);
  lds_sort<IDX>(key, idx, P);
  for (int r = threadIdx.x; r < m; r += blockDim.x) {
    sorted[p * m + r] = from_key(key[r]);
    if (IDX) index[p * m + r] = (int)idx[r];
  }
}

// General path, step 1: chunk `blockIdx.x % cpp` of plane `blockIdx.x / cpp`, sorted in LDS, to the
// workspace as keys (and plane-wide indices).
template <bool IDX>
__global__ __launch_bounds__(kMaxThreads) void chunk_sort_kernel(const float* __restrict__ x,
                                                                 uint32_t* __restrict__ kout,
                                                                 int* __restrict__ iout, int64_t m, int chunk,
                                                                 int64_t cpp, int P) {
  uint32_t* key = reinterpret_cast<uint32_t*>(efdm_smem);
  uint16_t* idx = reinterpret_cast<uint16_t*>(key + P);
  const int64_t p = blockIdx.x / cpp;
  const int64_t base = (blockIdx.x % cpp) * chunk;
  const int cnt = (int)(m - base < chunk ? m - base : chunk);
  lds_fill<IDX>(x + p * m + base, cnt, key, idx, P);
  lds_sort<IDX>(key, idx, P);
  for (int r = threadIdx.x; r < cnt; r += blockDim.x) {
    kout[p * m + base + r] = key[r];
    if (IDX) iout[p * m + base + r] = (int)(base + idx[r]);
  }
}

// General path, step 2: runs of length w merged in pairs into runs of 2w (the last pair of a plane
// may be short or a single run). Thread g of a plane writes outputs [8g, 8g + 8): its split of the
// two runs is the merge-path point of that diagonal. The left run holds the lower indices and wins
// ties, so the merge is stable without looking at the indices.
template <bool IDX>
__global__ __launch_bounds__(kMergeThreads) void merge_pass_kernel(const uint32_t* __restrict__ ksrc,
                                                                   uint32_t* __restrict__ kdst,
                                                                   const int* __restrict__ isrc,
                                                                   int* __restrict__ idst, int64_t m, int64_t w,
                                                                   int64_t bpp) {
  const int64_t p = blockIdx.x / bpp;
  const int64_t g = ((blockIdx.x % bpp) * kMergeThreads + threadIdx.x) * kMergeE;
  if (g >= m) return;
  const int64_t pair = g / (2 * w) * (2 * w);
  const int64_t la = m - pair < w ? m - pair : w;
  const int64_t lb = m - pair - la < w ? m - pair - la : w;
  const uint32_t* A = ksrc + p * m + pair;
  const uint32_t* B = A + la;
  const int64_t d = g - pair;
  int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  int64_t a = lo, b = d - lo;
  const int64_t left = la + lb - d;
  const int cnt = (int)(left < kMergeE ? left : kMergeE);
  uint32_t va = a < la ? A[a] : 0u, vb = b < lb ? B[b] : 0u;
  for (int e = 0; e < cnt; ++e) {
    const bool take_a = b >= lb || (a < la && va <= vb);
    const int64_t at = p * m + pair + d + e;
    if (take_a) {
      kdst[at] = va;
      if (IDX) idst[at] = isrc[p * m + pair + a];
      ++a;
      if (a < la) va = A[a];
    } else {
      kdst[at] = vb;
      if (IDX) idst[at] = isrc[p * m + pair + la + b];
      ++b;
      if (b < lb) vb = B[b];
    }
  }
}

// General path, step 3 of plane_sort: keys back to floats (and the indices out of the workspace).
template <bool IDX>
__global__ __launch_bounds__(kMergeThreads) void emit_sorted_kernel(const uint32_t* __restrict__ keys,
                                                                    const int* __restrict__ idx,
                                                                    float* __restrict__ sorted,
                                                                    int* __restrict__ index, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * kMergeThreads + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kMergeThreads) {
    sorted[i] = from_key(keys[i]);
    if (IDX) index[i] = idx[i];
  }
}

// General path, step 3 of efdm: rank r of plane p is element cidx[p, r]; it takes S[j(r)].
__global__ __launch_bounds__(kMergeThreads) void efdm_scatter_kernel(const float* __restrict__ content,
                                                                     const int* __restrict__ cidx,
                                                                     const uint32_t* __restrict__ skey,
                                                                     float* __restrict__ out, int c,
                                                                     int style_shared, int64_t mc, int64_t ms,
                                                                     int64_t bpp, float alpha, int copy) {
  const int64_t p = blockIdx.x / bpp;
  const int64_t r = (blockIdx.x % bpp) * kMergeThreads + threadIdx.x;
  if (r >= mc) return;
  const int64_t sp = style_shared ? p % c : p;
  const int64_t i = cidx[p * mc + r];
  // (2r + 1) * ms < 2^32 * 2^31: exact in unsigned 64-bit arithmetic
  const int64_t j = ms == mc ? r : (int64_t)(((uint64_t)(2 * r + 1) * (uint64_t)ms) / (uint64_t)(2 * mc));
  const float t = from_key(skey[sp * ms + j]);
  out[p * mc + i] = copy ? t : blend(content[p * mc + i], t, alpha);
}

// ---- host side ------------------------------------------------------------------------------

int64_t pow2_padded(int64_t m) {   // the LDS sort length of m <= AST_EFDM_FUSED_MAX elements
  int64_t p = kTile;
  while (p < m) p <<= 1;
  return p;
}

int sort_threads(int64_t P) { return (int)(P / kE < kMaxThreads ? P / kE : kMaxThreads); }

bool chunk_ok(int chunk) {   // 0: automatic; else a power of two in 64..AST_EFDM_FUSED_MAX
  return chunk == 0 || (chunk >= 64 && chunk <= AST_EFDM_FUSED_MAX && (chunk & (chunk - 1)) == 0);
}

constexpr int64_t kMaxBlocks = 0x7fffffffLL;

// Dynamic LDS above 64 KB has to be allowed per kernel (as mobilenet.hip does).
template <typename K>
int allow_lds(K kern, size_t lds) {
  if (lds <= 64 * 1024) return 0;
  return (int)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// Whether the grids of a general-path sort of `planes` planes of m elements fit (checked before any launch).
bool general_fits(int64_t planes, int64_t m, int chunk) {
  const int64_t cpp = (m + chunk - 1) / chunk;
  const int64_t bpp = (m + (int64_t)kMergeE * kMergeThreads - 1) / ((int64_t)kMergeE * kMergeThreads);
  const int64_t bps = (m + kMergeThreads - 1) / kMergeThreads;   // the scatter's blocks per plane
  return planes <= kMaxBlocks / cpp && planes <= kMaxBlocks / bpp && planes <= kMaxBlocks / bps;
}

// The general-path sort: the result is in (*kres, *ires), one of the two buffer pairs.
template <bool IDX>
int sort_general(const float* x, int64_t planes, int64_t m, int chunk, uint32_t* k0, uint32_t* k1, int* i0,
                 int* i1, hipStream_t st, uint32_t** kres, int** ires) {
  const int64_t cpp = (m + chunk - 1) / chunk;
  const int P = (int)pow2_padded(chunk);
  const size_t lds = (size_t)P * (IDX ? 6 : 4);
  auto kern = chunk_sort_kernel<IDX>;
  int e = allow_lds(kern, lds);
  if (e) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(planes * cpp)), dim3(sort_threads(P)), lds, st, x, k0, i0, m, chunk, cpp,
                     P);
  e = (int)hipGetLastError();
  if (e) return e;
  const int64_t bpp = (m + (int64_t)kMergeE * kMergeThreads - 1) / ((int64_t)kMergeE * kMergeThreads);
  for (int64_t w = chunk; w < m; w *= 2) {
    hipLaunchKernelGGL(merge_pass_kernel<IDX>, dim3((unsigned)(planes * bpp)), dim3(kMergeThreads), 0, st,
                       (const uint32_t*)k0, k1, (const int*)i0, i1, m, w, bpp);
    e = (int)hipGetLastError();
    if (e) return e;
    uint32_t* tk = k0;
    k0 = k1, k1 = tk;
    int* ti = i0;
    i0 = i1, i1 = ti;
  }
  *kres = k0, *ires = i0;
  return 0;
}

bool efdm_fused(int64_t mc, int64_t ms, int chunk) {
  return chunk == 0 && mc <= AST_EFDM_FUSED_MAX && ms <= AST_EFDM_FUSED_MAX;
}

// The general-path sort's workspace: [keys | keys | indices | indices], two buffers each (the merge
// passes ping-pong); the indices only when wanted
struct SortWs {
  uint32_t* key[2];
  int* idx[2];
  int64_t bytes;
};

SortWs sort_ws(void* base, int64_t planes, int64_t m, bool want_index) {
  ast_ws::Walk wk(base);
  const int64_t b = 4 * planes * m;
  return {{wk.take<uint32_t>(b), wk.take<uint32_t>(b)},
          {want_index ? wk.take<int>(b) : nullptr, want_index ? wk.take<int>(b) : nullptr}, wk.off};
}

// The general path's workspace: [the content's sort with indices | the style's sort]
struct EfdmWs {
  void *content, *style;
  int64_t bytes;
};

EfdmWs efdm_ws(void* base, int64_t planes, int64_t splanes, int64_t mc, int64_t ms) {
  ast_ws::Walk wk(base);
  return {wk.take<void>(sort_ws(nullptr, planes, mc, true).bytes),
          wk.take<void>(sort_ws(nullptr, splanes, ms, false).bytes), wk.off};
}

// planes of m elements: both counts positive and within 2^31 - 1, at most 2^40 elements in all (the
// byte counts then stay far inside 64 bits)
bool planes_ok(int64_t planes, int64_t m) {
  return planes > 0 && m > 0 && planes <= 0x7fffffffLL && m <= 0x7fffffffLL && planes <= ((int64_t)1 << 40) / m;
}

bool efdm_shape_ok(int n, int ns, int c, int64_t mc, int64_t ms) {
  if (n <= 0 || c <= 0 || (ns != n && ns != 1)) return false;
  return planes_ok((int64_t)n * c, mc) && planes_ok((int64_t)ns * c, ms);
}

}  // namespace

extern "C" {

long long ast_efdm_ex_workspace_bytes(int n, int ns, int c, long long mc, long long ms, int chunk) {
  if (!efdm_shape_ok(n, ns, c, mc, ms)) return AST_E_SHAPE;
  if (!chunk_ok(chunk)) return AST_E_UNSUPPORTED;
  if (efdm_fused(mc, ms, chunk)) return 0;
  return efdm_ws(nullptr, (int64_t)n * c, (int64_t)ns * c, mc, ms).bytes;
}

long long ast_efdm_workspace_bytes(int n, int ns, int c, long long mc, long long ms) {
  return ast_efdm_ex_workspace_bytes(n, ns, c, mc, ms, 0);
}

int ast_efdm_ex_f32(const float* content, const float* style, float* out, int n, int ns, int c, int hc, int wc,
                    int hs, int ws, double alpha, int chunk, void* workspace, long long workspace_bytes,
                    void* stream) {
  if (!content || !style || !out) return AST_E_NULLPTR;
  if (hc <= 0 || wc <= 0 || hs <= 0 || ws <= 0) return AST_E_SHAPE;
  const int64_t mc = (int64_t)hc * wc, ms = (int64_t)hs * ws;
  if (!efdm_shape_ok(n, ns, c, mc, ms)) return AST_E_SHAPE;
  if (!chunk_ok(chunk)) return AST_E_UNSUPPORTED;
  const int64_t planes = (int64_t)n * c, splanes = (int64_t)ns * c;
  const float a = (float)alpha;
  const int copy = alpha == 1.0 ? 1 : 0;
  const int shared = ns == 1 ? 1 : 0;   // the style plane of (n, ch) is then ch
  hipStream_t st = (hipStream_t)stream;

  if (efdm_fused(mc, ms, chunk)) {
    const int pc = (int)pow2_padded(mc), ps = (int)pow2_padded(ms);
    const int pmax = pc > ps ? pc : ps;
    const size_t lds = (size_t)4 * pmax + (size_t)4 * pc;
    const int e = allow_lds(efdm_fused_kernel, lds);
    if (e) return e;
    hipLaunchKernelGGL(efdm_fused_kernel, dim3((unsigned)planes), dim3(sort_threads(pmax)), lds, st, content, style,
                       out, c, shared, (int)mc, (int)ms, pc, ps, a, copy);
    return (int)hipGetLastError();
  }

  if (chunk == 0) chunk = kAutoChunk;
  if (!workspace) return AST_E_NULLPTR;
  const EfdmWs w = efdm_ws(workspace, planes, splanes, mc, ms);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  if (((uintptr_t)workspace & 3) != 0) return AST_E_UNSUPPORTED;
  if (!general_fits(planes, mc, chunk) || !general_fits(splanes, ms, chunk)) return AST_E_SHAPE;
  const SortWs wc_ = sort_ws(w.content, planes, mc, true), ws_ = sort_ws(w.style, splanes, ms, false);
  uint32_t *ck = nullptr, *sk = nullptr;
  int *ci = nullptr, *si = nullptr;
  int e = sort_general<true>(content, planes, mc, chunk, wc_.key[0], wc_.key[1], wc_.idx[0], wc_.idx[1], st, &ck, &ci);
  if (e) return e;
  e = sort_general<false>(style, splanes, ms, chunk, ws_.key[0], ws_.key[1], nullptr, nullptr, st, &sk, &si);
  if (e) return e;
  const int64_t bps = (mc + kMergeThreads - 1) / kMergeThreads;
  hipLaunchKernelGGL(efdm_scatter_kernel, dim3((unsigned)(planes * bps)), dim3(kMergeThreads), 0, st, content,
                     (const int*)ci, (const uint32_t*)sk, out, c, shared, mc, ms, bps, a, copy);
  return (int)hipGetLastError();
}

int ast_efdm_f32(const float* content, const float* style, float* out, int n, int ns, int c, int hc, int wc, int hs,
                 int ws, double alpha, void* workspace, long long workspace_bytes, void* stream) {
  return ast_efdm_ex_f32(content, style, out, n, ns, c, hc, wc, hs, ws, alpha, 0, workspace, workspace_bytes, stream);
}

long long ast_plane_sort_workspace_bytes(long long planes, long long m, int want_index, int chunk) {
  if (!planes_ok(planes, m)) return AST_E_SHAPE;
  if (!chunk_ok(chunk)) return AST_E_UNSUPPORTED;
  if (chunk == 0 && m <= AST_EFDM_FUSED_MAX) return 0;
  return sort_ws(nullptr, planes, m, want_index != 0).bytes;
}

int ast_plane_sort_f32(const float* x, float* sorted, int* index_or_null, long long planes, long long m, int chunk,
                       void* workspace, long long workspace_bytes, void* stream) {
  if (!x || !sorted) return AST_E_NULLPTR;
  if (!planes_ok(planes, m)) return AST_E_SHAPE;
  if (!chunk_ok(chunk)) return AST_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const bool want_index = index_or_null != nullptr;

  if (chunk == 0 && m <= AST_EFDM_FUSED_MAX) {
    const int P = (int)pow2_padded(m);
    const size_t lds = (size_t)P * (want_index ? 6 : 4);
    const int e = want_index ? allow_lds(plane_sort_fused_kernel<true>, lds)
                             : allow_lds(plane_sort_fused_kernel<false>, lds);
    if (e) return e;
    if (want_index)
      hipLaunchKernelGGL(plane_sort_fused_kernel<true>, dim3((unsigned)planes), dim3(sort_threads(P)), lds, st, x,
                         sorted, index_or_null, (int)m, P);
    else
      hipLaunchKernelGGL(plane_sort_fused_kernel<false>, dim3((unsigned)planes), dim3(sort_threads(P)), lds, st, x,
                         sorted, index_or_null, (int)m, P);
    return (int)hipGetLastError();
  }

  if (chunk == 0) chunk = kAutoChunk;
  if (!workspace) return AST_E_NULLPTR;
  const SortWs w = sort_ws(workspace, planes, m, want_index);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  if (((uintptr_t)workspace & 3) != 0) return AST_E_UNSUPPORTED;
  if (!general_fits(planes, m, chunk)) return AST_E_SHAPE;
  uint32_t* kr = nullptr;
  int* ir = nullptr;
  int e = want_index ? sort_general<true>(x, planes, m, chunk, w.key[0], w.key[1], w.idx[0], w.idx[1], st, &kr, &ir)
                     : sort_general<false>(x, planes, m, chunk, w.key[0], w.key[1], nullptr, nullptr, st, &kr, &ir);
  if (e) return e;
  const int64_t total = planes * m;
  const int64_t want = (total + kMergeThreads - 1) / kMergeThreads;
  const unsigned blocks = (unsigned)(want < 65536 ? want : 65536);
  if (want_index)
    hipLaunchKernelGGL(emit_sorted_kernel<true>, dim3(blocks), dim3(kMergeThreads), 0, st, (const uint32_t*)kr,
                       (const int*)ir, sorted, index_or_null, total);
  else
    hipLaunchKernelGGL(emit_sorted_kernel<false>, dim3(blocks), dim3(kMergeThreads), 0, st, (const uint32_t*)kr,
                       (const int*)ir, sorted, index_or_null, total);
  return (int)hipGetLastError();
}

}  // extern "C"
