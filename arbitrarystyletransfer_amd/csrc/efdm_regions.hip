// Regional exact feature distribution matching for gfx950: EFDM (efdm.hip) per region of a label map,
// towards a per-region mix of a bank of styles. The reference has no counterpart.
//
// Definition (include/ast_hip.h states it in full). For sample n, channel ch and region k: the content
// pixel of stable ascending rank r among the Mc_k pixels labelled k takes, from every style s of
// non-zero weight, the value S_{s,k}[((2r + 1) * Ms_{s,k}) / (2 * Mc_k)] of that style's sorted values
// (of the whole plane, or with style labels of the style's own region k); the target is the weighted
// sum of those values in ascending s, which is the 1-D Wasserstein barycentre of the styles'
// distributions. Order and keys are those of efdm.hip (sort.h).
//
// The label map is shared by the channels of a sample and the bank by the batch, so every plane is
// sorted once, whatever K and S:
//   bank sort  one workgroup per style plane (s, ch): lds_sort of the (key, index) pairs, then a stable
//              partition by label. Every thread owns 8 or 16 consecutive sorted positions, counts their
//              labels, and one workgroup scan gives, for every position, the number of earlier positions
//              with the same label; the position's value goes to offset(label) + that count. The
//              counts are 16-bit fields (a plane has at most 16384 elements) packed four to a 64-bit
//              word, so the scan of 8 regions is the scan of two words; the pass-through class (label
//              >= K, stored last) needs no counter: its count is the position minus the other eight.
//              Without style labels it is the plain value sort.
//   apply      one workgroup per content plane (n, ch): the same pair sort and scan give rank[i], the
//              rank of pixel i inside its own region, and the region sizes Mc_k (the scan's totals);
//              then a coalesced pass over i gathers the bank values of the region's used styles,
//              mixes, blends and stores. The (weight, bank offset, Ms_{s,k}) rows of the used styles are
//              compacted per region in LDS once per workgroup.
// LDS: 6 * P bytes for the pairs (the 16-bit ranks take the place of the keys once the sort is done)
// plus 8.5 KB of scan scratch and tables: 104 KB at P = 16384, allowed per kernel above 64 KB.
// No atomics, no host synchronisation, no allocation; no launch parameter depends on the contents of a
// label map or of the mix, so a captured graph replays with other labels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ast_hip.h"
#include "sort.h"
#include "ws.h"

using namespace ast_sort;

namespace {

constexpr int kRows = AST_MAX_REGIONS * AST_MAX_STYLE_ROWS;   // (region, style) rows of the apply's tables
constexpr int kScanBytes = 2 * 8 * (kMaxThreads / 64);        // two 64-bit words per wave
constexpr int kTableBytes = kRows * (8 + 4 + 4) + 2 * 4 * AST_MAX_REGIONS;
constexpr size_t kMaxLds = 160 * 1024;                        // LDS of a gfx950 CU

__device__ __forceinline__ float blend(float c, float t, float alpha) { return c + alpha * (t - c); }

// t + w * v as an fp32 product and an fp32 sum: never contracted into an fma, so the mix is the same
// arithmetic on any device (and what a plain fp32 restatement computes)
__device__ __forceinline__ float add_product(float t, float w, float v) {
#pragma clang fp contract(off)
  const float p = w * v;
  return t + p;
}

__device__ __forceinline__ float product(float w, float v) {
#pragma clang fp contract(off)
  return w * v;
}

__device__ __forceinline__ uint32_t field(uint64_t w, uint32_t k) { return (uint32_t)(w >> (16 * k)) & 0xffffu; }

// The label scan over the sorted positions of a plane. Position p < m holds element idx[p], whose class
// is min(lab[idx[p]], K) (K = pass-through; the padding positions p >= m count as K too). Thread t owns
// positions [t * per, (t + 1) * per), per = P / blockDim.x <= 16.
struct LabelScan {
  uint64_t cls;        // the classes of the thread's positions, 4 bits each
  uint64_t ex0, ex1;   // 16-bit fields: positions before the thread's first with class 0..3 / 4..7
  uint64_t tot0, tot1; // the same over the whole plane: the region sizes
};

// sh: 2 words per wave. A barrier follows the last read of idx; none follows the last read of sh.
__device__ __forceinline__ LabelScan label_scan(const uint16_t* idx, const unsigned char* __restrict__ lab, int m,
                                                int P, uint32_t K, uint64_t* sh) {
  const int per = P / (int)blockDim.x;
  const int p0 = (int)threadIdx.x * per;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  LabelScan r;
  r.cls = 0;
  uint64_t c0 = 0, c1 = 0;
  for (int e = 0; e < per; ++e) {
    const int p = p0 + e;
    uint32_t k = K;
    if (p < m) {
      const uint32_t l = lab[idx[p]];
      k = l < K ? l : K;
    }
    r.cls |= (uint64_t)k << (4 * e);
    if (k < 4) c0 += 1ull << (16 * k);
    else if (k < K) c1 += 1ull << (16 * (k - 4));
  }
  uint64_t i0 = c0, i1 = c1;   // inclusive over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t a = __shfl_up((unsigned long long)i0, o, 64), b = __shfl_up((unsigned long long)i1, o, 64);
    if (lane >= o) i0 += a, i1 += b;
  }
  if (lane == 63) sh[2 * wave] = i0, sh[2 * wave + 1] = i1;
  __syncthreads();
  uint64_t b0 = 0, b1 = 0;
  r.tot0 = 0, r.tot1 = 0;
  for (int w = 0; w < waves; ++w) {
    const uint64_t a = sh[2 * w], b = sh[2 * w + 1];
    if (w < wave) b0 += a, b1 += b;
    r.tot0 += a, r.tot1 += b;
  }
  r.ex0 = b0 + i0 - c0, r.ex1 = b1 + i1 - c1;
  return r;
}

extern __shared__ __align__(16) unsigned char efdm_regions_smem[];

// Plane (s, ch) of x [S, C, m] in the order (min(label, K), key, index) into sorted [S, C, m], and (the
// workgroups of channel 0) count [S, K]. LAB == false: no labels, the plain value sort, count = (m, 0, ...).
template <bool LAB>
__global__ __launch_bounds__(kMaxThreads) void bank_sort_kernel(const float* __restrict__ x,
                                                                const unsigned char* __restrict__ labels,
                                                                float* __restrict__ sorted, int* __restrict__ count,
                                                                int c, int m, int P, int K) {
  uint32_t* key = reinterpret_cast<uint32_t*>(efdm_regions_smem);
  uint16_t* idx = reinterpret_cast<uint16_t*>(key + P);
  const int64_t p = blockIdx.x;
  const int64_t s = p / c;
  float* o = sorted + p * m;
  lds_fill<LAB>(x + p * m, m, key, idx, P);
  lds_sort<LAB>(key, idx, P);
  if (!LAB) {
    for (int r = threadIdx.x; r < m; r += blockDim.x) o[r] = from_key(key[r]);
    if (p % c == 0 && (int)threadIdx.x < K) count[s * K + threadIdx.x] = threadIdx.x == 0 ? m : 0;
    return;
  }
  uint64_t* sh = reinterpret_cast<uint64_t*>(efdm_regions_smem + (size_t)6 * P);
  const LabelScan sc = label_scan(idx, labels + s * m, m, P, (uint32_t)K, sh);
  if (p % c == 0 && (int)threadIdx.x < K)
    count[s * K + threadIdx.x] = (int)(threadIdx.x < 4 ? field(sc.tot0, threadIdx.x) : field(sc.tot1, threadIdx.x - 4));
  // where every class starts, and from there where this thread's first element of the class goes: at
  // most m <= 16384, so the sums stay inside their 16-bit fields
  uint64_t st0 = 0, st1 = 0;
  uint32_t run = 0, before = 0;   // before: the thread's earlier positions of classes 0..7
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) st0 |= (uint64_t)run << (16 * k), run += field(sc.tot0, k), before += field(sc.ex0, k);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) st1 |= (uint64_t)run << (16 * k), run += field(sc.tot1, k), before += field(sc.ex1, k);
  st0 += sc.ex0, st1 += sc.ex1;
  const int per = P / (int)blockDim.x;
  const int p0 = (int)threadIdx.x * per;
  uint32_t pass = run + ((uint32_t)p0 - before);   // the earlier positions are all real when p0 < m
  for (int e = 0; e < per; ++e) {
    const int q = p0 + e;
    if (q >= m) break;
    const uint32_t k = (uint32_t)(sc.cls >> (4 * e)) & 15u;
    uint32_t pos;
    if (k < 4) pos = field(st0, k), st0 += 1ull << (16 * k);
    else if (k < (uint32_t)K) pos = field(st1, k - 4), st1 += 1ull << (16 * (k - 4));
    else pos = pass++;
    o[pos] = from_key(key[q]);
  }
}

// One workgroup per content plane (n, ch). bank [S, C, ms] and count [S, K] are the bank sort's outputs
// (regional != 0: the bank is partitioned by style label; else every region takes the whole plane and
// count is not read). mix [1 or N, K, S], mix_stride = 0 or K * S.
__global__ __launch_bounds__(kMaxThreads) void efdm_regions_kernel(
    const float* __restrict__ content, const unsigned char* __restrict__ labels, const float* __restrict__ bank,
    const int* __restrict__ count, const float* __restrict__ mix, float* __restrict__ out, int c, int mc, int pc, int ms,
    int K, int S, int mix_stride, int regional, float alpha, int copy) {
  uint32_t* key = reinterpret_cast<uint32_t*>(efdm_regions_smem);
  uint16_t* idx = reinterpret_cast<uint16_t*>(key + pc);
  uint16_t* rank = reinterpret_cast<uint16_t*>(key);   // the keys are dead once the sort is done
  unsigned char* tail = efdm_regions_smem + (size_t)6 * pc;
  uint64_t* sh = reinterpret_cast<uint64_t*>(tail);
  int64_t* t_base = reinterpret_cast<int64_t*>(tail + kScanBytes);   // row k * S + j: start of S_{s,k} in the bank
  float* t_w = reinterpret_cast<float*>(t_base + kRows);             //                its weight
  int* t_ms = reinterpret_cast<int*>(t_w + kRows);                   //                Ms_{s,k}
  int* t_used = t_ms + kRows;                 // [K]: the rows of region k, -1: the region passes through
  int* t_mc = t_used + AST_MAX_REGIONS;       // [K]: Mc_k
  const int64_t p = blockIdx.x;
  const int64_t n = p / c, ch = p % c;
  const float* x = content + p * mc;
  const unsigned char* lab = labels + n * mc;
  float* o = out + p * mc;

  // every (region, style) row, dense; compacted to the used styles below (lds_fill ends with a barrier)
  for (int e = threadIdx.x; e < K * S; e += blockDim.x) {
    const int k = e / S, s = e % S;
    int64_t off = 0;
    int msk = ms;
    if (regional) {
      for (int q = 0; q < k; ++q) off += count[s * K + q];
      msk = count[s * K + k];
    }
    t_w[e] = mix[n * mix_stride + e];
    t_ms[e] = msk;
    t_base[e] = ((int64_t)s * c + ch) * ms + off;
  }
  lds_fill<true>(x, mc, key, idx, pc);
  lds_sort<true>(key, idx, pc);
  const LabelScan sc = label_scan(idx, lab, mc, pc, (uint32_t)K, sh);

  if ((int)threadIdx.x < K) {
    const int k = threadIdx.x;
    int used = 0;
    bool valid = true;
    for (int s = 0; s < S; ++s) {
      const float w = t_w[k * S + s];
      if (w != 0.f) {   // in place: row `used` <= s
        const int msk = t_ms[k * S + s];
        valid = valid && msk > 0;
        t_w[k * S + used] = w, t_ms[k * S + used] = msk, t_base[k * S + used] = t_base[k * S + s];
        ++used;
      }
    }
    t_used[k] = valid ? used : -1;
    t_mc[k] = (int)(k < 4 ? field(sc.tot0, k) : field(sc.tot1, k - 4));
  }
  {
    uint64_t r0 = sc.ex0, r1 = sc.ex1;
    const int per = pc / (int)blockDim.x;
    const int p0 = (int)threadIdx.x * per;
    for (int e = 0; e < per; ++e) {
      const int q = p0 + e;
      if (q >= mc) break;
      const uint32_t k = (uint32_t)(sc.cls >> (4 * e)) & 15u;
      uint32_t r = 0;
      if (k < 4) r = field(r0, k), r0 += 1ull << (16 * k);
      else if (k < (uint32_t)K) r = field(r1, k - 4), r1 += 1ull << (16 * (k - 4));
      rank[idx[q]] = (uint16_t)r;
    }
  }
  __syncthreads();

  for (int i = threadIdx.x; i < mc; i += blockDim.x) {
    const float cv = x[i];
    const int k = lab[i];
    float v = cv;
    const int used = k < K ? t_used[k] : -1;
    if (used >= 0) {
      const uint32_t r = rank[i], mk = (uint32_t)t_mc[k];
      const int row = k * S;
      float t = 0.f;
      for (int j = 0; j < used; ++j) {
        const uint32_t msk = (uint32_t)t_ms[row + j];
        // (2r + 1) * Ms < 2^30 for planes <= AST_EFDM_FUSED_MAX: 32-bit arithmetic is exact here
        const uint32_t at = msk == mk ? r : ((2u * r + 1u) * msk) / (2u * mk);
        const float sv = bank[t_base[row + j] + at];
        if (used == 1) t = sv;                                   // the style value's bits
        else if (j == 0) t = product(t_w[row], sv);
        else t = add_product(t, t_w[row + j], sv);
      }
      v = copy ? t : blend(cv, t, alpha);
    }
    o[i] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------

int pow2_padded(int64_t m) {   // the LDS sort length of m <= AST_EFDM_FUSED_MAX elements
  int p = kTile;
  while (p < m) p <<= 1;
  return p;
}

int sort_threads(int P) { return P / kE < kMaxThreads ? P / kE : kMaxThreads; }

size_t bank_lds(int P, bool lab) { return lab ? (size_t)6 * P + kScanBytes : (size_t)4 * P; }

size_t apply_lds(int P) { return (size_t)6 * P + kScanBytes + kTableBytes; }

template <typename Kern>
int allow_lds(Kern kern, size_t lds) {   // dynamic LDS above 64 KB has to be allowed per kernel
  if (lds <= 64 * 1024) return 0;
  return (int)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// `planes` planes of h * w elements for one workgroup each: 0, or the negative code
int planes_check(int64_t planes, int h, int w) {
  if (planes <= 0 || h <= 0 || w <= 0 || planes > 0x7fffffffLL) return AST_E_SHAPE;
  if ((int64_t)h * w > AST_EFDM_FUSED_MAX) return AST_E_UNSUPPORTED;
  return 0;
}

int regions_check(int n, int c, int hc, int wc, int regions, int styles, int hs, int ws) {
  if (n <= 0 || c <= 0 || regions < 1 || regions > AST_MAX_REGIONS || styles < 1 || styles > AST_MAX_STYLE_ROWS)
    return AST_E_SHAPE;
  const int e = planes_check((int64_t)n * c, hc, wc);
  return e ? e : planes_check((int64_t)styles * c, hs, ws);
}

int launch_bank_sort(const float* x, const unsigned char* labels, float* sorted, int* count, int s, int c, int m,
                     int regions, hipStream_t st) {
  const int P = pow2_padded(m);
  const size_t lds = bank_lds(P, labels != nullptr);
  const dim3 grid((unsigned)((int64_t)s * c)), block(sort_threads(P));
  if (labels)
    hipLaunchKernelGGL(bank_sort_kernel<true>, grid, block, lds, st, x, labels, sorted, count, c, m, P, regions);
  else
    hipLaunchKernelGGL(bank_sort_kernel<false>, grid, block, lds, st, x, labels, sorted, count, c, m, P, regions);
  return (int)hipGetLastError();
}

int allow_bank_sort(int m, bool lab) {
  const size_t lds = bank_lds(pow2_padded(m), lab);
  if (lds > kMaxLds) return AST_E_UNSUPPORTED;
  return lab ? allow_lds(bank_sort_kernel<true>, lds) : allow_lds(bank_sort_kernel<false>, lds);
}

// The whole op's workspace: [sorted bank | region counts of the bank]
struct RegionsWs {
  float* bank;
  int* count;
  int64_t bytes;
};

RegionsWs regions_ws(void* base, int c, int regions, int styles, int hs, int ws) {
  ast_ws::Walk wk(base);
  return {wk.take<float>((int64_t)4 * styles * c * hs * ws), wk.take<int>((int64_t)4 * styles * regions), wk.off};
}

}  // namespace

extern "C" {

int ast_efdm_region_sort_f32(const float* x, const unsigned char* labels_or_null, float* sorted, int* count, int s,
                             int c, int h, int w, int regions, void* stream) {
  if (!x || !sorted || !count) return AST_E_NULLPTR;
  if (s <= 0 || c <= 0 || regions < 1 || regions > AST_MAX_REGIONS) return AST_E_SHAPE;
  int e = planes_check((int64_t)s * c, h, w);
  if (e) return e;
  e = allow_bank_sort(h * w, labels_or_null != nullptr);
  if (e) return e;
  return launch_bank_sort(x, labels_or_null, sorted, count, s, c, h * w, regions, (hipStream_t)stream);
}

long long ast_efdm_regions_workspace_bytes(int n, int c, int hc, int wc, int regions, int styles, int hs, int ws) {
  const int e = regions_check(n, c, hc, wc, regions, styles, hs, ws);
  return e ? e : regions_ws(nullptr, c, regions, styles, hs, ws).bytes;
}

int ast_efdm_regions_f32(const float* content, const unsigned char* labels, const float* styles,
                         const unsigned char* style_labels_or_null, const float* mix, float* out, int n, int c, int hc,
                         int wc, int regions, int s, int hs, int ws, int mix_n, double alpha, void* workspace,
                         long long workspace_bytes, void* stream) {
  if (!content || !labels || !styles || !mix || !out || !workspace) return AST_E_NULLPTR;
  int e = regions_check(n, c, hc, wc, regions, s, hs, ws);
  if (e) return e;
  if (mix_n != 1 && mix_n != n) return AST_E_SHAPE;
  const RegionsWs w = regions_ws(workspace, c, regions, s, hs, ws);
  if (workspace_bytes < w.bytes) return AST_E_SHAPE;
  if (((uintptr_t)workspace & 3) != 0) return AST_E_UNSUPPORTED;
  const int mc = hc * wc, ms = hs * ws;
  const int pc = pow2_padded(mc);
  const size_t lds = apply_lds(pc);
  if (lds > kMaxLds) return AST_E_UNSUPPORTED;
  const bool regional = style_labels_or_null != nullptr;
  e = allow_bank_sort(ms, regional);
  if (e) return e;
  e = allow_lds(efdm_regions_kernel, lds);
  if (e) return e;
  hipStream_t st = (hipStream_t)stream;
  e = launch_bank_sort(styles, style_labels_or_null, w.bank, w.count, s, c, ms, regions, st);
  if (e) return e;
  hipLaunchKernelGGL(efdm_regions_kernel, dim3((unsigned)((int64_t)n * c)), dim3(sort_threads(pc)), lds, st, content,
                     labels, (const float*)w.bank, (const int*)w.count, mix, out, c, mc, pc, ms, regions, s,
                     mix_n == 1 ? 0 : regions * s, regional ? 1 : 0, (float)alpha, alpha == 1.0 ? 1 : 0);
  return (int)hipGetLastError();
}

}  // extern "C"
