// ------------------------------------------------------------------------------------------------
// Split-bf16 ("bf16x3") implicit GEMM: fp32 accuracy on the bf16 matrix cores.
//
// Every fp32 operand is split exactly into three bf16 terms, x = hi + mid + lo (hi = bf16(x),
// mid = bf16(x - hi), lo = x - hi - mid, which has <= 8 significant bits and so is exact in bf16).
// The product x*w is the sum of the 9 cross products; the 3 dropped ones (mid*lo, lo*mid, lo*lo) are
// below 2^-24 |x w|, i.e. under fp32's own rounding of the product. Six v_mfma_f32_32x32x16_bf16
// (products exact in fp32, fp32 accumulation) therefore give an fp32-accurate conv at 6 x 16 cycles
// per 32x32x16 block against 8 x 64 cycles (32x32x2 f32) for the same block on the fp32 MFMA:
// 2.67x the fp32 matrix peak (2.5 PF / 6 = 419 TF of fp32-equivalent work).
//
// Layout (16-byte units = 8 bf16 channels):
//  * LDS activations [plane][h][src row][src col]: h = which 8 of the chunk's 16 input channels.
//    The A operand of lane l (pixel l&31, channels 8(l>>5)..+7) is one ds_read_b128; 32 lanes read
//    32 consecutive 16-B units per half -> conflict-free under the b128 lane grouping.
//  * LDS weights [plane][tap][h][co]: the B operand of lane l (channel l&31) likewise.
//  * global weight pack (after the fp32 pack, see ast_conv3x3_packed_numel):
//    [chunk of 16 ci][plane][tap][h][cout_pad][8] bf16, so a chunk's slab rows are contiguous.
// The source tile (with halo, zero / reflect padding and the x2 nearest upsample resolved per
// pixel, as in the fp32 kernel) is gathered with dword loads coalesced along x, split on the VALU
// and written once per chunk; the next chunk's loads are in flight during the MFMAs.
// ------------------------------------------------------------------------------------------------
#include <algorithm>
#include "conv_x3.h"

namespace {

using namespace ast_conv;

// fp32 pack [ci_pad8][9][cout_pad] -> split pack [ci16 chunk][plane][tap][h][cout_pad][8]
__global__ void pack_x3_kernel(const float* __restrict__ wp, bf16* __restrict__ ws, int cin_pad8, int cin16,
                               int cout_pad) {
  const int64_t total = (int64_t)cin16 * 9 * cout_pad;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(idx % cout_pad);
    const int64_t rt = idx / cout_pad;
    const int tap = (int)(rt % 9);
    const int ci = (int)(rt / 9);
    const float v = ci < cin_pad8 ? wp[((int64_t)ci * 9 + tap) * cout_pad + co] : 0.f;
    bf16 t[3];
    ast_x3::split3(v, t[0], t[1], t[2]);
    const int kc = ci / kX3K, hh = (ci >> 3) & 1, e = ci & 7;
#pragma unroll
    for (int p = 0; p < 3; ++p)
      ws[((((int64_t)(kc * 3 + p) * 9 + tap) * 2 + hh) * cout_pad + co) * 8 + e] = t[p];
  }
}

template <int RM, int RN>
__device__ __forceinline__ void store_tiles_staged(const ConvArgs& a, const f32x16 (&acc)[RM][RN], int n, int x0,
                                                   int y0, int row0, int n0c, int h, int l32, int lane,
                                                   float* __restrict__ region) {
  constexpr int RP = 36;  // row pitch (floats): 32 px + 4
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    {
      const int co = n0c + j * 32 + l32;
      const float bv = (co < a.Cout && a.bias) ? a.bias[co] : 0.f;
#pragma unroll
      for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(region + (l32 * RM + i) * RP + 8 * g + 4 * h) =
              make_float4(acc[i][j][4 * g] + bv, acc[i][j][4 * g + 1] + bv, acc[i][j][4 * g + 2] + bv,
                          acc[i][j][4 * g + 3] + bv);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes are done
    __builtin_amdgcn_wave_barrier();
    store_region<RM>(a, region, n, x0, y0, row0, n0c + j * 32, lane);
    if (j + 1 < RN) {
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();  // reads of this j done before the next j's writes
    }
  }
}

// M16: the same kernel on v_mfma_f32_16x16x32_bf16 (16 pixels x 16 output channels x K 32). The six
// split products fold into three K-32 MFMAs -- K = (16 channels of one term | 16 of another):
//   [x_hi | x_mid] . [w_hi ; w_hi]  = x_hi w_hi  + x_mid w_hi
//   [x_hi | x_lo ] . [w_mid; w_hi]  = x_hi w_mid + x_lo w_hi
//   [x_hi | x_mid] . [w_lo ; w_mid] = x_hi w_lo  + x_mid w_mid
// -- the same products and cycles per FLOP as the 32x32x16 form; on random data the chip holds a
// higher clock with the 16x16 shape (MI355X_MICROARCH.md, DVFS give-back item 7). A lane's k-group
// g = lane >> 4 selects the term plane (g < 2: the first, else the second) and the 8-channel half
// (g & 1), so every operand is still one ds_read_b128 from the same LDS images.
// PER (M16 only): persistent form -- gridDim.x workgroups walk the blocks b = blockIdx.x + k gridDim.x
// (gridDim.x a multiple of 8, so b % 8 and the XCD stay fixed), the same code per block; between
// blocks an LDS-only barrier (the epilogue regions are read before the next prologue writes the
// tiles), so the epilogue's global stores drain under the next block's prologue instead of
// holding the CU until the workgroup retires.
template <int WM, int RM, int RN, int UP, int OCC, bool M16 = false, bool PER = false>
__global__ __launch_bounds__(WM * 64, OCC) void conv3x3_x3_kernel(ConvArgs a) {
  using C = X3Cfg<WM, RM, RN, UP>;
  constexpr int NT = C::NT, TH = C::TH, BN = C::BN, SR = C::SR, SC = C::SC, A_PLANE = C::A_PLANE;
  constexpr int HS = C::HS, A_ITEMS = C::A_ITEMS;
  constexpr int A_T = C::A_T, B_T = C::B_T, NS = C::NS;
  static_assert(RM % 2 == 0, "even rows per wave (pool windows, upsample row pairs)");
  extern __shared__ __attribute__((aligned(16))) u32x4 x3_smem[];
  u32x4* As = x3_smem;
  u32x4* Bs = x3_smem + C::A_UNITS;
  // M16: [lo plane][hi + mid planes, buffer 0][hi + mid planes, buffer 1] after the A tile
  u32x4* Blo = x3_smem + C::A_UNITS;
  u32x4* Bhm0 = Blo + 18 * BN;

#if X3_STAMP
  unsigned st0 = 0, st1 = 0, st2 = 0;
  {
    const int lane = threadIdx.x & 63;  // the block loop declares its own
    X3_ST(0);
  }
#endif
  static_assert(!PER || M16, "persistent form of the M16 kernel only");
  const int ntl = a.tiles_x * a.tiles_y * a.N, ngr = (a.Cout + BN - 1) / BN;
  const int nblk = (ntl + 7) / 8 * 8 * ngr;
  for (int bid = blockIdx.x;; bid += gridDim.x) {
  if constexpr (PER) {
    if (bid >= nblk) break;
    if (bid != (int)blockIdx.x) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // PER: the thread index laundered per block, so nothing derived from it is hoisted out of the
  // block loop and held live through it (that spilled 60-80 VGPRs); recomputing is a few VALU ops
  int tid_ = threadIdx.x;
  if constexpr (PER) asm volatile("" : "+v"(tid_));
  const int tid = tid_, wm = tid >> 6, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
  int t, grp;
  if (!decode_block(bid, ntl, ngr, t, grp)) {
    if constexpr (PER) continue;
    return;
  }
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int x0 = tx * TW, y0 = ty * TH;
  const int sx0 = x0 / UP, sy0 = y0 / UP - 1;
  const int n0 = grp * BN;
  const int Hin = a.Hin, Win = a.Win, plane_in = Hin * Win;
  const float* __restrict__ xin =
      n < a.nsplit ? a.x + (int64_t)n * a.Cin * plane_in : a.x2 + (int64_t)(n - a.nsplit) * a.Cin * plane_in;
  const u32x4* __restrict__ wsplit =
      reinterpret_cast<const u32x4*>(a.wp + x3_split_offset(a.Cin, a.Cout));
  const int nch = (a.Cin + kX3K - 1) / kX3K;
  const int64_t chunk_units = (int64_t)C::B_ROWS * a.cout_pad;

  // gather items: (h, source row, source column), fixed per thread for every chunk. Loads are
  // raw buffer loads: per-chunk descriptor (wave-uniform), per-item 32-bit voffset (pixel + 8h
  // channels), channel j in soffset: no per-load address arithmetic. A zero-padding pixel gets an
  // out-of-range voffset, which the buffer range check turns into 0.
  unsigned g_off[A_T], g_pix[A_T];
  int g_lds[A_T], g_h[A_T];
  bool g_ok[A_T];
#pragma unroll
  for (int i = 0; i < A_T; ++i) {
    const int e = min(tid + i * NT, A_ITEMS - 1);
    const int c = e % SC, rest = e / SC, r = rest % SR, hh = rest / SR;
    const int sy = src_index<UP>(sy0 + r, Hin, a.reflect), sx = src_index<UP>(sx0 - 1 + c, Win, a.reflect);
    g_ok[i] = sy >= 0 && sx >= 0;
    g_pix[i] = (unsigned)(max(sy, 0) * Win + max(sx, 0));
    g_off[i] = g_ok[i] ? 4u * (unsigned)(8 * hh * plane_in) + 4u * g_pix[i] : 0x7ffffff0u;
    g_lds[i] = hh * HS + r * SC + c;
    g_h[i] = hh;
  }
  const int plane_b = 4 * plane_in;
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u32x4*>(wsplit), 0, (int)min<int64_t>(0x7fffffff, (int64_t)nch * chunk_units * 16), 0x00020000);
  int b_src[B_T], b_dst[B_T];
#pragma unroll
  for (int i = 0; i < B_T; ++i) {
    const int u = min(tid + i * NT, C::B_UNITS - 1), row = u / BN, j = u - row * BN;
    b_src[i] = 16 * (row * a.cout_pad + n0 + j);
    b_dst[i] = u;
  }
  float ra[A_T][8];
  u32x4 rb[M16 ? 1 : B_T];
  bf16x8 pv[M16 ? A_T : 1][3];
  // channel ci0 + 8h + j of item i; a partial last chunk clamps the channel (values masked at store)
#define X3_LOAD_A(KC, I0, I1)                                                                           \
  {                                                                                                     \
    const int ci0 = (KC) * kX3K;                                                                        \
    if (ci0 + kX3K <= a.Cin) {                                                                          \
      const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(                              \
          const_cast<float*>(xin + (int64_t)ci0 * plane_in), 0, kX3K * plane_b, 0x00020000);           \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                     \
        _Pragma("unroll") for (int i = (I0); i < (I1); ++i)                                             \
          ra[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)g_off[i], j * plane_b, 0)); \
    } else {                                                                                            \
      _Pragma("unroll") for (int i = (I0); i < (I1); ++i)                                               \
        _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                   \
          ra[i][j] = xin[(int64_t)min(ci0 + 8 * g_h[i] + j, a.Cin - 1) * plane_in + g_pix[i]];          \
    }                                                                                                   \
  }
#define X3_LOAD_B(KC)                                                                                   \
  _Pragma("unroll") for (int i = 0; i < (M16 ? 0 : B_T); ++i)                                           \
    rb[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_src[i], (int)((KC) * chunk_units * 16), 0));
  // M16: the weight slab goes global -> LDS by LDS-DMA (global_load_lds_dwordx4, one lane-linear
  // 1-KiB piece of the slab per wave-instruction, no VGPRs and no ds_write), issued right after the
  // barrier that frees Bs; the barrier after the A tile's writes waits for it (vmcnt(0))
  // slab rows (plane, tap, half): hi + mid planes = rows 0-35, lo plane = rows 36-53
  static_assert((36 * BN) % 64 == 0 && (18 * BN) % 64 == 0, "whole 1-KiB pieces");
  constexpr int HM_PIECES = 36 * BN / 64, LO_PIECES = 18 * BN / 64;
#define X3_DMA_ROWS(KC, ROW0, NPIECES, DST)                                                             \
  _Pragma("unroll") for (int i = 0; i < ((NPIECES) + WM - 1) / WM; ++i) {                               \
    const int piece = wm + i * WM;                                                                      \
    if (piece < (NPIECES)) {                                                                            \
      const int u = piece * 64 + lane, row = u / BN, j = u - row * BN;                                  \
      const u32x4* src = wsplit + (int64_t)(KC) * chunk_units + (int64_t)((ROW0) + row) * a.cout_pad + n0 + j; \
      __builtin_amdgcn_global_load_lds((const void*)src,                                                \
                                       (__attribute__((address_space(3))) void*)((DST) + piece * 64), 16, 0, 0); \
    }                                                                                                   \
  }
#define X3_DMA_HM(KC) X3_DMA_ROWS(KC, 0, HM_PIECES, Bhm0 + ((KC) & 1) * 36 * BN)
#define X3_DMA_LO(KC) X3_DMA_ROWS(KC, 36, LO_PIECES, Blo)
  // M16: the gathered x split into its term planes in registers (before the barrier, in the slack of
  // a wave that finished its MFMAs early), written after it
#define X3_SPLIT_A(KC)                                                                                  \
  _Pragma("unroll") for (int i = 0; i < A_T; ++i) {                                                     \
    if ((KC) * kX3K + kX3K > a.Cin) { /* partial last chunk: padding and channels past Cin */            \
      const int cn = a.Cin - (KC) * kX3K - 8 * g_h[i];                                                  \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) ra[i][j] = (g_ok[i] && j < cn) ? ra[i][j] : 0.f;     \
    }                                                                                                   \
    ast_x3::split8(ra[i], pv[i][0], pv[i][1], pv[i][2]);                                                \
  }
#define X3_WRITE_A                                                                                      \
  _Pragma("unroll") for (int i = 0; i < A_T; ++i)                                                       \
    if (tid + i * NT < A_ITEMS)                                                                         \
      _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                     \
        As[p * A_PLANE + g_lds[i]] = __builtin_bit_cast(u32x4, pv[i][p]);
#define X3_LOAD(KC)         \
  {                         \
    X3_LOAD_A(KC, 0, A_T);  \
    X3_LOAD_B(KC);          \
  }
  // split into the three term planes (ast_x3::split8: paired conversions, bit-identical to split3)
#define X3_STORE(KC)                                                                                    \
  {                                                                                                     \
    _Pragma("unroll") for (int i = 0; i < A_T; ++i) {                                                   \
      if (tid + i * NT < A_ITEMS) {                                                                     \
        if ((KC) * kX3K + kX3K > a.Cin) { /* partial last chunk: padding and channels past Cin */        \
          const int cn = a.Cin - (KC) * kX3K - 8 * g_h[i];                                              \
          _Pragma("unroll") for (int j = 0; j < 8; ++j) ra[i][j] = (g_ok[i] && j < cn) ? ra[i][j] : 0.f; \
        }                                                                                               \
        bf16x8 pv[3];                                                                                   \
        ast_x3::split8(ra[i], pv[0], pv[1], pv[2]);                                                     \
        _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                   \
          As[p * A_PLANE + g_lds[i]] = __builtin_bit_cast(u32x4, pv[p]);                                \
      }                                                                                                 \
    }                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < B_T; ++i)                                                     \
      if (tid + i * NT < C::B_UNITS) Bs[b_dst[i]] = rb[i];                                              \
  }

  constexpr int Q = 2 * RN;  // M16: 16-channel column tiles per wave
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  f32x16 acc[M16 ? 1 : RM][M16 ? 1 : RN];
  f32x4v acc16[M16 ? RM : 1][M16 ? 2 : 1][M16 ? Q : 1];
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc16[i][pt][q] = f32x4v{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }

  int acol[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) acol[kx] = ((x0 + l32 + kx - 1) >> (UP - 1)) - sx0 + 1;
  const int srow0 = wm * RM / UP;
  // M16 lane roles: pixel / channel l16 of a 16-tile, k-group g16 -> (term plane, 8-channel half)
  const int l16 = lane & 15, g16 = lane >> 4, hh16 = g16 & 1;
  int acol16[2][3];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) acol16[pt][kx] = ((x0 + 16 * pt + l16 + kx - 1) >> (UP - 1)) - sx0 + 1;
  const int apl1 = (g16 < 2 ? 0 : 1) * A_PLANE, apl2 = (g16 < 2 ? 0 : 2) * A_PLANE;  // [hi|mid], [hi|lo]

  if constexpr (M16) {
    X3_DMA_HM(0);
    X3_DMA_LO(0);
    X3_LOAD_A(0, 0, A_T);
    X3_SPLIT_A(0);
    X3_WRITE_A;
  } else {
    X3_LOAD(0);
    X3_STORE(0);
  }
  __syncthreads();
  X3_ST(1);
  static_assert(A_T < 9, "one gather item per tap of the MFMA phase");
  for (int kc = 0; kc < nch; ++kc) {
    if (!M16 && kc + 1 < nch) X3_LOAD(kc + 1);
    __builtin_amdgcn_sched_barrier(0);
    X3_ST(2 + 4 * kc);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (M16) {
      // Software-pipelined MFMA phase (round 5): steps s = (kx, ky, row i), kx outermost; the LDS operands of step s + 1 (its A fragments and, when it opens a
      // tap, the tap's B fragments) are read while step s's MFMAs run. The stamps showed the wave
      // that finishes a chunk last, alone on its SIMD, issuing MFMAs at ~70% of the pipe rate: each
      // step waited on reads issued just before it (profiles/r05_x3_stamps.txt). Same products in
      // the same order per accumulator as the round-4 loop: bit-identical. A step opens with an MFMA
      // and its reads follow, one per MFMA: with a read first, every step began by waiting
      // (lgkmcnt(0)) for a read issued one instruction earlier (profiles/r10_x3_step_boundaries.txt).
      constexpr int NSTEP = 9 * RM;
      bf16x8 gb[2][3][Q];  // B fragments (g1, g2, g3) of a tap, by tap parity
      bf16x8 fa[2][2][2];  // A fragments (f1, f2) x pixel tile of a step, by step parity
      // this chunk's B planes: g1 = [hi; hi], g2 = [mid | hi; hi], g3 = [lo; mid] by k-group
      const u32x4* __restrict__ bhm = Bhm0 + (kc & 1) * 36 * BN;
      const u32x4* __restrict__ bp1 = bhm;                                         // hi
      const u32x4* __restrict__ bp2 = bhm + (g16 < 2 ? 18 * BN : 0);               // mid | hi
      const u32x4* __restrict__ bp3 = g16 < 2 ? Blo : bhm + 18 * BN;               // lo | mid
#define X3P_READ_B(BUF, T)                                                                              \
      {                                                                                                 \
        const int tap_ = ((T) % 3) * 3 + (T) / 3;                                                       \
        _Pragma("unroll") for (int q = 0; q < Q; ++q) {                                                 \
          const int col = q * 16 + l16;                                                                 \
          gb[BUF][0][q] = __builtin_bit_cast(bf16x8, bp1[(tap_ * 2 + hh16) * BN + col]);               \
          gb[BUF][1][q] = __builtin_bit_cast(bf16x8, bp2[(tap_ * 2 + hh16) * BN + col]);               \
          gb[BUF][2][q] = __builtin_bit_cast(bf16x8, bp3[(tap_ * 2 + hh16) * BN + col]);               \
        }                                                                                               \
      }
#define X3P_READ_A(BUF, S)                                                                              \
      {                                                                                                 \
        const int t_ = (S) / RM, i_ = (S) % RM, kx_ = t_ / 3, ky_ = t_ % 3;                             \
        const int srow = hh16 * HS + (srow0 + x3_srel<UP>(i_, ky_)) * SC;                               \
        _Pragma("unroll") for (int pt = 0; pt < 2; ++pt) {                                              \
          fa[BUF][0][pt] = __builtin_bit_cast(bf16x8, As[apl1 + srow + acol16[pt][kx_]]);               \
          fa[BUF][1][pt] = __builtin_bit_cast(bf16x8, As[apl2 + srow + acol16[pt][kx_]]);               \
        }                                                                                               \
      }
      X3P_READ_B(0, 0);
      X3P_READ_A(0, 0);
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        const int t = st / RM, i = st % RM, sb = st & 1, tb = t & 1;
        X3_ST_STEP(kc, nch, st);
        // the next chunk's global loads, spread over the first taps (one gather item per tap):
        // issued all at once they queued behind the CU's memory pipeline for ~3k cycles per chunk
        // with no MFMA issued (scripts/x3_stamps.py, profiles/r05_x3_stamps.txt)
        if (i == 0 && t < A_T && kc + 1 < nch) {
          __builtin_amdgcn_sched_barrier(0);
          X3_LOAD_A(kc + 1, t, t + 1)
          __builtin_amdgcn_sched_barrier(0);
        }
        // the next chunk's hi + mid weight planes into the other buffer (LDS-DMA, no VGPRs)
        if (i == 0 && t == A_T && kc + 1 < nch) {
          __builtin_amdgcn_sched_barrier(0);
          X3_DMA_HM(kc + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        int nrd = 0;
        if (st + 1 < NSTEP) {
          X3P_READ_A(sb ^ 1, st + 1);
          nrd = 4;
        }
        // (an `if` of its own: nested in the one above, the compiler put reads next to the step's
        // boundary wait again in 6 of the 16 instantiations, profiles/r10_x3_step_boundaries.txt)
        if (st + 1 < NSTEP && (st + 1) % RM == 0) {
          X3P_READ_B(tb ^ 1, (st + 1) / RM);
          nrd += 3 * Q;
        }
        // the three products of an accumulator in the same order, but product-major: 2Q
        // independent MFMAs separate each from the next one on the same accumulator
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
          for (int q = 0; q < Q; ++q)
            acc16[i][pt][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sb][0][pt], gb[tb][2][q], acc16[i][pt][q], 0, 0, 0);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
          for (int q = 0; q < Q; ++q)
            acc16[i][pt][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sb][1][pt], gb[tb][1][q], acc16[i][pt][q], 0, 0, 0);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
          for (int q = 0; q < Q; ++q)
            acc16[i][pt][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sb][0][pt], gb[tb][0][q], acc16[i][pt][q], 0, 0, 0);
        // an MFMA opens the step, then one LDS read per MFMA while the next step's reads last, then
        // the rest of the MFMAs: the wait for this step's operands, which the compiler puts ahead of
        // the step's first MFMA, then covers no read issued after the previous step's MFMAs
#pragma unroll
        for (int r = 0; r < nrd; ++r) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        if (nrd == 4) __builtin_amdgcn_sched_group_barrier(0x008, 6 * Q - 4, 0);
        else if (nrd == 4 + 3 * Q) __builtin_amdgcn_sched_group_barrier(0x008, 3 * Q - 4, 0);
        else __builtin_amdgcn_sched_group_barrier(0x008, 6 * Q, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#undef X3P_READ_A
#undef X3P_READ_B
    } else {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        bf16x8 bfr[3][RN][3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int p = 0; p < 3; ++p)
              bfr[ky][j][p] = __builtin_bit_cast(bf16x8, Bs[((p * 9 + ky * 3 + kx) * 2 + h) * BN + j * 32 + l32]);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          bf16x8 af[3];
#pragma unroll
          for (int p = 0; p < 3; ++p)
            af[p] = __builtin_bit_cast(bf16x8, As[p * A_PLANE + h * HS + (srow0 + s) * SC + acol[kx]]);
#pragma unroll
          for (int i = 0; i < RM; ++i)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
              if (x3_srel<UP>(i, ky) != s) continue;
#pragma unroll
              for (int j = 0; j < RN; ++j) {
                f32x16 c = acc[i][j];
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], bfr[ky][j][0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bfr[ky][j][2], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bfr[ky][j][1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], bfr[ky][j][0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bfr[ky][j][1], c, 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], bfr[ky][j][0], c, 0, 0, 0);
              }
            }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    X3_ST(3 + 4 * kc);
    if (kc + 1 < nch) {
      if constexpr (M16) {
        X3_SPLIT_A(kc + 1);
        __syncthreads();  // every wave is done reading this chunk
        X3_ST(4 + 4 * kc);
        X3_DMA_LO(kc + 1);
        X3_WRITE_A;
      } else {
        __syncthreads();  // every wave is done reading this chunk
        X3_ST(4 + 4 * kc);
        X3_STORE(kc + 1);
      }
      __syncthreads();
      X3_ST(5 + 4 * kc);
    }
  }
#undef X3_LOAD
#undef X3_LOAD_A
#undef X3_LOAD_B
#undef X3_STORE
#undef X3_DMA_ROWS
#undef X3_DMA_HM
#undef X3_DMA_LO
#undef X3_SPLIT_A
#undef X3_WRITE_A
  if constexpr (M16) {
    // staged epilogue, 32 channels (two 16-tiles) per pass: lane (l16, g16) holds pixels 16 pt + 4 g16
    // + r of channel 16 q + l16 -> one float4 per (row, pixel tile) into the region
    __syncthreads();  // every wave is done reading the last chunk's tiles
    X3_ST(2 + 4 * nch);
    float* region = reinterpret_cast<float*>(x3_smem) + wm * 32 * RM * 36;
    // ReLU + 2x2 max-pool as the only output (the encoder's pool layers in config 2): pooled in
    // registers -- a lane holds both rows of its windows (acc16[2pr], acc16[2pr + 1]) and 4
    // consecutive pixels -- with no LDS round trip. One exchange with lane ^ 16 gives every lane 4
    // consecutive pooled pixels: even g16 its own pair and the partner's of tile pt = 0, odd g16 the
    // partner's and its own of pt = 1, so the 4 lanes of a channel store its 16 pooled pixels as one
    // 64-byte run (store_region's granularity). Same max_nan order as store_region: bit-identical.
    if (a.y_pool && !a.y_pre && !a.y_act && !a.e_sum2 && !dgrad_epi(a)) {
      const int Ho = a.H >> 1, Wo = a.W >> 1;
      const bool odd = g16 & 1;
      const int pc = (x0 >> 1) + (odd ? 8 + 2 * (g16 - 1) : 2 * g16);
      const bool vec = (Wo & 3) == 0 && pc + 3 < Wo;
#pragma unroll
      for (int q = 0; q < 2 * RN; ++q) {
        const int co = n0 + 16 * q + l16;
        const float bv = (co < a.Cout && a.bias) ? a.bias[co] : 0.f;
#pragma unroll
        for (int pr = 0; pr < RM / 2; ++pr) {
          float pv[2][2];
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) {
            const f32x4v r0 = acc16[2 * pr][pt][q], r1 = acc16[2 * pr + 1][pt][q];
            const float m0 = max_nan(relu_f(r0[0] + bv), relu_f(r1[0] + bv));
            const float m1 = max_nan(relu_f(r0[1] + bv), relu_f(r1[1] + bv));
            const float m2 = max_nan(relu_f(r0[2] + bv), relu_f(r1[2] + bv));
            const float m3 = max_nan(relu_f(r0[3] + bv), relu_f(r1[3] + bv));
            pv[pt][0] = max_nan(m0, m1);
            pv[pt][1] = max_nan(m2, m3);
          }
          const float e0 = __shfl_xor(odd ? pv[0][0] : pv[1][0], 16, 64);
          const float e1 = __shfl_xor(odd ? pv[0][1] : pv[1][1], 16, 64);
          const float o[4] = {odd ? e0 : pv[0][0], odd ? e1 : pv[0][1], odd ? pv[1][0] : e0, odd ? pv[1][1] : e1};
          const int py = ((y0 + wm * RM) >> 1) + pr;
          if (co >= a.Cout || py >= Ho) continue;
          float* dst = a.y_pool + ((int64_t)n * a.Cout + co) * Ho * Wo + (int64_t)py * Wo + pc;
          if (vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (pc + k < Wo) dst[k] = o[k];
          }
        }
      }
    } else
#pragma unroll
    for (int j = 0; j < RN; ++j) {
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const int q = 2 * j + qq, co = n0 + 16 * q + l16;
        const float bv = (co < a.Cout && a.bias) ? a.bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) {
            const f32x4v v = acc16[i][pt][q];
            *reinterpret_cast<float4*>(region + ((16 * qq + l16) * RM + i) * 36 + 16 * pt + 4 * g16) =
                make_float4(v[0] + bv, v[1] + bv, v[2] + bv, v[3] + bv);
          }
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      __builtin_amdgcn_wave_barrier();
      store_region<RM>(a, region, n, x0, y0, wm * RM, n0 + 32 * j, lane);
      if (j + 1 < RN) {
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
      }
    }
#if X3_STAMP
    __builtin_amdgcn_s_waitcnt(0);  // the epilogue's stores have left (vmcnt 0)
    X3_ST(3 + 4 * nch);
    if (blockIdx.x < kX3StampWgs) {
      unsigned* rec = x3_stamp_buf + ((size_t)blockIdx.x * 16 + wm) * kX3StampRec;
      rec[lane] = st0;
      rec[64 + lane] = st1;
      rec[128 + lane] = st2;
      if (lane == 0) {
        rec[192] = __builtin_amdgcn_s_getreg(4 | (31 << 11));   // HW_REG_HW_ID: wave, SIMD, CU, SE
        rec[193] = __builtin_amdgcn_s_getreg(20 | (3 << 11));   // HW_REG_XCC_ID
        rec[194] = blockIdx.x;
        rec[195] = nch;
        rec[196] = 0x57a3u;
      }
    }
#endif
  } else {
#if X3_STAGED_EPI
    __syncthreads();  // every wave is done reading the last chunk's tiles
    store_tiles_staged<RM, RN>(a, acc, n, x0, y0, wm * RM, n0, h, l32, lane,
                               reinterpret_cast<float*>(x3_smem) + wm * 32 * RM * 36);
#else
    store_tiles<RM, RN>(a, acc, n, x0, y0, wm * RM, n0, h, l32);
#endif
  }
  if constexpr (!PER) break;
  }  // block loop
}

template <int WM, int RM, int RN, int UP, int OCC, bool M16, bool PER = false>
int launch_x3_one(const ConvArgs& a0, hipStream_t s) {
  using C = X3Cfg<WM, RM, RN, UP>;
  ConvArgs a = a0;
  int64_t nblk;
  if (const int e = conv_grid(a, C::TH, C::BN, nblk)) return e;
  if (PER) {  // one workgroup per CU slot, a multiple of 8 (the XCD of a block stays fixed)
    const int64_t slots = (int64_t)(cu_count() + 7) / 8 * 8 * OCC;
    nblk = nblk < slots ? nblk : slots;
  }
  auto kern = conv3x3_x3_kernel<WM, RM, RN, UP, OCC, M16, PER>;
  constexpr int lds = M16 ? C::LDS_BYTES_M16 : C::LDS_BYTES;
  static_assert(lds * OCC <= 160 * 1024, "LDS per CU");
  [[maybe_unused]] static const void* const attr_set = with_dynamic_lds((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(C::NT), lds, s, a);
  return (int)hipGetLastError();
}

// Persistent form of the M16 split-bf16 kernel (round 4). One workgroup per CU
// slot walks the blocks b = blockIdx.x + k * gridDim.x (same XCD for all of them: b % 8 is fixed,
// and decode_block keeps the output-channel groups of a pixel tile on one XCD), and per block:
//   * the NEXT block's first K-chunk (its gather and weight slab) is loaded during the current
//     block's last chunk of MFMAs, so no block starts with an unoverlapped gather;
//   * the epilogue's global stores are left in flight (LDS-only barriers after it), so the store
//     tail of one block runs under the next block's first MFMAs instead of holding the CU.
// Per block the arithmetic, k order and rounding are conv3x3_x3_kernel<M16>'s: bit-identical.
// Measured on config 2 (profiles/r04_conv_persistent.txt): 1-2 % SLOWER per dispatch than the
// one-block-per-workgroup form, also on grids of one block per slot, so the loss is per-block code
// (argument re-reads, per-block address recomputation), not the static block walk; reached by config
// number only (32-35, and 38-41; no automatic choice takes them).
// It shares this translation unit with conv3x3_x3_kernel on purpose: both call store_region<2>, and
// the compiler's interprocedural passes look at all of a helper's call sites in the file. Compiled
// apart, every conv3x3_x3_kernel got a differently scheduled epilogue (same registers; one opt-in
// form measured 4% slower, profiles/r09_x3_apart_kernels_ab.txt).
__device__ __forceinline__ void x3_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// The kernel's ConvArgs re-read from the kernarg segment at the point of use: the empty asm hides the
// pointer's provenance, so the compiler cannot hoist the argument loads out of the block loop and keep
// every field in SGPRs across it (the persistent loop otherwise runs out of SGPRs and spills).
// A wave-uniform pointer the divergence analysis cannot see as one (it is assigned under the block
// loop's control flow): pinned to SGPRs, so the buffer descriptors built from it need no
// readfirstlane loop per load.
__device__ __forceinline__ const float* x3p_uniform(const float* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ const ConvArgs& x3p_args() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const ConvArgs*)p;
}

template <int WM, int RM, int RN, int UP, int OCC>
__global__ __launch_bounds__(WM * 64, OCC) void conv3x3_x3p_kernel(ConvArgs, int nblk) {
#define A_ x3p_args()
  using C = X3Cfg<WM, RM, RN, UP>;
  constexpr int NT = C::NT, TH = C::TH, BN = C::BN, SR = C::SR, SC = C::SC, A_PLANE = C::A_PLANE;
  constexpr int HS = C::HS, A_ITEMS = C::A_ITEMS;
  constexpr int A_T = C::A_T, B_T = C::B_T;
  constexpr int Q = 2 * RN;
  static_assert(RM % 2 == 0, "even rows per wave (pool windows, upsample row pairs)");
  extern __shared__ __attribute__((aligned(16))) u32x4 x3_smem[];
  u32x4* As = x3_smem;
  u32x4* Bs = x3_smem + C::A_UNITS;
  typedef float f32x4v __attribute__((ext_vector_type(4)));

  const int tid = threadIdx.x, wm = tid >> 6, lane = tid & 63;
  const int nch = (A_.Cin + kX3K - 1) / kX3K;

  // the blocks of this workgroup: b = blockIdx.x + k * gridDim.x; a padding block (tile >= ntiles)
  // is only ever followed by padding blocks, so the walk ends at the first one
#define X3P_DECODE(B, OK, X0, Y0, IMG, N0)                                                            \
  {                                                                                                 \
    int t_, grp_;                                                                                   \
    OK = (B) < nblk && decode_block((B), A_.tiles_x * A_.tiles_y * A_.N, (A_.Cout + BN - 1) / BN, t_, grp_);                                 \
    if (OK) {                                                                                       \
      X0 = (t_ % A_.tiles_x) * TW;                                                                   \
      t_ /= A_.tiles_x;                                                                              \
      Y0 = (t_ % A_.tiles_y) * TH;                                                                   \
      IMG = t_ / A_.tiles_y;                                                                           \
      N0 = grp_ * BN;                                                                               \
    }                                                                                               \
  }
  // gather state of the block whose chunks are being loaded
  unsigned g_off[A_T], g_pix[A_T];
  int g_lds[A_T], g_h[A_T];
  bool g_ok[A_T];
  int b_src[B_T];
  const float* __restrict__ xin = A_.x;
#define X3P_SETUP(X0, Y0, IMG, N0)                                                                   \
  {                                                                                                 \
    const int plane_in = (A_.Hin * A_.Win), Hin = A_.Hin, Win = A_.Win;                                \
    xin = x3p_uniform((IMG) < A_.nsplit ? A_.x + (int64_t)(IMG) * A_.Cin * plane_in                      \
                                     : A_.x2 + (int64_t)((IMG) - A_.nsplit) * A_.Cin * plane_in);        \
    const int sx0_ = (X0) / UP, sy0_ = (Y0) / UP - 1;                                               \
    int tv_ = tid; /* laundered: the per-thread item decode is redone here, not hoisted and spilled */ \
    asm volatile("" : "+v"(tv_));                                                                   \
    _Pragma("unroll") for (int i = 0; i < A_T; ++i) {                                               \
      const int e = min(tv_ + i * NT, A_ITEMS - 1);                                                 \
      const int c = e % SC, rest = e / SC, r = rest % SR, hh = rest / SR;                           \
      const int sy = src_index<UP>(sy0_ + r, Hin, A_.reflect), sx = src_index<UP>(sx0_ - 1 + c, Win, A_.reflect); \
      g_ok[i] = sy >= 0 && sx >= 0;                                                                 \
      g_pix[i] = (unsigned)(max(sy, 0) * Win + max(sx, 0));                                         \
      g_off[i] = g_ok[i] ? 4u * (unsigned)(8 * hh * plane_in) + 4u * g_pix[i] : 0x7ffffff0u;        \
      g_lds[i] = hh * HS + r * SC + c;                                                              \
      g_h[i] = hh;                                                                                  \
    }                                                                                               \
    _Pragma("unroll") for (int i = 0; i < B_T; ++i) {                                               \
      const int u = min(tv_ + i * NT, C::B_UNITS - 1), row = u / BN, j = u - row * BN;              \
      b_src[i] = 16 * (row * A_.cout_pad + (N0) + j);                                                \
    }                                                                                               \
  }
  float ra[A_T][8];
  u32x4 rb[B_T];
#define X3P_LOAD(KC)                                                                                    \
  {                                                                                                     \
    const int ci0 = (KC) * kX3K, plane_in = (A_.Hin * A_.Win), plane_b = 4 * plane_in;                       \
    const int64_t chunk_units = ((int64_t)C::B_ROWS * A_.cout_pad);                                                        \
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(                             \
        const_cast<float*>(A_.wp + x3_split_offset(A_.Cin, A_.Cout)), 0,                               \
        (int)min<int64_t>(0x7fffffff, (int64_t)nch * chunk_units * 16), 0x00020000);                   \
    if (ci0 + kX3K <= A_.Cin) {                                                                          \
      const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(                              \
          const_cast<float*>(xin + (int64_t)ci0 * plane_in), 0, kX3K * plane_b, 0x00020000);           \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                     \
        _Pragma("unroll") for (int i = 0; i < A_T; ++i)                                                 \
          ra[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)g_off[i], j * plane_b, 0)); \
    } else {                                                                                            \
      _Pragma("unroll") for (int i = 0; i < A_T; ++i)                                                   \
        _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                   \
          ra[i][j] = xin[(int64_t)min(ci0 + 8 * g_h[i] + j, A_.Cin - 1) * plane_in + g_pix[i]];          \
    }                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < B_T; ++i)                                                     \
      rb[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_src[i], (int)((KC) * chunk_units * 16), 0)); \
  }
#define X3P_STORE(KC)                                                                                   \
  {                                                                                                     \
    const ConvArgs& ka_ = x3p_args(); /* one laundered argument pointer per expansion */                \
    _Pragma("unroll") for (int i = 0; i < A_T; ++i) {                                                   \
      if (tid + i * NT < A_ITEMS) {                                                                     \
        if ((KC) * kX3K + kX3K > ka_.Cin) {                                                               \
          const int cn = ka_.Cin - (KC) * kX3K - 8 * g_h[i];                                              \
          _Pragma("unroll") for (int j = 0; j < 8; ++j) ra[i][j] = (g_ok[i] && j < cn) ? ra[i][j] : 0.f; \
        }                                                                                               \
        bf16x8 pv[3];                                                                                   \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                 \
          bf16 t0, t1, t2;                                                                              \
          ast_x3::split3(ra[i][j], t0, t1, t2);                                                                \
          pv[0][j] = t0;                                                                                \
          pv[1][j] = t1;                                                                                \
          pv[2][j] = t2;                                                                                \
        }                                                                                               \
        _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                   \
          As[p * A_PLANE + g_lds[i]] = __builtin_bit_cast(u32x4, pv[p]);                                \
      }                                                                                                 \
    }                                                                                                   \
    _Pragma("unroll") for (int i = 0; i < B_T; ++i)                                                     \
      if (tid + i * NT < C::B_UNITS) Bs[tid + i * NT] = rb[i];                                          \
  }

  int b = blockIdx.x, x0 = 0, y0 = 0, n = 0, n0 = 0;
  bool ok;
  X3P_DECODE(b, ok, x0, y0, n, n0);
  if (!ok) return;  // uniform: the whole workgroup
  X3P_SETUP(x0, y0, n, n0);
  X3P_LOAD(0);
  X3P_STORE(0);
  x3_lds_barrier();
  while (true) {
    const int b2 = b + gridDim.x;
    int nx0 = 0, ny0 = 0, nn = 0, nn0 = 0;
    bool has_next;
    X3P_DECODE(b2, has_next, nx0, ny0, nn, nn0);
    // the MFMA loop's LDS addresses derive from lane values laundered per block, so they are
    // recomputed here rather than hoisted out of the block loop and held live through the epilogue
    int lv = lane, wv = wm;
    asm volatile("" : "+v"(lv), "+v"(wv));
    const int ml16 = lv & 15, mg16 = lv >> 4, mhh16 = mg16 & 1;
    const int apl1 = (mg16 < 2 ? 0 : 1) * A_PLANE, apl2 = (mg16 < 2 ? 0 : 2) * A_PLANE;  // [hi|mid], [hi|lo]
    const int bpl1 = 0, bpl2 = mg16 < 2 ? 1 : 0, bpl3 = mg16 < 2 ? 2 : 1;              // [hi;hi], [mid;hi], [lo;mid]
    const int srow0 = wv * RM / UP;
    int acol16[2][3];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acol16[pt][kx] = ((x0 + 16 * pt + ml16 + kx - 1) >> (UP - 1)) - x0 / UP + 1;
    f32x4v acc16[RM][2][Q];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc16[i][pt][q] = f32x4v{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < nch; ++kc) {
      if (kc + 1 < nch) X3P_LOAD(kc + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int tap = ky * 3 + kx;
          bf16x8 g1[Q], g2[Q], g3[Q];
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const int col = q * 16 + ml16;
            g1[q] = __builtin_bit_cast(bf16x8, Bs[((bpl1 * 9 + tap) * 2 + mhh16) * BN + col]);
            g2[q] = __builtin_bit_cast(bf16x8, Bs[((bpl2 * 9 + tap) * 2 + mhh16) * BN + col]);
            g3[q] = __builtin_bit_cast(bf16x8, Bs[((bpl3 * 9 + tap) * 2 + mhh16) * BN + col]);
          }
#pragma unroll
          for (int i = 0; i < RM; ++i) {
            const int srow = mhh16 * HS + (srow0 + x3_srel<UP>(i, ky)) * SC;
            bf16x8 f1[2], f2[2];
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
              f1[pt] = __builtin_bit_cast(bf16x8, As[apl1 + srow + acol16[pt][kx]]);
              f2[pt] = __builtin_bit_cast(bf16x8, As[apl2 + srow + acol16[pt][kx]]);
            }
            // the three products of an accumulator in the same order, but product-major: 2Q
            // independent MFMAs separate each from the next one on the same accumulator
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
              for (int q = 0; q < Q; ++q)
                acc16[i][pt][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1[pt], g3[q], acc16[i][pt][q], 0, 0, 0);
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
              for (int q = 0; q < Q; ++q)
                acc16[i][pt][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f2[pt], g2[q], acc16[i][pt][q], 0, 0, 0);
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
              for (int q = 0; q < Q; ++q)
                acc16[i][pt][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1[pt], g1[q], acc16[i][pt][q], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kc + 1 < nch) {  // LDS-only barriers: the previous block's epilogue stores keep draining
        x3_lds_barrier();  // every wave is done reading this chunk
        X3P_STORE(kc + 1);
        x3_lds_barrier();
      }
    }
    // epilogue: as conv3x3_x3_kernel<M16>, but every accumulator goes to the wave's LDS region first
    // (RN x 32 channels: the accumulators are dead before the stores, while the next block's first
    // chunk is held in registers), and the global stores are left in flight
    if (has_next) {  // the next block's first chunk, in flight during this block's epilogue
      X3P_SETUP(nx0, ny0, nn, nn0);
      X3P_LOAD(0);
    }
    x3_lds_barrier();  // every wave is done reading the last chunk's tiles
    int el = lane, ew = wm;  // laundered as in the MFMA loop
    asm volatile("" : "+v"(el), "+v"(ew));
    const int el16 = el & 15, eg16 = el >> 4;
    float* region = reinterpret_cast<float*>(x3_smem) + ew * 32 * RM * 36;
#pragma unroll
    for (int j = 0; j < RN; ++j) {
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const int q = 2 * j + qq, co = n0 + 16 * q + el16;
        const float bv = (co < A_.Cout && A_.bias) ? A_.bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) {
            const f32x4v v = acc16[i][pt][q];
            *reinterpret_cast<float4*>(region + ((16 * qq + el16) * RM + i) * 36 + 16 * pt + 4 * eg16) =
                make_float4(v[0] + bv, v[1] + bv, v[2] + bv, v[3] + bv);
          }
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      store_region<RM>(A_, region, n, x0, y0, ew * RM, n0 + 32 * j, el);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
    if (!has_next) break;
    x3_lds_barrier();  // every wave is done with its epilogue region (the stores stay in flight)
    X3P_STORE(0);      // the next block's first chunk (loaded during the last MFMAs)
    x3_lds_barrier();
    b = b2;
    x0 = nx0;
    y0 = ny0;
    n = nn;
    n0 = nn0;
  }
#undef X3P_DECODE
#undef X3P_SETUP
#undef X3P_LOAD
#undef X3P_STORE
#undef A_
}

// persistent form: one workgroup per CU slot (OCC per CU), a multiple of 8 (XCD-consistent stride)
template <int WM, int RM, int RN, int UP, int OCC>
int launch_x3p_one(const ConvArgs& a0, hipStream_t s) {
  using C = X3Cfg<WM, RM, RN, UP>;
  ConvArgs a = a0;
  int64_t nblk;
  if (const int e = conv_grid(a, C::TH, C::BN, nblk)) return e;
  const int64_t slots = (int64_t)(cu_count() + 7) / 8 * 8 * OCC;
  const unsigned grid = (unsigned)(nblk < slots ? nblk : slots);
  auto kern = conv3x3_x3p_kernel<WM, RM, RN, UP, OCC>;
  constexpr int lds = C::LDS_BYTES;
  static_assert(lds * OCC <= 160 * 1024, "LDS per CU");
  [[maybe_unused]] static const void* const attr_set = with_dynamic_lds((const void*)kern, lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NT), lds, s, a, (int)nblk);
  return (int)hipGetLastError();
}

}  // namespace

namespace ast_conv {

// split-bf16 MFMA kernel: no fused input normalisation (conv_1 runs the direct cin<=4 kernel)
template <int WM, int RM, int RN, int OCC, bool M16, bool PER>
int launch_x3(const ConvArgs& a, hipStream_t s, int up) {
  if (a.in_mean) return AST_E_UNSUPPORTED;
  if ((int64_t)a.Cin * a.Hin * a.Win * 4 >= ((int64_t)1 << 31)) return AST_E_UNSUPPORTED;  // 32-bit buffer offsets
  return up == 2 ? launch_x3_one<WM, RM, RN, 2, OCC, M16, PER>(a, s) : launch_x3_one<WM, RM, RN, 1, OCC, M16, PER>(a, s);
}

template <int WM, int RM, int RN, int OCC>
int launch_x3p(const ConvArgs& a, hipStream_t s, int up) {
  if (a.in_mean) return AST_E_UNSUPPORTED;
  if ((int64_t)a.Cin * a.Hin * a.Win * 4 >= ((int64_t)1 << 31)) return AST_E_UNSUPPORTED;  // 32-bit buffer offsets
  return up == 2 ? launch_x3p_one<WM, RM, RN, 2, OCC>(a, s) : launch_x3p_one<WM, RM, RN, 1, OCC>(a, s);
}

// the four tiles (WM, RM, RN, OCC) of 24-27, as 28-31 (M16), 38-41 (M16, PER) and 32-35 (x3p)
#define X3_TILES(F, ...)                                                                            \
  CONV_INSTANTIATE(F<8, 2, 2, 1 __VA_ARGS__>) CONV_INSTANTIATE(F<4, 2, 2, 1 __VA_ARGS__>)           \
  CONV_INSTANTIATE(F<4, 2, 1, 2 __VA_ARGS__>) CONV_INSTANTIATE(F<8, 2, 1, 1 __VA_ARGS__>)
X3_TILES(launch_x3, , false, false) X3_TILES(launch_x3, , true, false) X3_TILES(launch_x3, , true, true)
X3_TILES(launch_x3p)
#undef X3_TILES

}  // namespace ast_conv

extern "C" {

int ast_conv3x3_pack_split_f32(float* w_packed, int cout, int cin, void* stream) {
  if (!w_packed) return AST_E_NULLPTR;
  if (cout <= 0 || cin <= 0) return AST_E_SHAPE;
  const int cout_pad = round_up(cout, kCoutAlign);
  const int64_t total = (int64_t)round_up(cin, kX3K) * 9 * cout_pad;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(pack_x3_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_packed,
                     reinterpret_cast<bf16*>(w_packed + x3_split_offset(cin, cout)), round_up(cin, kCinAlign),
                     round_up(cin, kX3K), cout_pad);
  return (int)hipGetLastError();
}

#if X3_STAMP
// diagnostic build only: copy / clear the stamp records of conv3x3_x3_kernel<M16>
int ast_dbg_x3_stamps(void* host, size_t bytes, int clear) { return x3_stamps_read(host, bytes, clear); }
#endif

}  // extern "C"
