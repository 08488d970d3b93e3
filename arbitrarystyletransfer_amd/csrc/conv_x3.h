// Shared by the split-bf16 ("x3") kernels -- conv_x3.hip and conv_up2c.hip, whose
// kernel takes the x3 kernel's gather, A-tile layout and staged epilogue: the tile sizes (X3Cfg), the
// row stores of a staged epilogue region (store_region), and the stamps of the diagnostic build.
#pragma once
#include "conv_common.h"
#include "x3.h"

namespace ast_conv {

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // (HIP's uint4 struct defeats SROA: scratch)

#ifndef X3_HS_PAD
#define X3_HS_PAD 1
#endif

template <int WM, int RM, int RN, int UP>
struct X3Cfg {
  static constexpr int NT = WM * 64;
  static constexpr int TH = WM * RM;                 // output rows per tile
  static constexpr int BN = RN * 32;                 // output channels per tile
  static constexpr int SR = TH / UP + 2;             // source rows incl. halo
  static constexpr int SC = TW / UP + 2;             // source columns incl. halo
  static constexpr int A_ITEMS = 2 * SR * SC;        // gather items: 16-B units of 8 channels, both halves
  // 16-B units per 8-channel half, padded to a multiple of 16 units (64 banks): the M16 A operand
  // reads both halves (and two planes) in one ds_read_b128, whose lane groups {0-3,12-15,20-27} /
  // {4-11,16-19,28-31} mix the halves -- unpadded (612 units = 16 banks apart) they collide on 16
  // banks per group (2-way, profiles/r04p: 22% of the LDS cycles were conflicts)
  static constexpr int HS = X3_HS_PAD ? (SR * SC + 15) / 16 * 16 : SR * SC;
  static constexpr int A_PLANE = 2 * HS;             // 16-B units per plane
  static constexpr int A_UNITS = 3 * A_PLANE;
  static constexpr int B_ROWS = 3 * 9 * 2;           // (plane, tap, h)
  static constexpr int B_UNITS = B_ROWS * BN;
  static constexpr int A_T = (A_ITEMS + NT - 1) / NT;  // gather items per thread (one item = 8 channels)
  static constexpr int B_T = (B_UNITS + NT - 1) / NT;
  static constexpr int NS = UP == 1 ? RM + 2 : RM / 2 + 2;  // source rows a wave's RM output rows read
  static constexpr int LDS_TILES = (A_UNITS + B_UNITS) * 16;
  // staged epilogue regions: the M16 and persistent kernels always stage through LDS, whatever
  // X3_STAGED_EPI (which only selects the 32x32 kernel's direct-store A/B form) says
  static constexpr int LDS_EPI = WM * 32 * RM * 36 * 4;
  static constexpr int LDS_BYTES = LDS_TILES > LDS_EPI ? LDS_TILES : LDS_EPI;
  // M16 kernel: A tile, the weight slab's lo plane, and its hi + mid planes twice (the next chunk's
  // arrive by LDS-DMA during the current chunk's MFMAs)
  static constexpr int LDS_TILES_M16 = (A_UNITS + 18 * BN + 2 * 36 * BN) * 16;
  static constexpr int LDS_BYTES_M16 = LDS_TILES_M16 > LDS_EPI ? LDS_TILES_M16 : LDS_EPI;
};

// source row (relative to the wave's first) of output row i at tap row ky
template <int UP>
__host__ __device__ constexpr int x3_srel(int i, int ky) { return UP == 1 ? i + ky : ((i + ky - 1) >> 1) + 1; }

// Epilogue through LDS (x3 kernel): in the MFMA layout a lane holds one output channel, so a
// direct float4 store scatters over 64 rows/planes per instruction (store-issue-bound). Each wave
// writes its accumulators (+bias) to its own LDS region [32 channels][RM rows][32 px + 4], then
// stores rows: 8 lanes per 128-byte run, pre-ReLU / ReLU / 2x2 max-pool as store_tiles. The
// caller's barrier must precede it (the region overlaps the operand tiles).
// Row stores of one 32-channel group from a wave's staged region [32 channels][RM rows][36 floats]
// (channel ch = output channel cbase + ch): pre-ReLU / ReLU float4 rows, 8 lanes per 128-byte run,
// and the fused 2x2 max-pool.
template <int RM>
__device__ __forceinline__ void store_region(const ConvArgs& a, const float* __restrict__ region, int n, int x0,
                                             int y0, int row0, int cbase, int lane) {
  constexpr int RP = 36;  // row pitch (floats): 32 px + 4
  const int H = a.H, W = a.W;
  const int64_t plane = (int64_t)H * W;
  const bool vec4 = (W & 3) == 0;
  const int Ho = H >> 1, Wo = W >> 1;
  if (a.y_pre || a.y_act) {
#pragma unroll
    for (int it = 0; it < 32 * RM * 8 / 64; ++it) {
      const int item = it * 64 + lane;
      const int q = item & 7, row = (item >> 3) % RM, ch = item / (8 * RM);
      const int co = cbase + ch, yy = y0 + row0 + row, xx = x0 + 4 * q;
      if (co >= a.Cout || yy >= H || xx >= W) continue;
      const float4 v = *reinterpret_cast<const float4*>(region + (ch * RM + row) * RP + 4 * q);
      const int64_t off = ((int64_t)n * a.Cout + co) * plane + (int64_t)yy * W + xx;
      const bool full = vec4 && xx + 3 < W;
      const float vv[4] = {v.x, v.y, v.z, v.w};
      if (dgrad_epi(a)) {  // input gradient: y_pre only
        if (full) *reinterpret_cast<float4*>(a.y_pre + off) = dgrad_epi4(a, v, off);
        else for (int r = 0; r < 4; ++r) if (xx + r < W) a.y_pre[off + r] = dgrad_epi_one(a, vv[r], off + r);
        continue;
      }
      if (a.y_pre) {
        if (full) *reinterpret_cast<float4*>(a.y_pre + off) = v;
        else for (int r = 0; r < 4; ++r) if (xx + r < W) a.y_pre[off + r] = vv[r];
      }
      if (a.y_act) {
        const float4 u = make_float4(relu_f(v.x), relu_f(v.y), relu_f(v.z), relu_f(v.w));
        if (full) *reinterpret_cast<float4*>(a.y_act + off) = u;
        else for (int r = 0; r < 4; ++r) if (xx + r < W) a.y_act[off + r] = relu_f(vv[r]);
      }
    }
  }
  if (a.y_pool) {
#pragma unroll
    for (int it = 0; it < 32 * (RM / 2) * 8 / 64; ++it) {
      const int item = it * 64 + lane;
      const int q = item & 7, prow = (item >> 3) % (RM / 2), ch = item / (8 * (RM / 2));
      const int co = cbase + ch, py = (y0 + row0) / 2 + prow, px = (x0 + 4 * q) >> 1;
      if (co >= a.Cout || py >= Ho || px >= Wo) continue;
      const float4 r0 = *reinterpret_cast<const float4*>(region + (ch * RM + 2 * prow) * RP + 4 * q);
      const float4 r1 = *reinterpret_cast<const float4*>(region + (ch * RM + 2 * prow + 1) * RP + 4 * q);
      const int64_t off = ((int64_t)n * a.Cout + co) * Ho * Wo + (int64_t)py * Wo + px;
      float p0, p1;
      if (a.e_sum2) {  // nearest-upsample adjoint: the window's sum, row by row (pad_up_adjoint's order)
        p0 = dgrad_epi_one(a, ((r0.x + r0.y) + r1.x) + r1.y, off);
        p1 = px + 1 < Wo ? dgrad_epi_one(a, ((r0.z + r0.w) + r1.z) + r1.w, off + 1) : 0.f;
      } else {
        const float m0 = max_nan(relu_f(r0.x), relu_f(r1.x)), m1 = max_nan(relu_f(r0.y), relu_f(r1.y));
        const float m2 = max_nan(relu_f(r0.z), relu_f(r1.z)), m3 = max_nan(relu_f(r0.w), relu_f(r1.w));
        p0 = max_nan(m0, m1);
        p1 = max_nan(m2, m3);
      }
      if (px + 1 < Wo && (Wo & 1) == 0) {
        *reinterpret_cast<float2*>(a.y_pool + off) = make_float2(p0, p1);
      } else {
        a.y_pool[off] = p0;
        if (px + 1 < Wo) a.y_pool[off + 1] = p1;
      }
    }
  }
}

// Diagnostic build only (X3_STAMP=1, scripts/build_variants.sh; never the product library): every
// wave of the first X3_STAMP_WGS workgroups records the shader-clock counter at its phase boundaries
// (entry, prologue done, and per K chunk: loads issued / MFMAs done / first barrier / store + second
// barrier; epilogue start / end) in three VGPRs (lane k holds stamp k), stored once at the end to
// x3_stamp_buf, which no other code reads; scripts/x3_stamps.py reads it back. The buffer is per
// translation unit: the file built with X3_STAMP=1 (conv_x3.hip, or conv_up2c.hip for its kernel;
// one per variant library) exports ast_dbg_x3_stamps over its own.
#ifndef X3_STAMP
#define X3_STAMP 0
#endif
#if X3_STAMP
constexpr int kX3StampWgs = 2048, kX3StampRec = 200;
static __device__ unsigned x3_stamp_buf[kX3StampWgs * 16 * kX3StampRec];
// copy / clear the stamp records (the body of ast_dbg_x3_stamps)
static int x3_stamps_read(void* host, size_t bytes, int clear) {
  const size_t n = bytes < sizeof(x3_stamp_buf) ? bytes : sizeof(x3_stamp_buf);
  if (clear) {
    void* d = nullptr;
    const hipError_t e = hipGetSymbolAddress(&d, HIP_SYMBOL(x3_stamp_buf));
    return e ? (int)e : (int)hipMemset(d, 0, sizeof(x3_stamp_buf));
  }
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(x3_stamp_buf), n, 0, hipMemcpyDeviceToHost);
}
#define X3_ST(IDX)                                                                  \
  {                                                                                 \
    const unsigned t_ = (unsigned)__builtin_readcyclecounter();                     \
    const int i_ = (IDX);                                                           \
    st0 = lane == i_ ? t_ : st0;                                                    \
    st1 = lane == i_ - 64 ? t_ : st1;                                               \
    st2 = lane == i_ - 128 ? t_ : st2;                                              \
  }
#define X3_ST_STEP(KC, NCH, ST)                                                        \
  if ((KC) == 5) X3_ST(4 + 4 * (NCH) + (ST))  /* per-step stamps of chunk 5 */
#else
#define X3_ST(IDX)
#define X3_ST_STEP(KC, NCH, ST)
#endif

}  // namespace ast_conv
