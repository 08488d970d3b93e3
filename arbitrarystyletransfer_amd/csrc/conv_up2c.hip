// ------------------------------------------------------------------------------------------------
// Collapsed upsampled conv ("up2c"): nearest x2 -> ReflectionPad(1) -> conv3x3 with 2x2 taps per
// output phase instead of 3x3. The 9 taps of an output pixel touch 4 distinct source
// pixels, so for the output phase (py, px) = (row & 1, col & 1)
//   out[2i + py][2j + px] = sum_{a, b in {0, 1}} Wc[py][px][a][b] . src[clamp(i + py - 1 + a)][clamp(j + px - 1 + b)]
// with Wc the tap sums of pack_up2c_kernel: 16 phase-taps per source pixel against 36 tap
// applications, 2.25x fewer MFMAs. Gather, split, A-tile layout, LDS-DMA and the staged epilogue are
// conv3x3_x3_kernel<M16>'s; the products per 16 channels are its three K-32 MFMAs.
//  * workgroup: 8 waves, 32 x 32 output pixels (16 x 16 source pixels + halo) x 32 output channels;
//    a wave owns two source rows = four output rows, M tile = the 16 source pixels of a row for one
//    phase, accumulators [source row][py][px][16-channel tile] (64 VGPRs)
//  * the phase-taps run ordered by the source position (dy, dx) = (py + a, px + b) they read, so the
//    9 positions' A fragments are read once each and every B fragment feeds both source rows:
//    (16 x 6 + 9 x 4) = 132 ds_read_b128 for 192 MFMAs per chunk and wave
//  * weight slab [plane hi|mid|lo][phase-tap 16][half][32 channels] = 48 KiB per chunk, whole and
//    double-buffered (the next chunk's arrives by LDS-DMA under the current chunk's MFMAs):
//    31.5 KiB A tile + 96 KiB = 127.5 KiB, under the 144 KiB of the staged epilogue's regions
// ------------------------------------------------------------------------------------------------
#include <algorithm>
#include "conv_x3.h"
#include "env.h"

namespace {

using namespace ast_conv;

constexpr int kUp2cTaps = 16;  // phase-taps c = ((py * 2 + px) * 2 + a) * 2 + b
constexpr int kUp2cBN = 32;    // output channels per workgroup

__host__ __device__ constexpr int64_t up2c_numel(int cin, int cout) {  // floats of the collapsed slab
  return (int64_t)((cin + kX3K - 1) / kX3K * kX3K) * kUp2cTaps * ((cout + 63) / 64 * 64) * 3 / 2;
}

// the phase-tap run at step t of a chunk: ordered by source position (dy, dx), row-major
__host__ __device__ constexpr int up2c_tap(int t) { return (int)((0xFEBAD7C693825410ull >> (4 * t)) & 15); }
__host__ __device__ constexpr int up2c_pos(int c) { return ((c >> 3) + ((c >> 1) & 1)) * 3 + ((c >> 2) & 1) + (c & 1); }

// fp32 pack [ci_pad8][9][cout_pad] -> collapsed split pack [ci16 chunk][plane][phase-tap][h][cout_pad][8]:
// the tap sums in fp64, rounded once to fp32, then split3 as the plain pack. Phase 0 of a dimension
// reads source offsets {-1, 0} with {w[0], w[1] + w[2]}, phase 1 offsets {0, +1} with {w[0] + w[1], w[2]}.
__global__ void pack_up2c_kernel(const float* __restrict__ wp, bf16* __restrict__ ws, int cin_pad8, int cin16,
                                 int cout_pad) {
  const int64_t total = (int64_t)cin16 * kUp2cTaps * cout_pad;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(idx % cout_pad);
    const int64_t rt = idx / cout_pad;
    const int c = (int)(rt % kUp2cTaps);
    const int ci = (int)(rt / kUp2cTaps);
    const int py = c >> 3, px = (c >> 2) & 1, ta = (c >> 1) & 1, tb = c & 1;
    const int ky0 = ta == 0 ? 0 : (py == 0 ? 1 : 2), ky1 = ta == 0 ? (py == 0 ? 0 : 1) : 2;
    const int kx0 = tb == 0 ? 0 : (px == 0 ? 1 : 2), kx1 = tb == 0 ? (px == 0 ? 0 : 1) : 2;
    double s = 0.0;
    if (ci < cin_pad8)
      for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) s += (double)wp[((int64_t)ci * 9 + ky * 3 + kx) * cout_pad + co];
    bf16 t[3];
    ast_x3::split3((float)s, t[0], t[1], t[2]);
    const int kc = ci / kX3K, hh = (ci >> 3) & 1, e = ci & 7;
#pragma unroll
    for (int p = 0; p < 3; ++p)
      ws[((((int64_t)(kc * 3 + p) * kUp2cTaps + c) * 2 + hh) * cout_pad + co) * 8 + e] = t[p];
  }
}

// SLABS = 2: the 8-wave form above. SLABS = 1 (with WM = 4: 16 x 32 output pixels, a 10 x 18 source
// tile, 18 KiB A tile + one 48-KiB slab under the 72 KiB of the epilogue regions): two workgroups per
// CU, so one's prologue, barrier windows, slab landing and epilogue run under the other's MFMAs. The
// single buffer is refilled between the chunk's two barriers.
template <int WM, int SLABS = 2>
struct Up2cCfg {
  using X = X3Cfg<WM, 4, 1, 2>;  // 4 output rows per wave, 32 channels: tile, gather and epilogue sizes
  static_assert(SLABS == 1 || SLABS == 2, "");
  static constexpr int OCC = SLABS == 1 ? 2 : 1;  // workgroups per CU the form is sized for
  static_assert(X::BN == kUp2cBN && X::TH == 4 * WM, "");
  static constexpr int B_ROWS = 3 * kUp2cTaps * 2;  // (plane, phase-tap, h)
  static constexpr int B_PLANE = kUp2cTaps * 2 * kUp2cBN;
  static constexpr int B_UNITS = B_ROWS * kUp2cBN;
  static constexpr int LDS_TILES = (X::A_UNITS + SLABS * B_UNITS) * 16;
  static constexpr int LDS_BYTES = LDS_TILES > X::LDS_EPI ? LDS_TILES : X::LDS_EPI;
};

template <int WM, int SLABS = 2>
__global__ __launch_bounds__(WM * 64, SLABS == 1 ? 2 : 1) void conv3x3_up2c_kernel(ConvArgs a, const u32x4* __restrict__ wc) {
  using U = Up2cCfg<WM, SLABS>;
  static_assert(U::OCC == (SLABS == 1 ? 2 : 1), "");
  using C = typename U::X;
  constexpr int NT = C::NT, TH = C::TH, BN = kUp2cBN, SR = C::SR, SC = C::SC, A_PLANE = C::A_PLANE;
  constexpr int HS = C::HS, A_ITEMS = C::A_ITEMS, A_T = C::A_T;
  constexpr int B_UNITS = U::B_UNITS, B_PLANE = U::B_PLANE;
  extern __shared__ __attribute__((aligned(16))) u32x4 x3_smem[];
  u32x4* As = x3_smem;
  u32x4* Bs = x3_smem + C::A_UNITS;  // [SLABS][plane][phase-tap][h][BN]

  const int tid = threadIdx.x, wm = tid >> 6, lane = tid & 63;
#if X3_STAMP
  unsigned st0 = 0, st1 = 0, st2 = 0;
  X3_ST(0);
#endif
  const int ntl = a.tiles_x * a.tiles_y * a.N, ngr = (a.Cout + BN - 1) / BN;
  int t, grp;
  if (!decode_block(blockIdx.x, ntl, ngr, t, grp)) return;
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int x0 = tx * TW, y0 = ty * TH;
  const int sx0 = x0 / 2, sy0 = y0 / 2 - 1;
  const int n0 = grp * BN;
  const int Hin = a.Hin, Win = a.Win, plane_in = Hin * Win;
  const float* __restrict__ xin =
      n < a.nsplit ? a.x + (int64_t)n * a.Cin * plane_in : a.x2 + (int64_t)(n - a.nsplit) * a.Cin * plane_in;
  const int nch = (a.Cin + kX3K - 1) / kX3K;
  const int64_t chunk_units = (int64_t)U::B_ROWS * a.cout_pad;

  // gather items (h, source row, source column) as conv3x3_x3_kernel: raw buffer loads, replicate
  // padding of the source grid by src_index<2>
  unsigned g_off[A_T], g_pix[A_T];
  int g_lds[A_T], g_h[A_T];
#pragma unroll
  for (int i = 0; i < A_T; ++i) {
    const int e = min(tid + i * NT, A_ITEMS - 1);
    const int c = e % SC, rest = e / SC, r = rest % SR, hh = rest / SR;
    const int sy = src_index<2>(sy0 + r, Hin, 1), sx = src_index<2>(sx0 - 1 + c, Win, 1);
    g_pix[i] = (unsigned)(sy * Win + sx);
    g_off[i] = 4u * (unsigned)(8 * hh * plane_in) + 4u * g_pix[i];
    g_lds[i] = hh * HS + r * SC + c;
    g_h[i] = hh;
  }
  const int plane_b = 4 * plane_in;
  float ra[A_T][8];
  bf16x8 pv[A_T][3];
#define UP2C_LOAD_A(KC, I0, I1)                                                                         \
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
  // the whole slab of chunk KC (48 lane-linear 1-KiB pieces, 48 / WM per wave) into buffer KC & (SLABS - 1)
  static_assert(B_UNITS % (64 * WM) == 0, "whole 1-KiB pieces, the same count per wave");
#define UP2C_DMA(KC)                                                                                    \
  _Pragma("unroll") for (int i = 0; i < B_UNITS / 64 / WM; ++i) {                                       \
    const int piece = wm + i * WM;                                                                      \
    const int u = piece * 64 + lane, row = u / BN, j = u - row * BN;                                    \
    const u32x4* src = wc + (int64_t)(KC) * chunk_units + (int64_t)row * a.cout_pad + n0 + j;           \
    __builtin_amdgcn_global_load_lds((const void*)src,                                                  \
                                     (__attribute__((address_space(3))) void*)(Bs + ((KC) & (SLABS - 1)) * B_UNITS + piece * 64), \
                                     16, 0, 0);                                                         \
  }
#define UP2C_SPLIT_A(KC)                                                                                \
  _Pragma("unroll") for (int i = 0; i < A_T; ++i) {                                                     \
    if ((KC) * kX3K + kX3K > a.Cin) { /* partial last chunk: channels past Cin */                        \
      const int cn = a.Cin - (KC) * kX3K - 8 * g_h[i];                                                  \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) ra[i][j] = j < cn ? ra[i][j] : 0.f;                  \
    }                                                                                                   \
    ast_x3::split8(ra[i], pv[i][0], pv[i][1], pv[i][2]);                                                \
  }
#define UP2C_WRITE_A                                                                                    \
  _Pragma("unroll") for (int i = 0; i < A_T; ++i)                                                       \
    if (tid + i * NT < A_ITEMS)                                                                         \
      _Pragma("unroll") for (int p = 0; p < 3; ++p)                                                     \
        As[p * A_PLANE + g_lds[i]] = __builtin_bit_cast(u32x4, pv[i][p]);

  typedef float f32x4v __attribute__((ext_vector_type(4)));
  f32x4v acc[2][2][2][2];  // [source row][py][px][16-channel tile]
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) acc[r][p >> 1][p & 1][q] = f32x4v{0.f, 0.f, 0.f, 0.f};

  // lane roles as the M16 kernel: source pixel / channel l16 of a 16-tile, k-group g16 -> (term plane, half)
  const int l16 = lane & 15, g16 = lane >> 4, hh16 = g16 & 1;
  const int apl1 = (g16 < 2 ? 0 : 1) * A_PLANE, apl2 = (g16 < 2 ? 0 : 2) * A_PLANE;  // [hi|mid], [hi|lo]
  const int arow = hh16 * HS + (2 * wm) * SC + l16;  // source position (0, 0) of the wave's first row

  UP2C_DMA(0);
  UP2C_LOAD_A(0, 0, A_T);
  UP2C_SPLIT_A(0);
  UP2C_WRITE_A;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the slab has landed
  __syncthreads();
  X3_ST(1);
  static_assert(A_T < kUp2cTaps - 1, "one gather item per step, then the slab DMA");
  for (int kc = 0; kc < nch; ++kc) {
    __builtin_amdgcn_sched_barrier(0);
    X3_ST(2 + 4 * kc);
    bf16x8 gb[2][3][2];  // B fragments (g1, g2, g3) of a phase-tap, by step parity
    bf16x8 fa[2][2][2];  // A fragments (f1, f2) of the two source rows, by position parity
    const u32x4* __restrict__ bs = Bs + (kc & (SLABS - 1)) * B_UNITS;
    const u32x4* __restrict__ bp1 = bs;                                           // hi
    const u32x4* __restrict__ bp2 = bs + (g16 < 2 ? B_PLANE : 0);                 // mid | hi
    const u32x4* __restrict__ bp3 = bs + (g16 < 2 ? 2 * B_PLANE : B_PLANE);       // lo | mid
#define UP2C_READ_B(BUF, TAP)                                                                           \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                     \
      const int bi = ((TAP) * 2 + hh16) * BN + q * 16 + l16;                                            \
      gb[BUF][0][q] = __builtin_bit_cast(bf16x8, bp1[bi]);                                              \
      gb[BUF][1][q] = __builtin_bit_cast(bf16x8, bp2[bi]);                                              \
      gb[BUF][2][q] = __builtin_bit_cast(bf16x8, bp3[bi]);                                              \
    }
#define UP2C_READ_A(POS)                                                                                \
    _Pragma("unroll") for (int r = 0; r < 2; ++r) {                                                     \
      const int ai = arow + (r + (POS) / 3) * SC + (POS) % 3;                                           \
      fa[(POS) & 1][r][0] = __builtin_bit_cast(bf16x8, As[apl1 + ai]);                                  \
      fa[(POS) & 1][r][1] = __builtin_bit_cast(bf16x8, As[apl2 + ai]);                                  \
    }
    UP2C_READ_B(0, up2c_tap(0));
    UP2C_READ_A(0);
#pragma unroll
    for (int st = 0; st < kUp2cTaps; ++st) {
      const int c = up2c_tap(st), py = c >> 3, px = (c >> 2) & 1, pos = up2c_pos(c), ab = pos & 1, bb = st & 1;
      // the next chunk's gather, one item per step, then its weight slab into the other buffer
      if (st < A_T && kc + 1 < nch) {
        __builtin_amdgcn_sched_barrier(0);
        UP2C_LOAD_A(kc + 1, st, st + 1)
        __builtin_amdgcn_sched_barrier(0);
      }
      if (SLABS == 2 && st == A_T && kc + 1 < nch) {
        __builtin_amdgcn_sched_barrier(0);
        UP2C_DMA(kc + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      int nrd = 0;
      if (st + 1 < kUp2cTaps) {
        UP2C_READ_B(bb ^ 1, up2c_tap(st + 1));
        nrd = 6;
        if (up2c_pos(up2c_tap(st + 1)) != pos) {
          UP2C_READ_A(up2c_pos(up2c_tap(st + 1)));
          nrd += 4;
        }
      }
      // the three products of an accumulator in the M16 kernel's order, product-major
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
          acc[r][py][px][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ab][r][0], gb[bb][2][q], acc[r][py][px][q], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
          acc[r][py][px][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ab][r][1], gb[bb][1][q], acc[r][py][px][q], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q)
          acc[r][py][px][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ab][r][0], gb[bb][0][q], acc[r][py][px][q], 0, 0, 0);
      // one LDS read per MFMA while the next step's reads last, then the rest of the 12 MFMAs
#pragma unroll
      for (int r = 0; r < nrd; ++r) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      if (nrd == 10) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      else if (nrd == 6) __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
      else __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#undef UP2C_READ_A
#undef UP2C_READ_B
    __builtin_amdgcn_sched_barrier(0);
    X3_ST(3 + 4 * kc);
    if (kc + 1 < nch) {
      UP2C_SPLIT_A(kc + 1);
      if constexpr (SLABS == 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the next slab has landed
        __syncthreads();  // every wave is done reading this chunk's A tile
        X3_ST(4 + 4 * kc);
        UP2C_WRITE_A;
        __syncthreads();
      } else {
        // one slab buffer: it is refilled once every wave is done reading it. Nothing orders another
        // wave's ds_read behind a pending LDS-DMA but the issuing wave's vmcnt wait and a barrier
        // after it: the landing is exposed here, for the CU's other workgroup to run under.
        __syncthreads();  // every wave is done reading this chunk's A tile and slab (no DMA pending)
        X3_ST(4 + 4 * kc);
        UP2C_DMA(kc + 1);
        UP2C_WRITE_A;
        X3_ST(120 + kc);  // SLABS = 1 only: slab DMA issued and A tile written; to 5 + 4 kc = the exposed landing
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the next slab has landed
        __syncthreads();
      }
      X3_ST(5 + 4 * kc);
    }
  }
#undef UP2C_LOAD_A
#undef UP2C_DMA
#undef UP2C_SPLIT_A
#undef UP2C_WRITE_A

  // staged epilogue: lane (l16, g16) holds source pixels 4 g16 + k of channel 16 q + l16 for both
  // px, i.e. output pixels 8 g16 .. + 7 once interleaved: two float4 per (output row, channel)
  __syncthreads();  // every wave is done reading the last chunk's tiles
  X3_ST(2 + 4 * nch);
  float* region = reinterpret_cast<float*>(x3_smem) + wm * 32 * 4 * 36;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int co = n0 + 16 * q + l16;
    const float bv = (co < a.Cout && a.bias) ? a.bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int py = 0; py < 2; ++py) {
        const f32x4v v0 = acc[r][py][0][q], v1 = acc[r][py][1][q];
        float* dst = region + ((16 * q + l16) * 4 + 2 * r + py) * 36 + 8 * g16;
        *reinterpret_cast<float4*>(dst) = make_float4(v0[0] + bv, v1[0] + bv, v0[1] + bv, v1[1] + bv);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(v0[2] + bv, v1[2] + bv, v0[3] + bv, v1[3] + bv);
      }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  store_region<4>(a, region, n, x0, y0, 4 * wm, n0, lane);
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
      rec[197] = WM * 16 + SLABS;  // the up2c form (0 in conv3x3_x3_kernel's records)
    }
  }
#endif
}

// collapsed upsampled conv (conv3x3_up2c_kernel): 32x32 px x 32 ch tiles, 8 waves; not in kConfigs --
// it reads the collapsed slab, a buffer of its own (ast_conv3x3_up2c_fwd_f32)
constexpr int kUp2cFourWaveMaxChunks = 16;  // K chunks per block up to which a full launch takes the 4-wave form

template <int WM, int SLABS>
const void* up2c_kernel_ptr() {  // the kernel with its dynamic-LDS attribute set (once per instantiation)
  using U = Up2cCfg<WM, SLABS>;
  static_assert(U::LDS_BYTES * U::OCC <= 160 * 1024, "LDS per CU");
  static const void* const kern = with_dynamic_lds((const void*)conv3x3_up2c_kernel<WM, SLABS>, U::LDS_BYTES);
  return kern;
}

template <int WM, int SLABS>
int launch_up2c_one(const ConvArgs& a0, const float* w_up2c, hipStream_t s) {
  using U = Up2cCfg<WM, SLABS>;
  ConvArgs a = a0;
  int64_t nblk;  // (kUp2cBN divides kCoutAlign: the slab-width check of conv_grid never refuses)
  if (const int e = conv_grid(a, U::X::TH, kUp2cBN, nblk)) return e;
  (void)up2c_kernel_ptr<WM, SLABS>();
  hipLaunchKernelGGL((conv3x3_up2c_kernel<WM, SLABS>), dim3((unsigned)nblk), dim3(U::X::NT), U::LDS_BYTES, s, a,
                     reinterpret_cast<const u32x4*>(w_up2c));
  return (int)hipGetLastError();
}

// The form auto takes (8: 8 waves, one workgroup per CU; 4: 4 waves, one slab buffer, two per CU).
// AST_UP2C_TILE=8|4 (read once) forces one for A/B runs; the rule is the measured one of DESIGN.md §3.
int up2c_auto_variant(const ConvArgs& a) {
  static const int forced = ast_env::get("AST_UP2C_TILE", 0);
  if (forced == 4 || forced == 8) return forced;
  // measured (profiles/r08_up2c_*): a launch whose 8-wave workgroups do not fill the
  // CUs runs on twice as many as 4-wave ones; a full launch gains most where prologue and epilogue
  // weigh most (-18% at 4 chunks per block, -3% at 16 inside the decoder); past 16 nothing is measured
  if (conv_blocks(a, Up2cCfg<8, 2>::X::TH, kUp2cBN) < cu_count()) return 4;
  return cdiv(a.Cin, kX3K) <= kUp2cFourWaveMaxChunks ? 4 : 8;
}

int launch_up2c(const ConvArgs& a, const float* w_up2c, hipStream_t s, int variant) {
  if (variant == 0) variant = up2c_auto_variant(a);
  if (variant == 4) return launch_up2c_one<4, 1>(a, w_up2c, s);
  if (variant == 8) return launch_up2c_one<8, 2>(a, w_up2c, s);
  return AST_E_UNSUPPORTED;
}

}  // namespace

extern "C" {

size_t ast_conv3x3_up2c_numel(int cout, int cin) {
  if (cout <= 0 || cin <= 0) return 0;
  return (size_t)up2c_numel(cin, cout);
}

int ast_conv3x3_pack_up2c_f32(const float* w_packed, float* w_up2c, int cout, int cin, void* stream) {
  if (!w_packed || !w_up2c) return AST_E_NULLPTR;
  if (cout <= 0 || cin <= 0) return AST_E_SHAPE;
  const int cout_pad = round_up(cout, kCoutAlign);
  const int64_t total = (int64_t)round_up(cin, kX3K) * kUp2cTaps * cout_pad;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(pack_up2c_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_packed,
                     reinterpret_cast<bf16*>(w_up2c), round_up(cin, kCinAlign), round_up(cin, kX3K), cout_pad);
  return (int)hipGetLastError();
}

int ast_conv3x3_up2c_fwd_f32_cfg(int variant, const float* x, const float* x2, int n2, const float* w_up2c,
                                 const float* bias, float* y_pre, float* y_act, int n, int cin, int h_in, int w_in,
                                 int cout, int upsample, int pad_mode, void* stream) {
  if (!x || !w_up2c) return AST_E_NULLPTR;
  if (variant != 0 && variant != 4 && variant != 8) return AST_E_UNSUPPORTED;
  if (n2 < 0 || (n2 > 0 && !x2)) return AST_E_NULLPTR;
  if (!y_pre && !y_act) return AST_E_NULLPTR;
  if (n <= 0 || cin <= 0 || h_in <= 0 || w_in <= 0 || cout <= 0) return AST_E_SHAPE;
  if (upsample != 2 || pad_mode != 1 || cin < kX3K) return AST_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(w_up2c) & 15) != 0) return AST_E_UNSUPPORTED;  // 16-byte slab units
  if ((int64_t)cin * h_in * w_in * 4 >= ((int64_t)1 << 31)) return AST_E_UNSUPPORTED;  // 32-bit buffer offsets
  if ((int64_t)round_up(cin, kX3K) * kUp2cTaps * round_up(cout, kCoutAlign) >= ((int64_t)1 << 31)) return AST_E_SHAPE;
  ConvArgs a{};
  a.x = x; a.x2 = x2; a.nsplit = n; a.bias = bias;
  a.y_pre = y_pre; a.y_act = y_act;
  a.N = n + n2; a.Cin = cin; a.Hin = h_in; a.Win = w_in; a.Cout = cout; a.H = 2 * h_in; a.W = 2 * w_in;
  a.cin_pad = round_up(cin, kCinAlign);
  a.cout_pad = round_up(cout, kCoutAlign);
  a.reflect = 1;
  return launch_up2c(a, w_up2c, (hipStream_t)stream, variant);
}

int ast_conv3x3_up2c_fwd_f32(const float* x, const float* x2, int n2, const float* w_up2c, const float* bias,
                             float* y_pre, float* y_act, int n, int cin, int h_in, int w_in, int cout, int upsample,
                             int pad_mode, void* stream) {
  return ast_conv3x3_up2c_fwd_f32_cfg(0, x, x2, n2, w_up2c, bias, y_pre, y_act, n, cin, h_in, w_in, cout, upsample,
                                      pad_mode, stream);
}

int ast_conv3x3_up2c_variant(int n, int cin, int h_in, int w_in, int cout) {
  if (n <= 0 || cin <= 0 || h_in <= 0 || w_in <= 0 || cout <= 0) return AST_E_SHAPE;
  ConvArgs a{};
  a.N = n; a.Cin = cin; a.Cout = cout; a.H = 2 * h_in; a.W = 2 * w_in;
  return up2c_auto_variant(a);
}

int ast_conv3x3_up2c_occupancy(int variant) {
  int nb = 0;
  hipError_t e = hipErrorInvalidValue;
  if (variant == 4)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, up2c_kernel_ptr<4, 1>(), Up2cCfg<4, 1>::X::NT, Up2cCfg<4, 1>::LDS_BYTES);
  else if (variant == 8)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, up2c_kernel_ptr<8, 2>(), Up2cCfg<8, 2>::X::NT, Up2cCfg<8, 2>::LDS_BYTES);
  return e == hipSuccess ? nb : -1;
}

#if X3_STAMP
// diagnostic build of this file only: the stamp records of conv3x3_up2c_kernel (conv_x3.h)
int ast_dbg_x3_stamps(void* host, size_t bytes, int clear) { return x3_stamps_read(host, bytes, clear); }
#endif

}  // extern "C"
