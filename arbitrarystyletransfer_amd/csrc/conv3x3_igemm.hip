// 3x3 stride-1 convolution as an MFMA-fp32 implicit GEMM for gfx950 (MI355X / CDNA4).
//
// Replaces the reference's nn.Conv2d(k3,p1)+ReLU(+MaxPool) chain of PretrainedEncoder
// (models.py:199-240) and the [Upsample]+ReflectionPad+Conv+ReLU chain of the mirrored decoder
// (models.py:598-628). GEMM view: out[pixel][cout] = sum_{cin,tap} in[pixel+tap][cin] * w[cin,tap][cout].
//
// Design:
//  * v_mfma_f32_32x32x2_f32: exact fp32 products (an fmaf chain), 64 FLOP/clk/SIMD = the
//    157.3 TF fp32 matrix peak. Lane l feeds A[i=l&31][k=l>>5] and B[k=l>>5][j=l&31].
//  * M = one 32-pixel output row segment per MFMA tile (lanes -> consecutive x: conflict-free
//    LDS reads and float4 NCHW stores), N = 32 output channels, K pair = two input channels at
//    the same tap.
//  * A workgroup owns a TH x 32 output tile x BN channels. Per K-chunk of CK input channels it
//    stages the SOURCE tile (before the x2 nearest upsample) with a 1-pixel halo in LDS: float4
//    row loads for the interior, scalar loads for the two halo columns, rows remapped for
//    zero / reflect padding. Upsample + reflect padding of the upsampled grid equals
//    replicate-padding of the source grid, so both are resolved by the per-lane LDS read
//    address. The conv_1 ImageNet normalisation is applied to loaded values (padding stays 0,
//    as the reference pads the normalised image). The CK x 9 x BN weight slab is staged beside
//    it; both double-buffered, next chunk's global loads in flight while the MFMAs run.
//  * Epilogue: bias, optional pre-ReLU store (the conv_i taps of the loss network), ReLU store,
//    and a fused 2x2 max-pool done in registers (a lane holds both rows of a window).
//
// This file also holds the configuration table (kConfigs), the heuristic (auto_config) and the conv
// C ABI. The other kernel families are translation units of their own, reached through the launcher
// declarations of conv_common.h (which lists them) and cin3.h.
#include <algorithm>
#include "conv_common.h"
#include "cin3.h"
#include "env.h"

namespace {

using namespace ast_conv;

typedef float f32x4 __attribute__((ext_vector_type(4)));  // register staging (HIP float4 arrays defeat SROA)

template <int WM, int WN, int RM, int RN, int CK, int UP>
struct Cfg {
  static constexpr int NT = WM * WN * 64;
  static constexpr int TH = WM * RM;             // output rows per tile
  static constexpr int BN = WN * RN * 32;        // output channels per tile
  static constexpr int SW = TW / UP;             // source columns per tile (interior)
  static constexpr int SR = TH / UP + 2;         // source rows per tile incl. halo
  static constexpr int RS = SW + 8;              // LDS row stride: [pad3|halo|interior(16B aligned)|halo|pad]
  static constexpr int C0 = 4;                   // LDS column of source column sx0
  static constexpr int A_ELEMS = CK * SR * RS;
  static constexpr int B_ELEMS = CK * 9 * BN;
  static constexpr int QV = SW / 4;              // float4 per interior row
  static constexpr int A_ITEMS = CK * SR * (QV + 2);     // fast path: QV vectors + 2 halo scalars per row
  static constexpr int A_PER_T = (A_ITEMS + NT - 1) / NT;
  static constexpr int S_ITEMS = CK * SR * (SW + 2);     // slow path: scalar per column
  static constexpr int B_VEC = B_ELEMS / 4;
  static constexpr int B_PER_T = (B_VEC + NT - 1) / NT;
  static constexpr int LDS_BYTES = 2 * (A_ELEMS + B_ELEMS) * 4;
};

template <int WM, int WN, int RM, int RN, int CK, int UP, bool SWAP, bool NORM>
__global__ __launch_bounds__(WM * WN * 64, WM * WN >= 16 ? 1 : 2) void conv3x3_f32_kernel(ConvArgs a) {
  using C = Cfg<WM, WN, RM, RN, CK, UP>;
  constexpr int NT = C::NT, TH = C::TH, BN = C::BN, SW = C::SW, SR = C::SR, RS = C::RS, QV = C::QV;
  constexpr int A_ELEMS = C::A_ELEMS, B_ELEMS = C::B_ELEMS;
  static_assert(CK % 2 == 0, "two channels per MFMA k-pair");
  static_assert(TH % 2 == 0, "even tile height (pool windows, upsample row pairs)");
  static_assert(UP == 1 || UP == 2, "");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                // [2][CK][SR][RS]
  float* Bs = smem + 2 * A_ELEMS;  // [2][CK*9][BN]

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int h = lane >> 5, l32 = lane & 31;
  const int wm = wave % WM, wn = wave / WM;

  int t, grp;
  if (!decode_block(blockIdx.x, a.tiles_x * a.tiles_y * a.N, (a.Cout + BN - 1) / BN, t, grp)) return;
  const int tx = t % a.tiles_x;
  t /= a.tiles_x;
  const int ty = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int x0 = tx * TW, y0 = ty * TH;
  const int sx0 = x0 / UP, sy0 = y0 / UP - 1;  // source tile origin (row includes the halo)
  const int n0 = grp * BN;
  const int Hin = a.Hin, Win = a.Win;
  const bool fast = (sx0 + SW <= Win) && ((Win & 3) == 0);  // block-uniform

  const float* __restrict__ xin =
      n < a.nsplit ? a.x + (int64_t)n * a.Cin * Hin * Win : a.x2 + (int64_t)(n - a.nsplit) * a.Cin * Hin * Win;
  const int plane_in = Hin * Win;
  const int nchunks = (a.Cin + CK - 1) / CK;

  f32x16 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Per-lane LDS column of the A operand for each kx: source column of output x0+l32+kx-1.
  int acol[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) acol[kx] = C::C0 + (((x0 + l32 + kx - 1) >> (UP - 1)) - sx0);
  const int abase = h * SR * RS;                       // lane half h reads channel 2kp+h
  const int bbase = h * 9 * BN + wn * RN * 32 + l32;

  // One K-chunk of MFMAs from LDS buffer `buf` (CK input channels x 9 taps).
#define CONV_CHUNK_MFMA(buf)                                                                                 \
  {                                                                                                         \
    const float* as = As + (buf) * A_ELEMS + abase;                                                         \
    const float* bs = Bs + (buf) * B_ELEMS + bbase;                                                         \
    _Pragma("unroll") for (int ky = 0; ky < 3; ++ky) {                                                      \
      _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) {                                                    \
        const int tap = ky * 3 + kx;                                                                        \
        _Pragma("unroll") for (int kp = 0; kp < CK / 2; ++kp) {                                             \
          float av[RM], bv[RN];                                                                             \
          _Pragma("unroll") for (int i = 0; i < RM; ++i) {                                                  \
            const int orow = wm * RM + i + ky - 1; /* -1 .. TH */                                           \
            const int srow = (UP == 1) ? orow + 1 : (orow >> 1) + 1;                                        \
            av[i] = as[(2 * kp * SR + srow) * RS + acol[kx]];                                               \
          }                                                                                                 \
          _Pragma("unroll") for (int j = 0; j < RN; ++j) bv[j] = bs[(2 * kp * 9 + tap) * BN + j * 32];      \
          _Pragma("unroll") for (int i = 0; i < RM; ++i)                                                    \
            _Pragma("unroll") for (int j = 0; j < RN; ++j)                                                  \
              acc[i][j] = SWAP ? __builtin_amdgcn_mfma_f32_32x32x2f32(bv[j], av[i], acc[i][j], 0, 0, 0)     \
                               : __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);    \
        }                                                                                                   \
      }                                                                                                     \
    }                                                                                                       \
  }

  // Weight slab staging: B_VEC float4 per chunk; indices past the slab are clamped onto its last
  // vector (duplicate loads and identical LDS writes, no branch).
  constexpr int B_VEC = C::B_VEC, B_T = C::B_PER_T;
  int boff[B_T];
#pragma unroll
  for (int i = 0; i < B_T; ++i) {
    const int vi = min(tid + i * NT, B_VEC - 1), f = vi * 4, row = f / BN;
    boff[i] = row * a.cout_pad + (f - row * BN);
  }
  const float* __restrict__ wbase = a.wp + n0;

  if (fast) {
    // Source-tile staging, branch-free: per-lane offsets computed once per tile; per chunk the
    // channel base is a wave-uniform pointer. Interior items are float4 row pieces; each halo item
    // is the aligned float4 that holds the (zero / reflect / replicate) halo column, one component kept.
    constexpr int AI = CK * SR * QV, AI_T = (AI + NT - 1) / NT;
    constexpr int AH = CK * SR * 2, AH_T = (AH + NT - 1) / NT;
    int ai_g[AI_T], ai_l[AI_T], ai_c[AI_T];
    bool ai_ok[AI_T];
#pragma unroll
    for (int i = 0; i < AI_T; ++i) {
      const int e = min(tid + i * NT, AI - 1), q = e % QV, cr = e / QV, r = cr % SR, c = cr / SR;
      const int sy = src_index<UP>(sy0 + r, Hin, a.reflect);
      ai_ok[i] = sy >= 0;
      ai_c[i] = c;
      ai_g[i] = c * plane_in + max(sy, 0) * Win + sx0 + 4 * q;
      ai_l[i] = cr * RS + C::C0 + 4 * q;
    }
    int ah_g[AH_T], ah_l[AH_T], ah_c[AH_T], ah_k[AH_T];  // ah_k: component 0..3, or -1 = zero
#pragma unroll
    for (int i = 0; i < AH_T; ++i) {
      const int e = min(tid + i * NT, AH - 1), side = e & 1, cr = e >> 1, r = cr % SR, c = cr / SR;
      const int sy = src_index<UP>(sy0 + r, Hin, a.reflect);
      const int sx = src_index<UP>(side ? sx0 + SW : sx0 - 1, Win, a.reflect);
      const bool ok = sy >= 0 && sx >= 0;
      ah_k[i] = ok ? (sx & 3) : -1;
      ah_c[i] = c;
      ah_g[i] = c * plane_in + max(sy, 0) * Win + (ok ? (sx & ~3) : 0);
      ah_l[i] = cr * RS + (side ? C::C0 + SW : C::C0 - 1);
    }
    f32x4 ra[AI_T], rh[AH_T], rb[B_T];
    float nm[NORM ? AI_T : 1], ns[NORM ? AI_T : 1], hm[NORM ? AH_T : 1], hs[NORM ? AH_T : 1];

    // issue every global load of chunk KC (no waits: the values are consumed by CONV_WRITE_CHUNK).
    // (macros, not lambdas: a by-reference closure over the register arrays sends them to scratch)
#define CONV_LOAD_CHUNK(KC)                                                                               \
    {                                                                                                     \
      const int cin0 = (KC) * CK;                                                                         \
      const int cmax = a.Cin - 1 - cin0; /* chunk channels > cmax are zero */                             \
      const float* __restrict__ xb = xin + (int64_t)cin0 * plane_in;                                      \
      _Pragma("unroll") for (int i = 0; i < AI_T; ++i) {                                                  \
        ra[i] = *reinterpret_cast<const f32x4*>(xb + (ai_c[i] <= cmax ? ai_g[i] : 0));                   \
        if (NORM) {                                                                                       \
          const int ch = cin0 + min(ai_c[i], cmax);                                                       \
          nm[i] = a.in_mean[ch];                                                                          \
          ns[i] = a.in_std[ch];                                                                           \
        }                                                                                                 \
      }                                                                                                   \
      _Pragma("unroll") for (int i = 0; i < AH_T; ++i) {                                                  \
        rh[i] = *reinterpret_cast<const f32x4*>(xb + (ah_c[i] <= cmax ? ah_g[i] : 0));                   \
        if (NORM) {                                                                                       \
          const int ch = cin0 + min(ah_c[i], cmax);                                                       \
          hm[i] = a.in_mean[ch];                                                                          \
          hs[i] = a.in_std[ch];                                                                           \
        }                                                                                                 \
      }                                                                                                   \
      const float* __restrict__ wb = wbase + (int64_t)cin0 * 9 * a.cout_pad;                              \
      _Pragma("unroll") for (int i = 0; i < B_T; ++i) rb[i] = *reinterpret_cast<const f32x4*>(wb + boff[i]); \
    }
#define CONV_WRITE_CHUNK(KC, BUF)                                                                         \
    {                                                                                                     \
      const int cmax = a.Cin - 1 - (KC) * CK;                                                             \
      float* as = As + (BUF) * A_ELEMS;                                                                   \
      _Pragma("unroll") for (int i = 0; i < AI_T; ++i) {                                                  \
        f32x4 v = ra[i];                                                                                  \
        if (NORM) v = (v - nm[i]) / ns[i];                                                                \
        if (!(ai_ok[i] && ai_c[i] <= cmax)) v = f32x4{0.f, 0.f, 0.f, 0.f};                                \
        *reinterpret_cast<f32x4*>(as + ai_l[i]) = v;                                                      \
      }                                                                                                   \
      _Pragma("unroll") for (int i = 0; i < AH_T; ++i) {                                                  \
        const int k = ah_k[i];                                                                            \
        const f32x4 q4 = rh[i];                                                                           \
        float v = k == 0 ? q4.x : (k == 1 ? q4.y : (k == 2 ? q4.z : q4.w));                               \
        if (NORM) v = (v - hm[i]) / hs[i];                                                                \
        as[ah_l[i]] = (k >= 0 && ah_c[i] <= cmax) ? v : 0.f;                                              \
      }                                                                                                   \
      float* bs = Bs + (BUF) * B_ELEMS;                                                                   \
      _Pragma("unroll") for (int i = 0; i < B_T; ++i)                                                     \
        *reinterpret_cast<f32x4*>(bs + min(tid + i * NT, B_VEC - 1) * 4) = rb[i];                         \
    }

    CONV_LOAD_CHUNK(0);
    CONV_WRITE_CHUNK(0, 0);
    __syncthreads();
    for (int kc = 0; kc < nchunks; ++kc) {
      const int buf = kc & 1;
      const int kn = min(kc + 1, nchunks - 1);  // the last iteration re-loads into the idle buffer
      CONV_LOAD_CHUNK(kn);
      __builtin_amdgcn_sched_barrier(0);         // keep the loads ahead of the MFMAs
      CONV_CHUNK_MFMA(buf);
      __builtin_amdgcn_sched_barrier(0);
      CONV_WRITE_CHUNK(kn, buf ^ 1);
      __syncthreads();
    }
  } else {
    // Irregular tiles (right edge narrower than the tile, or W % 4 != 0): scalar gather, no prefetch.
    auto fill_a_slow = [&](int cin0, float* as) {
      for (int e = tid; e < C::S_ITEMS; e += NT) {
        const int col = e % (SW + 2);
        const int cr = e / (SW + 2);
        const int r = cr % SR, c = cr / SR;
        const int cin = cin0 + c;
        const int sy = src_index<UP>(sy0 + r, Hin, a.reflect);
        const int sx = src_index<UP>(sx0 - 1 + col, Win, a.reflect);
        float v = 0.f;
        if (cin < a.Cin && sy >= 0 && sx >= 0) {
          v = xin[cin * plane_in + sy * Win + sx];
          if (NORM) v = (v - a.in_mean[cin]) / a.in_std[cin];
        }
        as[cr * RS + C::C0 - 1 + col] = v;
      }
    };
    for (int kc = 0; kc < nchunks; ++kc) {
      const int cin0 = kc * CK;
      fill_a_slow(cin0, As);
      const float* __restrict__ wb = wbase + (int64_t)cin0 * 9 * a.cout_pad;
#pragma unroll
      for (int i = 0; i < B_T; ++i)
        *reinterpret_cast<float4*>(Bs + min(tid + i * NT, B_VEC - 1) * 4) = *reinterpret_cast<const float4*>(wb + boff[i]);
      __syncthreads();
      CONV_CHUNK_MFMA(0);
      __syncthreads();
    }
  }
#undef CONV_CHUNK_MFMA
#undef CONV_LOAD_CHUNK
#undef CONV_WRITE_CHUNK

  // ---------------- epilogue ----------------
  const int H = a.H, W = a.W;
  const int64_t plane = (int64_t)H * W;
  const int Ho = H >> 1, Wo = W >> 1;
  if constexpr (SWAP) {
    // C^T: lane l32 = output column x0+l32, register r = channel (r&3)+8(r>>2)+4h of the
    // 32-channel tile. One dword store per register writes two whole 128-B row segments.
    const int xx = x0 + l32;
#pragma unroll
    for (int j = 0; j < RN; ++j) {
      const int cbase = n0 + (wn * RN + j) * 32 + 4 * h;
      float bvr[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cbase + (r & 3) + 8 * (r >> 2);
        bvr[r] = (co < a.Cout && a.bias) ? a.bias[co] : 0.f;
      }
      if (a.y_pre || a.y_act) {
#pragma unroll
        for (int i = 0; i < RM; ++i) {
          const int yy = y0 + wm * RM + i;
          if (yy >= H || xx >= W) continue;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = cbase + (r & 3) + 8 * (r >> 2);
            if (co >= a.Cout) continue;
            const float v = acc[i][j][r] + bvr[r];
            const int64_t off = ((int64_t)n * a.Cout + co) * plane + (int64_t)yy * W + xx;
            if (a.y_pre) a.y_pre[off] = v;
            if (a.y_act) a.y_act[off] = relu_f(v);
          }
        }
      }
      if (a.y_pool) {
        const int px = xx >> 1;
#pragma unroll
        for (int i = 0; i + 1 < RM; i += 2) {
          const int py = (y0 + wm * RM + i) >> 1;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = cbase + (r & 3) + 8 * (r >> 2);
            float m = max_nan(relu_f(acc[i][j][r] + bvr[r]), relu_f(acc[i + 1][j][r] + bvr[r]));
            m = max_nan(m, __shfl_xor(m, 1, 64));  // horizontal neighbour = adjacent lane
            if ((l32 & 1) == 0 && co < a.Cout && py < Ho && px < Wo)
              a.y_pool[((int64_t)n * a.Cout + co) * Ho * Wo + (int64_t)py * Wo + px] = m;
          }
        }
      }
    }
    return;
  }
  store_tiles<RM, RN>(a, acc, n, x0, y0, wm * RM, n0 + wn * RN * 32, h, l32);
}

__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int cout, int cin,
                                    int cout_pad, int cin_pad) {
  const int64_t total = (int64_t)cin_pad * 9 * cout_pad;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(idx % cout_pad);
    const int64_t rt = idx / cout_pad;
    const int tap = (int)(rt % 9);
    const int ci = (int)(rt / 9);
    wp[idx] = (ci < cin && co < cout) ? w[((int64_t)co * cin + ci) * 9 + tap] : 0.f;
  }
}

template <int WM, int WN, int RM, int RN, int CK, int UP, bool SWAP, bool NORM>
int launch_one(const ConvArgs& a0, hipStream_t s) {
  using C = Cfg<WM, WN, RM, RN, CK, UP>;
  ConvArgs a = a0;
  int64_t nblk;
  if (const int e = conv_grid(a, C::TH, C::BN, nblk)) return e;
  auto kern = conv3x3_f32_kernel<WM, WN, RM, RN, CK, UP, SWAP, NORM>;
  [[maybe_unused]] static const void* const attr_set = with_dynamic_lds((const void*)kern, C::LDS_BYTES);
  hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(C::NT), C::LDS_BYTES, s, a);
  return (int)hipGetLastError();
}

template <int WM, int WN, int RM, int RN, int CK, bool SWAP = false>
int launch_cfg(const ConvArgs& a, hipStream_t s, int up) {
  if (a.in_mean)  // ImageNet normalisation in the gather: conv_1 only (never upsampled)
    return up == 2 ? launch_one<WM, WN, RM, RN, CK, 2, SWAP, true>(a, s) : launch_one<WM, WN, RM, RN, CK, 1, SWAP, true>(a, s);
  return up == 2 ? launch_one<WM, WN, RM, RN, CK, 2, SWAP, false>(a, s) : launch_one<WM, WN, RM, RN, CK, 1, SWAP, false>(a, s);
}

// split-bf16 MFMA conv of a 1..3-channel input (conv_cin3.hip): no pool / upsample
template <int TH>
int launch_cin3x3(const ConvArgs& a, hipStream_t s, int up) {
  if (a.Cin > 3 || a.y_pool || up != 1) return AST_E_UNSUPPORTED;
  Cin3Args c{};
  c.x = a.x; c.x2 = a.x2; c.nsplit = a.nsplit; c.wp = a.wp; c.bias = a.bias;
  c.y_pre = a.y_pre; c.y_act = a.y_act; c.in_mean = a.in_mean; c.in_std = a.in_std;
  c.e_mask = a.e_mask; c.e_add_pre = a.e_add_pre; c.e_add_post = a.e_add_post;
  c.N = a.N; c.Cin = a.Cin; c.H = a.H; c.W = a.W; c.Cout = a.Cout; c.cout_pad = a.cout_pad; c.reflect = a.reflect;
  return launch_conv_cin3_x3(c, TH, s);
}

struct CfgEntry {
  int (*fn)(const ConvArgs&, hipStream_t, int);
  int bn;        // output channels per workgroup (weight-slab width)
  int th;        // output rows per workgroup
  int rm;        // output rows per wave (pool needs an even count)
  int max_cout;  // 0 = any
  int dgrad;     // input-gradient epilogue (ast_conv3x3_dgrad_f32): kNoDgrad, kDgrad, or kDgradSum2
};
// kDgrad: the kernel applies ConvArgs' e_mask / e_add_* on y_pre; kDgradSum2: also on the 2x2 sum in
// y_pool (e_sum2). An entry whose kernel lacks the epilogue leaves the field out (0).
enum { kNoDgrad = 0, kDgrad = 1, kDgradSum2 = 2 };

// Index -> configuration. Keep the table stable (tests/tuner address entries by index).
const CfgEntry kConfigs[] = {
    {launch_cfg<4, 1, 2, 2, 8>, 64, 8, 2, 0},    // 0: 8x32 px x 64 ch, CK 8, 4 waves
    {launch_cfg<4, 1, 2, 2, 4>, 64, 8, 2, 0},    // 1: 8x32 px x 64 ch, CK 4, 4 waves
    {launch_cfg<2, 2, 4, 2, 4>, 128, 8, 4, 0},   // 2: 8x32 px x 128 ch, CK 4, 4 waves
    {launch_cfg<2, 2, 2, 2, 8>, 128, 4, 2, 0},   // 3: 4x32 px x 128 ch, CK 8, 4 waves
    {launch_cfg<4, 1, 4, 2, 4>, 64, 16, 4, 0},   // 4: 16x32 px x 64 ch, CK 4, 4 waves
    {launch_cfg<2, 2, 2, 2, 4>, 128, 4, 2, 0},   // 5: 4x32 px x 128 ch, CK 4, 4 waves
    {launch_cfg<4, 2, 2, 2, 4>, 128, 8, 2, 0},   // 6: 8x32 px x 128 ch, CK 4, 8 waves
    {launch_cfg<8, 1, 2, 2, 4>, 64, 16, 2, 0},   // 7: 16x32 px x 64 ch, CK 4, 8 waves
    {launch_cfg<4, 2, 4, 2, 4>, 128, 16, 4, 0},  // 8: 16x32 px x 128 ch, CK 4, 8 waves
    {launch_cfg<2, 1, 2, 2, 4>, 64, 4, 2, 0},    // 9: 4x32 px x 64 ch, CK 4, 2 waves
    {launch_smallc<3>, 4, 8, 2, 3},              // 10: direct VALU conv, cout <= 3
    {launch_smallc<4>, 4, 8, 2, 4},              // 11: direct VALU conv, cout <= 4
    // swapped operands (C^T: pixels on lanes -> whole-line dword stores)
    {launch_cfg<8, 1, 2, 2, 4, true>, 64, 16, 2, 0},   // 12: as 7
    {launch_cfg<4, 2, 2, 2, 4, true>, 128, 8, 2, 0},   // 13: as 6
    {launch_cfg<4, 2, 4, 2, 4, true>, 128, 16, 4, 0},  // 14: as 8
    {launch_cfg<4, 1, 2, 2, 4, true>, 64, 8, 2, 0},    // 15: as 1
    {launch_cfg<8, 2, 2, 2, 4>, 128, 16, 2, 0},        // 16: 16x32 px x 128 ch, CK 4, 16 waves (1 WG/CU)
    {launch_cfg<8, 2, 2, 2, 4, true>, 128, 16, 2, 0},  // 17: as 16, swapped
    {launch_cin4<8, false>, 64, 8, 1, 0, kDgrad},       // 18: direct VALU conv, cin <= 4, no pool/upsample
    {launch_cin4<16, false>, 64, 16, 1, 0, kDgrad},     // 19: as 18, 16-row tiles
    {launch_cin4<8, true>, 64, 8, 1, 0, kDgrad},        // 20: as 18, nontemporal stores
    {launch_cin4<4, false>, 64, 4, 1, 0, kDgrad},       // 21: as 18, 4-row tiles
    {launch_cin4<16, true>, 64, 16, 1, 0, kDgrad},      // 22: 16-row tiles, nontemporal stores
    {launch_cin4<32, true>, 64, 32, 1, 0, kDgrad},      // 23: 32-row tiles, nontemporal stores
    // split-bf16 (fp32-accurate) MFMA implicit GEMM
    {launch_x3<8, 2, 2>, 64, 16, 2, 0, kDgradSum2},     // 24: 16x32 px x 64 ch, 8 waves
    {launch_x3<4, 2, 2>, 64, 8, 2, 0, kDgradSum2},      // 25: 8x32 px x 64 ch, 4 waves
    {launch_x3<4, 2, 1, 2>, 32, 8, 2, 0, kDgradSum2},   // 26: 8x32 px x 32 ch, 4 waves, 2 workgroups/CU
    {launch_x3<8, 2, 1, 1>, 32, 16, 2, 0, kDgradSum2},  // 27: 16x32 px x 32 ch, 8 waves
    // the same tiles on the 16x16x32 bf16 MFMA (three K-32 products per block)
    {launch_x3<8, 2, 2, 1, true>, 64, 16, 2, 0, kDgradSum2},  // 28: as 24
    {launch_x3<4, 2, 2, 1, true>, 64, 8, 2, 0, kDgradSum2},  // 29: as 25
    {launch_x3<4, 2, 1, 2, true>, 32, 8, 2, 0, kDgradSum2},  // 30: as 26
    {launch_x3<8, 2, 1, 1, true>, 32, 16, 2, 0, kDgradSum2},  // 31: as 27
    // persistent forms of 28-31 (next block's first chunk under the last MFMAs, store tail overlapped)
    {launch_x3p<8, 2, 2>, 64, 16, 2, 0, kDgradSum2},    // 32: as 28
    {launch_x3p<4, 2, 2>, 64, 8, 2, 0, kDgradSum2},     // 33: as 29
    {launch_x3p<4, 2, 1, 2>, 32, 8, 2, 0, kDgradSum2},  // 34: as 30
    {launch_x3p<8, 2, 1, 1>, 32, 16, 2, 0, kDgradSum2},  // 35: as 31
    // register-streaming direct VALU conv for cout <= 4 (no LDS tile, no per-channel barrier)
    {launch_smallc2<3>, 4, 8, 2, 3},                    // 36: cout <= 3
    {launch_smallc2<4>, 4, 8, 2, 4},                    // 37: cout <= 4
    // persistent forms of 28-31 (round 5): the same kernel looping over blocks (the kernel has the
    // input-gradient epilogue, but ast_conv3x3_dgrad_f32 has never taken these: left refused)
    {launch_x3<8, 2, 2, 1, true, true>, 64, 16, 2, 0},  // 38: as 28
    {launch_x3<4, 2, 2, 1, true, true>, 64, 8, 2, 0},   // 39: as 29
    {launch_x3<4, 2, 1, 2, true, true>, 32, 8, 2, 0},   // 40: as 30
    {launch_x3<8, 2, 1, 1, true, true>, 32, 16, 2, 0},  // 41: as 31
    // split-bf16 MFMA conv of a 1..3-channel input, K = 27 in one K-32 block (round 6, conv_cin3.hip)
    {launch_cin3x3<16>, 64, 16, 1, 0, kDgrad},          // 42: 16x64 px x 64 ch, 4 waves
    {launch_cin3x3<8>, 64, 8, 1, 0, kDgrad},            // 43: 8x64 px x 64 ch, 4 waves
};
constexpr int kNumConfigs = sizeof(kConfigs) / sizeof(kConfigs[0]);

int auto_config(int cin, int cout, int n, int h, int w, int up, bool pool, bool norm) {
  // cout <= 4: the register-streaming direct conv where it applies (W % 4 == 0, no upsample / pool /
  // normalisation), else the LDS-staged one (profiles/r05_smallc.txt: 8x64x512^2 -> 3, 0.294 -> 0.226 ms)
  if (cout <= 4 && up == 1 && !pool && !norm && (w & 3) == 0) return cout <= 3 ? 36 : 37;
  if (cout <= 3) return 10;
  if (cout <= 4) return 11;
  // image-input convs (conv_1) and the decoder's last input gradient: the split-bf16 MFMA kernel for
  // cin <= 3 (profiles/r06c3_ab5.txt: 16 x 64 x 512^2 conv_1 0.41 -> 0.31 ms), else the direct conv
  if (cin <= 3 && up == 1 && !pool) return 42;
  if (cin <= 4 && up == 1 && !pool) return 20;
  if (cin >= kX3K && !norm && (long)cin * (h / up) * (w / up) * 4 < (1L << 31)) {
    // split-bf16 MFMA (fp32-accurate, 2.67x the fp32 matrix rate): 8x32 px x 32 ch tiles, two
    // workgroups per CU; upsampled convs the 16-row tile (profiles/r02_conv_cfgs.log)
    const long t16 = (long)n * cdiv(h, 16) * cdiv(w, 32) * cdiv(cout, 32);
    return (up == 2 && t16 >= 512) ? 27 : 26;
  }
  // 16x32 px x 64 ch, 8 waves: fastest on every VGG shape measured (profiles/, conv_tuning.json);
  // the 4-wave 8x32 tile when that leaves too few workgroups to fill 256 CUs.
  const long tiles = (long)n * cdiv(h, 16) * cdiv(w, 32) * cdiv(cout, 64);
  return tiles >= 256 ? 7 : 1;
}

// AST_CONV_M16=0|1 (default 1): the split-bf16 tiles on the 32x32x16 MFMA (24-27) | the 16x16x32 one (28-31),
// for the forward and the dgrad entry alike
int m16_config(int cfg) {
  static const int m16 = ast_env::get("AST_CONV_M16", 1);
  if (cfg >= 24 && cfg <= 27 && m16 == 1) return cfg + 4;
  if (cfg >= 28 && cfg <= 31 && m16 == 0) return cfg - 4;
  return cfg;
}

}  // namespace

extern "C" {

const char* ast_version(void) { return "ast_hip 0.3 gfx950"; }

int ast_loss_acc_floats(void) { return AST_LOSS_ACC_FLOATS; }

size_t ast_conv3x3_packed_numel(int cout, int cin) {
  if (cout <= 0 || cin <= 0) return 0;
  const size_t cout_pad = (size_t)round_up(cout, kCoutAlign);
  // fp32 pack [cin_pad8][9][cout_pad], then the split-bf16 pack [cin_pad16][9][cout_pad] x 3 bf16
  return (size_t)round_up(cin, kCinAlign) * 9 * cout_pad + (size_t)round_up(cin, kX3K) * 9 * cout_pad * 3 / 2;
}

int ast_conv3x3_pack_weights_f32(const float* w, float* w_packed, int cout, int cin, void* stream) {
  if (!w || !w_packed) return AST_E_NULLPTR;
  if (cout <= 0 || cin <= 0) return AST_E_SHAPE;
  const int cout_pad = round_up(cout, kCoutAlign), cin_pad = round_up(cin, kCinAlign);
  const int64_t total = (int64_t)cin_pad * 9 * cout_pad;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, w_packed, cout, cin,
                     cout_pad, cin_pad);
  const int e = (int)hipGetLastError();
  return e ? e : ast_conv3x3_pack_split_f32(w_packed, cout, cin, stream);
}

int ast_conv3x3_num_configs(void) { return kNumConfigs; }

int ast_conv3x3_fwd_f32_cfg(int cfg, const float* x, const float* x2, int n2, const float* w_packed,
                            const float* bias, float* y_pre, float* y_act, float* y_pool, const float* in_mean,
                            const float* in_std, int n, int cin, int h_in, int w_in, int cout, int upsample,
                            int pad_mode, void* stream) {
  if (!x || !w_packed) return AST_E_NULLPTR;
  if (n2 < 0 || (n2 > 0 && !x2)) return AST_E_NULLPTR;
  if (!y_pre && !y_act && !y_pool) return AST_E_NULLPTR;
  if ((in_mean == nullptr) != (in_std == nullptr)) return AST_E_NULLPTR;
  if (n <= 0 || cin <= 0 || h_in <= 0 || w_in <= 0 || cout <= 0) return AST_E_SHAPE;
  if (upsample != 1 && upsample != 2) return AST_E_UNSUPPORTED;
  if (pad_mode != 0 && pad_mode != 1) return AST_E_UNSUPPORTED;
  const int H = h_in * upsample, W = w_in * upsample;
  if (pad_mode == 1 && (H < 2 || W < 2)) return AST_E_SHAPE;  // ReflectionPad2d(1) needs size >= 2
  if ((int64_t)cin * h_in * w_in >= ((int64_t)1 << 31)) return AST_E_SHAPE;         // per-image offsets are 32-bit
  if ((int64_t)round_up(cin, kCinAlign) * 9 * round_up(cout, kCoutAlign) >= ((int64_t)1 << 31)) return AST_E_SHAPE;
  if (cfg < 0) cfg = auto_config(cin, cout, n + n2, H, W, upsample, y_pool != nullptr, in_mean != nullptr);
  if (cfg >= kNumConfigs) return AST_E_UNSUPPORTED;
  cfg = m16_config(cfg);
  const CfgEntry& e = kConfigs[cfg];
  if (y_pool && (e.rm % 2 != 0 || e.max_cout)) return AST_E_UNSUPPORTED;
  if (e.max_cout && cout > e.max_cout) return AST_E_UNSUPPORTED;
  if (e.bn > kCoutAlign && (cout % e.bn) != 0) return AST_E_UNSUPPORTED;
  ConvArgs a{};
  a.x = x; a.x2 = x2; a.nsplit = n; a.wp = w_packed; a.bias = bias;
  a.y_pre = y_pre; a.y_act = y_act; a.y_pool = y_pool;
  a.in_mean = in_mean; a.in_std = in_std;
  a.N = n + n2; a.Cin = cin; a.Hin = h_in; a.Win = w_in; a.Cout = cout; a.H = H; a.W = W;
  a.cin_pad = round_up(cin, kCinAlign);
  a.cout_pad = round_up(cout, kCoutAlign);
  a.reflect = pad_mode;
  return e.fn(a, (hipStream_t)stream, upsample);
}

int ast_conv3x3_dgrad_f32(int cfg, const float* dy, const float* w_tf_packed, float* dx, const float* mask,
                          const float* add_pre, const float* add_post, int n, int cout, int h, int w, int cin,
                          int upsample, void* stream) {
  if (!dy || !w_tf_packed || !dx) return AST_E_NULLPTR;
  if (n <= 0 || cout <= 0 || h <= 0 || w <= 0 || cin <= 0) return AST_E_SHAPE;
  if (upsample != 1 && upsample != 2) return AST_E_UNSUPPORTED;
  if (upsample == 2 && ((h | w) & 1)) return AST_E_SHAPE;  // the upsampled grid has even sides
  if ((int64_t)cout * h * w >= ((int64_t)1 << 31)) return AST_E_SHAPE;
  if ((int64_t)round_up(cout, kCinAlign) * 9 * round_up(cin, kCoutAlign) >= ((int64_t)1 << 31)) return AST_E_SHAPE;
  const bool sum2 = upsample == 2;
  if (cfg < 0) cfg = auto_config(cout, cin, n, h, w, 1, sum2, false);
  // which kernels have the epilogue, and which of them its 2x2-sum form, is the table's dgrad field
  if (cfg >= kNumConfigs || kConfigs[cfg].dgrad < (sum2 ? kDgradSum2 : kDgrad)) return AST_E_UNSUPPORTED;
  cfg = m16_config(cfg);
#if !X3_STAGED_EPI
  // the 32x32 kernels' direct-store epilogue (store_tiles) has no input-gradient epilogue: the
  // caller then runs the plain conv and ast_dgrad_finish_f32
  if (cfg >= 24 && cfg <= 27) return AST_E_UNSUPPORTED;
#endif
  const CfgEntry& e = kConfigs[cfg];
  if (sum2 && e.rm % 2 != 0) return AST_E_UNSUPPORTED;
  if (e.bn > kCoutAlign && (cin % e.bn) != 0) return AST_E_UNSUPPORTED;
  ConvArgs a{};
  a.x = dy; a.nsplit = n; a.wp = w_tf_packed;
  (sum2 ? a.y_pool : a.y_pre) = dx;
  a.e_mask = mask; a.e_add_pre = add_pre; a.e_add_post = add_post; a.e_sum2 = sum2 ? 1 : 0;
  a.N = n; a.Cin = cout; a.Hin = h; a.Win = w; a.Cout = cin; a.H = h; a.W = w;
  a.cin_pad = round_up(cout, kCinAlign);
  a.cout_pad = round_up(cin, kCoutAlign);
  a.reflect = 0;  // the interior of the padded-input gradient: a zero-padded same conv of dy
  return e.fn(a, (hipStream_t)stream, 1);
}

int ast_conv3x3_fwd_f32(const float* x, const float* w_packed, const float* bias, float* y_pre, float* y_act,
                        float* y_pool, const float* in_mean, const float* in_std, int n, int cin, int h_in, int w_in,
                        int cout, int upsample, int pad_mode, void* stream) {
  return ast_conv3x3_fwd_f32_cfg(-1, x, nullptr, 0, w_packed, bias, y_pre, y_act, y_pool, in_mean, in_std, n, cin, h_in, w_in,
                                 cout, upsample, pad_mode, stream);
}

}  // extern "C"
