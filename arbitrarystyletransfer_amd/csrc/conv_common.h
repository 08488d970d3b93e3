// What more than one 3x3-conv kernel family uses: the kernel arguments, the padding / ReLU / block
// decode helpers, the epilogues shared between families, the launch helpers, and the launcher entry
// points through which the configuration table of conv3x3_igemm.hip reaches the other families:
//   conv3x3_igemm.hip  fp32-MFMA implicit GEMM, fp32 weight pack, configuration table, C ABI
//   conv_x3.hip        split-bf16 ("x3") kernel, its persistent form     (conv_x3.h: tile sizes,
//                      x3p, and the split weight pack                     staged row stores, stamps)
//   conv_up2c.hip      collapsed upsampled kernel, its pack and C ABI
//   conv_direct.hip    direct VALU kernels for Cout <= 4 and Cin <= 4
//   conv_cin3.hip      split-bf16 conv of a 1..3-channel input (cin3.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ast_hip.h"

namespace ast_conv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TW = 32;  // output tile width = one MFMA M-tile

struct ConvArgs {
  const float* x;
  const float* x2;  // optional second input batch: images [nsplit, N) read from x2 (content|style pair)
  int nsplit;
  const float* wp;  // packed [cin_pad][9][cout_pad]
  const float* bias;
  float* y_pre;
  float* y_act;
  float* y_pool;
  const float* in_mean;
  const float* in_std;
  int N, Cin, Hin, Win, Cout, H, W;
  int cin_pad, cout_pad;
  int reflect;  // 0: zero pad, 1: reflect pad (of the upsampled grid)
  int tiles_x, tiles_y;
  // input-gradient epilogue (x3 kernels only; ast_conv3x3_dgrad_f32): with v the conv output at an
  // output position (of y_pre, or of y_pool when e_sum2), v = v + e_add_pre; then
  // v = e_mask > 0 ? e_add_post + v : e_add_post (the ReLU backward of the layer below, with its
  // pre-ReLU tap gradient; a missing add_post reads as 0, a missing mask as > 0)
  const float* e_mask;
  const float* e_add_pre;
  const float* e_add_post;
  int e_sum2;  // y_pool holds the 2x2 SUM of the output (nearest-upsample adjoint), no ReLU / max
};

__device__ __forceinline__ bool dgrad_epi(const ConvArgs& a) { return a.e_mask || a.e_add_pre || a.e_add_post; }

// the input-gradient epilogue of one output value at flat offset off (see ConvArgs)
__device__ __forceinline__ float dgrad_epi_one(const ConvArgs& a, float v, int64_t off) {
  if (a.e_add_pre) v = v + a.e_add_pre[off];
  const bool keep = !a.e_mask || a.e_mask[off] > 0.f;
  if (a.e_add_post) return keep ? a.e_add_post[off] + v : a.e_add_post[off];
  return keep ? v : 0.f;
}

__device__ __forceinline__ float4 dgrad_epi4(const ConvArgs& a, float4 v, int64_t off) {
  if (a.e_add_pre) {
    const float4 u = *reinterpret_cast<const float4*>(a.e_add_pre + off);
    v = make_float4(v.x + u.x, v.y + u.y, v.z + u.z, v.w + u.w);
  }
  float4 m = make_float4(1.f, 1.f, 1.f, 1.f), p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.e_mask) m = *reinterpret_cast<const float4*>(a.e_mask + off);
  if (a.e_add_post) {
    p = *reinterpret_cast<const float4*>(a.e_add_post + off);
    return make_float4(m.x > 0.f ? p.x + v.x : p.x, m.y > 0.f ? p.y + v.y : p.y, m.z > 0.f ? p.z + v.z : p.z,
                       m.w > 0.f ? p.w + v.w : p.w);
  }
  return make_float4(m.x > 0.f ? v.x : 0.f, m.y > 0.f ? v.y : 0.f, m.z > 0.f ? v.z : 0.f, m.w > 0.f ? v.w : 0.f);
}

constexpr int kCinAlign = 8;    // packed cin padding (>= every CK)
constexpr int kCoutAlign = 64;  // packed cout padding

// Source-grid index of padded coordinate g (may be -1 or n) for the pad mode; -1 = zero.
//  reflect, no upsample: ReflectionPad2d(1)        -> reflect
//  reflect, upsample x2: reflect on 2n grid        -> replicate on the n grid
//  zeros:                                          -> -1 outside
template <int UP>
__device__ __forceinline__ int src_index(int g, int n, int reflect) {
  if (g >= 0 && g < n) return g;
  if (!reflect) return -1;
  if (UP == 2) return g < 0 ? 0 : n - 1;
  int r = g < 0 ? -g : 2 * (n - 1) - g;
  return r < 0 ? 0 : (r >= n ? n - 1 : r);
}

// torch semantics: relu(NaN) = NaN, max_pool propagates NaN.
__device__ __forceinline__ float relu_f(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

// Workgroup -> (spatial tile, output-channel group). The G channel groups of one spatial tile
// read the same input tile, so they get ids b, b+8, ..., b+8(G-1): dispatched together, and onto
// one XCD under the observed round-robin placement (speed only, never correctness).
__device__ __forceinline__ bool decode_block(int id, int ntiles, int groups, int& tile, int& group) {
  const int xcd = id & 7, rest = id >> 3;
  group = rest % groups;
  tile = (rest / groups) * 8 + xcd;
  return tile < ntiles;
}

// Epilogue of a wave's RM x RN tiles of 32x32 accumulators (A = pixels, B = channels: lane l32 =
// output channel n0c + 32j + l32, register 4g + r = pixel x0 + 8g + 4h + r of row y0 + row0 + i):
// +bias, pre-ReLU / ReLU float4 stores, fused 2x2 max-pool (a lane holds both rows of a window).
template <int RM, int RN>
__device__ __forceinline__ void store_tiles(const ConvArgs& a, const f32x16 (&acc)[RM][RN], int n, int x0, int y0,
                                            int row0, int n0c, int h, int l32) {
  const int H = a.H, W = a.W;
  const int64_t plane = (int64_t)H * W;
  const bool vec4 = (W & 3) == 0;
  const int Ho = H >> 1, Wo = W >> 1;
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int co = n0c + j * 32 + l32;
    const bool cok = co < a.Cout;
    const float bv = (cok && a.bias) ? a.bias[co] : 0.f;
    const int64_t obase = ((int64_t)n * a.Cout + co) * plane;
    if (a.y_pre || a.y_act) {
#pragma unroll
      for (int i = 0; i < RM; ++i) {
        const int yy = y0 + row0 + i;
        if (!cok || yy >= H) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int xx = x0 + 8 * g + 4 * h;
          if (xx >= W) continue;
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[i][j][4 * g + r] + bv;
          const int64_t off = obase + (int64_t)yy * W + xx;
          const bool full = vec4 && xx + 3 < W;
          if (a.y_pre) {
            if (full) *reinterpret_cast<float4*>(a.y_pre + off) = make_float4(v[0], v[1], v[2], v[3]);
            else for (int r = 0; r < 4; ++r) if (xx + r < W) a.y_pre[off + r] = v[r];
          }
          if (a.y_act) {
            float u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) u[r] = relu_f(v[r]);
            if (full) *reinterpret_cast<float4*>(a.y_act + off) = make_float4(u[0], u[1], u[2], u[3]);
            else for (int r = 0; r < 4; ++r) if (xx + r < W) a.y_act[off + r] = u[r];
          }
        }
      }
    }
    if (a.y_pool && cok) {
      const int64_t pbase = ((int64_t)n * a.Cout + co) * Ho * Wo;
#pragma unroll
      for (int i = 0; i + 1 < RM; i += 2) {
        const int py = (y0 + row0 + i) >> 1;
        if (py >= Ho) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int px = (x0 + 8 * g + 4 * h) >> 1;
          if (px >= Wo) continue;
          float m[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            m[r] = max_nan(relu_f(acc[i][j][4 * g + r] + bv), relu_f(acc[i + 1][j][4 * g + r] + bv));
          const float p0 = max_nan(m[0], m[1]), p1 = max_nan(m[2], m[3]);
          const int64_t off = pbase + (int64_t)py * Wo + px;
          if (px + 1 < Wo && (Wo & 1) == 0) {
            *reinterpret_cast<float2*>(a.y_pool + off) = make_float2(p0, p1);
          } else {
            a.y_pool[off] = p0;
            if (px + 1 < Wo) a.y_pool[off + 1] = p1;
          }
        }
      }
    }
  }
}

constexpr int kX3K = 16;  // split-bf16 kernels: input channels per chunk (= the MFMA K)
// build knob, here because both the x3 kernel (conv_x3.hip) and ast_conv3x3_dgrad_f32 read it
#ifndef X3_STAGED_EPI
#define X3_STAGED_EPI 1  // epilogue through LDS (store_tiles_staged); 0 = direct stores (A/B)
#endif

__host__ __device__ constexpr int64_t x3_split_offset(int cin, int cout) {  // floats before the split part
  return (int64_t)((cin + 7) / 8 * 8) * 9 * ((cout + 63) / 64 * 64);
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return cdiv(a, b) * b; }

inline int cu_count() {  // CUs of the current device (looked up on a device's first call)
  static int cus_of[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  int cus = dev >= 0 && dev < 64 ? cus_of[dev] : 0;
  if (!cus) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (dev >= 0 && dev < 64) cus_of[dev] = cus;
  }
  return cus;
}

// workgroups of TW x th pixels x bn channels: the spatial tiles rounded up to 8 (decode_block) x channel groups
inline int64_t conv_blocks(const ConvArgs& a, int th, int bn) {
  const int64_t ntiles = (int64_t)cdiv(a.W, TW) * cdiv(a.H, th) * a.N;
  return (ntiles + 7) / 8 * 8 * cdiv(a.Cout, bn);
}

// launch preamble of the tiled kernels: sets a.tiles_x / a.tiles_y and nblk; 0 or the error code
inline int conv_grid(ConvArgs& a, int th, int bn, int64_t& nblk) {
  a.tiles_x = cdiv(a.W, TW);
  a.tiles_y = cdiv(a.H, th);
  if (cdiv(a.Cout, bn) * bn > a.cout_pad) return AST_E_UNSUPPORTED;  // weight-slab reads stay in bounds
  nblk = conv_blocks(a, th, bn);
  return nblk >= 0x7fffffff ? AST_E_SHAPE : 0;
}

// kern with its dynamic-LDS limit raised to bytes; kept in a function-local static, so set once per kernel
inline const void* with_dynamic_lds(const void* kern, int bytes) {
  (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return kern;
}

// Launcher entry points of the families (the fn of a CfgEntry), defined in the family's file and
// explicitly instantiated there (CONV_INSTANTIATE) for exactly the forms the configuration table names.
template <int WM, int RM, int RN, int OCC = 1, bool M16 = false, bool PER = false>
int launch_x3(const ConvArgs& a, hipStream_t s, int up);  // conv_x3.hip
template <int WM, int RM, int RN, int OCC = 1> int launch_x3p(const ConvArgs& a, hipStream_t s, int up);
template <int COUT> int launch_smallc(const ConvArgs& a, hipStream_t s, int up);  // conv_direct.hip
template <int COUT> int launch_smallc2(const ConvArgs& a, hipStream_t s, int up);
template <int TH, bool NTS, int OCC = 1> int launch_cin4(const ConvArgs& a, hipStream_t s, int up);
#define CONV_INSTANTIATE(...) template int __VA_ARGS__(const ConvArgs&, hipStream_t, int);

}  // namespace ast_conv
