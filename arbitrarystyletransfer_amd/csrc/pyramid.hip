// Bilinear resize (torch.nn.functional.interpolate(mode="bilinear", align_corners=False,
// antialias=False)), its adjoint, and with them the Laplacian pyramid of STROTSS (Kolkin et al.,
// CVPR 2019) for gfx950. Not augment.hip's resize: that one is the antialiased (area-weighted)
// filter of the data pipeline; the two share nothing but the word.
//
// Planes [planes][h][w] fp32 -> [planes][H][W], any sizes from 1 to 4096 per side, any ratio: up,
// down and an arbitrary rescale are one code path. Coordinates as PyTorch computes them:
//   scale = (float)in / out;  s = max(scale * (o + 0.5) - 0.5, 0);  i0 = min((int)s, in - 1);
//   i1 = i0 + (i0 < in - 1);  l1 = s - i0;  l0 = 1 - l1
//   out = l0y * (l0x * x[i0y][i0x] + l1x * x[i0y][i1x]) + l1y * (l0x * x[i1y][i0x] + l1x * x[i1y][i1x])
// The product scale * (o + 0.5) - 0.5 is one fma in both kernels, so the adjoint is the transpose
// of the forward in bits of the weights.
//
// Forward: one thread per output pixel, four gathers, one store; with `add` the store is
// add + add_sign * resize(x), which is lap_l = cur - up(down(cur)) of the pyramid build and
// cur = lap_l + up(cur) of its collapse in one launch each.
//
// Adjoint: one thread per *source* pixel. The outputs whose footprint touches source row sy are
// those with i0(o) in {sy - 1, sy}; i0 is monotone in o, so they are one contiguous range per
// axis: long when up-sampling, at most two when down-sampling. Its ends come from inverting the
// coordinate map, (sy - 0.5) / scale - 0.5 <= o < (sy + 1.5) / scale - 0.5, widened by one on each
// side against the rounding of that inverse; inside the range the *forward* map decides whether an
// output touches the pixel and with what weight, so a widened end contributes nothing and a
// touching output is never missed. Sums run in ascending (oy, ox) order in one thread: no atomics,
// bitwise reproducible. A source pixel that feeds very many outputs (1 -> 4096 per side) is one
// long serial loop; the pyramid's ratios are 2.
//
// Algorithmic bytes: forward reads h*w (+ H*W with add) and writes H*W floats per plane; the
// adjoint reads H*W and writes h*w (+ reads h*w with accumulate). No LDS, no workspace, no host
// synchronisation: capture-safe.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ast_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 2048;
constexpr int kMaxSide = 4096;

// source cell and upper weight of output index o (PyTorch's area_pixel_compute_source_index)
__device__ __forceinline__ void src_map(int o, float scale, int in, int& i0, int& i1, float& l1) {
  float s = __builtin_fmaf(scale, (float)o + 0.5f, -0.5f);
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// Grid: x over the H*W output pixels of a plane, y over planes (both grid-stride).
template <bool ADD>
__global__ __launch_bounds__(kThreads) void resize_bilinear_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ add,
                                                                   float* __restrict__ out, int planes, int h, int w,
                                                                   int H, int W, float sy, float sx, float add_sign) {
  const int npix = H * W;
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const float* xp = x + (int64_t)p * h * w;
    const int64_t obase = (int64_t)p * npix;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < npix; i += gridDim.x * kThreads) {
      const int oy = i / W, ox = i - oy * W;
      int y0, y1, x0, x1;
      float ly, lx;
      src_map(oy, sy, h, y0, y1, ly);
      src_map(ox, sx, w, x0, x1, lx);
      const float a = xp[y0 * w + x0], b = xp[y0 * w + x1], c = xp[y1 * w + x0], d = xp[y1 * w + x1];
      const float mx = 1.f - lx, my = 1.f - ly;
      const float v = my * (mx * a + lx * b) + ly * (mx * c + lx * d);
      out[obase + i] = ADD ? add[obase + i] + add_sign * v : v;
    }
  }
}

// [lo, hi]: a superset, within [0, out - 1], of the outputs with a non-zero weight on source index s
// (an output clamped to s = 0 has l1 = 0: it names pixel 1 as i1 but does not touch it)
__device__ __forceinline__ void touch_range(int s, float inv, int out, int& lo, int& hi) {
  lo = (int)floorf(((float)s - 0.5f) * inv - 0.5f) - 1;
  hi = (int)ceilf(((float)s + 1.5f) * inv - 0.5f) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}

// weight of source index s in output o along one axis; false when it is zero (o does not touch s)
__device__ __forceinline__ bool touch_weight(int o, float scale, int in, int s, float& wgt) {
  int i0, i1;
  float l1;
  src_map(o, scale, in, i0, i1, l1);
  wgt = (i0 == s ? 1.f - l1 : 0.f) + (i1 == s ? l1 : 0.f);
  return i0 == s || (i1 == s && l1 > 0.f);
}

// Grid: x over the h*w source pixels of a plane, y over planes (both grid-stride).
template <bool ACC>
__global__ __launch_bounds__(kThreads) void resize_bilinear_adjoint_kernel(const float* __restrict__ g,
                                                                           float* __restrict__ dx, int planes, int h,
                                                                           int w, int H, int W, float sy, float sx,
                                                                           float iy, float ix) {
  const int npix = h * w;
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const float* gp = g + (int64_t)p * H * W;
    const int64_t base = (int64_t)p * npix;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < npix; i += gridDim.x * kThreads) {
      const int py = i / w, px = i - py * w;
      int ylo, yhi, xlo, xhi;
      touch_range(py, iy, H, ylo, yhi);
      touch_range(px, ix, W, xlo, xhi);
      float acc = 0.f;
      for (int oy = ylo; oy <= yhi; ++oy) {
        float wy;
        if (!touch_weight(oy, sy, h, py, wy)) continue;
        const float* row = gp + oy * W;
        for (int ox = xlo; ox <= xhi; ++ox) {
          float wx;
          if (!touch_weight(ox, sx, w, px, wx)) continue;
          acc += (wy * wx) * row[ox];
        }
      }
      dx[base + i] = ACC ? dx[base + i] + acc : acc;
    }
  }
}

inline dim3 grid_for(int npix, int planes) {
  const int bx = (npix + kThreads - 1) / kThreads;
  return dim3((unsigned)(bx < kMaxBlocksX ? bx : kMaxBlocksX), (unsigned)(planes < 65535 ? planes : 65535));
}

inline bool bad_side(int v) { return v < 1 || v > kMaxSide; }

}  // namespace

extern "C" {

int ast_resize_bilinear_f32(const float* x, float* out, int planes, int h, int w, int H, int W, const float* add,
                            float add_sign, void* stream) {
  if (!x || !out) return AST_E_NULLPTR;
  if (planes <= 0 || bad_side(h) || bad_side(w) || bad_side(H) || bad_side(W)) return AST_E_SHAPE;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  hipStream_t st = (hipStream_t)stream;
  if (add)
    hipLaunchKernelGGL((resize_bilinear_kernel<true>), grid_for(H * W, planes), dim3(kThreads), 0, st, x, add, out,
                       planes, h, w, H, W, sy, sx, add_sign);
  else
    hipLaunchKernelGGL((resize_bilinear_kernel<false>), grid_for(H * W, planes), dim3(kThreads), 0, st, x, add, out,
                       planes, h, w, H, W, sy, sx, add_sign);
  return (int)hipGetLastError();
}

int ast_resize_bilinear_adjoint_f32(const float* g, float* dx, int planes, int h, int w, int H, int W,
                                    int accumulate, void* stream) {
  if (!g || !dx) return AST_E_NULLPTR;
  if (planes <= 0 || bad_side(h) || bad_side(w) || bad_side(H) || bad_side(W)) return AST_E_SHAPE;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const float iy = (float)H / (float)h, ix = (float)W / (float)w;
  hipStream_t st = (hipStream_t)stream;
  if (accumulate)
    hipLaunchKernelGGL((resize_bilinear_adjoint_kernel<true>), grid_for(h * w, planes), dim3(kThreads), 0, st, g, dx,
                       planes, h, w, H, W, sy, sx, iy, ix);
  else
    hipLaunchKernelGGL((resize_bilinear_adjoint_kernel<false>), grid_for(h * w, planes), dim3(kThreads), 0, st, g,
                       dx, planes, h, w, H, W, sy, sx, iy, ix);
  return (int)hipGetLastError();
}

}  // extern "C"
