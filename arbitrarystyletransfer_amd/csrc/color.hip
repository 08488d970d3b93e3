// RGB <-> XYZ <-> Lab colour conversion for gfx950 (model_util.py:11-140) and the colour-preserving
// (luminance-only) recombination built on it.
//
// NCHW images with C = 3: each thread reads the three planes of a pixel run, converts in registers
// and writes three planes; the composites (RGB2LAB, LAB2RGB, luma_transfer) chain their stages in
// registers with no intermediate store. Algorithmic bytes per pixel: read 3 + write 3 elements
// (24 B fp32, 12 B bf16); backward reads x and g and writes dx (36 B); luma_transfer reads two
// images and writes one. All arithmetic is fp32 whatever the storage type.
//
// Transcendentals: x**2.4, x**(1/2.4) and the cube root run on the hardware v_log_f32 / v_exp_f32
// (exp2(p * log2(x))); the cube root, whose error a and b amplify by 500 and 200, adds one Newton
// step. -DAST_COLOR_LIBM=1 builds the same kernels on powf / cbrtf for the A/B in DESIGN.md §3.
//
// NaN convention (the reference blends `f(x)*mask + g(x)*(1-mask)`, so a NaN of the unselected
// branch survives): rgb -> linear is NaN below -0.055, xyz -> f(.) is NaN for a negative component,
// and an infinite input is NaN in both. lab -> xyz and xyz -> rgb clamp and stay finite.
// Backward: the derivative of the selected branch, zero where a max(., 0) clamp is active; finite
// where the reference's autograd is NaN only because the unselected branch has an infinite slope.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ast_hip.h"

#ifndef AST_COLOR_LIBM
#define AST_COLOR_LIBM 0
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 4096;

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// white point (0.95047, 1, 1.08883) and the reference's matrices (model_util.py:23-25, 43-45)
constexpr float kWx = 0.95047f, kWz = 1.08883f;
constexpr float kT0 = 16.f / 116.f;

__device__ __forceinline__ float qnan() { return __builtin_nanf(""); }

// x**p for x > 0 (the callers select another branch elsewhere)
__device__ __forceinline__ float pow_pos(float x, float p) {
#if AST_COLOR_LIBM
  return powf(x, p);
#else
  return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x));
#endif
}

__device__ __forceinline__ float cbrt_pos(float x) {
#if AST_COLOR_LIBM
  return cbrtf(x);
#else
  const float y = __builtin_amdgcn_exp2f(0.33333334f * __builtin_amdgcn_logf(x));
  // one Newton step on y^3 = x; the residual comes out of one fma, the slope may be approximate
  const float y2 = y * y;
  const float r = __builtin_fmaf(y2, y, -x);
  return y - r * __builtin_amdgcn_rcpf(3.f * y2);
#endif
}

// ---- stages (forward) ---------------------------------------------------------------------------

// sRGB -> linear, one channel (model_util.py:17-21)
__device__ __forceinline__ float rgb_lin(float v) {
  const float b = (v + 0.055f) * (1.f / 1.055f);
  if (v > 0.04045f) return v == INFINITY ? qnan() : pow_pos(b, 2.4f);
  return b < 0.f ? qnan() : v * (1.f / 12.92f);
}

__device__ __forceinline__ void rgb2xyz(float& a, float& b, float& c) {
  const float r = rgb_lin(a), g = rgb_lin(b), bl = rgb_lin(c);
  a = .412453f * r + .357580f * g + .180423f * bl;
  b = .212671f * r + .715160f * g + .072169f * bl;
  c = .019334f * r + .119193f * g + .950227f * bl;
}

// f of xyz2lab on a white-scaled component (model_util.py:73-77)
__device__ __forceinline__ float lab_f(float s) {
  if (s > 0.008856f) return s == INFINITY ? qnan() : cbrt_pos(s);
  return s < 0.f ? qnan() : 7.787f * s + kT0;
}

__device__ __forceinline__ void xyz2lab(float& a, float& b, float& c) {
  const float fx = lab_f(a * (1.f / kWx)), fy = lab_f(b), fz = lab_f(c * (1.f / kWz));
  a = 116.f * fy - 16.f;
  b = 500.f * (fx - fy);
  c = 200.f * (fy - fz);
}

__device__ __forceinline__ float lab_finv(float t) {
  return t > 0.2068966f ? t * t * t : (t - kT0) * (1.f / 7.787f);
}

__device__ __forceinline__ void lab2xyz(float& a, float& b, float& c) {
  const float ty = (a + 16.f) * (1.f / 116.f);
  const float tx = b * (1.f / 500.f) + ty;
  float tz = ty - c * (1.f / 200.f);
  tz = tz < 0.f ? 0.f : tz;
  a = lab_finv(tx) * kWx;
  b = lab_finv(ty);
  c = lab_finv(tz) * kWz;
}

__device__ __forceinline__ float lin_rgb(float v) {
  v = v < 0.f ? 0.f : v;
  return v > 0.0031308f ? 1.055f * pow_pos(v, 1.f / 2.4f) - 0.055f : 12.92f * v;
}

__device__ __forceinline__ void xyz2rgb(float& a, float& b, float& c) {
  const float r = 3.24048134f * a - 1.53715152f * b - 0.49853633f * c;
  const float g = -0.96925495f * a + 1.87599f * b + .04155593f * c;
  const float bl = .05564664f * a - .20404134f * b + 1.05731107f * c;
  a = lin_rgb(r);
  b = lin_rgb(g);
  c = lin_rgb(bl);
}

template <int MODE>
__device__ __forceinline__ void convert(float& a, float& b, float& c) {
  if (MODE == AST_COLOR_RGB2XYZ) rgb2xyz(a, b, c);
  if (MODE == AST_COLOR_XYZ2RGB) xyz2rgb(a, b, c);
  if (MODE == AST_COLOR_XYZ2LAB) xyz2lab(a, b, c);
  if (MODE == AST_COLOR_LAB2XYZ) lab2xyz(a, b, c);
  if (MODE == AST_COLOR_RGB2LAB) {   // model_util.py:117-119
    rgb2xyz(a, b, c);
    xyz2lab(a, b, c);
    a = (a * 0.01f + 1.f) * 0.5f;
    b = (b * 0.01f + 1.f) * 0.5f;
    c = (c * 0.01f + 1.f) * 0.5f;
  }
  if (MODE == AST_COLOR_LAB2RGB) {   // model_util.py:134-135
    a = (a * 2.f - 1.f) * 100.f;
    b = (b * 2.f - 1.f) * 100.f;
    c = (c * 2.f - 1.f) * 100.f;
    lab2xyz(a, b, c);
    xyz2rgb(a, b, c);
  }
}

// ---- stages (vector-Jacobian products): (a, b, c) the stage input, (ga, gb, gc) cotangent in/out

__device__ __forceinline__ float rgb_lin_d(float v) {
  if (v > 0.04045f) return (2.4f / 1.055f) * pow_pos((v + 0.055f) * (1.f / 1.055f), 1.4f);
  return 1.f / 12.92f;
}

__device__ __forceinline__ void rgb2xyz_vjp(float a, float b, float c, float& ga, float& gb, float& gc) {
  const float r = .412453f * ga + .212671f * gb + .019334f * gc;
  const float g = .357580f * ga + .715160f * gb + .119193f * gc;
  const float bl = .180423f * ga + .072169f * gb + .950227f * gc;
  ga = r * rgb_lin_d(a);
  gb = g * rgb_lin_d(b);
  gc = bl * rgb_lin_d(c);
}

__device__ __forceinline__ float lab_f_d(float s) {
  if (s > 0.008856f) {
    const float y = cbrt_pos(s);
    return (1.f / 3.f) / (y * y);
  }
  return 7.787f;
}

__device__ __forceinline__ void xyz2lab_vjp(float a, float b, float c, float& ga, float& gb, float& gc) {
  const float dfx = 500.f * gb;
  const float dfy = 116.f * ga - 500.f * gb + 200.f * gc;
  const float dfz = -200.f * gc;
  ga = dfx * lab_f_d(a * (1.f / kWx)) * (1.f / kWx);
  gb = dfy * lab_f_d(b);
  gc = dfz * lab_f_d(c * (1.f / kWz)) * (1.f / kWz);
}

__device__ __forceinline__ float lab_finv_d(float t) { return t > 0.2068966f ? 3.f * t * t : 1.f / 7.787f; }

__device__ __forceinline__ void lab2xyz_vjp(float a, float b, float c, float& ga, float& gb, float& gc) {
  const float ty = (a + 16.f) * (1.f / 116.f);
  const float tx = b * (1.f / 500.f) + ty;
  const float tz = ty - c * (1.f / 200.f);
  const float dx = ga * kWx * lab_finv_d(tx);
  const float dy = gb * lab_finv_d(ty);
  const float dz = tz < 0.f ? 0.f : gc * kWz * lab_finv_d(tz);
  ga = (dx + dy + dz) * (1.f / 116.f);
  gb = dx * (1.f / 500.f);
  gc = dz * (-1.f / 200.f);
}

__device__ __forceinline__ float lin_rgb_d(float v) {
  if (v < 0.f) return 0.f;
  return v > 0.0031308f ? (1.055f / 2.4f) * pow_pos(v, 1.f / 2.4f - 1.f) : 12.92f;
}

__device__ __forceinline__ void xyz2rgb_vjp(float a, float b, float c, float& ga, float& gb, float& gc) {
  const float r = 3.24048134f * a - 1.53715152f * b - 0.49853633f * c;
  const float g = -0.96925495f * a + 1.87599f * b + .04155593f * c;
  const float bl = .05564664f * a - .20404134f * b + 1.05731107f * c;
  const float dr = ga * lin_rgb_d(r), dg = gb * lin_rgb_d(g), db = gc * lin_rgb_d(bl);
  ga = 3.24048134f * dr - 0.96925495f * dg + .05564664f * db;
  gb = -1.53715152f * dr + 1.87599f * dg - .20404134f * db;
  gc = -0.49853633f * dr + .04155593f * dg + 1.05731107f * db;
}

template <int MODE>
__device__ __forceinline__ void convert_vjp(float a, float b, float c, float& ga, float& gb, float& gc) {
  if (MODE == AST_COLOR_RGB2XYZ) rgb2xyz_vjp(a, b, c, ga, gb, gc);
  if (MODE == AST_COLOR_XYZ2RGB) xyz2rgb_vjp(a, b, c, ga, gb, gc);
  if (MODE == AST_COLOR_XYZ2LAB) xyz2lab_vjp(a, b, c, ga, gb, gc);
  if (MODE == AST_COLOR_LAB2XYZ) lab2xyz_vjp(a, b, c, ga, gb, gc);
  if (MODE == AST_COLOR_RGB2LAB) {
    float x = a, y = b, z = c;
    rgb2xyz(x, y, z);
    ga *= 0.005f;
    gb *= 0.005f;
    gc *= 0.005f;
    xyz2lab_vjp(x, y, z, ga, gb, gc);
    rgb2xyz_vjp(a, b, c, ga, gb, gc);
  }
  if (MODE == AST_COLOR_LAB2RGB) {
    const float l = (a * 2.f - 1.f) * 100.f, m = (b * 2.f - 1.f) * 100.f, n = (c * 2.f - 1.f) * 100.f;
    float x = l, y = m, z = n;
    lab2xyz(x, y, z);
    xyz2rgb_vjp(x, y, z, ga, gb, gc);
    lab2xyz_vjp(l, m, n, ga, gb, gc);
    ga *= 200.f;
    gb *= 200.f;
    gc *= 200.f;
  }
}

// ---- luminance-only recombination ---------------------------------------------------------------

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// lab2rgb(cat(L(rgb2lab(clamp01(s))), ab(rgb2lab(clamp01(c))))): L needs the stylised Y alone, a
// and b the content's f(X), f(Y), f(Z); the Lab normalisation and its inverse cancel.
__device__ __forceinline__ void luma(float s0, float s1, float s2, float& a, float& b, float& c) {
  const float sr = rgb_lin(clamp01(s0)), sg = rgb_lin(clamp01(s1)), sb = rgb_lin(clamp01(s2));
  const float fys = lab_f(.212671f * sr + .715160f * sg + .072169f * sb);
  a = clamp01(a);
  b = clamp01(b);
  c = clamp01(c);
  rgb2xyz(a, b, c);
  const float fx = lab_f(a * (1.f / kWx)), fy = lab_f(b), fz = lab_f(c * (1.f / kWz));
  a = 116.f * fys - 16.f;
  b = 500.f * (fx - fy);
  c = 200.f * (fy - fz);
  lab2xyz(a, b, c);
  xyz2rgb(a, b, c);
}

// ---- plane access: V consecutive elements of one plane ------------------------------------------

template <int V>
__device__ __forceinline__ void load(const float* p, float (&v)[V]) {
  if (V == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int k = 0; k < V; k += 4) {
      const float4 t = *reinterpret_cast<const float4*>(p + k);
      v[k] = t.x, v[k + 1] = t.y, v[k + 2] = t.z, v[k + 3] = t.w;
    }
  }
}

template <int V>
__device__ __forceinline__ void load(const bf16* p, float (&v)[V]) {
  if (V == 1) {
    v[0] = (float)p[0];
  } else {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = (float)t[k];
  }
}

template <int V>
__device__ __forceinline__ void store(float* p, const float (&v)[V]) {
  if (V == 1) {
    p[0] = v[0];
  } else {
#pragma unroll
    for (int k = 0; k < V; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
  }
}

template <int V>
__device__ __forceinline__ void store(bf16* p, const float (&v)[V]) {
  if (V == 1) {
    p[0] = (bf16)v[0];
  } else {
    bf16x8 t;
#pragma unroll
    for (int k = 0; k < V; ++k) t[k] = (bf16)v[k];
    *reinterpret_cast<bf16x8*>(p) = t;
  }
}

// Grid: x over the hw / V pixel runs of an image, y over images (both grid-stride).
template <int MODE, typename TI, typename TO, int V>
__global__ __launch_bounds__(kThreads) void color_kernel(const TI* __restrict__ x, TO* __restrict__ out, int64_t hw,
                                                         int n) {
  const int64_t runs = hw / V;
  for (int img = blockIdx.y; img < n; img += gridDim.y) {
    const TI* p = x + (int64_t)img * 3 * hw;
    TO* o = out + (int64_t)img * 3 * hw;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < runs; i += (int64_t)gridDim.x * kThreads) {
      float a[V], b[V], c[V];
      load<V>(p + i * V, a);
      load<V>(p + hw + i * V, b);
      load<V>(p + 2 * hw + i * V, c);
#pragma unroll
      for (int k = 0; k < V; ++k) convert<MODE>(a[k], b[k], c[k]);
      store<V>(o + i * V, a);
      store<V>(o + hw + i * V, b);
      store<V>(o + 2 * hw + i * V, c);
    }
  }
}

template <int MODE, int V>
__global__ __launch_bounds__(kThreads) void color_backward_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ g,
                                                                  float* __restrict__ dx, int64_t hw, int n) {
  const int64_t runs = hw / V;
  for (int img = blockIdx.y; img < n; img += gridDim.y) {
    const int64_t base = (int64_t)img * 3 * hw;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < runs; i += (int64_t)gridDim.x * kThreads) {
      float a[V], b[V], c[V], ga[V], gb[V], gc[V];
      load<V>(x + base + i * V, a);
      load<V>(x + base + hw + i * V, b);
      load<V>(x + base + 2 * hw + i * V, c);
      load<V>(g + base + i * V, ga);
      load<V>(g + base + hw + i * V, gb);
      load<V>(g + base + 2 * hw + i * V, gc);
#pragma unroll
      for (int k = 0; k < V; ++k) convert_vjp<MODE>(a[k], b[k], c[k], ga[k], gb[k], gc[k]);
      store<V>(dx + base + i * V, ga);
      store<V>(dx + base + hw + i * V, gb);
      store<V>(dx + base + 2 * hw + i * V, gc);
    }
  }
}

template <typename T, int V>
__global__ __launch_bounds__(kThreads) void luma_transfer_kernel(const T* __restrict__ stylised,
                                                                 const T* __restrict__ content, T* __restrict__ out,
                                                                 int64_t hw, int n) {
  const int64_t runs = hw / V;
  for (int img = blockIdx.y; img < n; img += gridDim.y) {
    const int64_t base = (int64_t)img * 3 * hw;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < runs; i += (int64_t)gridDim.x * kThreads) {
      float a[V], b[V], c[V], s0[V], s1[V], s2[V];
      load<V>(stylised + base + i * V, s0);
      load<V>(stylised + base + hw + i * V, s1);
      load<V>(stylised + base + 2 * hw + i * V, s2);
      load<V>(content + base + i * V, a);
      load<V>(content + base + hw + i * V, b);
      load<V>(content + base + 2 * hw + i * V, c);
#pragma unroll
      for (int k = 0; k < V; ++k) luma(s0[k], s1[k], s2[k], a[k], b[k], c[k]);
      store<V>(out + base + i * V, a);
      store<V>(out + base + hw + i * V, b);
      store<V>(out + base + 2 * hw + i * V, c);
    }
  }
}

// V elements per thread when every plane of every tensor starts 16-byte aligned: hw a multiple of V
// (the planes of an odd-hw image are unaligned even when the base pointer is) and aligned bases.
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline dim3 grid_for(int64_t hw, int v, int n) {
  const int64_t bx = (hw / v + kThreads - 1) / kThreads;
  return dim3((unsigned)(bx < kMaxBlocksX ? bx : kMaxBlocksX), (unsigned)(n < 65535 ? n : 65535));
}

template <int MODE, typename TI, typename TO>
int launch_convert(const TI* x, TO* out, int n, int64_t hw, hipStream_t st) {
  constexpr int V = 16 / sizeof(TI);
  if (hw % V == 0 && aligned16(x) && aligned16(out))
    hipLaunchKernelGGL((color_kernel<MODE, TI, TO, V>), grid_for(hw, V, n), dim3(kThreads), 0, st, x, out, hw, n);
  else
    hipLaunchKernelGGL((color_kernel<MODE, TI, TO, 1>), grid_for(hw, 1, n), dim3(kThreads), 0, st, x, out, hw, n);
  return (int)hipGetLastError();
}

template <typename TI, typename TO>
int convert_any(const void* x, void* out, int n, long long hw, int mode, void* stream) {
  if (!x || !out) return AST_E_NULLPTR;
  if (n <= 0 || hw <= 0) return AST_E_SHAPE;
  const TI* xi = static_cast<const TI*>(x);
  TO* o = static_cast<TO*>(out);
  hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case AST_COLOR_RGB2XYZ: return launch_convert<AST_COLOR_RGB2XYZ>(xi, o, n, (int64_t)hw, st);
    case AST_COLOR_XYZ2RGB: return launch_convert<AST_COLOR_XYZ2RGB>(xi, o, n, (int64_t)hw, st);
    case AST_COLOR_XYZ2LAB: return launch_convert<AST_COLOR_XYZ2LAB>(xi, o, n, (int64_t)hw, st);
    case AST_COLOR_LAB2XYZ: return launch_convert<AST_COLOR_LAB2XYZ>(xi, o, n, (int64_t)hw, st);
    case AST_COLOR_RGB2LAB: return launch_convert<AST_COLOR_RGB2LAB>(xi, o, n, (int64_t)hw, st);
    case AST_COLOR_LAB2RGB: return launch_convert<AST_COLOR_LAB2RGB>(xi, o, n, (int64_t)hw, st);
    default: return AST_E_SHAPE;
  }
}

template <int MODE>
int launch_backward(const float* x, const float* g, float* dx, int n, int64_t hw, hipStream_t st) {
  if (hw % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(dx))
    hipLaunchKernelGGL((color_backward_kernel<MODE, 4>), grid_for(hw, 4, n), dim3(kThreads), 0, st, x, g, dx, hw, n);
  else
    hipLaunchKernelGGL((color_backward_kernel<MODE, 1>), grid_for(hw, 1, n), dim3(kThreads), 0, st, x, g, dx, hw, n);
  return (int)hipGetLastError();
}

template <typename T>
int luma_any(const void* stylised, const void* content, void* out, int n, long long hw, void* stream) {
  if (!stylised || !content || !out) return AST_E_NULLPTR;
  if (n <= 0 || hw <= 0) return AST_E_SHAPE;
  constexpr int V = 16 / sizeof(T);
  const T* s = static_cast<const T*>(stylised);
  const T* c = static_cast<const T*>(content);
  T* o = static_cast<T*>(out);
  hipStream_t st = (hipStream_t)stream;
  if (hw % V == 0 && aligned16(s) && aligned16(c) && aligned16(o))
    hipLaunchKernelGGL((luma_transfer_kernel<T, V>), grid_for(hw, V, n), dim3(kThreads), 0, st, s, c, o, (int64_t)hw,
                       n);
  else
    hipLaunchKernelGGL((luma_transfer_kernel<T, 1>), grid_for(hw, 1, n), dim3(kThreads), 0, st, s, c, o, (int64_t)hw,
                       n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int ast_color_convert_f32(const float* x, float* out, int n, long long hw, int mode, void* stream) {
  return convert_any<float, float>(x, out, n, hw, mode, stream);
}

int ast_color_convert_bf16_f32(const void* x, float* out, int n, long long hw, int mode, void* stream) {
  return convert_any<bf16, float>(x, out, n, hw, mode, stream);
}

int ast_color_convert_bf16(const void* x, void* out, int n, long long hw, int mode, void* stream) {
  return convert_any<bf16, bf16>(x, out, n, hw, mode, stream);
}

int ast_color_convert_backward_f32(const float* x, const float* grad_out, float* grad_in, int n, long long hw,
                                   int mode, void* stream) {
  if (!x || !grad_out || !grad_in) return AST_E_NULLPTR;
  if (n <= 0 || hw <= 0) return AST_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case AST_COLOR_RGB2XYZ: return launch_backward<AST_COLOR_RGB2XYZ>(x, grad_out, grad_in, n, (int64_t)hw, st);
    case AST_COLOR_XYZ2RGB: return launch_backward<AST_COLOR_XYZ2RGB>(x, grad_out, grad_in, n, (int64_t)hw, st);
    case AST_COLOR_XYZ2LAB: return launch_backward<AST_COLOR_XYZ2LAB>(x, grad_out, grad_in, n, (int64_t)hw, st);
    case AST_COLOR_LAB2XYZ: return launch_backward<AST_COLOR_LAB2XYZ>(x, grad_out, grad_in, n, (int64_t)hw, st);
    case AST_COLOR_RGB2LAB: return launch_backward<AST_COLOR_RGB2LAB>(x, grad_out, grad_in, n, (int64_t)hw, st);
    case AST_COLOR_LAB2RGB: return launch_backward<AST_COLOR_LAB2RGB>(x, grad_out, grad_in, n, (int64_t)hw, st);
    default: return AST_E_SHAPE;
  }
}

int ast_luma_transfer_f32(const float* stylised, const float* content, float* out, int n, long long hw,
                          void* stream) {
  return luma_any<float>(stylised, content, out, n, hw, stream);
}

int ast_luma_transfer_bf16(const void* stylised, const void* content, void* out, int n, long long hw, void* stream) {
  return luma_any<bf16>(stylised, content, out, n, hw, stream);
}

}  // extern "C"
