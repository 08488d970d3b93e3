// Direct (VALU) 3x3 convs for gfx950: the shapes whose GEMM view would leave the MFMA tiles idle --
// Cout <= 4 (the decoder's last conv; configurations 10, 11 and the register-streaming 36, 37) and
// Cin <= 4 (VGG conv_1; configurations 18-23). Reached from the table of conv3x3_igemm.hip.
#include "conv_common.h"

namespace {

using namespace ast_conv;

// Direct (VALU) 3x3 conv for cout <= 4 — the decoder's final 64->3 conv (models.py:627). As a
// GEMM its N = 3 would leave >90% of every MFMA tile idle; as a direct conv each thread makes
// 4 adjacent output pixels x COUT channels, weights are wave-uniform scalar loads, and the kernel
// is bound by reading its input once from HBM. Same source-tile staging as the MFMA kernel.
template <int COUT, int UP>
__global__ __launch_bounds__(256, 3) void conv3x3_smallc_kernel(ConvArgs a) {
  constexpr int NT = 256, TH = 8, TWS = 128, CK = 4;
  constexpr int SW = TWS / UP, SR = TH / UP + 2, RS = SW + 8, C0 = 4, QV = SW / 4;
  constexpr int A_ITEMS = CK * SR * (QV + 2);
  __shared__ __attribute__((aligned(16))) float As[CK * SR * RS];

  const int tid = threadIdx.x;
  const int tx = tid & 31, ty = tid >> 5;
  int t = blockIdx.x;
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int x0 = bx * TWS, y0 = by * TH;
  const int sx0 = x0 / UP, sy0 = y0 / UP - 1;
  const int Hin = a.Hin, Win = a.Win;
  const bool fast = (sx0 + SW <= Win) && ((Win & 3) == 0);
  const float* __restrict__ xin =
      n < a.nsplit ? a.x + (int64_t)n * a.Cin * Hin * Win : a.x2 + (int64_t)(n - a.nsplit) * a.Cin * Hin * Win;
  const float* __restrict__ wp = a.wp;
  const int plane_in = Hin * Win;

  float acc[COUT][4];
#pragma unroll
  for (int co = 0; co < COUT; ++co)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[co][j] = 0.f;

  __shared__ __attribute__((aligned(16))) float Ws[CK * 9 * 4];  // [c][tap][co(4)] of this chunk
  constexpr int A_PER_T = (A_ITEMS + NT - 1) / NT;
  for (int cin0 = 0; cin0 < a.Cin; cin0 += CK) {
    float4 ra[A_PER_T];
    if (fast) {  // issue every global load of the chunk before the barrier, store after it
#pragma unroll
      for (int i = 0; i < A_PER_T; ++i) {
        const int e = tid + i * NT;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < A_ITEMS) {
          const int q = e % (QV + 2);
          const int cr = e / (QV + 2);
          const int r = cr % SR, c = cr / SR;
          const int cin = cin0 + c;
          const int sy = src_index<UP>(sy0 + r, Hin, a.reflect);
          if (cin < a.Cin && sy >= 0) {
            const float* row = xin + cin * plane_in + sy * Win;
            if (q < QV) {
              v = *reinterpret_cast<const float4*>(row + sx0 + 4 * q);
            } else {
              const int sx = src_index<UP>(q == QV ? sx0 - 1 : sx0 + SW, Win, a.reflect);
              if (sx >= 0) v.x = row[sx];
            }
          }
        }
        ra[i] = v;
      }
    }
    float wv = 0.f;
    if (tid < CK * 9 * 4) {
      const int c = tid / 36, rem = tid % 36, tap = rem / 4, co = rem % 4;
      if (cin0 + c < a.Cin && co < COUT) wv = wp[((cin0 + c) * 9 + tap) * a.cout_pad + co];
    }
    __syncthreads();  // previous chunk's reads are done
    if (tid < CK * 9 * 4) Ws[tid] = wv;
    if (fast) {
#pragma unroll
      for (int i = 0; i < A_PER_T; ++i) {
        const int e = tid + i * NT;
        if (e < A_ITEMS) {
          const int q = e % (QV + 2);
          float* row = As + (e / (QV + 2)) * RS;
          if (q < QV) *reinterpret_cast<float4*>(row + C0 + 4 * q) = ra[i];
          else row[q == QV ? C0 - 1 : C0 + SW] = ra[i].x;
        }
      }
    } else {
      for (int e = tid; e < CK * SR * (SW + 2); e += NT) {
        const int col = e % (SW + 2);
        const int cr = e / (SW + 2);
        const int r = cr % SR, c = cr / SR;
        const int cin = cin0 + c;
        const int sy = src_index<UP>(sy0 + r, Hin, a.reflect);
        const int sx = src_index<UP>(sx0 - 1 + col, Win, a.reflect);
        As[cr * RS + C0 - 1 + col] = (cin < a.Cin && sy >= 0 && sx >= 0) ? xin[cin * plane_in + sy * Win + sx] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < CK; ++c) {  // channels past Cin hold zero inputs and zero weights
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int orow = ty + ky - 1;
        const int srow = (UP == 1) ? orow + 1 : (orow >> 1) + 1;
        const float* rowp = As + (c * SR + srow) * RS + C0;
        constexpr int NV = UP == 1 ? 6 : 4;
        float v[NV];
        if constexpr (UP == 1) {
          // columns 4tx-1 .. 4tx+4: one aligned 16-byte read (consecutive lanes, conflict-free) and
          // the two neighbours from the adjacent lanes (lane shuffles); the scalar reads at a
          // 4-word lane stride were 4-way bank conflicts. Each half-wave is one output row, so its
          // first and last lanes read their outer neighbour themselves.
          const float4 mid = *reinterpret_cast<const float4*>(rowp + 4 * tx);
          // (lane shuffles; the DPP wave_shr / wave_shl forms these replaced are GFX8/9-era controls)
          float left = __shfl_up(mid.w, 1, 64);
          float right = __shfl_down(mid.x, 1, 64);
          if (tx == 0) left = rowp[-1];
          if (tx == 31) right = rowp[128];
          v[0] = left;
          v[1] = mid.x;
          v[2] = mid.y;
          v[3] = mid.z;
          v[4] = mid.w;
          v[5] = right;
        } else {
#pragma unroll
          for (int m = 0; m < NV; ++m) v[m] = rowp[2 * tx - 1 + m];
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float4 w4 = *reinterpret_cast<const float4*>(Ws + (c * 9 + ky * 3 + kx) * 4);  // LDS broadcast
          const float wco[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int co = 0; co < COUT; ++co) {
            const float w = wco[co];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int m = UP == 1 ? j + kx : ((j + kx - 1) >> 1) + 1;
              acc[co][j] = fmaf(v[m], w, acc[co][j]);
            }
          }
        }
      }
    }
  }

  const int H = a.H, W = a.W;
  const int yy = y0 + ty, xx = x0 + 4 * tx;
  if (yy >= H || xx >= W) return;
  const bool full = ((W & 3) == 0) && xx + 3 < W;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    if (co >= a.Cout) break;
    const float bv = a.bias ? a.bias[co] : 0.f;
    float v[4], u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = acc[co][j] + bv;
      u[j] = relu_f(v[j]);
    }
    const int64_t off = (((int64_t)n * a.Cout + co) * H + yy) * W + xx;
    if (a.y_pre) {
      if (full) *reinterpret_cast<float4*>(a.y_pre + off) = make_float4(v[0], v[1], v[2], v[3]);
      else for (int j = 0; j < 4; ++j) if (xx + j < W) a.y_pre[off + j] = v[j];
    }
    if (a.y_act) {
      if (full) *reinterpret_cast<float4*>(a.y_act + off) = make_float4(u[0], u[1], u[2], u[3]);
      else for (int j = 0; j < 4; ++j) if (xx + j < W) a.y_act[off + j] = u[j];
    }
  }
}

// Direct (VALU) 3x3 conv for cout <= 4, register-streaming form (round 5; configs 36, 37): no LDS
// tile and no barrier per input channel. A wave owns 2 output rows x 256 columns (4 per lane); per
// input channel each lane loads its 4 source rows as one 16-byte piece each, takes the columns left
// and right of its piece from the neighbouring lanes (the wave's edge lanes and the image borders
// load theirs), and accumulates 2 rows x 4 pixels x COUT outputs over the 9 taps (weights: one LDS
// broadcast float4 per tap). The next two channels' rows are in flight during the current channel's
// FMAs. Same tap-major, channel-minor FMA order per output as conv3x3_smallc_kernel: bit-identical.
// The smallc form stages 4-channel chunks in LDS behind two barriers each and ran at ~2 TB/s of its
// input (latency-bound, 8x64x512^2 -> 3: 0.27 ms); this one streams.
template <int COUT>
__global__ __launch_bounds__(256) void conv3x3_smallc2_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Wsm[];  // [cin][9 taps][4 co]
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  int t = blockIdx.x;
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int H = a.H, W = a.W, Cin = a.Cin;
  const int x = bx * 256 + 4 * lane, y0 = by * 8 + 2 * wv;
  for (int e = tid; e < Cin * 36; e += 256) {
    const int ci = e / 36, rem = e - ci * 36, tap = rem >> 2, co = rem & 3;
    Wsm[e] = co < COUT ? a.wp[((int64_t)ci * 9 + tap) * a.cout_pad + co] : 0.f;
  }
  __syncthreads();
  const float* __restrict__ xin =
      n < a.nsplit ? a.x + (int64_t)n * Cin * H * W : a.x2 + (int64_t)(n - a.nsplit) * Cin * H * W;
  const int64_t plane = (int64_t)H * W;
  // source rows y0 - 1 .. y0 + 2 (zero pad: -1 = none; reflect: mirrored)
  int srow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) srow[r] = src_index<1>(y0 - 1 + r, H, a.reflect);
  const bool inx = x < W;                                      // W % 4 == 0 (host)
  const int xl = src_index<1>(x - 1, W, a.reflect), xr = src_index<1>(x + 4, W, a.reflect);
  const bool own_l = lane == 0 || x == 0, own_r = lane == 63 || x + 4 >= W;  // load the neighbour itself
  float acc[2][COUT][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][co][j] = 0.f;
  // three channel buffers: channels c + 1 and c + 2 are in flight while channel c is computed
  float4 cen[3][4];
  float el[3][4], er[3][4];
  auto load = [&](int c, float4 (&cv)[4], float (&l)[4], float (&r)[4]) {
    const float* xc = xin + (int64_t)c * plane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = srow[k] >= 0;
      const float* row = xc + (int64_t)(ok ? srow[k] : 0) * W;
      cv[k] = (ok && inx) ? *reinterpret_cast<const float4*>(row + x) : make_float4(0.f, 0.f, 0.f, 0.f);
      l[k] = (ok && own_l && xl >= 0) ? row[xl] : 0.f;
      r[k] = (ok && own_r && xr >= 0) ? row[xr] : 0.f;
    }
  };
  auto compute = [&](int c, const float4 (&cv)[4], const float (&l)[4], const float (&r)[4]) {
    float v[4][6];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float left = __shfl_up(cv[k].w, 1, 64), right = __shfl_down(cv[k].x, 1, 64);
      v[k][0] = own_l ? l[k] : left;
      v[k][1] = cv[k].x;
      v[k][2] = cv[k].y;
      v[k][3] = cv[k].z;
      v[k][4] = cv[k].w;
      v[k][5] = own_r ? r[k] : right;
    }
    const float4* wc = reinterpret_cast<const float4*>(Wsm + c * 36);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float4 w4 = wc[ky * 3 + kx];
        const float wco[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int co = 0; co < COUT; ++co)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][co][j] = fmaf(v[i + ky][j + kx], wco[co], acc[i][co][j]);
      }
  };
  load(0, cen[0], el[0], er[0]);
  if (Cin > 1) load(1, cen[1], el[1], er[1]);
  for (int c0 = 0; c0 < Cin; c0 += 3) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {  // buffer u holds channel c0 + u
      const int c = c0 + u;
      if (c < Cin) {
        if (c + 2 < Cin) load(c + 2, cen[(u + 2) % 3], el[(u + 2) % 3], er[(u + 2) % 3]);
        compute(c, cen[u], el[u], er[u]);
      }
    }
  }
  if (!inx) return;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int yy = y0 + i;
    if (yy >= H) continue;
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      if (co >= a.Cout) break;
      const float bv = a.bias ? a.bias[co] : 0.f;
      const float4 o = make_float4(acc[i][co][0] + bv, acc[i][co][1] + bv, acc[i][co][2] + bv, acc[i][co][3] + bv);
      const int64_t off = (((int64_t)n * a.Cout + co) * H + yy) * W + x;
      if (a.y_pre) *reinterpret_cast<float4*>(a.y_pre + off) = o;
      if (a.y_act) *reinterpret_cast<float4*>(a.y_act + off) = make_float4(relu_f(o.x), relu_f(o.y), relu_f(o.z), relu_f(o.w));
    }
  }
}

// Direct (VALU) 3x3 conv for cin <= 4 — VGG conv_1 (3->64, models.py:199-216, with the
// Normalization of models.py:120-131 applied in the gather). As an implicit GEMM its K = 27 runs
// in 4-channel K-chunks behind 64-channel MFMA tiles and the launch is bound by writing 21x its
// input bytes; here a workgroup stages its 8x128-pixel source tile (+halo) once, each thread keeps
// its 3x6 input window per channel in registers and loops over the output channels 4 at a time:
// the workgroup's weights sit in LDS and each tap's 4 output channels are one broadcast 16-byte
// read (as wave-uniform scalar loads, 108 weights per trip spilled 150 SGPRs: 2 SGPR reloads per
// FMA pair); every store is a 512-B row run.
// NTS (configs 20, 22, 23) used to store through nontemporal stores; it is kept only as a
// configuration index and stores normally: the nontemporal form was the first suspect for the
// run-to-run differences seen under a second process's GPU load (DESIGN.md §4 open item), and the
// plain form costs nothing measurable (config 2: 568.6 img/s, profiles/r03_race_fix_trials.txt) --
// but the differences persist without it, so it was not their cause.
template <int CIN, bool NORM, int TH, bool NTS, int OCC>
__global__ __launch_bounds__(TH * 32, OCC) void conv3x3_cin4_kernel(ConvArgs a, const float* __restrict__ wp) {
  constexpr int NT = TH * 32, TWS = 128, COG = 4;
  constexpr int SR = TH + 2, RS = TWS + 8, C0 = 4;
  __shared__ __attribute__((aligned(16))) float As[CIN * SR * RS];
  extern __shared__ __attribute__((aligned(16))) float cin4_w[];  // [CIN * 9][cout_pad]

  const int tid = threadIdx.x;
  const int tx = tid & 31, ty = tid >> 5;
  int t = blockIdx.x;
  const int bx = t % a.tiles_x;
  t /= a.tiles_x;
  const int by = t % a.tiles_y;
  const int n = t / a.tiles_y;
  const int x0 = bx * TWS, y0 = by * TH;
  const int H = a.H, W = a.W;
  const float* __restrict__ xin =
      n < a.nsplit ? a.x + (int64_t)n * a.Cin * H * W : a.x2 + (int64_t)(n - a.nsplit) * a.Cin * H * W;
  const int plane = H * W;

  // Source tile, normalised; zero for zero padding and for channels past Cin (padding is
  // applied to the normalised image, as the reference pads after Normalization).
  // (all loads issued before any LDS store: one memory latency per tile, not one per element)
  constexpr int ST = CIN * SR * (TWS + 2), ST_T = (ST + NT - 1) / NT;
  float sv[ST_T];
#pragma unroll
  for (int i = 0; i < ST_T; ++i) {
    const int e = min(tid + i * NT, ST - 1);
    const int col = e % (TWS + 2);
    const int cr = e / (TWS + 2);
    const int r = cr % SR, c = cr / SR;
    const int sy = src_index<1>(y0 - 1 + r, H, a.reflect);
    const int sx = src_index<1>(x0 - 1 + col, W, a.reflect);
    const bool ok = c < a.Cin && sy >= 0 && sx >= 0;
    sv[i] = ok ? xin[c * plane + max(sy, 0) * W + max(sx, 0)] : 0.f;
  }
  for (int i = tid; i < CIN * 9 * a.cout_pad / 4; i += NT)
    reinterpret_cast<float4*>(cin4_w)[i] = reinterpret_cast<const float4*>(wp)[i];
#pragma unroll
  for (int i = 0; i < ST_T; ++i) {
    const int e = tid + i * NT;
    if (e < ST) {
      const int col = e % (TWS + 2);
      const int cr = e / (TWS + 2);
      const int c = cr / SR;
      float v = sv[i];
      if (NORM) {
        const int r = cr % SR;
        const bool ok = c < a.Cin && src_index<1>(y0 - 1 + r, H, a.reflect) >= 0 &&
                        src_index<1>(x0 - 1 + col, W, a.reflect) >= 0;
        v = ok ? (v - a.in_mean[c]) / a.in_std[c] : 0.f;  // padding stays 0 after normalisation
      }
      As[cr * RS + C0 - 1 + col] = v;
    }
  }
  __syncthreads();

  float v[CIN][3][6];
#pragma unroll
  for (int c = 0; c < CIN; ++c)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int m = 0; m < 6; ++m) v[c][ky][m] = As[(c * SR + ty + ky) * RS + C0 - 1 + 4 * tx + m];

  const int yy = y0 + ty, xx = x0 + 4 * tx;
  const bool ok = yy < H && xx < W;
  const bool full = ((W & 3) == 0) && xx + 3 < W;
  const int64_t obase = (int64_t)n * a.Cout * plane + (int64_t)yy * W + xx;
  const int cout_pad = a.cout_pad;
  for (int co0 = 0; co0 < a.Cout; co0 += COG) {  // cout_pad is a multiple of COG: slab reads in bounds
    float acc[COG][4];
#pragma unroll
    for (int k = 0; k < COG; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
    // tap-major, channel-minor: the MFMA kernel's accumulation order (bit-identical results)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int c = 0; c < CIN; ++c) {
          const float4 w4 = *reinterpret_cast<const float4*>(cin4_w + (c * 9 + ky * 3 + kx) * cout_pad + co0);
          const float wk[COG] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int k = 0; k < COG; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[k][j] = fmaf(v[c][ky][j + kx], wk[k], acc[k][j]);
          }
        }
    if (!ok) continue;
#pragma unroll
    for (int k = 0; k < COG; ++k) {
      const int co = co0 + k;
      if (co >= a.Cout) break;
      const float bv = a.bias ? a.bias[co] : 0.f;
      float o[4], u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = acc[k][j] + bv;
        u[j] = relu_f(o[j]);
      }
      const int64_t off = obase + (int64_t)co * plane;
      if (a.y_pre && dgrad_epi(a)) {  // input gradient (ast_conv3x3_dgrad_f32): y_pre only
        if (full) {
          *reinterpret_cast<float4*>(a.y_pre + off) = dgrad_epi4(a, make_float4(o[0], o[1], o[2], o[3]), off);
        } else {
          for (int j = 0; j < 4; ++j) if (xx + j < W) a.y_pre[off + j] = dgrad_epi_one(a, o[j], off + j);
        }
        continue;
      }
      if (a.y_pre) {
        if (full) {
          *reinterpret_cast<float4*>(a.y_pre + off) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
          for (int j = 0; j < 4; ++j) if (xx + j < W) a.y_pre[off + j] = o[j];
        }
      }
      if (a.y_act) {
        if (full) {
          *reinterpret_cast<float4*>(a.y_act + off) = make_float4(u[0], u[1], u[2], u[3]);
        } else {
          for (int j = 0; j < 4; ++j) if (xx + j < W) a.y_act[off + j] = u[j];
        }
      }
    }
  }
}

}  // namespace

namespace ast_conv {

template <int COUT>
int launch_smallc(const ConvArgs& a0, hipStream_t s, int up) {
  ConvArgs a = a0;
  if (a.Cout > COUT || a.y_pool) return AST_E_UNSUPPORTED;
  a.tiles_x = cdiv(a.W, 128);
  a.tiles_y = cdiv(a.H, 8);
  const int64_t nblk = (int64_t)a.tiles_x * a.tiles_y * a.N;
  if (nblk >= 0x7fffffff) return AST_E_SHAPE;
  if (up == 2)
    hipLaunchKernelGGL((conv3x3_smallc_kernel<COUT, 2>), dim3((unsigned)nblk), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((conv3x3_smallc_kernel<COUT, 1>), dim3((unsigned)nblk), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

template <int COUT>
int launch_smallc2(const ConvArgs& a0, hipStream_t s, int up) {
  ConvArgs a = a0;
  if (a.Cout > COUT || a.y_pool || up != 1 || (a.W & 3) || a.in_mean || a.Cin > 1024) return AST_E_UNSUPPORTED;
  a.tiles_x = cdiv(a.W, 256);
  a.tiles_y = cdiv(a.H, 8);
  const int64_t nblk = (int64_t)a.tiles_x * a.tiles_y * a.N;
  if (nblk >= 0x7fffffff) return AST_E_SHAPE;
  const int lds = a.Cin * 36 * 4;
  auto kern = conv3x3_smallc2_kernel<COUT>;
  [[maybe_unused]] static const void* const attr_set = with_dynamic_lds((const void*)kern, 1024 * 36 * 4);
  hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(256), lds, s, a);
  return (int)hipGetLastError();
}

template <int TH, bool NTS, int OCC>
int launch_cin4(const ConvArgs& a0, hipStream_t s, int up) {
  ConvArgs a = a0;
  if (a.Cin > 4 || a.y_pool || up != 1) return AST_E_UNSUPPORTED;
  a.tiles_x = cdiv(a.W, 128);
  a.tiles_y = cdiv(a.H, TH);
  const int64_t nblk = (int64_t)a.tiles_x * a.tiles_y * a.N;
  if (nblk >= 0x7fffffff) return AST_E_SHAPE;
  const dim3 g((unsigned)nblk), b(TH * 32);
  const bool norm = a.in_mean != nullptr;
  // weights in LDS: the instantiation's CIN (3, else 4: Cin 1 and 2 run the CIN = 4 kernel, which
  // copies and reads 4 channels' slabs -- the packed fp32 part holds cin_pad8 >= 4 of them, zero past
  // Cin), not a.Cin, or channels Cin..3 are read past the allocation
  const int cin_k = a.Cin == 3 ? 3 : 4;
  const size_t wl = (size_t)cin_k * 9 * a.cout_pad * sizeof(float);
  if (a.cout_pad % 4 || wl > 32 * 1024) return AST_E_UNSUPPORTED;
  if (a.Cin == 3) {
    if (norm) hipLaunchKernelGGL((conv3x3_cin4_kernel<3, true, TH, NTS, OCC>), g, b, wl, s, a, a.wp);
    else hipLaunchKernelGGL((conv3x3_cin4_kernel<3, false, TH, NTS, OCC>), g, b, wl, s, a, a.wp);
  } else {
    if (norm) hipLaunchKernelGGL((conv3x3_cin4_kernel<4, true, TH, NTS, OCC>), g, b, wl, s, a, a.wp);
    else hipLaunchKernelGGL((conv3x3_cin4_kernel<4, false, TH, NTS, OCC>), g, b, wl, s, a, a.wp);
  }
  return (int)hipGetLastError();
}

// the forms the configuration table names (10, 11; 36, 37; 18-23)
CONV_INSTANTIATE(launch_smallc<3>) CONV_INSTANTIATE(launch_smallc<4>)
CONV_INSTANTIATE(launch_smallc2<3>) CONV_INSTANTIATE(launch_smallc2<4>)
CONV_INSTANTIATE(launch_cin4<8, false, 1>) CONV_INSTANTIATE(launch_cin4<16, false, 1>)
CONV_INSTANTIATE(launch_cin4<8, true, 1>) CONV_INSTANTIATE(launch_cin4<4, false, 1>)
CONV_INSTANTIATE(launch_cin4<16, true, 1>) CONV_INSTANTIATE(launch_cin4<32, true, 1>)

}  // namespace ast_conv
