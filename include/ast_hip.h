/* ast_hip.h — C ABI of the MI355X (gfx950) AdaIN style-transfer hot path.
 *
 * The reference (rwickman/ArbitraryStyleTransfer) is pure Python: its "plugin" surface is the
 * nn.Module / function API of models.py, model_util.py and losses.py. Each entry point below is
 * the native kernel that replaces one reference operator; arbitrarystyletransfer_amd/ binds them
 * with ctypes behind that same module API (see INTEGRATION.md for the binding).
 *
 * Conventions: every tensor is a dense device pointer (HBM), fp32, NCHW unless stated;
 * `stream` is a hipStream_t passed as void*; no call allocates, copies to host or synchronises,
 * so every call is legal inside hipGraph capture. Return value: 0 on success, a negative
 * AST_E* code for an argument error (nothing launched), or a positive hipError_t.
 *
 * Determinism: every result is bitwise reproducible run to run on the same device and shapes.
 * No floating-point partial sum meets another through an atomic: reductions split across
 * workgroups write their partials into a caller-provided `workspace` (size from the matching
 * *_workspace_floats query; device memory, 16-byte aligned) and are summed in a fixed order, and
 * scalar losses accumulate into a loss accumulator (below).
 */
#ifndef AST_HIP_H
#define AST_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AST_OK 0
#define AST_E_NULLPTR (-1)
#define AST_E_SHAPE (-2)
#define AST_E_UNSUPPORTED (-3)

/* Library version / capability string (e.g. "ast_hip 0.1 gfx950"). */
const char* ast_version(void);

/* Loss accumulator: AST_LOSS_ACC_FLOATS device floats, zeroed once by the caller. [0] holds the
 * accumulated value; [1] is an arrival counter that every launch leaves at 0; [2..] hold one
 * partial per workgroup of the running launch, summed in workgroup order by the last workgroup
 * to finish. One stream at a time per accumulator. */
#define AST_LOSS_SLOTS 4096
#define AST_LOSS_ACC_FLOATS (2 + AST_LOSS_SLOTS)
int ast_loss_acc_floats(void);

/* ---------------------------------------------------------------------------------------------
 * 3x3 convolution, stride 1, "same" size, as an MFMA-fp32 implicit GEMM.
 * Replaces nn.Conv2d(k=3, padding=1) + ReLU (+ MaxPool2d(2,2)) of PretrainedEncoder
 * (models.py:199-224, forward :230-240) and ReflectionPad2d(1) + Conv2d + ReLU (+ the preceding
 * nn.Upsample(x2, nearest)) of the mirrored decoder (models.py:598-628).
 * ------------------------------------------------------------------------------------------ */

/* Number of floats of the packed weight buffer for a [cout, cin, 3, 3] filter bank. */
size_t ast_conv3x3_packed_numel(int cout, int cin);

/* Repack w[cout][cin][3][3] into the kernel layout (zero padded). The packed buffer holds the
 * fp32 pack [cin_pad8][9][cout_pad64] followed by the split-bf16 pack of the same weights (three
 * bf16 terms per value, w = hi + mid + lo exactly) that the fp32-accurate bf16-MFMA kernel reads. */
int ast_conv3x3_pack_weights_f32(const float* w, float* w_packed, int cout, int cin, void* stream);

/* (Re)build the split-bf16 part of a packed buffer from its fp32 part (the pack functions call it). */
int ast_conv3x3_pack_split_f32(float* w_packed, int cout, int cin, void* stream);

/* y = conv3x3(pad(upsample(x))) + bias, with fused epilogue stores.
 *   x        [n, cin, h_in, w_in]; output spatial size h = h_in*upsample, w = w_in*upsample
 *   upsample 1 or 2 (nearest, applied before padding, as Upsample -> ReflectionPad -> Conv)
 *   pad_mode 0 = zeros (VGG encoder, Conv2d(padding=1)), 1 = reflect (ReflectionPad2d(1))
 *   in_mean/in_std  optional [cin]: input normalised as (x - mean)/std before padding
 *                   (Normalization, models.py:120-131, fused into conv_1; may be NULL)
 *   y_pre    optional [n, cout, h, w]      conv output before ReLU (the conv_i taps)
 *   y_act    optional [n, cout, h, w]      ReLU(conv) (relu_i)
 *   y_pool   optional [n, cout, h/2, w/2]  MaxPool2d(2,2)(ReLU(conv)) (pool_i)
 *   bias     optional [cout]
 */
int ast_conv3x3_fwd_f32(const float* x, const float* w_packed, const float* bias,
                        float* y_pre, float* y_act, float* y_pool,
                        const float* in_mean, const float* in_std,
                        int n, int cin, int h_in, int w_in, int cout,
                        int upsample, int pad_mode, void* stream);

/* General form. cfg selects a kernel configuration (0..ast_conv3x3_num_configs()-1, tuner /
 * tests), cfg < 0 = automatic. x2/n2: optional second input batch of n2 images appended after
 * the n images of x (one launch encodes a content batch and a style batch; outputs hold n + n2
 * images). x2 = NULL and n2 = 0 for a single batch. */
int ast_conv3x3_num_configs(void);
int ast_conv3x3_fwd_f32_cfg(int cfg, const float* x, const float* x2, int n2,
                            const float* w_packed, const float* bias,
                            float* y_pre, float* y_act, float* y_pool,
                            const float* in_mean, const float* in_std,
                            int n, int cin, int h_in, int w_in, int cout,
                            int upsample, int pad_mode, void* stream);

/* Collapsed form of the upsampled decoder convs (nearest x2 -> ReflectionPad2d(1) -> conv3x3): the 9
 * taps of an output pixel touch 4 source pixels, so each output phase (row & 1, col & 1) is a 2x2
 * conv of the source with tap sums of w: 16 phase-taps per source pixel instead of 36 tap
 * applications. The collapsed slab (split-bf16, ast_conv3x3_up2c_numel floats, 16-byte aligned) is
 * derived from the fp32 part of a packed buffer, once per parameter version. The forward covers
 * upsample = 2, pad_mode = 1 (reflect), cin >= 16, outputs y_pre and / or y_act; anything else
 * returns AST_E_UNSUPPORTED (run ast_conv3x3_fwd_f32_cfg instead). Results differ from the 9-tap
 * kernels' by the fp32 rounding of the tap sums; an output reached by a non-finite input is
 * non-finite in both, but may be +-inf here where the 9-tap form gives NaN (opposite-sign taps). */
size_t ast_conv3x3_up2c_numel(int cout, int cin);
int ast_conv3x3_pack_up2c_f32(const float* w_packed, float* w_up2c, int cout, int cin, void* stream);
int ast_conv3x3_up2c_fwd_f32(const float* x, const float* x2, int n2, const float* w_up2c,
                             const float* bias, float* y_pre, float* y_act,
                             int n, int cin, int h_in, int w_in, int cout,
                             int upsample, int pad_mode, void* stream);
/* The same with the kernel form given: variant 8 = 8 waves, 32 x 32 output pixels, one workgroup
 * per CU; 4 = 4 waves, 16 x 32 output pixels, one weight-slab buffer, two workgroups per CU; 0 =
 * auto (what ast_conv3x3_up2c_fwd_f32 runs; AST_UP2C_TILE=8|4, read once, forces one). Both forms
 * give the same bits. ast_conv3x3_up2c_variant: the form auto takes for a shape (n images in all).
 * ast_conv3x3_up2c_occupancy: workgroups of a form that fit on one CU at its launch size (-1: error). */
int ast_conv3x3_up2c_fwd_f32_cfg(int variant, const float* x, const float* x2, int n2, const float* w_up2c,
                                 const float* bias, float* y_pre, float* y_act,
                                 int n, int cin, int h_in, int w_in, int cout,
                                 int upsample, int pad_mode, void* stream);
int ast_conv3x3_up2c_variant(int n, int cin, int h_in, int w_in, int cout);
int ast_conv3x3_up2c_occupancy(int variant);

/* ---------------------------------------------------------------------------------------------
 * Per-channel statistics and AdaIN.
 * ------------------------------------------------------------------------------------------ */

/* mean[p], std[p] over each of `planes` contiguous planes of `hw` elements.
 * std = sqrt(sum((x-mean)^2) / (hw - unbiased) + eps).
 *   channel_stats (model_util.py:3-8):  unbiased=1, eps=0
 *   calc_mean_std (models.py:54-62):    unbiased=1, eps=1e-5 */
int ast_channel_stats_f32(const float* x, float* mean, float* std, long long planes, long long hw,
                          int unbiased, float eps, void* stream);

/* AdaIN.forward (models.py:43-51) + alpha blend (models.py:471), one launch:
 *   t   = (c - mu_c) / sigma_c * scale + shift,   stats = channel_stats (unbiased, no eps)
 *   out = alpha * t + (1 - alpha) * c
 * swap_style_stats=1 reproduces the reference literally (scale = mu_s, shift = sigma_s,
 * SURVEY.md F1); 0 is canonical AdaIN (scale = sigma_s, shift = mu_s).
 * content [n, c, hc, wc], style [n, c, hs, ws], out [n, c, hc, wc]. */
int ast_adain_f32(const float* content, const float* style, float* out,
                  int n, int c, int hc, int wc, int hs, int ws,
                  double alpha, int swap_style_stats, void* stream);

/* AdaIN with precomputed style statistics (one-style-many-contents mode, SURVEY §8e: the rank
 * owning the style image computes them and broadcasts 2*C floats). style_mean/style_std are
 * indexed [n * style_stride_n + c]; style_stride_n = 0 shares one style across the batch.
 * std is the unbiased standard deviation (channel_stats, model_util.py:3-8). */
int ast_adain_stats_f32(const float* content, const float* style_mean, const float* style_std,
                        float* out, int n, int c, int hc, int wc, int style_stride_n, double alpha,
                        int swap_style_stats, void* stream);

/* Backward of ast_adain_f32: d_content and/or d_style (either may be NULL) from grad_out. */
int ast_adain_backward_f32(const float* content, const float* style, const float* grad_out,
                           float* d_content, float* d_style, int n, int c, int hc, int wc,
                           int hs, int ws, double alpha, int swap_style_stats, void* stream);

/* Regional multi-style AdaIN (csrc/adain_regions.hip; an extension, no reference counterpart).
 * labels [n, h, w] uint8, shared by the c planes of a sample: label k < regions puts the pixel in
 * region k, any label >= regions (255 by convention) passes it through untouched and keeps it out
 * of every statistic. Region statistics are the two-pass mean and unbiased std (no eps) over the
 * region's pixels only: NaN mean and std for an empty region, NaN std for a one-pixel region. */
#define AST_MAX_REGIONS 8
#define AST_MAX_STYLE_ROWS 64

/* Nearest-neighbour resize of label maps [n, hs, ws] -> [n, hd, wd]: src = (dst * in) / out per
 * axis in integer arithmetic (what F.interpolate(mode="nearest") picks). */
int ast_resize_labels_u8(const unsigned char* src, unsigned char* dst, long long n,
                         int hs, int ws, int hd, int wd, void* stream);

/* mean, std [n, regions, c] and count [n, regions] (int32) of x [n, c, h, w] per region. */
int ast_region_stats_f32(const float* x, const unsigned char* labels, float* mean, float* std,
                         int* count, int n, int c, int h, int w, int regions, void* stream);

/* One launch: for region k of sample n and channel ch, (m, s) = sum_t mix[n, k, t] * (style_mean,
 * style_std)[t, ch] over the `rows` rows of the table [rows, c] (rows with weight exactly 0 are
 * skipped, so they may hold NaN), (scale, shift) = (m, s) when swap_style_stats, else (s, m), and
 *   out = alpha * ((c - mu_k) / sd_k * scale + shift) + (1 - alpha) * c      on the region's pixels,
 *   out = c bit for bit                                                     where label >= regions.
 * mix [n or 1, regions, rows]; regions 1..AST_MAX_REGIONS, rows 1..AST_MAX_STYLE_ROWS. */
int ast_adain_regions_f32(const float* content, const unsigned char* labels,
                          const float* style_mean, const float* style_std, const float* mix,
                          float* out, int n, int c, int h, int w, int regions, int rows,
                          int mix_stride_n /* 0: one mix for the batch, else regions*rows */,
                          double alpha, int swap_style_stats, void* stream);

/* Exact feature distribution matching (EFDM, Zhang et al. CVPR 2022; csrc/efdm.hip; an extension,
 * no reference counterpart) and the segmented plane sort under it.
 * Order: IEEE-754 totalOrder of the bits -- as a signed integer key = b < 0 ? -(b & 0x7fffffff) - 1
 * : b for the int32 view b -- so -0 < +0, negative NaNs first, positive NaNs last, and equal keys
 * are equal bits. Ties keep index order (a stable ascending sort).
 * For every plane (n, ch), Mc = hc*wc, Ms = hs*ws: r(i) = the stable rank of content element i,
 * S = the style plane's values in ascending order, j(r) = ((2r + 1) * Ms) / (2 * Mc) in 64-bit
 * integers (the identity when Ms == Mc), t[i] = S[j(r(i))], and
 *   out[i] = t[i]                           when alpha == 1 (the style value's bits, no arithmetic),
 *   out[i] = c[i] + alpha * (t[i] - c[i])   otherwise, in fp32.
 * content, out [n, c, hc, wc]; style [ns, c, hs, ws] with ns == n, or ns == 1 (one style shared by
 * the batch). Planes of at most AST_EFDM_FUSED_MAX elements (both maps) run in one launch with no
 * workspace; anything larger, up to 2^31 - 1 elements per plane, sorts chunks in LDS and merges
 * them through `workspace` (device memory, 4-byte aligned, ast_efdm_workspace_bytes bytes; may be
 * NULL when that is 0). No host synchronisation, no atomics: bitwise reproducible, capturable.
 * The _ex form takes the LDS chunk length of the general path: 0 = automatic (what the plain entry
 * passes), else a power of two in 64..AST_EFDM_FUSED_MAX (AST_E_UNSUPPORTED otherwise), which
 * forces the general path at any size; its workspace is ast_efdm_ex_workspace_bytes with the same
 * chunk. AST_E_SHAPE: a size <= 0, ns not in {1, n}, a plane over 2^31 - 1 or a map over 2^40
 * elements, or a workspace smaller than the query. The workspace queries return the same negative codes for bad arguments. */
#define AST_EFDM_FUSED_MAX 16384
long long ast_efdm_workspace_bytes(int n, int ns, int c, long long mc, long long ms);
long long ast_efdm_ex_workspace_bytes(int n, int ns, int c, long long mc, long long ms, int chunk);
int ast_efdm_f32(const float* content, const float* style, float* out, int n, int ns, int c,
                 int hc, int wc, int hs, int ws, double alpha, void* workspace,
                 long long workspace_bytes, void* stream);
int ast_efdm_ex_f32(const float* content, const float* style, float* out, int n, int ns, int c,
                    int hc, int wc, int hs, int ws, double alpha, int chunk, void* workspace,
                    long long workspace_bytes, void* stream);

/* The segmented sort on its own: every row of x [planes, m] in the order above, as values
 * (`sorted`) and, when index_or_null is given, the int32 source index of each (ties in index
 * order). chunk and workspace as ast_efdm_ex_f32; the query takes want_index (0/1). */
long long ast_plane_sort_workspace_bytes(long long planes, long long m, int want_index, int chunk);
int ast_plane_sort_f32(const float* x, float* sorted, int* index_or_null, long long planes,
                       long long m, int chunk, void* workspace, long long workspace_bytes,
                       void* stream);

/* Regional EFDM (csrc/efdm_regions.hip; an extension, no reference counterpart): the matching above
 * per region of a label map, towards a per-region mix of a bank of styles. Order, keys and ties are
 * those of ast_efdm_f32.
 * Inputs: content c [n, ch, h, w] fp32; labels uint8 [n, h, w], shared by the channels of a sample;
 * K = regions in 1..AST_MAX_REGIONS: label k < K puts the pixel in region k, any label >= K (255 by
 * convention) passes it through. Styles [S, ch, hs, ws] shared by the batch, S in
 * 1..AST_MAX_STYLE_ROWS, optionally with style_labels uint8 [S, hs, ws]. mix fp32 [n or 1, K, S] on
 * the device, non-negative (the caller normalises the rows). Mc = h*w and Ms = hs*ws are at most
 * AST_EFDM_FUSED_MAX: a larger plane gives AST_E_UNSUPPORTED (the chunk-and-merge path of
 * ast_efdm_f32 has no regional form).
 * Rule, for sample b, channel and region k: I_k = the pixels with labels[b] == k, Mc_k their number,
 * r(i) the stable ascending rank of pixel i among I_k only. For style s, J_(s,k) = all its pixels or,
 * with style_labels, those with style_labels[s] == k; Ms_(s,k) their number; S_(s,k) the plane's
 * values on J_(s,k) in ascending order. t_s[i] = S_(s,k)[((2 r(i) + 1) * Ms_(s,k)) / (2 * Mc_k)] and
 * t[i] = sum_s mix[b, k, s] * t_s[i] in fp32 in ascending s (fp32 products, fp32 sums, nothing fused):
 * the 1-D Wasserstein barycentre of the styles' distributions. A weight of exactly 0 is skipped and its
 * style's values never reach the result (they may be NaN); when exactly one weight of the row is
 * non-zero, t[i] is that t_s[i] bit for bit, with no multiply; a row of zeros gives the empty sum, 0.
 *   out[i] = t[i]                           when alpha == 1,
 *   out[i] = c[i] + alpha * (t[i] - c[i])   otherwise, in fp32.
 * Pass-through, out = c bit for bit whatever alpha: where label >= K; in a region k for which a style
 * of non-zero weight has Ms_(s,k) == 0 (the rule of regional WCT). A non-finite value stays inside
 * its own region's ranking.
 * One region, one style and no style_labels is ast_efdm_f32 with ns = 1, bit for bit at alpha == 1.
 * Every plane is sorted once whatever K and S: the bank by one launch shared by the batch, the
 * content inside the apply launch; the rank inside a region is the count of earlier sorted positions
 * with the same label. No atomics, no host synchronisation, no allocation: bitwise reproducible; no
 * launch parameter depends on the contents of a label map, so a captured graph replays with other
 * labels. workspace: device memory, 4-byte aligned (AST_E_UNSUPPORTED otherwise), at least
 * ast_efdm_regions_workspace_bytes; it holds the sorted bank.
 * AST_E_NULLPTR: a null pointer (but the optional one). AST_E_SHAPE: a size <= 0, regions or S out of
 * range, a mix batch outside {1, n}, more than 2^31 - 1 planes, a short workspace. The query returns
 * the same negative codes. All checks run before the first launch. */

/* The bank stage on its own: every plane of x [s, c, h, w] in the order (min(label, K), key, index) --
 * region after region, each ascending, the pixels labelled >= K last -- as `sorted` [s, c, h*w], and
 * count [s, K] (int32), the pixels of every region. labels_or_null uint8 [s, h, w]; NULL: one region
 * holds everything (the plain ascending sort, count[:, 0] = h*w and 0 elsewhere). Any s >= 1. */
int ast_efdm_region_sort_f32(const float* x, const unsigned char* labels_or_null, float* sorted,
                             int* count, int s, int c, int h, int w, int regions, void* stream);

/* The whole op: the bank sort into the workspace, then one launch over the content planes. */
long long ast_efdm_regions_workspace_bytes(int n, int c, int hc, int wc, int regions, int styles,
                                           int hs, int ws);
int ast_efdm_regions_f32(const float* content, const unsigned char* labels, const float* styles,
                         const unsigned char* style_labels_or_null, const float* mix, float* out,
                         int n, int c, int hc, int wc, int regions, int styles_n, int hs, int ws,
                         int mix_n, double alpha, void* workspace, long long workspace_bytes,
                         void* stream);

/* Whitening and colouring transform (WCT, Li et al. NeurIPS 2017; csrc/wct.hip; an extension, no
 * reference counterpart): the feature transform that matches the cross-channel covariance.
 * content x [n, c, hc, wc], style s [ns, c, hs, ws] with ns == n, or ns == 1 (one style shared by the
 * batch); fp32; Mc = hc*wc, Ms = hs*ws, both >= 2. Per sample, with its map viewed as C x M:
 *   mu    = the per-channel mean;
 *   Sigma = (X - mu)(X - mu)^T / (M - 1) + eps I, centred in two passes (never E[xx^T] - mu mu^T),
 *           eps = eps_rel * max(tr / C, 1e-20), tr the trace of the unregularised covariance;
 *           Sigma equals its transpose bit for bit;
 *   T     = Sigma_s^(1/2) Sigma_c^(-1/2), the symmetric roots (ZCA whitening, then colouring);
 *   t     = T (x - mu_c) + mu_s,   out = alpha t + (1 - alpha) x.
 * A constant content map has tr = 0 exactly (the mean of a constant plane is its value) and gives
 * out = mu_s at alpha = 1. A non-finite value stays inside its own sample of the batch.
 * The roots are the coupled Newton-Schulz iteration, which fixes the fp32 behaviour:
 *   A = Sigma / ||Sigma||_F, Y_0 = A, Z_0 = I;  P_k = 1.5 I - 0.5 Z_k Y_k;
 *   Y_(k+1) = Y_k P_k, Z_(k+1) = P_k Z_k;  Sigma^(1/2) = Y sqrt(||Sigma||_F), Sigma^(-1/2) = Z / sqrt(||Sigma||_F)
 * for a fixed count `iters` (never a convergence test on the host). iters = 0 takes the default
 * ast_wct_default_iters(c, eps_rel) = ceil(log_2.25(c / eps_rel)) + 5 (22 for c = 512, eps_rel =
 * 1e-3): lambda_min(A) >= eps_rel / c, a small eigenvalue of Z Y grows 2.25x per step, and about five
 * quadratic steps finish from 0.5. eps_rel must lie in [1e-4, 1] (the default is 1e-3): below that
 * the fp32 iteration loses a rank-deficient covariance. Every product is an fp32
 * MFMA; ||.||_F, the trace and the split-K partial tiles of the covariance are summed in a fixed
 * order. c <= 1024.
 * Workspaces are device memory, 256-byte aligned, of at least the matching *_workspace_bytes query.
 * AST_E_SHAPE: a size <= 0, an M below 2, ns outside {1, n}, more than 32767 matrices, a short
 * workspace. AST_E_UNSUPPORTED: eps_rel outside [1e-4, 1], c > 1024, iters < 0. The queries return
 * the same negative codes. All checks run before the first launch. */
int ast_wct_default_iters(int c, float eps_rel);

/* mean [n, c] and cov [n, c, c] (ridge included) of x [n, c, m]. */
long long ast_wct_cov_workspace_bytes(int n, int c, long long m);
int ast_wct_cov_f32(const float* x, float* mean, float* cov, int n, int c, long long m, float eps_rel,
                    void* workspace, long long workspace_bytes, void* stream);

/* Sigma^(1/2) and / or Sigma^(-1/2) [b, c, c] of cov [b, c, c] (either output may be NULL, not both).
 * iters = 0 is the default count for eps_rel = 1e-3. */
long long ast_wct_sqrt_workspace_bytes(int b, int c);
int ast_wct_sqrt_f32(const float* cov, float* sqrt_or_null, float* isqrt_or_null, int b, int c, int iters,
                     void* workspace, long long workspace_bytes, void* stream);

/* out from the parts: content_mean [n, c], style_mean [ns, c], style_sqrt [ns, c, c],
 * content_isqrt [n, c, c]; T takes the workspace and t is never stored. */
long long ast_wct_apply_workspace_bytes(int n, int c);
int ast_wct_apply_f32(const float* content, const float* content_mean, const float* style_mean,
                      const float* style_sqrt, const float* content_isqrt, float* out, int n, int ns, int c,
                      long long mc, double alpha, void* workspace, long long workspace_bytes, void* stream);

/* The whole op: the two covariances, the roots of all n + ns matrices as one batch, the apply. */
long long ast_wct_workspace_bytes(int n, int ns, int c, long long mc, long long ms);
int ast_wct_f32(const float* content, const float* style, float* out, int n, int ns, int c,
                int hc, int wc, int hs, int ws, double alpha, float eps_rel,
                int iters /* 0 = the default above */, void* workspace, long long workspace_bytes,
                void* stream);

/* Regional WCT (Li et al. 2017, section 4: spatial control and style interpolation; csrc/wct.hip):
 * the transform above per region of a label map, towards a per-region mix of a bank of styles.
 * Inputs: content x [n, c, h, w] fp32; labels uint8 [n, h, w], M = h*w <= 2^24, K = regions in
 * 1..AST_MAX_REGIONS: label k < K puts the pixel in region k, any label >= K (255 by convention)
 * passes it through and keeps it out of every statistic. Styles s [S, c, hs, ws] shared by the batch,
 * S in 1..AST_MAX_STYLE_ROWS, optionally with style_labels uint8 [S, hs, ws]. mix fp32 [n or 1, K, S]
 * on the device, non-negative, rows summing to 1 (the caller normalises). c <= 1024 and
 * n K + S (K with style labels, else 1) <= 32767.
 * Region statistics: for region k of sample b take the M_k pixels labelled k in ascending pixel
 * index as a c x M_k map; mu and Sigma are exactly those of ast_wct_cov_f32 on that map, bit for bit
 * (mean x0 + sum(x - x0) / M_k with x0 the region's first pixel, two-pass centring, / (M_k - 1), the
 * ridge eps_rel * max(tr / c, 1e-20), Sigma symmetric in bits). A region with M_k < 2 is invalid: its
 * Sigma is stored as the identity and its mean as 0, so the batched roots stay finite. The style side
 * is ast_wct_cov_f32 of the whole style map or, with style_labels, the regional statistics of style
 * s's own region k.
 * Transform of region k: U_k = the styles with mix[b, k, s] != 0; C_k = sum_{s in U_k} w_s Sigma_s^(1/2)
 * and m_k = sum_{s in U_k} w_s mu_s in ascending s, the first used term the product w Y and the later
 * ones fmaf(w, Y, acc), so a one-hot row reproduces Sigma_s^(1/2) and mu_s in bits; a style of weight
 * exactly 0 is never read and may hold NaN. T_k = C_k Sigma_(c,k)^(-1/2), t = T_k (x - mu_(c,k)) + m_k,
 * out = alpha t + (1 - alpha) x on the region's pixels: the paper's interpolation, a blend of the
 * transformed features, as one GEMM per region.
 * Pass-through, out = x bit for bit whatever alpha: where label >= K; in an invalid content region;
 * in a region one of whose used styles has an invalid region k (style_labels: the class is absent
 * from the bank); in a region whose weights are all 0.
 * Roots: ast_wct_sqrt_f32, same eps_rel range and iters default, all matrices as one batch.
 * The pixels are binned by region once (a permutation ordered by (min(label, K), pixel index) and K
 * counts per sample) and every product reads its pixel axis through it: the MFMA work is that of the
 * unmasked transform whatever K. No atomics, no host synchronisation, no allocation; no launch
 * parameter depends on the contents of a label map, so a captured graph replays with other labels.
 * A non-finite value stays inside its own region of its own sample.
 * Workspaces are device memory, 256-byte aligned, of at least the matching *_workspace_bytes query.
 * AST_E_NULLPTR: a null pointer (but the optional ones). AST_E_SHAPE: a size <= 0, a plane over 2^24
 * pixels, a style plane below 2 pixels without style labels, regions or S out of range, a mix batch
 * outside {1, n}, too many matrices, a short workspace. AST_E_UNSUPPORTED: eps_rel outside [1e-4, 1],
 * c > 1024, iters < 0. The queries return the same negative codes. All checks run before the first
 * launch. */

/* mean [n, K, c], cov [n, K, c, c] (ridge included; the identity and 0 for an invalid region) and
 * count [n, K] (int32) of x under labels. */
long long ast_wct_region_cov_workspace_bytes(int n, int c, int h, int w, int regions);
int ast_wct_region_cov_f32(const float* x, const unsigned char* labels, float* mean, float* cov,
                           int* count, int n, int c, int h, int w, int regions, float eps_rel,
                           void* workspace, long long workspace_bytes, void* stream);

/* out from the parts: content_mean [n, K, c], content_isqrt [n, K, c, c]; style_mean [S, c] and
 * style_sqrt [S, c, c] or, with style_regional != 0, [S, K, c] and [S, K, c, c] with their counts
 * style_count_or_null [S, K] (NULL: every style region is valid; ignored when style_regional == 0);
 * mix [mix_n, K, S] with mix_n == 1 or n. The content is binned again here; C_k, m_k and T_k take
 * the workspace and t is never stored. */
long long ast_wct_region_apply_workspace_bytes(int n, int c, int h, int w, int regions);
int ast_wct_region_apply_f32(const float* content, const unsigned char* labels,
                             const float* content_mean, const float* content_isqrt,
                             const float* style_mean, const float* style_sqrt, const float* mix,
                             const int* style_count_or_null, float* out, int n, int c, int h, int w,
                             int regions, int styles, int mix_n, int style_regional, double alpha,
                             void* workspace, long long workspace_bytes, void* stream);

/* The whole op: exactly ast_wct_region_cov_f32 of the content, ast_wct_cov_f32 (or, with style
 * labels, ast_wct_region_cov_f32) of the styles, ast_wct_sqrt_f32 of all the matrices as one batch
 * (content regions first) and ast_wct_region_apply_f32, bit for bit. */
long long ast_wct_regions_workspace_bytes(int n, int c, int hc, int wc, int regions, int styles,
                                          int hs, int ws, int style_regional);
int ast_wct_regions_f32(const float* content, const unsigned char* labels, const float* styles,
                        const unsigned char* style_labels_or_null, const float* mix, float* out,
                        int n, int c, int hc, int wc, int regions, int styles_count, int hs, int ws,
                        int mix_n, double alpha, float eps_rel, int iters /* 0 = the default above */,
                        void* workspace, long long workspace_bytes, void* stream);

/* Style swap (Chen & Schmidt 2016; the style decorator of Avatar-Net, Sheng et al. CVPR 2018, when the
 * keys are normalised features; csrc/swap.hip; an extension, no reference counterpart): every 3x3
 * patch of the content map is replaced by the most similar patch of the style map and the overlaps
 * are averaged.
 * Inputs, all fp32 dense NCHW: content key ck [n, c, hc, wc], style key sk and style value sv
 * [ns, c, hs, ws] with ns == n, or ns == 1 (one style shared by the batch), content x [n, c, hc, wc].
 * Every side is at least 3, a map has at most 2^24 pixels, n <= 65535, c in 1..1024.
 * Patches: content patch i = y (wc - 2) + x exists for 0 <= y <= hc - 3, 0 <= x <= wc - 3, style patch
 * j = jy (ws - 2) + jx for 0 <= jy <= hs - 3, 0 <= jx <= ws - 3; a patch is the c x 3 x 3 block whose
 * top-left corner is at that position.
 * Match: score(i, j) = <ck patch i, sk patch j> / ||sk patch j||_2; a style patch of zero norm scores
 * exactly 0; index(i) = the j of maximal score, the lowest j on exactly equal scores; a NaN score
 * never wins. A score replaces the running pair (-inf, 0) only when strictly greater, so a content
 * patch for which nothing wins returns index 0 (and score -inf). The content patch's own norm does
 * not enter. index [n, hc - 2, wc - 2] int32 and the winning score [same shape] are outputs.
 * A score is one fp32 fma chain over (channel, tap) in a fixed order times the style patch's inverse
 * norm: it depends on the values of the two patches only, not on where the style patch sits, which
 * tile it falls in or how the style patches were split across workgroups.
 * Reconstruct: with (jy, jx) = index(y - dy, x - dx),
 *   out[n, ch, y, x] = (1 - alpha) x[n, ch, y, x] + alpha (1 / cnt(y, x)) sum sv[n', ch, jy + dy, jx + dx]
 * over the (dy, dx) in {0, 1, 2}^2 whose content patch (y - dy, x - dx) exists, in ascending (dy, dx)
 * order; cnt, 1..9, is the number of such terms. An index outside 0 .. (hs - 2)(ws - 2) - 1 given to
 * ast_patch_gather_f32 is clamped into that range.
 * Three stages and their composition, ast_style_swap_f32 (bit for bit). Workspaces are device
 * memory, 256-byte aligned, of at least the matching *_workspace_bytes query. No atomics, no host
 * synchronisation; a non-finite value stays inside its own sample of the batch.
 * AST_E_NULLPTR: a null pointer. AST_E_SHAPE: a side below 3, a size <= 0 or over the limits above, ns
 * outside {1, n}, a short workspace. AST_E_UNSUPPORTED: c > 1024, splits < 0. The queries return the
 * same negative codes. All checks run before the first launch. */

/* inv_norm [ns, (hs - 2)(ws - 2)] = 1 / ||sk patch j||_2, 0 for a zero (or non-finite) norm: the squared
 * norm of every pixel over the channels, a 3x3 box sum, a reciprocal square root, in the same order
 * at every position, so two equal style patches have equal inverse norms in bits. */
long long ast_patch_norms_workspace_bytes(int ns, int hs, int ws);
int ast_patch_norms_f32(const float* style_key, float* inv_norm, int ns, int c, int hs, int ws,
                        void* workspace, long long workspace_bytes, void* stream);

/* index (and score, when given) from the keys and the inverse norms. The style patches are split
 * across workgroups when the content tiles alone cannot fill the chip; the _ex form takes the split
 * count: 0 = the library's choice (what the plain entry passes), else that many (clamped to the
 * number of 64-patch style tiles and to 64). The result does not depend on it, bit for bit. The
 * query takes the same splits. */
long long ast_patch_match_workspace_bytes(int n, int ns, int hc, int wc, int hs, int ws, int splits);
int ast_patch_match_f32(const float* content_key, const float* style_key, const float* inv_norm,
                        int* index, float* score_or_null, int n, int ns, int c, int hc, int wc,
                        int hs, int ws, void* workspace, long long workspace_bytes, void* stream);
int ast_patch_match_ex_f32(const float* content_key, const float* style_key, const float* inv_norm,
                           int* index, float* score_or_null, int n, int ns, int c, int hc, int wc,
                           int hs, int ws, int splits, void* workspace, long long workspace_bytes,
                           void* stream);

/* out from the style value, the indices and the content (the alpha blend fused); one launch. */
int ast_patch_gather_f32(const float* style_value, const int* index, const float* content, float* out,
                         int n, int ns, int c, int hc, int wc, int hs, int ws, double alpha,
                         void* stream);

/* The whole op: norms of style_key, match, gather. index and score are written when given. */
long long ast_style_swap_workspace_bytes(int n, int ns, int hc, int wc, int hs, int ws);
int ast_style_swap_f32(const float* content_key, const float* style_key, const float* style_value,
                       const float* content, float* out, int* index_or_null, float* score_or_null,
                       int n, int ns, int c, int hc, int wc, int hs, int ws, double alpha,
                       void* workspace, long long workspace_bytes, void* stream);

/* Guided style swap (semantic / "neural doodle" patch transfer: Champandard 2016; Li & Wand CVPR 2016;
 * csrc/swap.hip): the patch match above, constrained to style patches of the content patch's own
 * class, over a bank of styles.
 * Inputs: content key ck and content x [n, c, hc, wc] as above; the style bank, keys sk and values sv
 * [s, c, hs, ws], s >= 1, shared by the batch. Ns = (hs - 2)(ws - 2); the global style patch index is
 * j = st Ns + jy (ws - 2) + jx for style st; s Ns < 2^31. Limits as above, with s in place of ns.
 * Classes, one per patch: content_class uint8 [n, hc - 2, wc - 2], style_class uint8 [s, hs - 2, ws - 2].
 * A class >= AST_SWAP_MAX_CLASSES takes no part: such a content patch gets no match, such a style patch
 * is never a candidate.
 * Match: score(i, j) is the score above, in bits (the same fma chain and inverse norm); index(i) = the
 * j of maximal score among the j with style_class(j) == content_class(i) < AST_SWAP_MAX_CLASSES; the
 * lowest global j wins on equal scores (so the lower style of the bank); a NaN never wins; without an
 * admissible candidate, or with none above -inf, index -1 and score -inf. With one class and s = 1 this
 * is the unguided match except for that -1 (there 0).
 * Reconstruct: the overlap average above over the covering content patches whose index is >= 0, in
 * ascending (dy, dx) order, cnt counting those; a pixel with cnt = 0 returns x[y, x] in bits, whatever
 * alpha. A negative index given to ast_patch_gather_guided_f32 is "no match"; one >= s Ns is clamped.
 * Stages: ast_patch_norms_f32 with ns = s gives the bank's inverse norms; the guided match first writes
 * one 64-bit class-presence mask per 64-patch content tile and per bank tile (a bank tile lies within
 * one style) into its workspace, then a workgroup visits a bank tile only if the two masks meet --
 * the work is the sum over classes of content tiles x bank tiles holding the class instead of all pairs
 * --; flag AST_SWAP_NO_SKIP of the _ex entry visits every tile (a test hook, like splits). The result
 * does not depend on the flag or on splits, bit for bit. ast_style_swap_guided_f32 is norms, guided
 * match, guided gather, bit for bit. Errors as above; s Ns >= 2^31 is AST_E_SHAPE, an unknown flag
 * AST_E_UNSUPPORTED. No atomics, no host synchronisation, no allocation. */
#define AST_SWAP_MAX_CLASSES 64
#define AST_SWAP_NO_SKIP 1
long long ast_patch_match_guided_workspace_bytes(int n, int s, int hc, int wc, int hs, int ws, int splits);
int ast_patch_match_guided_ex_f32(const float* content_key, const float* style_keys, const float* inv_norm,
                                  const unsigned char* content_class, const unsigned char* style_class,
                                  int* index, float* score_or_null, int n, int s, int c, int hc, int wc,
                                  int hs, int ws, int splits, int flags, void* workspace,
                                  long long workspace_bytes, void* stream);
int ast_patch_gather_guided_f32(const float* style_values, const int* index, const float* content, float* out,
                                int n, int s, int c, int hc, int wc, int hs, int ws, double alpha,
                                void* stream);
long long ast_style_swap_guided_workspace_bytes(int n, int s, int hc, int wc, int hs, int ws);
int ast_style_swap_guided_f32(const float* content_key, const float* style_keys, const float* style_values,
                              const float* content, const unsigned char* content_class,
                              const unsigned char* style_class, float* out, int* index_or_null,
                              float* score_or_null, int n, int s, int c, int hc, int wc, int hs, int ws,
                              double alpha, void* workspace, long long workspace_bytes, void* stream);

/* Relaxed earth mover's distance style loss (Kolkin et al., STROTSS, CVPR 2019; csrc/remd.hip; an
 * extension, no reference counterpart): a two-way nearest-neighbour match in cosine distance between
 * the pixels of two feature maps, exact (every pixel takes part, nothing is sampled), with a backward
 * to the first map.
 * Inputs, fp32 dense NCHW with the spatial sides flattened: x [n, c, m], the differentiable side, and
 * y [ns, c, p] with ns == n, or ns == 1 (one style shared by the batch). Pixel i of x and pixel j of y
 * are c-vectors. Limits: c in 1..AST_REMD_MAX_C, m and p in 1..AST_REMD_MAX_PIXELS, n <= 65535.
 * Inverse norms: u_i = 1 / ||x_i||_2, v_j = 1 / ||y_j||_2, exactly 0 when the squared norm is not
 * positive (or not finite). The squared norm is summed in one fixed order at every position, so equal
 * vectors have equal inverse norms in bits.
 * Distance: D(i, j) = 1 - (<x_i, y_j> u_i) v_j, the inner product one fp32 fma chain over the channels
 * in a fixed order: it depends on the two vectors only, not on where they sit, which tile they fall
 * in or how the style pixels were split across workgroups. A zero vector is at distance 1 from
 * everything.
 * Two-way match: r_i = min_j D(i, j) with arg-min a_i, c_j = min_i D(i, j) with arg-min b_j; the lowest
 * index on equal values; a NaN never wins; a value replaces the running (+inf, 0) only when strictly
 * less, so (+inf, 0) is what a pixel without a winner returns. row_min, row_index [n, m] and col_min,
 * col_index [n, p] (per sample also when ns == 1); the indices are int32. The distances are never stored.
 * Loss: rbar_b = (sum_i r_i) / m and cbar_b = (sum_j c_j) / p, each summed in a fixed order; sample b
 * takes the row branch (branch[b] = 1) when rbar_b >= cbar_b and the column branch (branch[b] = 2)
 * otherwise, and *loss += weight / n * sum_b (row branch ? rbar_b : cbar_b), the samples in a fixed
 * order: weight * mean_b max(rbar_b, cbar_b). force_branch 1 or 2 gives every sample that branch (a
 * test hook; 0 is the rule above). loss is a loss accumulator (AST_LOSS_ACC_FLOATS floats, above).
 * Backward, to x only (y is data). With g = *grad_scale (a device scalar), xh_i = u_i x_i:
 *   row branch     dx_i = -(g weight / (n m)) u_i (v_a y_a - (1 - r_i) xh_i),   a = a_i
 *   column branch  dx_i = -(g weight / (n p)) u_i sum over { j : b_j = i }, ascending, of
 *                         (v_j y_j - (1 - c_j) xh_i)
 * and exactly 0 where u_i = 0 or, in the column branch, where no column chose i. The lists of the
 * column branch are built with integer work alone (count, scan, stable fill), no atomics. An index
 * outside its map given to the backward is clamped into it.
 * Stages and their composition: ast_remd_loss_f32 is ast_cosine_norms_f32 on x, on y,
 * ast_cosine_match_f32 with splits 0 and ast_remd_means_f32, bit for bit. Workspaces are device
 * memory, 256-byte aligned, of at least the matching *_workspace_bytes query. No floating-point
 * atomics, no host synchronisation, no allocation; a non-finite value stays inside its own sample.
 * AST_E_NULLPTR: a null pointer. AST_E_SHAPE: a size <= 0 or over the limits above, ns outside {1, n},
 * a short workspace. AST_E_UNSUPPORTED: c > AST_REMD_MAX_C, splits < 0, force_branch outside 0..2. The
 * queries return the same negative codes. All checks run before the first launch. */
#define AST_REMD_MAX_C 1024
#define AST_REMD_MAX_PIXELS 4194304

/* inv_norm [n, pixels] of x [n, c, pixels]; one launch. */
int ast_cosine_norms_f32(const float* x, float* inv_norm, int n, int c, int pixels, void* stream);

/* The two-way match from the maps and their inverse norms. The style pixels are split across
 * workgroups when the content tiles alone cannot fill the chip: splits 0 = the library's choice, else
 * that many (clamped to the number of 64-pixel style tiles and to 64). The result does not depend on
 * it, bit for bit. The workspace holds one partial (min, index) pair per 64-pixel content tile and
 * style pixel, and per split and content pixel: 8 n (ceil(m / 64) p + splits m) bytes and alignment. */
long long ast_cosine_match_workspace_bytes(int n, int ns, int m, int p, int splits);
int ast_cosine_match_f32(const float* x, const float* y, const float* inv_x, const float* inv_y,
                         float* row_min, int* row_index, float* col_min, int* col_index, int n, int ns,
                         int c, int m, int p, int splits, void* workspace, long long workspace_bytes,
                         void* stream);

/* row_mean, col_mean [n], branch [n] uint8 and the loss from the minima; two launches. */
int ast_remd_means_f32(const float* row_min, const float* col_min, float* row_mean, float* col_mean,
                       unsigned char* branch, float* loss, int n, int m, int p, float weight,
                       int force_branch, void* stream);

/* The whole forward; every output is also what the backward reads. */
long long ast_remd_loss_workspace_bytes(int n, int ns, int m, int p);
int ast_remd_loss_f32(const float* x, const float* y, float* inv_x, float* inv_y, float* row_min,
                      int* row_index, float* col_min, int* col_index, float* row_mean, float* col_mean,
                      unsigned char* branch, float* loss, int n, int ns, int c, int m, int p, float weight,
                      int force_branch, void* workspace, long long workspace_bytes, void* stream);

/* dx [n, c, m] from the forward's outputs: the inverse lists (one launch), then one gather launch per
 * branch; every element of dx is written. Workspace: 4 n (2 m + 1 + p) bytes and alignment. */
long long ast_remd_loss_backward_workspace_bytes(int n, int m, int p);
int ast_remd_loss_backward_f32(const float* x, const float* y, const float* inv_x, const float* inv_y,
                               const float* row_min, const int* row_index, const float* col_min,
                               const int* col_index, const unsigned char* branch, const float* grad_scale,
                               float* dx, int n, int ns, int c, int m, int p, float weight, void* workspace,
                               long long workspace_bytes, void* stream);

/* Self-similarity content loss (Kolkin et al., STROTSS, CVPR 2019; csrc/selfsim.hip; an extension, no
 * reference counterpart): the pattern of pairwise cosine distances inside the stylised map is asked to
 * equal the pattern inside the content map, exact (every pixel pair takes part, nothing is sampled),
 * with a backward to the stylised map.
 * Inputs, fp32 dense NCHW with the spatial sides flattened: x [n, c, pixels], the differentiable side,
 * and cmap of the same shape. N = pixels. Limits: c in 1..AST_REMD_MAX_C, pixels in
 * 1..AST_SELFSIM_MAX_PIXELS, n <= 65535. Per sample, for either map f:
 * Inverse norm: u_i = 1 / ||f_i||_2, exactly 0 unless the squared norm is positive: ast_cosine_norms_f32.
 * Distance: D_f(i, j) = 1 - <f_i, f_j> (u_i u_j) for i != j and D_f(i, i) = 0 by definition (it is not
 * computed as 1 - ||fh||^2). The inner product is one fp32 fma chain over the channels in a fixed order:
 * its bits depend on the two vectors only, not on which tile either falls in, and D_f(i, j) = D_f(j, i)
 * in bits. A zero vector is at distance 1 from every other pixel.
 * Column sum: r_f(j) = sum_i D_f(i, j), computed as (N - 1) - (<fh_j, S> - ||fh_j||^2) with fh = u f and
 * S = sum_i fh_i, each sum in a fixed order. q_f(j) = 1 / r_f(j) when r_f(j) is positive and finite, else
 * 0: a map of one pixel gives q = 0, loss 0 and gradient 0.
 * Difference: e(i, j) = D_x(i, j) q_x(j) - D_c(i, j) q_c(j), the two products rounded on their own (equal
 * maps give exactly 0); s(i, j) = +1 / -1 / 0 for e > 0 / < 0 / otherwise: e == 0, a NaN and the diagonal
 * give 0.
 * Loss: L_b = (1 / N) sum_{i != j} |e(i, j)|, in [0, 2]; sums[b] = L_b; *loss += weight / n * sum_b L_b,
 * the samples in a fixed order. loss is a loss accumulator (AST_LOSS_ACC_FLOATS floats, above).
 * Column signed sum: t(j) = q_x(j) sum_{k != j} s(k, j) D_x(k, j).
 * Sign planes: pos and neg, int64 [n, N, ceil(N / 64)]: bit k of word (i, J) is set in pos when
 * s(i, 64 J + k) = +1 and in neg when it is -1. Diagonal bits and bits past N are 0.
 * Backward, to x only (cmap is data, and is not read). With g = *grad_scale (a device scalar), xh = u x:
 *   W(m, j) = (s(m, j) - t(j)) q_x(j) + (s(j, m) - t(m)) q_x(m)        (m != j; symmetric)
 *   G_m     = sum_{j != m} W(m, j) u_j x_j      (j ascending in pairs, the MFMA's order)
 *   dxh_m   = -(g weight / (n N)) G_m
 *   dx_m    = u_m (dxh_m - xh_m <xh_m, dxh_m>), exactly 0 where u_m = 0
 * No cosine is recomputed: the planes cost N^2 / 4 bytes per sample. Every element of dx is written once.
 * Stages and their composition: ast_selfsim_loss_f32 is ast_cosine_norms_f32 on x, on cmap,
 * ast_selfsim_colsum_f32 on x, on cmap, ast_selfsim_pairs_f32 and ast_selfsim_total_f32, bit for bit.
 * Workspaces are device memory, 256-byte aligned, of at least the matching *_workspace_bytes query. No
 * floating-point atomics, no host synchronisation, no allocation; a non-finite value stays inside its
 * own sample.
 * AST_E_NULLPTR: a null pointer. AST_E_SHAPE: a size <= 0 or over the limits above, a short workspace.
 * AST_E_UNSUPPORTED: c > AST_REMD_MAX_C. The queries return the same negative codes. All checks run
 * before the first launch. */
#define AST_SELFSIM_MAX_PIXELS 16384

/* col_sum [n, pixels] = r_f of x [n, c, pixels] and its inverse norms; two launches. Workspace: the
 * channel sums S, 4 n c bytes and alignment. */
long long ast_selfsim_colsum_workspace_bytes(int n, int c);
int ast_selfsim_colsum_f32(const float* x, const float* inv_norm, float* col_sum, int n, int c, int pixels,
                           void* workspace, long long workspace_bytes, void* stream);

/* sums [n], t [n, pixels] and the planes from the maps, their inverse norms and column sums: one
 * workgroup per pair (I <= J) of 64-pixel tiles, 2 N^2 c FLOP per sample, then the merge of t in tile
 * order and the per-sample sum. Workspace: one partial of t per (tile, pixel) and one loss partial per
 * tile pair: 4 n (ceil(N / 64) N + pairs) bytes and alignment. */
long long ast_selfsim_pairs_workspace_bytes(int n, int pixels);
int ast_selfsim_pairs_f32(const float* x, const float* cmap, const float* inv_x, const float* inv_c,
                          const float* r_x, const float* r_c, float* sums, float* t, long long* pos,
                          long long* neg, int n, int c, int pixels, void* workspace,
                          long long workspace_bytes, void* stream);

/* *loss += weight / n * sum_b sums[b]; one workgroup. */
int ast_selfsim_total_f32(const float* sums, float* loss, int n, float weight, void* stream);

/* The whole forward; inv_x, r_x, t, pos and neg are what the backward reads. */
long long ast_selfsim_loss_workspace_bytes(int n, int c, int pixels);
int ast_selfsim_loss_f32(const float* x, const float* cmap, float* inv_x, float* inv_c, float* r_x,
                         float* r_c, float* t, long long* pos, long long* neg, float* sums, float* loss,
                         int n, int c, int pixels, float weight, void* workspace,
                         long long workspace_bytes, void* stream);

/* dx [n, c, pixels] from the forward's outputs: the GEMM of W' with x (2 N^2 c FLOP per sample) into
 * the workspace, then the normalisation backward. Workspace: G, 4 n c pixels bytes and alignment. */
long long ast_selfsim_loss_backward_workspace_bytes(int n, int c, int pixels);
int ast_selfsim_loss_backward_f32(const float* x, const float* inv_x, const float* r_x, const float* t,
                                  const long long* pos, const long long* neg, const float* grad_scale,
                                  float* dx, int n, int c, int pixels, float weight, void* workspace,
                                  long long workspace_bytes, void* stream);

/* Contextual loss (Mechrez, Talmi, Zelnik-Manor, ECCV 2018; csrc/cx.hip; an extension, no reference
 * counterpart): the soft counterpart of the relaxed EMD above, on the same pairwise cosine distances,
 * exact, without ever storing an m x p tensor. tests/cx_ref.py restates the definition.
 * Inputs, fp32 NCHW with the spatial sides flattened: x [n, c, m], the stylised map and the
 * differentiable side; y [ns, c, p], ns = n or 1, data (no gradient); h > 0, the bandwidth, a runtime
 * float; eps = AST_CX_EPS. Limits: c in 1..AST_CX_MAX_C, m and p in 1..AST_CX_MAX_PIXELS, n <= 65535.
 * Centring (center != 0, the authors' default): mu[c] = mean_j y[c, j], summed in a fixed order;
 *   xc = x - mu, yc = y - mu. With center == 0, xc = x and yc = y and mu, xc, yc may be null.
 * Distances: u_i, v_j and D(i, j) = 1 - (<xc_i, yc_j> u_i) v_j are those of ast_cosine_norms_f32 /
 *   ast_cosine_match_f32 on (xc, yc), bit for bit: the same inverse-norm rule, the same fma chain, a
 *   zero vector at distance 1 from everything. No clamp: eps keeps r_i + eps positive.
 * Row side: r_i = min_j D(i, j) with arg-min m_i (ast_cosine_match_f32 as it is); k_i = 1 / (r_i + eps);
 *   w(i, j) = exp((1 - D(i, j) k_i) / h);  S_i = sum_j w(i, j);  E_i = sum_j w(i, j) D(i, j).
 * Column side: CX(i, j) = w(i, j) / S_i; c_j = max_i CX(i, j) with arg-max a_j, the lowest index on
 *   equal values; a NaN never wins; without a winner the pair stays (-inf, 0).
 * Loss: CX_b = (1 / p) sum_j c_j, summed in a fixed order; *loss += weight / n * sum_b -log CX_b, the
 *   samples in sample order, into the loss accumulator (ast_loss_acc_floats).
 * Gradient, to x only, g = *grad_scale; xh_i = u_i xc_i, yh_j = v_j yc_j; J_i = { j : a_j = i }, ascending:
 *   A_i = sum_{j in J_i} w(i, j);  B_i = sum_{j in J_i} w(i, j) D(i, j);  T_i = B_i / S_i - A_i E_i / S_i^2
 *   G_i = (k_i / (h S_i)) (sum_{j in J_i} w(i, j) yh_j - (A_i / S_i) sum_j w(i, j) yh_j)
 *         - (k_i^2 T_i / h) yh_{m_i}
 *   dx_i = -(g weight / (n p CX_b)) u_i (G_i - xh_i <xh_i, G_i>)
 *   A row with empty J_i has dx_i = 0 exactly, and so does a row with u_i = 0. mu is data, so dx is the
 *   gradient of x itself.
 * Stages and their composition: ast_cx_loss_f32 is ast_cx_center_f32 (when center), ast_cosine_norms_f32
 * on xc, on yc, ast_cosine_match_f32 with splits 0 (its column outputs go to the workspace, unused),
 * ast_cx_rowsum_f32 and ast_cx_colmax_f32 with splits 0 and ast_cx_value_f32, bit for bit. The forward
 * is three passes of 2 m p c FLOP per sample; the backward recomputes D once per group of 512 channels
 * and multiplies the weight tile once: 2 m p c (ceil(c / 512) + 1) FLOP. Workspaces are device memory,
 * 256-byte aligned, of at least the matching *_workspace_bytes query. No floating-point atomics, no
 * host synchronisation, no allocation; a non-finite value stays inside its own sample.
 * AST_E_NULLPTR: a null pointer. AST_E_SHAPE: a size <= 0 or over the limits above, ns neither n nor 1,
 * a short workspace. AST_E_UNSUPPORTED: c > AST_CX_MAX_C, splits < 0, h <= 0 or not finite. The queries
 * return the same negative codes. All checks run before the first launch. */
#define AST_CX_MAX_C 1024
#define AST_CX_MAX_PIXELS 16384
#define AST_CX_EPS 1e-5f

/* mu [ns, c], xc [n, c, m], yc [ns, c, p]: three launches. */
int ast_cx_center_f32(const float* x, const float* y, float* mu, float* xc, float* yc, int n, int ns, int c,
                      int m, int p, void* stream);

/* row_sum = S, row_dsum = E [n, m] from the centred maps, their inverse norms and the match's row
 * minima. splits: the workgroups that share a row's style tiles; 0 is the library's choice, which depends
 * on the shapes alone. The partials of a row are added in split order, so the result is reproducible for
 * a given splits; it need not be equal across split counts. Workspace: 8 n splits m bytes and alignment. */
long long ast_cx_rowsum_workspace_bytes(int n, int ns, int m, int p, int splits);
int ast_cx_rowsum_f32(const float* xc, const float* yc, const float* inv_x, const float* inv_y,
                      const float* row_min, float* row_sum, float* row_dsum, int n, int ns, int c, int m, int p,
                      float h, int splits, void* workspace, long long workspace_bytes, void* stream);

/* col_cx = c_j, col_index = a_j, col_dist = D(a_j, j) [n, p]. The result does not depend on splits, bit
 * for bit. Workspace: one (value, index, distance) per content tile and style pixel,
 * 12 n ceil(m / 64) p bytes and alignment. */
long long ast_cx_colmax_workspace_bytes(int n, int ns, int m, int p);
int ast_cx_colmax_f32(const float* xc, const float* yc, const float* inv_x, const float* inv_y,
                      const float* row_min, const float* row_sum, float* col_cx, int* col_index,
                      float* col_dist, int n, int ns, int c, int m, int p, float h, int splits, void* workspace,
                      long long workspace_bytes, void* stream);

/* sample_cx [n] = CX_b; *loss += weight / n * sum_b -log CX_b; two launches. */
int ast_cx_value_f32(const float* col_cx, float* sample_cx, float* loss, int n, int p, float weight,
                     void* stream);

/* The whole forward; xc, yc (x, y when center == 0), inv_x, inv_y, row_min, row_index, row_sum, row_dsum,
 * col_index, col_dist and sample_cx are what the backward reads. Workspace: the match's unused column
 * outputs, 8 n p bytes, and the largest stage workspace. */
long long ast_cx_loss_workspace_bytes(int n, int ns, int m, int p);
int ast_cx_loss_f32(const float* x, const float* y, float* mu, float* xc, float* yc, float* inv_x,
                    float* inv_y, float* row_min, int* row_index, float* row_sum, float* row_dsum,
                    float* col_cx, int* col_index, float* col_dist, float* sample_cx, float* loss, int n,
                    int ns, int c, int m, int p, float weight, float h, int center, void* workspace,
                    long long workspace_bytes, void* stream);

/* dx [n, c, m] from the forward's outputs: the inverse lists, the row scalars, the dense pass and the
 * finishing pass. Workspace: the lists (4 n (2 m + 1 + p) bytes), the row scalars and flags
 * (16 n m + 4 n ceil(m / 64)) and G (4 n c m), each aligned. */
long long ast_cx_loss_backward_workspace_bytes(int n, int c, int m, int p);
int ast_cx_loss_backward_f32(const float* xc, const float* yc, const float* inv_x, const float* inv_y,
                             const float* row_min, const int* row_index, const float* row_sum,
                             const float* row_dsum, const int* col_index, const float* col_dist,
                             const float* sample_cx, const float* grad_scale, float* dx, int n, int ns, int c,
                             int m, int p, float weight, float h, void* workspace, long long workspace_bytes,
                             void* stream);

/* Feature k-means and the label mode filter (csrc/kmeans.hip; an extension, no reference counterpart):
 * the stage that makes the uint8 label maps of the regional transforms above from the features
 * themselves, as Multimodal Style Transfer (Zhang et al., ICCV 2019) clusters the style's relu4_1
 * features into sub-styles and assigns every content pixel to one of them.
 * A bank is x [b, c, h, w], fp32 dense NCHW: point g = map * h w + pixel is the c-vector at that pixel
 * and all b h w points are clustered together. 1 <= c <= AST_KMEANS_MAX_C, h, w >= 1,
 * b h w <= AST_KMEANS_MAX_POINTS. Centroids are [k, c] fp32, 1 <= k <= AST_KMEANS_MAX_K (= AST_MAX_REGIONS).
 * d(g, j) = sum over channels of (x - centroid_j)^2 in fp32, a fixed summation order that depends on
 * the shape alone, so equal centroids give equal distances in bits.
 * Assign: label(g) = the j of least d, the lowest j on equal distances; a distance replaces the running
 * (+inf, 255) only when strictly smaller, so a NaN never wins and a point without a winner gets label
 * 255 and belongs to no cluster (the "label >= K" convention above). labels is uint8 [b, h, w].
 * Update: from x, labels and the previous centroids, sum_j = the fp32 sum of the points labelled j and
 * count_j (int32) their number; centroid_j = sum_j / count_j, and a cluster of count 0 keeps its previous
 * centroid in bits. centroids may be prev_centroids. Workgroups write partial sums into the workspace
 * and a second launch adds them in a fixed order: no floating-point atomics.
 * Seed ("maximin"): m = the mean of all points; seed 0 = the g of largest d(g, m); seed j = the g of
 * largest min over the earlier seeds of d(g, seed); ties to the lowest g; a point whose distance is a
 * NaN is never chosen, and 0 is returned where none compares. seeds is int32 [k], global point indices.
 * Lloyd, ast_kmeans_f32: the initial centroids are bitwise copies of init [k, c], or, with init null,
 * of the points at the maximin seeds (also written to seeds_or_null when given); then `iters` rounds of
 * assign and update -- one launch that stages a tile of pixels, labels it and adds it into the
 * workgroup's partial sums, so the bank is read once per round, and the small reduction --, then one
 * final assign, so the returned labels and counts belong to the returned centroids. It equals the
 * composition of the three stages bit for bit. The number of launches is fixed: no convergence test,
 * no host synchronisation, no allocation; the op can be captured into a graph.
 * One workspace query serves every entry. AST_E_NULLPTR: a null pointer (but the optional ones).
 * AST_E_SHAPE: a size <= 0, too many points, a short workspace. AST_E_UNSUPPORTED: c or k over the limit,
 * iters < 0. The query returns the same negative codes. All checks run before the first launch. */
#define AST_KMEANS_MAX_K 8
#define AST_KMEANS_MAX_C 1024
#define AST_KMEANS_MAX_POINTS (1 << 24)
long long ast_kmeans_workspace_bytes(int b, int c, int h, int w, int k);
int ast_kmeans_seed_f32(const float* x, int* seeds, int b, int c, int h, int w, int k, void* workspace,
                        long long workspace_bytes, void* stream);
int ast_kmeans_assign_f32(const float* x, const float* centroids, unsigned char* labels, int b, int c,
                          int h, int w, int k, void* stream);
int ast_kmeans_update_f32(const float* x, const unsigned char* labels, const float* prev_centroids,
                          float* centroids, int* counts, int b, int c, int h, int w, int k,
                          void* workspace, long long workspace_bytes, void* stream);
int ast_kmeans_f32(const float* x, const float* init_or_null, float* centroids, unsigned char* labels,
                   int* counts, int* seeds_or_null, int b, int c, int h, int w, int k, int iters,
                   void* workspace, long long workspace_bytes, void* stream);

/* `passes` rounds of a 3x3 majority vote over uint8 label maps [n, h, w] (out must not be labels): the
 * window is clipped at the borders, only labels < regions vote, the most frequent label wins; on a tie
 * the centre's own label if it is among the tied, else the lowest. A pixel whose own label is
 * >= regions passes through. passes = 0 copies. More than one pass needs the workspace of the query.
 * regions outside 1..AST_MAX_REGIONS or passes < 0: AST_E_UNSUPPORTED. */
long long ast_label_mode_filter_workspace_bytes(int n, int h, int w, int passes);
int ast_label_mode_filter_u8(const unsigned char* labels, unsigned char* out, int n, int h, int w,
                             int regions, int passes, void* workspace, long long workspace_bytes,
                             void* stream);

/* out = (x - mean[p]) / std[p] per plane (mean_variance_norm, models.py:64-68, given stats). */
int ast_plane_normalize_f32(const float* x, const float* mean, const float* std, float* out,
                            long long planes, long long hw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 3x3 conv backward (training step). Input gradients run ast_conv3x3_fwd_f32_cfg on a
 * transposed+flipped pack of the filter (cin' = cout, cout' = cin, zero padding):
 * dgrad_same(dy) = gradient of the padded input at its interior.
 * ------------------------------------------------------------------------------------------ */

/* transpose_flip = 0: same as ast_conv3x3_pack_weights_f32. transpose_flip = 1: pack
 * W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx] / (in_scale ? in_scale[ci] : 1) (in_scale folds
 * the conv_1 normalisation's 1/std into the image gradient); its packed size is
 * ast_conv3x3_packed_numel(cin, cout). */
int ast_conv3x3_pack_weights_ex_f32(const float* w, float* w_packed, int cout, int cin,
                                    int transpose_flip, const float* in_scale, void* stream);

/* Backward of y_pre -> ReLU -> [MaxPool2d(2,2)] (models.py:216-218):
 * dy = g_pre + (pre > 0) * (g_act + unpool(g_pool)); any of g_pre/g_act/g_pool may be NULL.
 * pre [planes, h, w], g_pool [planes, h/2, w/2]. */
int ast_conv_act_backward_f32(const float* pre, const float* g_pre, const float* g_act,
                              const float* g_pool, float* dy, long long planes, int h, int w,
                              void* stream);

/* out = mask > 0 ? g : 0 (ReLU backward given the ReLU output). */
int ast_relu_mask_f32(const float* g, const float* mask, float* out, long long n, void* stream);

/* Decoder dgrad, step 1: out_pad [planes, h+2, pitch] = zero-padded (mask > 0 ? g : 0)
 * (g [planes, h, w]; mask = the layer's ReLU output, or NULL). A zero-padded same conv of
 * out_pad with the transposed+flipped filter is then the FULL gradient of the padded input. */
int ast_grad_pad_f32(const float* g, const float* mask, float* out_pad, long long planes,
                     int h, int w, int pitch, void* stream);

/* Decoder dgrad, step 3: adjoint of Upsample(x upsample, nearest) -> ReflectionPad2d(1): folds
 * the full padded-input gradient dp_full [planes, h_in*up+2, pitch] onto dx [planes, h_in, w_in]. */
int ast_pad_up_adjoint_f32(const float* dp_full, float* dx, long long planes, int h_in, int w_in,
                           int upsample, int pitch, void* stream);

/* Input gradient with a fused epilogue (round 5; replaces the grad_pad -> dgrad -> pad_up_adjoint
 * chain of the decoder and the ReLU backward of the layer below, models.py:216-218, 598-628).
 * For the forward y = conv3x3(pad(upsample(x))) with dy [n, cout, h, w] (h, w: the conv's output
 * grid, = upsample x the source grid): dx [n, cin, h/up, w/up] = epi(S(D)) where D = the zero-padded
 * same conv of dy with the transposed+flipped pack w_tf_packed (the interior of the padded-input
 * gradient), S = the 2x2 window sum when upsample == 2 (the nearest-upsample adjoint), and
 * epi(v) = mask > 0 ? add_post + (v + add_pre) : add_post per element of dx (mask, add_pre,
 * add_post [n, cin, h/up, w/up], each optional: no mask keeps every element, no add_post reads 0).
 * Reflect padding's border fold is ast_dgrad_reflect_border_f32, run after this.
 * The epilogue is the split-bf16 kernels' (cfg 24-35) and, for upsample 1, the cout <= 4 direct
 * kernels' (cfg 18-23) and the cout <= 3 split-bf16 ones' (cfg 42, 43; -1 = heuristic):
 * AST_E_UNSUPPORTED for any other configuration -- the
 * caller then runs ast_conv3x3_fwd_f32_cfg + ast_dgrad_finish_f32. */
int ast_conv3x3_dgrad_f32(int cfg, const float* dy, const float* w_tf_packed, float* dx,
                          const float* mask, const float* add_pre, const float* add_post, int n,
                          int cout, int h, int w, int cin, int upsample, void* stream);

/* The same epilogue as a separate pass over a plain input-gradient conv's output raw
 * [planes, h*up, w*up]: dx [planes, h, w] = epi(S(raw)). */
int ast_dgrad_finish_f32(const float* raw, float* dx, const float* mask, const float* add_pre,
                         const float* add_post, long long planes, int h, int w, int upsample,
                         void* stream);

/* Reflect-pad border of the input gradient of conv3x3(ReflectionPad2d(1)(upsample(x))): adds to
 * dx [n, cin, h, w_in] the padded-input gradient's four border lines (computed from dy [n, cout,
 * h*up, w_in*up] and the forward filter w [cout, cin, 3, 3] into the workspace, with dy's edge
 * columns made contiguous there first) folded as the
 * reflect pad and upsample map them, masked like the interior (mask [n, cin, h, w_in] > 0, or
 * NULL). workspace: ast_dgrad_reflect_border_workspace_floats floats. */
long long ast_dgrad_reflect_border_workspace_floats(int n, int cout, int cin, int h, int w_in, int upsample);
int ast_dgrad_reflect_border_f32(const float* dy, const float* w, float* dx, const float* mask,
                                 float* workspace, long long workspace_floats, int n, int cout,
                                 int cin, int h, int w_in, int upsample, void* stream);

/* dw [cout, cin, 3, 3] = sum over images/pixels of dy x pad(upsample(x)) (overwritten; split-bf16
 * MFMA, split over pixel tiles: each split's partial dW/db goes to the workspace, then one ordered
 * reduce); db [cout] = sum of dy (optional). workspace: ast_conv3x3_wgrad_workspace_floats floats. */
long long ast_conv3x3_wgrad_workspace_floats(int n, int cin, int h_in, int w_in, int cout, int upsample);
int ast_conv3x3_wgrad_f32(const float* x, const float* dy, float* dw, float* db,
                          int n, int cin, int h_in, int w_in, int cout,
                          int upsample, int pad_mode, float* workspace, long long workspace_floats,
                          void* stream);

/* Same with dy read through (pitch, plane stride, offset of element (0,0)) — e.g. the padded
 * gradient buffer of ast_grad_pad_f32 (pitch, (h+2)*pitch, pitch+1). dy_pitch = 0: dense. */
int ast_conv3x3_wgrad_ex_f32(const float* x, const float* dy, float* dw, float* db,
                             int n, int cin, int h_in, int w_in, int cout, int upsample,
                             int pad_mode, int dy_pitch, long long dy_plane, long long dy_offset,
                             float* workspace, long long workspace_floats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses (losses.py). Loss values are ADDED into the loss accumulator `loss` (AST_LOSS_ACC_FLOATS
 * floats, value at [0]; may be NULL); gradients are written (accumulate=0) or added
 * (accumulate=1) into `dx` (may be NULL = value only). `weight` multiplies both; `gscale` (device
 * scalar or NULL) multiplies the gradient only (autograd's grad_output).
 * ------------------------------------------------------------------------------------------ */

/* gram_matrix (losses.py:105-109): gram[b] = scale * feat[b] feat[b]^T, feat [n, c, hw],
 * gram [n, c, c] (overwritten; split-K MFMA, the K-splits' partial tiles summed in order through
 * the workspace of ast_gram_workspace_floats floats, 0 when the launch needs no split). */
long long ast_gram_workspace_floats(int n, int c, long long hw);
int ast_gram_f32(const float* feat, float* gram, int n, int c, long long hw, float scale, float* workspace,
                 long long workspace_floats, void* stream);

/* dfeat[b] (+)= scale * (dgram[b] + dgram[b]^T) feat[b] + row_a[b,i] * feat[b,i,:] + row_b[b,i]
 * (the backward of gram_matrix, with compute_style_loss's mean/std gradients fused: row_a/row_b
 * from ast_style_moments_ws_f32, or both NULL). */
int ast_gram_backward_f32(const float* feat, const float* dgram, float* dfeat,
                          const float* row_a, const float* row_b,
                          int n, int c, long long hw, float scale, const float* gscale,
                          int accumulate, void* stream);

/* compute_content_loss(mean_variance_norm(x), mean_variance_norm(y)) (losses.py:124-126,
 * models.py:64-68; train.py:225): loss += weight * mean(huber(mvn(x) - mvn(y))). With pstats
 * [planes, 6] (or NULL) it also keeps what the backward needs.
 * Split over (chunk, plane) workgroups: partial moments and Huber sums of each chunk of 8192
 * elements go to `workspace` (ast_plane_stats_workspace_floats(planes, hw) floats) and are merged
 * in chunk order, so few large planes fill the chip. Three launches. */
long long ast_plane_stats_workspace_floats(long long planes, long long hw);
int ast_mvn_huber_ws_f32(const float* x, const float* y, long long planes, long long hw, float weight,
                         float* loss, float* pstats, float* workspace, long long workspace_floats,
                         void* stream);

/* d/dx of the above (y constant), from the forward's pstats: one pass over x and y. */
int ast_mvn_huber_backward_f32(const float* x, const float* y, const float* pstats, long long planes,
                               long long hw, float weight, const float* gscale, float* dx,
                               int accumulate, void* stream);

/* compute_content_loss(x, y) = F.huber_loss(x, y) (delta 1, mean). */
int ast_huber_f32(const float* x, const float* y, long long n, float weight, const float* gscale,
                  float* loss, float* dx, int accumulate, void* stream);

/* Mean/std part of compute_style_loss (losses.py:130-134):
 * loss += weight * 1.25 * (mean huber(mu_x - mu_y) + mean huber(sd_x - sd_y)) over planes,
 * stats [planes, 4] = (mu_x, sd_x, mu_y, sd_y); row_a/row_b [planes] = per-plane gradient
 * d/dx = row_a * x + row_b (NULL: value only). The plane moments are split over (chunk, plane)
 * workgroups through `workspace` (ast_plane_stats_workspace_floats(planes, hw) floats; merged in
 * chunk order). */
int ast_style_moments_ws_f32(const float* x, const float* y, long long planes, long long hw, float weight,
                             const float* gscale, float* stats, float* loss, float* row_a, float* row_b,
                             float* workspace, long long workspace_floats, void* stream);

/* Gram part of compute_style_loss (losses.py:135-137): loss += weight * 10 * mean(huber(gx-gy)),
 * dgram = d/dgx (NULL: value only). */
int ast_gram_huber_f32(const float* gx, const float* gy, long long n, float weight, const float* gscale,
                       float* loss, float* dgram, void* stream);

/* tv_loss (losses.py:90-103): loss += weight * tv(x); dx (+)= d/dx. x [planes, h, w]. */
int ast_tv_loss_f32(const float* x, long long planes, int h, int w, float weight, const float* gscale,
                    float* loss, float* dx, int accumulate, void* stream);

/* Backward of mean_variance_norm (models.py:64-68) given the output gradient g. */
int ast_mvn_backward_f32(const float* x, const float* g, float* dx, long long planes, long long hw,
                         float eps, void* stream);

/* Backward of channel_stats / calc_mean_std: dx (+)= dmean/N + dstd*(x-mean)/((N-unbiased)*std);
 * dmean or dstd may be NULL. */
int ast_channel_stats_backward_f32(const float* x, const float* mean, const float* std,
                                   const float* dmean, const float* dstd, float* dx,
                                   long long planes, long long hw, int unbiased, int accumulate,
                                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer (train.py:287-300): clip_grad_norm_ + torch.optim.Adam over many tensors in two
 * launches. The caller builds a tensor table on the host (ast_optim_build_table, returns the
 * number of 64K-element chunks = workgroups), copies it to device memory once, and reuses it.
 * ------------------------------------------------------------------------------------------ */
size_t ast_optim_table_bytes(int ntensors);
long long ast_optim_build_table(void* host_table, int ntensors, float* const* params,
                                float* const* grads, float* const* exp_avg,
                                float* const* exp_avg_sq, const long long* numel);

/* state[0] = sqrt(sum of squared grads), state[1] = min(1, max_norm/(state[0]+1e-6))
 * (max_norm <= 0: coefficient 1). partial: nchunks floats of scratch. */
int ast_grad_norm_f32(const void* dev_table, int ntensors, long long nchunks, float* partial,
                      float max_norm, float* state, void* stream);

/* grads *= state[1] (the clip_grad_norm_ scaling alone). */
int ast_grad_scale_f32(const void* dev_table, int ntensors, long long nchunks, const float* state,
                       void* stream);

/* grads *= state[1] (if state) then one Adam step (step = 1-based count; lr, betas, eps as in
 * torch.optim.Adam, amsgrad off, no weight decay). */
int ast_adam_step_f32(const void* dev_table, int ntensors, long long nchunks, const float* state,
                      double lr, double beta1, double beta2, double eps, int step, void* stream);

/* The same step with its step count on the device (hipGraph replays): sched [4] floats =
 * [step count, skip flag, lr / bias_correction1, sqrt(bias_correction2)]; the call advances
 * sched[0] and computes the rest on the device. check_finite: a non-finite gradient norm state[0]
 * sets the skip flag and leaves parameters, moments, gradients and the step count unchanged (the
 * caller reads state[0] after the step and raises, as clip_grad_norm_(error_if_nonfinite)). */
int ast_adam_step_sched_f32(const void* dev_table, int ntensors, long long nchunks, const float* state,
                            double lr, double beta1, double beta2, double eps, float* sched, int check_finite,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * MobileNet-style variant (config 5). dtype / dtype_in / dtype_out: 0 = fp32,
 * 1 = bf16 storage (fp32 accumulate). All maps NCHW contiguous. BatchNorm (eval) is folded into
 * the weights by the caller.
 * ------------------------------------------------------------------------------------------ */

/* DepthWiseConv.forward (mobilenetv2.py:153-165) up to the SE pool: the expand 1x1 conv
 * (w1p != NULL: packed [round_up(hid,16)][cin_pad] in dtype, cin_pad a multiple of 16 (bf16) or 4
 * (fp32), zero padded; b1 [hid]) + Hardswish, then the depthwise k x k conv (k 3|5, stride 1|2,
 * reflect pad (k-1)/2; wdw [hid][k*k], bdw [hid]) + Hardswish, written to d [n][hid][ho][wo];
 * pool [n][hid] receives the per-plane sums of d (overwritten: each output tile's sums go to the
 * workspace, [n][hid][tile], and one ordered reduce makes pool). w1p == NULL is the ratio-1 form
 * (mobilenetv2.py:103-116): hid == cin, k == 3, and up == 2 applies DecoderBlock's nearest
 * Upsample (models.py:264-266) to x first. x2 != NULL feeds channels [c1, cin) from a second
 * tensor (the torch.cat before ada_out, models.py:335). workspace: the floats returned by
 * ast_mb_expand_dw_workspace_floats for the same arguments (has_x2 = x2 != NULL,
 * expand = w1p != NULL); <= 0 means the shape is unsupported. d == NULL is the pool-only pass
 * of the fused block pair (ast_mb_expand_dw_pw): pool is made, nothing else is written (bf16, k 3,
 * stride 1, expand blocks; AST_E_UNSUPPORTED elsewhere). */
long long ast_mb_expand_dw_workspace_floats(int dtype, int has_x2, int c1, int n, int cin, int h, int w, int up,
                                            int expand, int hid, int cin_pad, int k, int stride, int ho, int wo);
int ast_mb_expand_dw(int dtype, const void* x1, const void* x2, int c1, int n, int cin, int h, int w,
                     int up, const void* w1p, const float* b1, int hid, int cin_pad,
                     const float* wdw, const float* bdw, int k, int stride, void* d, float* pool,
                     int ho, int wo, float* workspace, long long workspace_floats, void* stream);

/* The fused block pair (DepthWiseConv.forward, mobilenetv2.py:153-165, without its hidden-width
 * tensor in memory): after ast_mb_expand_dw(d = NULL) made pool and ast_mb_se_fold made wg, this
 * recomputes the expand + depthwise of x and applies wg directly: out[n][co] = sum_c wg[n][co][c] *
 * D[n][c] + b2[co] (+ res[n][co]) in bf16, bit-identical to ast_mb_expand_dw + ast_mb_pw. Shapes:
 * ast_mb_expand_dw_pw_supported (1 = supported: bf16, k 3, stride 1, up 1, no x2, and the
 * (cin_pad, hid, cout) combinations instantiated). b2 and res may be NULL; hid_pad =
 * round_up(hid, 32), cout_pad = round_up(cout, 16). */
int ast_mb_expand_dw_pw_supported(int dtype, int has_x2, int cin, int cin_pad, int hid, int cout, int k,
                                  int stride, int up, int ho, int wo);
int ast_mb_expand_dw_pw(int dtype, const void* x, int n, int cin, int h, int w, const void* w1p,
                        const float* b1, int hid, int cin_pad, const float* wdw, const float* bdw, int k,
                        const void* wg, int cout, int cout_pad, int hid_pad, const float* b2,
                        const void* res, void* out, void* stream);

/* SELayer (mobilenetv2.py:63-81) on the pooled sums (mean = pool / hw), folded into the pw-linear
 * weights w2 [cout][hid]: wg[n][co][c] = w2[co][c] * gate[n][c], written as dtype
 * [n][cout_pad][hid_pad] with zero padding. fc1w [red][hid], fc2w [hid][red]. */
int ast_mb_se_fold(int dtype, const float* pool, int n, int hid, long long hw, const float* fc1w,
                   const float* fc1b, int red, const float* fc2w, const float* fc2b, const float* w2,
                   int cout, int cout_pad, int hid_pad, void* wg, void* stream);

/* pw-linear conv: out[n][co] = sum_c wg[n*wg_stride + co*hid_pad + c] * d[n][c] + bias[co]
 * (+ res[n][co], or res at (y/2, x/2) when res_up: the upsampled identity of models.py:266).
 * hid_pad a multiple of 32, cout_pad a multiple of 16 (16..128, except 112). bias may be NULL. */
int ast_mb_pw(int dtype, const void* d, int n, int hid, int hid_pad, int h, int w, const void* wg,
              long long wg_stride, const float* bias, int cout, int cout_pad, const void* res,
              int res_up, void* out, void* stream);

/* The expand half of DepthWiseConv (mobilenetv2.py:170-173) on its own, for blocks whose input is
 * too wide for the fused expand+depthwise kernels (AutoEncoder/AST ada_out, models.py:335: 256 ->
 * 768): out[n][co] = Hardswish(sum_c w1p[co][c] * cat(x1, x2)[n][c] + b1[co]) in bf16 (dtype 1),
 * [n][hid][h][w]. The depthwise then runs as the ratio-1 form of ast_mb_expand_dw on out.
 * cin_pad a multiple of 32, hid a multiple of 128; x2 != NULL feeds channels [c1, cin). */
int ast_mb_expand_gemm(int dtype, const void* x1, const void* x2, int c1, int n, int cin, int h, int w,
                       const void* w1p, const float* b1, int hid, int cin_pad, void* out, void* stream);

/* Eval-mode BatchNorm folded into the conv before it (mobilenetv2.py:223-231 _fold, the planned
 * inference path of DepthWiseConv; reference layers mobilenetv2.py:146-160): w is [cout][k],
 * s = gamma / sqrt(var + eps), w_out[r][c] = w[r][c] * s[r] for r < cout, c < k and 0 in the padding
 * of the [rows_out][ld] output; b_out[r] = beta[r] - mean[r] * s[r] (NULL: not written). has_bn 0:
 * a padded copy and a zero bias. Same roundings as the torch expression. */
int ast_mb_fold_bn_f32(const float* w, int cout, int k, const float* gamma, const float* beta, const float* mean,
                       const float* var, float eps, int has_bn, float* w_out, int ld, int rows_out, float* b_out,
                       void* stream);

/* Dense 3x3 reflect-pad convs of the variant: block 0 (conv_3x3_bn, mobilenetv2.py:38-43:
 * cin 3 -> cout 16, no bias, act 1 = Hardswish, fp32 input) and the decoder output conv
 * (models.py:300-316: cin 16 -> cout 3 + bias, fp32 output, act 2 = Hardtanh(0,1) when exporting,
 * act 0 otherwise). wt [cout][cin][3][3]. */
int ast_mb_conv3x3_dense(int dtype_in, int dtype_out, const void* x, const float* wt,
                         const float* bias, void* y, int n, int cin, int cout, int h, int w, int act,
                         void* stream);

/* AdaIN (as ast_adain_f32) on bf16 maps, fp32 statistics. */
int ast_adain_bf16(const void* content, const void* style, void* out, int n, int c, int hc, int wc,
                   int hs, int ws, double alpha, int swap_style_stats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * AdaAttN (models.py:70-115; SURVEY §8f "next" #1): attention-weighted style statistics.
 *   q = W_q(IN(content)), k = W_k(IN(style)), v = W_v(style)     (1x1 convs, no bias)
 *   A = softmax over style pixels of q^T k; mean = A v; std = sqrt(relu(A v^2 - mean^2))
 *   out = std * IN(content) + mean,   IN = InstanceNorm2d (biased var, eps 1e-5, no affine)
 * content [n][c][hc][wc], style [n][c][hs][ws], out like content (dtype 0 = fp32);
 * wq/wk/wv [c][c] fp32 (the Conv2d weights [c][c][1][1]). c <= 128.
 * workspace: device scratch of ast_adaattn_workspace_bytes() bytes (Q, K, V, statistics). */
/* ---------------------------------------------------------------------------------------------
 * AdaAttN backward stages (csrc/adaattn_bwd.hip; the GEMMs between them are ast_mbt_gemm_f32).
 * Notation per image: C channels, N content pixels, M style pixels; O = [mean | ex2] [N][2C].
 * ------------------------------------------------------------------------------------------ */
/* s[r][:] = softmax(s[r][:]) in place, rows x cols (nn.Softmax(dim=-1), models.py:97-99). */
int ast_softmax_rows_f32(float* s, long long rows, int cols, void* stream);
/* From O [n][N][2C], G = dL/dout [n][C][N] and IN(c) [n][C][N]: dO [n][N][2C] (d mean | d ex2 of
 * out = sqrt(relu(ex2 - mean^2)) IN(c) + mean, models.py:101-115), D[n*N] = rowsum(dO * O) and
 * optionally std [n][C][N]. */
int ast_adaattn_dstats_f32(const float* o2, const float* g, const float* chat, float* do2, float* drow,
                           float* std_out, int n, int c, int npix, void* stream);
/* dS = P * (dP - D[row]) in place in dp (softmax backward), rows x cols. */
int ast_softmax_backward_f32(const float* p, float* dp, const float* drow, long long rows, int cols,
                             void* stream);
/* vv [n][2][cm]: vv[b][1] = vv[b][0]^2 (the [V; V^2] operand). */
int ast_adaattn_square_f32(float* vv, int n, long long cm, void* stream);
/* dv [n][cm] = dvv[b][0] + 2 vv[b][0] * dvv[b][1]. */
int ast_adaattn_dv_f32(const float* dvv, const float* vv, float* dv, int n, long long cm, void* stream);
/* InstanceNorm2d backward (no affine) per plane, given the forward's mean / std = sqrt(var + eps)
 * (biased var): dx (=|+=) (dxh - mean(dxh) - xh mean(dxh xh)) / std. */
int ast_instance_norm_backward_f32(const float* x, const float* mean, const float* std, const float* dxh,
                                   float* dx, long long planes, long long hw, int accumulate, void* stream);
/* dst += a * b elementwise. */
int ast_fma_inplace_f32(float* dst, const float* a, const float* b, long long n, void* stream);
/* Flash-style AdaAttN backward (csrc/adaattn_flash.hip; replaces the materialised P / dS of the
 * calls above for large maps). q [n][C][N], k [n][C][M], vv [n][2C][M] ([V; V^2]) as above;
 * C a multiple of 16, at most 128, not 80 or 112 (ast_adaattn_flash_supported).
 * stats: o2 [n][N][2C] = softmax(Q^T K) [V; V^2]^T and lse2 [n][N] (log2-domain row log-sum-exp).
 * bwd_kv: dk [n][C][M] = Q dS, dvv [n][2C][M] = dO^T P, from do2 / drow of ast_adaattn_dstats_f32.
 * bwd_q: dq [n][C][N] = K dS^T. Deterministic (one lane sums each output in a fixed order). */
int ast_adaattn_flash_supported(int c);
int ast_adaattn_flash_stats_f32(const float* q, const float* k, const float* vv, float* o2, float* lse2, int n, int c,
                                int nq, int nk, void* stream);
int ast_adaattn_flash_bwd_kv_f32(const float* q, const float* k, const float* vv, const float* do2, const float* lse2,
                                 const float* drow, float* dk, float* dvv, int n, int c, int nq, int nk, void* stream);
int ast_adaattn_flash_bwd_q_f32(const float* q, const float* k, const float* vv, const float* do2, const float* lse2,
                                const float* drow, float* dq, int n, int c, int nq, int nk, void* stream);

size_t ast_adaattn_workspace_bytes(int dtype, int n, int c, int hc, int wc, int hs, int ws);
int ast_adaattn_fwd(int dtype, const void* content, const void* style, const float* wq,
                    const float* wk, const float* wv, void* out, void* workspace,
                    size_t workspace_bytes, int n, int c, int hc, int wc, int hs, int ws,
                    void* stream);
/* The attention launch ast_adaattn_fwd makes for these sizes (host only; the launcher takes its
 * launch from the same function, so this is the plan of the call, not a model of it).
 * waves: queries per workgroup / 32 (4 on the fp32 path; 4 or 8 for bf16). ksplit: parts the keys
 * are split into (1: no split, no merge kernel); kchunk: 32-key blocks per part. nqp / nkp: the
 * padded query / key counts of the workspace's Q and K, V. Returns the shape and dtype errors of
 * ast_adaattn_fwd; AST_E_NULLPTR for a null output pointer. */
int ast_adaattn_plan(int dtype, int n, int c, int hc, int wc, int hs, int ws, int* waves, int* ksplit,
                     int* kchunk, int* nqp, int* nkp);

/* ---------------------------------------------------------------------------------------------
 * Remaining train.py loss terms (SURVEY §8f "next" #2). Scalars are added into the loss
 * accumulator `loss` (AST_LOSS_ACC_FLOATS floats, zeroed once by the caller); gscale (device
 * scalar, may be NULL = 1) scales gradients.
 * ------------------------------------------------------------------------------------------ */

/* SingleDimHistLayer (losses.py:40-57): hist[b][k] = inv_norm * sum_i phi_k(x[b][i]) over the
 * m = C*H*W values of image b (m < 2^30), K = 256 bins, L = 1/256, W = L/2.5 (inv_norm = 1/(C*H):
 * the reference divides by x.size(1)*x.size(2)). hist [n][256] is overwritten. The bin sums are
 * exact 32.32 fixed-point integers (order-independent), kept in the workspace of
 * ast_soft_hist_workspace_floats(n) floats. */
long long ast_soft_hist_workspace_floats(int n);
int ast_soft_hist_f32(const float* x, int n, long long m, float inv_norm, float* hist, float* workspace,
                      long long workspace_floats, void* stream);

/* EarthMoversDistanceLoss (losses.py:8-22) of two histograms [n][256], mean over n
 * (compute_hist_loss, losses.py:84-87): *loss += weight * mean_b sum_t (cdf_x - cdf_y)^2;
 * ghist [n][256] (may be NULL) = gscale * d/dhx. */
int ast_emd_loss_f32(const float* hx, const float* hy, int n, float weight, const float* gscale,
                     float* loss, float* ghist, void* stream);

/* Backward of ast_soft_hist_f32: dx (+)= inv_norm * sum_k ghist[b][k] * dphi_k/dx. */
int ast_soft_hist_backward_f32(const float* x, int n, long long m, float inv_norm,
                               const float* ghist, float* dx, int accumulate, void* stream);

/* out_of_range_loss (train.py:259): *loss += weight * mean huber(x - clip(x, 0, 1)) (the clipped
 * copy is detached); dx (+)= its gradient. */
int ast_range_loss_f32(const float* x, long long numel, float weight, const float* gscale,
                       float* loss, float* dx, int accumulate, void* stream);

/* *loss += weight * mean((x - y)^2) (org_img_loss pixel term, train.py:268); dx (+)= d/dx. */
int ast_sqdiff_mean_f32(const float* x, const float* y, long long numel, float weight,
                        const float* gscale, float* loss, float* dx, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * On-device augmentation (SURVEY §8f "next" #3): the get_transform pipeline of data_loader.py:110-135
 * on [C][H][W] fp32 images (torchvision tensor semantics). Random parameters are drawn by the caller.
 * ------------------------------------------------------------------------------------------ */

/* transforms.ToTensor: uint8 [h][w][cs] (cs >= 3; RGB first) -> fp32 [3][h][w] / 255. */
int ast_aug_to_tensor(const unsigned char* src, int h, int w, int cs, float* dst, void* stream);

/* Integer-affine gather (torch.rot90 / hflip / vflip, data_loader.py:14-24, :115-116):
 * dst[c][y][x] = src[c][sy][sx], sy = coef[0]*y + coef[1]*x + coef[2], sx = coef[3]*y + coef[4]*x +
 * coef[5]; coef is a HOST array of 6 ints; every (y, x) must map inside src. */
int ast_aug_remap_f32(const float* src, int c, int hi, int wi, float* dst, int ho, int wo,
                      const int* coef, void* stream);

/* acc[0] = sum over pixels of rgb_to_grayscale(img) (adjust_contrast's mean * h*w); acc is a loss
 * accumulator (AST_LOSS_ACC_FLOATS floats, zeroed once by the caller; [0] is overwritten here). */
int ast_aug_gray_sum_f32(const float* img, int h, int w, float* acc, void* stream);

/* ColorJitter's adjustments and RandomGrayscale on a 3-channel image: op 0 brightness, 1 contrast
 * (gray_sum from ast_aug_gray_sum_f32), 2 saturation, 3 hue (factor in [-0.5, 0.5]), 4 grayscale. */
int ast_aug_color_f32(const float* src, int h, int w, int op, float factor, const float* gray_sum,
                      float* dst, void* stream);

/* Resize / RandomResizedCrop: the crop [y0, y0+crop_h) x [x0, x0+crop_w) of src resized to ho x wo
 * with antialiased bilinear weights (torch upsample aa, align_corners=False). tmp: device scratch
 * of ast_aug_resize_workspace_floats(c, crop_h, wo) floats. */
size_t ast_aug_resize_workspace_floats(int c, int crop_h, int wo);
int ast_aug_resize_f32(const float* src, int c, int h, int w, int y0, int x0, int crop_h, int crop_w,
                       float* dst, int ho, int wo, float* tmp, void* stream);

/* GaussianBlur: separable normalised taps (HOST array of k floats, k odd <= 15), reflect padding;
 * tmp: device scratch of c*h*w floats. */
int ast_aug_blur_f32(const float* src, int c, int h, int w, const float* taps, int k, float* dst,
                     float* tmp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MobileNet-variant training (SURVEY §8f "next" #4: AutoEncoder training, train_autoencoder.py),
 * fp32, composable kernels with their backward (csrc/mbtrain.hip).
 * ------------------------------------------------------------------------------------------ */

/* Side-by-side packing for small-plane zero-padded 3x3 convs (csrc/pack.hip; ops.conv3x3):
 * xp[ceil(n/G)][c][h][G*(w+gap)-gap] holds images x[0..n1) then x2[0..n2), G per row band,
 * `gap` zero columns between them; unpack reads image i at column (i%G)*sp of packed plane i/G. */
int ast_pack_images_f32(const float* x, int n1, const float* x2, int n2, int c, int h, int w, int G,
                        int gap, float* xp, void* stream);
int ast_unpack_images_f32(const float* yp, int n, int c, int h, int w, int G, int sp, int wp,
                          float* out, void* stream);

/* C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n] with element strides (1x1 convs and their grads).
 * ksplit > 1 splits K across workgroups, and sCb == 0 with batch > 1 shares C across the batch:
 * then every (image, K-split) tile goes to the workspace (ast_mbt_gemm_workspace_floats floats,
 * 0 when neither applies) and one ordered reduce writes / adds C.
 * foldN = P > 0 (batch 1, B n-contiguous): column n is pixel n % P of image n / P, reached through
 * the image strides sBb / sCb; foldK = P > 0 (batch 1, A and B k-contiguous): the same for K. */
long long ast_mbt_gemm_workspace_floats(int M, int N, int batch, int ksplit, long long sCb);
int ast_mbt_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int batch,
                     long long sAb, long long sAm, long long sAk, long long sBb, long long sBk,
                     long long sBn, long long sCb, long long sCm, long long sCn, int ksplit,
                     int accumulate, int foldK, int foldN, float* workspace, long long workspace_floats,
                     void* stream);

/* Depthwise k x k conv (k 3|5, stride 1|2, reflect pad (k-1)/2; mobilenetv2.py:148-149, :116-117),
 * LDS-tiled (csrc/mbt_dw.hip): mode 0 out = conv(x, w); 1 out = dx from g (overwritten, one pass,
 * no workspace); 2 out = dw [c][k*k] from x, g (overwritten; the workspace holds one partial row
 * per (channel, image, tile group), summed in that order). Mode 2 needs
 * ast_mbt_dw_workspace_floats floats of workspace (modes 0 and 1 ignore it). */
long long ast_mbt_dw_workspace_floats(int n, int c, int h, int wd, int k);
int ast_mbt_dw_f32(int mode, const float* x, const float* w, const float* g, float* out, int n,
                   int c, int h, int wd, int k, int s, float* workspace, long long workspace_floats,
                   void* stream);
/* The same with DepthWiseConv's Hardswish -> depthwise conv pair fused (mobilenetv2.py:144-149):
 * act 1 means the conv's input is hardswish(x) with x the stored pre-activation -- modes 0 and 2
 * apply it while staging x, mode 1 (x required then) returns the gradient w.r.t. x, taken on
 * through the Hardswish. Bit-identical to the materialised activation. act 0 = ast_mbt_dw_f32. */
int ast_mbt_dw_act_f32(int mode, const float* x, const float* w, const float* g, float* out, int n,
                       int c, int h, int wd, int k, int s, int act, float* workspace,
                       long long workspace_floats, void* stream);

/* BatchNorm2d in training mode (batch statistics, biased var + eps; running stats updated with
 * momentum and the unbiased variance when run_mean/run_var are given). mean/invstd [c] saved.
 * workspace: ast_mbt_bn_workspace_floats(n, c, hw) floats of per-segment partial statistics.
 * The composites below are stats -> merge(1 part) -> apply and bwd_sums -> bwd_apply; SyncBatchNorm
 * (data-parallel AutoEncoder training, dp.convert_sync_batchnorm) calls the stages itself with a
 * gather of the per-rank stats and an all-reduce of the backward sums in between. */
long long ast_mbt_bn_workspace_floats(int n, int c, long long hw);
int ast_mbt_bn_fwd_f32(const float* x, int n, int c, long long hw, const float* gamma,
                       const float* beta, float eps, float momentum, float* mean, float* invstd,
                       float* run_mean, float* run_var, float* y, float* workspace,
                       long long workspace_floats, void* stream);
int ast_mbt_bn_bwd_f32(const float* x, const float* dy, int n, int c, long long hw,
                       const float* mean, const float* invstd, const float* gamma, float* dgamma,
                       float* dbeta, float* dx, float* workspace, long long workspace_floats,
                       void* stream);
/* this process's per-channel (count, mean, M2) as double [c][3] */
int ast_mbt_bn_stats_f32(const float* x, int n, int c, long long hw, float* workspace,
                         long long workspace_floats, double* stats, void* stream);
/* merge [parts][c][3] stats (Chan) -> mean, invstd, running stats (nullable), 1/count [1] (nullable) */
int ast_mbt_bn_merge_f32(const double* stats, int parts, int c, float eps, float momentum, float* mean,
                         float* invstd, float* run_mean, float* run_var, float* inv_count, void* stream);
int ast_mbt_bn_apply_f32(const float* x, int n, int c, long long hw, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, float* y,
                         void* stream);
/* sums [2][c]: sum(dy), sum(dy * xhat) over this process's images */
int ast_mbt_bn_bwd_sums_f32(const float* x, const float* dy, int n, int c, long long hw,
                            const float* mean, const float* invstd, float* workspace,
                            long long workspace_floats, float* sums, void* stream);
/* dx from (all-reduced) sums and the device 1/count written by ast_mbt_bn_merge_f32 */
int ast_mbt_bn_bwd_apply_f32(const float* x, const float* dy, int n, int c, long long hw,
                             const float* mean, const float* invstd, const float* gamma,
                             const float* sums, const float* inv_count, float* dx, void* stream);

/* The same stages with DepthWiseConv's BatchNorm2d -> Hardswish pair (mobilenetv2.py:122-126,
 * :150-153) fused: act 1 makes y = hardswish(BN(x)) in the apply pass, and the backward takes dy as
 * the gradient of that output (through the Hardswish at the recomputed BN output, bit-identical to
 * the forward's); act 0 is plain BatchNorm (the entries above are these with act 0). beta is needed
 * by the backward only when act is 1. */
int ast_mbt_bn_act_fwd_f32(const float* x, int n, int c, long long hw, const float* gamma,
                           const float* beta, float eps, float momentum, float* mean, float* invstd,
                           float* run_mean, float* run_var, int act, float* y, float* workspace,
                           long long workspace_floats, void* stream);
int ast_mbt_bn_act_apply_f32(const float* x, int n, int c, long long hw, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, int act, float* y,
                             void* stream);
int ast_mbt_bn_act_bwd_f32(const float* x, const float* dy, int n, int c, long long hw,
                           const float* mean, const float* invstd, const float* gamma, const float* beta,
                           int act, float* dgamma, float* dbeta, float* dx, float* workspace,
                           long long workspace_floats, void* stream);
int ast_mbt_bn_act_bwd_sums_f32(const float* x, const float* dy, int n, int c, long long hw,
                                const float* mean, const float* invstd, const float* gamma,
                                const float* beta, int act, float* workspace, long long workspace_floats,
                                float* sums, void* stream);
int ast_mbt_bn_act_bwd_apply_f32(const float* x, const float* dy, int n, int c, long long hw,
                                 const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, int act, const float* sums, const float* inv_count,
                                 float* dx, void* stream);

/* op 0 y = hardswish(a); 1 y = hardswish'(a) * b; 2 y = a + b; 3 y = nearest-upsample x2 of a
 * (n planes of h x w); 4 its backward (a = grad of the 2h x 2w planes). */
int ast_mbt_eltwise_f32(int op, const float* a, const float* b, float* y, long long n, int h,
                        int w, void* stream);

/* op 0 out[p] = mean(x[p]) (AdaptiveAvgPool2d(1)); 1 out[p] = sum(x[p] * y[p]);
 * 2 out = x * gate[p] (+ gadd[p]) over planes of hw elements. */
int ast_mbt_plane_f32(int op, const float* x, const float* y, const float* gate, const float* gadd,
                      float* out, long long planes, long long hw, void* stream);
/* ops 0-2 as above, plus the Hardswish -> SELayer pair over the stored pre-activation
 * (mobilenetv2.py:151-156): 3 out[p] = mean(hardswish(x[p])); 4 out[p] = sum(x[p] * hardswish(y[p]));
 * 5 out = hardswish(x) * gate[p]; 6 out = hardswish'(a) * (x * gate[p] + gadd[p]) (a: the
 * pre-activation). Bit-identical to the materialised activation. */
int ast_mbt_plane_act_f32(int op, const float* x, const float* y, const float* gate, const float* gadd,
                          const float* a, float* out, long long planes, long long hw, void* stream);

/* SELayer MLP (mobilenetv2.py:63-81): hid = relu(W1 pool + b1), z = W2 hid + b2, gate = clamp(z,0,1);
 * backward from dgate: parameter gradients (overwritten, summed over images in image order) and
 * dpool / hw; workspace n * (c + red) floats (the per-image dz, dh). */
int ast_mbt_se_fc_fwd_f32(const float* pool, const float* w1, const float* b1, const float* w2,
                          const float* b2, int n, int c, int red, float* hid, float* z, float* gate,
                          void* stream);
int ast_mbt_se_fc_bwd_f32(const float* dgate, const float* z, const float* hid, const float* pool,
                          const float* w1, const float* w2, int n, int c, int red, long long hw,
                          float* dw1, float* db1, float* dw2, float* db2, float* dpool, float* workspace,
                          long long workspace_floats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Colour spaces (model_util.py:11-140) on NCHW images with 3 channels: x, out [n][3][hw].
 * mode: one AST_COLOR_* below. RGB2LAB and LAB2RGB include the reference's (lab/100 + 1)/2 and
 * (x*2 - 1)*100 normalisation (model_util.py:117-140). The reference's constants and matrices
 * (0.412453..., white point 0.95047, 1, 1.08883) and its NaN set: rgb below -0.055 and negative
 * xyz components give NaN, lab2xyz / xyz2rgb clamp and stay finite. fp32 arithmetic throughout;
 * _bf16_f32 reads bf16 and writes fp32 (what the reference returns), _bf16 writes bf16.
 * backward: grad_in = J^T grad_out at x, the selected branch's derivative (zero where a clamp is
 * active), finite where the reference's autograd is NaN through its unselected branch.
 * AST_E_SHAPE for n <= 0, hw <= 0 or an unknown mode. */
enum {
  AST_COLOR_RGB2XYZ = 0,
  AST_COLOR_XYZ2RGB = 1,
  AST_COLOR_XYZ2LAB = 2,
  AST_COLOR_LAB2XYZ = 3,
  AST_COLOR_RGB2LAB = 4,
  AST_COLOR_LAB2RGB = 5
};
int ast_color_convert_f32(const float* x, float* out, int n, long long hw, int mode, void* stream);
int ast_color_convert_bf16_f32(const void* x, float* out, int n, long long hw, int mode, void* stream);
int ast_color_convert_bf16(const void* x, void* out, int n, long long hw, int mode, void* stream);
int ast_color_convert_backward_f32(const float* x, const float* grad_out, float* grad_in, int n,
                                   long long hw, int mode, void* stream);

/* Colour-preserving recombination, one launch: out = lab2rgb(cat(L of rgb2lab(clamp01(stylised)),
 * ab of rgb2lab(clamp01(content)))), the stylised luminance with the content's chroma.
 * stylised, content, out [n][3][hw], all fp32 or all bf16. */
int ast_luma_transfer_f32(const float* stylised, const float* content, float* out, int n, long long hw,
                          void* stream);
int ast_luma_transfer_bf16(const void* stylised, const void* content, void* out, int n, long long hw,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Moment-matching style loss (the l_m of Kolkin et al., STROTSS, CVPR 2019, its `moment_loss`;
 * csrc/moment.hip; an extension, no reference counterpart): L1 distance between the channel means and
 * between the channel covariances of two maps, with a backward to the first. tests/moment_ref.py
 * restates the definition.
 * Inputs, fp32 dense NCHW with the spatial sides flattened: x [n, c, m], the differentiable side, and
 * the target y [ns, c, p], ns == n or ns == 1 (one style shared by the batch), of any size p; the loss
 * sees y only through its statistics. Limits: c in 1..AST_MOMENT_MAX_C, m and p in 2..2^31 - 1,
 * n <= 32767.
 * Statistics, per sample: mu = the mean over the pixels, computed as x_0 + sum(x - x_0) / m (exact for a
 * constant plane); Cov = (X - mu)(X - mu)^T / (m - 1), with no ridge, the products summed on the fp32
 * matrix cores over the upper-triangle 64x64 tiles, split along the pixels, the splits added in split
 * order; Cov is symmetric in bits. `splits`: 0 = the library's choice, else that many (clamped so that
 * every split has pixels; a test hook: the result depends on it only by rounding).
 * Loss: L_b = (1 / c) sum_i |mu_x - mu_y|_i + (1 / c^2) sum_ij |Cov_x - Cov_y|_ij; sums[b] = L_b;
 * *loss += weight / n * sum_b L_b, the samples in a fixed order. loss is a loss accumulator
 * (AST_LOSS_ACC_FLOATS floats, above). Cov_x is never stored.
 * Signs: sign_mu [n, c] = sign(mu_x - mu_y) and sign_cov [n, c, c] = sign(Cov_x - Cov_y), int8 with
 * values +1, -1 and 0 for a difference that is zero or NaN; sign_cov is computed on the upper-triangle
 * tiles and mirrored, so it is symmetric in bits.
 * Backward, to x only (the target is data). With g = *gscale (a device scalar; NULL: 1):
 *   dx[b, i, k] (+)= g weight / n (sign_mu[i] / (c m)
 *                                  + 2 / (c^2 (m - 1)) sum_j sign_cov[i, j] (x[j, k] - mu_x[j]))
 * one GEMM per sample, j ascending in pairs (the MFMA's order); the centring projection of the
 * covariance drops out because the rows of X - mu sum to zero. accumulate != 0 adds into dx, else every
 * element of dx is written.
 * Non-finite values: a NaN or infinity in sample b of x makes mu_x, Cov entries, sums[b] and hence
 * *loss non-finite; a NaN difference has sign 0, an infinite one its sign; dx of sample b is what the
 * GEMM gives on those values. Every other sample's sums, signs and dx are unchanged in bits: a sample
 * is a grid index in every launch.
 * No floating-point atomics, no host synchronisation, no allocation. Workspaces are device memory,
 * 256-byte aligned, of at least the matching *_workspace_bytes query: the partial tiles,
 * 4 n splits pairs 64^2 bytes with pairs = t (t + 1) / 2, t = ceil(c / 64), and for the loss one
 * partial sum per sample and tile pair, each rounded up to 256.
 * AST_E_NULLPTR: a null pointer (gscale may be null). AST_E_SHAPE: a size out of the limits above, ns
 * outside {1, n}, a short workspace. AST_E_UNSUPPORTED: c > AST_MOMENT_MAX_C, splits < 0. The queries
 * return the same negative codes. All checks run before the first launch. */
#define AST_MOMENT_MAX_C 1024

/* mean [n, c] and cov [n, c, c] of y [n, c, m]; three launches. */
long long ast_moment_stats_workspace_bytes(int n, int c, long long m, int splits);
int ast_moment_stats_f32(const float* y, float* mean, float* cov, int n, int c, long long m, int splits,
                         void* workspace, long long workspace_bytes, void* stream);

/* The forward from x and the target's statistics y_mean [ns, c], y_cov [ns, c, c]; five launches.
 * mean_x [n, c], sign_mu and sign_cov are what the backward reads. */
long long ast_moment_loss_workspace_bytes(int n, int c, long long m, int splits);
int ast_moment_loss_f32(const float* x, const float* y_mean, const float* y_cov, float* mean_x,
                        signed char* sign_mu, signed char* sign_cov, float* sums, float* loss, int n, int ns,
                        int c, long long m, float weight, int splits, void* workspace,
                        long long workspace_bytes, void* stream);

/* dx [n, c, m] from the forward's state; one launch, 2 c^2 m FLOP per sample, no workspace. */
int ast_moment_loss_backward_f32(const float* x, const float* mean_x, const signed char* sign_mu,
                                 const signed char* sign_cov, const float* gscale, float* dx, int n, int c,
                                 long long m, float weight, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bilinear resize of fp32 planes and its adjoint (csrc/pyramid.hip): x [planes][h][w] ->
 * out [planes][H][W], every side in 1..4096, any ratio. The filter is
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False):
 *   scale = (float)in / out;  s = max(scale * (o + 0.5) - 0.5, 0);  i0 = min((int)s, in - 1);
 *   i1 = min(i0 + 1, in - 1);  l1 = s - i0;  value = (1 - l1) * x[i0] + l1 * x[i1]   per axis
 * (not the antialiased filter of ast_aug_resize_f32). With `add` [planes][H][W] non-null,
 * out = add + add_sign * resize(x); out must not alias add or x. This one launch is a level of the
 * Laplacian pyramid both ways: lap = cur - resize(down(cur)) (add_sign -1) and
 * cur = lap + resize(cur) (add_sign +1).
 * The adjoint is the transpose: dx [planes][h][w] = R^T g for g [planes][H][W] (accumulate != 0:
 * dx += R^T g). One thread owns a source pixel and sums, in ascending (oy, ox) order, the outputs
 * that have a non-zero weight on it, so two runs agree in bits; a non-finite g reaches only those
 * source pixels (PyTorch's autograd also adds 0 * g to a cell's second pixel when l1 = 0). A source pixel feeding k outputs costs k serial steps (fine for the pyramid's
 * factor 2; 1 -> 4096 per side is 16M steps in one thread).
 * No workspace, no atomics, no host synchronisation. AST_E_SHAPE for planes <= 0 or a side outside
 * 1..4096. */
int ast_resize_bilinear_f32(const float* x, float* out, int planes, int h, int w, int H, int W,
                            const float* add, float add_sign, void* stream);
int ast_resize_bilinear_adjoint_f32(const float* g, float* dx, int planes, int h, int w, int H, int W,
                                    int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AST_HIP_H */
