"""torch.ops.ast_hip.*: the hot-path ops as PyTorch custom operators -- the path the drop-in
modules (models.py, mobilenetv2.py) and losses.py call ("What the C++ side
exports").

Every op launches the same C-ABI kernels of libast_hip.so as the ctypes helpers in ops.py /
functional.py (its implementation IS those helpers), on PyTorch's current HIP stream. Each op has
a fake (meta) implementation, so torch.compile / FakeTensor tracing sees shapes without running
kernels -- `torch.compile(models.AdaINStyleTransfer(), fullgraph=True)` traces the forward with no
graph break -- and the differentiable ones carry their backward formula
(torch.library.register_autograd), whose kernels are the HIP backward kernels (conv dgrad / wgrad,
AdaIN backward, the fused loss gradients). A backward is written once: conv3x3 and adain_map call the
bodies they share with the eager Function classes (functional.encoder_conv_backward,
decoder_conv_backward, adain_backward); the loss formulas below are the only copy, there being no
Function class for a loss. The native C++ registration (csrc/torch_ops.cpp,
libast_torch_ops.so: adain, channel_stats, conv3x3_pack, conv3x3_fwd, gram) shares the namespace;
gram gets its autograd formula here.

Op                      reference (file:line)                       autograd
conv3x3                 models.py:199-240 (encoder), :598-628 (decoder)   dx, dW, db
adain_map               models.py:43-51 (+ alpha blend :471)         d content, d style (fp32)
gram (C++)              losses.py:105-109                            d feat
content_mvn_loss        losses.py:124-126 on mean_variance_norm      d x
style_loss              losses.py:128-139                            d x
huber_loss              losses.py:124-126 (compute_content_loss)     d x, d y
tv_loss                 losses.py:90-103                             d img
hist_loss               losses.py:84-87 (SingleDimHist + EMD)        d x
remd_loss               -- (relaxed EMD: two-way cosine match)       d x
selfsim_loss            -- (self-similarity of pixel-pair distances) d x
cx_loss                 -- (contextual loss: softmax over a cosine match) d x
moment_loss             -- (STROTSS moment matching: L1 of mean and covariance) d x
range_loss              train.py:259                                 d x
sqdiff_mean             train.py:268                                 d x
mb_expand_dw            mobilenetv2.py:153-161 (to the SE pool)      -- (eval BN folded: inference)
mb_se_fold              mobilenetv2.py:63-81 folded into the pw conv --
mb_pw                   mobilenetv2.py:162-165                       --
mb_expand_gemm          models.py:335 (ada_out expand half)          --
mb_conv3x3_dense        mobilenetv2.py:38-43, models.py:300-316      --
color_convert           model_util.py:11-140 (six conversions)       d x
luma_transfer           -- (colour-preserving recombination)         --
resize_bilinear         F.interpolate(bilinear, align_corners=False) (+ add)   d x (the adjoint kernel), d add
resize_labels           -- (nearest resize of uint8 label maps)      --
region_stats            -- (masked per-region channel statistics)    --
adain_regions           -- (regional multi-style AdaIN)              --
efdm                    -- (exact feature distribution matching)     d content = grad (straight-through)
plane_sort              -- (segmented totalOrder sort of planes)     --
efdm_regions            -- (EFDM per region, mix of a style bank)    raises NotImplementedError
wct                     -- (whitening and colouring transform)       raises NotImplementedError
wct_regions             -- (WCT per region, mix of a style bank)     raises NotImplementedError
style_swap              -- (patch-matching style swap)               raises NotImplementedError
style_swap_guided       -- (class-guided style swap over a bank)     raises NotImplementedError
kmeans                  -- (feature k-means: centroids, labels, counts)   raises NotImplementedError
kmeans_assign           -- (nearest centroid per pixel, uint8 labels)     raises NotImplementedError
label_mode_filter       -- (3x3 majority vote over uint8 label maps)      --
The MobileNet inference ops fold eval-mode BatchNorm; training runs the composable kernels of
mbtrain.py (their own autograd), as the drop-in DepthWiseConv does.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op, register_autograd, register_fake

from . import functional as Fn
from . import ops, torch_ops
from ._lib import check, lib, loss_accumulator, ptr, stream_ptr, workspace

torch_ops.load()   # the native registrations (and libast_hip.so) first: no fallback

PADS = ("zeros", "reflect")


def _empty(like: Tensor) -> Tensor:
    return like.new_empty((0,))


# ------------------------------------------------------------------------------------------------
# conv3x3: [Upsample x2] -> pad(1) -> Conv3x3 -> (+bias) -> {pre, ReLU, ReLU + MaxPool2x2}
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::conv3x3", mutates_args=())
def conv3x3(x: Tensor, weight: Tensor, w_packed: Tensor, bias: Optional[Tensor], upsample: int, pad_mode: int,
            in_mean: Optional[Tensor], in_std: Optional[Tensor], want_pre: bool, want_act: bool, want_pool: bool,
            x2: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """Outputs (pre, act, pool); unrequested ones are empty. `weight` [cout, cin, 3, 3] is the
    unpacked filter (the backward's dW and transposed pack come from it); `w_packed` its pack."""
    pre, act, pool = ops.conv3x3(x, w_packed, bias, int(weight.shape[0]), upsample=upsample,
                                 pad_mode=PADS[pad_mode], in_mean=in_mean, in_std=in_std, want_pre=want_pre,
                                 want_act=want_act, want_pool=want_pool, x2=x2)
    return (pre if pre is not None else _empty(x), act if act is not None else _empty(x),
            pool if pool is not None else _empty(x))


@register_fake("ast_hip::conv3x3")
def _(x, weight, w_packed, bias, upsample, pad_mode, in_mean, in_std, want_pre, want_act, want_pool, x2):
    n = x.shape[0] + (x2.shape[0] if x2 is not None else 0)
    cout, H, W = weight.shape[0], x.shape[2] * upsample, x.shape[3] * upsample
    mk = lambda want, h, w: x.new_empty((n, cout, h, w)) if want else x.new_empty((0,))  # noqa: E731
    return mk(want_pre, H, W), mk(want_act, H, W), mk(want_pool, H // 2, W // 2)


def _conv_setup(ctx, inputs, output):
    x, weight, w_packed, bias, upsample, pad_mode, in_mean, in_std, want_pre, want_act, want_pool, x2 = inputs
    if x2 is not None:
        raise NotImplementedError("ast_hip::conv3x3: the two-batch form (x2) has no backward; call it per batch")
    pre, act, _ = output
    if pad_mode == 0 and not want_pre:
        raise NotImplementedError("ast_hip::conv3x3 (zero padding) under autograd needs want_pre=True "
                                  "(the ReLU / max-pool backward reads the pre-activation)")
    if pad_mode == 1 and want_pool:
        raise NotImplementedError("ast_hip::conv3x3 (reflect padding) under autograd: no max-pool backward")
    mask = pre if pad_mode == 0 else (act if want_act else None)
    ctx.save_for_backward(x, weight, mask, in_mean, in_std)
    ctx.cfg = (upsample, pad_mode, bias is not None, want_act)


def _conv_backward(ctx, g_pre, g_act, g_pool):
    x, weight, mask, mean, std = ctx.saved_tensors
    upsample, pad_mode, has_bias, want_act = ctx.cfg
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[3])
    if pad_mode == 0:   # the encoder layer; mask = pre
        dx, dw, db = Fn.encoder_conv_backward(x, weight, mask, mean, std, g_pre, g_act, g_pool, need_x, need_w,
                                              has_bias)
    else:               # the decoder layer; mask = the ReLU output (None without ReLU)
        dx, dw, db = Fn.decoder_conv_backward(x, weight, g_act if want_act else g_pre, mask, upsample, need_x,
                                              need_w, has_bias)
    return dx, dw, None, db, None, None, None, None, None, None, None, None


register_autograd("ast_hip::conv3x3", _conv_backward, setup_context=_conv_setup)


# ------------------------------------------------------------------------------------------------
# AdaIN (+ alpha blend)
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::adain_map", mutates_args=())
def adain_map(content: Tensor, style: Tensor, alpha: float, swap_style_stats: bool) -> Tensor:
    return ops.adain(content, style, alpha=alpha, swap_style_stats=swap_style_stats)


@register_fake("ast_hip::adain_map")
def _(content, style, alpha, swap_style_stats):
    return torch.empty_like(content)


def _adain_setup(ctx, inputs, output):
    content, style, alpha, swap = inputs
    if content.dtype != torch.float32:
        raise NotImplementedError("ast_hip::adain_map backward runs in float32")
    ctx.save_for_backward(content, style)
    ctx.alpha, ctx.swap = alpha, swap


def _adain_backward(ctx, g):
    content, style = ctx.saved_tensors
    return Fn.adain_backward(content, style, g, ctx.alpha, ctx.swap, *ctx.needs_input_grad[:2]) + (None, None)


register_autograd("ast_hip::adain_map", _adain_backward, setup_context=_adain_setup)


# ------------------------------------------------------------------------------------------------
# gram (native registration) + its backward
# ------------------------------------------------------------------------------------------------

def _gram_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _gram_backward(ctx, dg):
    (f,) = ctx.saved_tensors
    b, c, h, w = f.shape
    df = torch.empty_like(f)
    check(lib().ast_gram_backward_f32(ptr(f), ptr(dg.contiguous()), ptr(df), None, None, b, c, h * w,
                                      1.0 / (c * h * w), None, 0, stream_ptr(f.device)), "gram_backward")
    return df


register_autograd("ast_hip::gram", _gram_backward, setup_context=_gram_setup)


# ------------------------------------------------------------------------------------------------
# Losses: value ops with the gradient state as extra (non-differentiable) outputs
# ------------------------------------------------------------------------------------------------

def _acc(like):
    return loss_accumulator(like.device, pooled=False)   # custom-op outputs: storage of their own


@custom_op("ast_hip::content_mvn_loss", mutates_args=())
def content_mvn_loss(x: Tensor, y: Tensor, weight: float, want_grad: bool) -> Tuple[Tensor, Tensor]:
    """weight * compute_content_loss(mean_variance_norm(x), mean_variance_norm(y)); second output:
    the per-plane statistics of the backward (empty unless want_grad)."""
    n, c = x.shape[:2]
    acc = _acc(x)
    pstats = torch.empty((n * c, 6), device=x.device) if want_grad else _empty(x)
    Fn.mvn_huber(x, y, weight, acc, pstats if want_grad else None)
    return acc[0], pstats


@register_fake("ast_hip::content_mvn_loss")
def _(x, y, weight, want_grad):
    return x.new_empty(()), x.new_empty((x.shape[0] * x.shape[1], 6) if want_grad else (0,))


def _mvn_setup(ctx, inputs, output):
    x, y, weight, want_grad = inputs
    if not want_grad:
        raise NotImplementedError("ast_hip::content_mvn_loss under autograd needs want_grad=True")
    ctx.save_for_backward(x, y, output[1])
    ctx.weight = weight


def _mvn_backward(ctx, g, _):
    x, y, pstats = ctx.saved_tensors
    n, c = x.shape[:2]
    dx = torch.empty_like(x)
    check(lib().ast_mvn_huber_backward_f32(ptr(x), ptr(y), ptr(pstats), n * c, x[0, 0].numel(), ctx.weight,
                                           ptr(g.contiguous()), ptr(dx), 0, stream_ptr(x.device)), "mvn_huber_backward")
    return dx, None, None, None


register_autograd("ast_hip::content_mvn_loss", _mvn_backward, setup_context=_mvn_setup)


@custom_op("ast_hip::style_loss", mutates_args=())
def style_loss(x: Tensor, y: Tensor, weight: float, want_grad: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """weight * compute_style_loss(x, y); extra outputs: dG, row_a, row_b of the gradient."""
    acc = _acc(x)
    dg, ra, rb = Fn._style_terms(x, y, weight, acc, want_grad=want_grad)
    e = lambda: _empty(x)  # noqa: E731
    return acc[0], dg if dg is not None else e(), ra if ra is not None else e(), rb if rb is not None else e()


@register_fake("ast_hip::style_loss")
def _(x, y, weight, want_grad):
    b, c = x.shape[:2]
    if want_grad:
        return x.new_empty(()), x.new_empty((b, c, c)), x.new_empty((b * c,)), x.new_empty((b * c,))
    return x.new_empty(()), x.new_empty((0,)), x.new_empty((0,)), x.new_empty((0,))


def _style_setup(ctx, inputs, output):
    x, y, weight, want_grad = inputs
    if not want_grad:
        raise NotImplementedError("ast_hip::style_loss under autograd needs want_grad=True")
    ctx.save_for_backward(x, output[1], output[2], output[3])


def _style_backward(ctx, g, *_):
    x, dg, ra, rb = ctx.saved_tensors
    b, c, h, w = x.shape
    dx = torch.empty_like(x)
    check(lib().ast_gram_backward_f32(ptr(x), ptr(dg), ptr(dx), ptr(ra), ptr(rb), b, c, h * w, 1.0 / (c * h * w),
                                      ptr(g.contiguous()), 0, stream_ptr(x.device)), "gram_backward")
    return dx, None, None, None


register_autograd("ast_hip::style_loss", _style_backward, setup_context=_style_setup)


@custom_op("ast_hip::content_style_loss", mutates_args=())
def content_style_loss(x: Tensor, yc: Tensor, ys: Tensor, wc: float, ws: float,
                       want_grad: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(wc * content_mvn_loss(x, yc), ws * compute_style_loss(x, ys)) of ONE feature map x (the
    trainers apply both to every loss tap, train.py:217-245): the backward writes dx once -- the
    Gram-backward GEMM, then the content gradient added in place (the same fp32 sum autograd's add
    of the two gradients made, one read-modify-write of dx fewer). Extra outputs: the backward's
    state (pstats, dG, row_a, row_b; empty unless want_grad)."""
    n, c = x.shape[:2]
    acc_c, acc_s = _acc(x), _acc(x)
    pstats = torch.empty((n * c, 6), device=x.device) if want_grad else None
    Fn.mvn_huber(x, yc, wc, acc_c, pstats)
    dg, ra, rb = Fn._style_terms(x, ys, ws, acc_s, want_grad=want_grad)
    e = lambda t: t if t is not None else _empty(x)  # noqa: E731
    return acc_c[0], acc_s[0], e(pstats), e(dg), e(ra), e(rb)


@register_fake("ast_hip::content_style_loss")
def _(x, yc, ys, wc, ws, want_grad):
    b, c = x.shape[:2]
    if want_grad:
        return (x.new_empty(()), x.new_empty(()), x.new_empty((b * c, 6)), x.new_empty((b, c, c)),
                x.new_empty((b * c,)), x.new_empty((b * c,)))
    return (x.new_empty(()), x.new_empty(()), x.new_empty((0,)), x.new_empty((0,)), x.new_empty((0,)),
            x.new_empty((0,)))


def _cs_setup(ctx, inputs, output):
    x, yc, ys, wc, ws, want_grad = inputs
    if not want_grad:
        raise NotImplementedError("ast_hip::content_style_loss under autograd needs want_grad=True")
    ctx.save_for_backward(x, yc, output[2], output[3], output[4], output[5])
    ctx.wc = wc


def _cs_backward(ctx, gc, gs, *_):
    x, yc, pstats, dg, ra, rb = ctx.saved_tensors
    b, c, h, w = x.shape
    st = stream_ptr(x.device)
    dx = torch.empty_like(x)
    first = True
    if gs is not None:
        check(lib().ast_gram_backward_f32(ptr(x), ptr(dg), ptr(dx), ptr(ra), ptr(rb), b, c, h * w, 1.0 / (c * h * w),
                                          ptr(gs.contiguous()), 0, st), "gram_backward")
        first = False
    if gc is not None:
        check(lib().ast_mvn_huber_backward_f32(ptr(x), ptr(yc), ptr(pstats), b * c, h * w, ctx.wc,
                                               ptr(gc.contiguous()), ptr(dx), 0 if first else 1, st),
              "mvn_huber_backward")
        first = False
    if first:
        dx.zero_()
    return dx, None, None, None, None, None


register_autograd("ast_hip::content_style_loss", _cs_backward, setup_context=_cs_setup)


@custom_op("ast_hip::huber_loss", mutates_args=())
def huber_loss(x: Tensor, y: Tensor) -> Tensor:
    acc = _acc(x)
    check(lib().ast_huber_f32(ptr(x), ptr(y), x.numel(), 1.0, None, ptr(acc), None, 0, stream_ptr(x.device)), "huber")
    return acc[0]


@register_fake("ast_hip::huber_loss")
def _(x, y):
    return x.new_empty(())


def _huber_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _huber_backward(ctx, g):
    x, y = ctx.saved_tensors
    g = g.contiguous()
    dx = dy = None
    if ctx.needs_input_grad[0]:
        dx = torch.empty_like(x)
        check(lib().ast_huber_f32(ptr(x), ptr(y), x.numel(), 1.0, ptr(g), None, ptr(dx), 0, stream_ptr(x.device)),
              "huber")
    if ctx.needs_input_grad[1]:
        dy = torch.empty_like(y)
        check(lib().ast_huber_f32(ptr(y), ptr(x), y.numel(), 1.0, ptr(g), None, ptr(dy), 0, stream_ptr(y.device)),
              "huber")
    return dx, dy


register_autograd("ast_hip::huber_loss", _huber_backward, setup_context=_huber_setup)


@custom_op("ast_hip::tv_loss", mutates_args=())
def tv_loss(img: Tensor) -> Tensor:
    n, c, h, w = img.shape
    acc = _acc(img)
    check(lib().ast_tv_loss_f32(ptr(img), n * c, h, w, 1.0, None, ptr(acc), None, 0, stream_ptr(img.device)),
          "tv_loss")
    return acc[0]


@register_fake("ast_hip::tv_loss")
def _(img):
    return img.new_empty(())


def _tv_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])


def _tv_backward(ctx, g):
    (img,) = ctx.saved_tensors
    n, c, h, w = img.shape
    dx = torch.empty_like(img)
    check(lib().ast_tv_loss_f32(ptr(img), n * c, h, w, 1.0, ptr(g.contiguous()), None, ptr(dx), 0,
                                stream_ptr(img.device)), "tv_loss")
    return dx


register_autograd("ast_hip::tv_loss", _tv_backward, setup_context=_tv_setup)


@custom_op("ast_hip::hist_loss", mutates_args=())
def hist_loss(x: Tensor, y: Tensor, weight: float) -> Tuple[Tensor, Tensor, Tensor]:
    """weight * compute_hist_loss(x, y); extra outputs: the two soft histograms."""
    hx, hy = Fn.soft_histogram(x), Fn.soft_histogram(y)
    acc = _acc(x)
    check(lib().ast_emd_loss_f32(ptr(hx), ptr(hy), x.shape[0], float(weight), None, ptr(acc), None,
                                 stream_ptr(x.device)), "emd_loss")
    return acc[0], hx, hy


@register_fake("ast_hip::hist_loss")
def _(x, y, weight):
    return x.new_empty(()), x.new_empty((x.shape[0], Fn.HIST_BINS)), x.new_empty((y.shape[0], Fn.HIST_BINS))


def _hist_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output[1], output[2])
    ctx.weight = float(inputs[2])


def _hist_backward(ctx, g, *_):
    x, hx, hy = ctx.saved_tensors
    b = x.shape[0]
    ghist = torch.empty_like(hx)
    check(lib().ast_emd_loss_f32(ptr(hx), ptr(hy), b, ctx.weight, ptr(g.contiguous()), None, ptr(ghist),
                                 stream_ptr(x.device)), "emd_loss")
    dx = torch.empty_like(x)
    check(lib().ast_soft_hist_backward_f32(ptr(x), b, x.numel() // b, 1.0 / (x.shape[1] * x.shape[2]), ptr(ghist),
                                           ptr(dx), 0, stream_ptr(x.device)), "soft_hist_backward")
    return dx, None, None


register_autograd("ast_hip::hist_loss", _hist_backward, setup_context=_hist_setup)


@custom_op("ast_hip::remd_loss", mutates_args=())
def remd_loss(x: Tensor, y: Tensor, weight: float, branch: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor,
                                                                         Tensor, Tensor, Tensor, Tensor, Tensor]:
    """weight * the relaxed earth mover's distance of ops.remd_loss (branch: its _branch); outputs (loss,
    row_mean, col_mean, branch, inv_x, inv_y, row_min, row_index, col_min, col_index)."""
    loss, rmean, cmean, br, state = ops.remd_loss(x, y, float(weight), int(branch), acc=_acc(x))
    return (loss, rmean, cmean, br) + tuple(state)


@register_fake("ast_hip::remd_loss")
def _(x, y, weight, branch):
    n, (h, w), (hs, ws) = x.shape[0], x.shape[2:], y.shape[2:]
    i32 = dict(dtype=torch.int32)
    return (x.new_empty(()), x.new_empty((n,)), x.new_empty((n,)), x.new_empty((n,), dtype=torch.uint8),
            x.new_empty((n, h, w)), x.new_empty((y.shape[0], hs, ws)), x.new_empty((n, h, w)),
            x.new_empty((n, h, w), **i32), x.new_empty((n, hs, ws)), x.new_empty((n, hs, ws), **i32))


def _remd_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], *output[3:])
    ctx.weight = float(inputs[2])


def _remd_backward(ctx, g, *_):
    x, y, branch, *state = ctx.saved_tensors
    return ops.remd_loss_backward(x, y, tuple(state), branch, g.contiguous(), ctx.weight), None, None, None


register_autograd("ast_hip::remd_loss", _remd_backward, setup_context=_remd_setup)


@custom_op("ast_hip::selfsim_loss", mutates_args=())
def selfsim_loss(x: Tensor, c: Tensor, weight: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor,
                                                               Tensor, Tensor]:
    """weight * the self-similarity content loss of ops.selfsim_loss; outputs (loss, per_sample, inv_x, inv_c,
    r_x, r_c, t, pos, neg)."""
    loss, sums, state = ops.selfsim_loss(x, c, float(weight), acc=_acc(x))
    return (loss, sums) + tuple(state)


@register_fake("ast_hip::selfsim_loss")
def _(x, c, weight):
    n, (h, w) = x.shape[0], x.shape[2:]
    planes = (n, h * w, (h * w + 63) // 64)
    return ((x.new_empty(()), x.new_empty((n,))) + tuple(x.new_empty((n, h, w)) for _ in range(5))
            + (x.new_empty(planes, dtype=torch.int64), x.new_empty(planes, dtype=torch.int64)))


def _selfsim_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], *output[2:])
    ctx.weight = float(inputs[2])


def _selfsim_backward(ctx, g, *_):
    x, *state = ctx.saved_tensors
    return ops.selfsim_loss_backward(x, tuple(state), g.contiguous(), ctx.weight), None, None


register_autograd("ast_hip::selfsim_loss", _selfsim_backward, setup_context=_selfsim_setup)


@custom_op("ast_hip::cx_loss", mutates_args=())
def cx_loss(x: Tensor, y: Tensor, weight: float, h: float, center: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor,
                                                                                 Tensor, Tensor, Tensor, Tensor, Tensor,
                                                                                 Tensor, Tensor, Tensor]:
    """weight * the contextual loss of ops.cx_loss; outputs (loss, xc, yc, inv_x, inv_y, row_min, row_index,
    row_sum, row_dsum, col_cx, col_index, col_dist, per_sample_cx); xc and yc are empty when center is off."""
    loss, _, state = ops.cx_loss(x, y, float(weight), float(h), bool(center), acc=_acc(x))
    return (loss,) + tuple(state)


@register_fake("ast_hip::cx_loss")
def _(x, y, weight, h, center):
    n, (hh, ww), (hs, ws) = x.shape[0], x.shape[2:], y.shape[2:]
    i32 = dict(dtype=torch.int32)
    xc, yc = (torch.empty_like(x), torch.empty_like(y)) if center else (x.new_empty((0,)), x.new_empty((0,)))
    return (x.new_empty(()), xc, yc, x.new_empty((n, hh, ww)), x.new_empty((y.shape[0], hs, ws)),
            x.new_empty((n, hh, ww)), x.new_empty((n, hh, ww), **i32), x.new_empty((n, hh, ww)),
            x.new_empty((n, hh, ww)), x.new_empty((n, hs, ws)), x.new_empty((n, hs, ws), **i32),
            x.new_empty((n, hs, ws)), x.new_empty((n,)))


def _cx_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], *output[1:])
    ctx.weight, ctx.h = float(inputs[2]), float(inputs[3])


def _cx_backward(ctx, g, *_):
    x, y, *state = ctx.saved_tensors
    return ops.cx_loss_backward(x, y, tuple(state), g.contiguous(), ctx.weight, ctx.h), None, None, None, None


register_autograd("ast_hip::cx_loss", _cx_backward, setup_context=_cx_setup)


@custom_op("ast_hip::moment_loss", mutates_args=())
def moment_loss(x: Tensor, y_mean: Tensor, y_cov: Tensor, weight: float) -> Tuple[Tensor, Tensor, Tensor, Tensor,
                                                                                  Tensor]:
    """weight * the moment-matching style loss of ops.moment_loss against the statistics of
    ops.moment_stats; outputs (loss, per_sample, mean_x, sign_mu, sign_cov)."""
    loss, (mean_x, sign_mu, sign_cov, sums) = ops.moment_loss(x, y_mean, y_cov, float(weight), acc=_acc(x))
    return loss, sums, mean_x, sign_mu, sign_cov


@register_fake("ast_hip::moment_loss")
def _(x, y_mean, y_cov, weight):
    n, c = x.shape[:2]
    return (x.new_empty(()), x.new_empty((n,)), x.new_empty((n, c)), x.new_empty((n, c), dtype=torch.int8),
            x.new_empty((n, c, c), dtype=torch.int8))


def _moment_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], *output[2:])
    ctx.weight = float(inputs[3])


def _moment_backward(ctx, g, *_):
    x, *state = ctx.saved_tensors
    return ops.moment_loss_backward(x, tuple(state), g.contiguous(), ctx.weight), None, None, None


register_autograd("ast_hip::moment_loss", _moment_backward, setup_context=_moment_setup)


@custom_op("ast_hip::range_loss", mutates_args=())
def range_loss(x: Tensor, weight: float) -> Tensor:
    acc = _acc(x)
    check(lib().ast_range_loss_f32(ptr(x), x.numel(), float(weight), None, ptr(acc), None, 0, stream_ptr(x.device)),
          "range_loss")
    return acc[0]


@register_fake("ast_hip::range_loss")
def _(x, weight):
    return x.new_empty(())


def _range_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.weight = float(inputs[1])


def _range_backward(ctx, g):
    (x,) = ctx.saved_tensors
    dx = torch.empty_like(x)
    check(lib().ast_range_loss_f32(ptr(x), x.numel(), ctx.weight, ptr(g.contiguous()), None, ptr(dx), 0,
                                   stream_ptr(x.device)), "range_loss")
    return dx, None


register_autograd("ast_hip::range_loss", _range_backward, setup_context=_range_setup)


@custom_op("ast_hip::sqdiff_mean", mutates_args=())
def sqdiff_mean(x: Tensor, y: Tensor, weight: float) -> Tensor:
    acc = _acc(x)
    check(lib().ast_sqdiff_mean_f32(ptr(x), ptr(y), x.numel(), float(weight), None, ptr(acc), None, 0,
                                    stream_ptr(x.device)), "sqdiff")
    return acc[0]


@register_fake("ast_hip::sqdiff_mean")
def _(x, y, weight):
    return x.new_empty(())


def _sqdiff_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.weight = float(inputs[2])


def _sqdiff_backward(ctx, g):
    x, y = ctx.saved_tensors
    dx = torch.empty_like(x)
    check(lib().ast_sqdiff_mean_f32(ptr(x), ptr(y), x.numel(), ctx.weight, ptr(g.contiguous()), None, ptr(dx), 0,
                                    stream_ptr(x.device)), "sqdiff")
    return dx, None, None


register_autograd("ast_hip::sqdiff_mean", _sqdiff_backward, setup_context=_sqdiff_setup)


# ------------------------------------------------------------------------------------------------
# MobileNet-variant inference ops (eval-mode BatchNorm folded into the weights)
# ------------------------------------------------------------------------------------------------

_DT = {torch.float32: 0, torch.bfloat16: 1}


@custom_op("ast_hip::mb_expand_dw", mutates_args=())
def mb_expand_dw(x: Tensor, x2: Optional[Tensor], w1p: Optional[Tensor], b1: Optional[Tensor], wdw: Tensor,
                 bdw: Tensor, hid: int, cin_pad: int, k: int, stride: int, up: int) -> Tuple[Tensor, Tensor]:
    """expand 1x1 (+ folded BN, Hardswish) -> depthwise kxk (reflect, + folded BN, Hardswish):
    the depthwise output D [n, hid, ho, wo] and the SE pool sums [n, hid]."""
    from .mobilenetv2 import _expand_dw
    n, c1, h, w = x.shape
    cin = c1 + (x2.shape[1] if x2 is not None else 0)
    p = (k - 1) // 2
    ho, wo = (h * up + 2 * p - k) // stride + 1, (w * up + 2 * p - k) // stride + 1
    d = torch.empty((n, hid, ho, wo), device=x.device, dtype=x.dtype)
    pool = torch.empty((n, hid), device=x.device, dtype=torch.float32)
    check(_expand_dw(x.dtype, x, x2, c1, n, cin, h, w, up, w1p, b1, hid, cin_pad, wdw, bdw, k, stride, d, pool, ho, wo,
                     stream_ptr(x.device)), "mb_expand_dw")
    return d, pool


@register_fake("ast_hip::mb_expand_dw")
def _(x, x2, w1p, b1, wdw, bdw, hid, cin_pad, k, stride, up):
    n, _, h, w = x.shape
    p = (k - 1) // 2
    ho, wo = (h * up + 2 * p - k) // stride + 1, (w * up + 2 * p - k) // stride + 1
    return x.new_empty((n, hid, ho, wo)), x.new_empty((n, hid), dtype=torch.float32)


@custom_op("ast_hip::mb_se_fold", mutates_args=())
def mb_se_fold(pool: Tensor, hw: int, fc1w: Tensor, fc1b: Tensor, fc2w: Tensor, fc2b: Tensor, w2: Tensor,
               cout_pad: int, hid_pad: int, bf16: bool) -> Tensor:
    """SELayer's MLP on the pooled means, its Hardtanh(0, 1) gate folded into the pw-linear weights:
    [n, cout_pad, hid_pad] (zero padded) in the activations' dtype."""
    n, hid = pool.shape
    cout = w2.shape[0]
    dt = torch.bfloat16 if bf16 else torch.float32
    wg = torch.empty((n, cout_pad, hid_pad), device=pool.device, dtype=dt)
    check(lib().ast_mb_se_fold(_DT[dt], ptr(pool), n, hid, hw, ptr(fc1w), ptr(fc1b), fc1w.shape[0], ptr(fc2w),
                               ptr(fc2b), ptr(w2), cout, cout_pad, hid_pad, ptr(wg), stream_ptr(pool.device)),
          "mb_se_fold")
    return wg


@register_fake("ast_hip::mb_se_fold")
def _(pool, hw, fc1w, fc1b, fc2w, fc2b, w2, cout_pad, hid_pad, bf16):
    return pool.new_empty((pool.shape[0], cout_pad, hid_pad), dtype=torch.bfloat16 if bf16 else torch.float32)


@custom_op("ast_hip::mb_pw", mutates_args=())
def mb_pw(d: Tensor, wg: Tensor, bias: Optional[Tensor], cout: int, res: Optional[Tensor], res_up: bool) -> Tensor:
    """pw-linear conv with the SE-gated weights (+ folded BN bias, + residual / upsampled residual)."""
    n, hid, h, w = d.shape
    cout_pad, hid_pad = wg.shape[1], wg.shape[2]
    out = torch.empty((n, cout, h, w), device=d.device, dtype=d.dtype)
    check(lib().ast_mb_pw(_DT[d.dtype], ptr(d), n, hid, hid_pad, h, w, ptr(wg), cout_pad * hid_pad, ptr(bias), cout,
                          cout_pad, ptr(res), 1 if res_up else 0, ptr(out), stream_ptr(d.device)), "mb_pw")
    return out


@register_fake("ast_hip::mb_pw")
def _(d, wg, bias, cout, res, res_up):
    return d.new_empty((d.shape[0], cout, d.shape[2], d.shape[3]))


@custom_op("ast_hip::mb_expand_gemm", mutates_args=())
def mb_expand_gemm(x: Tensor, x2: Optional[Tensor], w1p: Tensor, b1: Tensor, hid: int, cin_pad: int) -> Tensor:
    """The expand half of a wide DepthWiseConv (ada_out, 256 -> 768) as a GEMM + Hardswish."""
    n, c1, h, w = x.shape
    cin = c1 + (x2.shape[1] if x2 is not None else 0)
    out = torch.empty((n, hid, h, w), device=x.device, dtype=x.dtype)
    check(lib().ast_mb_expand_gemm(_DT[x.dtype], ptr(x), ptr(x2), c1, n, cin, h, w, ptr(w1p), ptr(b1), hid, cin_pad,
                                   ptr(out), stream_ptr(x.device)), "mb_expand_gemm")
    return out


@register_fake("ast_hip::mb_expand_gemm")
def _(x, x2, w1p, b1, hid, cin_pad):
    return x.new_empty((x.shape[0], hid, x.shape[2], x.shape[3]))


@custom_op("ast_hip::mb_conv3x3_dense", mutates_args=())
def mb_conv3x3_dense(x: Tensor, wt: Tensor, bias: Optional[Tensor], act: int, out_bf16: bool) -> Tensor:
    """Dense 3x3 reflect-pad conv of the variant (block 0 + Hardswish; the decoder image conv)."""
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    dt = torch.bfloat16 if out_bf16 else torch.float32
    y = torch.empty((n, cout, h, w), device=x.device, dtype=dt)
    check(lib().ast_mb_conv3x3_dense(_DT[x.dtype], _DT[dt], ptr(x), ptr(wt), ptr(bias), ptr(y), n, cin, cout, h, w,
                                     act, stream_ptr(x.device)), "mb_conv3x3_dense")
    return y


@register_fake("ast_hip::mb_conv3x3_dense")
def _(x, wt, bias, act, out_bf16):
    return x.new_empty((x.shape[0], wt.shape[0], x.shape[2], x.shape[3]),
                       dtype=torch.bfloat16 if out_bf16 else torch.float32)


# ------------------------------------------------------------------------------------------------
# Colour spaces (model_util.py:11-140) and colour-preserving recombination
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::color_convert", mutates_args=())
def color_convert(x: Tensor, mode: int, out_bf16: bool) -> Tensor:
    """mode: an AST_COLOR_* code (ops.COLOR_MODES); fp32 result unless out_bf16 (bf16 input only)."""
    return ops.color_convert(x, mode, torch.bfloat16 if out_bf16 else torch.float32)


@register_fake("ast_hip::color_convert")
def _(x, mode, out_bf16):
    return x.new_empty(x.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32)


@custom_op("ast_hip::color_convert_backward", mutates_args=())
def color_convert_backward(x: Tensor, grad: Tensor, mode: int) -> Tensor:
    """J^T grad of color_convert at x (fp32). An op of its own, so that a traced backward
    (torch.compile, AOT autograd) sees an opaque kernel with a fake implementation."""
    return ops.color_convert_backward(x, grad, mode)


@register_fake("ast_hip::color_convert_backward")
def _(x, grad, mode):
    return x.new_empty(x.shape)


def _color_setup(ctx, inputs, output):
    x, mode, out_bf16 = inputs
    if out_bf16:
        raise NotImplementedError("ast_hip::color_convert backward needs the float32 result (out_bf16=False)")
    ctx.save_for_backward(x)
    ctx.mode = mode


def _color_backward(ctx, g):
    (x,) = ctx.saved_tensors
    return torch.ops.ast_hip.color_convert_backward(x.float(), g, ctx.mode).to(x.dtype), None, None


register_autograd("ast_hip::color_convert", _color_backward, setup_context=_color_setup)


@custom_op("ast_hip::luma_transfer", mutates_args=())
def luma_transfer(stylised: Tensor, content: Tensor) -> Tensor:
    """The Lab luminance of clamp01(stylised) with the a, b of clamp01(content), as RGB."""
    return ops.luma_transfer(stylised, content)


@register_fake("ast_hip::luma_transfer")
def _(stylised, content):
    return content.new_empty(content.shape)


# ------------------------------------------------------------------------------------------------
# Bilinear resize and its adjoint (csrc/pyramid.hip): the Laplacian pyramid's level step
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::resize_bilinear", mutates_args=())
def resize_bilinear(x: Tensor, height: int, width: int, add: Optional[Tensor], sign: float) -> Tensor:
    """F.interpolate(x, (height, width), mode="bilinear", align_corners=False) on fp32 planes; with
    `add` the result is add + sign * resize(x)."""
    return ops.resize_bilinear(x, (height, width), add=add, sign=sign)


@register_fake("ast_hip::resize_bilinear")
def _(x, height, width, add, sign):
    return x.new_empty(tuple(x.shape[:-2]) + (height, width))


@custom_op("ast_hip::resize_bilinear_adjoint", mutates_args=())
def resize_bilinear_adjoint(grad: Tensor, height: int, width: int) -> Tensor:
    """The transpose of resize_bilinear from (height, width): an op of its own, so that a traced
    backward sees an opaque kernel with a fake implementation."""
    return ops.resize_bilinear_adjoint(grad, (height, width))


@register_fake("ast_hip::resize_bilinear_adjoint")
def _(grad, height, width):
    return grad.new_empty(tuple(grad.shape[:-2]) + (height, width))


def _resize_setup(ctx, inputs, output):
    x, _, _, add, sign = inputs
    ctx.in_size = (int(x.shape[-2]), int(x.shape[-1]))
    ctx.sign = float(sign) if add is not None else 1.0
    ctx.has_add = add is not None


def _resize_backward(ctx, g):
    dx = None
    if ctx.needs_input_grad[0]:
        dx = torch.ops.ast_hip.resize_bilinear_adjoint(g.contiguous(), ctx.in_size[0], ctx.in_size[1])
        if ctx.sign != 1.0:
            dx = dx * ctx.sign
    return dx, None, None, g if ctx.has_add and ctx.needs_input_grad[3] else None, None


register_autograd("ast_hip::resize_bilinear", _resize_backward, setup_context=_resize_setup)


# ------------------------------------------------------------------------------------------------
# Regional multi-style AdaIN (csrc/adain_regions.hip; inference only, no autograd)
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::resize_labels", mutates_args=())
def resize_labels(labels: Tensor, h: int, w: int) -> Tensor:
    """Nearest-neighbour resize of uint8 label maps [N, H, W] to [N, h, w]."""
    return ops.resize_labels(labels, h, w)


@register_fake("ast_hip::resize_labels")
def _(labels, h, w):
    return labels.new_empty((labels.shape[0], h, w))


@custom_op("ast_hip::region_stats", mutates_args=())
def region_stats(x: Tensor, labels: Tensor, regions: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Per-region mean and unbiased std [N, regions, C] and pixel counts [N, regions] (int32)."""
    return ops.region_stats(x, labels, regions)


@register_fake("ast_hip::region_stats")
def _(x, labels, regions):
    n, c = x.shape[:2]
    return (x.new_empty((n, regions, c)), x.new_empty((n, regions, c)),
            x.new_empty((n, regions), dtype=torch.int32))


@custom_op("ast_hip::adain_regions", mutates_args=())
def adain_regions(content: Tensor, labels: Tensor, style_mean: Tensor, style_std: Tensor, mix: Tensor, alpha: float,
                  swap_style_stats: bool) -> Tensor:
    """Per-region AdaIN against a per-region mix of the rows of a style-statistics table."""
    return ops.adain_regions(content, labels, style_mean, style_std, mix, alpha=alpha,
                             swap_style_stats=swap_style_stats)


@register_fake("ast_hip::adain_regions")
def _(content, labels, style_mean, style_std, mix, alpha, swap_style_stats):
    return torch.empty_like(content)


# ------------------------------------------------------------------------------------------------
# Exact feature distribution matching and the plane sort (csrc/efdm.hip)
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::efdm", mutates_args=())
def efdm(content: Tensor, style: Tensor, alpha: float) -> Tensor:
    """Rank r of every content plane takes the style plane's sorted value S[j(r)] (+ alpha blend)."""
    return ops.efdm(content, style, alpha=alpha)


@register_fake("ast_hip::efdm")
def _(content, style, alpha):
    return torch.empty_like(content)


def _efdm_backward(ctx, g):   # straight-through: d content = grad_out, none for the style; no kernel
    return g, None, None


register_autograd("ast_hip::efdm", _efdm_backward)


@custom_op("ast_hip::plane_sort", mutates_args=())
def plane_sort(x: Tensor) -> Tuple[Tensor, Tensor]:
    """Every plane sorted in IEEE totalOrder, ties in index order: (values, int32 indices)."""
    return ops.plane_sort(x, return_index=True)


@register_fake("ast_hip::plane_sort")
def _(x):
    return torch.empty_like(x), x.new_empty(x.shape, dtype=torch.int32)


@custom_op("ast_hip::efdm_regions", mutates_args=())
def efdm_regions(content: Tensor, labels: Tensor, styles: Tensor, mix: Tensor, style_labels: Optional[Tensor],
                 alpha: float) -> Tensor:
    """EFDM per region of a uint8 label map towards a per-region mix [N or 1, K, S] of a bank of styles."""
    return ops.efdm_regions(content, labels, styles, mix, style_labels=style_labels, alpha=alpha)


@register_fake("ast_hip::efdm_regions")
def _(content, labels, styles, mix, style_labels, alpha):
    return torch.empty_like(content)


def _efdm_regions_backward(ctx, g):
    raise NotImplementedError("ast_hip::efdm_regions has no backward: regional distribution matching is "
                              "inference-only")


register_autograd("ast_hip::efdm_regions", _efdm_regions_backward)


# ------------------------------------------------------------------------------------------------
# Whitening and colouring transform (csrc/wct.hip; inference only)
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::wct", mutates_args=())
def wct(content: Tensor, style: Tensor, alpha: float, eps_rel: float, iters: int) -> Tensor:
    """alpha * (T (c - mu_c) + mu_s) + (1 - alpha) * c with T = cov_s^(1/2) cov_c^(-1/2)."""
    return ops.wct(content, style, alpha=alpha, eps_rel=eps_rel, iters=iters)


@register_fake("ast_hip::wct")
def _(content, style, alpha, eps_rel, iters):
    return torch.empty_like(content)


def _wct_backward(ctx, g):
    raise NotImplementedError("ast_hip::wct has no backward: the whitening and colouring transform is inference-only")


register_autograd("ast_hip::wct", _wct_backward)


@custom_op("ast_hip::wct_regions", mutates_args=())
def wct_regions(content: Tensor, labels: Tensor, styles: Tensor, mix: Tensor, style_labels: Optional[Tensor],
                alpha: float, eps_rel: float, iters: int) -> Tensor:
    """WCT per region of a uint8 label map towards a per-region mix [N or 1, K, S] of a bank of styles."""
    return ops.wct_regions(content, labels, styles, mix, style_labels=style_labels, alpha=alpha, eps_rel=eps_rel,
                           iters=iters)


@register_fake("ast_hip::wct_regions")
def _(content, labels, styles, mix, style_labels, alpha, eps_rel, iters):
    return torch.empty_like(content)


def _wct_regions_backward(ctx, g):
    raise NotImplementedError("ast_hip::wct_regions has no backward: the whitening and colouring transform is "
                              "inference-only")


register_autograd("ast_hip::wct_regions", _wct_regions_backward)


# ------------------------------------------------------------------------------------------------
# Style swap (csrc/swap.hip; inference only)
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::style_swap", mutates_args=())
def style_swap(content: Tensor, style: Tensor, alpha: float, normalize: bool) -> Tensor:
    """Every 3x3 content patch replaced by its best-matching style patch, overlaps averaged (+ alpha blend)."""
    return ops.style_swap(content, style, alpha=alpha, normalize=normalize)


@register_fake("ast_hip::style_swap")
def _(content, style, alpha, normalize):
    return torch.empty_like(content)


def _style_swap_backward(ctx, g):
    raise NotImplementedError("ast_hip::style_swap has no backward: style swap is inference-only")


register_autograd("ast_hip::style_swap", _style_swap_backward)


@custom_op("ast_hip::style_swap_guided", mutates_args=())
def style_swap_guided(content: Tensor, styles: Tensor, content_class: Tensor, style_class: Tensor, alpha: float,
                      normalize: bool) -> Tensor:
    """Style swap over a bank of styles, every content patch matched within its own class (uint8 class maps)."""
    return ops.style_swap_guided(content, styles, content_class, style_class, alpha=alpha, normalize=normalize)


@register_fake("ast_hip::style_swap_guided")
def _(content, styles, content_class, style_class, alpha, normalize):
    return torch.empty_like(content)


def _style_swap_guided_backward(ctx, g):
    raise NotImplementedError("ast_hip::style_swap_guided has no backward: style swap is inference-only")


register_autograd("ast_hip::style_swap_guided", _style_swap_guided_backward)


# ------------------------------------------------------------------------------------------------
# Feature k-means and the label mode filter (csrc/kmeans.hip; inference only)
# ------------------------------------------------------------------------------------------------

@custom_op("ast_hip::kmeans", mutates_args=())
def kmeans(x: Tensor, k: int, iters: int, init: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """Lloyd's k-means over the points of a bank [B, C, H, W]: centroids [k, C], labels uint8 [B, H, W], counts [k]."""
    return ops.kmeans(x, k, iters=iters, init=init)


@register_fake("ast_hip::kmeans")
def _(x, k, iters, init):
    b, c, h, w = x.shape
    return (x.new_empty((k, c)), x.new_empty((b, h, w), dtype=torch.uint8), x.new_empty((k,), dtype=torch.int32))


def _kmeans_backward(ctx, *g):
    raise NotImplementedError("ast_hip::kmeans has no backward: the clustering is inference-only")


register_autograd("ast_hip::kmeans", _kmeans_backward)


@custom_op("ast_hip::kmeans_assign", mutates_args=())
def kmeans_assign(x: Tensor, centroids: Tensor) -> Tensor:
    """The nearest of the centroids [K, C] for every pixel of x [B, C, H, W]: uint8 [B, H, W]."""
    return ops.kmeans_assign(x, centroids)


@register_fake("ast_hip::kmeans_assign")
def _(x, centroids):
    return x.new_empty((x.shape[0], x.shape[2], x.shape[3]), dtype=torch.uint8)


def _kmeans_assign_backward(ctx, g):
    raise NotImplementedError("ast_hip::kmeans_assign has no backward: labels are not differentiable")


register_autograd("ast_hip::kmeans_assign", _kmeans_assign_backward)


@custom_op("ast_hip::label_mode_filter", mutates_args=())
def label_mode_filter(labels: Tensor, regions: int, passes: int) -> Tensor:
    """`passes` rounds of a 3x3 majority vote over uint8 label maps [N, H, W]."""
    return ops.label_mode_filter(labels, regions, passes=passes)


@register_fake("ast_hip::label_mode_filter")
def _(labels, regions, passes):
    return torch.empty_like(labels)


OPS: List[str] = ["conv3x3", "adain_map", "content_mvn_loss", "style_loss", "huber_loss", "tv_loss", "hist_loss",
                  "remd_loss", "selfsim_loss", "cx_loss", "moment_loss", "range_loss", "sqdiff_mean", "mb_expand_dw", "mb_se_fold", "mb_pw",
                  "mb_expand_gemm", "mb_conv3x3_dense", "color_convert", "color_convert_backward", "luma_transfer",
                  "resize_bilinear", "resize_bilinear_adjoint", "resize_labels",
                  "region_stats", "adain_regions", "efdm", "plane_sort", "efdm_regions", "wct", "wct_regions",
                  "style_swap", "style_swap_guided", "kmeans", "kmeans_assign", "label_mode_filter"]
