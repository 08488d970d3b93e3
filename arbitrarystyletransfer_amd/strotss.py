"""Stylisation by optimisation (STROTSS; Kolkin, Salavon, Shakhnarovich, CVPR 2019) on the library's own
loss kernels: the one mode that needs no trained decoder, only the frozen VGG loss network.

The image is parametrised as a Laplacian pyramid (ops.lap_build; its collapse is functional.LapCollapseFn,
csrc/pyramid.hip) and optimised coarse to fine. Per scale s of `scales` (index k in that tuple):
  size        the longer side becomes min(s, the image's own longer side), the aspect is kept, both sides
              are rounded to multiples of 16 (the loss network's deepest tap is 1/16 of the image), at least
              16; a scale whose content size repeats the previous one is skipped
  alpha_k     content_weight / 2^k
  start       at the first scale `init` resized to it, or, without one, content - resize(down(content)) +
              the style's mean colour (the paper's start); afterwards the previous result, resized
  variables   the levels of ops.lap_build(start, levels), levels capped so that the coarsest side stays >= 1
  objective   (alpha_k sum_taps selfsim(taps(img), taps(content)) + remd_lam sum_taps remd(taps(img),
              taps(style)) + moment_lam sum_taps moment(taps(img), stats(taps(style))))
              / (alpha_k + remd_lam + moment_lam)
              every term exact and unsampled (the kernels make the paper's 1024-position sampling
              unnecessary), so nothing is random: a run is reproducible bit for bit. A term whose weight is
              0 launches nothing. The content and style taps and ops.moment_stats of the style taps are
              computed once per scale, under no_grad.
  optimiser   optim.FusedAdam on the levels, no clipping, its capturable step (step count on the device)
One iteration -- collapse, loss-network forward, losses, backward, Adam -- is one function; with graph=True
it is captured into a hipGraph once per scale and replayed `iters` times, with graph=False the same function
is called `iters` times: the two give the same image in bits. The paper's RMSprop and its palette (colour)
term are not implemented.
"""
from __future__ import annotations

import gc
import math

import torch

from . import _lib, models, ops
from . import functional as Fn
from . import losses as L
from ._lib import HipOpError
from .optim import FusedAdam
from .train import _TAPS, _tap_index

DEFAULT_SCALES = (64, 128, 256, 512)
DEFAULT_TAPS = ("relu_9", "relu_15")


# ---- the schedule: pure functions ------------------------------------------------------------------

def scale_size(size, scale: int):
    """(H, W) of an image of `size` at `scale`: longer side min(scale, own longer side), aspect kept, both
    sides rounded to the nearest multiple of 16 (halves up), at least 16."""
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or int(scale) < 1:
        raise ValueError(f"scale_size: sizes and scales are positive, got {size} at {scale}")
    longer = max(h, w)
    target = min(int(scale), longer)
    side = lambda v: max(16, 16 * ((2 * v * target + 16 * longer) // (32 * longer)))  # noqa: E731  round(v t / (16 l))
    return side(h), side(w)


def scale_schedule(size, scales):
    """[(k, (H, W))]: the scales that run, with their index in `scales`; a scale whose size repeats the
    previous kept one is skipped."""
    out = []
    for k, s in enumerate(scales):
        hw = scale_size(size, s)
        if not out or out[-1][1] != hw:
            out.append((k, hw))
    return out


def level_cap(size, levels: int) -> int:
    """`levels` capped so that halving never goes below one pixel: at most floor(log2(shorter side))."""
    if int(levels) < 0:
        raise ValueError(f"levels must be >= 0, got {levels}")
    return min(int(levels), int(math.floor(math.log2(min(int(size[0]), int(size[1]))))))


def content_weight_at(content_weight: float, k: int) -> float:
    """alpha_k = content_weight / 2^k."""
    return float(content_weight) / float(2 ** int(k))


def tap_stride(tap: str) -> int:
    """Image pixels per side of one pixel of a loss-network tap (VGG19: pools after convs 2, 4, 8, 12)."""
    i = int(tap.split("_")[1])
    return 1 if i <= 2 else 2 if i <= 4 else 4 if i <= 8 else 8 if i <= 12 else 16


def check_limits(schedule, style_sizes, selfsim_taps, remd_taps, alpha_on: bool, remd_on: bool):
    """Raise HipOpError for a scale whose tap maps exceed an op's pixel limit; nothing is launched."""
    for (k, (h, w)), (hs, ws) in zip(schedule, style_sizes):
        if alpha_on:
            for tap in selfsim_taps:
                px = (h // tap_stride(tap)) * (w // tap_stride(tap))
                if px > ops.SELFSIM_MAX_PIXELS:
                    raise HipOpError(f"stylize: scale {k} ({h}x{w}) gives {px} pixels at the self-similarity tap "
                                     f"{tap}; the limit is {ops.SELFSIM_MAX_PIXELS}. Use a smaller scale or a "
                                     f"deeper tap")
        if remd_on:
            for tap in remd_taps:
                px = max((h // tap_stride(tap)) * (w // tap_stride(tap)), (hs // tap_stride(tap)) * (ws // tap_stride(tap)))
                if px > ops.REMD_MAX_PIXELS:
                    raise HipOpError(f"stylize: scale {k} ({h}x{w}, style {hs}x{ws}) gives {px} pixels at the "
                                     f"relaxed-EMD tap {tap}; the limit is {ops.REMD_MAX_PIXELS}")


# ---- the stylizer ----------------------------------------------------------------------------------

class StrotssStylizer:
    """stylize(content, style) optimises an image against the frozen loss network (module docstring)."""

    def __init__(self, lossnet=None, device=None):
        self.device = torch.device(device or "cuda")
        self.lossnet = (lossnet or models.PretrainedEncoder(_TAPS)).to(self.device).eval()
        self.lossnet.requires_grad_(False)
        self.lossnet._content_layers = set(_TAPS)

    # -- one scale -----------------------------------------------------------------------------------
    def _targets(self, c_s, s_s, cfg):
        """What the objective compares against, computed once per scale: (content maps of the selfsim taps,
        style maps of the remd taps, style statistics of the moment taps)."""
        with torch.no_grad():
            c_taps = self.lossnet(c_s) if cfg["alpha"] > 0 else None
            s_taps = self.lossnet(s_s) if cfg["remd_lam"] > 0 or cfg["moment_lam"] > 0 else None
            content = [c_taps[i] for i in cfg["selfsim_idx"]] if cfg["alpha"] > 0 else []
            style = [s_taps[i] for i in cfg["remd_idx"]] if cfg["remd_lam"] > 0 else []
            stats = [ops.moment_stats(s_taps[i]) for i in cfg["moment_idx"]] if cfg["moment_lam"] > 0 else []
        return content, style, stats

    def _objective(self, img, targets, cfg):
        """{"objective": ..., and one entry per term whose weight is not 0}: 0-d tensors."""
        content, style, stats = targets
        taps = self.lossnet(img)
        out, total = {}, None
        if cfg["alpha"] > 0:
            out["selfsim"] = torch.stack([L.compute_selfsim_loss(taps[i], m) for i, m in zip(cfg["selfsim_idx"], content)]).sum()
            total = cfg["alpha"] * out["selfsim"]
        if cfg["remd_lam"] > 0:
            out["remd"] = torch.stack([L.compute_remd_loss(taps[i], m) for i, m in zip(cfg["remd_idx"], style)]).sum()
            total = cfg["remd_lam"] * out["remd"] if total is None else total + cfg["remd_lam"] * out["remd"]
        if cfg["moment_lam"] > 0:
            out["moment"] = torch.stack([torch.ops.ast_hip.moment_loss(taps[i], mean, cov, 1.0)[0]
                                         for i, (mean, cov) in zip(cfg["moment_idx"], stats)]).sum()
            total = cfg["moment_lam"] * out["moment"] if total is None else total + cfg["moment_lam"] * out["moment"]
        if total is None:
            raise ValueError("stylize: every term of the objective has weight 0")
        out["objective"] = total / (cfg["alpha"] + cfg["remd_lam"] + cfg["moment_lam"])
        return out

    def _evaluate(self, leaves, targets, cfg):
        with torch.no_grad(), _lib.accumulator_pool():
            return {k: v.clone() for k, v in self._objective(ops.lap_collapse(leaves), targets, cfg).items()}

    def _optimise(self, leaves, targets, cfg, iters, lr, graph, want_history):
        """`iters` Adam iterations on the leaves, in place; (objective terms before the first iteration,
        after the last) when asked for."""
        flat = torch.zeros(sum(t.numel() for t in leaves), device=leaves[0].device, dtype=torch.float32)
        off = 0
        for t in leaves:   # persistent gradient storage: the optimizer's device table points at it
            t.grad = flat[off:off + t.numel()].view(t.shape)
            off += t.numel()
        optim = FusedAdam(leaves, lr=lr, betas=(0.9, 0.999), eps=1e-8)
        self.lossnet.prepack()
        optim.prepare_static()
        optim.fill_static()

        def body():
            flat.zero_()
            with _lib.accumulator_pool():
                out = self._objective(Fn.LapCollapseFn.apply(*leaves), targets, cfg)
            out["objective"].backward()   # accumulates into the zeroed persistent gradients, in place
            optim.step_static()
            return {k: v.detach() for k, v in out.items()}

        before = None
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            gc.disable()   # no finalizer of unrelated garbage may run (and free or sync) inside the capture
            try:
                with torch.cuda.graph(g):
                    out = body()
            finally:
                gc.enable()
            for it in range(iters):
                g.replay()
                optim.after_static_step()
                if it == 0 and want_history:
                    before = {k: v.clone() for k, v in out.items()}
            torch.cuda.current_stream().synchronize()   # the replays are done before the graph's pool goes
            del g, out
        else:
            for it in range(iters):
                out = body()
                optim.after_static_step()
                if it == 0 and want_history:
                    before = {k: v.clone() for k, v in out.items()}
        for t in leaves:
            t.grad = None
        return (before, self._evaluate(leaves, targets, cfg)) if want_history else None

    # -- the whole run -------------------------------------------------------------------------------
    def stylize(self, content_img, style_img, *, init=None, scales=DEFAULT_SCALES, iters=200, lr=2e-3,
                content_weight=16.0, levels=5, remd_taps=DEFAULT_TAPS, moment_taps=DEFAULT_TAPS,
                selfsim_taps=DEFAULT_TAPS, remd_lam=1.0, moment_lam=1.0, graph=True, return_history=False,
                clamp=False):
        """The stylised image [N, 3, H, W] at the last scale's size (and, with return_history, per image the
        per-scale list of {"size", "before", "after"}: the objective and its terms before the first and
        after the last iteration, as device scalars). content_img [N, 3, H, W] in [0, 1]; style_img [N or 1,
        3, Hs, Ws] of any size; init (optional) [N, 3, h, w]: the image to refine. A batch runs image by
        image: the scales differ per pair."""
        content_img = ops._dev(content_img, "content_img")
        style_img = ops._dev(style_img, "style_img")
        if (content_img.dim() != 4 or content_img.shape[1] != 3 or style_img.dim() != 4 or style_img.shape[1] != 3
                or style_img.shape[0] not in (1, content_img.shape[0]) or content_img.numel() == 0):
            raise HipOpError(f"stylize needs [N, 3, H, W] content and [N or 1, 3, Hs, Ws] style images, got "
                             f"{tuple(content_img.shape)} and {tuple(style_img.shape)}")
        if init is not None:
            init = ops._dev(init, "init")
            if init.dim() != 4 or init.shape[:2] != content_img.shape[:2]:
                raise HipOpError(f"stylize: init must be [N, 3, h, w] for content {tuple(content_img.shape)}, got "
                                 f"{tuple(init.shape)}")
        if int(iters) < 0 or not scales:
            raise ValueError("stylize: iters >= 0 and at least one scale")
        if min(float(content_weight), float(remd_lam), float(moment_lam)) < 0:
            raise ValueError("stylize: the weights are not negative")
        cfg = dict(remd_lam=float(remd_lam), moment_lam=float(moment_lam),
                   selfsim_idx=[_tap_index(k, "selfsim_taps") for k in selfsim_taps],
                   remd_idx=[_tap_index(k, "remd_taps") for k in remd_taps],
                   moment_idx=[_tap_index(k, "moment_taps") for k in moment_taps])
        schedule = scale_schedule(content_img.shape[2:], scales)
        style_sizes = [scale_size(style_img.shape[2:], scales[k]) for k, _ in schedule]
        check_limits(schedule, style_sizes, selfsim_taps, remd_taps, float(content_weight) > 0, float(remd_lam) > 0)
        images, histories = [], []
        for n in range(content_img.shape[0]):
            content = content_img[n:n + 1]
            style = style_img[n:n + 1] if style_img.shape[0] > 1 else style_img
            img, history = (init[n:n + 1] if init is not None else None), []
            for j, ((k, size), ssize) in enumerate(zip(schedule, style_sizes)):
                with torch.no_grad():
                    c_s, s_s = ops.resize_bilinear(content, size), ops.resize_bilinear(style, ssize)
                    if img is not None:
                        start = ops.resize_bilinear(img, size)
                    else:   # the paper's start: the content's finest Laplacian level on the style's mean colour
                        start = ops.lap_build(c_s, 1)[0] + s_s.mean(dim=(2, 3), keepdim=True)
                if int(iters) == 0:
                    img = start
                    continue
                cfg["alpha"] = content_weight_at(content_weight, k)
                leaves = [t.requires_grad_(True) for t in ops.lap_build(start, level_cap(size, levels))]
                targets = self._targets(c_s, s_s, cfg)
                hist = self._optimise(leaves, targets, cfg, int(iters), float(lr), bool(graph), bool(return_history))
                if return_history:
                    history.append({"size": size, "before": hist[0], "after": hist[1]})
                with torch.no_grad():
                    img = ops.lap_collapse([t.detach() for t in leaves])
                del leaves, targets
                gc.collect()   # the scale's graph and its pool go before the next capture
            images.append(img.clamp(0.0, 1.0) if clamp else img)
            histories.append(history)
        out = torch.cat(images) if len(images) > 1 else images[0]
        return (out, histories if len(histories) > 1 else histories[0]) if return_history else out
