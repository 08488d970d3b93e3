"""Drop-in for the reference models.py: the same module names, constructor/forward signatures and
state-dict layouts, running on the HIP kernels of libast_hip.so.

`from arbitrarystyletransfer_amd.models import *` gives what `from models import *` gives the
reference callers (train.py:15-16): torch, nn, F, every conf name, the loss functions,
channel_stats / calc_mean_std / mean_variance_norm and the model classes.

Hot path: PretrainedEncoder(['relu_9']) -> AdaIN -> VGGDecoder, composed by
AdaINStyleTransfer. Tensors must live on a HIP device; there is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: F401  (re-exported like the reference)

from . import functional as Fn
from . import mbtrain, ops, synth
from .conf import *  # noqa: F401,F403
from .conf import device  # noqa: F401
from .losses import *  # noqa: F401,F403
from .model_util import channel_stats, lab2rgb, rgb2lab  # noqa: F401  (re-exported, models.py:4)

IMNET_MEAN = (0.485, 0.456, 0.406)   # models.py:189
IMNET_STD = (0.229, 0.224, 0.225)    # models.py:190


class AdaIN(nn.Module):
    """AdaIN.forward, models.py:37-51, as one HIP launch (stats of both maps + normalise-affine).

    The reference unpacks channel_stats' (mean, std) as `style_std, style_mean` (models.py:44), so
    it computes (c - mu_c)/sigma_c * mu_s + sigma_s. That is the default here, for
    parity; `canonical=True` gives Huang & Belongie's (c - mu_c)/sigma_c * sigma_s + mu_s.
    `alpha` (default 1.0) fuses the blend of models.py:471: alpha * t + (1 - alpha) * content.
    """

    def __init__(self, canonical: bool = False):
        super().__init__()
        self.canonical = canonical

    def forward(self, content_map, style_map, alpha: float = 1.0):
        if _compiling():   # torch.compile: the registered op (fake impl + autograd), no graph break
            return torch.ops.ast_hip.adain_map(content_map, style_map, float(alpha), not self.canonical)
        if torch.is_grad_enabled() and (content_map.requires_grad or style_map.requires_grad):
            return Fn.AdaINFn.apply(content_map, style_map, float(alpha), not self.canonical)
        return ops.adain(content_map, style_map, alpha=alpha, swap_style_stats=not self.canonical)


class EFDM(nn.Module):
    """Exact feature distribution matching (Zhang et al., CVPR 2022) as a drop-in for the AdaIN
    layer: every content channel keeps its spatial ordering and takes the style channel's whole
    empirical distribution (ops.efdm; the reference has no counterpart). `alpha` fuses the blend
    c + alpha * (t - c). Under autograd the gradient passes straight through to the content
    (Fn.EFDMFn); none reaches the style. No parameters."""

    def forward(self, content_map, style_map, alpha: float = 1.0):
        if _compiling():
            return _ops().efdm(content_map, style_map, float(alpha))
        if torch.is_grad_enabled() and (content_map.requires_grad or style_map.requires_grad):
            return Fn.EFDMFn.apply(content_map, style_map, float(alpha))
        return ops.efdm(content_map, style_map, alpha=alpha)


class WCT(nn.Module):
    """Whitening and colouring transform (Li et al., NeurIPS 2017) as a drop-in for the AdaIN layer:
    the content features are whitened with cov_c^(-1/2) and coloured with cov_s^(1/2), so their
    cross-channel covariance and mean become the style's (ops.wct; the reference has no
    counterpart). `alpha` fuses the blend alpha * t + (1 - alpha) * c. Inference only: there is no
    backward. No parameters."""

    def __init__(self, eps_rel: float = ops.WCT_EPS_REL, iters: int = 0):
        super().__init__()
        self.eps_rel, self.iters = float(eps_rel), int(iters)

    def forward(self, content_map, style_map, alpha: float = 1.0):
        if torch.is_grad_enabled() and (content_map.requires_grad or style_map.requires_grad):
            raise NotImplementedError("WCT is inference-only; run it under torch.no_grad()")
        if _compiling():
            return _ops().wct(content_map, style_map, float(alpha), self.eps_rel, self.iters)
        return ops.wct(content_map, style_map, alpha=alpha, eps_rel=self.eps_rel, iters=self.iters)


class StyleSwap(nn.Module):
    """Style swap (Chen & Schmidt 2016): every 3x3 patch of the content map is replaced by the most
    similar 3x3 patch of the style map and the overlaps are averaged, so the result is made of the
    style's own local structure (ops.style_swap; the reference has no counterpart).
    `normalize=True` matches on the instance-normalised maps and reconstructs from the raw style
    features (the style decorator of Avatar-Net). `alpha` fuses the blend alpha * t + (1 - alpha) * c.
    Inference only: there is no backward. No parameters."""

    def __init__(self, normalize: bool = False):
        super().__init__()
        self.normalize = bool(normalize)

    def forward(self, content_map, style_map, alpha: float = 1.0):
        if torch.is_grad_enabled() and (content_map.requires_grad or style_map.requires_grad):
            raise NotImplementedError("StyleSwap is inference-only; run it under torch.no_grad()")
        if _compiling():
            return _ops().style_swap(content_map, style_map, float(alpha), self.normalize)
        return ops.style_swap(content_map, style_map, alpha=alpha, normalize=self.normalize)


def calc_mean_std(feat, eps=1e-5):
    """models.py:54-62: per-(n,c) mean and sqrt(unbiased var + eps)."""
    if feat.dim() != 4:
        raise AssertionError("calc_mean_std expects a 4-D tensor")  # models.py:57
    return Fn.channel_stats(feat, unbiased=True, eps=eps)


def mean_variance_norm(feat):
    """models.py:64-68."""
    return Fn.mean_variance_norm(feat)


class AdaAttN(nn.Module):
    """AdaAttN, models.py:70-115: attention-weighted style mean/std (SURVEY.md §8f "next" #1).

    Same module tree as the reference (W_q/W_k/W_v 1x1 convs without bias, att_act, std_act and
    the three parameter-free InstanceNorm2d), so state dicts load unchanged. forward runs
    ops.adaattn: the Nq x Nk attention matrix is never materialised (one fused HIP kernel). Under
    autograd (fp32, training the reference's AST, train.py:287-300) the backward recomputes the
    attention on the MFMA GEMMs (attention.AdaAttNFn) and yields gradients for W_q, W_k, W_v and
    both inputs.
    """

    def __init__(self, inp_size):
        super().__init__()
        self.W_q = nn.Conv2d(inp_size, inp_size, 1, 1, 0, bias=False)
        self.W_k = nn.Conv2d(inp_size, inp_size, 1, 1, 0, bias=False)
        self.W_v = nn.Conv2d(inp_size, inp_size, 1, 1, 0, bias=False)
        self.att_act = nn.Softmax(dim=-1)
        self.std_act = nn.ReLU(True)
        self.inst_norm_1 = nn.InstanceNorm2d(inp_size)
        self.inst_norm_2 = nn.InstanceNorm2d(inp_size)
        self.inst_norm = nn.InstanceNorm2d(inp_size)
        self.inp_size = inp_size

    def forward(self, content_map, style_map):
        if content_map.shape[1] != self.inp_size:
            raise ops.HipOpError(f"expected {self.inp_size} channels, got {content_map.shape[1]}")
        if torch.is_grad_enabled() and (content_map.requires_grad or style_map.requires_grad
                                        or any(p.requires_grad for p in self.parameters())):
            from . import attention
            return attention.adaattn(self, content_map, style_map)
        return ops.adaattn(content_map, style_map, self.W_q.weight, self.W_k.weight, self.W_v.weight)


def _compiling() -> bool:
    """Under torch.compile / dynamo tracing the modules call torch.ops.ast_hip.* (library.py: the
    same C-ABI kernels behind registered custom ops with fake implementations) and pack weights
    with the ast_hip::conv3x3_pack op instead of the data_ptr-keyed caches, which dynamo cannot
    trace. Eager calls keep the direct C-ABI launches (no dispatcher overhead per launch)."""
    return torch.compiler.is_compiling()


def _ops():
    from . import library  # noqa: F401  (registers the ast_hip::* custom ops)
    return torch.ops.ast_hip


def _luma_transfer(stylised, content_img):
    if _compiling():
        return _ops().luma_transfer(stylised, content_img)
    return ops.luma_transfer(stylised, content_img)


def _color_convert(x, mode):
    """ops.color_convert keeping x's dtype (fp32 -> fp32, bf16 -> bf16)."""
    if _compiling():
        return _ops().color_convert(x, ops.COLOR_MODES[mode], x.dtype == torch.bfloat16)
    return ops.color_convert(x, mode, out_dtype=x.dtype)


def _needs_grad(x, module):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


class Normalization(nn.Module):
    """models.py:120-131. Mean/std are non-persistent buffers: the reference keeps them as plain
    tensors, so they never appear in its state dict."""

    def __init__(self, mean, std):
        super().__init__()
        self.register_buffer("mean", torch.as_tensor(mean, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("std", torch.as_tensor(std, dtype=torch.float32).view(-1, 1, 1), persistent=False)

    def forward(self, img):
        # Off the hot path: PretrainedEncoder fuses this into conv_1's gather.
        return (img - self.mean) / self.std


# --------------------------------------------------------------------------------------------
# VGG19 encoder / loss network
# --------------------------------------------------------------------------------------------

class _Named:
    @staticmethod
    def name(m: nn.Module, n: str) -> nn.Module:
        m.name = n
        return m


class _PackedConvCache:
    """Packed-weight copies of Conv2d modules, refreshed when the parameter changes."""

    def __init__(self):
        self._cache = {}

    def get(self, conv: nn.Conv2d, up2c: bool = False) -> torch.Tensor:
        """up2c: the extended pack (ops.pack_conv3x3), built when and as often as the plain one."""
        w = conv.weight
        key = (id(conv), up2c)
        stamp = (w.data_ptr(), w._version, w.device, ops.weight_epoch(w))
        hit = self._cache.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        packed = ops.pack_conv3x3(w.detach(), up2c=up2c)
        self._cache[key] = (stamp, packed)
        return packed


class PretrainedEncoder(nn.Module):
    """PretrainedEncoder, models.py:186-240: ImageNet normalisation + VGG19 `features` with layers
    named conv_i / relu_i / pool_i (models.py:199-224), returning the requested layers in network
    order and stopping once all are collected (models.py:235-238).

    `_vgg_layers` keeps the reference's ModuleList indices (Normalization at 0, torchvision
    features.N at N+1), so state dicts interchange. Weights: the reference downloads ImageNet
    VGG19 (models.py:192), which is unavailable offline; `weights="live"` (default) uses the
    deterministic live-init recipe (synth.py, seed `seed`), `weights=None` leaves PyTorch's
    default init; load real weights with load_state_dict / load_torchvision_features.

    HIP execution: each conv is one fused launch (conv_1 also applies the normalisation); ReLU and
    2x2 max-pool run in the conv epilogue; the pre-ReLU conv_i taps are dual-stored.
    """

    def __init__(self, content_layers=("conv_1", "conv_3", "conv_5", "conv_9", "conv_13", "relu_15"),
                 weights="live", seed: int = 1):
        super().__init__()
        self._content_layers = set(content_layers)
        norm = _Named.name(Normalization(IMNET_MEAN, IMNET_STD), "norm")
        layers = [norm]
        i, cin = 0, 3
        for v in synth.VGG19_CFG:
            if v == "M":
                layers.append(_Named.name(nn.MaxPool2d(kernel_size=2, stride=2), f"pool_{i}"))
            else:
                i += 1
                layers.append(_Named.name(nn.Conv2d(cin, v, kernel_size=3, padding=1), f"conv_{i}"))
                layers.append(_Named.name(nn.ReLU(inplace=False), f"relu_{i}"))
                cin = v
        self._vgg_layers = nn.ModuleList(layers)
        if weights == "live":
            self.load_live_init(seed)
        self._packed = _PackedConvCache()

    def convs(self):
        return [m for m in self._vgg_layers if isinstance(m, nn.Conv2d)]

    @torch.no_grad()
    def load_live_init(self, seed: int = 1):
        for conv, (w, b) in zip(self.convs(), synth.vgg_encoder_weights(seed)):
            conv.weight.copy_(torch.from_numpy(w))
            conv.bias.copy_(torch.from_numpy(b))

    @torch.no_grad()
    def load_torchvision_features(self, state_dict):
        """Load a torchvision vgg19().features state dict (keys 'N.weight' / 'N.bias')."""
        mapped = {f"_vgg_layers.{int(k.split('.')[0]) + 1}.{k.split('.', 1)[1]}": v for k, v in state_dict.items()}
        self.load_state_dict(mapped)

    def _plan(self):
        """[(conv_index, conv, want_pre, want_act, want_pool, [names collected in order])]."""
        wanted = self._content_layers
        got = set()
        plan = []
        mods = list(self._vgg_layers)
        k = 1
        while k < len(mods) and len(got) < len(wanted):
            conv = mods[k]
            idx = int(conv.name.split("_")[1])
            pool_follows = k + 2 < len(mods) and isinstance(mods[k + 2], nn.MaxPool2d)
            names = [conv.name, f"relu_{idx}"] + ([f"pool_{idx}"] if pool_follows else [])
            collect = [nm for nm in names if nm in wanted]
            got.update(collect)
            more = len(got) < len(wanted)
            want_pre = conv.name in wanted
            want_act = f"relu_{idx}" in wanted or (more and not pool_follows)
            want_pool = pool_follows and (f"pool_{idx}" in wanted or more)
            plan.append((idx, conv, want_pre, want_act, want_pool, collect))
            k += 3 if pool_follows else 2
        return plan

    def forward(self, x, x2=None):
        """Feature maps of the requested layers. `x2` (optional, same C/H/W): a second batch
        encoded in the same launches, outputs hold x's images then x2's."""
        norm = self._vgg_layers[0]
        if _compiling():
            return self._forward_ops(x, x2)
        if _needs_grad(x, self) or (x2 is not None and _needs_grad(x2, self)):
            if x2 is not None:
                return [torch.cat(p) for p in zip(self._forward_autograd(x), self._forward_autograd(x2))]
            return self._forward_autograd(x)
        outs = []
        cur, cur2 = x, x2
        for idx, conv, want_pre, want_act, want_pool, collect in self._plan():
            first = idx == 1
            pre, act, pool = ops.conv3x3(
                cur, self._packed.get(conv), conv.bias, conv.out_channels, pad_mode="zeros",
                in_mean=norm.mean.view(-1) if first else None, in_std=norm.std.view(-1) if first else None,
                want_pre=want_pre, want_act=want_act, want_pool=want_pool, x2=cur2)
            by_name = {conv.name: pre, f"relu_{idx}": act, f"pool_{idx}": pool}
            outs.extend(by_name[nm] for nm in collect)
            cur, cur2 = (pool if want_pool else act), None
        return outs

    def _forward_ops(self, x, x2=None):
        """The same walk through torch.ops.ast_hip.conv3x3 (torch.compile path; with autograd its
        registered backward runs the same HIP dgrad / wgrad kernels)."""
        A = _ops()
        norm = self._vgg_layers[0]
        outs = []
        cur, cur2 = x, x2
        grad = x2 is None and _needs_grad(x, self)
        for idx, conv, want_pre, want_act, want_pool, collect in self._plan():
            first = idx == 1
            pre, act, pool = A.conv3x3(cur, conv.weight, A.conv3x3_pack(conv.weight.detach()), conv.bias, 1, 0,
                                       norm.mean.view(-1) if first else None, norm.std.view(-1) if first else None,
                                       want_pre or grad, want_act, want_pool, cur2)
            by_name = {conv.name: pre, f"relu_{idx}": act, f"pool_{idx}": pool}
            outs.extend(by_name[nm] for nm in collect)
            cur, cur2 = (pool if want_pool else act), None
        return outs

    def prepack(self):
        """Build the forward and input-gradient weight packs of every conv this network runs, ahead
        of a hipGraph capture (train.StepGraph): the loss network is frozen, so its packs are made
        once, outside the graph, instead of being rebuilt by every replay."""
        norm = self._vgg_layers[0]
        for idx, conv, *_ in self._plan():
            self._packed.get(conv)
            Fn._TF.get(conv.weight, norm.std.view(-1) if idx == 1 else None)

    def _forward_autograd(self, x):
        """Same walk through EncoderConvFn (HIP forward + HIP backward; the pre-ReLU output is
        always kept for the ReLU / max-pool backward); frozen weights: one LossNetFn node for the
        whole walk (cross-layer fused backward)."""
        if not any(p.requires_grad for p in self.parameters()):
            return list(Fn.LossNetFn.apply(self, x))
        norm = self._vgg_layers[0]
        outs = []
        cur = x
        for idx, conv, want_pre, want_act, want_pool, collect in self._plan():
            first = idx == 1
            pre, act, pool = Fn.EncoderConvFn.apply(
                cur, conv.weight, conv.bias, self._packed.get(conv), want_act, want_pool,
                norm.mean.view(-1) if first else None, norm.std.view(-1) if first else None)
            by_name = {conv.name: pre, f"relu_{idx}": act, f"pool_{idx}": pool}
            outs.extend(by_name[nm] for nm in collect)
            cur = pool if want_pool else act
        return outs


# --------------------------------------------------------------------------------------------
# Mirrored VGG decoder (models.py:598-628)
# --------------------------------------------------------------------------------------------

class VGGDecoder(nn.Sequential):
    """The mirrored decoder spec at models.py:598-628 (a commented nn.Sequential in the
    reference), with the same Sequential indices so its state dict interchanges. Each
    [Upsample] + ReflectionPad + Conv + [ReLU] group is one fused HIP launch."""

    def __init__(self, weights="live", seed: int = 2):
        layers = []
        for cin, cout, up in synth.VGG_DECODER_SPEC:
            if up:
                layers.append(nn.Upsample(scale_factor=2, mode="nearest"))
            layers += [nn.ReflectionPad2d((1, 1, 1, 1)), nn.Conv2d(cin, cout, (3, 3))]
            if cout != 3:
                layers.append(nn.ReLU())
        super().__init__(*layers)
        self._groups = []
        up = False
        mods = list(self)
        for k, m in enumerate(mods):
            if isinstance(m, nn.Upsample):
                up = True
            elif isinstance(m, nn.Conv2d):
                relu = k + 1 < len(mods) and isinstance(mods[k + 1], nn.ReLU)
                self._groups.append((m, up, relu))
                up = False
        if weights == "live":
            self.load_live_init(seed)
        object.__setattr__(self, "_packed", _PackedConvCache())
        # the upsampled convs take the extended pack: the collapsed 2x2-taps-per-phase kernel (AST_CONV_UP2C=0: 9 taps)
        object.__setattr__(self, "_up2c", ops.up2c_enabled())

    def convs(self):
        return [g[0] for g in self._groups]

    @torch.no_grad()
    def load_live_init(self, seed: int = 2):
        for conv, (w, b) in zip(self.convs(), synth.vgg_decoder_weights(seed)):
            conv.weight.copy_(torch.from_numpy(w))
            conv.bias.copy_(torch.from_numpy(b))

    def forward(self, x):
        # inference (eager and compiled: the same bits) takes the extended pack on the upsampled convs.
        # Under autograd the module keeps plain packs: its forward stays bit-equal to DecoderConvFn
        # layers applied with ops.pack_conv3x3(w) (tests/test_gpu_dgrad_fused.py); DecoderConvFn and
        # the ast_hip::conv3x3 op themselves accept either pack
        if _compiling():
            A = _ops()
            tail = self._up2c and not _needs_grad(x, self)
            for conv, up, relu in self._groups:
                pre, act, _ = A.conv3x3(x, conv.weight, A.conv3x3_pack(conv.weight.detach(), up and tail),
                                        conv.bias, 2 if up else 1, 1, None, None, not relu, relu, False, None)
                x = act if relu else pre
            return x
        if _needs_grad(x, self):
            # each ReLU output feeds only the next conv: its ReLU backward runs in that conv's
            # input-gradient epilogue (mask_input), and the layer itself passes its gradient through
            g = self._groups
            for k, (conv, up, relu) in enumerate(g):
                x = Fn.DecoderConvFn.apply(x, conv.weight, conv.bias, self._packed.get(conv), 2 if up else 1, relu,
                                           k > 0 and g[k - 1][2], relu and k + 1 < len(g))
            return x
        for conv, up, relu in self._groups:
            pre, act, _ = ops.conv3x3(x, self._packed.get(conv, up and self._up2c), conv.bias, conv.out_channels,
                                      upsample=2 if up else 1, pad_mode="reflect",
                                      want_pre=not relu, want_act=relu)
            x = act if relu else pre
        return x


class AutoRegions:
    """Ask a regional method to make its own region maps: `labels=AutoRegions(4)` in place of a uint8
    label map. The style bank's relu4_1 features are clustered into `regions` sub-styles by k-means
    (ops.kmeans: maximin seeds, `iters` Lloyd rounds), every content pixel is assigned to the nearest
    of them (ops.kmeans_assign), and both label maps are smoothed by `smooth` passes of the 3x3 mode
    filter (ops.label_mode_filter) -- the clustering stage of Multimodal Style Transfer (Zhang et
    al., ICCV 2019). normalize=True clusters the per-image ops.mean_variance_norm of the maps, which
    makes content and style features comparable; False the maps themselves. regions in
    1..ops.MAX_REGIONS, iters >= 0, smooth >= 0 (ValueError otherwise); the object is immutable."""

    __slots__ = ("regions", "iters", "smooth", "normalize")

    def __init__(self, regions: int = 3, iters: int = ops.KMEANS_DEFAULT_ITERS, smooth: int = 1,
                 normalize: bool = True):
        def integer(v):
            return isinstance(v, int) and not isinstance(v, bool)
        if not integer(regions) or not 1 <= regions <= ops.MAX_REGIONS:
            raise ValueError(f"regions must be an int in 1..{ops.MAX_REGIONS}, got {regions!r}")
        if not integer(iters) or iters < 0:
            raise ValueError(f"iters must be an int >= 0, got {iters!r}")
        if not integer(smooth) or smooth < 0:
            raise ValueError(f"smooth must be an int >= 0, got {smooth!r}")
        if not isinstance(normalize, bool):
            raise ValueError(f"normalize must be a bool, got {normalize!r}")
        for name, v in (("regions", regions), ("iters", iters), ("smooth", smooth), ("normalize", normalize)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("AutoRegions is immutable")

    def __repr__(self):
        return (f"AutoRegions(regions={self.regions}, iters={self.iters}, smooth={self.smooth}, "
                f"normalize={self.normalize})")


def auto_region_weights(counts):
    """The region weights of AutoRegions from the pixel counts [K, S] of region k in style s (after
    smoothing): (weights float64 CPU [K, S], dead bool [K]). w[k, s] = the count where it is at least
    2, else 0 -- a standard deviation or a covariance needs two pixels. A region whose row is all zero
    is dead: the caller relabels it 255 in both maps, so nothing reads its row, which is set to 1 / S
    to stay a valid mix. Rows are not normalised here (region_weights does that)."""
    c = torch.as_tensor(counts).to(torch.float64).cpu()
    if c.dim() != 2 or c.numel() == 0:
        raise ValueError(f"counts must be a non-empty [K, S] array, got {tuple(c.shape)}")
    w = torch.where(c >= 2, c, torch.zeros_like(c))
    dead = w.sum(dim=1) <= 0
    w[dead] = 1.0 / c.shape[1]
    return w, dead


def _auto_regions(f_c, f_s, auto: AutoRegions):
    """(labels uint8 [N, h, w], style_labels uint8 [S, hs, ws], weights float64 CPU [K, S]) of
    AutoRegions from the relu4_1 maps of the content batch and of the style bank."""
    k = auto.regions
    key_c, key_s = (ops.mean_variance_norm(f_c), ops.mean_variance_norm(f_s)) if auto.normalize else (f_c, f_s)
    cen, sl, _ = ops.kmeans(key_s, k, iters=auto.iters)
    cl = ops.kmeans_assign(key_c, cen)
    if auto.smooth:
        cl = ops.label_mode_filter(cl, k, passes=auto.smooth)
        sl = ops.label_mode_filter(sl, k, passes=auto.smooth)
    every = torch.arange(256, device=sl.device, dtype=torch.uint8)
    ids, none = every[:k], every[255:]

    def counts(maps):                                                 # [maps, K], after smoothing
        return (maps.flatten(1).unsqueeze(1) == ids.view(1, k, 1)).sum(dim=2)

    def relabel(maps, keep):                                          # keep [maps or 1, K]: the others become 255
        lut = torch.cat([torch.where(keep, ids, none), every[k:].expand(keep.shape[0], -1)], dim=1)
        return lut.expand(maps.shape[0], -1).gather(1, maps.flatten(1).long()).view_as(maps)

    w, dead = auto_region_weights(counts(sl).t().cpu())               # the one host synchronisation
    live = ~dead.to(sl.device).unsqueeze(0)
    # a content sample's region of one pixel has no standard deviation either: it passes through too
    return relabel(cl, live & (counts(cl) >= 2)), relabel(sl, live), w


class AdaINStyleTransfer(nn.Module):
    """encoder (VGG19 to relu4_1) -> AdaIN -> alpha blend -> mirrored decoder.

    forward(content_img, style_img, alpha=1.0) -> stylised image [B, 3, H, W]. Content and
    style batches of the same shape are encoded in the same launches. `preserve_color=True`
    (inference only) keeps the content image's colours: the result is ops.luma_transfer(decoder
    output, content_img), the stylised Lab luminance with the content's a and b.
    `transform="efdm"` puts exact feature distribution matching (EFDM) in AdaIN's place, under the
    same attribute name `adain` (what AdaINTrainer calls); the statistics-based methods
    (style_statistics, stylize_with_stats, stylize_regions) then raise NotImplementedError.
    `transform="wct"` puts the whitening and colouring transform (WCT) there in the same way; it is
    inference-only (the forward raises NotImplementedError when a gradient is asked for).
    `stylize_swap` stylises by style swap (patch matching on the relu4_1 maps) with the same
    encoder and decoder, whatever the transform; `stylize_swap_regions` is its guided form over a
    bank of styles, steered by the label maps of `stylize_regions`. `stylize_regions_wct` is
    `stylize_regions` with WCT per region (ops.wct_regions), also whatever the transform, and
    `stylize_regions_efdm` the same with EFDM per region (ops.efdm_regions): the regional method of
    a model trained with transform="efdm".
    The four regional methods take `labels=AutoRegions(k)` in place of label maps: the maps, the
    style maps and the weights then come from a k-means over the style features (`auto_labels`).
    """

    TRANSFORMS = ("adain", "efdm", "wct")

    def __init__(self, canonical: bool = False, enc_seed: int = 1, dec_seed: int = 2, weights="live",
                 transform: str = "adain"):
        super().__init__()
        if transform not in self.TRANSFORMS:
            raise ValueError(f"transform must be one of {self.TRANSFORMS}, got {transform!r}")
        self.transform = transform
        self.encoder = PretrainedEncoder(content_layers=["relu_9"], weights=weights, seed=enc_seed)
        self.adain = {"adain": lambda: AdaIN(canonical=canonical), "efdm": EFDM, "wct": WCT}[transform]()
        self.decoder = VGGDecoder(weights=weights, seed=dec_seed)

    def _needs_statistics(self, what):
        if self.transform != "adain":
            other = ("; stylize_regions_efdm and stylize_regions_wct take the same arguments whatever the transform"
                     if what == "stylize_regions" else "")
            raise NotImplementedError(f"{what} works on per-channel mean and std, which transform="
                                      f"{self.transform!r} does not use; build the model with transform='adain'{other}")

    def encode_pair(self, content_img, style_img):
        if content_img.shape[1:] == style_img.shape[1:]:
            f = self.encoder(content_img, style_img)[0]
            b = content_img.shape[0]
            return f[:b], f[b:]
        return self.encoder(content_img)[0], self.encoder(style_img)[0]

    def _inference_only(self, what, *imgs):
        if torch.is_grad_enabled() and (any(i.requires_grad for i in imgs)
                                        or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(f"{what} is inference-only; run it under torch.no_grad()")

    def _decode(self, t, content_img, preserve_color):
        """The image of the transformed relu4_1 map t; preserve_color: with content_img's colours."""
        out = self.decoder(t)
        if preserve_color:
            return _luma_transfer(out, content_img)
        return out

    def forward(self, content_img, style_img, alpha: float = 1.0, preserve_color: bool = False):
        if preserve_color:
            self._inference_only("preserve_color", content_img, style_img)
        f_c, f_s = self.encode_pair(content_img, style_img)
        return self._decode(self.adain(f_c, f_s, alpha=alpha), content_img, preserve_color)

    def refine(self, content_img, style_img, stylizer, **kw):
        """The feed-forward result polished by optimisation: `stylizer` (strotss.StrotssStylizer) starts
        from self(content_img, style_img) instead of the content image; **kw as its stylize()."""
        with torch.no_grad():
            init = self(content_img, style_img)
        return stylizer.stylize(content_img, style_img, init=init, **kw)

    def stylize_swap(self, content_img, style_img, alpha: float = 1.0, normalize: bool = False,
                     preserve_color: bool = False):
        """Stylise by style swap (StyleSwap on the relu4_1 maps) instead of the model's feature
        transform: the same encoder, decoder and weights, whatever `transform` the model was built
        with. The two images may differ in size (each side at least 24 pixels: a 3x3 relu4_1 map);
        style_img is [N, 3, Hs, Ws] or [1, 3, Hs, Ws]. Inference only; normalize as StyleSwap,
        preserve_color as in forward."""
        self._inference_only("stylize_swap", content_img, style_img)
        f_c, f_s = self.encode_pair(content_img, style_img)
        if _compiling():
            t = _ops().style_swap(f_c, f_s, float(alpha), bool(normalize))
        else:
            t = ops.style_swap(f_c, f_s, alpha=alpha, normalize=bool(normalize))
        return self._decode(t, content_img, preserve_color)

    def auto_labels(self, content_img, style_imgs, auto: AutoRegions = AutoRegions()):
        """The region maps that `labels=auto` gives the regional methods, for content_img [N, 3, H, W]
        and the style bank style_imgs [S, 3, Hs, Ws]: (labels uint8 [N, h, w], style_labels uint8
        [S, hs, ws], weights float64 CPU [K, S]) at relu4_1 resolution, in the form stylize_regions,
        stylize_regions_wct, stylize_regions_efdm and stylize_swap_regions take. The bank's features are clustered together
        (see AutoRegions), so region k is the same sub-style in every map. weights[k, s] is the number
        of pixels of region k in style s after smoothing, 0 below two pixels; a region with no style
        pixels left is relabelled 255 in both maps (its content passes through, its style pixels
        leave the bank) and its row is 1 / S. A region with a single pixel in one content sample is
        relabelled 255 in that sample for the same reason: one pixel has no standard deviation.
        Fetching the style counts is the one host synchronisation. Inference only."""
        self._inference_only("auto_labels", content_img, style_imgs)
        if not isinstance(auto, AutoRegions):
            raise ValueError(f"auto must be an AutoRegions, got {type(auto).__name__}")
        if content_img.dim() != 4 or style_imgs.dim() != 4:
            raise ValueError("auto_labels needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]")
        return _auto_regions(self.encoder(content_img)[0], self.encoder(style_imgs)[0], auto)

    @staticmethod
    def _auto_request(labels, style_labels, weights=None):
        """labels when it is an AutoRegions (style_labels and weights must then be None), else None."""
        if not isinstance(labels, AutoRegions):
            return None
        if style_labels is not None or weights is not None:
            raise ValueError("labels=AutoRegions(...) makes style_labels and weights itself: leave both None")
        return labels

    # -- the front end of the four regional methods. A new one plugs in here: _regional_request, its own
    #    host-side rules, then _regional_inputs (or, without weights, _regional_features), one op, _decode
    def _regional_request(self, what, content_img, style_imgs, labels, style_labels, weights=None):
        """What every regional method checks first: (the AutoRegions request or None, N, S)."""
        self._inference_only(what, content_img, style_imgs)
        if content_img.dim() != 4 or style_imgs.dim() != 4:
            raise ValueError(f"{what} needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]")
        auto = self._auto_request(labels, style_labels, weights)
        return auto, int(content_img.shape[0]), int(style_imgs.shape[0])

    def _regional_features(self, content_img, style_imgs, labels, style_labels, auto):
        """(f_c, f_s, labels, style_labels, weights): both relu4_1 maps, and with an AutoRegions request
        the label maps and weights it makes from them (otherwise the labels as given, weights None)."""
        f_c = self.encoder(content_img)[0]
        f_s = self.encoder(style_imgs)[0]
        if auto is not None:
            return (f_c, f_s) + _auto_regions(f_c, f_s, auto)
        return f_c, f_s, labels, style_labels, None

    def _regional_inputs(self, content_img, style_imgs, labels, style_labels, auto, w):
        """What the weighted regional methods hand their op, after their own host-side rules: (f_c, f_s,
        content labels, style labels or None, w). The label maps are at relu4_1 resolution on the maps'
        device, one region (all 0) when labels is None; w, the [1 or N, K, S] float64 host-side mix of
        region_weights, is the caller's unless an AutoRegions request makes it here."""
        n, s = int(content_img.shape[0]), int(style_imgs.shape[0])
        f_c, f_s, labels, style_labels, weights = self._regional_features(content_img, style_imgs, labels,
                                                                          style_labels, auto)
        if auto is not None:
            w = region_weights(weights, n, s)
        if labels is None:
            lab = torch.zeros((n,) + tuple(f_c.shape[2:]), device=f_c.device, dtype=torch.uint8)
        else:
            lab = _feature_labels(labels, n, content_img.shape[2:], f_c.shape[2:], "labels").to(f_c.device)
        sl = None
        if style_labels is not None:
            sl = _feature_labels(style_labels, s, style_imgs.shape[2:], f_s.shape[2:], "style_labels").to(f_c.device)
        return f_c, f_s, lab, sl, w

    def _regional_mix(self, what, content_img, style_imgs, labels, weights, style_labels):
        """The whole front end of a method whose op mixes the S styles themselves (at most
        ops.MAX_STYLE_ROWS of them): _regional_inputs with the mix as the op takes it, fp32 on the device."""
        auto, n, s = self._regional_request(what, content_img, style_imgs, labels, style_labels, weights)
        if s > ops.MAX_STYLE_ROWS:
            raise ValueError(f"at most {ops.MAX_STYLE_ROWS} styles, got {s}")
        w = None if auto is not None else region_weights(weights, n, s, single_region=labels is None)
        f_c, f_s, lab, sl, w = self._regional_inputs(content_img, style_imgs, labels, style_labels, auto, w)
        return f_c, f_s, lab, sl, w.float().to(f_c.device)

    def stylize_swap_regions(self, content_img, style_imgs, labels=None, style_labels=None, alpha: float = 1.0,
                             normalize: bool = False, preserve_color: bool = False):
        """Guided style swap (ops.style_swap_guided on the relu4_1 maps): content_img [N, 3, H, W]
        takes its patches from the bank of S styles style_imgs [S, 3, Hs, Ws] (shared by the batch),
        steered by the label maps of stylize_regions. Inference only, whatever `transform`.

        labels / style_labels: uint8 [N or S, H, W] (labels also [H, W]), at image or relu4_1
        resolution; a patch has the label of its centre pixel (ops.patch_classes).
        Neither: one class, every content patch takes its best patch from any of the styles.
        labels only: region k takes style k; a label >= S passes the content through.
        Both: a patch labelled k takes its best patch among those labelled k in any style ("sky
        takes sky"); label 255 (any label >= ops.SWAP_MAX_CLASSES) in a style map removes the patch
        from the bank, in the content map it passes the content through.
        style_labels without labels: ValueError. normalize as stylize_swap, preserve_color as forward.
        labels=AutoRegions(...): both maps as auto_labels makes them (style_labels must be None)."""
        auto, n, s = self._regional_request("stylize_swap_regions", content_img, style_imgs, labels, style_labels)
        if style_labels is not None and labels is None:
            raise ValueError("style_labels without labels: give the content's label map too")
        f_c, f_s, labels, style_labels, _ = self._regional_features(content_img, style_imgs, labels, style_labels, auto)
        dev = f_c.device
        if labels is None:
            cc = torch.zeros((n, f_c.shape[2] - 2, f_c.shape[3] - 2), device=dev, dtype=torch.uint8)
        else:
            cc = ops.patch_classes(_feature_labels(labels, n, content_img.shape[2:], f_c.shape[2:], "labels").to(dev))
        if style_labels is not None:
            sc = ops.patch_classes(
                _feature_labels(style_labels, s, style_imgs.shape[2:], f_s.shape[2:], "style_labels").to(dev))
        elif labels is None:
            sc = torch.zeros((s, f_s.shape[2] - 2, f_s.shape[3] - 2), device=dev, dtype=torch.uint8)
        else:
            if s > ops.SWAP_MAX_CLASSES:
                raise ValueError(f"labels alone assign style k to region k: at most {ops.SWAP_MAX_CLASSES} styles, "
                                 f"got {s}")
            sc = torch.arange(s, device=dev, dtype=torch.uint8).view(s, 1, 1).expand(
                s, f_s.shape[2] - 2, f_s.shape[3] - 2).contiguous()
        if _compiling():
            t = _ops().style_swap_guided(f_c, f_s, cc, sc, float(alpha), bool(normalize))
        else:
            t = ops.style_swap_guided(f_c, f_s, cc, sc, alpha=alpha, normalize=bool(normalize))
        return self._decode(t, content_img, preserve_color)

    # -- one style, many contents: the style owner encodes the style once and
    #    broadcasts its relu4_1 statistics (dp.broadcast_style_stats, 2*512 floats) --------------
    def style_statistics(self, style_img):
        """(mean, std) of the style's relu4_1 features, each [N_style, 512]."""
        self._needs_statistics("style_statistics")
        f_s = self.encoder(style_img)[0]
        m, s = channel_stats(f_s)
        return m.flatten(1), s.flatten(1)

    def stylize_with_stats(self, content_img, style_mean, style_std, alpha: float = 1.0,
                           preserve_color: bool = False):
        """Stylise a content batch with given style statistics ([512] shared, or [N, 512]);
        preserve_color as in forward."""
        self._needs_statistics("stylize_with_stats")
        self._inference_only("stylize_with_stats", content_img)
        f_c = self.encoder(content_img)[0]
        t = ops.adain_stats(f_c, style_mean, style_std, alpha=alpha, swap_style_stats=not self.adain.canonical)
        return self._decode(t, content_img, preserve_color)

    # -- several styles: interpolation and / or one mix of styles per region of the content --------
    def stylize_regions(self, content_img, style_imgs, labels=None, weights=None, alpha: float = 1.0,
                        style_labels=None, preserve_color: bool = False):
        """Stylise content_img [N, 3, H, W] with the S styles style_imgs [S, 3, Hs, Ws] (shared by
        the batch), region by region (ops.adain_regions on the relu4_1 maps; inference only).

        labels: uint8 [N, H, W] or [H, W], at image or already at relu4_1 resolution; region k is
        the pixels labelled k, a label >= K (255 by convention) leaves the pixel's features alone.
        None: one region, i.e. plain style interpolation.
        weights: host-side [K, S] or [N, K, S] (nested sequence or CPU tensor), non-negative, each
        row normalised to sum 1: region k moves to the weights[k]-mix of the styles' statistics.
        None: region k takes style k (K = S), or equal weights when labels is None.
        style_labels: uint8 [S, Hs, Ws] with the same region ids: region k then takes the
        statistics of each style's own region k instead of the whole style map (K * S <= 64).
        preserve_color as in forward.
        labels=AutoRegions(...): labels, style_labels and weights as auto_labels makes them from the
        features encoded here (style_labels and weights must be None; K * S <= 64)."""
        self._needs_statistics("stylize_regions")
        auto, n, s = self._regional_request("stylize_regions", content_img, style_imgs, labels, style_labels, weights)
        w = None if auto is not None else region_weights(weights, n, s, single_region=labels is None)
        k = auto.regions if auto is not None else int(w.shape[1])
        if s * (k if style_labels is not None or auto is not None else 1) > ops.MAX_STYLE_ROWS:
            raise ValueError(f"at most {ops.MAX_STYLE_ROWS} rows of style statistics (S, or K * S with style_labels)")
        f_c, f_s, lab, sl, w = self._regional_inputs(content_img, style_imgs, labels, style_labels, auto, w)
        if sl is None:
            mean, std = channel_stats(f_s)
            mean, std = mean.flatten(1), std.flatten(1)                       # [S, C]
            mix = w
        else:
            rm, rs, _ = ops.region_stats(f_s, sl, k)                          # [S, K, C]
            c = int(f_s.shape[1])
            mean = rm.transpose(0, 1).reshape(k * s, c)                       # row k * S + s
            std = rs.transpose(0, 1).reshape(k * s, c)
            mix = torch.zeros((w.shape[0], k, k * s), dtype=torch.float64)    # block-wise: region k reads block k
            for r in range(k):
                mix[:, r, r * s:(r + 1) * s] = w[:, r]
        t = ops.adain_regions(f_c, lab, mean, std, mix.float().to(f_c.device), alpha=alpha,
                              swap_style_stats=not self.adain.canonical)
        return self._decode(t, content_img, preserve_color)

    def stylize_regions_wct(self, content_img, style_imgs, labels=None, weights=None, alpha: float = 1.0,
                            style_labels=None, preserve_color: bool = False, eps_rel: float = ops.WCT_EPS_REL,
                            iters: int = 0):
        """stylize_regions with the whitening and colouring transform (ops.wct_regions on the relu4_1
        maps) in AdaIN's place: region k is whitened with its own covariance and coloured with the
        weights[k]-mix of the styles' covariance roots and means (Li et al. 2017, section 4). Inference
        only, whatever `transform` the model was built with.

        content_img, style_imgs, labels, weights, style_labels, alpha and preserve_color as in
        stylize_regions (labels=None: one region, plain style interpolation; weights=None: region k
        takes style k, or equal weights when labels is None). With style_labels region k takes the
        statistics of each style's own region k; where a style of non-zero weight has fewer than 2
        such pixels, the region keeps the content's features. eps_rel and iters as WCT.
        labels=AutoRegions(...) as in stylize_regions."""
        f_c, f_s, lab, sl, mix = self._regional_mix("stylize_regions_wct", content_img, style_imgs, labels, weights,
                                                    style_labels)
        if _compiling():
            t = _ops().wct_regions(f_c, lab, f_s, mix, sl, float(alpha), float(eps_rel), int(iters))
        else:
            t = ops.wct_regions(f_c, lab, f_s, mix, style_labels=sl, alpha=alpha, eps_rel=eps_rel, iters=iters)
        return self._decode(t, content_img, preserve_color)

    def stylize_regions_efdm(self, content_img, style_imgs, labels=None, weights=None, alpha: float = 1.0,
                             style_labels=None, preserve_color: bool = False):
        """stylize_regions with exact feature distribution matching (ops.efdm_regions on the relu4_1
        maps) in AdaIN's place: in region k the pixel of rank r among the region's own pixels takes
        the weights[k]-mix of the styles' sorted values at the matching quantile, channel by channel
        the Wasserstein barycentre of the styles' distributions. Inference only, whatever `transform`
        the model was built with; it is the regional method of a model trained with transform="efdm".

        content_img, style_imgs, labels, weights, style_labels, alpha and preserve_color as in
        stylize_regions (labels=None: one region, plain style interpolation; weights=None: region k
        takes style k, or equal weights when labels is None). With style_labels region k takes the
        values of each style's own region k; where a style of non-zero weight has no such pixel, the
        region keeps the content's features. relu4_1 maps of at most ops.EFDM_FUSED_MAX pixels (a
        1024 x 1024 image). labels=AutoRegions(...) as in stylize_regions."""
        f_c, f_s, lab, sl, mix = self._regional_mix("stylize_regions_efdm", content_img, style_imgs, labels, weights,
                                                    style_labels)
        if _compiling():
            t = _ops().efdm_regions(f_c, lab, f_s, mix, sl, float(alpha))
        else:
            t = ops.efdm_regions(f_c, lab, f_s, mix, style_labels=sl, alpha=alpha)
        return self._decode(t, content_img, preserve_color)


def region_weights(weights, n: int, s: int, single_region: bool = False):
    """The [1 or N, K, S] float64 CPU mix of stylize_regions from its `weights` argument (None, a
    nested sequence or a CPU tensor of shape [K, S] or [N, K, S]): entries non-negative and finite,
    every row summing to more than 0 (else ValueError), rows normalised to sum 1 in float64."""
    if weights is None:
        if single_region:
            return torch.full((1, 1, s), 1.0 / s, dtype=torch.float64)
        if s > ops.MAX_REGIONS:
            raise ValueError(f"weights=None assigns style k to region k: at most {ops.MAX_REGIONS} styles, got {s}")
        return torch.eye(s, dtype=torch.float64).unsqueeze(0)
    if isinstance(weights, torch.Tensor) and weights.device.type != "cpu":
        raise ValueError("weights are host-side: pass a nested sequence or a CPU tensor")
    try:
        w = torch.as_tensor(weights, dtype=torch.float64)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"weights must be a [K, S] or [N, K, S] array of numbers: {e}") from None
    if w.dim() == 2:
        w = w.unsqueeze(0)
    if w.dim() != 3 or w.shape[2] != s or w.shape[0] not in (1, n) or not 1 <= w.shape[1] <= ops.MAX_REGIONS:
        raise ValueError(f"weights must be [K, S] or [N, K, S] with N={n}, S={s}, K in 1..{ops.MAX_REGIONS}; "
                         f"got {tuple(w.shape)}")
    if single_region and w.shape[1] != 1:
        raise ValueError(f"labels=None is a single region: weights must have K = 1, got K = {w.shape[1]}")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("weights must be finite and non-negative")
    tot = w.sum(dim=2, keepdim=True)
    if bool((tot <= 0).any()):
        raise ValueError("every row of weights must sum to more than 0")
    return w / tot


def _feature_labels(labels, n, img_hw, feat_hw, name):
    """uint8 labels [n, H, W] or [H, W], at image or feature resolution -> [n, h, w] at feature
    resolution (ops.resize_labels when needed)."""
    if not isinstance(labels, torch.Tensor) or labels.dim() not in (2, 3):
        raise ValueError(f"{name} must be a uint8 tensor [N, H, W] or [H, W]")
    if labels.dim() == 2:
        labels = labels.unsqueeze(0).expand(n, -1, -1)
    if labels.shape[0] != n:
        raise ValueError(f"{name} has {labels.shape[0]} maps for a batch of {n}")
    hw, img_hw, feat_hw = tuple(labels.shape[1:]), tuple(img_hw), tuple(feat_hw)
    if hw != feat_hw and hw != img_hw:
        raise ValueError(f"{name} must be at the image resolution {img_hw} or the feature resolution {feat_hw}, "
                         f"got {hw}")
    labels = labels.contiguous()
    if hw == feat_hw:
        return labels
    if _compiling():
        return _ops().resize_labels(labels, feat_hw[0], feat_hw[1])
    return ops.resize_labels(labels, feat_hw[0], feat_hw[1])


# ------------------------------------------------------------------------------------------------
# MobileNet-style variant: Encoder -> per-layer AdaIN -> ada_out ->
# Decoder. Blocks are the DepthWiseConv/conv_3x3_bn mirrors of mobilenetv2.py (HIP forwards).
# ------------------------------------------------------------------------------------------------
from .mobilenetv2 import DTYPE_CODE, DepthWiseConv, SELayer, _make_divisible, act_dtype, check_inference  # noqa: E402,F401
from .mobilenetv2 import _trace_io  # noqa: E402
from .mobilenetv2 import conv_3x3_bn  # noqa: E402,F401
from ._lib import HipOpError, check, lib, ptr, stream_ptr  # noqa: E402


class Encoder(nn.Module):
    """models.py:140-184: conv_3x3_bn + 14 DepthWiseConv blocks from conf.enc_conv_shapes; returns
    the outputs of the blocks listed in out_layers. BatchNorm uses running statistics (eval)."""

    def __init__(self, exporting=False, use_inst_norm=False):
        super().__init__()
        blocks = [conv_3x3_bn(enc_conv_shapes[0][0], enc_conv_shapes[0][1], enc_conv_shapes[0][2])]
        for in_ch, out_ch, stride, kernel_size, expand_ratio in enc_conv_shapes[1:-1]:
            blocks.append(DepthWiseConv(in_ch, out_ch, stride, expand_ratio, use_norm=True, kernel_size=kernel_size))
        # models.py:153: the last block reuses the loop's final (in, out, stride) with EXPAND_RATIO
        blocks.append(DepthWiseConv(in_ch, out_ch, stride, EXPAND_RATIO, use_norm=True))
        self.mob_net = nn.ModuleList(blocks)

    def forward(self, x, out_layers=[], auto_enc=False):
        if auto_enc:
            for layer in self.mob_net:
                x = layer(x)
            return x
        outs = []
        last = max(out_layers) if len(out_layers) else -1   # later blocks cannot change the result
        if self.training and mbtrain.wants_training_path(self, x):
            last = len(self.mob_net) - 1   # train mode: every block runs (BatchNorm running statistics)
        for i, layer in enumerate(self.mob_net):
            if i > last:
                break
            x = layer(x)
            if i in out_layers:
                outs.append(x)
        return outs


class DecoderBlock(nn.Module):
    """models.py:242-272: DepthWiseConv (no BN), then optionally nearest Upsample x2 + ratio-1
    DepthWiseConv (the upsample is fused into that block's depthwise gather)."""

    def __init__(self, in_channels, out_channels, stride, kernel_size=3, upsample=False, expand_ratio=6):
        super().__init__()
        self._ref_pad = nn.ReflectionPad2d((1, 1, 1, 1))
        self._conv = DepthWiseConv(in_channels, out_channels, stride, expand_ratio, use_norm=False,
                                   kernel_size=kernel_size)
        self._should_upsample = upsample
        if self._should_upsample:
            self._ref_out = nn.ReflectionPad2d((1, 1, 1, 1))
            self._upsample_2 = DepthWiseConv(out_channels, out_channels, 1, 1, use_norm=False)
            self._upsample_3 = nn.Upsample(scale_factor=2, mode="nearest")

    def forward(self, x):
        x = self._conv(x)
        if self._should_upsample:
            x = self._upsample_2.run(x, None, up=2)   # training path: explicit upsample, then the block
        return x


class Decoder(nn.Module):
    """models.py:274-320: 14 DecoderBlocks from conf.decoder_conv_shapes (upsample where the
    channel count changes and i + 6 < 15, models.py:284), ReflectionPad + Conv(16->3, bias), and
    Hardtanh(0, 1) only when exporting. Output in the parameters' dtype."""

    def __init__(self, exporting=False):
        super().__init__()
        self.exporting = exporting
        blocks = []
        for i, conv_shape in enumerate(decoder_conv_shapes[:-1]):
            should_upsample = conv_shape[0] != conv_shape[1] and i + 6 < len(decoder_conv_shapes)
            blocks.append(DecoderBlock(conv_shape[0], conv_shape[1], conv_shape[2], upsample=should_upsample,
                                       expand_ratio=conv_shape[4], kernel_size=conv_shape[3]))
        self._decoder_blocks = nn.ModuleList(blocks)
        self._ref_out = nn.ReflectionPad2d((1, 1, 1, 1))
        self._img_out = nn.Conv2d(decoder_conv_shapes[-1][0], decoder_conv_shapes[-1][1], kernel_size=(3, 3))
        self.last_act = nn.Hardtanh(0.0, 1.0)

    def forward(self, x):
        for block in self._decoder_blocks:
            x = block(x)
        return self._image_conv(x)

    def _image_conv(self, x):
        conv = self._img_out
        if mbtrain.wants_training_path(self, x):
            y = Fn.DecoderConvFn.apply(x.float().contiguous(), conv.weight, conv.bias,
                                       ops.pack_conv3x3(conv.weight.detach().float()), 1, False)
            if self.exporting:
                raise NotImplementedError("Hardtanh output under autograd (exporting=True) is inference-only")
            return y
        check_inference(x, self)
        dt = act_dtype(self)
        if x.dtype != dt or x.device.type != "cuda" or x.dim() != 4 or x.shape[1] != conv.in_channels:
            raise HipOpError(f"decoder output conv expects ({conv.in_channels}-channel NCHW {dt} on HIP), "
                             f"got {tuple(x.shape)} {x.dtype} on {x.device}")
        x = x.contiguous()
        n, _, h, w = x.shape
        stamp = (dt, x.device, ops.weight_epoch(conv.weight), ops.weight_epoch(conv.bias), conv.weight._version,
                 conv.bias._version, conv.weight.data_ptr())
        if getattr(self, "_out_stamp", None) != stamp:
            self._w = conv.weight.detach().float().contiguous()
            self._b = conv.bias.detach().float().contiguous()
            self._out_stamp = stamp
        y = torch.empty((n, conv.out_channels, h, w), device=x.device, dtype=dt)
        nbytes = x.numel() * x.element_size() + y.numel() * y.element_size()
        _trace_io(nbytes)
        check(ops._timed("mb dense3x3 out", -nbytes, x.device, lambda: lib().ast_mb_conv3x3_dense(
            DTYPE_CODE[dt], DTYPE_CODE[dt], ptr(x), ptr(self._w), ptr(self._b), ptr(y), n, conv.in_channels,
            conv.out_channels, h, w, 2 if self.exporting else 0, stream_ptr(x.device))), "decoder output conv")
        return y


class AutoEncoder(nn.Module):
    """models.py:322-338: Encoder -> cat(layers 12, 14) -> ada_out -> Decoder."""

    def __init__(self):
        super().__init__()
        self.encoder = Encoder(use_inst_norm=True)
        self.ada_out = DepthWiseConv(enc_out_channels * 2, enc_out_channels, 1, EXPAND_RATIO, use_norm=False,
                                     use_identity=False)
        self.decoder = Decoder()

    def load_live_init(self, enc_seed: int = 5, dec_seed: int = 6, ada_seed: int = 7):
        synth.live_init_(self.encoder, enc_seed)
        synth.live_init_(self.decoder, dec_seed)
        synth.live_init_(self.ada_out, ada_seed)
        return self

    def forward(self, x):
        enc_x = self.encoder(x, out_layers=enc_out_layers)
        return self.decoder(self.ada_out(enc_x[0], enc_x[1]))


class AST(nn.Module):
    """The reference AST (models.py:393-582), MobileNet-variant encoder -> per-layer stylisation
    at enc_out_layers -> ada_out -> decoder.

    The reference class does not run (SyntaxError at models.py:459; ada_att_2 and
    ada_out are used by encode (models.py:557-565) but not defined). This keeps the constructor
    and forward signatures and return values (models.py:395,425,529-533) and the encode structure
    (models.py:535-566). `attention=False` (default, the north-star path) stylises each layer with
    AdaIN(content_i, style_i); `attention=True` uses the reference's own choice, AdaAttN modules
    `ada_att_1` / `ada_att_2` (models.py:407-408, 557-558), each over enc_out_channels.
    `lab_io=True` (with exporting=True only) is the reading of the commented models.py:427-429 and
    529: both images go through rgb2lab on the way in and the result through lab2rgb on the way
    out, in the tensors' own dtype (bf16 models: the bf16 -> bf16 colour kernels).
    Train mode with autograd (ASTTrainer, train.py:146-300) runs the training kernels: the
    detached eval-mode encoding of encode(detach=True), AdaAttN / ada_out / decoder with backward,
    and the train-mode (batch statistics) content encoding feeding org_out, as models.py:425-476.
    """

    def __init__(self, style_layers=[4, 7, 10, 12, 16], content_layers=[4, 7, 10, 12, 16], exporting=False,
                 attention=False, lab_io=False):
        super().__init__()
        if lab_io and not exporting:
            raise ValueError("lab_io=True needs exporting=True: the reference converts to Lab and back only "
                             "on its exporting path (models.py:427-429, 529)")
        self._lab_io = lab_io
        self._style_layers = style_layers
        self._content_layers = content_layers
        self._exporting = exporting
        self._enc = Encoder(self._exporting)
        self._dec = Decoder(self._exporting)
        self._attention = attention
        if attention:
            self.ada_att_1 = AdaAttN(enc_out_channels)
            self.ada_att_2 = AdaAttN(enc_out_channels)
        else:
            self._adain = AdaIN()
        self.ada_out = DepthWiseConv(enc_out_channels * 2, enc_out_channels, 1, EXPAND_RATIO, use_norm=False,
                                     use_identity=False)

    def load_live_init(self, enc_seed: int = 5, dec_seed: int = 6, ada_seed: int = 7, att_seed: int = 8):
        synth.live_init_(self._enc, enc_seed)
        synth.live_init_(self._dec, dec_seed)
        synth.live_init_(self.ada_out, ada_seed)
        if self._attention:
            synth.live_init_(self.ada_att_1, att_seed)
            synth.live_init_(self.ada_att_2, att_seed + 1)
        return self

    def stylize_maps(self, content_maps, style_maps):
        """Per-layer stylisation of the enc_out_layers maps (models.py:557-558)."""
        if self._attention:
            return self.ada_att_1(content_maps[0], style_maps[0]), self.ada_att_2(content_maps[1], style_maps[1])
        for m in content_maps:     # AdaIN reads content + style and writes its output
            _trace_io(3 * m.numel() * m.element_size())
        return self._adain(content_maps[0], style_maps[0]), self._adain(content_maps[1], style_maps[1])

    def encode(self, content_img, style_img, detach=False, return_maps=False):
        """models.py:535-566. detach=True: the encoder runs in eval mode (running statistics) and its
        maps are detached (models.py:537-545), so it runs here without recording autograd."""
        if detach:
            was = self._enc.training
            self._enc.eval()
            with torch.no_grad():
                content_maps = self._enc(content_img, out_layers=enc_out_layers)
                style_maps = self._enc(style_img, out_layers=enc_out_layers)
            self._enc.train(was)
        else:
            content_maps = self._enc(content_img, out_layers=enc_out_layers)
            style_maps = self._enc(style_img, out_layers=enc_out_layers)
        st1, st2 = self.stylize_maps(content_maps, style_maps)
        stylized_map = self.ada_out(st1, st2)
        self._last_content_maps = content_maps
        if return_maps:
            return st1, st2, stylized_map
        return stylized_map

    def forward(self, content_img, style_img, alpha=1.0):
        """models.py:425-533: t_cs when exporting, else (t_cs, t_return, org_out).

        t_return = (stylized_map_1, stylized_map_2), the per-layer stylised maps: train.py:276-277
        pairs t[i] with the stylised image's encoding at each of enc_out_layers, and calc_mean_std
        asserts 4-D maps (models.py:57), so this is the reading of the unparsable models.py:459
         under which the reference's training loop runs."""
        if self._exporting:
            if self._lab_io:   # models.py:427-429: the network sees Lab images, in their own dtype
                content_img = _color_convert(content_img, "rgb2lab")
                style_img = _color_convert(style_img, "rgb2lab")
            t = self.encode(content_img, style_img)
            self._last_content_maps = None
            t_cs = self._dec(t)
            if self._lab_io:   # models.py:529
                t_cs = _color_convert(t_cs, "lab2rgb")
            return t_cs
        st1, st2, t = self.encode(content_img, style_img, detach=True, return_maps=True)
        if self.training:
            # train mode: the content encoding for org_out uses batch statistics (and updates the
            # running ones), as the reference's second encoder call does (models.py:466-469)
            c = self._enc(content_img, out_layers=enc_out_layers)
        else:
            c = self._last_content_maps    # eval mode: the same maps encode() just computed
        self._last_content_maps = None
        content_map = self.ada_out(c[0], c[1])
        if alpha != 1.0:
            t = alpha * t + (1 - alpha) * content_map
        org_out = self._dec(content_map)
        t_cs = self._dec(t)
        return t_cs, (st1, st2), org_out
