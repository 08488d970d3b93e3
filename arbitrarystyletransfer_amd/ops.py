"""Functional wrappers over the HIP kernels (C ABI in include/ast_hip.h).

Each op takes device tensors, checks shapes/dtypes on the host (a kernel is never launched on a
shape it does not support), allocates outputs with the PyTorch caching allocator and enqueues the
kernel on the current HIP stream. No host synchronisation, so sequences of ops can be captured
into a hipGraph. CPU tensors raise: there is no CPU fallback in the product path.
"""
from __future__ import annotations

import os

import torch

from ._lib import HipOpError, check, lib, loss_accumulator, ptr, stream_ptr

PAD_MODES = {"zeros": 0, "reflect": 1}

# Bumped by optimizers that update parameters through raw pointers (optim.FusedAdam), which
# torch's per-tensor _version counter cannot see; weight-pack caches key on it. Per parameter
# (`_ast_epoch`), so the packs of frozen weights (the VGG loss network) survive optimizer steps.
WEIGHTS_EPOCH = [0]


def bump_weights_epoch(params=None):
    WEIGHTS_EPOCH[0] += 1
    for p in params or ():
        p._ast_epoch = getattr(p, "_ast_epoch", 0) + 1


def weight_epoch(t) -> int:
    """The update count of parameter t by raw-pointer optimizers (cache keys)."""
    return getattr(t, "_ast_epoch", 0)


class LaunchTimer:
    """Records a pair of HIP events around every conv3x3 launch, on the launch stream, while
    active (bench.py's live roofline measurement). Use as a context manager."""

    active = None

    def __init__(self):
        self.records = []  # (tag, flops, start_event, end_event)

    def __enter__(self):
        LaunchTimer.active = self
        return self

    def __exit__(self, *exc):
        LaunchTimer.active = None

    def results(self):
        """[(tag, flops, milliseconds)] — call after synchronising the device."""
        return [(tag, fl, s.elapsed_time(e)) for tag, fl, s, e in self.records]


def _timed(tag, flops, device, launch):
    t = LaunchTimer.active
    if t is None:
        return launch()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream(device)
    s.record(stream)
    code = launch()
    e.record(stream)
    t.records.append((tag, flops, s, e))
    return code


# ------------------------------------------------------------------------------------------------
# Argument checks shared by the ops. A new op composes these and adds only its own limits after them:
# _dev / _dev_typed (the device gate: every tensor argument passes it first), _pair (two NCHW maps),
# _map_and_labels / _labels (a map and its uint8 label map), _style_bank (the bank, mix and labels of a
# regional transform) and _like (a tensor that must look like one the library made: state, index, out).
# ------------------------------------------------------------------------------------------------

def _dev_typed(t: torch.Tensor, name: str, dtype: torch.dtype) -> torch.Tensor:
    """The device gate: t, a `dtype` tensor on a HIP device, made contiguous."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device.type != "cuda":
        raise HipOpError(f"{name} is on {t.device}; arbitrarystyletransfer_amd runs on MI355X (HIP) devices only")
    if t.dtype != dtype:
        raise HipOpError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    return _dev_typed(t, name, torch.float32)


def _like(t, device, dtype, what: str, shape=None, numel=None, msg=None) -> torch.Tensor:
    """t, which must be a `dtype` tensor on `device` of the given shape (or, with shape None, of `numel`
    elements), made contiguous. msg replaces the message where several tensors share one."""
    if (not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype
            or (tuple(t.shape) != tuple(shape) if shape is not None else t.numel() != numel)):
        size = tuple(shape) if shape is not None else f"of {numel} elements"
        raise HipOpError(msg or f"{what} must be a {dtype} tensor {size} on {device}")
    return t.contiguous()


def _pair(a: torch.Tensor, b: torch.Tensor, na: str, nb: str, what: str, batch: bool = True, side: int = 1,
          named: bool = True):
    """Two fp32 NCHW maps on one device, not empty, with equal C; batch: b's batch is a's or 1; side: the
    least height and width (3 where 3x3 patches are taken); named: the message names the two shapes.
    (a, b, n, nb, c, ha, wa, hb, wb)."""
    a, b = _dev(a, na), _dev(b, nb)
    if (a.dim() != 4 or b.dim() != 4 or a.shape[1] != b.shape[1] or (batch and b.shape[0] not in (1, a.shape[0]))
            or a.numel() == 0 or b.numel() == 0 or min(a.shape[2:]) < side or min(b.shape[2:]) < side):
        needs = ["equal C"] + ([f"sides of at least {side}"] if side > 1 else []) + (
            ["a style batch of N or 1"] if batch else [])
        needs = " and ".join(filter(None, [", ".join(needs[:-1]), needs[-1]]))
        la, lb = (f"{na} ", f"{nb} ") if named else ("", "")
        raise HipOpError(f"{what} needs non-empty NCHW maps with {needs}: "
                         f"{la}{tuple(a.shape)} vs {lb}{tuple(b.shape)}")
    if a.device != b.device:
        raise HipOpError(f"{nb} is on {b.device}, {na} on {a.device}")
    n, c, ha, wa = (int(s) for s in a.shape)
    return a, b, n, int(b.shape[0]), c, ha, wa, int(b.shape[2]), int(b.shape[3])


# ------------------------------------------------------------------------------------------------
# 3x3 convolution
# ------------------------------------------------------------------------------------------------

_TUNING = None


def tuned_config(n, cin, h_in, w_in, cout, up, pad_mode, pool, kind="") -> int:
    """Kernel configuration measured fastest for this shape (scripts/tune_conv.py writes
    conv_tuning.json); -1 (the library's own heuristic) for shapes never tuned. `kind` separates
    launches of the same GEMM shape with another epilogue (" dgrad": the input-gradient conv of
    ast_conv3x3_dgrad_f32, " dgrad sum2" with its 2x2-sum upsample adjoint), timed on their own."""
    global _TUNING
    if _TUNING is None:
        import json
        import os
        path = os.environ.get("AST_CONV_TUNING") or os.path.join(  # override: A/B of tuning tables
            os.path.dirname(os.path.abspath(__file__)), "conv_tuning.json")
        try:
            with open(path) as f:
                _TUNING = json.load(f)
        except (OSError, ValueError):
            _TUNING = {}
    k = f"{n}x{cin}x{h_in}x{w_in}->{cout} up{up} {pad_mode}{' pool' if pool else ''}{kind}"
    return int(_TUNING.get(k, -1))


_UP2C = None


def up2c_enabled() -> bool:
    """AST_CONV_UP2C=0: the model packs its upsampled decoder convs without the collapsed slab, so
    they run the 9-tap kernel (A/B runs). Read once per process."""
    global _UP2C
    if _UP2C is None:
        _UP2C = os.environ.get("AST_CONV_UP2C", "1") != "0"
    return _UP2C


def pack_conv3x3(weight: torch.Tensor, up2c: bool = False) -> torch.Tensor:
    """Repack a [cout, cin, 3, 3] filter bank into the kernel's [cin_pad][9][cout_pad] layout.
    up2c: the extended pack -- the usual one with the collapsed slab of the upsampled reflect-pad
    conv (2x2 taps per output phase, csrc/conv_up2c.hip) appended; conv3x3 accepts either."""
    w = _dev(weight, "weight")
    if w.dim() != 4 or w.shape[2:] != (3, 3):
        raise HipOpError(f"conv3x3 weight must be [cout, cin, 3, 3], got {tuple(w.shape)}")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    L = lib()
    base = int(L.ast_conv3x3_packed_numel(cout, cin))
    tail = int(L.ast_conv3x3_up2c_numel(cout, cin)) if up2c else 0
    out = torch.empty(base + tail, device=w.device, dtype=torch.float32)
    check(L.ast_conv3x3_pack_weights_f32(ptr(w), ptr(out), cout, cin, stream_ptr(w.device)), "pack_conv3x3")
    if up2c:
        check(L.ast_conv3x3_pack_up2c_f32(ptr(out), ptr(out[base:]), cout, cin, stream_ptr(w.device)),
              "pack_conv3x3 up2c")
    return out


def pack_plan(n: int, w: int, pool: bool):
    """(G, gap) for side-by-side packing of n planes of width w (csrc/pack.hip): the group size
    that best fills the conv kernel's 32-pixel MFMA row tiles, if it gains >= 15%; (1, 0) else."""
    if os.environ.get("AST_CONV_PACK", "1") == "0" or n < 2 or w > 64 or (pool and w % 2):
        return 1, 0
    gap = 2 if pool else 1
    base = w / (-(-w // 32) * 32)
    best_u, best_g = base, 1
    for g in range(2, min(n, 8) + 1):
        wp = g * (w + gap) - gap
        u = n * w / (-(-n // g) * (-(-wp // 32) * 32))
        if u > best_u * 1.0001:
            best_u, best_g = u, g
    return (best_g, gap) if best_u >= 1.15 * base else (1, 0)


def conv3x3(x: torch.Tensor, w_packed: torch.Tensor, bias, cout: int, *, upsample: int = 1,
            pad_mode: str = "zeros", in_mean=None, in_std=None,
            want_pre: bool = False, want_act: bool = True, want_pool: bool = False, cfg: int = -1,
            x2: torch.Tensor | None = None, _pack: bool = True, _flops=None, _up2c_tile: int = 0):
    """Fused [Upsample x2] -> pad(1) -> Conv3x3 -> (+bias) -> {pre, ReLU, ReLU+MaxPool2x2}.

    x2 (optional): a second batch with x's C, H, W; outputs hold x's images then x2's (one
    launch for a content batch and a style batch, no concatenation copy).
    Returns (pre, act, pool) with None for outputs not requested.
    _up2c_tile (tests): the collapsed kernel's form, 8 or 4 waves (0: the library's choice).
    """
    x = _dev(x, "x")
    if x.dim() != 4:
        raise HipOpError(f"x must be NCHW, got {tuple(x.shape)}")
    n1, cin, h_in, w_in = (int(s) for s in x.shape)
    n2 = 0
    if x2 is not None:
        x2 = _dev(x2, "x2")
        if x2.dim() != 4 or tuple(x2.shape[1:]) != tuple(x.shape[1:]) or x2.device != x.device:
            raise HipOpError(f"x2 {tuple(x2.shape)} must match x {tuple(x.shape)} in C, H, W")
        n2 = int(x2.shape[0])
    n = n1 + n2
    base = int(lib().ast_conv3x3_packed_numel(cout, cin))
    has_tail = w_packed.numel() == base + int(lib().ast_conv3x3_up2c_numel(cout, cin))   # extended pack
    if w_packed.numel() != base and not has_tail:
        raise HipOpError("packed weight does not match (cout, cin)")
    if bias is not None:
        bias = _dev(bias, "bias")
        if bias.numel() != cout:
            raise HipOpError("bias size mismatch")
    if (in_mean is None) != (in_std is None):
        raise HipOpError("in_mean and in_std go together")
    if in_mean is not None:
        in_mean, in_std = _dev(in_mean, "in_mean"), _dev(in_std, "in_std")
        if in_mean.numel() != cin or in_std.numel() != cin:
            raise HipOpError("normalisation stats must have cin entries")
    if pad_mode not in PAD_MODES:
        raise HipOpError(f"pad_mode must be one of {list(PAD_MODES)}")
    H, W = h_in * upsample, w_in * upsample
    mk = lambda hh, ww: torch.empty((n, cout, hh, ww), device=x.device, dtype=torch.float32)  # noqa: E731
    pre = mk(H, W) if want_pre else None
    act = mk(H, W) if want_act else None
    pool = mk(H // 2, W // 2) if want_pool else None
    if pool is not None and (H < 2 or W < 2):
        raise HipOpError("max-pool needs H, W >= 2")
    if pre is None and act is None and pool is None:
        raise HipOpError("conv3x3: no output requested")
    # the collapsed slab of an extended pack: 2x2 taps per output phase (4 products per output, not 9)
    up2c = (has_tail and upsample == 2 and pad_mode == "reflect" and not want_pool and cin >= 16
            and in_mean is None and cfg < 0)
    if cfg < 0:
        cfg = tuned_config(n, cin, h_in, w_in, cout, upsample, pad_mode, want_pool)
    G, gap = pack_plan(n, w_in, want_pool) if (_pack and pad_mode == "zeros" and upsample == 1
                                                and in_mean is None) else (1, 0)
    if G > 1:   # small planes: G images side by side per row band (identical results, fuller tiles)
        L = lib()
        ng, wp = -(-n // G), G * (w_in + gap) - gap
        xp = torch.empty((ng, cin, h_in, wp), device=x.device, dtype=torch.float32)
        check(L.ast_pack_images_f32(ptr(x), n1, ptr(x2), n2, cin, h_in, w_in, G, gap, ptr(xp),
                                    stream_ptr(x.device)), "pack")
        outs = conv3x3(xp, w_packed, bias, cout, want_pre=want_pre, want_act=want_act, want_pool=want_pool,
                       cfg=cfg, _pack=False, _flops=2 * n * H * W * cout * cin * 9)
        res = []
        for t, full, hh, ww in ((outs[0], pre, H, W), (outs[1], act, H, W), (outs[2], pool, H // 2, W // 2)):
            if t is not None:
                sp, wpp = (w_in + gap, wp) if hh == H else ((w_in + gap) // 2, wp // 2)
                check(L.ast_unpack_images_f32(ptr(t), n, cout, hh, ww, G, sp, wpp, ptr(full), stream_ptr(x.device)),
                      "unpack")
            res.append(full if t is not None else None)
        return tuple(res)
    flops = _flops if _flops is not None else 2 * n * H * W * cout * cin * 9   # algorithmic (9 taps)
    tag = f"conv3x3 {cin}->{cout} {H}x{W} up{upsample} {pad_mode}"
    if _up2c_tile and not up2c:
        raise HipOpError("_up2c_tile: this call does not run the collapsed kernel")
    if up2c:
        code = _timed(tag, flops, x.device, lambda: lib().ast_conv3x3_up2c_fwd_f32_cfg(
            _up2c_tile, ptr(x), ptr(x2), n2, ptr(w_packed[base:]), ptr(bias), ptr(pre), ptr(act), n1, cin, h_in, w_in, cout,
            upsample, PAD_MODES[pad_mode], stream_ptr(x.device)))
        check(code, "conv3x3 up2c")
        return pre, act, pool
    code = _timed(tag, flops, x.device, lambda: lib().ast_conv3x3_fwd_f32_cfg(
        cfg, ptr(x), ptr(x2), n2, ptr(w_packed), ptr(bias), ptr(pre), ptr(act), ptr(pool), ptr(in_mean),
        ptr(in_std), n1, cin, h_in, w_in, cout, upsample, PAD_MODES[pad_mode], stream_ptr(x.device)))
    check(code, "conv3x3")
    return pre, act, pool


# ------------------------------------------------------------------------------------------------
# Statistics / AdaIN
# ------------------------------------------------------------------------------------------------

def channel_stats(x: torch.Tensor, unbiased: bool = True, eps: float = 0.0):
    """Per-(n, c) mean and std over H, W, keepdim (model_util.py:3-8; calc_mean_std with eps)."""
    x = _dev(x, "x")
    if x.dim() != 4:
        raise HipOpError("channel_stats expects NCHW")
    n, c, h, w = x.shape
    mean = torch.empty((n, c, 1, 1), device=x.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    check(lib().ast_channel_stats_f32(ptr(x), ptr(mean), ptr(std), n * c, h * w, 1 if unbiased else 0,
                                      float(eps), stream_ptr(x.device)), "channel_stats")
    return mean, std


def adain(content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0, swap_style_stats: bool = True):
    """AdaIN (models.py:43-51) fused with the alpha blend of models.py:471."""
    if isinstance(content, torch.Tensor) and content.dtype == torch.bfloat16:
        return adain_bf16(content, style, alpha, swap_style_stats)
    content = _dev(content, "content_map")
    style = _dev(style, "style_map")
    if content.dim() != 4 or style.dim() != 4 or content.shape[:2] != style.shape[:2]:
        raise HipOpError(f"AdaIN needs NCHW maps with equal (N, C): {tuple(content.shape)} vs {tuple(style.shape)}")
    n, c, hc, wc = (int(s) for s in content.shape)
    hs, ws = int(style.shape[2]), int(style.shape[3])
    out = torch.empty_like(content)
    nbytes = 4 * (2 * content.numel() + style.numel())  # algorithmic: read c, read s, write out
    check(_timed(f"adain {c}ch {hc}x{wc}", -nbytes, content.device, lambda: lib().ast_adain_f32(
        ptr(content), ptr(style), ptr(out), n, c, hc, wc, hs, ws, float(alpha), 1 if swap_style_stats else 0,
        stream_ptr(content.device))), "adain")
    return out


def adain_stats(content: torch.Tensor, style_mean: torch.Tensor, style_std: torch.Tensor, alpha: float = 1.0,
                swap_style_stats: bool = True):
    """AdaIN of `content` [N, C, H, W] against given style statistics: [C] (one style shared by
    the batch) or [N, C] (any trailing 1-dims allowed), std unbiased as channel_stats."""
    content = _dev(content, "content_map")
    n, c, hc, wc = (int(s) for s in content.shape)
    m = _dev(style_mean, "style_mean").reshape(-1)
    s = _dev(style_std, "style_std").reshape(-1)
    if m.numel() != s.numel() or m.numel() not in (c, n * c):
        raise HipOpError(f"style statistics must have C={c} or N*C={n * c} entries, got {m.numel()}")
    out = torch.empty_like(content)
    check(lib().ast_adain_stats_f32(ptr(content), ptr(m), ptr(s), ptr(out), n, c, hc, wc,
                                    0 if m.numel() == c else c, float(alpha), 1 if swap_style_stats else 0,
                                    stream_ptr(content.device)), "adain_stats")
    return out


# Regional multi-style AdaIN (csrc/adain_regions.hip): AST_MAX_REGIONS / AST_MAX_STYLE_ROWS of ast_hip.h
MAX_REGIONS = 8
MAX_STYLE_ROWS = 64


def _uint8_first(t, name: str):
    """A label map of another dtype hears about its dtype before its device (a host-side int map is the
    usual mistake), and in _map_and_labels before anything about the map it goes with."""
    if isinstance(t, torch.Tensor) and t.dtype != torch.uint8:
        raise HipOpError(f"{name} must be uint8, got {t.dtype}")
    return t


def _labels(t: torch.Tensor, name: str, dtype_checked: bool = False) -> torch.Tensor:
    t = _dev_typed(t if dtype_checked else _uint8_first(t, name), name, torch.uint8)
    if t.dim() != 3 or t.numel() == 0:
        raise HipOpError(f"{name} must be a non-empty [N, H, W] uint8 map, got {tuple(t.shape)}")
    return t


def _regions(regions) -> int:
    if isinstance(regions, bool) or not isinstance(regions, int) or not 1 <= regions <= MAX_REGIONS:
        raise HipOpError(f"regions must be an int in 1..{MAX_REGIONS}, got {regions!r}")
    return regions


def resize_labels(labels: torch.Tensor, h: int, w: int):
    """Nearest-neighbour resize of uint8 label maps [N, H, W] to [N, h, w]: src = (dst * in) // out
    per axis, the pixel F.interpolate(mode="nearest") picks."""
    labels = _labels(labels, "labels")
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise HipOpError(f"resize_labels needs a positive size, got {(h, w)}")
    n, hs, ws = (int(s) for s in labels.shape)
    out = torch.empty((n, h, w), device=labels.device, dtype=torch.uint8)
    check(lib().ast_resize_labels_u8(ptr(labels), ptr(out), n, hs, ws, h, w, stream_ptr(labels.device)),
          "resize_labels")
    return out


def _map_and_labels(x, labels, what):
    labels = _uint8_first(labels, "labels")
    x = _dev(x, what)
    labels = _labels(labels, "labels", dtype_checked=True)
    if x.dim() != 4 or x.numel() == 0:
        raise HipOpError(f"{what} must be a non-empty NCHW map, got {tuple(x.shape)}")
    n, c, h, w = (int(s) for s in x.shape)
    if tuple(labels.shape) != (n, h, w) or labels.device != x.device:
        raise HipOpError(f"labels must be [N, H, W] = {(n, h, w)} on {x.device}, got {tuple(labels.shape)} "
                         f"on {labels.device}")
    return x, labels, n, c, h, w


def region_stats(x: torch.Tensor, labels: torch.Tensor, regions: int):
    """Per-region channel statistics of x [N, C, H, W] under labels [N, H, W] (uint8; a label
    >= regions belongs to no region): mean and unbiased std [N, regions, C] and pixel counts
    [N, regions] (int32). An empty region has NaN mean and std, a one-pixel region NaN std."""
    regions = _regions(regions)
    x, labels, n, c, h, w = _map_and_labels(x, labels, "x")
    mean = torch.empty((n, regions, c), device=x.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    count = torch.empty((n, regions), device=x.device, dtype=torch.int32)
    check(lib().ast_region_stats_f32(ptr(x), ptr(labels), ptr(mean), ptr(std), ptr(count), n, c, h, w, regions,
                                     stream_ptr(x.device)), "region_stats")
    return mean, std, count


def adain_regions(content: torch.Tensor, labels: torch.Tensor, style_mean: torch.Tensor, style_std: torch.Tensor,
                  mix: torch.Tensor, alpha: float = 1.0, swap_style_stats: bool = True):
    """Regional multi-style AdaIN in one launch. Region k of sample n (the pixels with
    labels[n] == k) is normalised with its own statistics and moved to the mix
    sum_t mix[n, k, t] * (style_mean, style_std)[t] of the rows of a style-statistics table [T, C];
    pixels labelled >= K pass through bit for bit. mix is [K, T] or [1, K, T] (shared by the batch)
    or [N, K, T]; rows with weight exactly 0 are skipped. alpha and swap_style_stats as adain_stats."""
    content, labels, n, c, h, w = _map_and_labels(content, labels, "content_map")
    m, s, mix = _dev(style_mean, "style_mean"), _dev(style_std, "style_std"), _dev(mix, "mix")
    if m.dim() != 2 or m.shape != s.shape or m.shape[1] != c or not 1 <= m.shape[0] <= MAX_STYLE_ROWS:
        raise HipOpError(f"style statistics must be two [T, C={c}] tables with T in 1..{MAX_STYLE_ROWS}, got "
                         f"{tuple(m.shape)} and {tuple(s.shape)}")
    rows = int(m.shape[0])
    if mix.dim() == 2:
        mix = mix.unsqueeze(0)
    if mix.dim() != 3 or mix.shape[0] not in (1, n) or not 1 <= mix.shape[1] <= MAX_REGIONS or mix.shape[2] != rows:
        raise HipOpError(f"mix must be [N={n} or 1, K <= {MAX_REGIONS}, T={rows}], got {tuple(mix.shape)}")
    regions = int(mix.shape[1])
    shared = mix.shape[0] == 1   # one sample: either stride reads the same row
    out = torch.empty_like(content)
    nbytes = 4 * 2 * content.numel() + labels.numel()   # algorithmic: read c and the label map, write out
    check(_timed(f"adain_regions {c}ch {h}x{w} K{regions}", -nbytes, content.device,
                 lambda: lib().ast_adain_regions_f32(
                     ptr(content), ptr(labels), ptr(m), ptr(s), ptr(mix), ptr(out), n, c, h, w, regions, rows,
                     0 if shared else regions * rows, float(alpha), 1 if swap_style_stats else 0,
                     stream_ptr(content.device))), "adain_regions")
    return out


# Exact feature distribution matching and the plane sort (csrc/efdm.hip): AST_EFDM_FUSED_MAX of ast_hip.h,
# the largest plane (of either map) that the one-launch, no-workspace path takes
EFDM_FUSED_MAX = 16384


def _ws_bytes(nbytes: int, what: str, device):
    """The device workspace of a *_workspace_bytes query (None for 0; a negative query is its error)."""
    if nbytes < 0:
        check(int(nbytes), what)
    return torch.empty((int(nbytes),), device=device, dtype=torch.uint8) if nbytes else None


def efdm(content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0, _chunk: int = 0):
    """Exact feature distribution matching (Zhang et al., CVPR 2022), a drop-in for adain: in every
    (n, c) plane the content element of rank r (stable ascending, floats in IEEE totalOrder of
    their bits) takes the style plane's sorted value S[((2r + 1) * Ms) // (2 * Mc)]. At alpha == 1
    every output is a copy of a style value; otherwise c + alpha * (t - c).
    content [N, C, Hc, Wc]; style [N, C, Hs, Ws] or [1, C, Hs, Ws] (shared by the batch).
    _chunk (tests): a power of two >= 64 forces the chunk-sort + merge path with that LDS chunk."""
    content, style, n, ns, c, hc, wc, hs, ws = _pair(content, style, "content_map", "style_map", "EFDM", named=False)
    L = lib()
    nbytes = int(L.ast_efdm_ex_workspace_bytes(n, ns, c, hc * wc, hs * ws, int(_chunk)))
    wsb = _ws_bytes(nbytes, "efdm workspace", content.device)
    out = torch.empty_like(content)
    algo = 4 * (2 * content.numel() + n * c * hs * ws)   # algorithmic: read c, read s, write out
    check(_timed(f"efdm {c}ch {hc}x{wc}", -algo, content.device, lambda: L.ast_efdm_ex_f32(
        ptr(content), ptr(style), ptr(out), n, ns, c, hc, wc, hs, ws, float(alpha), int(_chunk), ptr(wsb),
        max(nbytes, 0), stream_ptr(content.device))), "efdm")
    return out


def plane_sort(x: torch.Tensor, return_index: bool = False, _chunk: int = 0):
    """Every plane of x (all dimensions after the first two flattened; a 2-D x is [planes, M])
    sorted ascending in IEEE totalOrder of the bits (-0 < +0, negative NaNs first, positive NaNs
    last), ties in index order: the sorted values in x's shape and, with return_index, the int32
    index of each value within its plane."""
    x = _dev(x, "x")
    if x.dim() < 2 or x.numel() == 0:
        raise HipOpError(f"plane_sort needs a non-empty [planes, M] or [N, C, ...] tensor, got {tuple(x.shape)}")
    planes = int(x.shape[0]) if x.dim() == 2 else int(x.shape[0] * x.shape[1])
    m = x.numel() // planes
    L = lib()
    nbytes = int(L.ast_plane_sort_workspace_bytes(planes, m, 1 if return_index else 0, int(_chunk)))
    wsb = _ws_bytes(nbytes, "plane_sort workspace", x.device)
    vals = torch.empty_like(x)
    index = torch.empty(x.shape, device=x.device, dtype=torch.int32) if return_index else None
    check(_timed(f"plane_sort {planes}x{m}", -8 * x.numel(), x.device, lambda: L.ast_plane_sort_f32(
        ptr(x), ptr(vals), ptr(index), planes, m, int(_chunk), ptr(wsb), max(nbytes, 0), stream_ptr(x.device))),
        "plane_sort")
    return (vals, index) if return_index else vals


# Whitening and colouring transform (csrc/wct.hip): the limits of ast_hip.h
WCT_MAX_C = 1024
WCT_EPS_REL = 1e-3


def wct_default_iters(c: int, eps_rel: float = WCT_EPS_REL) -> int:
    """The Newton-Schulz step count that iters=0 selects: ceil(log_2.25(c / eps_rel)) + 5 (the library's
    own value, so both sides agree): 22 for (512, 1e-3)."""
    it = int(lib().ast_wct_default_iters(int(c), float(eps_rel)))
    if it < 0:
        check(it, f"wct_default_iters(c={c}, eps_rel={eps_rel})")
    return it


def wct_cov(x: torch.Tensor, eps_rel: float = WCT_EPS_REL):
    """(mean [N, C], cov [N, C, C]) of x [N, C, H, W] (or [N, C, M]): the two-pass centred covariance
    over each sample's pixels, / (M - 1), plus the ridge eps_rel * max(tr / C, 1e-20) on the diagonal;
    cov equals its transpose in bits."""
    x = _dev(x, "x")
    if x.dim() < 3 or x.numel() == 0:
        raise HipOpError(f"wct_cov needs a non-empty [N, C, H, W] or [N, C, M] tensor, got {tuple(x.shape)}")
    n, c = int(x.shape[0]), int(x.shape[1])
    m = x.numel() // (n * c)
    L = lib()
    nbytes = int(L.ast_wct_cov_workspace_bytes(n, c, m))
    wsb = _ws_bytes(nbytes, "wct_cov workspace", x.device)
    mean = torch.empty((n, c), device=x.device, dtype=torch.float32)
    cov = torch.empty((n, c, c), device=x.device, dtype=torch.float32)
    check(_timed(f"wct_cov {c}ch M={m}", n * c * (c + 1) * m, x.device, lambda: L.ast_wct_cov_f32(
        ptr(x), ptr(mean), ptr(cov), n, c, m, float(eps_rel), ptr(wsb), nbytes, stream_ptr(x.device))), "wct_cov")
    return mean, cov


def wct_sqrt(cov: torch.Tensor, iters: int = 0, eps_rel: float = WCT_EPS_REL):
    """(cov^(1/2), cov^(-1/2)) of symmetric positive definite matrices [B, C, C] by `iters` coupled
    Newton-Schulz steps (0: wct_default_iters(C, eps_rel), eps_rel being the relative ridge that the
    matrices carry); a fixed count, no convergence test."""
    cov = _dev(cov, "cov")
    if cov.dim() != 3 or cov.shape[1] != cov.shape[2] or cov.numel() == 0:
        raise HipOpError(f"wct_sqrt needs non-empty [B, C, C] matrices, got {tuple(cov.shape)}")
    b, c = int(cov.shape[0]), int(cov.shape[1])
    if int(iters) == 0 and c <= WCT_MAX_C:
        iters = wct_default_iters(c, eps_rel)
    L = lib()
    nbytes = int(L.ast_wct_sqrt_workspace_bytes(b, c))
    wsb = _ws_bytes(nbytes, "wct_sqrt workspace", cov.device)
    root, iroot = torch.empty_like(cov), torch.empty_like(cov)
    check(_timed(f"wct_sqrt {b}x{c}", 6 * b * c ** 3 * max(int(iters), 0), cov.device, lambda: L.ast_wct_sqrt_f32(
        ptr(cov), ptr(root), ptr(iroot), b, c, int(iters), ptr(wsb), nbytes, stream_ptr(cov.device))), "wct_sqrt")
    return root, iroot


def wct(content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0, eps_rel: float = WCT_EPS_REL,
        iters: int = 0):
    """Whitening and colouring transform (Li et al., NeurIPS 2017), a drop-in for adain that matches
    the cross-channel covariance: out = alpha * (T (c - mu_c) + mu_s) + (1 - alpha) * c with
    T = cov_s^(1/2) cov_c^(-1/2) (wct_cov, wct_sqrt). content [N, C, Hc, Wc]; style [N, C, Hs, Ws] or
    [1, C, Hs, Ws] (shared by the batch); C <= 1024, at least 2 pixels per map, eps_rel in [1e-4, 1]."""
    content, style, n, ns, c, hc, wc, hs, ws = _pair(content, style, "content_map", "style_map", "WCT", named=False)
    L = lib()
    nbytes = int(L.ast_wct_workspace_bytes(n, ns, c, hc * wc, hs * ws))
    wsb = _ws_bytes(nbytes, "wct workspace", content.device)
    out = torch.empty_like(content)
    check(_timed(f"wct {c}ch {hc}x{wc}", 0, content.device, lambda: L.ast_wct_f32(
        ptr(content), ptr(style), ptr(out), n, ns, c, hc, wc, hs, ws, float(alpha), float(eps_rel), int(iters),
        ptr(wsb), nbytes, stream_ptr(content.device))), "wct")
    return out


# Regional WCT (csrc/wct.hip): per-region whitening and colouring towards a per-region mix of styles

def _region_mix(mix, n: int, s: int, device, what: str):
    """mix [K, S], [1, K, S] or [N, K, S] on the device -> (mix [1 or N, K, S], K)."""
    mix = _dev(mix, "mix")
    if mix.dim() == 2:
        mix = mix.unsqueeze(0)
    if (mix.dim() != 3 or mix.shape[0] not in (1, n) or not 1 <= mix.shape[1] <= MAX_REGIONS or mix.shape[2] != s
            or mix.device != device):
        raise HipOpError(f"{what}: mix must be [N={n} or 1, K <= {MAX_REGIONS}, S={s}] on {device}, got "
                         f"{tuple(mix.shape)} on {mix.device}")
    return mix, int(mix.shape[1])


def _style_bank(styles, mix, style_labels, n: int, c: int, device, what: str):
    """The style side of a regional transform: the fp32 bank [S, C, Hs, Ws], the mix (_region_mix) and the
    bank's own labels uint8 [S, Hs, Ws] or None, all on `device`: (styles, S, Hs, Ws, mix, K, style_labels)."""
    styles = _dev(styles, "styles")
    if styles.dim() != 4 or styles.numel() == 0 or styles.shape[1] != c or styles.device != device:
        raise HipOpError(f"{what} needs a non-empty style bank [S, C={c}, Hs, Ws] on {device}, got "
                         f"{tuple(styles.shape)} on {styles.device}")
    s, hs, ws = int(styles.shape[0]), int(styles.shape[2]), int(styles.shape[3])
    mix, k = _region_mix(mix, n, s, device, what)
    if style_labels is not None:
        style_labels = _labels(style_labels, "style_labels")
        if tuple(style_labels.shape) != (s, hs, ws) or style_labels.device != device:
            raise HipOpError(f"style_labels must be [S, Hs, Ws] = {(s, hs, ws)} on {device}, got "
                             f"{tuple(style_labels.shape)} on {style_labels.device}")
    return styles, s, hs, ws, mix, k, style_labels


def wct_region_cov(x: torch.Tensor, labels: torch.Tensor, regions: int, eps_rel: float = WCT_EPS_REL):
    """(mean [N, K, C], cov [N, K, C, C], count [N, K] int32) of x [N, C, H, W] under labels [N, H, W]
    (uint8; a label >= regions belongs to no region): wct_cov of each region's pixels taken in
    ascending pixel index, bit for bit. A region of fewer than 2 pixels has mean 0 and cov = I."""
    regions = _regions(regions)
    x, labels, n, c, h, w = _map_and_labels(x, labels, "x")
    L = lib()
    nbytes = int(L.ast_wct_region_cov_workspace_bytes(n, c, h, w, regions))
    wsb = _ws_bytes(nbytes, "wct_region_cov workspace", x.device)
    mean = torch.empty((n, regions, c), device=x.device, dtype=torch.float32)
    cov = torch.empty((n, regions, c, c), device=x.device, dtype=torch.float32)
    count = torch.empty((n, regions), device=x.device, dtype=torch.int32)
    check(_timed(f"wct_region_cov {c}ch {h}x{w} K{regions}", n * c * (c + 1) * h * w, x.device,
                 lambda: L.ast_wct_region_cov_f32(ptr(x), ptr(labels), ptr(mean), ptr(cov), ptr(count), n, c, h, w,
                                                  regions, float(eps_rel), ptr(wsb), nbytes, stream_ptr(x.device))),
          "wct_region_cov")
    return mean, cov, count


def wct_region_apply(content: torch.Tensor, labels: torch.Tensor, content_mean: torch.Tensor,
                     content_isqrt: torch.Tensor, style_mean: torch.Tensor, style_sqrt: torch.Tensor, mix: torch.Tensor,
                     style_count: torch.Tensor = None, alpha: float = 1.0):
    """The apply stage of wct_regions from its parts: content_mean [N, K, C] and content_isqrt
    [N, K, C, C] (wct_region_cov, wct_sqrt); style_mean [S, C] and style_sqrt [S, C, C] of whole style
    maps, or [S, K, C] and [S, K, C, C] of their regions with style_count [S, K] (int32; None: every
    style region counts as valid); mix as wct_regions."""
    content, labels, n, c, h, w = _map_and_labels(content, labels, "content_map")
    sm, sr = _dev(style_mean, "style_mean"), _dev(style_sqrt, "style_sqrt")
    if sm.dim() not in (2, 3) or sm.numel() == 0:
        raise HipOpError(f"style_mean must be [S, C] or [S, K, C], got {tuple(sm.shape)}")
    s, regional = int(sm.shape[0]), sm.dim() == 3
    mix, k = _region_mix(mix, n, s, content.device, "wct_region_apply")
    cm, ci = _dev(content_mean, "content_mean"), _dev(content_isqrt, "content_isqrt")
    lead = (s, k) if regional else (s,)
    if (tuple(cm.shape) != (n, k, c) or tuple(ci.shape) != (n, k, c, c) or tuple(sm.shape) != lead + (c,)
            or tuple(sr.shape) != lead + (c, c)):
        raise HipOpError(f"wct_region_apply needs content statistics [{n}, {k}, {c}(, {c})] and style statistics "
                         f"{list(lead)} + [{c}(, {c})], got {tuple(cm.shape)}, {tuple(ci.shape)}, {tuple(sm.shape)}, "
                         f"{tuple(sr.shape)}")
    if any(t.device != content.device for t in (cm, ci, sm, sr)):
        raise HipOpError(f"wct_region_apply: every tensor must be on {content.device}")
    sc = None
    if style_count is not None:
        sc = _dev_typed(style_count, "style_count", torch.int32)
        if not regional or tuple(sc.shape) != (s, k) or sc.device != content.device:
            raise HipOpError(f"style_count goes with regional style statistics and must be [S={s}, K={k}] int32 on "
                             f"{content.device}, got {tuple(sc.shape)}")
    L = lib()
    nbytes = int(L.ast_wct_region_apply_workspace_bytes(n, c, h, w, k))
    wsb = _ws_bytes(nbytes, "wct_region_apply workspace", content.device)
    out = torch.empty_like(content)
    check(_timed(f"wct_region_apply {c}ch {h}x{w} K{k}", 2 * n * c * c * (h * w + k * c), content.device,
                 lambda: L.ast_wct_region_apply_f32(
                     ptr(content), ptr(labels), ptr(cm), ptr(ci), ptr(sm), ptr(sr), ptr(mix), ptr(sc), ptr(out), n, c, h,
                     w, k, s, int(mix.shape[0]), 1 if regional else 0, float(alpha), ptr(wsb), nbytes,
                     stream_ptr(content.device))), "wct_region_apply")
    return out


def wct_regions(content: torch.Tensor, labels: torch.Tensor, styles: torch.Tensor, mix: torch.Tensor,
                style_labels: torch.Tensor = None, alpha: float = 1.0, eps_rel: float = WCT_EPS_REL, iters: int = 0):
    """Regional WCT (Li et al., NeurIPS 2017, section 4): region k of sample n (the pixels with
    labels[n] == k) is whitened with its own mean and covariance and coloured with the mix
    sum_s mix[n, k, s] * (cov_s^(1/2), mu_s) of the S styles [S, C, Hs, Ws] (shared by the batch); with
    style_labels [S, Hs, Ws] the statistics are those of each style's own region k. Pixels labelled
    >= K, regions of fewer than 2 pixels and regions whose class a used style lacks pass through bit
    for bit. mix is [K, S], [1, K, S] or [N, K, S] on the device, rows summing to 1; a style of weight
    exactly 0 is never read. alpha, eps_rel and iters as wct."""
    content, labels, n, c, h, w = _map_and_labels(content, labels, "content_map")
    styles, s, hs, ws, mix, k, style_labels = _style_bank(styles, mix, style_labels, n, c, content.device,
                                                          "wct_regions")
    L = lib()
    nbytes = int(L.ast_wct_regions_workspace_bytes(n, c, h, w, k, s, hs, ws, 0 if style_labels is None else 1))
    wsb = _ws_bytes(nbytes, "wct_regions workspace", content.device)
    out = torch.empty_like(content)
    # the stages' counts: both covariances, the roots of all the matrices, T and the apply GEMM
    b = n * k + s * (1 if style_labels is None else k)
    it = int(iters) or (wct_default_iters(c, eps_rel) if c <= WCT_MAX_C and 1e-4 <= eps_rel <= 1 else 0)
    flops = c * (c + 1) * (n * h * w + s * hs * ws) + 6 * b * c ** 3 * max(it, 0) + 2 * n * c * c * (h * w + k * c)
    check(_timed(f"wct_regions {c}ch {h}x{w} K{k} S{s}", flops, content.device, lambda: L.ast_wct_regions_f32(
        ptr(content), ptr(labels), ptr(styles), ptr(style_labels), ptr(mix), ptr(out), n, c, h, w, k, s, hs, ws,
        int(mix.shape[0]), float(alpha), float(eps_rel), int(iters), ptr(wsb), nbytes, stream_ptr(content.device))),
        "wct_regions")
    return out


# Regional EFDM (csrc/efdm_regions.hip): distribution matching per region, towards a mix of a style bank

def efdm_region_sort(x: torch.Tensor, labels: torch.Tensor, regions: int):
    """The bank stage of efdm_regions: every plane of x [S, C, H, W] ordered by (min(label, regions),
    totalOrder key, index) -- region after region, each ascending, the pixels labelled >= regions
    last -- as (sorted [S, C, H*W], count [S, regions] int32). labels uint8 [S, H, W], or None: one
    region holds everything (the plain sort; count[:, 0] = H*W). Planes of at most EFDM_FUSED_MAX."""
    regions = _regions(regions)
    if labels is None:
        x = _dev(x, "x")
        if x.dim() != 4 or x.numel() == 0:
            raise HipOpError(f"x must be a non-empty NCHW map, got {tuple(x.shape)}")
        s, c, h, w = (int(d) for d in x.shape)
    else:
        x, labels, s, c, h, w = _map_and_labels(x, labels, "x")
    vals = torch.empty((s, c, h * w), device=x.device, dtype=torch.float32)
    count = torch.empty((s, regions), device=x.device, dtype=torch.int32)
    check(_timed(f"efdm_region_sort {c}ch {h}x{w} K{regions}", -8 * x.numel(), x.device,
                 lambda: lib().ast_efdm_region_sort_f32(ptr(x), ptr(labels), ptr(vals), ptr(count), s, c, h, w, regions,
                                                        stream_ptr(x.device))), "efdm_region_sort")
    return vals, count


def efdm_regions(content: torch.Tensor, labels: torch.Tensor, styles: torch.Tensor, mix: torch.Tensor,
                 style_labels: torch.Tensor = None, alpha: float = 1.0):
    """Regional EFDM: in region k of sample n (the pixels with labels[n] == k) the pixel of rank r among
    the region's Mc_k pixels takes sum_s mix[n, k, s] * S_sk[((2r + 1) * Ms_sk) // (2 * Mc_k)], S_sk the
    sorted values of style s's plane [S, C, Hs, Ws] (shared by the batch) or, with style_labels
    [S, Hs, Ws], of its own region k: per channel the Wasserstein barycentre of the styles'
    distributions. Pixels labelled >= K, and regions whose class a used style lacks, pass through bit
    for bit. mix is [K, S], [1, K, S] or [N, K, S] on the device, non-negative; a style of weight
    exactly 0 is never used, and a one-hot row copies style values (no arithmetic at alpha == 1).
    alpha as efdm. Planes of at most EFDM_FUSED_MAX elements."""
    content, labels, n, c, h, w = _map_and_labels(content, labels, "content_map")
    styles, s, hs, ws, mix, k, style_labels = _style_bank(styles, mix, style_labels, n, c, content.device,
                                                          "efdm_regions")
    L = lib()
    nbytes = int(L.ast_efdm_regions_workspace_bytes(n, c, h, w, k, s, hs, ws))
    wsb = _ws_bytes(nbytes, "efdm_regions workspace", content.device)
    out = torch.empty_like(content)
    algo = 4 * (2 * content.numel() + 2 * styles.numel()) + labels.numel()   # algorithmic: c, out, the bank in and out
    check(_timed(f"efdm_regions {c}ch {h}x{w} K{k} S{s}", -algo, content.device, lambda: L.ast_efdm_regions_f32(
        ptr(content), ptr(labels), ptr(styles), ptr(style_labels), ptr(mix), ptr(out), n, c, h, w, k, s, hs, ws,
        int(mix.shape[0]), float(alpha), ptr(wsb), nbytes, stream_ptr(content.device))), "efdm_regions")
    return out


# Style swap (csrc/swap.hip): the limits of ast_hip.h
SWAP_MAX_C = 1024


def _swap_pair(a: torch.Tensor, b: torch.Tensor, na: str, nb: str, what: str):
    """Two fp32 device NCHW maps with equal C, sides of at least 3 and b's batch equal to a's or 1:
    (a, b, n, ns, c, ha, wa, hb, wb)."""
    return _pair(a, b, na, nb, what, side=3)


def patch_match(content_key: torch.Tensor, style_key: torch.Tensor, return_score: bool = False, _splits: int = 0):
    """For every 3x3 patch of content_key [N, C, H, W], the index jy * (Ws - 2) + jx of the 3x3 patch of
    style_key [N or 1, C, Hs, Ws] with the largest <content patch, style patch> / ||style patch||
    (the lowest index on equal scores; a zero style patch scores 0; a NaN never wins): int32
    [N, H - 2, W - 2], and the winning score with return_score. The scores are never stored.
    _splits forces the number of workgroups that share the style patches (0: the library's choice)."""
    ck, sk, n, ns, c, hc, wc, hs, ws = _swap_pair(content_key, style_key, "content_key", "style_key", "patch_match")
    L, dev, st = lib(), ck.device, stream_ptr(ck.device)
    nb = int(L.ast_patch_norms_workspace_bytes(ns, hs, ws))
    wsn = _ws_bytes(nb, "patch_norms workspace", dev)
    inv = torch.empty((ns, hs - 2, ws - 2), device=dev, dtype=torch.float32)
    check(L.ast_patch_norms_f32(ptr(sk), ptr(inv), ns, c, hs, ws, ptr(wsn), nb, st), "patch_norms")
    mb = int(L.ast_patch_match_workspace_bytes(n, ns, hc, wc, hs, ws, int(_splits)))
    wsm = _ws_bytes(mb, "patch_match workspace", dev)
    index = torch.empty((n, hc - 2, wc - 2), device=dev, dtype=torch.int32)
    score = torch.empty((n, hc - 2, wc - 2), device=dev, dtype=torch.float32) if return_score else None
    flops = 2 * n * (hc - 2) * (wc - 2) * (hs - 2) * (ws - 2) * 9 * c
    check(_timed(f"patch_match {c}ch {hc}x{wc} vs {hs}x{ws}", flops, dev, lambda: L.ast_patch_match_ex_f32(
        ptr(ck), ptr(sk), ptr(inv), ptr(index), ptr(score), n, ns, c, hc, wc, hs, ws, int(_splits), ptr(wsm), mb, st)),
        "patch_match")
    return (index, score) if return_score else index


def patch_gather(style_value: torch.Tensor, index: torch.Tensor, content: torch.Tensor, alpha: float = 1.0):
    """The reconstruction of style swap: out[y, x] = (1 - alpha) content[y, x] + alpha * the mean, over the
    up-to-nine content patches covering (y, x), of the style_value pixel that the patch's match
    (index [N, H - 2, W - 2] int32, as patch_match returns) puts there. One launch."""
    c_, sv, n, ns, c, hc, wc, hs, ws = _swap_pair(content, style_value, "content_map", "style_value", "patch_gather")
    index = _like(index, c_.device, torch.int32, "index", shape=(n, hc - 2, wc - 2),
                  msg=f"index must be an int32 tensor {(n, hc - 2, wc - 2)} on {c_.device}")
    out = torch.empty_like(c_)
    check(_timed(f"patch_gather {c}ch {hc}x{wc}", -4 * 11 * c_.numel(), c_.device, lambda: lib().ast_patch_gather_f32(
        ptr(sv), ptr(index), ptr(c_), ptr(out), n, ns, c, hc, wc, hs, ws, float(alpha), stream_ptr(c_.device))),
        "patch_gather")
    return out


def style_swap(content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0, normalize: bool = False,
               return_index: bool = False):
    """Style swap (Chen & Schmidt 2016): every 3x3 patch of content [N, C, H, W] is replaced by the most
    similar 3x3 patch of style [N or 1, C, Hs, Ws] (patch_match), the overlaps are averaged and
    blended with the content by alpha (patch_gather). normalize=True matches on the per-channel
    instance-normalised maps (mean_variance_norm) and reconstructs from the raw style features, the
    style decorator of Avatar-Net. return_index adds the int32 match [N, H - 2, W - 2]."""
    c_, s_, n, ns, c, hc, wc, hs, ws = _swap_pair(content, style, "content_map", "style_map", "style_swap")
    ck, sk = (mean_variance_norm(c_), mean_variance_norm(s_)) if normalize else (c_, s_)
    L = lib()
    nbytes = int(L.ast_style_swap_workspace_bytes(n, ns, hc, wc, hs, ws))
    wsb = _ws_bytes(nbytes, "style_swap workspace", c_.device)
    out = torch.empty_like(c_)
    index = torch.empty((n, hc - 2, wc - 2), device=c_.device, dtype=torch.int32) if return_index else None
    flops = 2 * n * (hc - 2) * (wc - 2) * (hs - 2) * (ws - 2) * 9 * c
    check(_timed(f"style_swap {c}ch {hc}x{wc} vs {hs}x{ws}", flops, c_.device, lambda: L.ast_style_swap_f32(
        ptr(ck), ptr(sk), ptr(s_), ptr(c_), ptr(out), ptr(index), None, n, ns, c, hc, wc, hs, ws, float(alpha),
        ptr(wsb), nbytes, stream_ptr(c_.device))), "style_swap")
    return (out, index) if return_index else out


# Relaxed EMD style loss (csrc/remd.hip): the limits of ast_hip.h
REMD_MAX_C = 1024
REMD_MAX_PIXELS = 1 << 22
REMD_ROW, REMD_COL = 1, 2   # the values of `branch`


def _remd_pair(x: torch.Tensor, y: torch.Tensor, what: str):
    """Two fp32 device NCHW maps with equal C and y's batch equal to x's or 1, inside the limits of
    csrc/remd.hip: (x, y, n, ns, c, m, p) with m, p the pixel counts."""
    x, y, n, ns, c, h, w, hs, ws = _pair(x, y, "x", "y", what)
    m, p = h * w, hs * ws
    if c > REMD_MAX_C or max(m, p) > REMD_MAX_PIXELS or n > 65535:
        raise HipOpError(f"{what}: C is at most {REMD_MAX_C}, a map has at most {REMD_MAX_PIXELS} pixels and a batch "
                         f"65535 samples: x {tuple(x.shape)} vs y {tuple(y.shape)}")
    return x, y, n, ns, c, m, p


def cosine_norms(x: torch.Tensor) -> torch.Tensor:
    """1 / ||x[n, :, h, w]||_2 for every pixel of x [N, C, H, W]: [N, H, W], exactly 0 at a zero vector.
    Equal vectors have equal inverse norms in bits."""
    x = _dev(x, "x")
    if x.dim() != 4 or x.numel() == 0:
        raise HipOpError(f"cosine_norms needs a non-empty NCHW map, got {tuple(x.shape)}")
    n, c, h, w = (int(s) for s in x.shape)
    inv = torch.empty((n, h, w), device=x.device, dtype=torch.float32)
    check(lib().ast_cosine_norms_f32(ptr(x), ptr(inv), n, c, h * w, stream_ptr(x.device)), "cosine_norms")
    return inv


def cosine_match(x: torch.Tensor, y: torch.Tensor, _splits: int = 0):
    """The two-way nearest-neighbour match in cosine distance D(i, j) = 1 - <x_i, y_j> / (|x_i| |y_j|)
    between the pixels of x [N, C, H, W] and y [N or 1, C, Hs, Ws]: (row_min [N, H, W], row_index int32
    [N, H, W], col_min [N, Hs, Ws], col_index int32 [N, Hs, Ws]); the lowest index on equal distances,
    a NaN never wins, a zero vector is at distance 1 from everything. The distances are never stored.
    _splits forces the number of workgroups that share the style pixels (0: the library's choice)."""
    x, y, n, ns, c, m, p = _remd_pair(x, y, "cosine_match")
    L, dev, st = lib(), x.device, stream_ptr(x.device)
    u, v = cosine_norms(x), cosine_norms(y)
    nb = int(L.ast_cosine_match_workspace_bytes(n, ns, m, p, int(_splits)))
    wsb = _ws_bytes(nb, "cosine_match workspace", dev)
    (h, w), (hs, ws) = x.shape[2:], y.shape[2:]
    rmin = torch.empty((n, h, w), device=dev, dtype=torch.float32)
    ridx = torch.empty((n, h, w), device=dev, dtype=torch.int32)
    cmin = torch.empty((n, hs, ws), device=dev, dtype=torch.float32)
    cidx = torch.empty((n, hs, ws), device=dev, dtype=torch.int32)
    check(_timed(f"cosine_match {c}ch {m} vs {p}", 2 * n * m * p * c, dev, lambda: L.ast_cosine_match_f32(
        ptr(x), ptr(y), ptr(u), ptr(v), ptr(rmin), ptr(ridx), ptr(cmin), ptr(cidx), n, ns, c, m, p, int(_splits),
        ptr(wsb), nb, st)), "cosine_match")
    return rmin, ridx, cmin, cidx


def remd_means(row_min: torch.Tensor, col_min: torch.Tensor, weight: float = 1.0, _branch: int = 0, acc=None):
    """(loss, row_mean [N], col_mean [N], branch uint8 [N]) from the minima of cosine_match: the last
    stage of remd_loss. `acc`: the loss accumulator the value is added into (a fresh one if None)."""
    if (row_min.device.type != "cuda" or row_min.dtype != torch.float32 or col_min.dtype != torch.float32
            or row_min.device != col_min.device or row_min.shape[0] != col_min.shape[0] or row_min.numel() == 0
            or col_min.numel() == 0):
        raise HipOpError("remd_means needs the float32 device minima [N, ...] of cosine_match")
    row_min, col_min = row_min.contiguous(), col_min.contiguous()
    n, dev = int(row_min.shape[0]), row_min.device
    rmean = torch.empty((n,), device=dev, dtype=torch.float32)
    cmean = torch.empty((n,), device=dev, dtype=torch.float32)
    branch = torch.empty((n,), device=dev, dtype=torch.uint8)
    acc = loss_accumulator(dev) if acc is None else acc
    check(lib().ast_remd_means_f32(ptr(row_min), ptr(col_min), ptr(rmean), ptr(cmean), ptr(branch), ptr(acc), n,
                                   row_min.numel() // n, col_min.numel() // n, float(weight), int(_branch),
                                   stream_ptr(dev)), "remd_means")
    return acc[0], rmean, cmean, branch


def remd_loss(x: torch.Tensor, y: torch.Tensor, weight: float = 1.0, _branch: int = 0, acc=None):
    """The relaxed earth mover's distance style loss (Kolkin et al., CVPR 2019), exact: with r, c the row
    and column minima of cosine_match(x, y), weight * mean over the batch of max(mean r, mean c) per
    sample. Returns (loss, row_mean [N], col_mean [N], branch uint8 [N], state): branch is REMD_ROW where
    mean r >= mean c, else REMD_COL; state = (inv_x, inv_y, row_min, row_index, col_min, col_index) is what
    remd_loss_backward reads. _branch (tests): 1 / 2 takes the row / column branch for every sample."""
    x, y, n, ns, c, m, p = _remd_pair(x, y, "remd_loss")
    if _branch not in (0, 1, 2):
        raise HipOpError(f"remd_loss: _branch is 0, 1 or 2, got {_branch}")
    L, dev = lib(), x.device
    nb = int(L.ast_remd_loss_workspace_bytes(n, ns, m, p))
    wsb = _ws_bytes(nb, "remd_loss workspace", dev)
    (h, w), (hs, ws) = x.shape[2:], y.shape[2:]
    f32 = dict(device=dev, dtype=torch.float32)
    u, v = torch.empty((n, h, w), **f32), torch.empty((ns, hs, ws), **f32)
    rmin, cmin = torch.empty((n, h, w), **f32), torch.empty((n, hs, ws), **f32)
    ridx = torch.empty((n, h, w), device=dev, dtype=torch.int32)
    cidx = torch.empty((n, hs, ws), device=dev, dtype=torch.int32)
    rmean, cmean = torch.empty((n,), **f32), torch.empty((n,), **f32)
    branch = torch.empty((n,), device=dev, dtype=torch.uint8)
    acc = loss_accumulator(dev) if acc is None else acc
    check(_timed(f"remd_loss {c}ch {m} vs {p}", 2 * n * m * p * c, dev, lambda: L.ast_remd_loss_f32(
        ptr(x), ptr(y), ptr(u), ptr(v), ptr(rmin), ptr(ridx), ptr(cmin), ptr(cidx), ptr(rmean), ptr(cmean),
        ptr(branch), ptr(acc), n, ns, c, m, p, float(weight), int(_branch), ptr(wsb), nb, stream_ptr(dev))),
        "remd_loss")
    return acc[0], rmean, cmean, branch, (u, v, rmin, ridx, cmin, cidx)


def remd_loss_backward(x: torch.Tensor, y: torch.Tensor, state, branch: torch.Tensor, grad: torch.Tensor,
                       weight: float = 1.0) -> torch.Tensor:
    """d loss / d x [N, C, H, W] of remd_loss from its state and branch, scaled by the device scalar
    `grad`; nothing flows to y. One launch builds the column branch's inverse lists, one gather launch
    per branch follows."""
    x, y, n, ns, c, m, p = _remd_pair(x, y, "remd_loss_backward")
    u, v, rmin, ridx, cmin, cidx = state
    dev = x.device
    want = ((u, n * m, torch.float32), (v, ns * p, torch.float32), (rmin, n * m, torch.float32),
            (ridx, n * m, torch.int32), (cmin, n * p, torch.float32), (cidx, n * p, torch.int32),
            (branch, n, torch.uint8), (grad, 1, torch.float32))
    msg = "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"
    u, v, rmin, ridx, cmin, cidx, branch, grad = [_like(t, dev, dt, "state", numel=numel, msg=msg)
                                                  for t, numel, dt in want]
    L = lib()
    nb = int(L.ast_remd_loss_backward_workspace_bytes(n, m, p))
    wsb = _ws_bytes(nb, "remd_loss_backward workspace", dev)
    dx = torch.empty_like(x)
    check(_timed(f"remd_loss_backward {c}ch {m} vs {p}", -4 * 3 * x.numel(), dev,
                 lambda: L.ast_remd_loss_backward_f32(
                     ptr(x), ptr(y), ptr(u), ptr(v), ptr(rmin), ptr(ridx), ptr(cmin), ptr(cidx), ptr(branch),
                     ptr(grad), ptr(dx), n, ns, c, m, p, float(weight), ptr(wsb), nb, stream_ptr(dev))),
          "remd_loss_backward")
    return dx


# Self-similarity content loss (csrc/selfsim.hip): AST_SELFSIM_MAX_PIXELS of ast_hip.h, where the two sign
# planes take 64 MiB per sample
SELFSIM_MAX_PIXELS = 1 << 14


def _selfsim_pair(x: torch.Tensor, c: torch.Tensor, what: str):
    """Two fp32 device NCHW maps of equal shape inside the limits of csrc/selfsim.hip: (x, c, n, ch, pixels).
    The checks of _remd_pair, and equal shapes."""
    x, c, n, _, ch, m, _ = _remd_pair(x, c, what)
    if x.shape != c.shape:
        raise HipOpError(f"{what} needs maps of equal shape: x {tuple(x.shape)} vs c {tuple(c.shape)}")
    if m > SELFSIM_MAX_PIXELS:
        raise HipOpError(f"{what}: a map has at most {SELFSIM_MAX_PIXELS} pixels, got {tuple(x.shape)}")
    return x, c, n, ch, m


def _selfsim_planes(x: torch.Tensor):
    n, _, h, w = x.shape
    return (n, h * w, (h * w + 63) // 64)


def selfsim_colsum(x: torch.Tensor, inv_norm: torch.Tensor) -> torch.Tensor:
    """r [N, H, W]: r(j) = sum_i D(i, j) over the pixels i != j of the same sample, D the cosine distance
    between pixels of x [N, C, H, W], from inv_norm = cosine_norms(x); computed as (HW - 1) - (<xh_j, S> -
    ||xh_j||^2) with S the sum of the unit vectors: no pass over pairs."""
    x, _, n, ch, m = _selfsim_pair(x, x, "selfsim_colsum")
    u = _like(inv_norm, x.device, torch.float32, "selfsim_colsum: inv_norm", shape=(n,) + tuple(x.shape[2:]))
    L, dev = lib(), x.device
    nb = int(L.ast_selfsim_colsum_workspace_bytes(n, ch))
    wsb = _ws_bytes(nb, "selfsim_colsum workspace", dev)
    r = torch.empty_like(u)
    check(L.ast_selfsim_colsum_f32(ptr(x), ptr(u), ptr(r), n, ch, m, ptr(wsb), nb, stream_ptr(dev)), "selfsim_colsum")
    return r


def selfsim_pairs(x: torch.Tensor, c: torch.Tensor, inv_x: torch.Tensor, inv_c: torch.Tensor, r_x: torch.Tensor,
                  r_c: torch.Tensor):
    """The pass over the pixel pairs of the self-similarity loss: (sums [N], t [N, H, W], pos, neg int64
    [N, HW, ceil(HW / 64)]). With e(i, j) = D_x(i, j) / r_x(j) - D_c(i, j) / r_c(j) (1 / r taken as 0
    unless r is positive and finite), sums[b] = (1 / HW) sum_{i != j} |e|, t(j) = (1 / r_x(j)) sum_k
    sign(e(k, j)) D_x(k, j), and bit k of word (i, J) of pos / neg is set where e(i, 64 J + k) > 0 / < 0."""
    x, c, n, ch, m = _selfsim_pair(x, c, "selfsim_pairs")
    shp = (n,) + tuple(x.shape[2:])
    u, v, rx, rc = (_like(t, x.device, torch.float32, f"selfsim_pairs: {k}", shape=shp)
                    for t, k in ((inv_x, "inv_x"), (inv_c, "inv_c"), (r_x, "r_x"), (r_c, "r_c")))
    L, dev = lib(), x.device
    nb = int(L.ast_selfsim_pairs_workspace_bytes(n, m))
    wsb = _ws_bytes(nb, "selfsim_pairs workspace", dev)
    sums = torch.empty((n,), device=dev, dtype=torch.float32)
    t = torch.empty(shp, device=dev, dtype=torch.float32)
    pos = torch.empty(_selfsim_planes(x), device=dev, dtype=torch.int64)
    neg = torch.empty_like(pos)
    check(_timed(f"selfsim_pairs {ch}ch {m}", 2 * n * m * m * ch, dev, lambda: L.ast_selfsim_pairs_f32(
        ptr(x), ptr(c), ptr(u), ptr(v), ptr(rx), ptr(rc), ptr(sums), ptr(t), ptr(pos), ptr(neg), n, ch, m, ptr(wsb),
        nb, stream_ptr(dev))), "selfsim_pairs")
    return sums, t, pos, neg


def selfsim_total(sums: torch.Tensor, weight: float = 1.0, acc=None) -> torch.Tensor:
    """weight * mean of the per-sample values of selfsim_pairs: the last stage of selfsim_loss. `acc`: the
    loss accumulator the value is added into (a fresh one if None)."""
    if (not isinstance(sums, torch.Tensor) or sums.device.type != "cuda" or sums.dtype != torch.float32
            or sums.dim() != 1 or sums.numel() == 0):
        raise HipOpError("selfsim_total needs the float32 device sums [N] of selfsim_pairs")
    sums, dev = sums.contiguous(), sums.device
    acc = loss_accumulator(dev) if acc is None else acc
    check(lib().ast_selfsim_total_f32(ptr(sums), ptr(acc), int(sums.numel()), float(weight), stream_ptr(dev)),
          "selfsim_total")
    return acc[0]


def selfsim_loss(x: torch.Tensor, c: torch.Tensor, weight: float = 1.0, acc=None):
    """The self-similarity content loss (Kolkin et al., CVPR 2019), exact: weight * mean over the batch of
    (1 / HW) sum_{i != j} |D_x(i, j) / r_x(j) - D_c(i, j) / r_c(j)|, D the cosine distances between the pixels
    inside x (the stylised map) and inside c (the content map, same shape), r their column sums. Returns
    (loss, per_sample [N], state); state = (inv_x, inv_c, r_x, r_c, t, pos, neg) is what
    selfsim_loss_backward reads. The distance matrices are never stored."""
    x, c, n, ch, m = _selfsim_pair(x, c, "selfsim_loss")
    L, dev = lib(), x.device
    nb = int(L.ast_selfsim_loss_workspace_bytes(n, ch, m))
    wsb = _ws_bytes(nb, "selfsim_loss workspace", dev)
    shp = (n,) + tuple(x.shape[2:])
    u, v, rx, rc, t = (torch.empty(shp, device=dev, dtype=torch.float32) for _ in range(5))
    pos = torch.empty(_selfsim_planes(x), device=dev, dtype=torch.int64)
    neg = torch.empty_like(pos)
    sums = torch.empty((n,), device=dev, dtype=torch.float32)
    acc = loss_accumulator(dev) if acc is None else acc
    check(_timed(f"selfsim_loss {ch}ch {m}", 2 * n * m * m * ch, dev, lambda: L.ast_selfsim_loss_f32(
        ptr(x), ptr(c), ptr(u), ptr(v), ptr(rx), ptr(rc), ptr(t), ptr(pos), ptr(neg), ptr(sums), ptr(acc), n, ch, m,
        float(weight), ptr(wsb), nb, stream_ptr(dev))), "selfsim_loss")
    return acc[0], sums, (u, v, rx, rc, t, pos, neg)


def selfsim_loss_backward(x: torch.Tensor, state, grad: torch.Tensor, weight: float = 1.0) -> torch.Tensor:
    """d loss / d x [N, C, H, W] of selfsim_loss from its state, scaled by the device scalar `grad`; nothing
    flows to the content map, which is not read. A GEMM of the weights rebuilt from the sign planes with
    x, then the normalisation backward; no cosine is recomputed."""
    x, _, n, ch, m = _selfsim_pair(x, x, "selfsim_loss_backward")
    if not isinstance(state, (tuple, list)) or len(state) != 7:
        raise HipOpError("selfsim_loss_backward needs the state (inv_x, inv_c, r_x, r_c, t, pos, neg) of selfsim_loss")
    shp, pshape, dev = (n,) + tuple(x.shape[2:]), _selfsim_planes(x), x.device
    what = "selfsim_loss_backward: {}"
    u = _like(state[0], dev, torch.float32, what.format("inv_x"), shape=shp)
    rx = _like(state[2], dev, torch.float32, what.format("r_x"), shape=shp)
    t = _like(state[4], dev, torch.float32, what.format("t"), shape=shp)
    pos = _like(state[5], dev, torch.int64, what.format("pos"), shape=pshape)
    neg = _like(state[6], dev, torch.int64, what.format("neg"), shape=pshape)
    grad = _like(grad, dev, torch.float32, "grad", numel=1,
                 msg="selfsim_loss_backward needs a float32 device scalar grad")
    L = lib()
    nb = int(L.ast_selfsim_loss_backward_workspace_bytes(n, ch, m))
    wsb = _ws_bytes(nb, "selfsim_loss_backward workspace", dev)
    dx = torch.empty_like(x)
    check(_timed(f"selfsim_loss_backward {ch}ch {m}", 2 * n * m * m * ch, dev,
                 lambda: L.ast_selfsim_loss_backward_f32(
                     ptr(x), ptr(u), ptr(rx), ptr(t), ptr(pos), ptr(neg), ptr(grad), ptr(dx), n, ch, m, float(weight),
                     ptr(wsb), nb, stream_ptr(dev))), "selfsim_loss_backward")
    return dx


# Contextual loss (csrc/cx.hip): the limits of ast_hip.h
CX_MAX_C = 1024
CX_MAX_PIXELS = 1 << 14
CX_EPS = 1e-5


def _cx_pair(x: torch.Tensor, y: torch.Tensor, what: str, h: float = 0.5):
    """The checks of _remd_pair inside the limits of csrc/cx.hip, and a positive finite bandwidth:
    (x, y, n, ns, c, m, p)."""
    x, y, n, ns, c, m, p = _remd_pair(x, y, what)
    if c > CX_MAX_C or max(m, p) > CX_MAX_PIXELS:
        raise HipOpError(f"{what}: C is at most {CX_MAX_C} and a map has at most {CX_MAX_PIXELS} pixels: "
                         f"x {tuple(x.shape)} vs y {tuple(y.shape)}")
    h = float(h)
    if not (h > 0.0) or h == float("inf"):
        raise HipOpError(f"{what}: the bandwidth h must be positive and finite, got {h}")
    return x, y, n, ns, c, m, p


def cx_center(x: torch.Tensor, y: torch.Tensor):
    """(mu [Ns, C], xc, yc): the channel means of y [N or 1, C, Hs, Ws] over its pixels, summed in a fixed
    order, and both maps with them subtracted: the centring of the contextual loss."""
    x, y, n, ns, c, m, p = _cx_pair(x, y, "cx_center")
    mu = torch.empty((ns, c), device=x.device, dtype=torch.float32)
    xc, yc = torch.empty_like(x), torch.empty_like(y)
    check(lib().ast_cx_center_f32(ptr(x), ptr(y), ptr(mu), ptr(xc), ptr(yc), n, ns, c, m, p, stream_ptr(x.device)),
          "cx_center")
    return mu, xc, yc


def _cx_rows(x, y, inv_x, inv_y, row_min, what, n, ns, m, p):
    dev, f = x.device, torch.float32
    return (_like(inv_x, dev, f, f"{what}: inv_x", numel=n * m), _like(inv_y, dev, f, f"{what}: inv_y", numel=ns * p),
            _like(row_min, dev, f, f"{what}: row_min", numel=n * m))


def cx_rowsum(xc: torch.Tensor, yc: torch.Tensor, inv_x: torch.Tensor, inv_y: torch.Tensor, row_min: torch.Tensor,
              h: float = 0.5, _splits: int = 0):
    """(S, E) [N, H, W] of the contextual loss: with D the cosine distances of cosine_match(xc, yc), r its
    row minima and w(i, j) = exp((1 - D(i, j) / (r_i + eps)) / h), S_i = sum_j w(i, j) and E_i = sum_j w(i, j)
    D(i, j). The distances are never stored. _splits as in cosine_match."""
    x, y, n, ns, c, m, p = _cx_pair(xc, yc, "cx_rowsum", h)
    u, v, r = _cx_rows(x, y, inv_x, inv_y, row_min, "cx_rowsum", n, ns, m, p)
    L, dev = lib(), x.device
    nb = int(L.ast_cx_rowsum_workspace_bytes(n, ns, m, p, int(_splits)))
    wsb = _ws_bytes(nb, "cx_rowsum workspace", dev)
    S = torch.empty((n,) + tuple(x.shape[2:]), device=dev, dtype=torch.float32)
    E = torch.empty_like(S)
    check(_timed(f"cx_rowsum {c}ch {m} vs {p}", 2 * n * m * p * c, dev, lambda: L.ast_cx_rowsum_f32(
        ptr(x), ptr(y), ptr(u), ptr(v), ptr(r), ptr(S), ptr(E), n, ns, c, m, p, float(h), int(_splits), ptr(wsb), nb,
        stream_ptr(dev))), "cx_rowsum")
    return S, E


def cx_colmax(xc: torch.Tensor, yc: torch.Tensor, inv_x: torch.Tensor, inv_y: torch.Tensor, row_min: torch.Tensor,
              row_sum: torch.Tensor, h: float = 0.5, _splits: int = 0):
    """(col_cx [N, Hs, Ws], col_index int32, col_dist): c_j = max_i w(i, j) / S_i, its arg-max (the lowest
    index on equal values, a NaN never wins) and the distance D(a_j, j) there. Bit-equal for every
    _splits."""
    x, y, n, ns, c, m, p = _cx_pair(xc, yc, "cx_colmax", h)
    u, v, r = _cx_rows(x, y, inv_x, inv_y, row_min, "cx_colmax", n, ns, m, p)
    S = _like(row_sum, x.device, torch.float32, "cx_colmax: row_sum", numel=n * m)
    L, dev = lib(), x.device
    nb = int(L.ast_cx_colmax_workspace_bytes(n, ns, m, p))
    wsb = _ws_bytes(nb, "cx_colmax workspace", dev)
    shp = (n,) + tuple(y.shape[2:])
    ccx = torch.empty(shp, device=dev, dtype=torch.float32)
    cidx = torch.empty(shp, device=dev, dtype=torch.int32)
    cdist = torch.empty_like(ccx)
    check(_timed(f"cx_colmax {c}ch {m} vs {p}", 2 * n * m * p * c, dev, lambda: L.ast_cx_colmax_f32(
        ptr(x), ptr(y), ptr(u), ptr(v), ptr(r), ptr(S), ptr(ccx), ptr(cidx), ptr(cdist), n, ns, c, m, p, float(h),
        int(_splits), ptr(wsb), nb, stream_ptr(dev))), "cx_colmax")
    return ccx, cidx, cdist


def cx_value(col_cx: torch.Tensor, weight: float = 1.0, acc=None):
    """(loss, per_sample_cx [N]) from the column maxima of cx_colmax: CX_b = mean_j c_j, loss = weight *
    mean_b -log CX_b: the last stage of cx_loss. `acc`: the loss accumulator the value is added into."""
    if (not isinstance(col_cx, torch.Tensor) or col_cx.device.type != "cuda" or col_cx.dtype != torch.float32
            or col_cx.dim() < 2 or col_cx.numel() == 0):
        raise HipOpError("cx_value needs the float32 device column maxima [N, ...] of cx_colmax")
    col_cx, dev, n = col_cx.contiguous(), col_cx.device, int(col_cx.shape[0])
    cxb = torch.empty((n,), device=dev, dtype=torch.float32)
    acc = loss_accumulator(dev) if acc is None else acc
    check(lib().ast_cx_value_f32(ptr(col_cx), ptr(cxb), ptr(acc), n, col_cx.numel() // n, float(weight),
                                 stream_ptr(dev)), "cx_value")
    return acc[0], cxb


def cx_loss(x: torch.Tensor, y: torch.Tensor, weight: float = 1.0, h: float = 0.5, center: bool = True, acc=None):
    """The contextual loss (Mechrez et al., ECCV 2018), exact: weight * mean over the batch of -log CX_b,
    CX_b = mean_j max_i softmax-like CX(i, j) of the cosine distances between the pixels of x [N, C, H, W]
    (the differentiable side) and y [N or 1, C, Hs, Ws], normalised per row by the row minimum, bandwidth h;
    center subtracts y's channel means from both maps first. Returns (loss, per_sample_cx [N], state); state
    = (xc, yc, inv_x, inv_y, row_min, row_index, row_sum, row_dsum, col_cx, col_index, col_dist, per_sample_cx)
    is what cx_loss_backward reads; xc and yc are empty when center is off (the maps themselves are used).
    No M x P tensor is stored."""
    x, y, n, ns, c, m, p = _cx_pair(x, y, "cx_loss", h)
    L, dev = lib(), x.device
    nb = int(L.ast_cx_loss_workspace_bytes(n, ns, m, p))
    wsb = _ws_bytes(nb, "cx_loss workspace", dev)
    (hh, ww), (hs, ws) = x.shape[2:], y.shape[2:]
    f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
    if center:
        mu, xc, yc = torch.empty((ns, c), **f32), torch.empty_like(x), torch.empty_like(y)
    else:
        mu, xc, yc = None, torch.empty((0,), **f32), torch.empty((0,), **f32)
    u, v = torch.empty((n, hh, ww), **f32), torch.empty((ns, hs, ws), **f32)
    rmin, ridx = torch.empty((n, hh, ww), **f32), torch.empty((n, hh, ww), **i32)
    S, E = torch.empty((n, hh, ww), **f32), torch.empty((n, hh, ww), **f32)
    ccx, cidx, cdist = torch.empty((n, hs, ws), **f32), torch.empty((n, hs, ws), **i32), torch.empty((n, hs, ws), **f32)
    cxb = torch.empty((n,), **f32)
    acc = loss_accumulator(dev) if acc is None else acc
    pc = (lambda t: ptr(t)) if center else (lambda t: None)
    check(_timed(f"cx_loss {c}ch {m} vs {p}", 6 * n * m * p * c, dev, lambda: L.ast_cx_loss_f32(
        ptr(x), ptr(y), pc(mu), pc(xc), pc(yc), ptr(u), ptr(v), ptr(rmin), ptr(ridx), ptr(S), ptr(E), ptr(ccx),
        ptr(cidx), ptr(cdist), ptr(cxb), ptr(acc), n, ns, c, m, p, float(weight), float(h), 1 if center else 0,
        ptr(wsb), nb, stream_ptr(dev))), "cx_loss")
    return acc[0], cxb, (xc, yc, u, v, rmin, ridx, S, E, ccx, cidx, cdist, cxb)


def cx_loss_backward(x: torch.Tensor, y: torch.Tensor, state, grad: torch.Tensor, weight: float = 1.0,
                     h: float = 0.5) -> torch.Tensor:
    """d loss / d x [N, C, H, W] of cx_loss from its state, scaled by the device scalar `grad`; nothing flows
    to y. The inverse lists of the column arg-maxima, the row scalars, then a dense pass that recomputes
    the distances and the weights tile by tile and a finishing pass."""
    x, y, n, ns, c, m, p = _cx_pair(x, y, "cx_loss_backward", h)
    if not isinstance(state, (tuple, list)) or len(state) != 12:
        raise HipOpError("cx_loss_backward needs the state of cx_loss (12 tensors)")
    dev, f, what = x.device, torch.float32, "cx_loss_backward: {}"
    xc, yc = state[0], state[1]
    if isinstance(xc, torch.Tensor) and xc.numel() == 0 and isinstance(yc, torch.Tensor) and yc.numel() == 0:
        xc, yc = x, y   # center was off
    xc = _like(xc, dev, f, what.format("xc"), numel=x.numel())
    yc = _like(yc, dev, f, what.format("yc"), numel=y.numel())
    u = _like(state[2], dev, f, what.format("inv_x"), numel=n * m)
    v = _like(state[3], dev, f, what.format("inv_y"), numel=ns * p)
    rmin = _like(state[4], dev, f, what.format("row_min"), numel=n * m)
    ridx = _like(state[5], dev, torch.int32, what.format("row_index"), numel=n * m)
    S = _like(state[6], dev, f, what.format("row_sum"), numel=n * m)
    E = _like(state[7], dev, f, what.format("row_dsum"), numel=n * m)
    cidx = _like(state[9], dev, torch.int32, what.format("col_index"), numel=n * p)
    cdist = _like(state[10], dev, f, what.format("col_dist"), numel=n * p)
    cxb = _like(state[11], dev, f, what.format("per_sample_cx"), numel=n)
    grad = _like(grad, dev, f, what.format("grad"), numel=1)
    L = lib()
    nb = int(L.ast_cx_loss_backward_workspace_bytes(n, c, m, p))
    wsb = _ws_bytes(nb, "cx_loss_backward workspace", dev)
    dx = torch.empty_like(x)
    flops = 2 * n * m * p * c * ((c + 511) // 512 + 1)
    check(_timed(f"cx_loss_backward {c}ch {m} vs {p}", flops, dev, lambda: L.ast_cx_loss_backward_f32(
        ptr(xc), ptr(yc), ptr(u), ptr(v), ptr(rmin), ptr(ridx), ptr(S), ptr(E), ptr(cidx), ptr(cdist), ptr(cxb),
        ptr(grad), ptr(dx), n, ns, c, m, p, float(weight), float(h), ptr(wsb), nb, stream_ptr(dev))),
        "cx_loss_backward")
    return dx


# Moment-matching style loss (csrc/moment.hip): AST_MOMENT_MAX_C of ast_hip.h
MOMENT_MAX_C = 1024


def _moment_map(x: torch.Tensor, name: str, what: str):
    """An fp32 device NCHW map inside the limits of csrc/moment.hip: (x, n, c, pixels)."""
    x = _dev(x, name)
    if x.dim() != 4 or x.numel() == 0:
        raise HipOpError(f"{what} needs a non-empty NCHW map, got {name} {tuple(x.shape)}")
    n, c, m = int(x.shape[0]), int(x.shape[1]), int(x.shape[2] * x.shape[3])
    if c > MOMENT_MAX_C or m < 2 or n > 32767:
        raise HipOpError(f"{what}: C is at most {MOMENT_MAX_C}, a map has at least 2 pixels and a batch at most "
                         f"32767 samples: {name} {tuple(x.shape)}")
    return x, n, c, m


def moment_stats(y: torch.Tensor, _splits: int = 0):
    """(mean [N, C], cov [N, C, C]) of the pixels of y [N, C, H, W]: cov = (Y - mean)(Y - mean)^T / (HW - 1)
    with no ridge, symmetric in bits. The target side of moment_loss: compute it once per style.
    _splits (tests) forces the number of pixel splits (0: the library's choice)."""
    y, n, c, p = _moment_map(y, "y", "moment_stats")
    L, dev = lib(), y.device
    nb = int(L.ast_moment_stats_workspace_bytes(n, c, p, int(_splits)))
    wsb = _ws_bytes(nb, "moment_stats workspace", dev)
    mean = torch.empty((n, c), device=dev, dtype=torch.float32)
    cov = torch.empty((n, c, c), device=dev, dtype=torch.float32)
    pairs = ((c + 63) // 64) * ((c + 63) // 64 + 1) // 2
    check(_timed(f"moment_stats {c}ch {p}", 2 * n * pairs * 4096 * p, dev, lambda: L.ast_moment_stats_f32(
        ptr(y), ptr(mean), ptr(cov), n, c, p, int(_splits), ptr(wsb), nb, stream_ptr(dev))), "moment_stats")
    return mean, cov


def moment_loss(x: torch.Tensor, y_mean: torch.Tensor, y_cov: torch.Tensor, weight: float = 1.0, acc=None,
                _splits: int = 0):
    """The moment-matching style loss of STROTSS (Kolkin et al., CVPR 2019) between x [N, C, H, W] and the
    statistics (y_mean [Ns, C], y_cov [Ns, C, C], Ns = N or 1) of moment_stats: weight * mean over the batch
    of mean_c |mu_x - mu_y| + mean_ij |Cov_x - Cov_y|. Returns (loss, state) with state = (mean_x [N, C],
    sign_mu int8 [N, C], sign_cov int8 [N, C, C], sums [N], the per-sample terms): what moment_loss_backward
    reads. Cov_x is never stored. `acc`: the loss accumulator the value is added into (a fresh one if
    None)."""
    x, n, c, m = _moment_map(x, "x", "moment_loss")
    L, dev = lib(), x.device
    if not isinstance(y_mean, torch.Tensor) or y_mean.dim() != 2 or y_mean.shape[0] not in (1, n):
        raise HipOpError(f"moment_loss: y_mean must be [N or 1, {c}], got "
                         f"{tuple(y_mean.shape) if isinstance(y_mean, torch.Tensor) else y_mean!r}")
    ns = int(y_mean.shape[0])
    y_mean = _like(y_mean, dev, torch.float32, "moment_loss: y_mean", shape=(ns, c))
    y_cov = _like(y_cov, dev, torch.float32, "moment_loss: y_cov", shape=(ns, c, c))
    nb = int(L.ast_moment_loss_workspace_bytes(n, c, m, int(_splits)))
    wsb = _ws_bytes(nb, "moment_loss workspace", dev)
    mean_x = torch.empty((n, c), device=dev, dtype=torch.float32)
    sign_mu = torch.empty((n, c), device=dev, dtype=torch.int8)
    sign_cov = torch.empty((n, c, c), device=dev, dtype=torch.int8)
    sums = torch.empty((n,), device=dev, dtype=torch.float32)
    acc = loss_accumulator(dev) if acc is None else acc
    pairs = ((c + 63) // 64) * ((c + 63) // 64 + 1) // 2
    check(_timed(f"moment_loss {c}ch {m}", 2 * n * pairs * 4096 * m, dev, lambda: L.ast_moment_loss_f32(
        ptr(x), ptr(y_mean), ptr(y_cov), ptr(mean_x), ptr(sign_mu), ptr(sign_cov), ptr(sums), ptr(acc), n, ns, c, m,
        float(weight), int(_splits), ptr(wsb), nb, stream_ptr(dev))), "moment_loss")
    return acc[0], (mean_x, sign_mu, sign_cov, sums)


def moment_loss_backward(x: torch.Tensor, state, grad: torch.Tensor = None, weight: float = 1.0,
                         out: torch.Tensor = None) -> torch.Tensor:
    """d loss / d x [N, C, H, W] of moment_loss from its state, scaled by the device scalar `grad` (None:
    1); nothing flows to the target. One GEMM launch, sign_cov (X - mean_x) per sample. With `out` the
    gradient is added into it."""
    x, n, c, m = _moment_map(x, "x", "moment_loss_backward")
    if not isinstance(state, (tuple, list)) or len(state) < 3:
        raise HipOpError("moment_loss_backward needs the state of moment_loss")
    dev, what = x.device, "moment_loss_backward: {}"
    mean_x = _like(state[0], dev, torch.float32, what.format("mean_x"), shape=(n, c))
    sign_mu = _like(state[1], dev, torch.int8, what.format("sign_mu"), shape=(n, c))
    sign_cov = _like(state[2], dev, torch.int8, what.format("sign_cov"), shape=(n, c, c))
    if grad is not None:
        grad = _like(grad.reshape(()) if isinstance(grad, torch.Tensor) and grad.numel() == 1 else grad, dev,
                     torch.float32, what.format("grad"), shape=())
    if out is not None:
        if not isinstance(out, torch.Tensor) or not out.is_contiguous():
            raise HipOpError("moment_loss_backward: out must be a contiguous tensor")
        out = _like(out, dev, torch.float32, what.format("out"), shape=x.shape)
    dx = out if out is not None else torch.empty_like(x)
    check(_timed(f"moment_loss_backward {c}ch {m}", 2 * n * c * c * m, dev, lambda: lib().ast_moment_loss_backward_f32(
        ptr(x), ptr(mean_x), ptr(sign_mu), ptr(sign_cov), ptr(grad), ptr(dx), n, c, m, float(weight),
        1 if out is not None else 0, stream_ptr(dev))), "moment_loss_backward")
    return dx


# Guided style swap (csrc/swap.hip): a class >= SWAP_MAX_CLASSES takes no part in the match
SWAP_MAX_CLASSES = 64
_SWAP_NO_SKIP = 1   # AST_SWAP_NO_SKIP


def patch_classes(labels: torch.Tensor) -> torch.Tensor:
    """One class per 3x3 patch from a feature-resolution label map uint8 [B, h, w]: the label of the
    patch's centre pixel, labels[:, 1:-1, 1:-1], as a dense uint8 [B, h - 2, w - 2]."""
    if (not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3
            or min(labels.shape[1:]) < 3):
        raise HipOpError("patch_classes needs a uint8 label map [B, h, w] with sides of at least 3")
    return labels[:, 1:-1, 1:-1].contiguous()


def _bank_patches(s: int, hs: int, ws: int, what: str) -> int:
    """S * (Hs - 2) * (Ws - 2), the number of style patches of a bank; it must stay below 2^31, the global
    patch index being an int32."""
    total = int(s) * (int(hs) - 2) * (int(ws) - 2)
    if total >= 2 ** 31:
        raise HipOpError(f"{what}: a bank of {s} styles {hs}x{ws} has {total} style patches, 2^31 or more")
    return total


def _swap_bank(a: torch.Tensor, b: torch.Tensor, na: str, nb: str, what: str):
    """Content-side maps a [N, C, H, W] and a style bank b [S, C, Hs, Ws] (fp32, on one device, equal C,
    sides of at least 3, S * (Hs - 2) * (Ws - 2) < 2^31): (a, b, n, S, c, ha, wa, hb, wb)."""
    a, b, n, s, c, ha, wa, hb, wb = _pair(a, b, na, nb, what, batch=False, side=3)
    _bank_patches(s, hb, wb, what)
    return a, b, n, s, c, ha, wa, hb, wb


def _swap_classes(cls, shape, device, name):
    """A class map for `shape` patches: None (all 0) or a uint8 tensor of that shape on `device`."""
    if cls is None:
        return torch.zeros(shape, device=device, dtype=torch.uint8)
    return _like(cls, device, torch.uint8, name, shape=shape,
                 msg=f"{name} must be a uint8 tensor {tuple(shape)} on {device}")


def patch_match_guided(content_key: torch.Tensor, style_keys: torch.Tensor, content_class: torch.Tensor,
                       style_class: torch.Tensor, return_score: bool = False, _splits: int = 0, _skip: bool = True):
    """patch_match under class guidance over a bank of styles. style_keys [S, C, Hs, Ws] is shared by the
    batch; content_class uint8 [N, H - 2, W - 2] and style_class uint8 [S, Hs - 2, Ws - 2] give one class
    per patch (None: all 0; patch_classes makes them from label maps). A content patch is matched
    against the style patches of its own class only; a class >= SWAP_MAX_CLASSES takes no part. Returns
    the global index s * (Hs - 2) * (Ws - 2) + jy * (Ws - 2) + jx, int32 [N, H - 2, W - 2] (the lowest on
    equal scores), -1 with score -inf where a patch has no candidate. Scores are those of patch_match,
    bit for bit. (content tile, bank tile) pairs that share no class are skipped. _splits as in
    patch_match; _skip=False visits every tile (the same result)."""
    ck, sk, n, s, c, hc, wc, hs, ws = _swap_bank(content_key, style_keys, "content_key", "style_keys",
                                                 "patch_match_guided")
    L, dev, st = lib(), ck.device, stream_ptr(ck.device)
    cc = _swap_classes(content_class, (n, hc - 2, wc - 2), dev, "content_class")
    sc = _swap_classes(style_class, (s, hs - 2, ws - 2), dev, "style_class")
    nb = int(L.ast_patch_norms_workspace_bytes(s, hs, ws))
    wsn = _ws_bytes(nb, "patch_norms workspace", dev)
    inv = torch.empty((s, hs - 2, ws - 2), device=dev, dtype=torch.float32)
    check(L.ast_patch_norms_f32(ptr(sk), ptr(inv), s, c, hs, ws, ptr(wsn), nb, st), "patch_norms")
    mb = int(L.ast_patch_match_guided_workspace_bytes(n, s, hc, wc, hs, ws, int(_splits)))
    wsm = _ws_bytes(mb, "patch_match_guided workspace", dev)
    index = torch.empty((n, hc - 2, wc - 2), device=dev, dtype=torch.int32)
    score = torch.empty((n, hc - 2, wc - 2), device=dev, dtype=torch.float32) if return_score else None
    flops = 2 * n * (hc - 2) * (wc - 2) * s * (hs - 2) * (ws - 2) * 9 * c     # an upper bound: nothing skipped
    check(_timed(f"patch_match_guided {c}ch {hc}x{wc} vs {s}x{hs}x{ws}", flops, dev,
                 lambda: L.ast_patch_match_guided_ex_f32(
                     ptr(ck), ptr(sk), ptr(inv), ptr(cc), ptr(sc), ptr(index), ptr(score), n, s, c, hc, wc, hs, ws,
                     int(_splits), 0 if _skip else _SWAP_NO_SKIP, ptr(wsm), mb, st)), "patch_match_guided")
    return (index, score) if return_score else index


def patch_gather_guided(style_values: torch.Tensor, index: torch.Tensor, content: torch.Tensor, alpha: float = 1.0):
    """patch_gather for the guided match: style_values [S, C, Hs, Ws] is the bank, index int32
    [N, H - 2, W - 2] global over it; a negative index is "no match" and adds no term to the overlap
    average; a pixel none of whose covering patches has a match is a copy of the content. One launch."""
    c_, sv, n, s, c, hc, wc, hs, ws = _swap_bank(content, style_values, "content_map", "style_values",
                                                 "patch_gather_guided")
    index = _like(index, c_.device, torch.int32, "index", shape=(n, hc - 2, wc - 2),
                  msg=f"index must be an int32 tensor {(n, hc - 2, wc - 2)} on {c_.device}")
    out = torch.empty_like(c_)
    check(_timed(f"patch_gather_guided {c}ch {hc}x{wc}", -4 * 11 * c_.numel(), c_.device,
                 lambda: lib().ast_patch_gather_guided_f32(ptr(sv), ptr(index), ptr(c_), ptr(out), n, s, c, hc, wc, hs,
                                                           ws, float(alpha), stream_ptr(c_.device))),
          "patch_gather_guided")
    return out


def style_swap_guided(content: torch.Tensor, styles: torch.Tensor, content_class: torch.Tensor = None,
                      style_class: torch.Tensor = None, alpha: float = 1.0, normalize: bool = False,
                      return_index: bool = False):
    """Guided style swap (semantic style transfer by patches): every 3x3 patch of content [N, C, H, W] is
    replaced by the most similar 3x3 patch of its own class from the bank styles [S, C, Hs, Ws]
    (patch_match_guided), the overlaps of the matched patches are averaged and blended with the content
    by alpha (patch_gather_guided); where nothing matched the content stays. Classes as in
    patch_match_guided (None: all 0). normalize=True matches on mean_variance_norm of every map and
    reconstructs from the raw style features, as style_swap does. return_index adds the int32 match."""
    c_, s_, n, s, c, hc, wc, hs, ws = _swap_bank(content, styles, "content_map", "style_maps", "style_swap_guided")
    cc = _swap_classes(content_class, (n, hc - 2, wc - 2), c_.device, "content_class")
    sc = _swap_classes(style_class, (s, hs - 2, ws - 2), c_.device, "style_class")
    ck, sk = (mean_variance_norm(c_), mean_variance_norm(s_)) if normalize else (c_, s_)
    L = lib()
    nbytes = int(L.ast_style_swap_guided_workspace_bytes(n, s, hc, wc, hs, ws))
    wsb = _ws_bytes(nbytes, "style_swap_guided workspace", c_.device)
    out = torch.empty_like(c_)
    index = torch.empty((n, hc - 2, wc - 2), device=c_.device, dtype=torch.int32) if return_index else None
    flops = 2 * n * (hc - 2) * (wc - 2) * s * (hs - 2) * (ws - 2) * 9 * c     # an upper bound: nothing skipped
    check(_timed(f"style_swap_guided {c}ch {hc}x{wc} vs {s}x{hs}x{ws}", flops, c_.device,
                 lambda: L.ast_style_swap_guided_f32(
                     ptr(ck), ptr(sk), ptr(s_), ptr(c_), ptr(cc), ptr(sc), ptr(out), ptr(index), None, n, s, c, hc, wc,
                     hs, ws, float(alpha), ptr(wsb), nbytes, stream_ptr(c_.device))), "style_swap_guided")
    return (out, index) if return_index else out


# Feature k-means and the label mode filter (csrc/kmeans.hip): the limits of ast_hip.h
KMEANS_MAX_C = 1024
KMEANS_MAX_POINTS = 1 << 24
KMEANS_DEFAULT_ITERS = 10


def _kmeans_bank(x: torch.Tensor, what: str):
    """An fp32 device bank [B, C, H, W] within the limits: (x, b, c, h, w)."""
    x = _dev(x, "x")
    if x.dim() != 4 or x.numel() == 0:
        raise HipOpError(f"{what} needs a non-empty NCHW bank, got {tuple(x.shape)}")
    b, c, h, w = (int(s) for s in x.shape)
    if c > KMEANS_MAX_C or b * h * w > KMEANS_MAX_POINTS:
        raise HipOpError(f"{what}: at most {KMEANS_MAX_C} channels and {KMEANS_MAX_POINTS} points, got "
                         f"{c} channels and {b * h * w} points")
    return x, b, c, h, w


def _kmeans_centroids(cen, c: int, device, name: str):
    """fp32 centroids [K, C] on `device`, K in 1..MAX_REGIONS: (centroids, k)."""
    cen = _dev(cen, name)
    if cen.dim() != 2 or cen.shape[1] != c or not 1 <= cen.shape[0] <= MAX_REGIONS or cen.device != device:
        raise HipOpError(f"{name} must be [K <= {MAX_REGIONS}, C={c}] on {device}, got {tuple(cen.shape)} "
                         f"on {cen.device}")
    return cen, int(cen.shape[0])


def _count(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise HipOpError(f"{name} must be an int >= 0, got {v!r}")
    return v


def kmeans_seed(x: torch.Tensor, k: int):
    """The k maximin seeds of the bank x [B, C, H, W] (point g = b * H * W + pixel, all points together):
    the point farthest from the mean of all points, then repeatedly the point farthest from the seeds
    so far; ties to the lowest g. int32 [k] of global point indices."""
    k = _regions(k)
    x, b, c, h, w = _kmeans_bank(x, "kmeans_seed")
    L = lib()
    nbytes = int(L.ast_kmeans_workspace_bytes(b, c, h, w, k))
    wsb = _ws_bytes(nbytes, "kmeans workspace", x.device)
    seeds = torch.empty((k,), device=x.device, dtype=torch.int32)
    check(L.ast_kmeans_seed_f32(ptr(x), ptr(seeds), b, c, h, w, k, ptr(wsb), nbytes, stream_ptr(x.device)),
          "kmeans_seed")
    return seeds


def kmeans_assign(x: torch.Tensor, centroids: torch.Tensor):
    """The nearest of centroids [K, C] for every point of x [B, C, H, W], by the squared distance over the
    channels: uint8 [B, H, W]. The lowest k wins on equal distances; a NaN never wins, and a point without
    a winner gets 255, the "no region" label of the regional ops. One launch."""
    x, b, c, h, w = _kmeans_bank(x, "kmeans_assign")
    cen, k = _kmeans_centroids(centroids, c, x.device, "centroids")
    labels = torch.empty((b, h, w), device=x.device, dtype=torch.uint8)
    check(_timed(f"kmeans_assign {c}ch {b}x{h}x{w} K{k}", -(4 * x.numel() + labels.numel()), x.device,
                 lambda: lib().ast_kmeans_assign_f32(ptr(x), ptr(cen), ptr(labels), b, c, h, w, k,
                                                     stream_ptr(x.device))), "kmeans_assign")
    return labels


def kmeans_update(x: torch.Tensor, labels: torch.Tensor, centroids: torch.Tensor):
    """One centroid update: (centroids [K, C], counts int32 [K]), centroid k the mean of the points of x
    labelled k (labels uint8 [B, H, W]; a label >= K belongs to no cluster), a cluster without points
    keeping its row of `centroids` bit for bit. Deterministic: partial sums per workgroup, added in a
    fixed order, no atomics."""
    x, labels, b, c, h, w = _map_and_labels(x, labels, "x")
    x, b, c, h, w = _kmeans_bank(x, "kmeans_update")
    cen, k = _kmeans_centroids(centroids, c, x.device, "centroids")
    L = lib()
    nbytes = int(L.ast_kmeans_workspace_bytes(b, c, h, w, k))
    wsb = _ws_bytes(nbytes, "kmeans workspace", x.device)
    out = torch.empty_like(cen)
    counts = torch.empty((k,), device=x.device, dtype=torch.int32)
    check(L.ast_kmeans_update_f32(ptr(x), ptr(labels), ptr(cen), ptr(out), ptr(counts), b, c, h, w, k, ptr(wsb),
                                  nbytes, stream_ptr(x.device)), "kmeans_update")
    return out, counts


def kmeans(x: torch.Tensor, k: int, iters: int = KMEANS_DEFAULT_ITERS, init: torch.Tensor = None):
    """Deterministic k-means (Lloyd) over the points of the bank x [B, C, H, W]: (centroids [k, C],
    labels uint8 [B, H, W], counts int32 [k]). The initial centroids are the points at the maximin
    seeds (kmeans_seed), or `init` [k, C]; then `iters` rounds of assign and update -- per round one
    launch that reads the bank once, and a small reduction -- and one final assign, so labels and counts
    belong to the returned centroids. The number of rounds is fixed, there is no convergence test and
    no host synchronisation (the op can be captured into a graph); iters=0 gives the initial centroids
    and one assign. The default of 10 rounds is a definitional constant, not a measured optimum."""
    k, iters = _regions(k), _count(iters, "iters")
    x, b, c, h, w = _kmeans_bank(x, "kmeans")
    if init is not None:
        init, ki = _kmeans_centroids(init, c, x.device, "init")
        if ki != k:
            raise HipOpError(f"init must have k = {k} rows, got {ki}")
    L = lib()
    nbytes = int(L.ast_kmeans_workspace_bytes(b, c, h, w, k))
    wsb = _ws_bytes(nbytes, "kmeans workspace", x.device)
    cen = torch.empty((k, c), device=x.device, dtype=torch.float32)
    labels = torch.empty((b, h, w), device=x.device, dtype=torch.uint8)
    counts = torch.empty((k,), device=x.device, dtype=torch.int32)
    # algorithmic bytes: the bank once per round and once more for the final assign (the seeding's k + 1
    # reads on top when there is no init), the labels written each time
    reads = iters + 1 + (0 if init is not None else k + 1)
    check(_timed(f"kmeans {c}ch {b}x{h}x{w} K{k} x{iters}", -(reads * 4 * x.numel() + (iters + 1) * labels.numel()),
                 x.device, lambda: L.ast_kmeans_f32(ptr(x), ptr(init), ptr(cen), ptr(labels), ptr(counts), None, b, c,
                                                    h, w, k, iters, ptr(wsb), nbytes, stream_ptr(x.device))), "kmeans")
    return cen, labels, counts


def label_mode_filter(labels: torch.Tensor, regions: int, passes: int = 1):
    """`passes` rounds of a 3x3 majority vote over uint8 label maps [N, H, W] (window clipped at the
    borders): only labels < regions vote, the most frequent wins, on a tie the centre's own label if it
    is among the tied, else the lowest; a pixel labelled >= regions passes through. Exact."""
    regions, passes = _regions(regions), _count(passes, "passes")
    labels = _labels(labels, "labels")
    n, h, w = (int(s) for s in labels.shape)
    L = lib()
    nbytes = int(L.ast_label_mode_filter_workspace_bytes(n, h, w, passes))
    wsb = _ws_bytes(nbytes, "label_mode_filter workspace", labels.device)
    out = torch.empty_like(labels)
    check(L.ast_label_mode_filter_u8(ptr(labels), ptr(out), n, h, w, regions, passes, ptr(wsb), nbytes,
                                     stream_ptr(labels.device)), "label_mode_filter")
    return out


def adain_bf16(content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0, swap_style_stats: bool = True):
    """AdaIN on bf16 maps (fp32 statistics and arithmetic, bf16 result)."""
    content = _dev_typed(content, "content_map", torch.bfloat16)
    style = _dev_typed(style, "style_map", torch.bfloat16)
    if content.dim() != 4 or style.dim() != 4 or content.shape[:2] != style.shape[:2]:
        raise HipOpError(f"AdaIN needs NCHW maps with equal (N, C): {tuple(content.shape)} vs {tuple(style.shape)}")
    n, c, hc, wc = (int(s) for s in content.shape)
    hs, ws = int(style.shape[2]), int(style.shape[3])
    out = torch.empty_like(content)
    nbytes = 2 * (2 * content.numel() + style.numel())
    check(_timed(f"adain bf16 {c}ch {hc}x{wc}", -nbytes, content.device, lambda: lib().ast_adain_bf16(
        ptr(content), ptr(style), ptr(out), n, c, hc, wc, hs, ws, float(alpha), 1 if swap_style_stats else 0,
        stream_ptr(content.device))), "adain_bf16")
    return out


# ------------------------------------------------------------------------------------------------
# Colour spaces (model_util.py:11-140) and colour-preserving recombination
# ------------------------------------------------------------------------------------------------

COLOR_MODES = {"rgb2xyz": 0, "xyz2rgb": 1, "xyz2lab": 2, "lab2xyz": 3, "rgb2lab": 4, "lab2rgb": 5}  # AST_COLOR_*


def _color_mode(mode) -> int:
    code = COLOR_MODES.get(mode, mode)
    if isinstance(code, bool) or not isinstance(code, int) or not 0 <= code < len(COLOR_MODES):
        raise HipOpError(f"colour mode must be one of {list(COLOR_MODES)}, got {mode!r}")
    return code


def _color_image(t: torch.Tensor, name: str) -> torch.Tensor:
    dt = t.dtype if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 else torch.float32
    t = _dev_typed(t, name, dt)
    if t.dim() != 4 or t.shape[1] != 3:
        raise HipOpError(f"{name} must be [N, 3, H, W], got {tuple(t.shape)}")
    if t.numel() == 0:
        raise HipOpError(f"{name} is empty: {tuple(t.shape)}")
    return t


def color_convert(x: torch.Tensor, mode, out_dtype: torch.dtype = torch.float32):
    """One of the six conversions of model_util.py:11-140 (`mode`: a COLOR_MODES name or its code)
    on an [N, 3, H, W] image, fp32 or bf16. The result is fp32 by default, as the reference
    returns for either input; out_dtype=torch.bfloat16 (bf16 input only) keeps bf16 storage."""
    code = _color_mode(mode)
    x = _color_image(x, "x")
    n, hw = int(x.shape[0]), int(x.shape[2] * x.shape[3])
    L = lib()
    if x.dtype == torch.float32 and out_dtype == torch.float32:
        fn = L.ast_color_convert_f32
    elif x.dtype == torch.bfloat16 and out_dtype == torch.float32:
        fn = L.ast_color_convert_bf16_f32
    elif x.dtype == torch.bfloat16 and out_dtype == torch.bfloat16:
        fn = L.ast_color_convert_bf16
    else:
        raise HipOpError(f"color_convert runs fp32->fp32, bf16->fp32 and bf16->bf16, not {x.dtype}->{out_dtype}")
    out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    nbytes = x.numel() * (x.element_size() + out.element_size())   # algorithmic: read x, write out
    name = mode if isinstance(mode, str) else list(COLOR_MODES)[code]
    check(_timed(f"color {name} {x.shape[2]}x{x.shape[3]}", -nbytes, x.device, lambda: fn(
        ptr(x), ptr(out), n, hw, code, stream_ptr(x.device))), "color_convert")
    return out


def color_convert_backward(x: torch.Tensor, g: torch.Tensor, mode):
    """J^T g of color_convert at x (fp32): the selected branch's derivative, zero where a clamp is
    active; finite where the reference's autograd is NaN through its unselected branch."""
    code = _color_mode(mode)
    x, g = _dev(x, "x"), _dev(g, "grad")
    if x.dim() != 4 or x.shape[1] != 3 or g.shape != x.shape or x.numel() == 0:
        raise HipOpError(f"color_convert_backward needs equal [N, 3, H, W] x and grad: "
                         f"{tuple(x.shape)} vs {tuple(g.shape)}")
    n, hw = int(x.shape[0]), int(x.shape[2] * x.shape[3])
    dx = torch.empty_like(x)
    check(_timed(f"color bwd {code} {x.shape[2]}x{x.shape[3]}", -4 * 3 * x.numel(), x.device,
                 lambda: lib().ast_color_convert_backward_f32(ptr(x), ptr(g), ptr(dx), n, hw, code,
                                                              stream_ptr(x.device))), "color_convert_backward")
    return dx


def luma_transfer(stylised: torch.Tensor, content: torch.Tensor):
    """Colour-preserving recombination in one launch: the Lab luminance of clamp01(stylised) with
    the a, b of clamp01(content), back to RGB. Both [N, 3, H, W], both fp32 or both bf16."""
    stylised = _color_image(stylised, "stylised")
    content = _color_image(content, "content")
    if stylised.shape != content.shape or stylised.dtype != content.dtype or stylised.device != content.device:
        raise HipOpError(f"luma_transfer needs equal shapes and dtypes: {tuple(stylised.shape)} {stylised.dtype} vs "
                         f"{tuple(content.shape)} {content.dtype}")
    n, hw = int(content.shape[0]), int(content.shape[2] * content.shape[3])
    out = torch.empty_like(content)
    fn = lib().ast_luma_transfer_bf16 if content.dtype == torch.bfloat16 else lib().ast_luma_transfer_f32
    nbytes = 3 * content.numel() * content.element_size()
    check(_timed(f"luma_transfer {content.shape[2]}x{content.shape[3]}", -nbytes, content.device, lambda: fn(
        ptr(stylised), ptr(content), ptr(out), n, hw, stream_ptr(content.device))), "luma_transfer")
    return out


# ------------------------------------------------------------------------------------------------
# Bilinear resize, its adjoint and the Laplacian pyramid (csrc/pyramid.hip)
# ------------------------------------------------------------------------------------------------

RESIZE_MAX_SIDE = 4096


def _resize_size(size, what: str):
    try:
        h, w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise HipOpError(f"{what} must be (height, width), got {size!r}") from None
    if not (1 <= h <= RESIZE_MAX_SIDE and 1 <= w <= RESIZE_MAX_SIDE):
        raise HipOpError(f"{what} must have sides in 1..{RESIZE_MAX_SIDE}, got {(h, w)}")
    return h, w


def _resize_planes(t: torch.Tensor, name: str) -> torch.Tensor:
    t = _dev(t, name)
    if t.dim() < 2 or t.numel() == 0:
        raise HipOpError(f"{name} must be [..., H, W] and not empty, got {tuple(t.shape)}")
    _resize_size(t.shape[-2:], f"{name}'s size")
    return t


def resize_bilinear(x: torch.Tensor, size, add: torch.Tensor = None, sign: float = 1.0):
    """F.interpolate(x, size, mode="bilinear", align_corners=False, antialias=False) on the planes
    of x [..., h, w] (fp32), any ratio; with `add` [..., H, W] the result is add + sign * resize(x)
    in the same launch (a level of lap_build / lap_collapse)."""
    x = _resize_planes(x, "x")
    h, w = int(x.shape[-2]), int(x.shape[-1])
    H, W = _resize_size(size, "size")
    shape = tuple(x.shape[:-2]) + (H, W)
    if add is not None:
        add = _dev(add, "add")
        if tuple(add.shape) != shape or add.device != x.device:
            raise HipOpError(f"resize_bilinear: add must be {shape} on {x.device}, got {tuple(add.shape)} on "
                             f"{add.device}")
    planes = x.numel() // (h * w)
    out = torch.empty(shape, device=x.device, dtype=torch.float32)
    nbytes = 4 * (x.numel() + out.numel() * (2 if add is not None else 1))
    check(_timed(f"resize {h}x{w}->{H}x{W}", -nbytes, x.device, lambda: lib().ast_resize_bilinear_f32(
        ptr(x), ptr(out), planes, h, w, H, W, ptr(add), float(sign), stream_ptr(x.device))),
        "resize_bilinear")
    return out


def resize_bilinear_adjoint(g: torch.Tensor, in_size, out: torch.Tensor = None):
    """The transpose of resize_bilinear: g [..., H, W] -> [..., h, w] with in_size = (h, w), so that
    <resize(x), g> = <x, adjoint(g)>. With `out` [..., h, w] the result is added into it."""
    g = _resize_planes(g, "grad")
    H, W = int(g.shape[-2]), int(g.shape[-1])
    h, w = _resize_size(in_size, "in_size")
    shape = tuple(g.shape[:-2]) + (h, w)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape
                or out.device != g.device or not out.is_contiguous()):
            raise HipOpError(f"resize_bilinear_adjoint: out must be a contiguous float32 {shape} on {g.device}")
        dx = out
    else:
        dx = torch.empty(shape, device=g.device, dtype=torch.float32)
    planes = g.numel() // (H * W)
    nbytes = 4 * (g.numel() + dx.numel() * (2 if out is not None else 1))
    check(_timed(f"resize adjoint {H}x{W}->{h}x{w}", -nbytes, g.device, lambda: lib().ast_resize_bilinear_adjoint_f32(
        ptr(g), ptr(dx), planes, h, w, H, W, 1 if out is not None else 0, stream_ptr(g.device))),
        "resize_bilinear_adjoint")
    return dx


def lap_down_size(size):
    """The next coarser pyramid size: (max(h // 2, 1), max(w // 2, 1))."""
    return max(int(size[0]) // 2, 1), max(int(size[1]) // 2, 1)


def lap_build(x: torch.Tensor, levels: int):
    """The Laplacian pyramid of STROTSS on x [..., H, W]: for l in 0..levels-1,
    lap_l = cur - resize(down(cur), size(cur)) and cur = down(cur), with down the bilinear resize
    to lap_down_size. Returns [lap_0, ..., lap_{levels-1}, cur]: two launches per level."""
    if isinstance(levels, bool) or not isinstance(levels, int) or levels < 0:
        raise HipOpError(f"lap_build: levels must be an int >= 0, got {levels!r}")
    cur = _resize_planes(x, "x")
    pyr = []
    for _ in range(levels):
        small = resize_bilinear(cur, lap_down_size(cur.shape[-2:]))
        pyr.append(resize_bilinear(small, cur.shape[-2:], add=cur, sign=-1.0))
        cur = small
    pyr.append(cur)
    return pyr


def lap_collapse(pyr):
    """The inverse of lap_build: cur = pyr[-1], then from coarse to fine
    cur = pyr[l] + resize(cur, size(pyr[l])); one launch per level."""
    pyr = list(pyr)
    if not pyr:
        raise HipOpError("lap_collapse: the pyramid is empty")
    cur = _resize_planes(pyr[-1], "pyr[-1]")
    for l in range(len(pyr) - 2, -1, -1):
        lvl = _resize_planes(pyr[l], f"pyr[{l}]")
        if lvl.shape[:-2] != cur.shape[:-2]:
            raise HipOpError(f"lap_collapse: pyr[{l}] is {tuple(lvl.shape)} but the coarser level is "
                             f"{tuple(cur.shape)}")
        cur = resize_bilinear(cur, lvl.shape[-2:], add=lvl, sign=1.0)
    return cur


def plane_normalize(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor):
    x = _dev(x, "x")
    mean, std = _dev(mean, "mean"), _dev(std, "std")
    n, c = x.shape[:2]
    hw = x.numel() // (n * c)
    out = torch.empty_like(x)
    check(lib().ast_plane_normalize_f32(ptr(x), ptr(mean), ptr(std), ptr(out), n * c, hw,
                                        stream_ptr(x.device)), "plane_normalize")
    return out


def mean_variance_norm(x: torch.Tensor):
    """models.py:64-68 (unbiased var + 1e-5)."""
    mean, std = channel_stats(x, unbiased=True, eps=1e-5)
    return plane_normalize(x, mean, std)


# ------------------------------------------------------------------------------------------------
# AdaAttN (models.py:70-115)
# ------------------------------------------------------------------------------------------------

ADAATTN_MAX_CHANNELS = 128


def adaattn(content: torch.Tensor, style: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor):
    """AdaAttN.forward (models.py:81-115) as HIP launches: instance-norm statistics, the Q/K/V 1x1
    projections, and one fused attention kernel (scores, online softmax, attention-weighted mean
    and std, `std * IN(content) + mean`); the Nq x Nk attention matrix is never materialised.
    content [N, C, H, W], style [N, C, Hs, Ws], both fp32 or both bf16 (bf16 storage, fp32
    accumulation); wq/wk/wv are the [C, C, 1, 1] (or [C, C]) Conv2d weights (any float dtype)."""
    if not isinstance(content, torch.Tensor) or not isinstance(style, torch.Tensor):
        raise TypeError("content_map and style_map must be tensors")
    if content.dtype == torch.bfloat16:
        dtype_code, content = 1, _dev_typed(content, "content_map", torch.bfloat16)
        style = _dev_typed(style, "style_map", torch.bfloat16)
    else:
        dtype_code, content, style = 0, _dev(content, "content_map"), _dev(style, "style_map")
    if content.dim() != 4 or style.dim() != 4 or content.shape[:2] != style.shape[:2]:
        raise HipOpError(f"AdaAttN needs NCHW maps with equal (N, C): {tuple(content.shape)} vs {tuple(style.shape)}")
    n, c, hc, wc = (int(s) for s in content.shape)
    hs, ws = int(style.shape[2]), int(style.shape[3])
    if hc * wc == 1 or hs * ws == 1:   # InstanceNorm2d's own error (models.py:78-80)
        raise ValueError("Expected more than 1 spatial element when training (InstanceNorm2d in AdaAttN)")
    if c > ADAATTN_MAX_CHANNELS:
        raise HipOpError(f"AdaAttN HIP kernel supports C <= {ADAATTN_MAX_CHANNELS}, got {c}")
    w = []
    for name, t in (("W_q", wq), ("W_k", wk), ("W_v", wv)):
        if t.device.type != "cuda":
            raise HipOpError(f"{name} is on {t.device}; arbitrarystyletransfer_amd runs on MI355X (HIP) devices only")
        t = t.detach().to(torch.float32).contiguous()
        if t.numel() != c * c:
            raise HipOpError(f"{name} must be [{c}, {c}, 1, 1], got {tuple(t.shape)}")
        w.append(t)
    out = torch.empty_like(content)
    nbytes = lib().ast_adaattn_workspace_bytes(dtype_code, n, c, hc, wc, hs, ws)
    ws_buf = torch.empty((nbytes,), dtype=torch.uint8, device=content.device)
    flops = 6 * n * c * (hc * wc) * (hs * ws)   # S (2C) + P[V, V^2] (4C) per score
    tag = f"adaattn{' bf16' if dtype_code else ''} {c}ch {hc}x{wc}<-{hs}x{ws}"
    check(_timed(tag, flops, content.device, lambda: lib().ast_adaattn_fwd(
        dtype_code, ptr(content), ptr(style), ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(out), ptr(ws_buf), nbytes,
        n, c, hc, wc, hs, ws, stream_ptr(content.device))), "adaattn")
    return out


def emd_rows(hx: torch.Tensor, hy: torch.Tensor):
    """EarthMoversDistanceLoss.forward (losses.py:11-22) on [B, 256] histograms: [B] values."""
    hx, hy = _dev(hx, "x"), _dev(hy, "y")
    if hx.dim() != 2 or hx.shape != hy.shape or hx.shape[1] != 256:
        raise HipOpError(f"earth movers: expected two [B, 256] tensors, got {tuple(hx.shape)} / {tuple(hy.shape)}")
    b = hx.shape[0]
    acc_n = int(lib().ast_loss_acc_floats())
    accs = torch.zeros((b, acc_n), device=hx.device, dtype=torch.float32)   # one loss accumulator per row
    for i in range(b):   # one scalar per row: the kernel accumulates weight/n * row sums
        check(lib().ast_emd_loss_f32(ptr(hx[i:i + 1]), ptr(hy[i:i + 1]), 1, 1.0, None, ptr(accs[i]), None,
                                     stream_ptr(hx.device)), "emd")
    return accs[:, 0]
