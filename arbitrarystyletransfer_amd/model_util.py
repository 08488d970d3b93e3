"""Drop-in for the reference model_util.py.

channel_stats (model_util.py:3-8) runs on the HIP channel-statistics kernel. The colour helpers
rgb2xyz, xyz2rgb, xyz2lab, lab2xyz, rgb2lab, lab2rgb (model_util.py:11-140) run on the HIP
colour kernels (csrc/color.hip): [N, 3, H, W] images, fp32 or bf16, on a HIP device; the result
is fp32, as the reference returns for either input. They keep the reference's constants and its
NaN set (rgb below -0.055, negative xyz components) and are differentiable: the backward is the
HIP vector-Jacobian product, finite where the reference's autograd is NaN through its unselected
branch ("Colour-space kernels"). Under torch.compile they route to
torch.ops.ast_hip.color_convert. There is no CPU implementation.
"""
import torch

from . import functional
from .ops import COLOR_MODES

ab_norm = 110   # model_util.py:61-63
l_norm = 100
l_cent = 50


def channel_stats(img):
    """Per-(n,c) spatial mean and unbiased std (no eps), keepdim: model_util.py:3-8."""
    return functional.channel_stats(img, unbiased=True, eps=0.0)


def _convert(x, mode):
    if torch.compiler.is_compiling():   # the registered op (fake impl + autograd), no graph break
        from . import library  # noqa: F401  (registers the ast_hip::* custom ops)
        return torch.ops.ast_hip.color_convert(x, COLOR_MODES[mode], False)
    return functional.color_convert(x, mode)


def rgb2xyz(rgb):
    """model_util.py:13-35: sRGB in [0, 1] -> XYZ. NaN for a pixel with a channel below -0.055."""
    return _convert(rgb, "rgb2xyz")


def xyz2rgb(xyz):
    """model_util.py:38-59: XYZ -> sRGB, negative linear values clamped to 0."""
    return _convert(xyz, "xyz2rgb")


def xyz2lab(xyz):
    """model_util.py:65-88: XYZ -> L, a, b (white point 0.95047, 1, 1.08883)."""
    return _convert(xyz, "xyz2lab")


def lab2xyz(lab):
    """model_util.py:90-115: L, a, b -> XYZ, z clamped at 0."""
    return _convert(lab, "lab2xyz")


def rgb2lab(rgb):
    """model_util.py:117-128: (xyz2lab(rgb2xyz(rgb)) / 100 + 1) / 2, one launch."""
    return _convert(rgb, "rgb2lab")


def lab2rgb(lab_rs):
    """model_util.py:130-140: xyz2rgb(lab2xyz((lab_rs * 2 - 1) * 100)), one launch."""
    return _convert(lab_rs, "lab2rgb")
