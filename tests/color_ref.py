"""Float64 restatement of the six colour conversions of model_util.py:11-140 and of their
vector-Jacobian products, on the CPU, for shapes too large to keep as fixtures.

Each map is a constant 3x3 mix and a piecewise scalar function, written here with torch.where on
the selected branch. Where the reference's `f*mask + g*(1-mask)` blend lets a NaN of the unselected
branch through (a channel below -0.055 in rgb2xyz, a negative component in xyz2lab), the same
elements are NaN here. The white point is the float32 rounding of (0.95047, 1, 1.08883): the
reference builds it with torch.Tensor, so its float64 run divides by those float32 values.
test_color_cpu.py pins every function and vjp to the fixture's reference values
(tests/golden/color.npz) before the GPU tests use them as comparators.

The vjps use the derivative of the selected branch, zero where a max(., 0) clamp is active: what
autograd gives on the reference wherever its gradient is finite.
"""
from __future__ import annotations

import numpy as np
import torch

MODES = ("rgb2xyz", "xyz2rgb", "xyz2lab", "lab2xyz", "rgb2lab", "lab2rgb")

M_RGB2XYZ = torch.tensor([[0.412453, 0.357580, 0.180423],
                          [0.212671, 0.715160, 0.072169],
                          [0.019334, 0.119193, 0.950227]], dtype=torch.float64)
M_XYZ2RGB = torch.tensor([[3.24048134, -1.53715152, -0.49853633],
                          [-0.96925495, 1.87599, 0.04155593],
                          [0.05564664, -0.20404134, 1.05731107]], dtype=torch.float64)
WHITE = torch.tensor(np.array([0.95047, 1.0, 1.08883], dtype=np.float32).astype(np.float64))
T0 = 16.0 / 116.0


def _mix(m, x):
    """Per-pixel m @ x on [N, 3, H, W], in the dtype of x."""
    m = m.to(x.dtype)
    return torch.stack([m[i, 0] * x[:, 0] + m[i, 1] * x[:, 1] + m[i, 2] * x[:, 2] for i in range(3)], dim=1)


def _white(x):
    return WHITE.to(x.dtype)[None, :, None, None]


def _nan_like(x):
    return torch.full_like(x, float("nan"))


# ---- forward maps ---------------------------------------------------------------------------------

def _rgb_lin(v):
    b = (v + 0.055) / 1.055
    up = b.clamp_min(0) ** 2.4
    lo = torch.where(b < 0, _nan_like(v), v / 12.92)
    return torch.where(v > 0.04045, up, lo)


def rgb2xyz(x):
    return _mix(M_RGB2XYZ, _rgb_lin(x))


def _lab_f(s):
    up = s.clamp_min(0) ** (1 / 3.0)
    lo = torch.where(s < 0, _nan_like(s), 7.787 * s + T0)
    return torch.where(s > 0.008856, up, lo)


def xyz2lab(x):
    f = _lab_f(x / _white(x))
    return torch.stack([116.0 * f[:, 1] - 16.0, 500.0 * (f[:, 0] - f[:, 1]), 200.0 * (f[:, 1] - f[:, 2])], dim=1)


def _lab_t(x):
    ty = (x[:, 0] + 16.0) / 116.0
    tx = x[:, 1] / 500.0 + ty
    tz = ty - x[:, 2] / 200.0
    return tx, ty, tz


def _lab_finv(t):
    return torch.where(t > 0.2068966, t ** 3.0, (t - T0) / 7.787)


def lab2xyz(x):
    tx, ty, tz = _lab_t(x)
    t = torch.stack([tx, ty, tz.clamp_min(0)], dim=1)
    return _lab_finv(t) * _white(x)


def _lin_rgb(v):
    return torch.where(v > 0.0031308, 1.055 * v ** (1.0 / 2.4) - 0.055, 12.92 * v)


def xyz2rgb(x):
    return _lin_rgb(_mix(M_XYZ2RGB, x).clamp_min(0))


def rgb2lab(x):
    return (xyz2lab(rgb2xyz(x)) / 100 + 1) / 2


def lab2rgb(x):
    return xyz2rgb(lab2xyz((x * 2 - 1) * 100))


def convert(mode, x):
    return globals()[mode](x)


def luma_transfer(stylised, content):
    """lab2rgb(cat(L of rgb2lab(clamp01(stylised)), ab of rgb2lab(clamp01(content))))."""
    ls = rgb2lab(stylised.clamp(0, 1))
    lc = rgb2lab(content.clamp(0, 1))
    return lab2rgb(torch.cat([ls[:, :1], lc[:, 1:]], dim=1))


# ---- vector-Jacobian products: J(x)^T g ----------------------------------------------------------

def rgb2xyz_vjp(x, g):
    b = (x + 0.055) / 1.055
    d = torch.where(x > 0.04045, (2.4 / 1.055) * b.clamp_min(0) ** 1.4, torch.full_like(x, 1 / 12.92))
    return _mix(M_RGB2XYZ.t(), g) * d


def xyz2lab_vjp(x, g):
    w = _white(x)
    s = x / w
    d = torch.where(s > 0.008856, s.clamp_min(1e-300) ** (-2 / 3.0) / 3.0, torch.full_like(s, 7.787))
    df = torch.stack([500.0 * g[:, 1], 116.0 * g[:, 0] - 500.0 * g[:, 1] + 200.0 * g[:, 2], -200.0 * g[:, 2]], dim=1)
    return df * d / w


def lab2xyz_vjp(x, g):
    tx, ty, tz = _lab_t(x)
    t = torch.stack([tx, ty, tz], dim=1)
    d = torch.where(t > 0.2068966, 3.0 * t * t, torch.full_like(t, 1 / 7.787))
    dt = g * _white(x) * d
    dz = torch.where(tz < 0, torch.zeros_like(tz), dt[:, 2])
    return torch.stack([(dt[:, 0] + dt[:, 1] + dz) / 116.0, dt[:, 0] / 500.0, -dz / 200.0], dim=1)


def xyz2rgb_vjp(x, g):
    v = _mix(M_XYZ2RGB, x)
    d = torch.where(v > 0.0031308, (1.055 / 2.4) * v.clamp_min(1e-300) ** (1.0 / 2.4 - 1.0), torch.full_like(v, 12.92))
    d = torch.where(v < 0, torch.zeros_like(v), d)
    return _mix(M_XYZ2RGB.t(), g * d)


def rgb2lab_vjp(x, g):
    return rgb2xyz_vjp(x, xyz2lab_vjp(rgb2xyz(x), g / 200))


def lab2rgb_vjp(x, g):
    lab = (x * 2 - 1) * 100
    return lab2xyz_vjp(lab, xyz2rgb_vjp(lab2xyz(lab), g)) * 200


def vjp(mode, x, g):
    return globals()[mode + "_vjp"](x, g)


def stage_input(mode, rgb):
    """A valid input of `mode` derived from an RGB image, as the fixture does: x, rgb2xyz(x),
    xyz2lab(rgb2xyz(x)) or rgb2lab(x)."""
    if mode in ("rgb2xyz", "rgb2lab"):
        return rgb
    if mode in ("xyz2rgb", "xyz2lab"):
        return rgb2xyz(rgb)
    if mode == "lab2xyz":
        return xyz2lab(rgb2xyz(rgb))
    return rgb2lab(rgb)
