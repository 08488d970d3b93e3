"""Float64 statement of the bilinear resize and the STROTSS Laplacian pyramid (csrc/pyramid.hip), and
the error bars of the fp32 kernels against it.

The oracle is torch.nn.functional.interpolate(mode="bilinear", align_corners=False,
antialias=False) itself, in float64 on the CPU (`interp`, `build`, `collapse`, `adjoint`).
`resize_ref` restates the kernel's definition -- the same filter with the source coordinate
computed in fp32, as PyTorch's fp32 kernels and csrc/pyramid.hip do -- in float64 arithmetic, so
that the kernel can also be held to its arithmetic rounding alone.

Bars (EPS = 2^-24, the unit roundoff of fp32; none comes from the code under test):

coordinate   s = fma(scale, o + 0.5, -0.5) with scale = fl(in / out): scale carries one rounding
             and the fma one more, so |s - s_exact| <= (2 s + 0.5) EPS <= in * 2 EPS (`coord_err`).
resize       Bilinear interpolation is continuous and piecewise linear in s: moving s by d moves
             the value by at most d * D, D the largest difference of adjacent source pixels along
             that axis -- also across a cell boundary, where a different index changes the value
             only by that much. So |fp32 - float64| <= Dy coord_err(h) + Dx coord_err(w) plus the
             arithmetic: 1 - l (2 roundings), 6 products, 3 sums of values <= max|x|, bounded by
             11 EPS max|x|; with `add`, two more roundings of |add| + |resize|.
adjoint      dx[s] = sum over touching outputs of wy wx g. The outputs with a non-zero weight on a
             source index have s within one cell of it, an interval of 2 out / in outputs: at most
             k = min(out, 2 ceil(out / in) + 2) per axis; each weight moves by at most
             coord_err, so the weights contribute n (coord_err(h) + coord_err(w)) max|g| with
             n = ky kx; the n-term running sum and the three roundings per term contribute
             (n + 3) EPS S max|g|, S = the largest sum of weights onto one source pixel (the
             float64 adjoint of ones).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24

# (h, w) -> (H, W) of the GPU tests
CASES = [((1, 1), (1, 1)), ((1, 3), (2, 7)), ((18, 25), (37, 50)), ((37, 50), (18, 25)), ((5, 4), (16, 16)),
         ((64, 64), (23, 41))]
BIG = ((512, 512), (256, 256))


def _planes(x):
    return x.reshape((1, -1) + tuple(x.shape[-2:]))


def interp(x, size):
    """The oracle: F.interpolate on the planes of x [..., h, w] (float64)."""
    size = (int(size[0]), int(size[1]))
    y = F.interpolate(_planes(x.double()), size=size, mode="bilinear", align_corners=False, antialias=False)
    return y.reshape(tuple(x.shape[:-2]) + size)


def adjoint(g, in_size):
    """The transpose of interp from in_size, by float64 autograd."""
    x = torch.zeros(tuple(g.shape[:-2]) + (int(in_size[0]), int(in_size[1])), dtype=torch.float64, requires_grad=True)
    interp(x, g.shape[-2:]).backward(g.double())
    return x.grad


def down_size(size):
    return max(int(size[0]) // 2, 1), max(int(size[1]) // 2, 1)


def build(x, levels):
    cur, pyr = x.double(), []
    for _ in range(levels):
        small = interp(cur, down_size(cur.shape[-2:]))
        pyr.append(cur - interp(small, cur.shape[-2:]))
        cur = small
    return pyr + [cur]


def collapse(pyr):
    cur = pyr[-1].double()
    for lvl in reversed(pyr[:-1]):
        cur = lvl.double() + interp(cur, lvl.shape[-2:])
    return cur


# ---- the kernel's definition: fp32 coordinates, float64 arithmetic ---------------------------------

def src_map(out, inn):
    """(i0, i1, l1) for every output index: s = fma(fl(in / out), o + 0.5, -0.5) in fp32."""
    scale = np.float32(inn) / np.float32(out)
    o = np.arange(out, dtype=np.float64)
    s = (np.float64(scale) * (o + 0.5) - 0.5).astype(np.float32)   # exact in float64, one rounding: the fma
    s = np.maximum(s, np.float32(0))
    i0 = np.minimum(s.astype(np.int64), inn - 1)
    i1 = np.minimum(i0 + 1, inn - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float64)
    return i0, i1, l1


def resize_ref(x, size):
    """resize with the kernel's fp32 source coordinates, differentiable, float64."""
    x = x.double()
    h, w = x.shape[-2:]
    y0, y1, ly = src_map(int(size[0]), h)
    x0, x1, lx = src_map(int(size[1]), w)
    y0, y1, x0, x1 = (torch.from_numpy(i) for i in (y0, y1, x0, x1))
    ly, lx = torch.from_numpy(ly)[:, None], torch.from_numpy(lx)
    top, bot = x[..., y0, :], x[..., y1, :]
    return ((1 - ly) * ((1 - lx) * top[..., x0] + lx * top[..., x1])
            + ly * ((1 - lx) * bot[..., x0] + lx * bot[..., x1]))


def adjoint_ref(g, in_size):
    x = torch.zeros(tuple(g.shape[:-2]) + (int(in_size[0]), int(in_size[1])), dtype=torch.float64, requires_grad=True)
    resize_ref(x, g.shape[-2:]).backward(g.double())
    return x.grad


def touch_range(s, inn, out, fused):
    """The adjoint kernel's candidate outputs [lo, hi] of source index s, in fp32 as it computes
    them (`fused`: with the multiply-subtract contracted into one fma, which the compiler may do)."""
    inv = np.float32(out) / np.float32(inn)
    s = np.asarray(s, dtype=np.float32)

    def end(c):
        a = s + np.float32(c)
        if fused:
            return (np.float64(inv) * a.astype(np.float64) - 0.5).astype(np.float32)
        return (a * inv).astype(np.float32) - np.float32(0.5)
    lo = np.floor(end(-0.5)).astype(np.int64) - 1
    hi = np.ceil(end(1.5)).astype(np.int64) + 1
    return np.maximum(lo, 0), np.minimum(hi, out - 1)


# ---- bars -------------------------------------------------------------------------------------------

def coord_err(inn):
    return inn * 2 * EPS


def _adjacent(x, dim):
    return float((x.narrow(dim, 1, x.shape[dim] - 1) - x.narrow(dim, 0, x.shape[dim] - 1)).abs().max()) \
        if x.shape[dim] > 1 else 0.0


def arith_bar(xmax, addmax=None):
    return 11 * EPS * xmax + (2 * EPS * (addmax + xmax) if addmax is not None else 0.0)


def resize_bar(x, addmax=None):
    """|fp32 kernel - interp| for source x (float64 tensor [..., h, w])."""
    x = x.double()
    h, w = x.shape[-2:]
    return _adjacent(x, -2) * coord_err(h) + _adjacent(x, -1) * coord_err(w) + arith_bar(float(x.abs().max()), addmax)


def touch_count(out, inn):
    return min(out, 2 * math.ceil(out / inn) + 2)


def weight_sum(in_size, out_size):
    """S: the largest sum of weights onto one source pixel."""
    return float(adjoint(torch.ones((int(out_size[0]), int(out_size[1])), dtype=torch.float64), in_size).max())


def adjoint_arith_bar(gmax, in_size, out_size):
    n = touch_count(out_size[0], in_size[0]) * touch_count(out_size[1], in_size[1])
    return gmax * (n + 3) * EPS * weight_sum(in_size, out_size)


def adjoint_bar(gmax, in_size, out_size):
    n = touch_count(out_size[0], in_size[0]) * touch_count(out_size[1], in_size[1])
    return gmax * n * (coord_err(in_size[0]) + coord_err(in_size[1])) + adjoint_arith_bar(gmax, in_size, out_size)


def build_bars(x, levels):
    """Per entry of build(x, levels): |fp32 kernels - float64|. The resize averages (gain <= 1), so
    an error of its input passes through unamplified: e(cur_{l+1}) <= e(cur_l) + bar(down),
    e(lap_l) <= e(cur_l) + e(cur_{l+1}) + bar(up with add)."""
    cur, e_cur, bars = x.double(), 0.0, []
    for _ in range(levels):
        small = interp(cur, down_size(cur.shape[-2:]))
        e_small = e_cur + resize_bar(cur)
        bars.append(e_cur + e_small + resize_bar(small, addmax=float(cur.abs().max())))
        cur, e_cur = small, e_small
    return bars + [e_cur]


def collapse_bar(pyr):
    """|fp32 kernels - float64| of collapse(pyr): every level adds its own resize-with-add bar to the
    error it inherits (gain <= 1)."""
    cur, err = pyr[-1].double(), 0.0
    for lvl in reversed(pyr[:-1]):
        err += resize_bar(cur, addmax=float(lvl.abs().max()))
        cur = lvl.double() + interp(cur, lvl.shape[-2:])
    return err


def collapse_grad_bars(sizes, g):
    """Per level: |fp32 adjoint chain - float64| for the gradient g of the collapsed image; level
    l + 1 inherits level l's error times the adjoint's gain S_l and adds its own adjoint bar."""
    g = g.double()
    bars, err = [0.0], 0.0
    for fine, coarse in zip(sizes[:-1], sizes[1:]):
        err = err * weight_sum(coarse, fine) + adjoint_bar(float(g.abs().max()), coarse, fine)
        g = adjoint(g, coarse)
        bars.append(err)
    return bars


def image(seed, shape):
    """A smooth-plus-noise fp32 test image in [0, 1] (fixed seed)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen, dtype=torch.float32)
