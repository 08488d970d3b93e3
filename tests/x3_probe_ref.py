"""Single-product probe of the split-bf16 ("x3") kernels: helpers, pure torch on the CPU.

csrc/x3.h carries an fp32 value as three bf16 terms x = hi + mid + lo and a product as the six
largest of the nine term products. Dense random inputs under rel_inf = max|a-b| / max|b| cannot
tell that from a kernel that lost a term. Here every output is ONE product (or a
handful), so summation cannot hide anything, and the error is counted in ulp of the product.

CPU emulation (tests/test_x3_probe_cpu.py pins the properties used below):
  * the six-term sum of one product, added smallest term first in fp32, is within 1.73 ulp
    (1 ulp = 2^-24 relative) of the exact product;
  * `loud` operands have |mid| >= 2^-10 |x| and |lo| >= 2^-18 |x|; with them, removing any one
    kept term moves EVERY product by at least 19.9 ulp.

Bars of check_products (ulp of A = the sum of the absolute products of an output):
  * BAR_ONE = 4 where an output is a single product: the emulated 1.73 with a margin of about
    2.3x for the order and internal rounding of the MFMA's own accumulation;
  * BAR_SUM = 8 where it is a sum of m > 1 products: 1.73 ulp of A from the products plus
    (m - 1) fp32 additions of at most half an ulp of A each. Reflection of an upsampled map puts
    up to nine products of one source pixel into a corner output (all nine taps land on it), so
    M_MAX = 9 and the budget is 1.73 + 8 * 0.5 = 5.73 <= 8; check_products refuses an m above it.
Neither bar may rise above 8 (12 for m > 1): a missing mid*mid term is 19.9 ulp.
"""
import math

import torch
import torch.nn.functional as F

ULP = 2.0 ** -24
BAR_ONE = 4.0
BAR_SUM = 8.0
M_MAX = 9
F32_MAX = 3.402823466e38
BF16_MAX = 3.38953139e38

HI, MID, LO = 0, 1, 2
# the six kept term products (term of a, term of b), smallest first: the order they are added in
SIX = ((MID, MID), (LO, HI), (HI, LO), (MID, HI), (HI, MID), (HI, HI))
TWO = ((MID, MID), (MID, HI), (HI, MID), (HI, HI))   # the terms a two-term split (no lo) has


def broken_variants():
    """name -> term list of every broken form the probe must catch: each kept term but hi*hi
    missing, and lo*hi staged twice in place of hi*lo."""
    out = {}
    for t in SIX[:-1]:
        out[f"no_{'hml'[t[0]]}{'hml'[t[1]]}"] = tuple(u for u in SIX if u != t)
    out["lohi_twice"] = tuple((LO, HI) if u == (HI, LO) else u for u in SIX)
    return out


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split3(x):
    """csrc/x3.h split3 on an fp32 tensor: (hi, mid, lo) as fp32 tensors of bf16 values. A finite
    value whose hi would round to inf has hi clamped to bf16's largest value (the remainder stays
    exact); a non-finite value has hi = x and mid = lo = 0."""
    x = x.to(torch.float32)
    finite = x.abs() <= F32_MAX
    hi = _bf16(x)
    over = finite & ~(hi.abs() <= F32_MAX)
    hi = torch.where(over, torch.copysign(torch.full_like(x, BF16_MAX), x), hi)
    r = torch.where(finite, x - hi, torch.zeros_like(x))
    mid = _bf16(r)
    lo = _bf16(r - mid)
    return hi, mid, lo


def split2(x):
    """The two-term split a kernel with no lo plane computes: (hi, mid, 0)."""
    hi, mid, _ = split3(x)
    return hi, mid, torch.zeros_like(hi)


def is_loud(x):
    hi, mid, lo = split3(x)
    ax = x.abs()
    return (mid.abs() >= 2.0 ** -10 * ax) & (lo.abs() >= 2.0 ** -18 * ax) & (ax >= 0.5) & (ax < 1.5)


def loud(seed, shape):
    """Seeded fp32 values in +-[0.5, 1.5) whose split has |mid| >= 2^-10 |x| and |lo| >= 2^-18 |x|
    (rejection: about 16 % of uniform draws qualify)."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    n = math.prod(shape)
    g = torch.Generator().manual_seed(int(seed))
    got, have = [], 0
    while have < n:
        k = max(1024, 8 * (n - have))
        mag = (torch.rand(k, generator=g, dtype=torch.float64) + 0.5).to(torch.float32)
        sgn = torch.randint(0, 2, (k,), generator=g).to(torch.float32) * 2 - 1
        x = mag * sgn
        x = x[is_loud(x)]
        got.append(x)
        have += x.numel()
    return torch.cat(got)[:n].reshape(shape).contiguous()


def grid_sparse(shape, phase, seed=0):
    """NCHW, zero except at pixels with y % 3 == phase[0] and x % 3 == phase[1]; at each of those
    exactly one channel is non-zero (a `loud` value), cycling through all channels over successive
    grid pixels. A 3x3 window sees at most one non-zero pixel."""
    n, c, h, w = (int(s) for s in shape)
    out = torch.zeros(n, c, h, w)
    ys = torch.arange(phase[0], h, 3)
    xs = torch.arange(phase[1], w, 3)
    if ys.numel() == 0 or xs.numel() == 0:
        return out
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    k = yy.numel()
    vals = loud(seed, (n, k))
    for b in range(n):
        ch = (torch.arange(k) + b * k) % c
        out[b, ch, yy, xx] = vals[b]
    return out


def one_pixel_per_plane(shape, positions, seed=0, per_image=False):
    """[n, c, h, w] with one non-zero (`loud`) pixel per channel: channel ch carries it at
    positions[ch % len(positions)], in image ch % n alone (per_image: in every image)."""
    n, c, h, w = (int(s) for s in shape)
    out = torch.zeros(n, c, h, w)
    vals = loud(seed, (n, c))
    for ch in range(c):
        y, x = positions[ch % len(positions)]
        assert 0 <= y < h and 0 <= x < w, (y, x, h, w)
        for b in (range(n) if per_image else (ch % n,)):
            out[b, ch, y, x] = vals[b, ch]
    return out


def one_column(n, c, hw, k0s, seed=0):
    """[n, c, hw] features for the Gram, zero except column k0s[b] of image b (`loud` values)."""
    assert len(k0s) == n
    out = torch.zeros(n, c, hw)
    vals = loud(seed, (n, c))
    for b, k0 in enumerate(k0s):
        assert 0 <= k0 < hw
        out[b, :, k0] = vals[b]
    return out


def ulps(got, ref64, A):
    """|got - ref64| in ulp of A, elementwise (0 where A == 0)."""
    d = (got.detach().cpu().double() - ref64).abs()
    return torch.where(A > 0, d / (ULP * A.clamp_min(1e-300)), torch.zeros_like(d))


def check_products(got, ref64, A, m, bar_one=BAR_ONE, bar_sum=BAR_SUM, what=""):
    """got against the float64 result ref64. A: the same op on |inputs| in float64 (the sum of the
    absolute products per output); m: the number of non-zero products per output (the same op on
    indicators). Elementwise |got - ref64| <= bar * 2^-24 * A with bar_one where m == 1 and bar_sum
    where m > 1, and got == 0 exactly where m == 0. Returns (largest ulp where m == 1, where m > 1)."""
    assert bar_one <= 8 and bar_sum <= 12, "a bar above its cap starts hiding the mid*mid term"
    g = got.detach().cpu().double()
    m = m.round()
    assert g.shape == ref64.shape == A.shape == m.shape, (g.shape, ref64.shape, A.shape, m.shape)
    assert float(m.max()) <= M_MAX, f"{what}: {float(m.max())} products in one output, the bars cover {M_MAX}"
    zero = m == 0
    assert bool((g[zero] == 0).all()), f"{what}: {int((g[zero] != 0).sum())} outputs with no product are not 0"
    u = ulps(g, ref64, A)
    u = torch.where(torch.isfinite(g), u, torch.full_like(u, float("inf")))
    one, many = m == 1, m > 1
    worst = []
    for sel, bar, name in ((one, bar_one, "single products"), (many, bar_sum, "sums of products")):
        if not bool(sel.any()):
            worst.append(0.0)
            continue
        us = torch.where(sel, u, torch.zeros_like(u))
        top = float(us.max())
        if not top <= bar:
            idx = tuple(int(i) for i in torch.unravel_index(us.argmax(), us.shape))
            raise AssertionError(f"{what}: {name}: {int((us > bar).sum())} of {int(sel.sum())} outputs over "
                                 f"{bar} ulp; worst {top:.2f} ulp at {idx}: got {float(g[idx])!r}, "
                                 f"float64 {float(ref64[idx])!r}, m {int(m[idx])}")
        worst.append(top)
    return tuple(worst)


# ------------------------------------------------------------------------------------------------
# float64 references of the probed ops (bilinear in their two operands)
# ------------------------------------------------------------------------------------------------

def conv64(x, w, up=1, pad="zeros"):
    """[upsample x2] -> pad(1) -> conv3x3 in float64, no bias."""
    x, w = x.double(), w.double()
    if up == 2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if pad == "reflect":
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w)
    return F.conv2d(x, w, padding=1)


def conv_ref(x, w, up=1, pad="zeros"):
    """(ref64, A, m) of the forward conv."""
    return (conv64(x, w, up, pad), conv64(x.abs(), w.abs(), up, pad),
            conv64((x != 0).double(), (w != 0).double(), up, pad))


def dgrad64(dy, w, in_hw, up=1, pad="zeros"):
    """dL/dx of conv64 given dL/dy (float64 autograd)."""
    cin = w.shape[1]
    x = torch.zeros(dy.shape[0], cin, *in_hw, dtype=torch.float64, requires_grad=True)
    y = conv64(x, w, up, pad)
    return torch.autograd.grad(y, x, dy.double())[0]


def dgrad_ref(dy, w, in_hw, up=1, pad="zeros"):
    return (dgrad64(dy, w, in_hw, up, pad), dgrad64(dy.abs(), w.abs(), in_hw, up, pad),
            dgrad64((dy != 0).double(), (w != 0).double(), in_hw, up, pad))


def wgrad64(x, dy, up=1, pad="zeros"):
    """(dW, db) of conv64 + bias given dL/dy (float64 autograd)."""
    cout, cin = dy.shape[1], x.shape[1]
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = conv64(x, w, up, pad)
    return torch.autograd.grad(y, w, dy.double())[0], dy.double().sum(dim=(0, 2, 3))


def wgrad_ref(x, dy, up=1, pad="zeros"):
    """((dW64, A, m), (db64, A, m))."""
    r = wgrad64(x, dy, up, pad)
    a = wgrad64(x.abs(), dy.abs(), up, pad)
    m = wgrad64((x != 0).double(), (dy != 0).double(), up, pad)
    return (r[0], a[0], m[0]), (r[1], a[1], m[1])


def gram64(f):
    """bmm(F, F^T) / (C * HW) of [n, c, hw] features in float64."""
    f = f.double()
    return torch.bmm(f, f.transpose(1, 2)) / (f.shape[1] * f.shape[2])


def gram_ref(f):
    fa, fi = f.double().abs(), (f != 0).double()
    return gram64(f), gram64(fa), torch.bmm(fi, fi.transpose(1, 2))


# ------------------------------------------------------------------------------------------------
# the kernels' arithmetic, emulated: term planes through a float64 op, summed in fp32
# ------------------------------------------------------------------------------------------------

def emulate(op, a, b, terms=SIX, split=split3):
    """op(a, b) as a split-bf16 kernel forms it: op is bilinear and runs in float64 on one term
    plane of each operand per kept term product (exact where an output is one product); the term
    results are rounded to fp32 and added in fp32 in the order of `terms`."""
    pa, pb = split(a), split(b)
    acc = None
    for ta, tb in terms:
        t = op(pa[ta].double(), pb[tb].double()).to(torch.float32)
        acc = t if acc is None else acc + t
    return acc
