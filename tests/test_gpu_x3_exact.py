"""Ulp-level single-product tests of the split-bf16 kernels (tests/x3_probe_ref.py): every output of
the forward conv, the input gradient, the weight gradient and the Gram is one product (or a sum of a
few, where reflection / upsampling fold taps together), compared in ulp of the product with the
float64 result. Bars: 4 ulp for a single product, 8 for a sum (x3_probe_ref.py says where they come
from); a kernel that lost any one of its six term products is at least 19.9 ulp off on EVERY single
product (tests/test_x3_probe_cpu.py). Every test prints the largest ulp it saw per kernel family."""
import pytest
import torch
import torch.nn.functional as F

import x3_probe_ref as P
from arbitrarystyletransfer_amd import functional as Fn
from arbitrarystyletransfer_amd import losses as L
from arbitrarystyletransfer_amd import ops
from arbitrarystyletransfer_amd._lib import lib
from oracle import ref_cpu as R
from test_gpu_parity import CONV_CASES

pytestmark = pytest.mark.gpu

PHASES = ((0, 0), (1, 1), (2, 2))
WORST = {}   # family -> [largest ulp over single products, over sums]


def note(family, one, many):
    w = WORST.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], one), max(w[1], many)


def report(prefix):
    for fam in sorted(k for k in WORST if k.startswith(prefix)):
        print(f"x3 probe max ulp: {fam}: single products {WORST[fam][0]:.2f}, sums {WORST[fam][1]:.2f}")


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# forward conv, every configuration
# ------------------------------------------------------------------------------------------------

FWD_CASES = CONV_CASES + [
    (2, 64, 16, 32, 64, 1, "zeros", False),    # four K chunks of the M16 tiles
    (1, 128, 8, 32, 128, 1, "zeros", False),   # eight K chunks, two channel groups
]


def conv_family(cfg):
    if cfg < 0:
        return "conv fwd: library's choice"
    if cfg in (10, 11, 36, 37):
        return "conv fwd: direct VALU, cout <= 4 (fp32)"
    if 18 <= cfg <= 23:
        return "conv fwd: direct VALU, cin <= 4 (fp32)"
    if 24 <= cfg <= 31:
        return "conv fwd: split-bf16 conv_x3 (24-31)"
    if 32 <= cfg <= 35:
        return "conv fwd: split-bf16 conv_x3 persistent (32-35)"
    if 38 <= cfg <= 41:
        return "conv fwd: split-bf16 conv_x3 block loop (38-41)"
    if cfg in (42, 43):
        return "conv fwd: split-bf16 conv_cin3 (42-43)"
    return "conv fwd: fp32 MFMA igemm (0-9, 12-17)"


def run_conv(xd, wp, cout, up, pad, mean, std, cfg):
    """(pre, act, pool) of one configuration; pool None where the configuration has no pooled output;
    None where it does not take this shape at all."""
    for pool in (True, False):
        try:
            out = ops.conv3x3(xd, wp, None, cout, upsample=up, pad_mode=pad, in_mean=mean, in_std=std,
                              want_pre=True, want_act=True, want_pool=pool, cfg=cfg)
        except Exception as e:  # configurations that do not support this shape are rejected on the host
            assert "unsupported" in str(e), e
            continue
        torch.cuda.synchronize()
        return out
    return None


def check_conv_outputs(out, ref, bar_one, what):
    pre, act, pool = out
    one, many = P.check_products(pre, *ref, bar_one=bar_one, what=what)
    assert torch.equal(bits(act), bits(torch.relu(pre))), what
    if pool is not None:
        assert torch.equal(bits(pool), bits(F.max_pool2d(act, 2, 2))), what
    return one, many


@pytest.mark.parametrize("case", FWD_CASES)
def test_conv3x3_single_products_all_configs(case, hip_device):
    n, cin, h, w, cout, up, pad, norm = case
    wt = P.loud(200 + cin, (cout, cin, 3, 3))
    wp = ops.pack_conv3x3(wt.to(hip_device))
    runs = []   # (x on the device, mean, std, (ref64, A, m), bar for single products, label)
    for ph in PHASES:
        x = P.grid_sparse((n, cin, h, w), ph, seed=100 + cin + ph[0])
        runs.append((x.to(hip_device), None, None, P.conv_ref(x, wt, up, pad), P.BAR_ONE, f"phase {ph}"))
        if norm:
            # background = mean[c], which normalises to exactly 0; the kernel's own rounding of
            # (x - mean) / std adds about 1 ulp, so the whole run is held to the bar for sums
            mean, std = torch.tensor(R.IMNET_MEAN), torch.tensor(R.IMNET_STD)
            xb = torch.where(x != 0, x, mean.view(1, -1, 1, 1).expand_as(x)).contiguous()
            xn = (xb.double() - mean.double().view(1, -1, 1, 1)) / std.double().view(1, -1, 1, 1)
            assert torch.equal(xn != 0, x != 0)
            runs.append((xb.to(hip_device), mean.to(hip_device), std.to(hip_device), P.conv_ref(xn, wt, up, pad),
                         P.BAR_SUM, f"phase {ph} normalised"))
    tried = 0
    for cfg in range(-1, lib().ast_conv3x3_num_configs()):
        ran = False
        for xd, mean, std, ref, bar_one, label in runs:
            out = run_conv(xd, wp, cout, up, pad, mean, std, cfg)
            if out is None:
                continue
            ran = True
            fam = conv_family(cfg) + (", normalised input" if mean is not None else "")
            note(fam, *check_conv_outputs(out, ref, bar_one, f"cfg {cfg} {label}"))
        tried += ran and cfg >= 0
    assert tried >= 1
    report("conv fwd")


# n, cin, h, w, cout: the collapsed kernel of the upsampled reflect-pad conv, both tile forms
UP2C_CASES = [(1, 32, 8, 16, 64), (2, 16, 5, 12, 128)]


@pytest.mark.parametrize("tile", [8, 4])
@pytest.mark.parametrize("case", UP2C_CASES)
def test_conv3x3_up2c_single_products(case, tile, hip_device):
    n, cin, h, w, cout = case
    wt = P.loud(230 + cin, (cout, cin, 3, 3))
    ext = ops.pack_conv3x3(wt.to(hip_device), up2c=True)
    for ph in PHASES:
        x = P.grid_sparse((n, cin, h, w), ph, seed=130 + cin + ph[0])
        pre, act, _ = ops.conv3x3(x.to(hip_device), ext, None, cout, upsample=2, pad_mode="reflect", want_pre=True,
                                  want_act=True, _up2c_tile=tile)
        torch.cuda.synchronize()
        note(f"conv fwd up2c: conv_up2c, {tile}-wave tile",
             *check_conv_outputs((pre, act, None), P.conv_ref(x, wt, 2, "reflect"), P.BAR_ONE, f"tile {tile} phase {ph}"))
    report("conv fwd up2c")


# ------------------------------------------------------------------------------------------------
# input gradient
# ------------------------------------------------------------------------------------------------

# n, cin -> cout of the forward conv, h x w of its input (dy: n x cout x up*h x up*w)
DGRAD_CASES = [(2, 64, 24, 12, 16), (1, 128, 64, 8, 32), (2, 64, 3, 9, 20)]
DGRAD_MODES = [(1, "zeros"), (1, "reflect"), (2, "reflect")]   # reflect: the border fold; up 2: the 2x2 sum


@pytest.mark.parametrize("up,pad", DGRAD_MODES)
@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv_input_grad_single_products(case, up, pad, hip_device):
    n, cin, cout, h, w = case
    wt = P.loud(300 + cin, (cout, cin, 3, 3))
    wd = wt.to(hip_device)
    ones = torch.ones(n, cin, h, w, device=hip_device)
    for ph in PHASES:
        dy = P.grid_sparse((n, cout, h * up, w * up), ph, seed=310 + cout + ph[0])
        ref = P.dgrad_ref(dy, wt, (h, w), up, pad)
        plain = Fn.conv_input_grad(dy.to(hip_device), wd, up, pad)
        masked = Fn.conv_input_grad(dy.to(hip_device), wd, up, pad, mask=ones)
        torch.cuda.synchronize()
        for got, label in ((plain, "no mask"), (masked, "mask of ones")):
            note(f"dgrad up{up} {pad}", *P.check_products(got, *ref, what=f"dgrad {case} up{up} {pad} {ph} {label}"))
    report("dgrad")


# ------------------------------------------------------------------------------------------------
# weight gradient, every family of ast_conv3x3_wgrad_ex_f32 (the dispatcher in csrc/conv3x3_bwd.hip)
# ------------------------------------------------------------------------------------------------

WGRAD_CASES = [
    # family, n, cin, h, w, cout, up
    ("wgrad3", 2, 64, 8, 32, 64, 1),
    ("wgrad3", 1, 64, 4, 16, 64, 2),
    ("wgrad_kernel", 2, 24, 13, 9, 40, 1),
    ("wgrad_kernel", 1, 8, 5, 7, 128, 2),
    ("wgrad_smallco<3,4>", 2, 16, 9, 37, 3, 2),
    ("wgrad_smallco<4,4>", 1, 5, 7, 9, 4, 1),
    ("wgrad_smallco<16,1>", 2, 3, 12, 20, 16, 1),
    ("wgrad_co3", 2, 64, 24, 48, 3, 1),
    ("wgrad_co3", 1, 40, 18, 32, 3, 2),
    ("wgrad_co3", 1, 130, 9, 32, 1, 1),
    ("wgrad_co3", 2, 64, 10, 16, 2, 1),
]


def pixel_positions(H, W):
    """The four corners, column 0 and column W - 1 (the border-column kernel of wgrad_co3), the first and
    last row, a pixel of the last (ragged) tile, and the interior."""
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 0), (H // 2 - 1, W - 1), (0, W // 2),
           (H - 1, W // 3), (H - 2, W - 3), (H // 2, W // 2), (1, 1)]
    assert len(set(pos)) == len(pos), pos
    return pos


def strided_dy(dy):
    """dy as a view into a larger buffer whose padding is NaN: (flat buffer, dy_layout)."""
    n, c, H, W = dy.shape
    pitch = W + 5
    plane = (H + 3) * pitch
    buf = torch.full((n * c, H + 3, pitch), float("nan"), device=dy.device)
    buf[:, 2:2 + H, 3:3 + W] = dy.reshape(n * c, H, W)
    return buf.reshape(-1), (pitch, plane, 2 * pitch + 3)


def run_wgrad(x, dy, cout, up, pad, dev):
    """dW, db from a dense dy and from the strided view of it: bit-identical, returned once."""
    xd, dyd = x.to(dev), dy.to(dev)
    assert xd.data_ptr() % 16 == 0
    dw, db = Fn.conv_weight_grad(xd, dyd, cout, up, pad)
    buf, layout = strided_dy(dyd)
    dw2, db2 = Fn.conv_weight_grad(xd, buf, cout, up, pad, dy_layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(bits(dw), bits(dw2)), "dW differs between the dense and the strided dy"
    assert torch.equal(bits(db), bits(db2)), "db differs between the dense and the strided dy"
    return dw, db


def rotations(positions, channels):
    """Position lists, rotated so that `channels` planes together visit every position."""
    return [positions[r:] + positions[:r] for r in range(0, len(positions), max(1, min(channels, len(positions))))]


@pytest.mark.parametrize("pad", ["reflect", "zeros"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_conv_wgrad_single_products(case, pad, hip_device):
    fam, n, cin, h, w, cout, up = case
    H, W = h * up, w * up
    fam = f"wgrad: {fam} up{up}"
    # dy = one pixel per output channel, x dense: dW[co, ci, tap] = dy[co, p] * xpad[ci, p + tap], db[co] = dy[co, p]
    x = P.loud(400 + cin, (n, cin, h, w))
    for r, pos in enumerate(rotations(pixel_positions(H, W), cout)):
        dy = P.one_pixel_per_plane((n, cout, H, W), pos, seed=410 + r)
        (rw, rb) = P.wgrad_ref(x, dy, up, pad)
        assert float(rb[2].max()) == 1
        dw, db = run_wgrad(x, dy, cout, up, pad, hip_device)
        note(fam, *P.check_products(dw, *rw, what=f"{case} {pad} sparse dy, rotation {r}: dW"))
        note(fam, *P.check_products(db, *rb, what=f"{case} {pad} sparse dy, rotation {r}: db"))
    # x = one pixel per input channel, dy dense (db is a dense sum then: outside the probe)
    dy = P.loud(420 + cout, (n, cout, H, W))
    for r, pos in enumerate(rotations(pixel_positions(h, w), cin)):
        xs = P.one_pixel_per_plane((n, cin, h, w), pos, seed=430 + r)
        (rw, _) = P.wgrad_ref(xs, dy, up, pad)
        dw, db = run_wgrad(xs, dy, cout, up, pad, hip_device)
        note(fam, *P.check_products(dw, *rw, what=f"{case} {pad} sparse x, rotation {r}: dW"))
        assert bool(torch.isfinite(db).all())
    report(fam)


# ------------------------------------------------------------------------------------------------
# Gram
# ------------------------------------------------------------------------------------------------

GRAM_CASES = [(3, 64, 8, 8), (2, 96, 9, 11), (1, 512, 4, 8), (4, 128, 5, 24)]   # (2, 96, 9, 11): K % 4 != 0


def gram_columns(hw):
    """Column 0, hw - 1, columns that are no multiple of 4, and both sides of the K boundaries of
    gram_x3_kernel's plan: at these sizes the plan is one split, inside which the four waves take
    interleaved 16-column steps and a wave's next step lies 64 columns on."""
    return [k for k in (0, hw - 1, 13, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 98) if k < hw]


def gram_bars(c, hw):
    """(bar for single products, label): the scale 1 / (c * hw) is exact where c * hw is a power of two;
    elsewhere it is one more rounding, held to the bar for sums."""
    pow2 = (c * hw) & (c * hw - 1) == 0
    return (P.BAR_ONE, "scale exact") if pow2 else (P.BAR_SUM, "scale rounded")


@pytest.mark.parametrize("shape", GRAM_CASES)
def test_gram_single_products(shape, hip_device):
    n, c, h, w = shape
    hw = h * w
    cols = gram_columns(hw)
    for r in range(0, len(cols), n):
        k0s = [cols[(r + b) % len(cols)] for b in range(n)]
        f = P.one_column(n, c, hw, k0s, seed=500 + r)
        got = L.gram_matrix(f.view(n, c, h, w).to(hip_device))
        torch.cuda.synchronize()
        bar, label = gram_bars(c, hw)
        note(f"gram: gram_x3_kernel, {label}",
             *P.check_products(got, *P.gram_ref(f), bar_one=bar, what=f"gram {shape} columns {k0s}"))
    report("gram: gram_x3")


@pytest.mark.parametrize("shape", GRAM_CASES)
def test_gram_backward_single_products(shape, hip_device):
    """dG with one non-zero entry (i0, j0), i0 != j0, per image: rows i0 and j0 of dF are single products
    scale * dG[i0, j0] * F[j0, :] and scale * dG[i0, j0] * F[i0, :], every other row is 0."""
    n, c, h, w = shape
    hw = h * w
    f = P.loud(520 + c, (n, c, hw))
    dg = torch.zeros(n, c, c)
    vals = P.loud(521, (n,))
    for b in range(n):
        dg[b, 3 + b, c - 5 - b] = vals[b]
    s = 1.0 / (c * hw)
    sym = dg.double() + dg.double().transpose(1, 2)
    ref = s * torch.bmm(sym, f.double())
    A = s * torch.bmm(sym.abs(), f.double().abs())
    m = torch.bmm((sym != 0).double(), (f != 0).double())
    fd = f.view(n, c, h, w).to(hip_device).requires_grad_(True)
    L.gram_matrix(fd).backward(dg.to(hip_device))
    torch.cuda.synchronize()
    bar, label = gram_bars(c, hw)
    note(f"gram: gram_bwd_kernel (fp32), {label}",
         *P.check_products(fd.grad.view(n, c, hw), ref, A, m, bar_one=bar, what=f"gram backward {shape}"))
    report("gram: gram_bwd")


# ------------------------------------------------------------------------------------------------
# the rare path of split8 (a wave with a value whose hi overflows, or a non-finite one) outside the
# forward conv
# ------------------------------------------------------------------------------------------------

RARE_WGRAD = [("wgrad3", 2, 64, 8, 32, 64, 1), ("wgrad_co3", 2, 64, 24, 48, 3, 1)]
TINY = 2.0 ** -10   # "about 1e-3", and exact: the scaled operands keep their mantissas


@pytest.mark.parametrize("case", RARE_WGRAD, ids=lambda c: c[0])
def test_conv_wgrad_large_finite_operand(case, hip_device):
    """One x of 3.4e38 (above bf16's largest value: hi is clamped, the remainder stays exact) beside
    operands of about 1e-3: finite, within the single-product bar, and every dW entry whose product does not
    involve it keeps its bits."""
    fam, n, cin, h, w, cout, up = case
    pos = [(h // 2, w // 2)] + pixel_positions(h, w)
    dy = P.one_pixel_per_plane((n, cout, h, w), pos, seed=600) * TINY
    x = P.loud(601, (n, cin, h, w)) * TINY
    xb = x.clone()
    big = torch.zeros_like(x)
    big[0, 5, h // 2, w // 2 + 1] = 1
    xb[big != 0] = 3.4e38
    involved = P.wgrad64(big, (dy != 0).double(), up, "zeros")[0] > 0
    assert bool(involved.any()) and dy[0, 0, h // 2, w // 2] != 0
    dw0, _ = run_wgrad(x, dy, cout, up, "zeros", hip_device)
    dw1, db1 = run_wgrad(xb, dy, cout, up, "zeros", hip_device)
    assert bool(torch.isfinite(dw1).all()) and bool(torch.isfinite(db1).all())
    (rw, rb) = P.wgrad_ref(xb, dy, up, "zeros")
    assert float(rw[2].max()) == 1
    one, _ = P.check_products(dw1, *rw, what=f"{fam} with a 3.4e38 x")
    P.check_products(db1, *rb, what=f"{fam} with a 3.4e38 x: db")
    assert float(dw1.cpu()[involved].abs().max()) > 1e34
    assert torch.equal(bits(dw1.cpu()[~involved]), bits(dw0.cpu()[~involved]))
    print(f"x3 probe max ulp: wgrad: {fam} with one 3.4e38 operand: single products {one:.2f}")


@pytest.mark.parametrize("case", RARE_WGRAD, ids=lambda c: c[0])
def test_conv_wgrad_nan_in_dy(case, hip_device):
    """One NaN in dy makes NaN exactly the dW / db entries torch's CPU result has as NaN (the trainers'
    non-finite-gradient check reads them)."""
    fam, n, cin, h, w, cout, up = case
    x = P.loud(610, (n, cin, h, w))
    dy = P.loud(611, (n, cout, h, w))
    dy[n - 1, cout - 2, h // 2, w // 2 - 1] = float("nan")
    rw, rb = P.wgrad64(x, dy, up, "reflect")
    assert bool(torch.isnan(rw[cout - 2]).all()) and int(torch.isnan(rb).sum()) == 1
    dw, db = Fn.conv_weight_grad(x.to(hip_device), dy.to(hip_device), cout, up, "reflect")
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(dw).cpu(), torch.isnan(rw))
    assert torch.equal(torch.isnan(db).cpu(), torch.isnan(rb))


def test_gram_large_finite_operand(hip_device):
    """One feature of 3.4e38 beside features of about 1e-3: its own diagonal entry is its square, past fp32
    (torch: +inf; here non-finite: 3.4e38 splits into hi 3.39e38, mid 1.05e36, lo -1.99e33, whose term
    products hi*hi = +inf and hi*lo = -inf meet as NaN, the "+-inf or NaN" of csrc/x3.h); the rest of its
    row and column is finite and within the single-product bar, and every other entry keeps its bits."""
    n, c, h, w = 3, 64, 8, 8
    hw = h * w
    k0s = [5, 40, 63]
    f = P.one_column(n, c, hw, k0s, seed=620) * TINY
    fb = f.clone()
    fb[1, 7, 40] = 3.4e38
    g0 = L.gram_matrix(f.view(n, c, h, w).to(hip_device)).cpu()
    g1 = L.gram_matrix(fb.view(n, c, h, w).to(hip_device)).cpu()
    assert not bool(torch.isfinite(g1[1, 7, 7]))
    ref, A, m = P.gram_ref(fb)
    g1z = g1.clone()
    for t in (g1z, ref, A, m):
        t[1, 7, 7] = 0
    assert bool(torch.isfinite(g1z).all())
    one, _ = P.check_products(g1z, ref, A, m, what="gram with a 3.4e38 feature")
    assert float(g1z[1, 7].abs().max()) > 1e30
    untouched = torch.ones(n, c, c, dtype=torch.bool)
    untouched[1, 7, :] = False
    untouched[1, :, 7] = False
    assert torch.equal(bits(g1[untouched]), bits(g0[untouched]))
    print(f"x3 probe max ulp: gram: gram_x3_kernel with one 3.4e38 operand: single products {one:.2f}")


def test_gram_nan_in_features(hip_device):
    n, c, h, w = 3, 64, 8, 8
    f = P.one_column(n, c, h * w, [5, 40, 63], seed=630)
    f[2, 11, 17] = float("nan")
    ref = R.gram_matrix(f.view(n, c, h, w))
    assert int(torch.isnan(ref).sum()) == 2 * c - 1
    got = L.gram_matrix(f.view(n, c, h, w).to(hip_device)).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    clean = L.gram_matrix(torch.nan_to_num(f).view(n, c, h, w).to(hip_device)).cpu()
    assert torch.equal(bits(got[:2]), bits(clean[:2]))   # the other images are untouched
