"""GPU: the collapsed upsampled conv (conv3x3_up2c_kernel: 2x2 taps per output phase, reached through
an extended pack, ops.pack_conv3x3(w, up2c=True)) against the float64 oracle of the 9-tap form --
nearest x2 -> ReflectionPad2d(1) -> conv3x3; tests/test_up2c_cpu.py holds the identity between the two.

Tolerances as tests/test_gpu_parity.py: single ops rel_inf = max|a-b| / max|b| <= 2e-5, the decoder
1e-3. The kernel's tile is 32 x 32 output pixels (16 x 16 source pixels) x 32 output channels, K
chunks of 16 input channels, the weight slab double-buffered.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arbitrarystyletransfer_amd import functional as Fn
from arbitrarystyletransfer_amd import models, ops, synth

pytestmark = pytest.mark.gpu

E2E_TOL = 1e-3
OP_TOL = 2e-5


def rel_inf(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def oracle_conv(x, w, b):
    """float64: Upsample(x2, nearest) -> ReflectionPad2d(1) -> Conv2d(3x3) (+ ReLU)."""
    x, w = x.double(), w.double()
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w, b.double() if b is not None else None)
    return y, F.relu(y)


def inputs(case, seed):
    n, cin, h, w, cout = case
    x = torch.from_numpy(synth.image(seed + cin, (n, cin, h, w)) * 2 - 0.5).float()
    wt = torch.from_numpy(synth.conv_weight(seed + 100 + cin, cout, cin, 3)).float()
    bs = torch.from_numpy(synth.conv_bias(seed + 200 + cin, cout)).float()
    return x, wt, bs


UP2C_CASES = [
    # n, cin, h_in, w_in, cout
    (1, 16, 1, 1, 16),     # a 1x1 source: every tap clamps; one chunk; a partial channel group
    (2, 24, 5, 7, 64),     # a partial last K chunk, odd sizes below one tile
    (1, 32, 17, 33, 128),  # one row / one column into the next 16x16-source tile, two chunks, four channel groups
    (2, 80, 16, 16, 192),  # five chunks (both slab buffers reused), six groups, one exactly full tile, two images
]


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", UP2C_CASES)
def test_up2c_vs_oracle(case, with_bias, hip_device):
    n, cin, h, w, cout = case
    x, wt, bs = inputs(case, 4000)
    pre_r, act_r = oracle_conv(x, wt, bs if with_bias else None)
    xd, wd = x.to(hip_device), wt.to(hip_device)
    bd = bs.to(hip_device) if with_bias else None
    ext, plain = ops.pack_conv3x3(wd, up2c=True), ops.pack_conv3x3(wd)
    assert ext.numel() > plain.numel() and torch.equal(ext[:plain.numel()], plain)
    kw = dict(upsample=2, pad_mode="reflect", want_pre=True, want_act=True)
    pre, act, _ = ops.conv3x3(xd, ext, bd, cout, **kw)
    pre9, act9, _ = ops.conv3x3(xd, plain, bd, cout, **kw)
    torch.cuda.synchronize()
    e_pre, e_act = rel_inf(pre, pre_r), rel_inf(act, act_r)
    print(f"up2c {case} bias={with_bias}: rel_inf pre {e_pre:.2e} act {e_act:.2e} | "
          f"9-tap pre {rel_inf(pre9, pre_r):.2e} act {rel_inf(act9, act_r):.2e}")
    assert e_pre <= OP_TOL, e_pre
    assert e_act <= OP_TOL, e_act
    # each output alone (pre only / act only) takes the same path and gives the same bits
    only_pre, none_act, _ = ops.conv3x3(xd, ext, bd, cout, upsample=2, pad_mode="reflect", want_pre=True,
                                        want_act=False)
    _, only_act, _ = ops.conv3x3(xd, ext, bd, cout, upsample=2, pad_mode="reflect")
    assert none_act is None and torch.equal(only_pre, pre) and torch.equal(only_act, act)


def test_up2c_non_finite(hip_device):
    """An output reached by an inf or NaN input is non-finite, as in the 9-tap form (there possibly
    NaN where this one gives +-inf: inf w1 + inf w2 against inf (w1 + w2) for opposite-sign taps);
    every other output meets the op bar."""
    case = (1, 16, 4, 4, 16)
    x, wt, bs = inputs(case, 4100)
    x[0, 3, 0, 1] = float("inf")
    x[0, 9, 3, 2] = float("nan")
    pre_r, _ = oracle_conv(x, wt, bs)
    bad = ~torch.isfinite(pre_r)
    assert bad.any() and not bad.all()
    d = hip_device
    pre, _, _ = ops.conv3x3(x.to(d), ops.pack_conv3x3(wt.to(d), up2c=True), bs.to(d), 16, upsample=2,
                            pad_mode="reflect", want_pre=True, want_act=False)
    pre = pre.cpu()
    assert not torch.isfinite(pre[bad]).any()
    assert torch.isfinite(pre[~bad]).all()
    err = float((pre[~bad].double() - pre_r[~bad]).abs().max() / pre_r[~bad].abs().max())
    print(f"up2c non-finite: {int(bad.sum())} outputs reached, rel_inf elsewhere {err:.2e}")
    assert err <= OP_TOL, err


def test_up2c_run_twice_bit_equal(hip_device):
    case = UP2C_CASES[2]
    x, wt, bs = inputs(case, 4200)
    d = hip_device
    xd, ext, bd = x.to(d), ops.pack_conv3x3(wt.to(d), up2c=True), bs.to(d)
    a = ops.conv3x3(xd, ext, bd, case[4], upsample=2, pad_mode="reflect", want_pre=True, want_act=True)
    b = ops.conv3x3(xd, ext, bd, case[4], upsample=2, pad_mode="reflect", want_pre=True, want_act=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_up2c_fallback_keeps_nine_tap_bits(hip_device):
    """A plain pack, and an extended pack outside the collapsed kernel's scope (zero padding, a fused
    pool, an explicit cfg), run the 9-tap kernel: the bits of cfg = -1 with a plain pack."""
    case = (2, 24, 6, 10, 64)
    x, wt, bs = inputs(case, 4300)
    d = hip_device
    xd, bd = x.to(d), bs.to(d)
    plain, ext = ops.pack_conv3x3(wt.to(d)), ops.pack_conv3x3(wt.to(d), up2c=True)
    for kw in (dict(pad_mode="reflect"), dict(pad_mode="zeros"), dict(pad_mode="reflect", want_pool=True)):
        ref = ops.conv3x3(xd, plain, bd, 64, upsample=2, want_pre=True, want_act=True, cfg=-1, **kw)
        pk = plain if kw == dict(pad_mode="reflect") else ext
        got = ops.conv3x3(xd, pk, bd, 64, upsample=2, want_pre=True, want_act=True, **kw)
        torch.cuda.synchronize()
        for r, g in zip(ref, got):
            assert (r is None) == (g is None)
            if r is not None:
                assert torch.equal(r, g), (kw, float((r - g).abs().max()))
    # an explicit configuration index with an extended pack: that configuration's 9-tap kernel
    ref = ops.conv3x3(xd, plain, bd, 64, upsample=2, pad_mode="reflect", cfg=28)
    got = ops.conv3x3(xd, ext, bd, 64, upsample=2, pad_mode="reflect", cfg=28)
    assert torch.equal(ref[1], got[1])


def _decoder(hip_device, up2c):
    dec = models.VGGDecoder().to(hip_device).eval()
    dec._up2c = up2c
    return dec


def test_up2c_decoder_matches_nine_tap(hip_device):
    """models.VGGDecoder (eval, 1x512x8x8) with extended packs against plain packs: eager inference,
    and the decoder's layers through DecoderConvFn with gradients. The backward does not read the
    collapsed slab: a DecoderConvFn layer's input and weight gradients for a given output gradient
    are bit-equal with either pack (last part). Through the whole chain the gradients are compared
    at the decoder bar, not bit for bit: each layer's gradients are computed from the previous
    layers' activations and ReLU masks, which carry the two forwards' rounding difference. (The
    module itself keeps plain packs under autograd, see VGGDecoder.forward.)"""
    x = torch.from_numpy(synth.image(4400, (1, 512, 8, 8))).float().to(hip_device)
    ext, plain = _decoder(hip_device, True), _decoder(hip_device, False)
    with torch.no_grad():
        y_ext, y_plain = ext(x), plain(x)
    torch.cuda.synchronize()
    e = rel_inf(y_ext, y_plain)
    print(f"up2c decoder 1x512x8x8: eager rel_inf extended vs plain packs {e:.2e}")
    assert e <= E2E_TOL, e
    assert not torch.equal(y_ext, y_plain)   # the extended packs did take the collapsed kernel

    grads = []
    for up2c in (True, False):
        xg = x.clone().requires_grad_(True)
        plain.zero_grad()
        t = xg
        for conv, up, relu in plain._groups:
            t = Fn.DecoderConvFn.apply(t, conv.weight, conv.bias,
                                       ops.pack_conv3x3(conv.weight.detach(), up2c=up and up2c), 2 if up else 1, relu)
        t.backward(torch.ones_like(t))
        grads.append((t.detach(), xg.grad, [c.weight.grad.clone() for c in plain.convs()]))
    torch.cuda.synchronize()
    (ye, dxe, dwe), (yp, dxp, dwp) = grads
    assert torch.equal(ye, y_ext) and torch.equal(yp, y_plain)   # the same kernels as the inference path
    print(f"up2c decoder grads: dx {rel_inf(dxe, dxp):.2e} dw max {max(rel_inf(a, b) for a, b in zip(dwe, dwp)):.2e}")
    assert rel_inf(dxe, dxp) <= E2E_TOL
    for a, b in zip(dwe, dwp):
        assert rel_inf(a, b) <= E2E_TOL

    # one upsampled layer, no ReLU: the same output gradient gives the same bits with either pack
    case = (2, 32, 9, 12, 48)
    xs, wt, bs = inputs(case, 4500)
    g = torch.from_numpy(synth.image(4501, (2, 48, 18, 24))).float().to(hip_device) - 0.5
    res = []
    for up2c in (True, False):
        xd = xs.to(hip_device).requires_grad_(True)
        wd = wt.to(hip_device).requires_grad_(True)
        bd = bs.to(hip_device).requires_grad_(True)
        y = Fn.DecoderConvFn.apply(xd, wd, bd, ops.pack_conv3x3(wd.detach(), up2c=up2c), 2, False)
        y.backward(g)
        res.append((y.detach(), xd.grad, wd.grad, bd.grad))
    torch.cuda.synchronize()
    assert rel_inf(res[0][0], res[1][0]) <= OP_TOL
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)
