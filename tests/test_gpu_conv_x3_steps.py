"""The step schedule of the split-bf16 M16 conv kernel (conv3x3_x3_kernel, configs 28-31 and their
block-loop forms 38-41) on the smallest shapes at which each of its paths runs.

A step of the MFMA phase opens with an MFMA and reads the next step's LDS operands between its
MFMAs; the order of those reads is the compiler's to place, the products and their order per
accumulator are not. So every output must equal, bit for bit, the persistent kernel's
(conv3x3_x3p_kernel, configs 32-35: its own plain loop, the same arithmetic), the block-loop form's,
and a second launch's; and stay within the single-op bar of tests/test_gpu_parity.py against
F.conv2d on the CPU.

Cin 16: one K chunk (no gather or weight DMA inside the steps); 32: one chunk with the interleaved
gather, then the last chunk; 40: a partial last chunk; 64: both parities of the hi + mid weight
buffer. Each as a zero-padded UP = 1 and a reflect-padded UP = 2 launch (cfg given, so the 9-tap
kernel runs, not the collapsed one), Cout 64 and ragged 40 and 192, on 2 images of 18 x 36 (partial
row and column tiles for the 8- and 16-row tiles, several blocks)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arbitrarystyletransfer_amd import ops, synth

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5  # tests/test_gpu_parity.py
N, H, W = 2, 18, 36
CINS = (16, 32, 40, 64)
COUTS = (64, 40, 192)
MODES = ((1, "zeros"), (2, "reflect"))
CFGS = (28, 29, 30, 31)


def rel_inf(a, b):
    a = np.asarray(a.detach().cpu(), np.float64)
    b = np.asarray(b.detach().cpu(), np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


@functools.lru_cache(maxsize=None)
def case(cin, cout, up, pad):
    """Inputs and the CPU reference (pre, ReLU, pool) of one case, computed once."""
    x = torch.from_numpy(synth.image(900 + cin, (N, cin, H, W)) * 2 - 0.5)
    wt = torch.from_numpy(synth.conv_weight(910 + cin + cout, cout, cin, 3))
    bs = torch.from_numpy(synth.conv_bias(920 + cout, cout))
    xu = F.interpolate(x, scale_factor=2, mode="nearest") if up == 2 else x
    if pad == "reflect":
        pre = F.conv2d(F.pad(xu, (1, 1, 1, 1), mode="reflect"), wt, bs)
    else:
        pre = F.conv2d(xu, wt, bs, padding=1)
    act = F.relu(pre)
    return x, wt, bs, (pre, act, F.max_pool2d(act, 2, 2))


@pytest.mark.parametrize("up,pad", MODES)
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
def test_x3_step_schedule(cin, cout, up, pad, hip_device):
    x, wt, bs, ref = case(cin, cout, up, pad)
    xd, bd = x.to(hip_device), bs.to(hip_device)
    wp = ops.pack_conv3x3(wt.to(hip_device))

    def run(cfg, pre=True, act=True):
        # _pack=False: the images as they are, not side by side in one plane
        out = ops.conv3x3(xd, wp, bd, cout, upsample=up, pad_mode=pad, want_pre=pre, want_act=act, want_pool=True,
                          cfg=cfg, _pack=False)
        torch.cuda.synchronize()
        return out

    for cfg in CFGS:
        got = run(cfg)
        for name, g, r in zip(("pre", "act", "pool"), got, ref):
            e = rel_inf(g, r)
            print(f"cin {cin} cout {cout} up {up} cfg {cfg} {name}: rel_inf {e:.2e}")
            assert e <= OP_TOL, (cfg, name, e)
        for other in (cfg + 4, cfg + 10, cfg):  # persistent kernel, block-loop form, a second launch
            for name, g, o in zip(("pre", "act", "pool"), got, run(other)):
                assert torch.equal(g, o), (cfg, other, name, float((g - o).abs().max()))
        pool_only = run(cfg, pre=False, act=False)[2]  # the in-register pool epilogue
        assert torch.equal(pool_only, got[2]), (cfg, float((pool_only - got[2]).abs().max()))
