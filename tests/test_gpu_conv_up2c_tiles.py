"""GPU: the two forms of the collapsed upsampled conv (conv3x3_up2c_kernel) -- 8 waves
on 32 x 32 output pixels with the weight slab double-buffered, one workgroup per CU, and 4 waves on
16 x 32 output pixels with one slab buffer, two workgroups per CU. Every accumulator receives the
same products in the same order in both, so their outputs are compared bit for bit (as int32, so
NaNs compare too); the 4-wave form is also held against the float64 oracle at the op bar of
tests/test_gpu_conv_up2c.py, with inputs built as there.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arbitrarystyletransfer_amd import ops, synth
from arbitrarystyletransfer_amd._lib import HipOpError, lib

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5

UP2C_CASES = [  # those of tests/test_gpu_conv_up2c.py: n, cin, h_in, w_in, cout
    (1, 16, 1, 1, 16),
    (2, 24, 5, 7, 64),
    (1, 32, 17, 33, 128),
    (2, 80, 16, 16, 192),
]


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


# n, cin, h_in, w_in, cout, n2 (the last n2 images passed as x2)
MANY_BLOCKS = (4, 16, 64, 64, 160, 2)  # 128 16-row tiles x 5 groups = 640 workgroups > 512 resident slots: CUs are
#                                        shared between workgroups and a later round runs
TILE_CASES = [c + (0,) for c in UP2C_CASES] + [
    (1, 32, 9, 17, 64, 0),    # 18 output rows: two 16-row tiles against one 32-row tile; one column into the next tile
    (1, 24, 5, 7, 40, 0),     # a partial last chunk and a partial channel group together
    MANY_BLOCKS,
]
assert (2, 80, 16, 16, 192, 0) in TILE_CASES  # five chunks through the single slab buffer, six channel groups


def bits(t):
    return t.contiguous().view(torch.int32)


def run(case, with_bias, tile, dev, x=None):
    n, cin, h, w, cout, n2 = case
    xs, wt, bs = inputs(case[:5], 4600)
    if x is not None:
        xs = x
    xd = xs.to(dev)
    x1, x2 = (xd[:n - n2], xd[n - n2:]) if n2 else (xd, None)
    ext = ops.pack_conv3x3(wt.to(dev), up2c=True)
    pre, act, _ = ops.conv3x3(x1, ext, bs.to(dev) if with_bias else None, cout, upsample=2, pad_mode="reflect",
                              want_pre=True, want_act=True, x2=x2, _up2c_tile=tile)
    torch.cuda.synchronize()
    return pre, act


@functools.lru_cache(maxsize=None)
def eight_wave(case, with_bias, dev):
    """The 8-wave form's outputs: computed once per case, shared, never written."""
    return run(case, with_bias, 8, dev)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", TILE_CASES)
def test_four_wave_bits_equal_eight_wave(case, with_bias, hip_device):
    pre8, act8 = eight_wave(case, with_bias, str(hip_device))
    pre4, act4 = run(case, with_bias, 4, hip_device)
    assert pre4.shape == pre8.shape == (case[0], case[4], 2 * case[2], 2 * case[3])
    assert torch.equal(bits(pre4), bits(pre8))
    assert torch.equal(bits(act4), bits(act8))


def test_four_wave_bits_equal_eight_wave_non_finite(hip_device):
    case = (1, 16, 4, 4, 16, 0)
    x, _, _ = inputs(case[:5], 4600)
    x[0, 3, 0, 1] = float("inf")
    x[0, 9, 3, 2] = float("nan")
    pre8, act8 = run(case, True, 8, hip_device, x=x)
    pre4, act4 = run(case, True, 4, hip_device, x=x)
    bad = ~torch.isfinite(pre8)
    assert bad.any() and not bad.all()
    assert torch.equal(bits(pre4), bits(pre8))
    assert torch.equal(bits(act4), bits(act8))


@pytest.mark.parametrize("case", [(1, 32, 9, 17, 64, 0), (2, 80, 16, 16, 192, 0)])
def test_four_wave_vs_oracle(case, hip_device):
    x, wt, bs = inputs(case[:5], 4600)
    pre_r, act_r = oracle_conv(x, wt, bs)
    pre, act = run(case, True, 4, hip_device)
    e_pre, e_act = rel_inf(pre, pre_r), rel_inf(act, act_r)
    print(f"up2c 4-wave {case}: rel_inf pre {e_pre:.2e} act {e_act:.2e}")
    assert e_pre <= OP_TOL, e_pre
    assert e_act <= OP_TOL, e_act


def test_four_wave_run_twice_bit_equal(hip_device):
    a = run(MANY_BLOCKS, True, 4, hip_device)
    b = run(MANY_BLOCKS, True, 4, hip_device)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_four_wave_two_workgroups_per_cu(hip_device):
    """The 4-wave form exists to put two workgroups on a CU: at its launch size (256 threads, its
    dynamic LDS, its registers) the runtime must place exactly two, the 8-wave form one."""
    assert lib().ast_conv3x3_up2c_occupancy(4) == 2
    assert lib().ast_conv3x3_up2c_occupancy(8) == 1


# below the rule's thresholds / a full launch at few chunks / a full launch past 16 chunks per block (17)
@pytest.mark.parametrize("case", [UP2C_CASES[0] + (0,), MANY_BLOCKS, (2, 272, 64, 64, 256, 0)])
def test_auto_is_one_of_the_forms(case, hip_device):
    """launch_up2c's rule: 4 waves when the 8-wave workgroups would not fill the CUs or a block has
    at most 16 K chunks, else 8 (AST_UP2C_TILE forces one); auto then gives that form's bits."""
    n, cin, h, w, cout, n2 = case
    tile = lib().ast_conv3x3_up2c_variant(n, cin, h, w, cout)
    forced = os.environ.get("AST_UP2C_TILE")
    if forced in ("4", "8"):
        assert tile == int(forced)
    else:
        cdiv = lambda a, b: -(-a // b)  # noqa: E731
        wg8 = cdiv(n * cdiv(2 * h, 32) * cdiv(2 * w, 32), 8) * 8 * cdiv(cout, 32)
        cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
        assert tile == (4 if wg8 < cus or cdiv(cin, 16) <= 16 else 8), (tile, wg8, cus)
    auto, chosen = run(case, True, 0, hip_device), run(case, True, tile, hip_device)
    assert torch.equal(bits(auto[0]), bits(chosen[0])) and torch.equal(bits(auto[1]), bits(chosen[1]))
    with pytest.raises(HipOpError):  # the keyword reaches the collapsed kernel only
        ops.conv3x3(torch.zeros(1, cin, h, w, device=hip_device), ops.pack_conv3x3(
            torch.zeros(cout, cin, 3, 3, device=hip_device)), None, cout, upsample=2, pad_mode="reflect", _up2c_tile=4)
