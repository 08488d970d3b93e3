"""CPU: the identity behind the collapsed upsampled conv (conv3x3_up2c_kernel).

nearest x2 -> ReflectionPad2d(1) -> conv3x3 equals, per output phase (py, px) = (row & 1, col & 1),
a 2x2 conv of the replicate-padded SOURCE with tap sums of the 3x3 filter:

    out[2i + py, 2j + px] = sum_{a, b in {0, 1}} Wc[py][px][a][b] . src[clamp(i + py - 1 + a), clamp(j + px - 1 + b)]

py = 0 uses rows {w[0], w[1] + w[2]}, py = 1 rows {w[0] + w[1], w[2]}; columns alike. The phase form
is kept here in pure torch; tests/test_gpu_conv_up2c.py relies on the identity when it compares the
kernel with the 9-tap float64 oracle.
"""
import pytest
import torch
import torch.nn.functional as F


def collapse_weights(w):
    """[cout, cin, 3, 3] -> Wc[py][px] of [cout, cin, 2, 2] (tap sums, in w's dtype)."""
    def pair(t, phase, dim):   # the two summed taps of one dimension, stacked on `dim`
        t0, t1, t2 = t.unbind(dim)
        return torch.stack((t0, t1 + t2) if phase == 0 else (t0 + t1, t2), dim)
    return [[pair(pair(w, py, 2), px, 3) for px in (0, 1)] for py in (0, 1)]


def up2c_conv(x, w, b, round_weights_fp32=False):
    """The phase form of conv3x3(reflect_pad(upsample2(x))) on the source grid."""
    n, _, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    wc = collapse_weights(w)
    out = x.new_zeros((n, w.shape[0], 2 * h, 2 * wd))
    for py in (0, 1):
        for px in (0, 1):
            k = wc[py][px]
            if round_weights_fp32:
                k = k.float().to(x.dtype)
            # src[i + py - 1 + a, j + px - 1 + b] = xp[i + py + a, j + px + b]
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + wd + 1], k)
    return out + b.view(1, -1, 1, 1)


def reference(x, w, b):
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w, b)


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (9, 17)])
@pytest.mark.parametrize("cin,cout", [(3, 4), (16, 8)])
def test_phase_form_matches_upsampled_reflect_conv(hw, cin, cout):
    g = torch.Generator().manual_seed(1000 + 17 * hw[0] + hw[1] + cin)
    x = torch.randn((2, cin) + hw, generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64).float().double()   # fp32 parameters
    b = torch.randn((cout,), generator=g, dtype=torch.float64)
    ref = reference(x, w, b)
    scale = ref.abs().max().item()
    exact = (up2c_conv(x, w, b) - ref).abs().max().item() / scale
    rounded = (up2c_conv(x, w, b, round_weights_fp32=True) - ref).abs().max().item() / scale
    print(f"up2c phase form {hw} {cin}->{cout}: rel_inf exact {exact:.2e}, fp32 tap sums {rounded:.2e}")
    assert exact <= 1e-12     # the identity itself: float64 reassociation only
    assert rounded <= 1e-6    # + the tap sums rounded once to fp32 (2^-24 per weight)


def test_collapsed_weights_are_tap_sums():
    w = torch.arange(9, dtype=torch.float64).view(1, 1, 3, 3)
    wc = collapse_weights(w)
    assert wc[0][0][0, 0].tolist() == [[0.0, 1.0 + 2.0], [3.0 + 6.0, 4.0 + 5.0 + 7.0 + 8.0]]
    assert wc[1][1][0, 0].tolist() == [[0.0 + 1.0 + 3.0 + 4.0, 2.0 + 5.0], [6.0 + 7.0, 8.0]]
    assert sum(float(wc[py][px].sum()) for py in (0, 1) for px in (0, 1)) == 4 * 36.0
