"""CPU: the surface of regional multi-style AdaIN (ops, library, models, header constants), the
C-ABI and host-side argument checks, the fake kernels, and the float64 restatement
tests/regions_ref.py pinned to the project's oracle and to F.interpolate. Nothing is launched."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import regions_ref as RR
from arbitrarystyletransfer_amd import _lib
from oracle import ref_cpu as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")


def test_surface():
    from arbitrarystyletransfer_amd import library, models, ops
    for name in ("resize_labels", "region_stats", "adain_regions"):
        assert callable(getattr(ops, name)), name
        assert name in library.OPS
        assert hasattr(torch.ops.ast_hip, name), name
    assert callable(models.AdaINStyleTransfer.stylize_regions)
    for name in ("ast_resize_labels_u8", "ast_region_stats_f32", "ast_adain_regions_f32"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name


def test_header_constants_match_python_limits():
    from arbitrarystyletransfer_amd import ops
    src = open(HEADER).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(AST_MAX_\w+)\s+(\d+)", src)}
    assert consts["AST_MAX_REGIONS"] == ops.MAX_REGIONS == RR.MAX_REGIONS == 8
    assert consts["AST_MAX_STYLE_ROWS"] == ops.MAX_STYLE_ROWS == RR.MAX_STYLE_ROWS == 64


@pytest.mark.parametrize("call", [
    # resize_labels: each pointer, zero sizes
    lambda L: L.ast_resize_labels_u8(None, 1, 1, 4, 4, 2, 2, None),
    lambda L: L.ast_resize_labels_u8(1, None, 1, 4, 4, 2, 2, None),
    lambda L: L.ast_resize_labels_u8(1, 1, 0, 4, 4, 2, 2, None),
    lambda L: L.ast_resize_labels_u8(1, 1, 1, 0, 4, 2, 2, None),
    lambda L: L.ast_resize_labels_u8(1, 1, 1, 4, 0, 2, 2, None),
    lambda L: L.ast_resize_labels_u8(1, 1, 1, 4, 4, 0, 2, None),
    lambda L: L.ast_resize_labels_u8(1, 1, 1, 4, 4, 2, 0, None),
    # region_stats: each pointer, zero sizes, regions 0 and 9
    lambda L: L.ast_region_stats_f32(None, 1, 1, 1, 1, 1, 2, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, None, 1, 1, 1, 1, 2, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, None, 1, 1, 1, 2, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, None, 1, 1, 2, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, None, 1, 2, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, 1, 0, 2, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, 1, 1, 0, 4, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, 1, 1, 2, 0, 4, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, 1, 1, 2, 4, 0, 2, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, 1, 1, 2, 4, 4, 0, None),
    lambda L: L.ast_region_stats_f32(1, 1, 1, 1, 1, 1, 2, 4, 4, 9, None),
    # adain_regions: each pointer, zero sizes, regions 0 and 9, rows 0 and 65, a bad stride
    lambda L: L.ast_adain_regions_f32(None, 1, 1, 1, 1, 1, 1, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, None, 1, 1, 1, 1, 1, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, None, 1, 1, 1, 1, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, None, 1, 1, 1, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, None, 1, 1, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, None, 1, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 0, 2, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 0, 4, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 0, 4, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 0, 2, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 4, 0, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 4, 9, 3, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 4, 2, 0, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 4, 2, 65, 0, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 4, 2, 3, 5, 1.0, 1, None),
    lambda L: L.ast_adain_regions_f32(1, 1, 1, 1, 1, 1, 1, 2, 4, 4, 2, 3, -6, 1.0, 1, None),
])
def test_argument_errors_rejected_before_launch(call):
    assert call(_lib.lib()) < 0


def test_cpu_tensors_and_wrong_label_dtype_are_rejected():
    from arbitrarystyletransfer_amd import ops
    x = torch.rand(1, 2, 4, 4)
    lab = torch.zeros(1, 4, 4, dtype=torch.uint8)
    tab = torch.rand(1, 2)
    mix = torch.ones(1, 1, 1)
    with pytest.raises(_lib.HipOpError):
        ops.resize_labels(lab, 2, 2)
    with pytest.raises(_lib.HipOpError):
        ops.region_stats(x, lab, 1)
    with pytest.raises(_lib.HipOpError):
        ops.adain_regions(x, lab, tab, tab, mix)
    # the label dtype is checked before the device, so the message names it here too
    for bad in (lab.long(), lab.float(), lab.to(torch.int8)):
        with pytest.raises(_lib.HipOpError, match="uint8"):
            ops.resize_labels(bad, 2, 2)
        with pytest.raises(_lib.HipOpError, match="uint8"):
            ops.region_stats(x, bad, 1)
        with pytest.raises(_lib.HipOpError, match="uint8"):
            ops.adain_regions(x, bad, tab, tab, mix)
    with pytest.raises(_lib.HipOpError):
        ops.region_stats(x, lab, 0)
    with pytest.raises(_lib.HipOpError):
        ops.region_stats(x, lab, 9)


@pytest.mark.parametrize("weights", [
    [[1.0, -0.5], [0.5, 0.5]],            # a negative entry
    [[1.0, float("nan")], [0.5, 0.5]],    # a NaN
    [[1.0, float("inf")], [0.5, 0.5]],    # not finite
    [[0.0, 0.0], [0.5, 0.5]],             # a zero row
    [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],   # wrong S
    [1.0, 0.0],                           # wrong rank
    torch.ones(3, 2, 2),                  # wrong N
    torch.ones(9, 2),                     # too many regions
])
def test_bad_weights_raise_value_error(weights):
    from arbitrarystyletransfer_amd import models
    net = models.AdaINStyleTransfer(weights="live")
    c = torch.zeros(2, 3, 64, 72)
    s = torch.zeros(2, 3, 64, 72)
    lab = torch.zeros(2, 64, 72, dtype=torch.uint8)
    with torch.no_grad(), pytest.raises(ValueError):
        net.stylize_regions(c, s, labels=lab, weights=weights)
    with pytest.raises(ValueError):
        models.region_weights(weights, 2, 2)


def test_weights_are_normalised_in_float64():
    from arbitrarystyletransfer_amd import models
    w = models.region_weights([[2.0, 6.0], [1.0, 0.0]], 3, 2)
    assert w.dtype == torch.float64 and tuple(w.shape) == (1, 2, 2)
    assert torch.equal(w, torch.tensor([[[0.25, 0.75], [1.0, 0.0]]], dtype=torch.float64))
    assert torch.equal(models.region_weights(None, 3, 2), torch.eye(2, dtype=torch.float64)[None])
    assert torch.equal(models.region_weights(None, 3, 4, single_region=True),
                       torch.full((1, 1, 4), 0.25, dtype=torch.float64))
    assert tuple(models.region_weights(torch.ones(3, 2, 2), 3, 2).shape) == (3, 2, 2)
    with pytest.raises(ValueError):   # labels=None is one region
        models.region_weights([[1.0, 0.0], [0.0, 1.0]], 3, 2, single_region=True)
    for args in ((None, 3, 2), ([[2.0, 6.0], [1.0, 0.0]], 3, 2)):
        assert torch.equal(models.region_weights(*args), RR.normalise_weights(*args))


def test_stylize_regions_is_inference_only():
    from arbitrarystyletransfer_amd import models
    net = models.AdaINStyleTransfer(weights="live")
    assert any(p.requires_grad for p in net.parameters())
    c = torch.zeros(1, 3, 64, 72)
    with pytest.raises(NotImplementedError):
        net.stylize_regions(c, c)


def test_fake_kernels_give_shapes_and_dtypes():
    from arbitrarystyletransfer_amd import library  # noqa: F401
    o = torch.ops.ast_hip
    m = torch.device("meta")
    x = torch.empty(2, 16, 8, 12, device=m)
    lab = torch.empty(2, 8, 12, device=m, dtype=torch.uint8)
    r = o.resize_labels(torch.empty(2, 64, 96, device=m, dtype=torch.uint8), 8, 12)
    assert r.shape == (2, 8, 12) and r.dtype == torch.uint8
    mean, std, count = o.region_stats(x, lab, 3)
    assert mean.shape == std.shape == (2, 3, 16) and mean.dtype == std.dtype == torch.float32
    assert count.shape == (2, 3) and count.dtype == torch.int32
    out = o.adain_regions(x, lab, torch.empty(5, 16, device=m), torch.empty(5, 16, device=m),
                          torch.empty(1, 3, 5, device=m), 0.5, True)
    assert out.shape == x.shape and out.dtype == torch.float32


@pytest.mark.parametrize("alpha", [1.0, 0.3])
def test_restatement_degenerates_to_the_oracle(alpha):
    """K = 1, T = 1, all-zero labels: the oracle's AdaIN from statistics (swapped affine) and blend."""
    c = RR.features(3001, (2, 5, 9, 13)).double()
    mean, std = (t.double() for t in RR.style_table(3002, 1, 5))
    lab = torch.zeros(2, 9, 13, dtype=torch.uint8)
    got = RR.adain_regions(c, lab, mean, std, torch.ones(1, 1, 1, dtype=torch.float64), alpha, True)
    ref = R.alpha_blend(R.adain_from_stats(c, mean[0], std[0]), c, alpha)
    assert RR.rel_inf(got, ref) <= 1e-12
    # not swapped: the same with the two tables exchanged
    got = RR.adain_regions(c, lab, mean, std, torch.ones(1, 1, 1, dtype=torch.float64), alpha, False)
    ref = R.alpha_blend(R.adain_from_stats(c, std[0], mean[0]), c, alpha)
    assert RR.rel_inf(got, ref) <= 1e-12
    # and its statistics are the oracle's channel_stats
    m, s, n = RR.region_stats(c, lab, 1)
    om, os_ = R.channel_stats(c)
    assert RR.rel_inf(m[:, 0], om.flatten(1)) <= 1e-12 and RR.rel_inf(s[:, 0], os_.flatten(1)) <= 1e-12
    assert n.tolist() == [[117], [117]]


def test_restatement_region_semantics():
    """Regions are independent, zero weights skip their rows, labels >= K pass through, and the
    empty and one-pixel regions give NaN in kind."""
    c = RR.features(3003, (1, 3, 6, 8)).double()
    lab = RR.label_map(1, 6, 8, 2)
    lab[0, 0, 0], lab[0, 5, 7], lab[0, 2, 2] = 255, 9, 3
    mean, std = (t.double() for t in RR.style_table(3004, 2, 3))
    nan_mean = mean.clone()
    nan_mean[1] = float("nan")
    mix = torch.tensor([[[1.0, 0.0], [0.25, 0.75]]], dtype=torch.float64)
    out = RR.adain_regions(c, lab, mean, std, mix, 1.0, True)
    keep = lab[0] >= 2
    assert int(keep.sum()) == 3 and torch.equal(out[0][:, keep], c[0][:, keep])
    # region 0 alone, with the other pixels relabelled as pass-through, gives the same region 0
    only0 = torch.where(lab == 0, lab, torch.full_like(lab, 255))
    out0 = RR.adain_regions(c, only0, mean, std, mix[:, :1], 1.0, True)
    assert torch.equal(out0[0][:, lab[0] == 0], out[0][:, lab[0] == 0])
    # a NaN row that region 0 does not use reaches region 1 only
    outn = RR.adain_regions(c, lab, nan_mean, std, mix, 1.0, True)
    assert torch.equal(outn[0][:, lab[0] == 0], out[0][:, lab[0] == 0])
    assert torch.isnan(outn[0][:, lab[0] == 1]).all()
    m, s, n = RR.region_stats(c, lab, 4)
    assert n.tolist() == [[int((lab == k).sum()) for k in range(4)]] and n[0, 2] == 0 and n[0, 3] == 1
    assert torch.isnan(m[0, 2]).all() and torch.isnan(s[0, 2]).all()
    assert torch.isfinite(m[0, 3]).all() and torch.isnan(s[0, 3]).all()
    assert torch.isfinite(m[0, :2]).all() and torch.isfinite(s[0, :2]).all()


@pytest.mark.parametrize("src,dst", RR.RESIZE_PAIRS)
def test_restatement_resize_is_interpolate_nearest(src, dst):
    g = torch.Generator().manual_seed(src[0] * 1000 + src[1])
    lab = torch.randint(0, 256, (2,) + src, dtype=torch.uint8, generator=g)
    ref = F.interpolate(lab[:, None], size=dst, mode="nearest")[:, 0]
    got = RR.resize_labels(lab, *dst)
    assert got.dtype == torch.uint8 and torch.equal(got, ref)


@pytest.mark.parametrize("idx", range(len(RR.CASES)))
def test_generated_regions_are_populated(idx):
    """Every region of every parity case has at least 19 pixels (so its statistics are far from the
    one-pixel NaN), and the holes are where the pass-through tests expect them."""
    shape, k, _, hole = RR.CASES[idx]
    _, lab, _, _, _, _ = RR.case_inputs(idx)
    for i in range(shape[0]):
        counts = [int((lab[i] == r).sum()) for r in range(k)]
        assert min(counts) >= 19, (idx, i, counts)
    assert bool((lab == 255).any()) == hole
    assert bool(((lab >= k) & (lab != 255)).any()) is False


def test_fp32_restatement_noise_is_far_below_the_op_tolerance():
    """The bar of the GPU tests (2e-5) against the reference's own float32 rounding on the same cases."""
    worst = 0.0
    for idx in range(len(RR.CASES)):
        c, lab, mean, std, mix, k = RR.case_inputs(idx)
        r64 = RR.adain_regions(c.double(), lab, mean.double(), std.double(), mix.double(), 0.3, True)
        r32 = RR.adain_regions(c, lab, mean, std, mix, 0.3, True)
        worst = max(worst, RR.rel_inf(r32, r64, lab < k))
    print(f"fp32 restatement vs float64: {worst:.2e}")
    assert worst <= 2e-6
