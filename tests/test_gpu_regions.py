"""GPU: regional multi-style AdaIN (csrc/adain_regions.hip: adain_regions, region_stats,
resize_labels) and AdaINStyleTransfer.stylize_regions against the float64 restatement
tests/regions_ref.py, which test_regions_cpu.py pins to the project's oracle.

OP_TOL is the project's single-op bar (test_gpu_parity.py). rel_inf = max|a - b| / max|b| over the
labelled pixels. On these cases the restatement run in float32 on the CPU sits at or under 2.0e-7
from its float64 run (test_regions_cpu.py asserts 2e-6), so the bar is about 100x the reference's
own rounding noise. Every test prints the figure it asserts on."""
import functools

import pytest
import torch

import regions_ref as RR
from arbitrarystyletransfer_amd import _lib, models, ops

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5
OFFSET_CASE = 2   # "hw is more than one pass of the block": the third case


@functools.lru_cache(maxsize=None)
def _case(idx, shared=False):
    return RR.case_inputs(idx, shared_mix=shared)


@functools.lru_cache(maxsize=None)
def _ref(idx, shared, alpha, swap, offset=0.0):
    c, lab, mean, std, mix, _ = _case(idx, shared)
    c = (c + offset) if offset else c          # the float32 input the kernel sees
    return RR.adain_regions(c.double(), lab, mean.double(), std.double(), mix.double(), alpha, swap)


def _run(dev, c, lab, mean, std, mix, alpha=1.0, swap=True):
    return ops.adain_regions(c.to(dev), lab.to(dev), mean.to(dev), std.to(dev), mix.to(dev), alpha=alpha,
                             swap_style_stats=swap)


def _check(got, ref, lab, k, what):
    """rel_inf over the labelled pixels within OP_TOL; pass-through pixels bit-equal to `ref` there
    (the restatement copies the content)."""
    got = got.cpu()
    err = RR.rel_inf(got, ref, lab < k)
    print(f"{what}: rel_inf {err:.2e}")
    assert err <= OP_TOL, (what, err)
    return got


# 1 ------------------------------------------------------------------------------------------------
PARITY = [(i, False) for i in range(len(RR.CASES))] + [(0, True), (2, True)]


@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 0.3])
@pytest.mark.parametrize("idx,shared", PARITY)
def test_adain_regions_parity(idx, shared, alpha, swap, hip_device):
    c, lab, mean, std, mix, k = _case(idx, shared)
    assert mix.shape[0] == (1 if shared else c.shape[0])
    got = _check(_run(hip_device, c, lab, mean, std, mix, alpha, swap), _ref(idx, shared, alpha, swap), lab, k,
                 f"case {idx} shared={shared} alpha={alpha} swap={swap}")
    keep = (lab >= k)[:, None].expand_as(c)
    assert bool(keep.any()) == RR.CASES[idx][3]
    assert torch.equal(got[keep], c[keep])


# 2 ------------------------------------------------------------------------------------------------
def test_offset_input_needs_two_pass_statistics(hip_device):
    """Content + 30: E[x^2] - mu^2 in float32 loses the variance here (1.2e-4 measured for that
    form on the CPU, 1.4e-6 for the two-pass form), so only mean-then-deviations passes."""
    c, lab, mean, std, mix, k = _case(OFFSET_CASE)
    got = _run(hip_device, c + 30.0, lab, mean, std, mix, 1.0, False)
    _check(got, _ref(OFFSET_CASE, False, 1.0, False, 30.0), lab, k, "offset +30")


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [True, False])
@pytest.mark.parametrize("alpha", [1.0, 0.3])
def test_degenerate_case_agrees_with_existing_kernels(alpha, swap, hip_device):
    c = RR.features(3401, (1, 6, 12, 20)).to(hip_device)
    s = (RR.features(3402, (1, 6, 10, 14)) * 0.5 + 1).to(hip_device)
    m, sd = ops.channel_stats(s)
    lab = torch.zeros((1, 12, 20), device=hip_device, dtype=torch.uint8)
    mix = torch.ones((1, 1, 1), device=hip_device)
    got = ops.adain_regions(c, lab, m.flatten(1), sd.flatten(1), mix, alpha=alpha, swap_style_stats=swap)
    a = RR.rel_inf(got, ops.adain_stats(c, m[0], sd[0], alpha=alpha, swap_style_stats=swap))
    b = RR.rel_inf(got, ops.adain(c, s, alpha=alpha, swap_style_stats=swap))
    print(f"degenerate alpha={alpha} swap={swap}: vs adain_stats {a:.2e}, vs adain {b:.2e}")
    assert a <= OP_TOL and b <= OP_TOL


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan_row", [False, True])
def test_interpolation_endpoint_is_exact(nan_row, hip_device):
    c, lab, _, _, _, k = _case(0)
    mean, std = RR.style_table(3501, 2, c.shape[1])
    one = _run(hip_device, c, lab, mean[:1], std[:1], torch.ones(1, k, 1), 0.3)
    if nan_row:
        mean[1], std[1] = float("nan"), float("nan")
    two = _run(hip_device, c, lab, mean, std, torch.tensor([[[1.0, 0.0]] * k]), 0.3)
    assert torch.isfinite(one).all()
    assert torch.equal(one, two)


# 5 ------------------------------------------------------------------------------------------------
def test_single_pixel_region_is_nan_in_kind(hip_device):
    c, lab, _, _, _, k = _case(1)
    lab = lab.clone()
    lab[0, 5, 7] = k                     # region k: exactly one pixel; region k + 1 never occurs
    mean, std = RR.style_table(3601, 3, c.shape[1])
    mix = RR.mix_weights(3602, 1, k + 2, 3)
    got = _run(hip_device, c, lab, mean, std, mix).cpu()
    ref = RR.adain_regions(c.double(), lab, mean.double(), std.double(), mix.double())
    nan = torch.zeros_like(c, dtype=torch.bool)
    nan[0, :, 5, 7] = True
    assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(ref), nan)
    err = float((got.double() - ref)[~nan].abs().max() / ref[~nan].abs().max())
    print(f"single-pixel region: rel_inf elsewhere {err:.2e}")
    assert err <= OP_TOL


# 6 ------------------------------------------------------------------------------------------------
def test_out_of_range_labels_pass_through(hip_device):
    c, lab, mean, std, mix, k = _case(0)
    assert k == 3
    lab = lab.clone()
    lab[0, 0, :4], lab[0, 8, 5:], lab[1, 3, 3], lab[1, 4:6, 0] = 9, 200, 255, 3
    got = _run(hip_device, c, lab, mean, std, mix, 0.3).cpu()
    ref = RR.adain_regions(c.double(), lab, mean.double(), std.double(), mix.double(), 0.3)
    _check(got, ref, lab, k, "labels 3, 9, 200, 255 with K = 3")
    keep = (lab >= k)[:, None].expand_as(c)
    assert set(lab[lab >= k].tolist()) == {3, 9, 200, 255} and torch.equal(got[keep], c[keep])


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 2])
def test_region_stats(idx, hip_device):
    c, lab, _, _, _, k = _case(idx)
    mean, std, count = (t.cpu() for t in ops.region_stats(c.to(hip_device), lab.to(hip_device), k))
    rm, rs, rc = RR.region_stats(c.double(), lab, k)
    em, es = RR.rel_inf(mean, rm), RR.rel_inf(std, rs)
    print(f"region_stats case {idx}: mean {em:.2e} std {es:.2e}")
    assert em <= OP_TOL and es <= OP_TOL
    assert count.dtype == torch.int32 and torch.equal(count, rc)


def test_region_stats_empty_and_single_pixel_regions(hip_device):
    c, lab, _, _, _, k = _case(0)
    lab = lab.clone()
    lab[1, 2, 2] = k + 1                 # sample 1: region k empty, region k + 1 one pixel; sample 0: both empty
    mean, std, count = (t.cpu() for t in ops.region_stats(c.to(hip_device), lab.to(hip_device), k + 2))
    rm, rs, rc = RR.region_stats(c.double(), lab, k + 2)
    assert torch.equal(count, rc) and count[:, k].tolist() == [0, 0] and count[:, k + 1].tolist() == [0, 1]
    assert torch.equal(torch.isnan(mean), torch.isnan(rm)) and torch.equal(torch.isnan(std), torch.isnan(rs))
    assert torch.isnan(mean[:, k]).all() and torch.isnan(std[:, k:]).all() and torch.isfinite(mean[1, k + 1]).all()
    assert torch.equal(mean[1, k + 1], c[1, :, 2, 2])
    fm, fs = ~torch.isnan(rm), ~torch.isnan(rs)
    em = float((mean.double() - rm)[fm].abs().max() / rm[fm].abs().max())
    es = float((std.double() - rs)[fs].abs().max() / rs[fs].abs().max())
    print(f"region_stats with empty regions: mean {em:.2e} std {es:.2e}")
    assert em <= OP_TOL and es <= OP_TOL


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("src,dst", RR.RESIZE_PAIRS)
def test_resize_labels(src, dst, n, hip_device):
    g = torch.Generator().manual_seed(src[0] * 1000 + src[1] + n)
    lab = torch.randint(0, 256, (n,) + src, dtype=torch.uint8, generator=g)
    got = ops.resize_labels(lab.to(hip_device), *dst)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), RR.resize_labels(lab, *dst))


# 9 ------------------------------------------------------------------------------------------------
def _offset_view(t, elems=1):
    buf = torch.empty(t.numel() + elems, device=t.device, dtype=t.dtype)
    view = buf[elems:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == elems
    return view


def test_unaligned_bases(hip_device):
    c, lab, mean, std, mix, k = (t.to(hip_device) if torch.is_tensor(t) else t for t in _case(OFFSET_CASE))
    n, ch, h, w = c.shape
    assert (h * w) % 4 == 0
    ref = ops.adain_regions(c, lab, mean, std, mix, alpha=0.3)
    cv = _offset_view(c)
    assert cv.data_ptr() % 16 != 0
    assert torch.equal(ops.adain_regions(cv, lab, mean, std, mix, alpha=0.3), ref)
    lv = _offset_view(lab)               # labels one byte off a 32-bit boundary
    assert lv.data_ptr() % 4 != 0
    assert torch.equal(ops.adain_regions(c, lv, mean, std, mix, alpha=0.3), ref)
    # content and output both one element off, through the C ABI (ops allocates an aligned output)
    ov = _offset_view(torch.zeros_like(c))
    _lib.check(_lib.lib().ast_adain_regions_f32(cv.data_ptr(), lab.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                                mix.data_ptr(), ov.data_ptr(), n, ch, h, w, k, mean.shape[0],
                                                k * mean.shape[0], 0.3, 1, _lib.stream_ptr(hip_device)),
               "adain_regions")
    assert torch.equal(ov, ref)
    rs = ops.region_stats(c, lab, k)
    for a, b in zip(ops.region_stats(cv, lv, k), rs):
        assert torch.equal(a, b)


# 10 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["case", "96x100"])
def test_run_to_run_determinism(which, hip_device):
    if which == "case":
        c, lab, mean, std, mix, k = _case(OFFSET_CASE)
    else:
        k = 8
        c, lab = RR.features(3701, (1, 2, 96, 100)), RR.label_map(1, 96, 100, k, seed=RR.LABEL_SEED)
        mean, std = RR.style_table(3702, 4, 2)
        mix = RR.mix_weights(3703, 1, k, 4)
    c, lab, mean, std, mix = (t.to(hip_device) for t in (c, lab, mean, std, mix))
    a = ops.adain_regions(c, lab, mean, std, mix, alpha=0.3)
    sa = ops.region_stats(c, lab, k)
    b = ops.adain_regions(c, lab, mean, std, mix, alpha=0.3)
    sb = ops.region_stats(c, lab, k)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)


# 11 -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_device):
    """The net, a content batch (N = 2) and two styles at 64x72 (relu4_1: 8x9), left / right content
    halves and top / bottom style halves as labels, and the features on the CPU in float64."""
    from arbitrarystyletransfer_amd import synth
    net = models.AdaINStyleTransfer(weights="live").to(hip_device)
    c = torch.from_numpy(synth.image(3801, (2, 3, 64, 72))).to(hip_device)
    s = torch.from_numpy(synth.image(3802, (2, 3, 64, 72))).to(hip_device)
    lab = torch.zeros((2, 64, 72), dtype=torch.uint8)
    lab[:, :, 36:] = 1
    slab = torch.zeros((2, 64, 72), dtype=torch.uint8)
    slab[:, 32:, :] = 1
    with torch.no_grad():
        f_c, f_s = net.encoder(c)[0], net.encoder(s)[0]
    assert tuple(f_c.shape[2:]) == (8, 9)
    return dict(net=net, c=c, s=s, lab=lab.to(hip_device), slab=slab.to(hip_device), f_c=f_c.cpu().double(),
                f_s=f_s.cpu().double(), lab_f=RR.resize_labels(lab, 8, 9), slab_f=RR.resize_labels(slab, 8, 9))


WEIGHTS = [[4.0, 1.0], [0.9, 2.1]]


def _decode(model, t):
    with torch.no_grad():
        return model["net"].decoder(t.float().to(model["c"].device))


@pytest.mark.parametrize("weights,alpha", [(None, 1.0), (WEIGHTS, 0.8)])
def test_model_regions_from_image_labels(model, weights, alpha):
    net = model["net"]
    with torch.no_grad():
        y = net.stylize_regions(model["c"], model["s"], labels=model["lab"], weights=weights, alpha=alpha)
    w = RR.normalise_weights(weights, 2, 2)
    ref = _decode(model, RR.stylize_features(model["f_c"], model["f_s"], model["lab_f"], w, alpha, True))
    err = RR.rel_inf(y, ref)
    print(f"model (a) weights={weights} alpha={alpha}: rel_inf {err:.2e}")
    assert y.shape == model["c"].shape and err <= OP_TOL * 10


def test_model_single_style_equals_stylize_with_stats(model):
    net = model["net"]
    with torch.no_grad():
        y = net.stylize_regions(model["c"], model["s"][:1], alpha=0.8)
        m, sd = net.style_statistics(model["s"][:1])
        ref = net.stylize_with_stats(model["c"], m[0], sd[0], alpha=0.8)
    err = RR.rel_inf(y, ref)
    print(f"model (b): rel_inf {err:.2e}")
    assert err <= OP_TOL * 10


def test_model_interpolation_without_labels(model):
    """labels=None, S = 2: one region with equal weights (and with given ones)."""
    net = model["net"]
    lab0 = torch.zeros((2, 8, 9), dtype=torch.uint8)
    for weights in (None, [[1.0, 3.0]]):
        with torch.no_grad():
            y = net.stylize_regions(model["c"], model["s"], weights=weights, alpha=0.8)
        w = RR.normalise_weights(weights, 2, 2, single_region=True)
        ref = _decode(model, RR.stylize_features(model["f_c"], model["f_s"], lab0, w, 0.8, True))
        err = RR.rel_inf(y, ref)
        print(f"model interpolation weights={weights}: rel_inf {err:.2e}")
        assert err <= OP_TOL * 10


def test_model_style_labels(model):
    net = model["net"]
    with torch.no_grad():
        y = net.stylize_regions(model["c"], model["s"], labels=model["lab"], weights=WEIGHTS, alpha=0.8,
                                style_labels=model["slab"])
    w = RR.normalise_weights(WEIGHTS, 2, 2)
    ref = _decode(model, RR.stylize_features(model["f_c"], model["f_s"], model["lab_f"], w, 0.8, True,
                                             style_labels=model["slab_f"]))
    err = RR.rel_inf(y, ref)
    print(f"model (c): rel_inf {err:.2e}")
    assert err <= OP_TOL * 10
    with torch.no_grad():
        plain = net.stylize_regions(model["c"], model["s"], labels=model["lab"], weights=WEIGHTS, alpha=0.8)
    assert not torch.equal(plain, y)


def test_model_canonical_selects_the_swap(model, hip_device):
    net = models.AdaINStyleTransfer(canonical=True, weights="live").to(hip_device)
    with torch.no_grad():
        y = net.stylize_regions(model["c"], model["s"], labels=model["lab"], weights=WEIGHTS)
    w = RR.normalise_weights(WEIGHTS, 2, 2)
    ref = _decode(model, RR.stylize_features(model["f_c"], model["f_s"], model["lab_f"], w, 1.0, False))
    err = RR.rel_inf(y, ref)
    print(f"model canonical: rel_inf {err:.2e}")
    assert err <= OP_TOL * 10


def test_model_preserve_color_feature_labels_and_grad(model):
    net = model["net"]
    kw = dict(weights=WEIGHTS, alpha=0.8)
    with torch.no_grad():
        plain = net.stylize_regions(model["c"], model["s"], labels=model["lab"], **kw)
        kept = net.stylize_regions(model["c"], model["s"], labels=model["lab"], preserve_color=True, **kw)
        assert torch.equal(kept, models._luma_transfer(plain, model["c"]))                       # (d)
        lab_f = ops.resize_labels(model["lab"], 8, 9)
        assert torch.equal(lab_f.cpu(), model["lab_f"])
        assert torch.equal(net.stylize_regions(model["c"], model["s"], labels=lab_f, **kw), plain)   # (e)
        one = net.stylize_regions(model["c"], model["s"], labels=model["lab"][0], **kw)           # [H, W] labels
        assert torch.equal(one, plain)
    assert any(p.requires_grad for p in net.parameters())
    with pytest.raises(NotImplementedError):                                                     # (f)
        net.stylize_regions(model["c"], model["s"], labels=model["lab"], **kw)


# 12 -----------------------------------------------------------------------------------------------
def test_registered_ops_equal_the_direct_calls(hip_device):
    from arbitrarystyletransfer_amd import library  # noqa: F401
    o = torch.ops.ast_hip
    c, lab, mean, std, mix, k = (t.to(hip_device) if torch.is_tensor(t) else t for t in _case(0))
    assert torch.equal(o.adain_regions(c, lab, mean, std, mix, 0.3, False),
                       ops.adain_regions(c, lab, mean, std, mix, alpha=0.3, swap_style_stats=False))
    for a, b in zip(o.region_stats(c, lab, k), ops.region_stats(c, lab, k)):
        assert a.dtype == b.dtype and not torch.isnan(b.float()).any() and torch.equal(a, b)
    big = RR.label_map(3, 64, 72, 5, seed=1).to(hip_device)
    assert torch.equal(o.resize_labels(big, 8, 9), ops.resize_labels(big, 8, 9))
