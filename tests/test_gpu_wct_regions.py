"""GPU: the regional whitening and colouring transform (csrc/wct.hip: the binning, the gathered
covariance, the mix, the regional apply GEMM) and its wrapper / registered-op / model surface, against
tests/wct_regions_ref.py.

Bars. The regional covariance is a single op and meets OP_TOL against float64. The whole op inherits the
conditioning of each region's covariance, which the fp32 iteration pays on any hardware; so, as in
test_gpu_wct.py, every valid region is held to min(max(4 * e_cpu, OP_TOL), FP32_BAR) with e_cpu the error
of the fp32 CPU emulation against the same float64 reference over that region's pixels
(test_wct_regions_cpu.py holds e_cpu to 2.5e-4 at eps_rel = 1e-3). Everything the definition fixes in
bits -- the statistics of a region against wct_cov of its gathered map, a one-hot region against wct of
the gathered map, the stages against the whole op, pass-through pixels -- is compared in bits. Every
test prints the numbers it asserts on."""
import functools
import gc

import pytest
import torch

import wct_ref as WR
import wct_regions_ref as RR
from arbitrarystyletransfer_amd import _lib, library, models, ops, synth  # noqa: F401  (library registers the ops)

pytestmark = pytest.mark.gpu

OP_TOL, FP32_BAR = WR.OP_TOL, WR.FP32_BAR
ALPHAS = (1.0, 0.6)


@functools.lru_cache(maxsize=None)
def _case(name):
    return RR.case_inputs(name)


def _on(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


@functools.lru_cache(maxsize=None)
def _ref(name, variant, alpha, eps_rel):
    """(float64 reference, valid [n, K], {(b, k): e_cpu of the fp32 emulation over region (b, k)})."""
    c, lab, s, slab = _case(name)
    mix = RR.case_mix(name, variant)
    ref, valid = RR.wct_regions(c, lab, s, mix, slab, alpha, eps_rel)
    emu, _ = RR.wct_regions_emulated(c, lab, s, mix, slab, alpha, eps_rel)
    return ref, valid, RR.region_errors(emu, ref, lab, valid)


def _bar(e_cpu):
    return min(max(4.0 * e_cpu, OP_TOL), FP32_BAR)


def _mismatches(got, ref):
    return int((got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)).sum())


def _run(name, variant, dev, alpha=0.6, eps_rel=1e-3):
    c, lab, s, slab = _on(dev, *_case(name))
    return ops.wct_regions(c, lab, s, RR.case_mix(name, variant).float().to(dev), slab, alpha=alpha, eps_rel=eps_rel)


# ---- regional covariance -----------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0.0, 30.0])
@pytest.mark.parametrize("name", list(RR.CASES))
def test_region_cov_against_float64_and_wct_cov(name, offset, hip_device):
    """Mean and covariance of every region against float64 (OP_TOL) and, in bits, against ops.wct_cov of
    the region's gathered map; exact counts; the identity and a zero mean for an invalid region."""
    x, lab = _case(name)[:2]
    x = x + offset
    n, c = x.shape[:2]
    k = RR.CASES[name]["k"]
    xd = x.to(hip_device)
    mean, cov, count = ops.wct_region_cov(xd, lab.to(hip_device), k)
    assert mean.shape == (n, k, c) and cov.shape == (n, k, c, c) and count.shape == (n, k) and count.dtype == torch.int32
    assert count.cpu().tolist() == [list(cnt) for cnt in RR.CASES[name]["counts"]]
    for b in range(n):
        for r in range(k):
            idx = RR.region_index(lab, b, r)
            if idx.numel() < 2:
                assert bool((mean[b, r] == 0).all()) and _mismatches(cov[b, r], torch.eye(c, device=hip_device)) == 0
                print(f"wct_region_cov {name} +{offset:g} region ({b}, {r}): {idx.numel()} pixels, mean 0 and cov I")
                continue
            ref_mu, ref_cov, _ = WR.mean_cov(x[b:b + 1][:, :, lab[b] == r], 1e-3)
            em, ec = WR.rel_inf(mean[b, r].cpu(), ref_mu[0]), WR.rel_inf(cov[b, r].cpu(), ref_cov[0])
            g_mu, g_cov = ops.wct_cov(xd[b:b + 1].flatten(2)[:, :, idx.to(hip_device)].contiguous(), 1e-3)
            bad = _mismatches(mean[b, r], g_mu[0]) + _mismatches(cov[b, r], g_cov[0])
            asym = _mismatches(cov[b, r], cov[b, r].T)
            print(f"wct_region_cov {name} +{offset:g} region ({b}, {r}), {idx.numel()} pixels: mean {em:.2e}, cov {ec:.2e} "
                  f"(bar {OP_TOL:.0e}); {bad} bits off wct_cov of the gathered map, {asym} asymmetric")
            assert em <= OP_TOL and ec <= OP_TOL and bad == 0 and asym == 0


def test_a_region_that_takes_more_splits_than_its_plane(hip_device):
    """24 x 24 = 576 pixels split 6 ways as a whole plane (chunks of 96), but a region of 449..512 pixels
    splits 8 ways (chunks of 64): the regional covariance must launch and reduce the region's own 8
    splits. Statistics in bits against ops.wct_cov of the gathered map and within OP_TOL of float64, for
    the first and the last region of the batch; the whole op with one-hot weights in bits against
    ops.wct of the gathered map."""
    n, c, hw, counts = 2, 40, (24, 24), [(500, 60), (100, 449)]
    x = WR.features(9801, (n, c) + hw)
    s = WR.features(9802, (2, c, 6, 6))
    lab = RR.scatter_labels(9803, hw, counts)
    xd, ld, sd = x.to(hip_device), lab.to(hip_device), s.to(hip_device)
    mean, cov, count = ops.wct_region_cov(xd, ld, 2)
    out = ops.wct_regions(xd, ld, sd, torch.eye(2, device=hip_device), alpha=0.6)
    assert count.cpu().tolist() == [list(cnt) for cnt in counts]
    for b in range(n):
        for r in range(2):
            idx = RR.region_index(lab, b, r).to(hip_device)
            g = xd[b:b + 1].flatten(2)[:, :, idx].contiguous()
            g_mu, g_cov = ops.wct_cov(g, 1e-3)
            bad = _mismatches(mean[b, r], g_mu[0]) + _mismatches(cov[b, r], g_cov[0])
            ref_mu, ref_cov, _ = WR.mean_cov(x[b:b + 1][:, :, lab[b] == r], 1e-3)
            em, ec = WR.rel_inf(mean[b, r].cpu(), ref_mu[0]), WR.rel_inf(cov[b, r].cpu(), ref_cov[0])
            bad_op = _mismatches(out[b].flatten(1)[:, idx], ops.wct(g.unsqueeze(2), sd[r:r + 1], alpha=0.6)[0, :, 0])
            print(f"576-pixel plane, region ({b}, {r}) of {idx.numel()} pixels: {bad} bits off wct_cov of the gathered "
                  f"map, mean {em:.2e}, cov {ec:.2e} vs float64 (bar {OP_TOL:.0e}); whole op {bad_op} bits off ops.wct")
            assert bad == 0 and em <= OP_TOL and ec <= OP_TOL and bad_op == 0


# ---- the whole op against float64 -----------------------------------------------------------------------

@pytest.mark.parametrize("eps_rel", [1e-3, 1e-4])
@pytest.mark.parametrize("name,variant", RR.variants())
def test_regions_against_float64(name, variant, eps_rel, hip_device):
    c, lab = _case(name)[:2]
    res = []
    for alpha in ALPHAS:
        ref, valid, e_cpu = _ref(name, variant, alpha, eps_rel)
        got = _run(name, variant, hip_device, alpha, eps_rel).cpu()
        assert got.shape == c.shape
        keep = RR.passthrough_mask(lab, valid)[:, None].expand_as(c)
        through = _mismatches(got[keep], c[keep])
        for key, err in RR.region_errors(got, ref, lab, valid).items():
            print(f"wct_regions {name}/{variant} eps_rel={eps_rel:g} alpha={alpha} region {key}: gpu {err:.2e}, "
                  f"e_cpu {e_cpu[key]:.2e}, bar {_bar(e_cpu[key]):.2e}")
            res.append((err, _bar(e_cpu[key])))
        print(f"wct_regions {name}/{variant} eps_rel={eps_rel:g} alpha={alpha}: valid {valid.tolist()}, "
              f"{int(keep.sum())} pass-through values, {through} differ from the content")
        assert through == 0
    assert res and all(err <= bar for err, bar in res), res


# ---- what the definition fixes in bits ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["c8_odd_planes", "c48_two_splits", "c32_small_regions"])
def test_one_hot_region_is_wct_of_the_gathered_map(name, hip_device):
    """With one-hot weights region k equals ops.wct on the region's pixels as a [1, C, 1, M_k] map and
    style k, bit for bit: a column depends only on T_k and its own channels, not on the tile it is in."""
    c, lab, s, _ = _case(name)
    cd, sd = c.to(hip_device), s.to(hip_device)
    out = _run(name, "eye", hip_device, 0.6)
    bad = {}
    for b in range(c.shape[0]):
        for k in range(RR.CASES[name]["k"]):
            idx = RR.region_index(lab, b, k).to(hip_device)
            if idx.numel() < 2:
                continue
            g = cd[b:b + 1].flatten(2)[:, :, idx].unsqueeze(2).contiguous()
            bad[(b, k)] = _mismatches(out[b].flatten(1)[:, idx], ops.wct(g, sd[k:k + 1], alpha=0.6)[0, :, 0])
    print(f"one-hot regions vs ops.wct of the gathered maps, {name}: mismatches {bad}")
    assert bad and not any(bad.values())


def test_one_region_one_style_is_wct(hip_device):
    c, _, s, _ = _on(hip_device, *_case("c64_mixes"))
    lab = torch.zeros((c.shape[0],) + tuple(c.shape[2:]), device=hip_device, dtype=torch.uint8)
    got = ops.wct_regions(c, lab, s[:1], torch.ones(1, 1, 1, device=hip_device), alpha=0.6)
    bad = _mismatches(got, ops.wct(c, s[:1], alpha=0.6))
    print(f"K = 1, S = 1 vs ops.wct with a shared style: {bad} mismatches")
    assert bad == 0


@pytest.mark.parametrize("name,variant", [("c48_two_splits", "eye"), ("c64_mixes", "per_sample"),
                                          ("c160_style_labels", "absent_unused"), ("c160_style_labels", "absent_used")])
def test_stages_compose_to_the_whole_op(name, variant, hip_device):
    """ast_wct_regions_f32 is ast_wct_region_cov_f32, ast_wct_cov_f32 (or the regional one with style
    labels), ast_wct_sqrt_f32 on all the matrices and ast_wct_region_apply_f32, bit for bit."""
    c, lab, s, slab = _on(hip_device, *_case(name))
    mix = RR.case_mix(name, variant).float().to(hip_device)
    n, ch, k = c.shape[0], c.shape[1], mix.shape[1]
    whole = ops.wct_regions(c, lab, s, mix, slab, alpha=0.6, eps_rel=1e-4)
    mu_c, cov_c, _ = ops.wct_region_cov(c, lab, k, 1e-4)
    if slab is None:
        (mu_s, cov_s), scount = ops.wct_cov(s, 1e-4), None
    else:
        mu_s, cov_s, scount = ops.wct_region_cov(s, slab, k, 1e-4)
    root, iroot = ops.wct_sqrt(torch.cat([cov_c.reshape(-1, ch, ch), cov_s.reshape(-1, ch, ch)]), eps_rel=1e-4)
    out = ops.wct_region_apply(c, lab, mu_c, iroot[:n * k].reshape(n, k, ch, ch).contiguous(), mu_s,
                               root[n * k:].reshape(cov_s.shape).contiguous(), mix, scount, alpha=0.6)
    bad = _mismatches(out, whole)
    print(f"stages vs whole op, {name}/{variant}: {bad} mismatches")
    assert bad == 0


def test_registered_op_matches_and_has_no_backward(hip_device):
    for name, variant in (("c64_mixes", "shared"), ("c160_style_labels", "absent_used")):
        c, lab, s, slab = _on(hip_device, *_case(name))
        mix = RR.case_mix(name, variant).float().to(hip_device)
        bad = _mismatches(torch.ops.ast_hip.wct_regions(c, lab, s, mix, slab, 0.6, 1e-3, 0), _run(name, variant, hip_device))
        print(f"torch.ops.ast_hip.wct_regions vs ops.wct_regions, {name}: {bad} mismatches")
        assert bad == 0
    with pytest.raises(NotImplementedError):
        torch.ops.ast_hip.wct_regions(c.clone().requires_grad_(), lab, s, mix, slab, 0.6, 1e-3, 0).sum().backward()


@pytest.mark.parametrize("name,variant", [("c48_two_splits", "eye"), ("c160_style_labels", "absent_unused")])
def test_run_twice_bitwise(name, variant, hip_device):
    bad = _mismatches(_run(name, variant, hip_device), _run(name, variant, hip_device))
    print(f"run to run, {name}: {bad} mismatches")
    assert bad == 0


def test_replays_from_a_hip_graph_with_other_labels(hip_device):
    """One ops.wct_regions call captured on a single stream with one label map and replayed with another
    of the same shape (other region sizes, a one-pixel region): the eager result's bits, so no launch
    parameter depended on the labels."""
    name = "c48_two_splits"
    c, lab, s, _ = _case(name)
    lab2 = RR.scatter_labels(9901, RR.CASES[name]["hw"], [(30, 40, 20), (1, 90, 5)])
    mix = RR.case_mix(name, "eye").float().to(hip_device)
    cd, sd = c.to(hip_device), s.to(hip_device)
    eager = [ops.wct_regions(cd, l.to(hip_device), sd, mix, alpha=0.6) for l in (lab, lab2)]
    sl = lab.to(hip_device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            out = ops.wct_regions(cd, sl, sd, mix, alpha=0.6)
    finally:
        gc.enable()
    bad = []
    for l, ref in zip((lab, lab2, lab), eager + eager[:1]):
        sl.copy_(l)
        g.replay()
        torch.cuda.synchronize()
        bad.append(_mismatches(out, ref))
    differ = _mismatches(eager[0], eager[1])
    print(f"graph replays vs eager: {bad} mismatches; the two label maps' results differ in {differ} values")
    assert bad == [0, 0, 0] and differ > 0


def test_all_pass_through_labels_return_the_content(hip_device):
    c, lab, s, _ = _on(hip_device, *_case("c48_two_splits"))
    mix = RR.case_mix("c48_two_splits", "eye").float().to(hip_device)
    out = ops.wct_regions(c, torch.full_like(lab, 255), s, mix, alpha=0.6)
    bad = _mismatches(out, c)
    print(f"all-255 labels vs the content: {bad} mismatches")
    assert bad == 0


def test_a_zero_weight_style_is_never_read(hip_device):
    c, lab, s, _ = _on(hip_device, *_case("c8_odd_planes"))
    s_nan = s.clone()
    s_nan[1] = float("nan")
    w = torch.tensor([[[1.0, 0.0], [1.0, 0.0]]], device=hip_device)
    got = ops.wct_regions(c, lab, s_nan, w, alpha=0.6)
    one = ops.wct_regions(c, lab, s[:1], w[:, :, :1].contiguous(), alpha=0.6)
    bad = _mismatches(got, one)
    print(f"weights [1, 0] with NaN in style 1 vs the one-style call: {bad} mismatches, finite {bool(torch.isfinite(got).all())}")
    assert bad == 0 and bool(torch.isfinite(got).all())


def test_a_nan_stays_in_its_region(hip_device):
    name = "c64_mixes"
    c, lab, s, _ = _case(name)
    clean = _run(name, "shared", hip_device)
    pix = int(RR.region_index(lab, 0, 0)[3])
    poisoned = c.clone()
    poisoned.flatten(2)[0, 5, pix] = float("nan")
    out = ops.wct_regions(poisoned.to(hip_device), lab.to(hip_device), s.to(hip_device),
                          RR.case_mix(name, "shared").float().to(hip_device), alpha=0.6)
    other = (lab[0] != 0).to(hip_device)
    bad0 = _mismatches(out[0][:, other], clean[0][:, other])
    bad1 = _mismatches(out[1], clean[1])
    hit = not bool(torch.isfinite(out[0][:, ~other]).all())
    print(f"NaN in region 0 of sample 0: the rest of sample 0 differs in {bad0} values, sample 1 in {bad1}; region 0 hit: {hit}")
    assert bad0 == 0 and bad1 == 0 and hit


def test_wrappers_reject_bad_inputs(hip_device):
    c, lab, s, _ = _on(hip_device, *_case("c8_odd_planes"))
    mix = torch.eye(2, device=hip_device)
    with pytest.raises(_lib.HipOpError, match="float32"):
        ops.wct_regions(c.double(), lab, s, mix)
    with pytest.raises(_lib.HipOpError, match="mix must be"):
        ops.wct_regions(c, lab, s, torch.ones(2, 3, device=hip_device))
    with pytest.raises(_lib.HipOpError, match="style bank"):
        ops.wct_regions(c, lab, s[:, :4], mix)
    with pytest.raises(_lib.HipOpError, match="style_labels must be"):
        ops.wct_regions(c, lab, s, mix, style_labels=lab)
    with pytest.raises(_lib.HipOpError, match="unsupported"):
        ops.wct_regions(c, lab, s, mix, eps_rel=1e-5)
    with pytest.raises(_lib.HipOpError, match="bad shape"):
        ops.wct_regions(c, lab, s[:, :, :1, :1], mix)


# ---- model ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets(hip_device):
    return {t: models.AdaINStyleTransfer(transform=t).to(hip_device).eval() for t in ("adain", "wct")}


@pytest.fixture(scope="module")
def imgs(hip_device):
    """32 x 32 images (a 4 x 4 relu4_1 map), two styles, an irregular label map at image resolution."""
    c = torch.from_numpy(synth.image(9701, (1, 3, 32, 32))).to(hip_device)
    s = torch.from_numpy(synth.image(9702, (2, 3, 32, 32))).to(hip_device)
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    lab = ((yy + 2 * xx) % 32 < 14).to(torch.uint8)
    lab[(yy - 12) ** 2 + (xx - 20) ** 2 < 40] = 255   # 4 of the 16 feature pixels; 6 in each region
    return c, s, lab.unsqueeze(0).to(hip_device)


def test_model_stylize_regions_wct(nets, imgs):
    c, s, lab = imgs
    net = nets["wct"]
    with torch.no_grad():
        f_c, f_s = net.encoder(c)[0], net.encoder(s)[0]
        fl = ops.resize_labels(lab, 4, 4)
        eye = torch.eye(2, device=c.device).unsqueeze(0)
        bad = [_mismatches(net.stylize_regions_wct(c, s, lab, alpha=a), net.decoder(ops.wct_regions(f_c, fl, f_s, eye, alpha=a)))
               for a in ALPHAS]
        w = [[0.25, 0.75]]
        interp = net.stylize_regions_wct(c, s, weights=w)
        bad.append(_mismatches(interp, net.decoder(ops.wct_regions(
            f_c, torch.zeros_like(fl), f_s, torch.tensor([w], device=c.device)))))
        bad.append(_mismatches(net.stylize_regions_wct(c, s, fl), net.stylize_regions_wct(c, s, lab)))
        y = net.stylize_regions_wct(c, s, lab, style_labels=lab.expand(2, -1, -1))
        other = _mismatches(nets["adain"].stylize_regions_wct(c, s, lab), net.stylize_regions_wct(c, s, lab))
        yc = net.stylize_regions_wct(c, s, lab, preserve_color=True)
        plain = net.stylize_regions_wct(c, s, lab)
        t = ops.wct_regions(f_c, fl, f_s, eye).cpu()
        ref, valid = RR.wct_regions(f_c.cpu(), fl.cpu(), f_s.cpu(), eye.cpu().double())
        errs = RR.region_errors(t, ref, fl.cpu(), valid)
    print(f"model vs decoder(ops.wct_regions(...)): {bad} mismatches; relu4_1 map {tuple(f_c.shape)}, labels "
          f"{fl.cpu().flatten().tolist()}; adain-built model differs in {other} values; transform vs float64 {errs}")
    assert tuple(f_c.shape) == (1, 512, 4, 4) and bad == [0, 0, 0, 0] and other == 0
    assert y.shape == c.shape and bool(torch.isfinite(y).all()) and bool(torch.isfinite(interp).all())
    assert errs and all(e <= FP32_BAR for e in errs.values())
    assert yc.shape == c.shape and _mismatches(yc, ops.luma_transfer(plain, c)) == 0


def test_model_compile_fullgraph_bit_identical(nets, imgs):
    torch._dynamo.reset()
    c, s, lab = imgs
    net = nets["wct"]
    with torch.no_grad():
        ref = net.stylize_regions_wct(c, s, lab, None, 0.8)
        cm = torch.compile(net.stylize_regions_wct, fullgraph=True, dynamic=False)
        out = cm(c, s, lab, None, 0.8)
        out2 = cm(c, s, lab, None, 0.8)
    torch.cuda.synchronize()
    bad = _mismatches(out, ref) + _mismatches(out2, ref)
    print(f"compiled stylize_regions_wct vs eager: {bad} mismatches")
    assert bad == 0


def test_model_raises_under_grad(nets, imgs):
    c, s, lab = imgs
    with pytest.raises(NotImplementedError):
        nets["wct"].stylize_regions_wct(c.clone().requires_grad_(), s, lab)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        nets["wct"].stylize_regions(c, s, lab)
