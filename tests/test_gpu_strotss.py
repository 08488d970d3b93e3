"""GPU: the optimisation-based stylizer (arbitrarystyletransfer_amd/strotss.py) on a 64x48 content and an
80x64 style, scales (32, 64), three pyramid levels, the live-init loss network."""
import pytest
import torch
import torch.nn.functional as F

import lap_ref as LR
from arbitrarystyletransfer_amd import _lib, models, ops, strotss, synth
from arbitrarystyletransfer_amd import functional as Fn
from moment_ref import OP_TOL, rel_inf

pytestmark = pytest.mark.gpu

SCALES = (32, 64)
KW = dict(scales=SCALES, levels=3)
_CACHE = {}


def _setup(dev):
    if "st" not in _CACHE:
        _CACHE["c"] = torch.from_numpy(synth.image(5001, (1, 3, 64, 48)))
        _CACHE["s"] = torch.from_numpy(synth.image(5002, (1, 3, 80, 64)))
        _CACHE["st"] = strotss.StrotssStylizer(device=dev)
    return _CACHE["st"], _CACHE["c"].to(dev), _CACHE["s"].to(dev)


def _run(dev, key, **kw):
    """A stylize() result computed once per distinct call and left unchanged."""
    if key not in _CACHE:
        st, c, s = _setup(dev)
        _CACHE[key] = st.stylize(c, s, **{**KW, **kw})
    return _CACHE[key]


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def test_start_image_follows_the_initialisation_rule(hip_device):
    """iters = 0 returns the start image: content_s - resize(down(content_s)) + the style's mean colour at
    the first scale, within the resize bars of lap_ref: each resize adds its bar to the error it inherits
    (the content's twice: directly and through up(down())); the mean of 1024 values in [0, 1] is a tree sum
    of log2(1024) = 10 roundings, the division and the final add three more, of values below 2."""
    st, c, s = _setup(hip_device)
    got = st.stylize(c, s, scales=(32,), levels=3, iters=0)
    c64, s64 = _CACHE["c"].double(), _CACHE["s"].double()
    c_s, s_s = LR.interp(c64, (32, 32)), LR.interp(s64, (32, 32))
    want = LR.build(c_s, 1)[0] + s_s.mean(dim=(2, 3), keepdim=True)
    e_cs = LR.resize_bar(c64)
    bar = 2 * e_cs + LR.build_bars(c_s, 1)[0] + LR.resize_bar(s64) + 2 * 13 * LR.EPS
    err = float((got.double().cpu() - want).abs().max())
    print(f"start image: {err:.2e} (bar {bar:.2e})")
    assert got.shape == (1, 3, 32, 32) and err <= bar
    # later scales start from the previous result, resized
    both = st.stylize(c, s, iters=0, **KW)
    assert _same(both, ops.resize_bilinear(got, (64, 48)))


def test_init_is_resized_to_the_first_scale(hip_device):
    st, c, s = _setup(hip_device)
    init = torch.from_numpy(synth.image(5003, (1, 3, 40, 56))).to(hip_device)
    got = st.stylize(c, s, init=init, scales=(32,), levels=3, iters=0)
    want = LR.interp(init.double().cpu(), (32, 32))
    assert float((got.double().cpu() - want).abs().max()) <= LR.resize_bar(init.double().cpu())
    assert _same(got, ops.resize_bilinear(init, (32, 32)))


def test_leaf_gradients_match_autograd_through_interpolate(hip_device):
    """One eager iteration's gradient on every pyramid level against PyTorch autograd with F.interpolate
    on the GPU in LapCollapseFn's place, same loss network and losses. The reference image is shifted onto
    the kernels' image (a + (b - a).detach()), so that both see the same signs in the L1 terms and only
    the collapse's backward differs."""
    st, c, s = _setup(hip_device)
    size = (64, 48)
    c_s, s_s = ops.resize_bilinear(c, size), ops.resize_bilinear(s, strotss.scale_size(s.shape[2:], 64))
    cfg = dict(alpha=8.0, remd_lam=1.0, moment_lam=1.0, selfsim_idx=[4, 6], remd_idx=[4, 6], moment_idx=[4, 6])
    targets = st._targets(c_s, s_s, cfg)
    start = ops.lap_build(c_s, 1)[0] + s_s.mean(dim=(2, 3), keepdim=True)
    pyr = ops.lap_build(start, 3)
    assert [tuple(p.shape[-2:]) for p in pyr] == [(64, 48), (32, 24), (16, 12), (8, 6)]
    leaves = [p.clone().requires_grad_(True) for p in pyr]
    img = Fn.LapCollapseFn.apply(*leaves)
    with _lib.accumulator_pool():
        st._objective(img, targets, cfg)["objective"].backward()
    ref = [p.clone().requires_grad_(True) for p in pyr]
    cur = ref[-1]
    for lvl in reversed(ref[:-1]):
        cur = lvl + F.interpolate(cur, size=lvl.shape[-2:], mode="bilinear", align_corners=False)
    cur = cur + (img.detach() - cur.detach())
    with _lib.accumulator_pool():
        st._objective(cur, targets, cfg)["objective"].backward()
    for l, (a, b) in enumerate(zip(leaves, ref)):
        err = rel_inf(a.grad.cpu(), b.grad.cpu())
        print(f"level {l}: leaf gradient rel_inf {err:.2e}")
        assert float(b.grad.abs().max()) > 0 and err <= OP_TOL


def test_graph_and_eager_give_the_same_image_in_bits(hip_device):
    a = _run(hip_device, "graph3", iters=3, graph=True, return_history=True)[0]
    b = _run(hip_device, "eager3", iters=3, graph=False)
    assert a.shape == (1, 3, 64, 48) and bool(torch.isfinite(a).all())
    assert _same(a, b)
    st, c, s = _setup(hip_device)
    assert not _same(a, st.stylize(c, s, iters=0, **KW))   # the iterations did move the image


def test_two_runs_agree_in_bits(hip_device):
    a, ha = _run(hip_device, "graph3", iters=3, graph=True, return_history=True)
    st, c, s = _setup(hip_device)
    b, hb = st.stylize(c, s, iters=3, graph=True, return_history=True, **KW)
    assert _same(a, b)
    for x, y in zip(ha, hb):
        assert x["size"] == y["size"]
        assert all(_same(x[w][k].reshape(1), y[w][k].reshape(1)) for w in ("before", "after") for k in x[w])


def test_history_reports_the_terms_that_run(hip_device):
    _, hist = _run(hip_device, "graph3", iters=3, graph=True, return_history=True)
    assert [h["size"] for h in hist] == [(32, 32), (64, 48)]
    for h in hist:
        assert set(h["before"]) == set(h["after"]) == {"objective", "selfsim", "remd", "moment"}
        assert all(v.device.type == "cuda" and v.dim() == 0 for v in h["before"].values())
    st, c, s = _setup(hip_device)
    _, only = st.stylize(c, s, iters=1, content_weight=0.0, moment_lam=0.0, return_history=True, **KW)
    assert all(set(h["before"]) == set(h["after"]) == {"objective", "remd"} for h in only)
    assert all(_same(h["before"]["objective"].reshape(1), h["before"]["remd"].reshape(1)) for h in only)
    _, two = st.stylize(c, s, iters=1, remd_lam=0.0, graph=False, return_history=True, **KW)
    assert all(set(h["before"]) == {"objective", "selfsim", "moment"} for h in two)
    with pytest.raises(ValueError):
        st.stylize(c, s, iters=1, content_weight=0.0, remd_lam=0.0, moment_lam=0.0, **KW)


def test_objective_falls_at_every_scale(hip_device):
    """A sanity condition at the default lr: after 20 iterations the objective of each scale is below the
    one before its first."""
    img, hist = _run(hip_device, "graph20", iters=20, graph=True, return_history=True)
    vals = [(h["size"], float(h["before"]["objective"]), float(h["after"]["objective"])) for h in hist]   # read once
    for size, before, after in vals:
        print(f"scale {size}: objective {before:.6f} -> {after:.6f}")
    assert bool(torch.isfinite(img).all())
    assert all(after < before for _, before, after in vals)


def test_refine_equals_the_explicit_init(hip_device):
    st, c, s = _setup(hip_device)
    torch.manual_seed(77)
    net = models.AdaINStyleTransfer().to(hip_device).eval()
    got = net.refine(c, s, st, iters=2, **KW)
    with torch.no_grad():
        init = net(c, s)
    want = st.stylize(c, s, init=init, iters=2, **KW)
    assert _same(got, want)
    assert not _same(got, _run(hip_device, "graph2", iters=2))   # and the init is used


def test_batches_run_image_by_image(hip_device):
    st, c, s = _setup(hip_device)
    c2 = torch.cat([c, c.flip(3)])
    out = st.stylize(c2, s, iters=1, **KW)
    assert out.shape == (2, 3, 64, 48)
    assert _same(out[:1], st.stylize(c, s, iters=1, **KW)) and _same(out[1:], st.stylize(c.flip(3), s, iters=1, **KW))


def test_over_limit_scale_raises_before_any_launch(hip_device):
    st, c, s = _setup(hip_device)
    big = torch.empty((1, 3, 2048, 2048), device=hip_device)
    with ops.LaunchTimer() as timer:
        with pytest.raises(_lib.HipOpError, match="self-similarity tap relu_9"):
            st.stylize(big, s, scales=(64, 2048), iters=1)
        assert not timer.records                              # nothing was launched, not even the first resize
        st.stylize(big, s, scales=(64,), iters=0)             # within the limits the timer does see the resizes
        assert any("resize" in r[0] for r in timer.records)
    with pytest.raises(_lib.HipOpError):
        st.stylize(c[0], s)
    with pytest.raises(ValueError):
        st.stylize(c, s, remd_taps=("relu_99",))
