"""GPU: the bilinear resize, its adjoint and the Laplacian pyramid of csrc/pyramid.hip against
float64 F.interpolate (tests/lap_ref.py, where every bar is derived)."""
import pytest
import torch

import lap_ref as LR
from arbitrarystyletransfer_amd import functional as Fn
from arbitrarystyletransfer_amd import library, ops  # noqa: F401  (library registers the ops)

pytestmark = pytest.mark.gpu

ALL_CASES = LR.CASES + [LR.BIG]
_IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in ALL_CASES]
_CACHE = {}


def _case(src, dst):
    """Inputs and float64 references of one size pair, computed once and left unchanged."""
    key = (src, dst)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(1000 + 7 * src[0] + dst[1])
        x = torch.rand((3,) + src, generator=gen)
        add = torch.randn((3,) + dst, generator=gen)
        g = torch.randn((3,) + dst, generator=gen)
        _CACHE[key] = dict(x=x, add=add, g=g, y64=LR.interp(x, dst), yk64=LR.resize_ref(x, dst),
                           a64=LR.adjoint(g, src), ak64=LR.adjoint_ref(g, src))
    return _CACHE[key]


def _err(got, want):
    return float((got.detach().double().cpu() - want).abs().max())


@pytest.mark.parametrize("src,dst", ALL_CASES, ids=_IDS)
def test_resize_matches_interpolate(hip_device, src, dst):
    c = _case(src, dst)
    x, add = c["x"].to(hip_device), c["add"].to(hip_device)
    xmax, addmax = float(c["x"].abs().max()), float(c["add"].abs().max())
    y = ops.resize_bilinear(x, dst)
    assert y.shape == (3,) + dst and y.dtype == torch.float32
    err, tight = _err(y, c["y64"]), _err(y, c["yk64"])
    print(f"resize {src}->{dst}: vs F.interpolate {err:.2e} (bar {LR.resize_bar(c['x']):.2e}), "
          f"vs the fp32-coordinate statement {tight:.2e} (bar {LR.arith_bar(xmax):.2e})")
    assert err <= LR.resize_bar(c["x"])
    assert tight <= LR.arith_bar(xmax)
    for sign in (1.0, -1.0):
        z = ops.resize_bilinear(x, dst, add=add, sign=sign)
        want, wantk = c["add"].double() + sign * c["y64"], c["add"].double() + sign * c["yk64"]
        assert _err(z, want) <= LR.resize_bar(c["x"], addmax)
        assert _err(z, wantk) <= LR.arith_bar(xmax, addmax)


@pytest.mark.parametrize("src,dst", ALL_CASES, ids=_IDS)
def test_adjoint_matches_autograd(hip_device, src, dst):
    c = _case(src, dst)
    g = c["g"].to(hip_device)
    gmax = float(c["g"].abs().max())
    a = ops.resize_bilinear_adjoint(g, src)
    assert a.shape == (3,) + src and a.dtype == torch.float32
    err, tight = _err(a, c["a64"]), _err(a, c["ak64"])
    bar, tbar = LR.adjoint_bar(gmax, src, dst), LR.adjoint_arith_bar(gmax, src, dst)
    print(f"adjoint {dst}->{src}: vs autograd {err:.2e} (bar {bar:.2e}), vs the fp32-coordinate statement "
          f"{tight:.2e} (bar {tbar:.2e})")
    assert err <= bar
    assert tight <= tbar
    # accumulate: out += R^T g, one more rounding of |out| + |R^T g|
    base = torch.randn((3,) + src, generator=torch.Generator().manual_seed(5))
    out = base.to(hip_device)
    assert ops.resize_bilinear_adjoint(g, src, out=out) is out
    slack = 2 * LR.EPS * float((base.double().abs() + c["ak64"].abs()).max())
    assert _err(out, base.double() + c["ak64"]) <= tbar + slack


@pytest.mark.parametrize("src,dst", ALL_CASES, ids=_IDS)
def test_adjoint_identity_on_the_gpu_outputs(hip_device, src, dst):
    """<resize(c), g> = <c, adjoint(g)> with both sides from the kernels' own outputs, summed in
    float64: they differ by the kernels' arithmetic rounding only (the coordinates are shared)."""
    c = _case(src, dst)
    x64, g64 = c["x"].double(), c["g"].double()
    y = ops.resize_bilinear(c["x"].to(hip_device), dst).double().cpu()
    a = ops.resize_bilinear_adjoint(c["g"].to(hip_device), src).double().cpu()
    lhs, rhs = float((y * g64).sum()), float((x64 * a).sum())
    bar = (float(g64.abs().sum()) * LR.arith_bar(float(x64.abs().max()))
           + float(x64.abs().sum()) * LR.adjoint_arith_bar(float(g64.abs().max()), src, dst))
    print(f"adjoint identity {src}->{dst}: {lhs:.9e} vs {rhs:.9e}, bar {bar:.2e}")
    assert abs(lhs - rhs) <= bar


def test_nonfinite_gradient_stays_with_its_source_pixels(hip_device):
    src, dst = (18, 25), (37, 50)
    g = _case(src, dst)["g"].clone()
    g[1, 20, 30] = float("nan")
    a = ops.resize_bilinear_adjoint(g.to(hip_device), src).cpu()
    clean = ops.resize_bilinear_adjoint(_case(src, dst)["g"].to(hip_device), src).cpu()
    bad = torch.isnan(a)
    y0, y1, _ = LR.src_map(dst[0], src[0])
    x0, x1, _ = LR.src_map(dst[1], src[1])
    want = torch.zeros_like(bad)
    for yy in {int(y0[20]), int(y1[20])}:
        for xx in {int(x0[30]), int(x1[30])}:
            want[1, yy, xx] = True
    assert torch.equal(bad, want)
    assert torch.equal(a[~bad], clean[~bad])


def test_lap_build_sizes_and_values(hip_device):
    x = LR.image(21, (2, 3, 37, 50))
    ref = LR.build(x, 4)
    assert [tuple(p.shape[-2:]) for p in ref] == [(37, 50), (18, 25), (9, 12), (4, 6), (2, 3)]   # on the CPU
    pyr = ops.lap_build(x.to(hip_device), 4)
    assert [tuple(p.shape) for p in pyr] == [tuple(p.shape) for p in ref]
    for l, (got, want, bar) in enumerate(zip(pyr, ref, LR.build_bars(x, 4))):
        err = _err(got, want)
        print(f"lap_build level {l}: {err:.2e} (bar {bar:.2e})")
        assert err <= bar
    assert len(ops.lap_build(x.to(hip_device), 0)) == 1


@pytest.mark.parametrize("shape,levels", [((2, 3, 37, 50), 4), ((1, 3, 64, 48), 3), ((3, 512, 512), 5), ((1, 1, 1, 3), 2)])
def test_collapse_of_build_returns_the_image(hip_device, shape, levels):
    """Within 4 ulp of max|x| per level: a level stores cur - up and the collapse adds the same up
    (the coarser image is rebuilt to rounding), so each level leaves a few roundings of max|x|."""
    x = LR.image(22, shape)
    back = ops.lap_collapse(ops.lap_build(x.to(hip_device), levels))
    err = _err(back, x.double())
    bar = 4 * levels * 2.0 ** -23 * float(x.abs().max())
    print(f"collapse(build) {shape} {levels} levels: {err:.2e} (bar {bar:.2e})")
    assert back.shape == x.shape and err <= bar


def test_collapse_fn_gradients_reach_every_level(hip_device):
    x = LR.image(23, (2, 3, 37, 50))
    pyr32 = [p.float() for p in LR.build(x, 4)]   # fp32 leaves: both sides start from the same values
    ref = [p.double().requires_grad_(True) for p in pyr32]
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(24))
    out64 = LR.collapse(ref)
    out64.backward(g.double())
    leaves = [p.to(hip_device).requires_grad_(True) for p in pyr32]
    out = Fn.LapCollapseFn.apply(*leaves)
    assert _err(out, out64.detach()) <= LR.collapse_bar(pyr32)
    out.backward(g.to(hip_device))
    bars = LR.collapse_grad_bars([tuple(p.shape[-2:]) for p in ref], g)
    for l, (leaf, want, bar) in enumerate(zip(leaves, ref, bars)):
        err = _err(leaf.grad, want.grad)
        print(f"LapCollapseFn grad level {l}: {err:.2e} (bar {bar:.2e})")
        assert leaf.grad.shape == leaf.shape and err <= bar
    assert torch.equal(leaves[0].grad, g.to(hip_device))


def test_resize_fn_gradients(hip_device):
    src, dst = (18, 25), (37, 50)
    c = _case(src, dst)
    x = c["x"].to(hip_device).requires_grad_(True)
    add = c["add"].to(hip_device).requires_grad_(True)
    torch.ops.ast_hip.resize_bilinear(x, dst[0], dst[1], add, -1.0).backward(c["g"].to(hip_device))
    gmax = float(c["g"].abs().max())
    assert _err(x.grad, -c["ak64"]) <= LR.adjoint_arith_bar(gmax, src, dst)
    assert torch.equal(add.grad, c["g"].to(hip_device))
    x2 = c["x"].to(hip_device).requires_grad_(True)
    torch.ops.ast_hip.resize_bilinear(x2, dst[0], dst[1], None, 1.0).backward(c["g"].to(hip_device))
    assert torch.equal(x2.grad, ops.resize_bilinear_adjoint(c["g"].to(hip_device), src))


def test_two_runs_agree_in_bits(hip_device):
    for src, dst in ALL_CASES:
        c = _case(src, dst)
        x, add, g = (c[k].to(hip_device) for k in ("x", "add", "g"))
        assert torch.equal(ops.resize_bilinear(x, dst, add=add, sign=-1.0), ops.resize_bilinear(x, dst, add=add, sign=-1.0))
        assert torch.equal(ops.resize_bilinear_adjoint(g, src), ops.resize_bilinear_adjoint(g, src))
    x = LR.image(25, (1, 3, 64, 48)).to(hip_device)
    p1, p2 = ops.lap_build(x, 3), ops.lap_build(x, 3)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))
    assert torch.equal(ops.lap_collapse(p1), ops.lap_collapse(p2))


def test_custom_op_equals_the_ctypes_path(hip_device):
    src, dst = (18, 25), (37, 50)
    c = _case(src, dst)
    x, add, g = (c[k].to(hip_device) for k in ("x", "add", "g"))
    A = torch.ops.ast_hip
    assert torch.equal(A.resize_bilinear(x, dst[0], dst[1], None, 1.0), ops.resize_bilinear(x, dst))
    assert torch.equal(A.resize_bilinear(x, dst[0], dst[1], add, -1.0), ops.resize_bilinear(x, dst, add=add, sign=-1.0))
    assert torch.equal(A.resize_bilinear_adjoint(g, src[0], src[1]), ops.resize_bilinear_adjoint(g, src))
    leaf, aleaf = x.clone().requires_grad_(True), add.clone().requires_grad_(True)
    A.resize_bilinear(leaf, dst[0], dst[1], aleaf, -1.0).backward(g)
    assert torch.equal(leaf.grad, ops.resize_bilinear_adjoint(g, src) * -1.0)
    assert torch.equal(aleaf.grad, g)
    torch.library.opcheck(A.resize_bilinear, (x.clone().requires_grad_(True), dst[0], dst[1], None, 1.0))
    torch.library.opcheck(A.resize_bilinear, (x.clone().requires_grad_(True), dst[0], dst[1],
                                              add.clone().requires_grad_(True), -1.0))
    torch.library.opcheck(A.resize_bilinear_adjoint, (g, src[0], src[1]))
