"""CPU: the float64 statement of the bilinear resize and Laplacian pyramid (tests/lap_ref.py), the
bars derived there, the adjoint kernel's output ranges, and the host-side argument checks of
csrc/pyramid.hip through the C ABI (nothing is launched: no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

import lap_ref as LR
from arbitrarystyletransfer_amd import _lib, ops

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")
ALL_CASES = LR.CASES + [LR.BIG]


@pytest.mark.parametrize("size", [(37, 50), (64, 48), (1, 9), (5, 5)])
@pytest.mark.parametrize("levels", [0, 1, 4])
def test_collapse_of_build_is_identity(size, levels):
    x = LR.image(3, (2, 3) + size).double()
    pyr = LR.build(x, levels)
    assert len(pyr) == levels + 1
    assert float((LR.collapse(pyr) - x).abs().max()) <= 1e-12


def test_build_sizes():
    pyr = LR.build(LR.image(4, (3, 37, 50)), 4)
    assert [tuple(p.shape[-2:]) for p in pyr] == [(37, 50), (18, 25), (9, 12), (4, 6), (2, 3)]
    assert [tuple(p.shape[-2:]) for p in LR.build(LR.image(4, (1, 3)), 3)] == [(1, 3), (1, 1), (1, 1), (1, 1)]
    assert ops.lap_down_size((37, 50)) == LR.down_size((37, 50)) == (18, 25)
    assert ops.lap_down_size((1, 1)) == (1, 1)


@pytest.mark.parametrize("src,dst", ALL_CASES)
def test_adjoint_identity_float64(src, dst):
    gen = torch.Generator().manual_seed(11)
    c = torch.randn((3,) + src, generator=gen, dtype=torch.float64)
    g = torch.randn((3,) + dst, generator=gen, dtype=torch.float64)
    for fwd, adj in ((LR.interp, LR.adjoint), (LR.resize_ref, LR.adjoint_ref)):
        lhs, rhs = float((fwd(c, dst) * g).sum()), float((c * adj(g, src)).sum())
        assert abs(lhs - rhs) <= 1e-12 * float(c.abs().sum() + g.abs().sum())


@pytest.mark.parametrize("src,dst", ALL_CASES)
def test_fp32_coordinates_stay_within_the_coordinate_bar(src, dst):
    """The kernel's definition (fp32 source coordinates) against the oracle: within resize_bar less
    its arithmetic part, and the adjoint likewise -- the bars hold for the restatement itself."""
    gen = torch.Generator().manual_seed(12)
    x = torch.rand((3,) + src, generator=gen, dtype=torch.float64)
    err = float((LR.resize_ref(x, dst) - LR.interp(x, dst)).abs().max())
    bar = LR.resize_bar(x) - LR.arith_bar(float(x.abs().max()))
    print(f"{src}->{dst}: fp32-coordinate resize vs oracle {err:.2e}, coordinate bar {bar:.2e}")
    assert err <= bar + 1e-15
    g = torch.randn((3,) + dst, generator=gen, dtype=torch.float64)
    gmax = float(g.abs().max())
    err = float((LR.adjoint_ref(g, src) - LR.adjoint(g, src)).abs().max())
    bar = LR.adjoint_bar(gmax, src, dst) - LR.adjoint_arith_bar(gmax, src, dst)
    print(f"{src}->{dst}: fp32-coordinate adjoint vs oracle {err:.2e}, coordinate bar {bar:.2e}")
    assert err <= bar + 1e-15


def _pairs():
    rng = np.random.default_rng(5)
    pairs = [(a, b) for a in range(1, 41) for b in range(1, 41)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(1, 4097, size=(300, 2))]
    pairs += [(1, 4096), (4096, 1), (4096, 4096), (4095, 4096), (4096, 4095), (3, 4096), (4096, 3), (2048, 4096),
              (4096, 2048), (1365, 4096), (4096, 1365)]
    return pairs


def test_adjoint_ranges_cover_every_touching_output():
    """The adjoint thread of source index s visits [lo, hi] and lets the forward map decide: every
    output whose cell {i0, i1} holds s must lie inside, with the range ends rounded either way the
    compiler may (separate multiply and subtract, or one fma)."""
    for inn, out in _pairs():
        i0, i1, l1 = LR.src_map(out, inn)
        o = np.arange(out)
        for fused in (False, True):
            lo, hi = LR.touch_range(np.arange(inn), inn, out, fused)
            assert np.all((lo[i0] <= o) & (o <= hi[i0])), (inn, out, fused)
            assert np.all(((lo[i1] <= o) & (o <= hi[i1]))[l1 > 0]), (inn, out, fused)   # l1 = 0: weight 0 on i1
            assert np.all(hi - lo + 1 <= 2 * np.ceil(out / inn) + 6), (inn, out, fused)


def test_touch_count_bounds_the_forward_map():
    for inn, out in _pairs():
        i0, i1, l1 = LR.src_map(out, inn)
        ends = sorted(set(range(min(inn, 32))) | set(range(max(inn - 32, 0), inn)))
        per_index = [np.count_nonzero((i0 == s) | ((i1 == s) & (l1 > 0))) for s in ends]
        assert max(per_index) <= LR.touch_count(out, inn), (inn, out)


def test_header_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("ast_resize_bilinear_f32", 10), ("ast_resize_bilinear_adjoint_f32", 9)):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)
    from arbitrarystyletransfer_amd import library
    assert library.OPS[library.OPS.index("luma_transfer") + 1] == "resize_bilinear"
    assert "resize_bilinear_adjoint" in library.OPS
    for name in ("resize_bilinear", "resize_bilinear_adjoint"):
        assert hasattr(torch.ops.ast_hip, name)


@pytest.mark.parametrize("call", [
    lambda L: L.ast_resize_bilinear_f32(None, 1, 1, 2, 2, 4, 4, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, None, 1, 2, 2, 4, 4, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, 1, 0, 2, 2, 4, 4, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, 1, 1, 0, 2, 4, 4, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, 1, 1, 2, 4097, 4, 4, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, 1, 1, 2, 2, 0, 4, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, 1, 1, 2, 2, 4, 4097, None, 1.0, None),
    lambda L: L.ast_resize_bilinear_f32(1, 1, -1, 2, 2, 4, 4, 1, -1.0, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(None, 1, 1, 2, 2, 4, 4, 0, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(1, None, 1, 2, 2, 4, 4, 0, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(1, 1, 0, 2, 2, 4, 4, 0, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(1, 1, 1, 2, 0, 4, 4, 1, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(1, 1, 1, 4097, 2, 4, 4, 0, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(1, 1, 1, 2, 2, 4, 0, 0, None),
    lambda L: L.ast_resize_bilinear_adjoint_f32(1, 1, 1, 2, 2, 4097, 4, 0, None),
])
def test_argument_errors_rejected_before_launch(call):
    assert call(_lib.lib()) < 0


def test_python_surface_rejects_bad_calls():
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(_lib.HipOpError):
        ops.resize_bilinear(x, (8, 8))                    # a CPU tensor: there is no CPU path
    with pytest.raises(_lib.HipOpError):
        ops.resize_bilinear_adjoint(x, (2, 2))
    with pytest.raises(_lib.HipOpError):
        ops.lap_build(x, 2)
    with pytest.raises(_lib.HipOpError):
        ops.lap_collapse([])
    with pytest.raises(_lib.HipOpError):
        ops.lap_collapse([x])
    with pytest.raises(_lib.HipOpError):
        ops.lap_build(x, -1)
    with pytest.raises(_lib.HipOpError):
        ops._resize_size((0, 4), "size")
    with pytest.raises(_lib.HipOpError):
        ops._resize_size((4, 4097), "size")
    with pytest.raises(_lib.HipOpError):
        ops._resize_size(7, "size")


def test_fake_kernels_give_the_output_shapes():
    m = torch.device("meta")
    x = torch.empty(2, 3, 18, 25, device=m)
    y = torch.ops.ast_hip.resize_bilinear(x, 37, 50, None, 1.0)
    assert y.shape == (2, 3, 37, 50) and y.dtype == torch.float32
    assert torch.ops.ast_hip.resize_bilinear(x, 9, 12, torch.empty(2, 3, 9, 12, device=m), -1.0).shape == (2, 3, 9, 12)
    assert torch.ops.ast_hip.resize_bilinear_adjoint(y, 18, 25).shape == x.shape
