"""CPU: the feature k-means' definition (tests/kmeans_ref.py), the condition on the named cases' inputs,
the fp32 emulation against the float64 reference under the bars of the GPU tests, the mode filter's
rules, the counts-to-weights rule of AutoRegions, the C ABI's argument checks and workspace query, and
the wiring into the header, the registered ops and the model. No GPU needed: nothing is launched."""
import os
import re

import pytest
import torch

import kmeans_ref as R
from arbitrarystyletransfer_amd import _lib, library, models, ops  # noqa: F401  (library registers the ops)

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
OP_TOL = R.OP_TOL


def _same_partition(a, b, k):
    """Whether two label maps describe the same k clusters up to the clusters' names."""
    pairs = set(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()))
    return len(pairs) == k and len({p[0] for p in pairs}) == k and len({p[1] for p in pairs}) == k


# ---- the definition -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_reference_recovers_the_planted_clusters(name):
    """Maximin puts one seed into every planted cluster and Lloyd returns the planting exactly, with
    the runner-up far from the winner in every round."""
    k = R.ALL_CASES[name][3]
    x, planted = R.planted_inputs(name)
    seeds = R.seed(x, k)
    hit = sorted(int(planted.reshape(-1)[s]) for s in seeds)
    trace = []
    cen, lab, counts = R.lloyd(x, k, 3, trace=trace)
    margin = min(t[1] for t in trace) / float((R.points(x) ** 2).sum(1).max())
    print(f"{name}: seeds {seeds} lie in clusters {hit}; least runner-up margin {margin:.3f} max||x||^2 "
          f"(bar {R.PLANTED_MARGIN}); counts {counts.tolist()}")
    assert hit == list(range(k))
    assert _same_partition(lab, planted, k)
    assert counts.tolist() == torch.bincount(lab.reshape(-1).long(), minlength=k).tolist()
    assert k == 1 or margin >= R.PLANTED_MARGIN
    exact = R.update(x, planted, torch.zeros(k, x.shape[1]))[0]          # the planted clusters' own means
    order = [int(lab.reshape(-1)[(planted.reshape(-1) == j).nonzero()[0, 0]]) for j in range(k)]
    assert torch.equal(cen[order], exact)


def test_reference_edge_rules():
    """The lowest k wins an exact tie; a NaN never wins; a point whose distances are all NaN or +inf gets
    255 and belongs to no cluster; an empty cluster keeps its centroid; seeds tie to the lowest g."""
    nan, inf = float("nan"), float("inf")
    d = torch.tensor([[2.0, 1.0, 1.0], [nan, 3.0, 2.0], [nan, nan, nan], [inf, inf, inf], [inf, 5.0, nan]])
    assert R.argmin_rows(d).tolist() == [1, 2, 255, 255, 1]
    x = R.features(12901, (1, 6, 2, 3))
    cen = R.features(12902, (3, 6))
    cen[2] = cen[0]                                             # a duplicate: never chosen
    lab = R.assign(x, cen)
    assert not bool((lab == 2).any())
    x[0, 0, 0, 1] = nan
    lab = R.assign(x, cen)
    assert int(lab[0, 0, 1]) == 255
    new, counts = R.update(x, lab, cen)
    assert int(counts.sum()) == 5 and int(counts[2]) == 0 and torch.equal(new[2], cen[2].double())
    assert bool(torch.isfinite(new).all())                      # the NaN point is in no sum
    twice = torch.cat([R.features(12903, (1, 4, 1, 5))] * 2, dim=3)      # every point twice: g and g + 5
    assert all(s < 5 for s in R.seed(twice, 3))


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_inertia_never_rises(name):
    k = R.ALL_CASES[name][3]
    x, _ = R.case_inputs(name)
    trace = []
    R.lloyd(x, k, 6, trace=trace)
    inertia = [t[0] for t in trace]
    print(f"{name}: float64 inertia per round {[round(v, 4) for v in inertia]}")
    assert all(b <= a * (1 + 1e-12) for a, b in zip(inertia, inertia[1:]))


# ---- the inputs and the emulation -----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_near_ties_are_rare_in_the_reference(name):
    x, cen = R.case_inputs(name)
    frac = R.near_tie_fraction(x, cen)
    print(f"{name}: {100 * frac:.2f} % of the points have a runner-up within 2 * OP_TOL * E")
    assert frac <= R.NEAR_TIE_MAX


@pytest.mark.parametrize("name", list(R.ALL_CASES))
def test_emulation_meets_the_bars(name):
    x, cen = R.case_inputs(name)
    lab = R.assign(x, cen, torch.float32)
    short, same, total = R.check_assign(lab, x, cen)
    print(f"{name}: fp32 emulation assign shortfall {short:.2e} E (bar {2 * OP_TOL:.0e}), {same}/{total} labels equal "
          f"the float64 argmin")
    assert short <= 2 * OP_TOL
    ref, counts = R.update(x, lab, cen)
    emu, counts32 = R.update(x, lab, cen, torch.float32)
    e = R.rel_inf(emu, ref)
    print(f"  update {e:.2e} (bar {OP_TOL:.0e}), counts {counts.tolist()}")
    assert e <= OP_TOL and torch.equal(counts, counts32)
    k = cen.shape[0]
    worst = R.check_seeds(R.seed(x, k, torch.float32), x)
    print(f"  seeds {worst:.2e} E (bar {2 * OP_TOL:.0e})")
    assert worst <= 2 * OP_TOL


# ---- the mode filter ------------------------------------------------------------------------------------

def test_mode_filter_rules():
    u8 = torch.uint8
    one = torch.tensor([[[2]]], dtype=u8)
    assert torch.equal(R.mode_filter(one, 3), one)                                   # 1 x 1: its own vote
    row = torch.tensor([[[0, 1, 1, 0, 0]]], dtype=u8)
    # windows: {0,1} tie -> own 0; {0,1,1} -> 1; {1,1,0} -> 1; {1,0,0} -> 0; {0,0} -> 0
    assert R.mode_filter(row, 2).tolist() == [[[0, 1, 1, 0, 0]]]
    row = torch.tensor([[[2, 0, 1, 1, 2]]], dtype=u8)
    # {2,0} tie, own 2 among the tied; {2,0,1} three-way tie, own 0; {0,1,1} -> 1; {1,1,2} -> 1; {1,2} tie, own 2
    assert R.mode_filter(row, 3).tolist() == [[[2, 0, 1, 1, 2]]]
    tie = torch.tensor([[[0, 0, 0], [1, 2, 1], [1, 0, 1]]], dtype=u8)
    # the centre sees 0 x 4, 1 x 4, 2 x 1: its own label 2 is not among the tied, so the lowest, 0
    assert int(R.mode_filter(tie, 3)[0, 1, 1]) == 0
    tie[0, 1, 1] = 1                                            # now 1 x 5
    assert int(R.mode_filter(tie, 3)[0, 1, 1]) == 1
    hole = torch.tensor([[[0, 0, 0], [0, 255, 0], [0, 0, 1]]], dtype=u8)
    out = R.mode_filter(hole, 2)
    assert int(out[0, 1, 1]) == 255 and int(out[0, 2, 2]) == 0  # a hole passes through and does not vote
    assert int(R.mode_filter(hole, 1)[0, 2, 2]) == 1            # K = 1: label 1 is a hole too
    m = R.label_maps(12950, (2, 7, 9), 4)
    assert torch.equal(R.mode_filter(m, 4, 2), R.mode_filter(R.mode_filter(m, 4), 4))
    assert torch.equal(R.mode_filter(m, 4, 0), m)


# ---- AutoRegions ------------------------------------------------------------------------------------------

def test_auto_region_weights():
    w, dead = models.auto_region_weights([[5, 1, 0], [1, 0, 1], [2, 2, 7]])
    print(f"weights {w.tolist()}, dead {dead.tolist()}")
    assert w.dtype == torch.float64 and w.device.type == "cpu"
    assert w[0].tolist() == [5.0, 0.0, 0.0]                     # a count of 1 becomes 0
    assert dead.tolist() == [False, True, False]                # ones alone: no style has two pixels
    assert w[1].tolist() == [1 / 3] * 3                         # refilled, a valid mix
    assert w[2].tolist() == [2.0, 2.0, 7.0]
    mix = models.region_weights(w, 1, 3)                        # what the regional methods make of it
    assert torch.allclose(mix.sum(dim=2), torch.ones(1, 3, dtype=torch.float64))
    w, dead = models.auto_region_weights(torch.tensor([[0], [4]], dtype=torch.int32))
    assert w.tolist() == [[1.0], [4.0]] and dead.tolist() == [True, False]
    with pytest.raises(ValueError):
        models.auto_region_weights([1, 2, 3])


def test_auto_regions_validation():
    a = models.AutoRegions()
    assert (a.regions, a.iters, a.smooth, a.normalize) == (3, 10, 1, True)
    assert ops.KMEANS_DEFAULT_ITERS == 10
    b = models.AutoRegions(8, iters=0, smooth=0, normalize=False)
    assert (b.regions, b.iters, b.smooth, b.normalize) == (8, 0, 0, False) and "regions=8" in repr(b)
    for bad in (dict(regions=0), dict(regions=9), dict(regions=2.0), dict(regions=True), dict(iters=-1),
                dict(iters=1.5), dict(smooth=-1), dict(smooth=None), dict(normalize=1)):
        with pytest.raises(ValueError):
            models.AutoRegions(**bad)
    with pytest.raises(AttributeError):
        a.regions = 4


def test_auto_labels_exclude_explicit_maps():
    net = models.AdaINStyleTransfer()
    for p in net.parameters():
        p.requires_grad_(False)
    img, sty = torch.zeros(1, 3, 32, 32), torch.zeros(2, 3, 32, 32)
    sl = torch.zeros(2, 32, 32, dtype=torch.uint8)
    auto = models.AutoRegions(2)
    for method in (net.stylize_regions, net.stylize_regions_wct):
        with pytest.raises(ValueError, match="AutoRegions"):
            method(img, sty, labels=auto, style_labels=sl)
        with pytest.raises(ValueError, match="AutoRegions"):
            method(img, sty, labels=auto, weights=[[1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="AutoRegions"):
        net.stylize_swap_regions(img, sty, labels=auto, style_labels=sl)
    with pytest.raises(ValueError, match="at most 64 rows"):
        net.stylize_regions(img, torch.zeros(9, 3, 32, 32), labels=models.AutoRegions(8))
    with pytest.raises(ValueError, match="must be an AutoRegions"):
        net.auto_labels(img, sty, auto=3)
    with pytest.raises(ValueError):
        net.auto_labels(img[0], sty)
    assert callable(models.AdaINStyleTransfer.auto_labels)


def test_methods_raise_under_grad():
    net = models.AdaINStyleTransfer()
    img, sty = torch.zeros(1, 3, 32, 32), torch.zeros(2, 3, 32, 32)
    auto = models.AutoRegions(2)
    for call in (lambda: net.auto_labels(img, sty), lambda: net.stylize_regions(img, sty, labels=auto),
                 lambda: net.stylize_regions_wct(img, sty, labels=auto),
                 lambda: net.stylize_swap_regions(img, sty, labels=auto)):
        with pytest.raises(NotImplementedError):            # the parameters ask for a gradient
            call()


# ---- C ABI ----------------------------------------------------------------------------------------------

P = 256   # a non-null "pointer": every call below must return before anything is launched or read
BIG = 1 << 40


def _seed(L, x=P, seeds=P, b=2, c=8, h=4, w=5, k=3, ws=P, nbytes=BIG):
    return L.ast_kmeans_seed_f32(x, seeds, b, c, h, w, k, ws, nbytes, None)


def _assign(L, x=P, cen=P, labels=P, b=2, c=8, h=4, w=5, k=3):
    return L.ast_kmeans_assign_f32(x, cen, labels, b, c, h, w, k, None)


def _update(L, x=P, labels=P, prev=P, cen=P, counts=P, b=2, c=8, h=4, w=5, k=3, ws=P, nbytes=BIG):
    return L.ast_kmeans_update_f32(x, labels, prev, cen, counts, b, c, h, w, k, ws, nbytes, None)


def _whole(L, x=P, init=None, cen=P, labels=P, counts=P, b=2, c=8, h=4, w=5, k=3, iters=2, ws=P, nbytes=BIG):
    return L.ast_kmeans_f32(x, init, cen, labels, counts, None, b, c, h, w, k, iters, ws, nbytes, None)


def _mode(L, labels=P, out=2 * P, n=2, h=4, w=5, regions=3, passes=1, ws=P, nbytes=BIG):
    return L.ast_label_mode_filter_u8(labels, out, n, h, w, regions, passes, ws, nbytes, None)


@pytest.mark.parametrize("want,call", [
    (E_NULL, lambda L: _seed(L, x=None)),
    (E_NULL, lambda L: _seed(L, seeds=None)),
    (E_NULL, lambda L: _seed(L, ws=None)),
    (E_SHAPE, lambda L: _seed(L, b=0)),
    (E_SHAPE, lambda L: _seed(L, k=0)),
    (E_SHAPE, lambda L: _seed(L, nbytes=16)),
    (E_SHAPE, lambda L: _seed(L, b=5, h=2048, w=2048)),              # 5 * 2^22 points > 2^24
    (E_UNSUPPORTED, lambda L: _seed(L, k=9)),
    (E_UNSUPPORTED, lambda L: _seed(L, c=1025)),
    (E_NULL, lambda L: _assign(L, cen=None)),
    (E_NULL, lambda L: _assign(L, labels=None)),
    (E_SHAPE, lambda L: _assign(L, c=0)),
    (E_SHAPE, lambda L: _assign(L, h=0)),
    (E_SHAPE, lambda L: _assign(L, h=4097, w=4096)),
    (E_UNSUPPORTED, lambda L: _assign(L, k=9)),
    (E_UNSUPPORTED, lambda L: _assign(L, c=1025)),
    (E_NULL, lambda L: _update(L, labels=None)),
    (E_NULL, lambda L: _update(L, prev=None)),
    (E_NULL, lambda L: _update(L, counts=None)),
    (E_NULL, lambda L: _update(L, ws=None)),
    (E_SHAPE, lambda L: _update(L, w=0)),
    (E_SHAPE, lambda L: _update(L, nbytes=512)),
    (E_UNSUPPORTED, lambda L: _update(L, k=9)),
    (E_NULL, lambda L: _whole(L, x=None)),
    (E_NULL, lambda L: _whole(L, cen=None)),
    (E_NULL, lambda L: _whole(L, labels=None)),
    (E_NULL, lambda L: _whole(L, counts=None)),
    (E_NULL, lambda L: _whole(L, ws=None)),
    (E_SHAPE, lambda L: _whole(L, b=0)),
    (E_SHAPE, lambda L: _whole(L, nbytes=512)),
    (E_UNSUPPORTED, lambda L: _whole(L, iters=-1)),
    (E_UNSUPPORTED, lambda L: _whole(L, k=9)),
    (E_UNSUPPORTED, lambda L: _whole(L, c=1025)),
    (E_NULL, lambda L: _mode(L, labels=None)),
    (E_NULL, lambda L: _mode(L, out=None)),
    (E_NULL, lambda L: _mode(L, out=P)),                             # in place
    (E_NULL, lambda L: _mode(L, passes=2, ws=None)),
    (E_SHAPE, lambda L: _mode(L, n=0)),
    (E_SHAPE, lambda L: _mode(L, passes=2, nbytes=8)),
    (E_UNSUPPORTED, lambda L: _mode(L, regions=0)),
    (E_UNSUPPORTED, lambda L: _mode(L, regions=9)),
    (E_UNSUPPORTED, lambda L: _mode(L, passes=-1)),
])
def test_bad_arguments_are_rejected_before_launch(want, call):
    assert call(_lib.lib()) == want


def test_workspace_queries():
    L = _lib.lib()
    q = L.ast_kmeans_workspace_bytes
    by_points = [q(b, 64, 40, 40, 5) for b in (1, 2, 4)]
    by_k = [q(2, 64, 40, 40, k) for k in (1, 2, 5, 8)]
    by_c = [q(2, c, 40, 40, 5) for c in (8, 64, 512)]
    print(f"workspace bytes by maps {by_points}, by k {by_k}, by channels {by_c}")
    for sizes in (by_points, by_k, by_c):
        assert sizes[0] > 0 and sizes == sorted(set(sizes)), sizes      # positive, strictly growing
    # at least the distances of the seeding (one float per point) and one workgroup's partial sums
    assert q(2, 64, 40, 40, 5) >= 4 * 3200 + 4 * 5 * 64
    assert q(1, 8, 1, 1, 1) > 0
    assert q(0, 8, 4, 4, 2) == E_SHAPE and q(1, 8, 4, 4, 0) == E_SHAPE and q(5, 8, 2048, 2048, 2) == E_SHAPE
    assert q(1, 1025, 4, 4, 2) == E_UNSUPPORTED and q(1, 8, 4, 4, 9) == E_UNSUPPORTED
    m = L.ast_label_mode_filter_workspace_bytes
    assert m(2, 7, 9, 0) == 0 and m(2, 7, 9, 1) == 0 and m(2, 7, 9, 2) >= 2 * 7 * 9 and m(4, 40, 40, 3) > m(2, 40, 40, 3)
    assert m(0, 7, 9, 1) == E_SHAPE and m(2, 7, 9, -1) == E_UNSUPPORTED


def test_python_arguments_are_checked_before_launch():
    x = torch.rand(1, 4, 3, 3)
    for k in (0, 9, 2.0, True):
        with pytest.raises(_lib.HipOpError, match="regions must be an int"):
            ops.kmeans(x, k)
        with pytest.raises(_lib.HipOpError, match="regions must be an int"):
            ops.kmeans_seed(x, k)
    with pytest.raises(_lib.HipOpError, match="iters must be an int"):
        ops.kmeans(x, 2, iters=-1)
    with pytest.raises(_lib.HipOpError, match="passes must be an int"):
        ops.label_mode_filter(torch.zeros(1, 3, 3, dtype=torch.uint8), 2, passes=-1)
    with pytest.raises(_lib.HipOpError, match="regions must be an int"):
        ops.label_mode_filter(torch.zeros(1, 3, 3, dtype=torch.uint8), 0)
    for call in (lambda: ops.kmeans(x, 2), lambda: ops.kmeans_seed(x, 2),                  # CPU tensors
                 lambda: ops.kmeans_assign(x, torch.rand(2, 4)),
                 lambda: ops.kmeans_update(x, torch.zeros(1, 3, 3, dtype=torch.uint8), torch.rand(2, 4)),
                 lambda: ops.label_mode_filter(torch.zeros(1, 3, 3, dtype=torch.uint8), 2)):
        with pytest.raises(_lib.HipOpError):
            call()
    with pytest.raises(_lib.HipOpError, match="labels must be uint8"):
        ops.kmeans_update(x, torch.zeros(1, 3, 3, dtype=torch.int64), torch.rand(2, 4))
    assert ops.KMEANS_MAX_C == 1024 and ops.KMEANS_MAX_POINTS == 1 << 24


# ---- wiring ---------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ast_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ast_kmeans_workspace_bytes", "ast_kmeans_seed_f32", "ast_kmeans_assign_f32", "ast_kmeans_update_f32",
                 "ast_kmeans_f32", "ast_label_mode_filter_workspace_bytes", "ast_label_mode_filter_u8"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert re.search(r"#define\s+AST_KMEANS_MAX_K\s+8\b", src)
    assert re.search(r"#define\s+AST_KMEANS_MAX_C\s+1024\b", src)
    assert re.search(r"#define\s+AST_KMEANS_MAX_POINTS\s+\(1 << 24\)", src)


def test_registered_ops_and_meta_kernels():
    new = ["kmeans", "kmeans_assign", "label_mode_filter"]
    assert library.OPS[-3:] == new                               # appended: the earlier entries keep their order
    m = torch.device("meta")
    x = torch.empty(3, 16, 5, 7, device=m)
    cen, lab, counts = torch.ops.ast_hip.kmeans(x, 4, 10, None)
    assert cen.shape == (4, 16) and cen.dtype == torch.float32
    assert lab.shape == (3, 5, 7) and lab.dtype == torch.uint8
    assert counts.shape == (4,) and counts.dtype == torch.int32
    cen, lab, counts = torch.ops.ast_hip.kmeans(x, 2, 0, torch.empty(2, 16, device=m))
    assert cen.shape == (2, 16) and lab.device.type == "meta"
    lab = torch.ops.ast_hip.kmeans_assign(torch.empty(2, 16, 6, 4, device=m), torch.empty(5, 16, device=m))
    assert lab.shape == (2, 6, 4) and lab.dtype == torch.uint8
    out = torch.ops.ast_hip.label_mode_filter(lab, 5, 2)
    assert out.shape == lab.shape and out.dtype == torch.uint8 and out.device.type == "meta"
