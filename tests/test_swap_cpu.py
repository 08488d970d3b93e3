"""CPU: style swap's definition (tests/swap_ref.py), the condition on the named cases' inputs, the fp32
emulation against the float64 reference under the bars of the GPU tests, the C ABI's argument checks
and workspace queries, and the wiring of the op into the header, the registered ops and the model.
No GPU needed: nothing is launched."""
import functools
import os
import re

import pytest
import torch

import swap_ref as SR
from arbitrarystyletransfer_amd import _lib, library, models, ops  # noqa: F401  (library registers the ops)

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
OP_TOL = SR.OP_TOL


@functools.lru_cache(maxsize=None)
def _ref_scores(name):
    c, s = SR.case_inputs(name)
    return SR.scores(c, s)


# ---- the definition ---------------------------------------------------------------------------------

def test_reference_recovers_a_planted_crop():
    """A content that is a crop of the style at (2, 3): every patch finds itself (a patch's score
    against itself is its norm, the maximum by Cauchy-Schwarz), and the swap returns the crop."""
    s = SR.features(9901, (1, 6, 9, 11))
    c = s[:, :, 2:7, 3:9].clone()
    out, idx = SR.style_swap(c, s)
    y, x = torch.meshgrid(torch.arange(3), torch.arange(4), indexing="ij")
    assert torch.equal(idx[0], (y + 2) * 9 + (x + 3))
    assert SR.rel_inf(out, c) <= 1e-12
    half, _ = SR.style_swap(c, 2.0 * s, alpha=0.5)       # the style's scale leaves the match alone
    assert SR.rel_inf(half, 1.5 * c.double()) <= 1e-12


def test_reference_edge_rules():
    """A zero style patch scores 0 and loses to any positive score; an all-zero content patch ties
    everywhere and takes index 0; a NaN never wins; the first of equal scores wins."""
    s = SR.features(9902, (1, 4, 3, 7))
    s[:, :, :, :3] = 0.0                                   # style patch 0 is all zero
    c = SR.features(9903, (1, 4, 3, 4))
    c[:, :, :, :3] = 0.0                                   # content patch 0 is all zero
    sc = SR.scores(c, s)
    assert float(sc[0, :, 0].abs().max()) == 0.0 and float(sc[0, 0].abs().max()) == 0.0
    idx, best = SR.match(c, s)
    assert idx.flatten().tolist()[0] == 0 and idx.flatten().tolist()[1] != 0 and float(best.flatten()[1]) > 0
    sn = s.clone()
    sn[0, 0, 1, 6] = float("nan")                          # poisons style patches 4 only (columns 4..6)
    idx_n, _ = SR.match(c, sn)
    assert idx_n.flatten().tolist()[1] != 4 and idx_n.flatten().tolist()[0] == 0
    per = SR.features(9904, (1, 4, 3, 4)).repeat(1, 1, 1, 3)   # period 4 along x: patches j and j + 4 are equal
    idx_p, _ = SR.match(SR.features(9905, (1, 4, 5, 6)), per)
    assert int(idx_p.max()) < 4


def test_overlap_counts():
    """A constant value map reconstructs to the constant whatever the indices: the divisor is the
    number of covering patches (1 in a corner, 9 in the interior)."""
    sv = torch.full((1, 3, 5, 6), 0.7)
    idx = torch.randint(0, 12, (1, 4, 5), generator=torch.Generator().manual_seed(1))
    c = SR.features(9906, (1, 3, 6, 7))
    assert SR.rel_inf(SR.gather(sv, idx, c, 1.0), torch.full_like(c, 0.7)) <= 1e-12
    assert SR.rel_inf(SR.gather(sv, idx, c, 0.0), c) == 0.0


# ---- the inputs and the emulation -----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SR.CASES))
def test_near_ties_are_rare_in_the_reference(name):
    frac = SR.near_tie_fraction(_ref_scores(name))
    print(f"{name}: {100 * frac:.2f} % of the content patches have a runner-up within 2 * OP_TOL * S "
          f"(S = {SR.top_scale(_ref_scores(name)):.3f})")
    assert frac <= SR.NEAR_TIE_MAX


@pytest.mark.parametrize("name", list(SR.CASES))
def test_emulation_meets_both_bars(name):
    c, s = SR.case_inputs(name)
    idx, best = SR.match(c, s, torch.float32)
    e_score, shortfall = SR.check_match(idx, best, _ref_scores(name))
    print(f"{name}: fp32 emulation score error {e_score:.2e} S (bar {OP_TOL:.0e}), index shortfall {shortfall:.2e} S "
          f"(bar {2 * OP_TOL:.0e})")
    assert e_score <= OP_TOL and shortfall <= 2 * OP_TOL
    for alpha in (1.0, 0.6):
        got = SR.gather(s, idx, c, alpha, torch.float32)
        e = SR.rel_inf(got, SR.gather(s, idx, c, alpha))
        print(f"  gather alpha={alpha}: {e:.2e} (bar {SR.GATHER_TOL:.0e})")
        assert e <= SR.GATHER_TOL


# ---- C ABI ----------------------------------------------------------------------------------------------

P = 256   # a non-null "pointer": every call below must return before anything is launched or read
BIG = 1 << 40


@pytest.mark.parametrize("want,call", [
    # ast_style_swap_f32(ck, sk, sv, c, out, index, score, n, ns, c, hc, wc, hs, ws, alpha, ws, bytes, stream)
    (E_NULL, lambda L: L.ast_style_swap_f32(None, P, P, P, P, None, None, 2, 2, 8, 4, 4, 4, 4, 1.0, P, BIG, None)),
    (E_NULL, lambda L: L.ast_style_swap_f32(P, P, None, P, P, None, None, 2, 2, 8, 4, 4, 4, 4, 1.0, P, BIG, None)),
    (E_NULL, lambda L: L.ast_style_swap_f32(P, P, P, P, None, None, None, 2, 2, 8, 4, 4, 4, 4, 1.0, P, BIG, None)),
    (E_NULL, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 2, 8, 4, 4, 4, 4, 1.0, None, BIG, None)),
    (E_SHAPE, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 2, 8, 2, 4, 4, 4, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 2, 8, 4, 4, 4, 2, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 3, 8, 4, 4, 4, 4, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 0, 1, 8, 4, 4, 4, 4, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 2, 0, 4, 4, 4, 4, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 2, 8, 4, 4, 4, 4, 1.0, P, 512, None)),
    (E_UNSUPPORTED, lambda L: L.ast_style_swap_f32(P, P, P, P, P, None, None, 2, 2, 1025, 4, 4, 4, 4, 1.0, P, BIG, None)),
    # ast_patch_norms_f32(sk, inv, ns, c, hs, ws, ws, bytes, stream)
    (E_NULL, lambda L: L.ast_patch_norms_f32(P, None, 1, 8, 4, 4, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_patch_norms_f32(P, P, 1, 8, 4, 2, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_patch_norms_f32(P, P, 1, 8, 4, 4, P, 16, None)),
    (E_UNSUPPORTED, lambda L: L.ast_patch_norms_f32(P, P, 1, 1025, 4, 4, P, BIG, None)),
    # ast_patch_match_f32(ck, sk, inv, index, score, n, ns, c, hc, wc, hs, ws, ws, bytes, stream)
    (E_NULL, lambda L: L.ast_patch_match_f32(P, P, None, P, None, 2, 2, 8, 4, 4, 4, 4, P, BIG, None)),
    (E_NULL, lambda L: L.ast_patch_match_f32(P, P, P, None, None, 2, 2, 8, 4, 4, 4, 4, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_patch_match_f32(P, P, P, P, None, 2, 2, 8, 4, 2, 4, 4, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_patch_match_f32(P, P, P, P, None, 2, 3, 8, 4, 4, 4, 4, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_patch_match_f32(P, P, P, P, None, 2, 2, 8, 4, 4, 4, 4, P, 16, None)),
    (E_UNSUPPORTED, lambda L: L.ast_patch_match_f32(P, P, P, P, None, 2, 2, 1025, 4, 4, 4, 4, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_patch_match_ex_f32(P, P, P, P, None, 2, 2, 8, 4, 4, 4, 4, -1, P, BIG, None)),
    # ast_patch_gather_f32(sv, index, content, out, n, ns, c, hc, wc, hs, ws, alpha, stream)
    (E_NULL, lambda L: L.ast_patch_gather_f32(P, None, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, None)),
    (E_SHAPE, lambda L: L.ast_patch_gather_f32(P, P, P, P, 2, 2, 8, 4, 4, 2, 4, 1.0, None)),
    (E_SHAPE, lambda L: L.ast_patch_gather_f32(P, P, P, P, 2, 3, 8, 4, 4, 4, 4, 1.0, None)),
    (E_UNSUPPORTED, lambda L: L.ast_patch_gather_f32(P, P, P, P, 2, 2, 1025, 4, 4, 4, 4, 1.0, None)),
])
def test_bad_arguments_are_rejected_before_launch(want, call):
    assert call(_lib.lib()) == want


def test_workspace_queries():
    L = _lib.lib()
    n, ns, _, (hc, wc), (hs, ws) = SR.CASES["c512_split_keys"]
    by_splits = [L.ast_patch_match_workspace_bytes(n, ns, hc, wc, hs, ws, k) for k in (1, 2, 4, 8)]
    assert by_splits[0] > 0 and by_splits == sorted(set(by_splits)), by_splits      # positive, strictly growing
    assert L.ast_patch_match_workspace_bytes(n, ns, hc, wc, hs, ws, 0) > by_splits[0]   # the library splits this shape
    assert L.ast_patch_match_workspace_bytes(128, 128, 64, 64, 64, 64, 0) == L.ast_patch_match_workspace_bytes(128, 128, 64, 64, 64, 64, 1)
    assert L.ast_patch_match_workspace_bytes(1, 1, 64, 64, 64, 64, 0) > L.ast_patch_match_workspace_bytes(1, 1, 64, 64, 64, 64, 1)
    assert L.ast_patch_norms_workspace_bytes(1, 34, 34) >= 4 * 34 * 34
    whole = L.ast_style_swap_workspace_bytes(n, ns, hc, wc, hs, ws)
    assert whole >= L.ast_patch_match_workspace_bytes(n, ns, hc, wc, hs, ws, 0) + 4 * 1024 + 4 * 64
    assert L.ast_style_swap_workspace_bytes(2, 3, 4, 4, 4, 4) == E_SHAPE
    assert L.ast_style_swap_workspace_bytes(2, 2, 4, 2, 4, 4) == E_SHAPE
    assert L.ast_patch_match_workspace_bytes(2, 2, 4, 4, 4, 4, -1) == E_UNSUPPORTED
    assert L.ast_patch_norms_workspace_bytes(1, 2, 4) == E_SHAPE


# ---- wiring ---------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ast_hip.h")).read(), flags=re.S)
    for name in ("ast_patch_norms_workspace_bytes", "ast_patch_norms_f32", "ast_patch_match_workspace_bytes",
                 "ast_patch_match_f32", "ast_patch_match_ex_f32", "ast_patch_gather_f32",
                 "ast_style_swap_workspace_bytes", "ast_style_swap_f32"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name


def test_registered_op_and_meta_kernel():
    assert "style_swap" in library.OPS
    m = torch.device("meta")
    c, s = torch.empty(2, 16, 8, 12, device=m), torch.empty(1, 16, 5, 7, device=m)
    out = torch.ops.ast_hip.style_swap(c, s, 0.6, True)
    assert out.shape == c.shape and out.dtype == c.dtype and out.device.type == "meta"


def test_model_surface():
    mod = models.StyleSwap(normalize=True)
    assert mod.normalize is True and not list(mod.parameters()) and not list(mod.buffers())
    assert models.StyleSwap().normalize is False
    assert callable(getattr(models.AdaINStyleTransfer, "stylize_swap"))
    assert models.AdaINStyleTransfer.TRANSFORMS == ("adain", "efdm", "wct")
    net = models.AdaINStyleTransfer(transform="wct")
    assert not any("swap" in k for k in net.state_dict())
    assert list(net.state_dict()) == list(models.AdaINStyleTransfer().state_dict())


def test_cpu_tensors_and_gradients_are_rejected():
    x = torch.rand(1, 4, 5, 5)
    with pytest.raises(_lib.HipOpError):
        ops.style_swap(x, x)
    with pytest.raises(_lib.HipOpError):
        ops.patch_match(x, x)
    with pytest.raises(_lib.HipOpError):
        ops.patch_gather(x, torch.zeros(1, 3, 3, dtype=torch.int32), x)
    with pytest.raises(NotImplementedError):
        models.StyleSwap()(x.clone().requires_grad_(), x)
    net = models.AdaINStyleTransfer()
    with pytest.raises(NotImplementedError):          # the parameters ask for a gradient
        net.stylize_swap(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))
