"""CPU: guided style swap's definition (tests/swap_guided_ref.py), the condition on the named cases'
inputs, the fp32 emulation against the float64 reference under the bars of the GPU tests, the C ABI's
argument checks and workspace queries, and the wiring of the op into the header, the registered ops
and the model. No GPU needed: nothing is launched."""
import functools
import os
import re

import pytest
import torch

import swap_guided_ref as GR
import swap_ref as SR
from arbitrarystyletransfer_amd import _lib, library, models, ops  # noqa: F401  (library registers the ops)

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
OP_TOL = GR.OP_TOL
NEG_INF = float("-inf")


@functools.lru_cache(maxsize=None)
def _masked(name):
    c, s = GR.case_inputs(name)
    return GR.masked_scores(c, s, *GR.case_classes(name))


# ---- the definition ---------------------------------------------------------------------------------

def test_one_class_is_the_unguided_reference():
    """All classes 0 and S = 1: the unguided match and reconstruction."""
    c, s = SR.case_inputs("c48_k_tails")
    s = s[:1]
    cc = torch.zeros(2, 5, 7, dtype=torch.uint8)
    sc = torch.zeros(1, 4, 9, dtype=torch.uint8)
    idx, best = GR.match(c, s, cc, sc)
    ref_idx, ref_best = SR.match(c, s)
    assert torch.equal(idx, ref_idx) and torch.equal(best, ref_best)
    assert torch.equal(GR.gather(s, idx, c, 0.6), SR.gather(s, idx, c, 0.6))


def test_reference_edge_rules():
    """No candidate gives (-1, -inf); classes >= 64 take no part on either side; the lowest global j wins
    an exact tie, so the lower style of a bank of two equal styles; a NaN never wins; a patch whose
    candidates all score NaN returns -1."""
    c = SR.features(9951, (1, 4, 4, 5))                     # 2 x 3 content patches
    one = SR.features(9952, (1, 4, 5, 5))                   # 3 x 3 style patches
    bank = torch.cat([one, one])
    cc = torch.tensor([[[0, 1, 2], [64, 255, 0]]], dtype=torch.uint8)
    sc = torch.zeros(2, 3, 3, dtype=torch.uint8)
    sc[:, 1] = 1
    sc[:, 2, 0] = 64                                        # never a candidate, even for content class 64
    sc[:, 2, 1] = 255
    idx, best = GR.match(c, bank, cc, sc)
    idx, best = idx.flatten().tolist(), best.flatten().tolist()
    assert idx[2] == idx[3] == idx[4] == -1 and best[2] == best[3] == best[4] == NEG_INF   # class 2 absent; 64; 255
    assert 0 <= idx[0] < 9 and 0 <= idx[5] < 9 and 3 <= idx[1] < 6                           # the lower style
    assert idx[0] in (0, 1, 2, 8) and idx[5] in (0, 1, 2, 8)
    poisoned = c.clone()
    poisoned[0, 0, 0, 0] = float("nan")                     # content patch 0 alone holds the NaN
    idx_n, best_n = GR.match(poisoned, bank, cc, sc)
    assert idx_n.flatten().tolist() == [-1] + idx[1:] and best_n.flatten().tolist()[0] == NEG_INF
    nan = float("nan")
    rows = torch.tensor([[[nan, 1.0, NEG_INF, 1.0], [nan, NEG_INF, NEG_INF, nan], [NEG_INF, 2.0, nan, 3.0]]])
    i_r, b_r = GR.argmax_rows(rows)
    assert i_r.tolist() == [[1, -1, 3]] and b_r.tolist() == [[1.0, NEG_INF, 3.0]]


def test_reference_gather_rules():
    """cnt counts the matched covering patches only; a pixel with none of them is the content in bits,
    whatever alpha; an index past the bank is clamped; the index decodes (style, local patch)."""
    sv = torch.stack([torch.full((3, 5, 6), 0.25), torch.full((3, 5, 6), 0.75)])      # Ns = 12 per style
    c = SR.features(9953, (1, 3, 6, 7))                                                 # 4 x 5 content patches
    idx = torch.full((1, 4, 5), -1, dtype=torch.int64)
    idx[0, 0, 0] = 3                                        # style 0
    idx[0, 0, 1] = 12 + 5                                   # style 1
    out = GR.gather(sv, idx, c, 1.0)
    assert float(out[0, 0, 0, 0]) == 0.25 and float(out[0, 0, 0, 3]) == 0.75            # one covering patch each
    assert float(out[0, 0, 1, 1]) == 0.5                                                # both: the mean of two
    untouched = torch.ones(6, 7, dtype=torch.bool)
    untouched[0:3, 0:4] = False
    assert torch.equal(out[0, :, untouched], c.double()[0, :, untouched])
    for alpha in (1.0, 0.3):
        assert torch.equal(GR.gather(sv, torch.full((1, 4, 5), -1), c, alpha), c.double())
    assert torch.equal(GR.gather(sv, torch.full((1, 4, 5), 99), c, 1.0), GR.gather(sv, torch.full((1, 4, 5), 23), c, 1.0))
    assert SR.rel_inf(GR.gather(sv, idx, c, 0.0), c) == 0.0


def test_patch_classes_is_the_centre_pixel():
    lab = torch.arange(2 * 5 * 6, dtype=torch.uint8).reshape(2, 5, 6)
    got = ops.patch_classes(lab)
    assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got, lab[:, 1:-1, 1:-1])
    for bad in (lab.long(), lab[0], lab[:, :2]):
        with pytest.raises(_lib.HipOpError):
            ops.patch_classes(bad)
    assert ops.SWAP_MAX_CLASSES == GR.MAX_CLASSES == 64


# ---- the inputs and the emulation -----------------------------------------------------------------------

def test_case_classes_are_as_specified():
    unmatched = {}
    for name in GR.CASES:
        idx, _ = argmax = GR.argmax_rows(_masked(name))
        unmatched[name] = int((idx < 0).sum())
        assert argmax[1].shape == idx.shape
    print(f"unmatched content patches per case: {unmatched}")
    assert unmatched == {"g8_one_patch": 0, "g8_no_candidate": 1, "g48_bands": 0, "g64_bank_by_style": 0,
                         "g32_sky_takes_sky": 0, "g160_missing_class": 18, "g512_split_bank": 0}
    cc, sc = GR.case_classes("g64_bank_by_style")
    assert not bool((cc == 2).any()) and bool((sc[2] == 2).all())


@pytest.mark.parametrize("name", list(GR.CASES))
def test_near_ties_are_rare_in_the_reference(name):
    frac = GR.near_tie_fraction(_masked(name))
    print(f"{name}: {100 * frac:.2f} % of the content patches have an admissible runner-up within 2 * OP_TOL * S")
    assert frac <= GR.NEAR_TIE_MAX


@pytest.mark.parametrize("name", list(GR.CASES))
def test_emulation_meets_both_bars(name):
    c, s = GR.case_inputs(name)
    cc, sc = GR.case_classes(name)
    idx, best = GR.match(c, s, cc, sc, torch.float32)
    e_score, shortfall, wrong, disagree = GR.check_match(idx, best, _masked(name))
    print(f"{name}: fp32 emulation score error {e_score:.2e} S (bar {OP_TOL:.0e}), index shortfall {shortfall:.2e} S "
          f"(bar {2 * OP_TOL:.0e}), {wrong} wrong classes, {disagree} unmatched disagreements")
    assert e_score <= OP_TOL and shortfall <= 2 * OP_TOL and wrong == 0 and disagree == 0
    for alpha in (1.0, 0.6):
        e = SR.rel_inf(GR.gather(s, idx, c, alpha, torch.float32), GR.gather(s, idx, c, alpha))
        print(f"  gather alpha={alpha}: {e:.2e} (bar {GR.GATHER_TOL:.0e})")
        assert e <= GR.GATHER_TOL


# ---- C ABI ----------------------------------------------------------------------------------------------

P = 256   # a non-null "pointer": every call below must return before anything is launched or read
BIG = 1 << 40


def _match(L, ck=P, sk=P, inv=P, cc=P, sc=P, index=P, n=2, s=3, c=8, hc=4, wc=4, hs=4, ws=4, splits=0, flags=0,
           ws_ptr=P, nbytes=BIG):
    return L.ast_patch_match_guided_ex_f32(ck, sk, inv, cc, sc, index, None, n, s, c, hc, wc, hs, ws, splits, flags,
                                           ws_ptr, nbytes, None)


def _whole(L, ck=P, sv=P, cc=P, sc=P, out=P, n=2, s=3, c=8, hc=4, wc=4, hs=4, ws=4, ws_ptr=P, nbytes=BIG):
    return L.ast_style_swap_guided_f32(ck, P, sv, P, cc, sc, out, None, None, n, s, c, hc, wc, hs, ws, 1.0, ws_ptr,
                                       nbytes, None)


def _gather(L, sv=P, index=P, n=2, s=3, c=8, hc=4, wc=4, hs=4, ws=4):
    return L.ast_patch_gather_guided_f32(sv, index, P, P, n, s, c, hc, wc, hs, ws, 1.0, None)


@pytest.mark.parametrize("want,call", [
    (E_NULL, lambda L: _match(L, ck=None)),
    (E_NULL, lambda L: _match(L, cc=None)),
    (E_NULL, lambda L: _match(L, sc=None)),
    (E_NULL, lambda L: _match(L, index=None)),
    (E_NULL, lambda L: _match(L, ws_ptr=None)),
    (E_SHAPE, lambda L: _match(L, hc=2)),
    (E_SHAPE, lambda L: _match(L, ws=2)),
    (E_SHAPE, lambda L: _match(L, n=0)),
    (E_SHAPE, lambda L: _match(L, s=0)),
    (E_SHAPE, lambda L: _match(L, c=0)),
    (E_SHAPE, lambda L: _match(L, nbytes=16)),
    (E_SHAPE, lambda L: _match(L, s=65535, hs=202, ws=202)),        # S * Ns = 2.6e9 >= 2^31
    (E_UNSUPPORTED, lambda L: _match(L, c=1025)),
    (E_UNSUPPORTED, lambda L: _match(L, splits=-1)),
    (E_UNSUPPORTED, lambda L: _match(L, flags=2)),
    (E_NULL, lambda L: _whole(L, ck=None)),
    (E_NULL, lambda L: _whole(L, sv=None)),
    (E_NULL, lambda L: _whole(L, cc=None)),
    (E_NULL, lambda L: _whole(L, sc=None)),
    (E_NULL, lambda L: _whole(L, out=None)),
    (E_NULL, lambda L: _whole(L, ws_ptr=None)),
    (E_SHAPE, lambda L: _whole(L, wc=2)),
    (E_SHAPE, lambda L: _whole(L, hs=2)),
    (E_SHAPE, lambda L: _whole(L, s=0)),
    (E_SHAPE, lambda L: _whole(L, nbytes=512)),
    (E_SHAPE, lambda L: _whole(L, s=65535, hs=202, ws=202)),
    (E_UNSUPPORTED, lambda L: _whole(L, c=1025)),
    (E_NULL, lambda L: _gather(L, index=None)),
    (E_NULL, lambda L: _gather(L, sv=None)),
    (E_SHAPE, lambda L: _gather(L, hs=2)),
    (E_SHAPE, lambda L: _gather(L, s=65535, hs=202, ws=202)),
    (E_UNSUPPORTED, lambda L: _gather(L, c=1025)),
])
def test_bad_arguments_are_rejected_before_launch(want, call):
    assert call(_lib.lib()) == want


def test_workspace_queries():
    L = _lib.lib()
    _, n, s, _, (hc, wc), (hs, ws) = GR.CASES["g512_split_bank"]
    by_splits = [L.ast_patch_match_guided_workspace_bytes(n, s, hc, wc, hs, ws, k) for k in (1, 2, 4, 8)]
    assert by_splits[0] > 0 and by_splits == sorted(set(by_splits)), by_splits      # positive, strictly growing
    auto = L.ast_patch_match_guided_workspace_bytes(n, s, hc, wc, hs, ws, 0)
    assert auto > by_splits[0]                                                      # the library splits this shape
    # one content tile, 2 * 16 bank tiles: 33 masks of 8 bytes beside the score scratch
    assert by_splits[0] >= 4 * 64 + 8 * 33
    assert by_splits[0] > L.ast_patch_match_workspace_bytes(n, 1, hc, wc, hs, ws, 1)
    whole = L.ast_style_swap_guided_workspace_bytes(n, s, hc, wc, hs, ws)
    assert whole >= auto + 4 * s * 1024 + 4 * 64
    assert L.ast_style_swap_guided_workspace_bytes(2, 0, 4, 4, 4, 4) == E_SHAPE
    assert L.ast_style_swap_guided_workspace_bytes(2, 2, 4, 2, 4, 4) == E_SHAPE
    assert L.ast_style_swap_guided_workspace_bytes(1, 65535, 4, 4, 202, 202) == E_SHAPE
    assert L.ast_patch_match_guided_workspace_bytes(1, 65535, 4, 4, 202, 202, 0) == E_SHAPE
    assert L.ast_patch_match_guided_workspace_bytes(2, 2, 4, 4, 4, 4, -1) == E_UNSUPPORTED
    assert L.ast_style_swap_guided_workspace_bytes(2, 5, 4, 4, 4, 4) > 0            # any S: not tied to n


# ---- wiring ---------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ast_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ast_patch_match_guided_workspace_bytes", "ast_patch_match_guided_ex_f32",
                 "ast_patch_gather_guided_f32", "ast_style_swap_guided_workspace_bytes", "ast_style_swap_guided_f32"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert re.search(r"#define\s+AST_SWAP_MAX_CLASSES\s+64\b", src)
    assert re.search(r"#define\s+AST_SWAP_NO_SKIP\s+1\b", src)


def test_registered_op_and_meta_kernel():
    assert "style_swap_guided" in library.OPS
    assert library.OPS.index("style_swap_guided") == library.OPS.index("style_swap") + 1
    m = torch.device("meta")
    c, s = torch.empty(2, 16, 8, 12, device=m), torch.empty(3, 16, 5, 7, device=m)
    cc = torch.empty(2, 6, 10, device=m, dtype=torch.uint8)
    sc = torch.empty(3, 3, 5, device=m, dtype=torch.uint8)
    out = torch.ops.ast_hip.style_swap_guided(c, s, cc, sc, 0.6, True)
    assert out.shape == c.shape and out.dtype == c.dtype and out.device.type == "meta"


def test_model_surface():
    assert callable(getattr(models.AdaINStyleTransfer, "stylize_swap_regions"))
    assert models.AdaINStyleTransfer.TRANSFORMS == ("adain", "efdm", "wct")
    net = models.AdaINStyleTransfer(transform="efdm")
    assert not any("swap" in k for k in net.state_dict())
    for p in net.parameters():
        p.requires_grad_(False)
    img, sty = torch.zeros(1, 3, 32, 32), torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match="style_labels without labels"):
        net.stylize_swap_regions(img, sty, style_labels=torch.zeros(2, 32, 32, dtype=torch.uint8))
    with pytest.raises(ValueError):
        net.stylize_swap_regions(img[0], sty)


def test_cpu_tensors_bad_class_maps_and_gradients_are_rejected():
    x, bank = torch.rand(1, 4, 5, 5), torch.rand(2, 4, 6, 6)
    cc, sc = torch.zeros(1, 3, 3, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.HipOpError):
        ops.style_swap_guided(x, bank, cc, sc)
    with pytest.raises(_lib.HipOpError):
        ops.patch_match_guided(x, bank, cc, sc)
    with pytest.raises(_lib.HipOpError):
        ops.patch_gather_guided(bank, torch.zeros(1, 3, 3, dtype=torch.int32), x)
    # the class maps' dtype and shape, checked by the wrapper's own helper before anything is launched
    dev = torch.device("cpu")
    assert ops._swap_classes(None, (1, 3, 3), dev, "content_class").dtype == torch.uint8
    assert int(ops._swap_classes(None, (1, 3, 3), dev, "content_class").sum()) == 0
    for bad in (cc.int(), cc.float(), cc[:, :2], cc[0], [[0]]):
        with pytest.raises(_lib.HipOpError, match="content_class must be a uint8 tensor"):
            ops._swap_classes(bad, (1, 3, 3), dev, "content_class")
    with pytest.raises(_lib.HipOpError, match="style_class must be a uint8 tensor"):
        ops._swap_classes(sc, (3, 4, 4), dev, "style_class")
    assert ops._bank_patches(3, 34, 34, "x") == 3 * 1024
    with pytest.raises(_lib.HipOpError, match="2\\^31 or more"):      # S * Ns must fit the int32 index
        ops._bank_patches(65535, 202, 202, "patch_match_guided")
    net = models.AdaINStyleTransfer()
    with pytest.raises(NotImplementedError):          # the parameters ask for a gradient
        net.stylize_swap_regions(torch.zeros(1, 3, 32, 32), torch.zeros(2, 3, 32, 32))
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError):
        net.stylize_swap_regions(torch.zeros(1, 3, 32, 32).requires_grad_(), torch.zeros(2, 3, 32, 32))
