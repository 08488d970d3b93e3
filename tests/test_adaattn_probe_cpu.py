"""CPU: the AdaAttN probe constructions (tests/adaattn_probe_ref.py) are what they claim to be, and
their bounds separate a clean bf16 pipeline from a structurally wrong one.

  * every case satisfies the helper's conditions (bf16-exact V and V^2, zero-sum planes, distinct
    columns, the 128-nat margin, coverage of pi and of the twin placements): the builders assert them;
  * a plain torch emulation of the bf16 pipeline (Q, K, V, V^2, P rounded to bf16, fp32 sums, the
    planned key splits merged) is inside the bounds on every case;
  * each planted defect -- one padded key counted, the last key dropped, two keys of a 16-group
    exchanged in V only, one split merged with weight 1, query tile t reading tile t ^ 1 -- is
    outside them on every case it applies to (for the uniform probe at Nk > 1000 a miscounted key
    moves the output by about a bf16 half-ulp, so there a defect shows as a share of elements out
    of bounds: > 1 %, against exactly none for the clean emulation);
  * ast_adaattn_plan puts every case on the kernel the table names.
"""
import ctypes

import pytest
import torch

import adaattn_probe_ref as P
from arbitrarystyletransfer_amd import _lib

ALL_CASES = P.CASES + P.MEAN_CASES
IDS = [P.case_id(c) for c in P.CASES]


def _plan(case):
    return P.plan(1, case[0])


def _probe(kind, case):
    if kind == "uniform":
        return P.uniform(case[0], with_mean=case in P.MEAN_CASES)
    if kind == "planted":
        return P.planted(case[0])
    pl = _plan(case)
    return P.twin(case[0], pl.kchunk * 32 if pl.ksplit > 1 else 0)


def _applies(defect, kind, case, pl):
    (n, c, hc, wc, hs, ws) = case[0]
    nk = hs * ws
    if defect == "pad":      # a padded key has logit 0: only the uniform probe gives it a weight
        return kind == "uniform" and nk % 32 != 0
    if defect == "drop":
        return True
    if defect == "vswap":    # a sum over all keys does not see two of them exchanged
        return kind != "uniform"
    if defect == "merge":    # uniform: every split has the same maximum, weight 1 is right
        return kind != "uniform" and pl.ksplit > 1
    if defect == "qtile":    # uniform: K = 0, the output does not depend on Q
        return kind != "uniform" and hc * wc > pl.waves * 32
    raise AssertionError(defect)


@pytest.mark.parametrize("case", ALL_CASES, ids=[P.case_id(c) for c in ALL_CASES])
def test_plan_is_the_tabled_kernel(case):
    shape, waves, split, _ = case
    pl = _plan(case)
    assert pl.waves == waves and (pl.ksplit > 1) == split, (shape, vars(pl))
    n, c, hc, wc, hs, ws = shape
    assert pl.nqp % (pl.waves * 32) == 0 and pl.nqp >= hc * wc and pl.nkp % 32 == 0 and 0 <= pl.nkp - hs * ws < 32
    assert pl.kchunk * pl.ksplit >= pl.nkp // 32 > pl.kchunk * (pl.ksplit - 1)     # every split non-empty
    f = P.plan(0, shape)
    assert f.waves == 4 and f.nqp % 128 == 0 and f.nkp == pl.nkp


def test_plan_rejects_what_the_forward_rejects():
    L = _lib.lib()
    o = [ctypes.c_int(0) for _ in range(5)]
    ptrs = [ctypes.addressof(x) for x in o]
    assert L.ast_adaattn_plan(1, 1, 32, 4, 4, 4, 4, *ptrs) == 0 and o[0].value == 4
    assert L.ast_adaattn_plan(1, 0, 32, 4, 4, 4, 4, *ptrs) == -2       # AST_E_SHAPE
    assert L.ast_adaattn_plan(1, 1, 32, 4, 0, 4, 4, *ptrs) == -2
    assert L.ast_adaattn_plan(2, 1, 32, 4, 4, 4, 4, *ptrs) == -3       # AST_E_UNSUPPORTED: dtype
    assert L.ast_adaattn_plan(0, 1, 129, 4, 4, 4, 4, *ptrs) == -3      # c > 128
    assert L.ast_adaattn_plan(0, 1, 32, 1 << 15, 1 << 14, 4, 4, *ptrs) == -2
    assert L.ast_adaattn_plan(0, 1, 32, 4, 4, 4, 4, None, *ptrs[1:]) == -1


def test_the_table_reaches_every_kernel_form():
    """attend_bf16_kernel<1..4, 8>, the 4-wave unsplit many-block path and the split path."""
    seen = set()
    for case in P.CASES:
        (n, c, hc, wc, hs, ws), pl = case[0], _plan(case)
        seen.add((pl.waves, (c + 31) // 32, pl.ksplit > 1, pl.nkp // 32 >= 32))
    assert {(8, ct, False, False) for ct in (1, 2, 3, 4)} <= seen
    assert (4, 1, False, True) in seen and any(w == 4 and s for w, _, s, _ in seen)


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_probe_conditions(case):
    """The builders assert their own conditions; here: what they report."""
    shape = case[0]
    n, c, hc, wc, hs, ws = shape
    nk, pl = hs * ws, _plan(case)
    pr = _probe("planted", case)
    assert pr.margin >= P.MARGIN_NATS and set(pr.must) <= set(pr.pi.flatten().tolist())
    blk = min(k for k in pr.must if k not in (0, nk - 1)) // 32
    assert {0, nk - 1} | {32 * blk + p for p in (3, 4, 7, 8, 11, 12, 15, 16) if 32 * blk + p < nk} == set(pr.must)
    tw = _probe("twin", case)
    assert tw.margin >= P.MARGIN_NATS
    want = {"same16": True, "blocks": nk > 32, "splits": pl.ksplit > 1, "adjacent_splits": pl.ksplit > 1, "last": True}
    assert tw.placements == want, (tw.placements, want)
    un = _probe("uniform", case)
    assert float(un.ref.abs().max()) > 0 and float(un.slack.min()) >= 0


COMBOS = [(c, k) for c in P.CASES for k in ("uniform", "planted", "twin")] + [(c, "uniform") for c in P.MEAN_CASES]


@pytest.mark.parametrize("case,kind", COMBOS, ids=[f"{P.case_id(c)}-{k}" for c, k in COMBOS])
def test_clean_emulation_inside_and_defects_outside(case, kind):
    (n, c, hc, wc, hs, ws), pl = case[0], _plan(case)
    nk = hs * ws
    pr = _probe(kind, case)

    def outside(defect):
        out = P.emulate_bf16(pr, pl, defect)
        if kind == "planted":
            return (out.double() != pr.ref).double().mean().item()
        return (P.err_over_bound(out, pr, torch.bfloat16)[1] > 1).double().mean().item()

    assert outside(None) == 0.0, (kind, case[0])
    for defect in P.DEFECTS:
        if not _applies(defect, kind, case, pl):
            continue
        share = outside(defect)
        floor = 0.01 if (kind == "uniform" and nk > 1000) else 0.0
        assert share > floor, (kind, defect, case[0], share)
