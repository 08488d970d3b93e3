"""CPU: the reference of the contextual loss (tests/cx_ref.py) on its own -- the conditions on the test
inputs, the analytic gradient against torch.autograd, the fp32 emulation against the bars -- and the
host-side surface of the op (header, bindings, workspace queries, registered op, trainer defaults)."""
import functools
import json
import os
import re

import pytest
import torch

import cx_ref as X
import remd_ref as R
from arbitrarystyletransfer_amd import _lib, functional, library, losses, ops, train  # noqa: F401  (registers the ops)

OP_TOL = X.OP_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ast_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cx_workspace_bytes.json")
ENTRY_POINTS = {"ast_cx_center_f32": 11, "ast_cx_rowsum_workspace_bytes": 5, "ast_cx_rowsum_f32": 17,
                "ast_cx_colmax_workspace_bytes": 4, "ast_cx_colmax_f32": 19, "ast_cx_value_f32": 7,
                "ast_cx_loss_workspace_bytes": 4, "ast_cx_loss_f32": 27, "ast_cx_loss_backward_workspace_bytes": 4,
                "ast_cx_loss_backward_f32": 23}


@functools.lru_cache(maxsize=None)
def _case(name):
    return X.case_inputs(name)


@functools.lru_cache(maxsize=None)
def _parts(name):
    x, y, h = _case(name)
    return X.parts(x, y, h)


@functools.lru_cache(maxsize=None)
def _kappa(name):
    return X.kappa(*_case(name))


def _grad_err(got, ref):
    """rel_inf, or the absolute error where the true gradient is zero (one target pixel: CX = 1 whatever x
    is) and the float64 reference holds 0 or rounding noise far below 1e-12."""
    return X.grad_err(got, ref)


# ---- the conditions on the inputs ---------------------------------------------------------------------

def test_cases_are_those_of_the_relaxed_emd():
    assert len(X.CASES) == len(R.CASES) + 2
    for name, (base, c, h) in X.CASES.items():
        x, y, _ = _case(name)
        bx, by = R.case_inputs(base)
        assert tuple(x.shape[2:]) == tuple(bx.shape[2:]) and tuple(y.shape[2:]) == tuple(by.shape[2:])
        if c == R.CASES[base][2]:
            assert torch.equal(x, bx) and torch.equal(y, by)
    assert sorted(h for _, _, h in X.CASES.values()).count(0.1) == 2


@pytest.mark.parametrize("name", X.ALL_CASES)
def test_input_conditions(name):
    x, y, h = _case(name)
    q, kap = _parts(name), _kappa(name)
    cols = X.col_near_tie_fraction(q["cx"], 4 * kap * OP_TOL)
    rows = R.near_tie_fraction(q["d"])
    act = X.active_fraction(q["a"], q["d"].shape[1])
    print(f"{name}: kappa OP_TOL {kap * OP_TOL:.2e} (max {X.KAPPA_TOL_MAX:.0e}); near-tie share columns {cols:.4f}, rows "
          f"{rows:.4f} (max {X.NEAR_TIE_MAX}); active rows {act:.2f}")
    assert kap * OP_TOL <= X.KAPPA_TOL_MAX
    assert cols <= X.NEAR_TIE_MAX and rows <= X.NEAR_TIE_MAX
    assert bool(torch.isfinite(q["cxb"]).all()) and float(q["cxb"].min()) > 0


def test_inactive_rows_and_long_lists_occur():
    q = _parts("c32_many_queries")
    act = X.active_fraction(q["a"], 460)
    q2 = _parts("c24_few_content")
    longest = int(torch.bincount(q2["a"][0], minlength=4).max())
    print(f"c32_many_queries: {act:.2%} of the rows active; c24_few_content: longest inverse list {longest}")
    assert act <= 42 / 460 and longest >= 77


# ---- the analytic gradient ------------------------------------------------------------------------------

@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("name", X.ALL_CASES)
def test_analytic_gradient_equals_autograd(name, center):
    x, y, h = _case(name)
    xd = x.double().requires_grad_(True)
    (auto,) = torch.autograd.grad(X.loss_dense(xd, y, weight=0.7, h=h, center_on=center), xd)
    ana = X.grad(x, y, weight=0.7, h=h, center_on=center)
    err = _grad_err(ana, auto)
    print(f"{name} center={center}: analytic vs autograd {err:.2e}; max |grad| {float(auto.abs().max()):.2e}")
    assert err <= 1e-12


# ---- the fp32 emulation meets the bars --------------------------------------------------------------------

@pytest.mark.parametrize("name", X.ALL_CASES)
def test_fp32_emulation_meets_the_bars(name):
    x, y, h = _case(name)
    q, kap = _parts(name), _kappa(name)
    bar = kap * OP_TOL
    e = X.parts(x, y, h, torch.float32)
    e_s = float(((e["S"].double() - q["S"]) / q["S"]).abs().max())
    e_e = float(((e["E"].double() - q["E"]) / q["E"]).abs().max())
    at = q["cx"].transpose(1, 2).gather(2, e["a"][..., None])[..., 0]
    e_c = float(((e["c"].double() - at) / at).abs().max())
    short = float((at / q["c"]).min())
    e_l = float((torch.log(e["cxb"].double()) - torch.log(q["cxb"])).abs().max())
    idx = (q["m"], q["a"])
    e_g = _grad_err(X.grad(x, y, 0.8, 1.5, h, torch.float32, idx), X.grad(x, y, 0.8, 1.5, h, index=idx))
    print(f"{name} fp32 emulation: S {e_s:.2e}, E {e_e:.2e} (bar {bar:.2e}); col_cx {e_c:.2e} (bar {2 * bar:.2e}); value "
          f"at the index / maximum {short:.6f}; -log CX {e_l:.2e}; gradient {e_g:.2e} (a quarter of the bar "
          f"{bar:.2e})")
    assert max(e_s, e_e) <= bar and e_c <= 2 * bar and short >= 1 - 4 * bar and e_l <= 2 * bar
    assert e_g <= bar          # a quarter of 4 kappa OP_TOL


# ---- special inputs ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_style_pixel_is_exact(dtype):
    x = X.features(12900, (1, 16, 5, 7))
    y = X.features(12901, (1, 16, 1, 1))
    q = X.parts(x, y, 0.5, dtype, center_on=False)
    assert torch.all(q["c"] == 1.0) and float(X.loss(x, y, dtype=dtype, center_on=False)[0]) == 0.0


def test_argmax_rules():
    v = torch.tensor([[[float("nan"), 2.0, 2.0], [float("nan"), float("nan"), float("nan")]]])
    m, i = X.argmax_last(v)
    assert i.tolist() == [[1, 0]] and m.tolist() == [[2.0, float("-inf")]]


# ---- the host-side surface ----------------------------------------------------------------------------------

def test_c_abi_and_bindings():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name), name
    assert int(re.search(r"#define\s+AST_CX_MAX_C\s+(\d+)", src).group(1)) == ops.CX_MAX_C
    assert int(re.search(r"#define\s+AST_CX_MAX_PIXELS\s+(\d+)", src).group(1)) == ops.CX_MAX_PIXELS
    assert float(re.search(r"#define\s+AST_CX_EPS\s+([0-9.e-]+)f", src).group(1)) == ops.CX_EPS == X.EPS
    declared = set(re.findall(r"\b(ast_cx_\w+)\s*\(", src))
    assert declared == set(ENTRY_POINTS)


def test_workspace_queries_against_golden():
    golden = json.load(open(GOLDEN))
    L = _lib.lib()
    queries = {n for n in ENTRY_POINTS if n.endswith("_workspace_bytes")}
    assert set(golden) == queries
    for name, rows in golden.items():
        values = [r["bytes"] for r in rows]
        assert any(v > 0 for v in values) and any(v < 0 for v in values), name     # accepted and rejected tuples
        for r in rows:
            assert int(getattr(L, name)(*r["args"])) == r["bytes"], (name, r)


def test_workspace_formulas():
    L = _lib.lib()
    # 12 bytes per (content tile, style pixel); 8 per (split, content pixel); 256-byte aligned regions
    assert L.ast_cx_colmax_workspace_bytes(16, 16, 4096, 4096) == 12 * 16 * 64 * 4096
    assert L.ast_cx_colmax_workspace_bytes(1, 1, 1, 1) == 3 * 256
    assert L.ast_cx_rowsum_workspace_bytes(16, 16, 4096, 4096, 2) == 8 * 16 * 2 * 4096
    n, ns, _, (h, w), (hs, ws) = R.CASES["c512_split_keys"]
    auto, one = (L.ast_cx_rowsum_workspace_bytes(n, ns, h * w, hs * ws, k) for k in (0, 1))
    assert auto > one > 0                                                          # the library splits the style side
    # the whole loss: the match's unused column outputs and the largest stage
    stage = max(L.ast_cosine_match_workspace_bytes(16, 16, 4096, 4096, 0), L.ast_cx_colmax_workspace_bytes(16, 16, 4096, 4096),
                L.ast_cx_rowsum_workspace_bytes(16, 16, 4096, 4096, 0))
    assert L.ast_cx_loss_workspace_bytes(16, 16, 4096, 4096) == 8 * 16 * 4096 + stage
    # the backward: lists, row scalars and flags, G
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    want = (al(4 * 16 * 4097) + 2 * al(4 * 16 * 4096) + al(12 * 16 * 4096) + al(4 * 16 * 4096) + al(4 * 16 * 64)
            + al(4 * 16 * 512 * 4096))
    assert L.ast_cx_loss_backward_workspace_bytes(16, 512, 4096, 4096) == want


def test_host_checks_reject_before_launch():
    L = _lib.lib()
    assert L.ast_cx_loss_workspace_bytes(2, 3, 4, 4) == -2                         # a target batch neither N nor 1
    assert L.ast_cx_loss_workspace_bytes(1, 1, 0, 4) == -2                         # an empty map
    assert L.ast_cx_loss_workspace_bytes(1, 1, ops.CX_MAX_PIXELS + 1, 4) == -2
    assert L.ast_cx_rowsum_workspace_bytes(1, 1, 4, 4, -1) == -3
    assert L.ast_cx_colmax_workspace_bytes(65536, 1, 4, 4) == -2
    assert L.ast_cx_loss_backward_workspace_bytes(1, ops.CX_MAX_C + 1, 4, 4) == -3
    assert L.ast_cx_loss_backward_workspace_bytes(1, 0, 4, 4) == -2
    assert L.ast_cx_center_f32(None, None, None, None, None, 1, 1, 8, 4, 4, None) == -1
    assert L.ast_cx_value_f32(None, None, None, 1, 4, 1.0, None) == -1
    # the checks run before any pointer is read or any launch is made: non-null dummies, bad arguments
    p = 256
    assert L.ast_cx_rowsum_f32(p, p, p, p, p, p, p, 1, 1, 8, 4, 4, 0.0, 0, p, 1 << 20, None) == -3          # h = 0
    assert L.ast_cx_rowsum_f32(p, p, p, p, p, p, p, 1, 1, 8, 4, 4, -1.0, 0, p, 1 << 20, None) == -3
    assert L.ast_cx_rowsum_f32(p, p, p, p, p, p, p, 1, 1, 8, 4, 4, float("inf"), 0, p, 1 << 20, None) == -3
    assert L.ast_cx_rowsum_f32(p, p, p, p, p, p, p, 1, 1, 8, 4, 4, float("nan"), 0, p, 1 << 20, None) == -3
    assert L.ast_cx_rowsum_f32(p, p, p, p, p, p, p, 1, 1, 8, 4, 4, 0.5, 0, p, 16, None) == -2               # short workspace
    assert L.ast_cx_colmax_f32(p, p, p, p, p, p, p, p, p, 1, 1, 8, 4, 4, 0.5, 0, p, 16, None) == -2
    assert L.ast_cx_colmax_f32(p, p, p, p, p, p, p, p, p, 1, 1, 8, 4, 4, 0.5, -1, p, 1 << 20, None) == -3
    assert L.ast_cx_loss_f32(*([p] * 16), 1, 1, 8, 4, 4, 1.0, 0.5, 1, p, 16, None) == -2
    assert L.ast_cx_loss_f32(*([p] * 16), 1, 1, 8, 4, 4, 1.0, 0.0, 1, p, 1 << 20, None) == -3
    assert L.ast_cx_loss_f32(p, p, None, None, None, *([p] * 11), 1, 1, 8, 4, 4, 1.0, 0.5, 1, p, 1 << 20, None) == -1
    assert L.ast_cx_loss_f32(*([p] * 16), 1, 1, ops.CX_MAX_C + 1, 4, 4, 1.0, 0.5, 1, p, 1 << 20, None) == -3
    assert L.ast_cx_loss_backward_f32(*([p] * 13), 1, 1, 8, 4, 4, 1.0, 0.5, p, 16, None) == -2
    assert L.ast_cx_loss_backward_f32(*([p] * 13), 1, 1, 8, 4, 4, 1.0, -0.5, p, 1 << 20, None) == -3
    assert L.ast_cx_loss_backward_f32(*([p] * 13), 2, 3, 8, 4, 4, 1.0, 0.5, p, 1 << 20, None) == -2


def test_cpu_tensors_and_bad_bandwidths_are_rejected():
    x, y = torch.zeros(1, 8, 2, 2), torch.zeros(1, 8, 2, 2)
    for call in (lambda: ops.cx_loss(x, y), lambda: ops.cx_center(x, y), lambda: losses.compute_contextual_loss(x, y)):
        with pytest.raises(_lib.HipOpError):
            call()


def test_registered_op_and_meta_kernel():
    assert library.OPS[library.OPS.index("selfsim_loss") + 1] == "cx_loss"
    assert re.search(r"^cx_loss\s.*d x", library.__doc__, flags=re.M)              # the table of the docstring
    assert "compute_contextual_loss" in losses.__all__
    m = torch.device("meta")
    x, y = torch.empty(2, 16, 5, 7, device=m), torch.empty(1, 16, 4, 3, device=m)
    for center in (True, False):
        out = torch.ops.ast_hip.cx_loss(x, y, 1.0, 0.5, center)
        maps = [(2, 16, 5, 7), (1, 16, 4, 3)] if center else [(0,), (0,)]
        shapes = [()] + maps + [(2, 5, 7), (1, 4, 3), (2, 5, 7), (2, 5, 7), (2, 5, 7), (2, 5, 7), (2, 4, 3), (2, 4, 3),
                                (2, 4, 3), (2,)]
        dtypes = [torch.float32] * 6 + [torch.int32] + [torch.float32] * 3 + [torch.int32] + [torch.float32] * 2
        assert [tuple(t.shape) for t in out] == shapes and [t.dtype for t in out] == dtypes
        assert all(t.device.type == "meta" for t in out)


def test_trainer_defaults_launch_nothing_new():
    a = train.default_args()
    assert a.cx_lam == 0.0 and a.cx_content_lam == 0.0 and a.cx_h == 0.5
    assert tuple(a.cx_taps) == ("relu_9", "relu_15") and tuple(a.cx_content_taps) == ("relu_15",)
    assert all(t in train._TAPS for t in tuple(a.cx_taps) + tuple(a.cx_content_taps))
    with pytest.raises(ValueError):
        train._tap_index("relu_99", "cx_taps")
