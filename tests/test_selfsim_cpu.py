"""CPU: the reference of the self-similarity content loss (tests/selfsim_ref.py) on its own -- the
conditions on the test inputs, the analytic gradient against torch.autograd, the fp32 emulation against
the bars -- and the host-side surface of the op (header, bindings, registered op, limits, trainer)."""
import functools
import inspect
import os
import re

import pytest
import torch

import selfsim_ref as R
from arbitrarystyletransfer_amd import _lib, library, losses, ops, train  # noqa: F401  (library registers the ops)

OP_TOL = R.OP_TOL
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")
ENTRY_POINTS = {"ast_selfsim_colsum_workspace_bytes": 2, "ast_selfsim_colsum_f32": 9,
                "ast_selfsim_pairs_workspace_bytes": 2, "ast_selfsim_pairs_f32": 16, "ast_selfsim_total_f32": 5,
                "ast_selfsim_loss_workspace_bytes": 3, "ast_selfsim_loss_f32": 18,
                "ast_selfsim_loss_backward_workspace_bytes": 3, "ast_selfsim_loss_backward_f32": 15}


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.case_inputs(name)


# ---- the conditions on the inputs ---------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_input_conditions(name):
    x, c = _case(name)
    assert float(R.inv_norms(x).min()) > 0 and float(R.inv_norms(c).min()) > 0      # no zero vector
    share = R.near_tie_fraction(x, c)
    print(f"{name}: share of off-diagonal pairs inside the sign margin {share:.4%} (max {R.NEAR_TIE_MAX:.0%})")
    if name not in R.DEGENERATE:
        assert share <= R.NEAR_TIE_MAX


def test_degenerate_cases():
    x, c = _case("s8_one_pixel")
    l, per = R.loss(x, c)
    assert float(l) == 0.0 and float(R.grad(x, c).abs().max()) == 0.0 and float(R.colsum(x)) == 0.0
    x, c = _case("s8_two_pixels")
    e = R.differences(x, c)[0]
    print(f"s8_two_pixels: max |e| {float(e.abs().max()):.2e}")
    assert float(R.loss(x, c)[0]) <= OP_TOL


# ---- the analytic gradient ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_analytic_gradient_equals_autograd(name):
    x, c = _case(name)
    xd = x.double().requires_grad_(True)
    (auto,) = torch.autograd.grad(R.loss_dense(xd, c, weight=0.7), xd)
    ana = R.grad(x, c, weight=0.7)
    err = float((auto - ana).abs().max())
    print(f"{name}: |analytic - autograd| = {err:.2e}; max |grad| {float(ana.abs().max()):.2e}")
    assert err <= 1e-10


# ---- the fp32 emulation meets the bars --------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_emulation_meets_the_bars(name):
    x, c = _case(name)
    npix = x.shape[2] * x.shape[3]
    e_r = max(float((R.colsum_fast(f, torch.float32).double() - R.colsum(f)).abs().max()) for f in (x, c))
    l64, per64 = R.loss(x, c)
    l32, per32 = R.loss(x, c, dtype=torch.float32)
    e_l = max(abs(float(l32) - float(l64)), float((per32.double() - per64).abs().max()))
    e32, _, _, _ = R.differences(x, c, torch.float32)
    e64, _, qx, qc = R.differences(x, c)
    e_e = float(((e32.double() - e64).abs() / (qx + qc)[:, None, :].clamp_min(1e-300)).max()) if npix > 1 else 0.0
    s32 = R.sign_of(e32).double()
    wrong, outside = R.check_signs(s32, x, c)
    e_t = float((R.signed_sums(x, c, torch.float32).double() - R.signed_sums(x, c, signs=s32)).abs().max())
    e_g = R.grad_error(R.grad(x, c, dtype=torch.float32, signs=s32), x, c, signs=s32)
    print(f"{name} fp32 emulation: column sums {e_r:.2e} (bar {OP_TOL * npix:.1e}), loss {e_l:.2e}, e within "
          f"{e_e:.2e} (q_x + q_c), {wrong} signs differ ({outside} outside the margin), t {e_t:.2e}, gradient "
          f"{e_g:.2e} (bar {OP_TOL:.0e})")
    assert e_r <= OP_TOL * npix and e_l <= OP_TOL and outside == 0 and e_t <= OP_TOL and e_g <= OP_TOL


# ---- equal maps, zero vectors -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_equal_maps_give_zero(dtype):
    x, _ = _case("s64_tiles")
    l, per = R.loss(x, x.clone(), dtype=dtype)
    assert float(l) == 0.0 and float(per.abs().max()) == 0.0
    assert float(R.grad(x, x.clone(), dtype=dtype).abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_zero_vectors(dtype):
    x = R.features(12900, (1, 8, 3, 4)) + 0.01
    c = R.features(12901, (1, 8, 3, 4)) + 0.01
    x[:, :, 1, 2] = 0.0           # pixel 6
    d = R.distances(x, dtype)
    others = [i for i in range(12) if i != 6]
    assert torch.all(d[0, 6, others] == 1.0) and torch.all(d[0, others, 6] == 1.0) and float(d[0, 6, 6]) == 0.0
    g = R.grad(x, c, dtype=dtype)
    assert torch.all(g[0, :, 1, 2] == 0.0) and torch.isfinite(g).all()
    xd = x.double().requires_grad_(True)
    (auto,) = torch.autograd.grad(R.loss_dense(xd, c), xd)
    assert torch.all(auto[0, :, 1, 2] == 0.0)


def test_plane_unpacker():
    pos = torch.tensor([[[0b0110, 0], [-(1 << 63), 1]]], dtype=torch.int64)   # [1, 2, 2]: 2 rows, 128 columns; bit 63
    neg = torch.tensor([[[0b1000, 0], [0, 2]]], dtype=torch.int64)
    s, stray = R.unpack_planes(pos, neg, 100)
    assert s.shape == (1, 2, 100) and stray == 0
    assert s[0, 0, :5].tolist() == [0.0, 1.0, 1.0, -1.0, 0.0] and s[0, 1, 63:66].tolist() == [1.0, 1.0, -1.0]
    assert R.unpack_planes(pos, neg, 65)[1] == 1


# ---- the host-side surface ----------------------------------------------------------------------------------

def test_c_abi_and_bindings():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name), name
    assert int(re.search(r"#define\s+AST_SELFSIM_MAX_PIXELS\s+(\d+)", src).group(1)) == ops.SELFSIM_MAX_PIXELS == 16384


def test_host_checks_reject_before_launch():
    L = _lib.lib()
    big = ops.SELFSIM_MAX_PIXELS + 1
    assert L.ast_selfsim_pairs_workspace_bytes(1, 0) == -2                   # an empty map
    assert L.ast_selfsim_pairs_workspace_bytes(1, big) == -2
    assert L.ast_selfsim_pairs_workspace_bytes(65536, 4) == -2
    assert L.ast_selfsim_loss_workspace_bytes(1, ops.REMD_MAX_C + 1, 4) == -3
    assert L.ast_selfsim_loss_workspace_bytes(1, 0, 4) == -2
    assert L.ast_selfsim_loss_backward_workspace_bytes(1, 8, big) == -2
    assert L.ast_selfsim_colsum_workspace_bytes(1, ops.REMD_MAX_C + 1) == -3
    # 4 bytes per (tile, pixel) and per tile pair, 256-byte aligned; the backward holds G
    assert L.ast_selfsim_pairs_workspace_bytes(1, 64) == 2 * 256
    assert L.ast_selfsim_pairs_workspace_bytes(16, 4096) == 4 * 16 * 64 * 4096 + 4 * 16 * 2080
    assert L.ast_selfsim_loss_backward_workspace_bytes(16, 512, 4096) == 4 * 16 * 512 * 4096
    assert (L.ast_selfsim_loss_workspace_bytes(2, 48, 63)
            == L.ast_selfsim_colsum_workspace_bytes(2, 48) + L.ast_selfsim_pairs_workspace_bytes(2, 63))
    p = 256                                                                  # a non-null pointer, never followed
    assert L.ast_selfsim_colsum_f32(None, p, p, 1, 8, 4, p, 1 << 20, None) == -1
    assert L.ast_selfsim_pairs_f32(p, p, p, p, p, p, p, p, None, p, 1, 8, 4, p, 1 << 20, None) == -1
    assert L.ast_selfsim_total_f32(p, None, 1, 1.0, None) == -1
    assert L.ast_selfsim_loss_f32(p, p, p, p, p, p, p, p, p, p, None, 1, 8, 4, 1.0, p, 1 << 20, None) == -1
    assert L.ast_selfsim_loss_backward_f32(p, p, p, p, p, p, None, p, 1, 8, 4, 1.0, p, 1 << 20, None) == -1
    for n, ch, pix, want in ((1, 8, 0, -2), (1, 8, big, -2), (1, ops.REMD_MAX_C + 1, 4, -3), (0, 8, 4, -2)):
        assert L.ast_selfsim_colsum_f32(p, p, p, n, ch, pix, p, 1 << 40, None) == want
        assert L.ast_selfsim_pairs_f32(p, p, p, p, p, p, p, p, p, p, n, ch, pix, p, 1 << 40, None) == want
        assert L.ast_selfsim_loss_f32(p, p, p, p, p, p, p, p, p, p, p, n, ch, pix, 1.0, p, 1 << 40, None) == want
        assert L.ast_selfsim_loss_backward_f32(p, p, p, p, p, p, p, p, n, ch, pix, 1.0, p, 1 << 40, None) == want
    short = L.ast_selfsim_loss_workspace_bytes(1, 8, 4) - 1                  # a short workspace
    assert L.ast_selfsim_loss_f32(p, p, p, p, p, p, p, p, p, p, p, 1, 8, 4, 1.0, p, short, None) == -2
    assert L.ast_selfsim_pairs_f32(p, p, p, p, p, p, p, p, p, p, 1, 8, 4, p, 0, None) == -2
    assert L.ast_selfsim_colsum_f32(p, p, p, 1, 8, 4, p, 0, None) == -2
    assert L.ast_selfsim_loss_backward_f32(p, p, p, p, p, p, p, p, 1, 8, 4, 1.0, p, 0, None) == -2


def test_cpu_tensors_are_rejected():
    x, c = torch.zeros(1, 8, 2, 2), torch.zeros(1, 8, 2, 2)
    u = torch.zeros(1, 2, 2)
    for call in (lambda: ops.selfsim_loss(x, c), lambda: ops.selfsim_colsum(x, u),
                 lambda: ops.selfsim_pairs(x, c, u, u, u, u), lambda: ops.selfsim_total(torch.zeros(1)),
                 lambda: ops.selfsim_loss_backward(x, (u,) * 7, torch.tensor(1.0)),
                 lambda: losses.compute_selfsim_loss(x, c)):
        with pytest.raises(_lib.HipOpError):
            call()


def test_registered_op_and_meta_kernel():
    assert library.OPS[library.OPS.index("remd_loss") + 1] == "selfsim_loss"
    assert re.search(r"^selfsim_loss\s.*d x", library.__doc__, flags=re.M)       # the table of the docstring
    assert "compute_selfsim_loss" in losses.__all__
    m = torch.device("meta")
    x, c = torch.empty(2, 16, 5, 13, device=m), torch.empty(2, 16, 5, 13, device=m)
    out = torch.ops.ast_hip.selfsim_loss(x, c, 1.0)
    shapes = [(), (2,)] + [(2, 5, 13)] * 5 + [(2, 65, 2)] * 2
    dtypes = [torch.float32] * 7 + [torch.int64] * 2
    assert [tuple(t.shape) for t in out] == shapes and [t.dtype for t in out] == dtypes
    assert all(t.device.type == "meta" for t in out)


def test_trainer_defaults_launch_nothing_new():
    a = train.default_args()
    assert a.selfsim_lam == 0.0 and tuple(a.selfsim_taps) == ("relu_9", "relu_15")
    assert all(t in train._TAPS for t in a.selfsim_taps)
    with pytest.raises(ValueError, match="selfsim_taps"):
        train._tap_index("relu_99", "selfsim_taps")
    with pytest.raises(ValueError, match="remd_taps"):
        train._tap_index("relu_99")
    # the one call of the loss sits behind the test of selfsim_lam, and takes the content half of the taps
    src = inspect.getsource(train.AdaINTrainer.compute_losses)
    assert src.count("compute_selfsim_loss") == 1
    guard, call = src.index("if selfsim_lam > 0:"), src.index("compute_selfsim_loss")
    assert guard < call and "\n        if " not in src[guard + 1:call]
    assert "compute_selfsim_loss(s_taps[i], taps[i][:b])" in src
