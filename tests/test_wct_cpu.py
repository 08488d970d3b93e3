"""CPU: the whitening and colouring transform's definition (tests/wct_ref.py), the fp32 emulation of the
library's Newton-Schulz iteration against the float64 eigh reference, the default iteration count,
the model wiring, the C ABI's argument checks and the registered op's meta kernel. No GPU needed:
nothing is launched."""
import functools

import pytest
import torch

import wct_ref as WR
from arbitrarystyletransfer_amd import _lib, library, models, ops  # noqa: F401  (library registers the ops)

E_SHAPE, E_UNSUPPORTED = -2, -3


# ---- the definition ---------------------------------------------------------------------------------

def test_output_takes_the_style_mean_and_covariance():
    """Full-rank content, a ridge of 1e-12 relative: the transformed map has the style's mean and
    covariance (float64, 1e-6)."""
    g = torch.Generator().manual_seed(7900)
    c = torch.randn(2, 6, 9, 11, generator=g, dtype=torch.float64) * 2.0 + 1.0
    s = torch.randn(2, 6, 8, 8, generator=g, dtype=torch.float64) @ torch.randn(8, 8, generator=g, dtype=torch.float64)
    out = WR.wct(c, s, 1.0, 1e-12)
    mu_o, cov_o, _ = WR.mean_cov(out, 0.0)
    mu_s, cov_s, _ = WR.mean_cov(s, 0.0)
    em, ec = WR.rel_inf(mu_o, mu_s), WR.rel_inf(cov_o, cov_s)
    print(f"mean rel_inf {em:.2e}, covariance rel_inf {ec:.2e}")
    assert em <= 1e-6 and ec <= 1e-6
    half = WR.wct(c, s, 0.5, 1e-12)
    assert WR.rel_inf(half, 0.5 * out + 0.5 * c) <= 1e-12


def test_constant_content_map_gives_the_style_mean():
    s = WR.features(7901, (1, 8, 6, 6))
    c = torch.full((1, 8, 5, 7), 0.3)
    mu_s = WR.mean_cov(s, 1e-3)[0]
    for out in (WR.wct(c, s), WR.wct_emulated(c, s)):
        assert bool(torch.isfinite(out).all())
        assert WR.rel_inf(out, mu_s[:, :, None, None].expand_as(c)) <= 1e-6
    assert float(WR.mean_cov(c, 1e-3, torch.float32)[2]) == pytest.approx(1e-23, rel=1e-6)


# ---- the emulation against the reference --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _e_cpu(name, alpha, eps_rel):
    c, s = WR.case_inputs(name)
    return WR.rel_inf(WR.wct_emulated(c, s, alpha, eps_rel), WR.wct(c, s, alpha, eps_rel))


@pytest.mark.parametrize("eps_rel", [1e-3, 1e-4])
@pytest.mark.parametrize("name", list(WR.CASES))
def test_emulation_reaches_the_reference_at_the_default_count(name, eps_rel):
    """The fp32 iteration at wct_default_iters against float64 eigh. E_CPU_MAX is the precondition
    of the GPU bars (max(4 e_cpu, OP_TOL), never above FP32_BAR): 4 * 2.5e-4 stays under 1e-3."""
    for alpha in (1.0, 0.6):
        e = _e_cpu(name, alpha, eps_rel)
        print(f"{name} eps_rel={eps_rel:g} alpha={alpha}: e_cpu {e:.2e} "
              f"({WR.default_iters(WR.CASES[name][2], eps_rel)} iterations)")
        assert e <= WR.E_CPU_MAX <= WR.FP32_BAR / 4


def test_truncation_error_at_the_default_count_and_four_steps_earlier():
    """Rank-1 covariance plus the ridge (the slowest case) in float64: converged at the formula's
    count, visibly not four steps before."""
    for c in (8, 64, 512):
        g = torch.Generator().manual_seed(7902 + c)
        v = torch.randn(c, 1, generator=g, dtype=torch.float64)
        cov = v @ v.T
        cov = cov + 1e-3 * (cov.trace() / c) * torch.eye(c, dtype=torch.float64)
        ref = WR.eigh_roots(cov)[1]
        n = WR.default_iters(c, 1e-3)
        at, before = (WR.rel_inf(WR.newton_schulz_roots(cov[None], k)[1][0], ref) for k in (n, n - 4))
        print(f"C={c}: {n} iterations {at:.1e}, {n - 4} iterations {before:.1e}")
        assert at <= 5e-9 and before >= 1e-3   # four steps fewer would already miss the fp32 bar


def test_default_iters_matches_the_formula():
    assert ops.wct_default_iters(512, 1e-3) == WR.default_iters(512, 1e-3) == 22
    assert ops.wct_default_iters(48, 1e-3) == WR.default_iters(48, 1e-3) == 19
    for c, e in ((1, 1.0), (8, 1e-2), (160, 1e-4), (1024, 1e-4)):
        assert ops.wct_default_iters(c, e) == WR.default_iters(c, e), (c, e)
    with pytest.raises(_lib.HipOpError):
        ops.wct_default_iters(512, 1e-5)
    with pytest.raises(_lib.HipOpError):
        ops.wct_default_iters(2048, 1e-3)


# ---- model wiring -------------------------------------------------------------------------------------

def test_constructor_accepts_wct_and_rejects_unknown_names():
    assert models.AdaINStyleTransfer.TRANSFORMS == ("adain", "efdm", "wct")
    net = models.AdaINStyleTransfer(transform="wct")
    assert isinstance(net.adain, models.WCT) and net.transform == "wct"
    assert not list(net.adain.parameters()) and not list(net.adain.buffers())
    assert list(net.state_dict()) == list(models.AdaINStyleTransfer().state_dict())
    with pytest.raises(ValueError):
        models.AdaINStyleTransfer(transform="zca")
    assert "wct" in library.OPS


def test_statistics_methods_raise_under_wct():
    net = models.AdaINStyleTransfer(transform="wct")
    img = torch.zeros(1, 3, 32, 32)
    with torch.no_grad():
        for call in (lambda: net.style_statistics(img), lambda: net.stylize_with_stats(img, torch.zeros(512), torch.ones(512)),
                     lambda: net.stylize_regions(img, img)):
            with pytest.raises(NotImplementedError):
                call()


def test_cpu_tensors_and_gradients_are_rejected():
    x = torch.rand(1, 4, 3, 3)
    with pytest.raises(_lib.HipOpError):
        ops.wct(x, x)
    with pytest.raises(_lib.HipOpError):
        ops.wct_cov(x)
    with pytest.raises(_lib.HipOpError):
        ops.wct_sqrt(torch.eye(4)[None])
    with pytest.raises(NotImplementedError):
        models.WCT()(x.requires_grad_(), x)


# ---- C ABI ----------------------------------------------------------------------------------------------

P = 256   # a non-null "pointer": every call below must return before anything is launched or read
BIG = 1 << 40


@pytest.mark.parametrize("want,call", [
    # ast_wct_f32(content, style, out, n, ns, c, hc, wc, hs, ws, alpha, eps_rel, iters, ws, bytes, stream)
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 0, 1, 8, 4, 4, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 0, 4, 4, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 0, 4, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 1, 1, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),   # Mc = 1
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 1, 1, 1.0, 1e-3, 0, P, BIG, None)),   # Ms = 1
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 3, 2, 8, 4, 4, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),   # ns not in {1, n}
    (E_SHAPE, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, 1e-3, 0, P, 1024, None)),  # short workspace
    (E_UNSUPPORTED, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, 5e-5, 0, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, 1.5, 0, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, float("nan"), 0, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 1025, 4, 4, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, 1e-3, -1, P, BIG, None)),
    (-1, lambda L: L.ast_wct_f32(P, None, P, 2, 2, 8, 4, 4, 4, 4, 1.0, 1e-3, 0, P, BIG, None)),
    (-1, lambda L: L.ast_wct_f32(P, P, P, 2, 2, 8, 4, 4, 4, 4, 1.0, 1e-3, 0, None, BIG, None)),
    # ast_wct_cov_f32(x, mean, cov, n, c, m, eps_rel, ws, bytes, stream)
    (E_SHAPE, lambda L: L.ast_wct_cov_f32(P, P, P, 0, 8, 16, 1e-3, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_cov_f32(P, P, P, 1, 8, 1, 1e-3, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_cov_f32(P, P, P, 1, 8, 16, 1e-3, P, 16, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_cov_f32(P, P, P, 1, 8, 16, 2.0, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_cov_f32(P, P, P, 1, 1025, 16, 1e-3, P, BIG, None)),
    # ast_wct_sqrt_f32(cov, sqrt, isqrt, b, c, iters, ws, bytes, stream)
    (E_SHAPE, lambda L: L.ast_wct_sqrt_f32(P, P, P, 0, 8, 0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_sqrt_f32(P, P, P, 1, 8, 0, P, 16, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_sqrt_f32(P, P, P, 1, 8, -3, P, BIG, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_sqrt_f32(P, P, P, 1, 1025, 0, P, BIG, None)),
    (-1, lambda L: L.ast_wct_sqrt_f32(P, None, None, 1, 8, 0, P, BIG, None)),
    # ast_wct_apply_f32(content, mean_c, mean_s, sqrt_s, isqrt_c, out, n, ns, c, mc, alpha, ws, bytes, stream)
    (E_SHAPE, lambda L: L.ast_wct_apply_f32(P, P, P, P, P, P, 2, 3, 8, 16, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_apply_f32(P, P, P, P, P, P, 2, 2, 8, 1, 1.0, P, BIG, None)),
    (E_SHAPE, lambda L: L.ast_wct_apply_f32(P, P, P, P, P, P, 2, 2, 8, 16, 1.0, P, 16, None)),
    (E_UNSUPPORTED, lambda L: L.ast_wct_apply_f32(P, P, P, P, P, P, 2, 2, 1025, 16, 1.0, P, BIG, None)),
])
def test_bad_arguments_are_rejected_before_launch(want, call):
    assert call(_lib.lib()) == want


def test_workspace_queries():
    L = _lib.lib()
    assert L.ast_wct_workspace_bytes(2, 2, 8, 16, 16) > 0 and L.ast_wct_workspace_bytes(8, 1, 512, 4096, 4096) > 0
    assert L.ast_wct_workspace_bytes(2, 3, 8, 16, 16) == E_SHAPE and L.ast_wct_workspace_bytes(2, 2, 8, 1, 16) == E_SHAPE
    assert L.ast_wct_workspace_bytes(2, 2, 1025, 16, 16) == E_UNSUPPORTED
    assert L.ast_wct_cov_workspace_bytes(1, 8, 1) == E_SHAPE and L.ast_wct_cov_workspace_bytes(1, 8, 99) > 0
    assert L.ast_wct_sqrt_workspace_bytes(0, 8) == E_SHAPE and L.ast_wct_sqrt_workspace_bytes(2, 1025) == E_UNSUPPORTED
    assert L.ast_wct_apply_workspace_bytes(2, 8) >= 4 * 2 * 8 * 8
    # the whole op's workspace covers each stage's
    whole = L.ast_wct_workspace_bytes(2, 1, 48, 99, 91)
    assert whole >= max(L.ast_wct_cov_workspace_bytes(2, 48, 99), L.ast_wct_sqrt_workspace_bytes(3, 48))


# ---- registered op ------------------------------------------------------------------------------------------

def test_meta_kernel_returns_the_content_shape():
    m = torch.device("meta")
    c, s = torch.empty(2, 16, 8, 12, device=m), torch.empty(1, 16, 5, 7, device=m)
    out = torch.ops.ast_hip.wct(c, s, 0.6, 1e-3, 0)
    assert out.shape == c.shape and out.dtype == c.dtype and out.device.type == "meta"
