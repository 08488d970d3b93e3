"""CPU: the surface of exact feature distribution matching (ops, library, models, losses, header
constant), the C-ABI argument checks of the three entry points and their workspace queries, the
host-side checks of the wrappers, the fake kernels, and the restatement tests/efdm_ref.py pinned to
a brute-force rank count and to the paper's formulation. Nothing is launched."""
import inspect
import os
import re

import pytest
import torch

import efdm_ref as ER
from arbitrarystyletransfer_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")
ENTRY_POINTS = ("ast_efdm_f32", "ast_efdm_ex_f32", "ast_plane_sort_f32")
QUERIES = ("ast_efdm_workspace_bytes", "ast_efdm_ex_workspace_bytes", "ast_plane_sort_workspace_bytes")


def test_surface():
    from arbitrarystyletransfer_amd import functional, library, losses, models, ops
    for name in ("efdm", "plane_sort"):
        assert callable(getattr(ops, name)), name
        assert name in library.OPS
        assert hasattr(torch.ops.ast_hip, name), name
        assert re.search(rf"^{name}\s", library.__doc__, flags=re.M), name   # the table of the docstring
    for name in ENTRY_POINTS + QUERIES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert issubclass(functional.EFDMFn, torch.autograd.Function)
    assert issubclass(models.EFDM, torch.nn.Module) and not list(models.EFDM().parameters())
    assert callable(losses.compute_efdm_loss) and "compute_efdm_loss" in losses.__all__
    sig = inspect.signature(models.AdaINStyleTransfer.__init__)
    assert sig.parameters["transform"].default == "adain"
    assert "_chunk" in inspect.signature(ops.efdm).parameters
    with pytest.raises(ValueError):
        models.AdaINStyleTransfer(transform="histogram")


def test_header_constant_matches_python_limit():
    from arbitrarystyletransfer_amd import ops
    src = open(HEADER).read()
    (value,) = re.findall(r"#define\s+AST_EFDM_FUSED_MAX\s+(\d+)", src)
    assert int(value) == ops.EFDM_FUSED_MAX == ER.FUSED_MAX
    assert ops.EFDM_FUSED_MAX >= 4096   # the relu4_1 map of a 512^2 image takes the fused path


# ast_efdm_f32(content, style, out, n, ns, c, hc, wc, hs, ws, alpha, workspace, workspace_bytes, stream)
# ast_efdm_ex_f32(..., alpha, chunk, workspace, workspace_bytes, stream)
# ast_plane_sort_f32(x, sorted, index_or_null, planes, m, chunk, workspace, workspace_bytes, stream)
BIG = ER.FUSED_MAX + 1   # a plane of the general path: the workspace arguments are looked at
BIG_WS = 10 ** 9


@pytest.mark.parametrize("call", [
    # efdm: each pointer
    lambda L: L.ast_efdm_f32(None, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, None, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, None, 2, 2, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    # each zero size
    lambda L: L.ast_efdm_f32(1, 1, 1, 0, 1, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 0, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 2, 0, 4, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 2, 3, 0, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 2, 3, 4, 0, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 2, 3, 4, 4, 0, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 0, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 2, 3, -4, 4, 4, 4, 1.0, None, 0, None),
    # ns not in {1, n}
    lambda L: L.ast_efdm_f32(1, 1, 1, 4, 2, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 2, 3, 3, 4, 4, 4, 4, 1.0, None, 0, None),
    # the general path (a content or a style plane past the fused limit): no workspace, too small a one, a misaligned one
    lambda L: L.ast_efdm_f32(1, 1, 1, 1, 1, 1, 1, BIG, 4, 4, 1.0, None, BIG_WS, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 1, 1, 1, 4, 4, BIG, 1, 1.0, None, BIG_WS, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 1, 1, 1, 1, BIG, 4, 4, 1.0, 256, 0, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 1, 1, 1, 1, BIG, 4, 4, 1.0, 256,
                             L.ast_efdm_workspace_bytes(1, 1, 1, BIG, 16) - 1, None),
    lambda L: L.ast_efdm_f32(1, 1, 1, 1, 1, 1, 1, BIG, 4, 4, 1.0, 258, BIG_WS, None),
    # efdm_ex: the same checks ...
    lambda L: L.ast_efdm_ex_f32(None, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, None, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, None, 2, 2, 3, 4, 4, 4, 4, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 0, 1, 3, 4, 4, 4, 4, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 0, 4, 4, 4, 4, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 0, 4, 4, 4, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 0, 1.0, 0, None, 0, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 4, 3, 3, 4, 4, 4, 4, 1.0, 0, None, 0, None),
    # ... a forced chunk makes a small shape need its workspace ...
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 256, None, BIG_WS, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 256, 256,
                                L.ast_efdm_ex_workspace_bytes(2, 2, 3, 16, 16, 256) - 1, None),
    # ... and a bad chunk: not a power of two, under 64, over the fused limit, negative
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 100, 256, BIG_WS, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 32, 256, BIG_WS, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 2 * ER.FUSED_MAX, 256, BIG_WS, None),
    lambda L: L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, -64, 256, BIG_WS, None),
    # plane_sort: each required pointer, zero sizes, a bad chunk, the workspace of the general path
    lambda L: L.ast_plane_sort_f32(None, 1, None, 3, 16, 0, None, 0, None),
    lambda L: L.ast_plane_sort_f32(1, None, None, 3, 16, 0, None, 0, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 0, 16, 0, None, 0, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 3, 0, 0, None, 0, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 3, 2 ** 31, 0, 256, 2 ** 40, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 3, 16, 96, 256, BIG_WS, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 3, 16, 32, 256, BIG_WS, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 3, 16, 64, None, BIG_WS, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 1, BIG, 0, None, BIG_WS, None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 1, BIG, 0, 256,
                                   L.ast_plane_sort_workspace_bytes(1, BIG, 0, 0) - 1, None),
    # with indices the same workspace is too small
    lambda L: L.ast_plane_sort_f32(1, 1, 1, 1, BIG, 0, 256, L.ast_plane_sort_workspace_bytes(1, BIG, 0, 0), None),
    lambda L: L.ast_plane_sort_f32(1, 1, None, 1, BIG, 0, 257, BIG_WS, None),
])
def test_argument_errors_rejected_before_launch(call):
    assert call(_lib.lib()) < 0


def test_error_codes_are_the_documented_ones():
    L = _lib.lib()
    assert L.ast_efdm_f32(None, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, None, 0, None) == -1          # AST_E_NULLPTR
    assert L.ast_efdm_f32(1, 1, 1, 4, 2, 3, 4, 4, 4, 4, 1.0, None, 0, None) == -2             # AST_E_SHAPE
    assert L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 100, 256, BIG_WS, None) == -3  # AST_E_UNSUPPORTED
    assert L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 256, None, BIG_WS, None) == -1
    assert L.ast_efdm_ex_f32(1, 1, 1, 2, 2, 3, 4, 4, 4, 4, 1.0, 256, 256, 8, None) == -2
    assert L.ast_plane_sort_f32(1, 1, None, 3, 16, 96, 256, BIG_WS, None) == -3


def test_workspace_queries():
    L = _lib.lib()
    m = ER.FUSED_MAX
    # 0 wherever the fused path serves the shape; the plain query is the _ex one with chunk 0
    assert L.ast_efdm_workspace_bytes(8, 8, 512, 4096, 4096) == 0
    assert L.ast_efdm_workspace_bytes(8, 1, 512, m, m) == 0
    assert L.ast_plane_sort_workspace_bytes(4096, m, 1, 0) == 0
    for args in ((2, 2, 3, m + 1, 16), (2, 1, 3, 16, m + 1), (1, 1, 64, 262144, 262144)):
        assert L.ast_efdm_workspace_bytes(*args) == L.ast_efdm_ex_workspace_bytes(*args, 0) > 0
    # two buffers of content keys and indices and of style keys, each a multiple of 256 bytes
    assert L.ast_efdm_workspace_bytes(1, 1, 64, 262144, 262144) == (4 + 2) * 4 * 64 * 262144
    assert L.ast_efdm_ex_workspace_bytes(2, 2, 3, 16, 16, 256) == 6 * 512
    assert L.ast_efdm_ex_workspace_bytes(2, 1, 3, 16, 16, 256) == 4 * 512 + 2 * 256
    assert L.ast_plane_sort_workspace_bytes(512, 262144, 0, 0) == 2 * 4 * 512 * 262144
    assert L.ast_plane_sort_workspace_bytes(512, 262144, 1, 0) == 4 * 4 * 512 * 262144
    assert L.ast_plane_sort_workspace_bytes(3, 16, 1, 64) == 4 * 256
    # bad arguments come back as the negative codes
    assert L.ast_efdm_workspace_bytes(2, 3, 3, 16, 16) == -2
    assert L.ast_efdm_workspace_bytes(2, 2, 0, 16, 16) == -2
    assert L.ast_efdm_workspace_bytes(2, 2, 3, 2 ** 31, 16) == -2
    assert L.ast_efdm_workspace_bytes(2 ** 15, 1, 2 ** 15, 2 ** 20, 16) == -2      # a map over 2^40 elements
    assert L.ast_efdm_workspace_bytes(2 ** 15, 1, 2 ** 15, 2 ** 10, 16) == 0      # 2^40: allowed, and fused
    assert L.ast_plane_sort_workspace_bytes(2 ** 30, 2 ** 20, 0, 0) == -2
    assert L.ast_efdm_ex_workspace_bytes(2, 2, 3, 16, 16, 48) == -3
    assert L.ast_plane_sort_workspace_bytes(0, 16, 0, 0) == -2
    assert L.ast_plane_sort_workspace_bytes(3, 16, 0, 3) == -3


def test_wrappers_reject_cpu_tensors_mismatches_and_dtypes():
    from arbitrarystyletransfer_amd import losses, models, ops
    c, s = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4)
    with pytest.raises(_lib.HipOpError, match="cpu"):
        ops.efdm(c, s)
    with pytest.raises(_lib.HipOpError, match="cpu"):
        ops.plane_sort(c)
    with pytest.raises(_lib.HipOpError, match="cpu"):
        models.EFDM()(c, s)
    with pytest.raises(_lib.HipOpError, match="cpu"):
        losses.compute_efdm_loss(c, s)
    # other dtypes are turned away by the same gate (on a device: test_gpu_efdm.py)
    for bad in (c.double(), c.half(), c.to(torch.bfloat16), c.int()):
        with pytest.raises(_lib.HipOpError):
            ops.efdm(bad, s)
        with pytest.raises(_lib.HipOpError):
            ops.plane_sort(bad)


def test_wrapper_shape_checks(monkeypatch):
    """The channel / batch / rank checks of ops.efdm and ops.plane_sort, with the device gate opened
    (it is the first check, and no GPU is here): they raise before the library is asked anything."""
    from arbitrarystyletransfer_amd import ops
    monkeypatch.setattr(ops, "_dev", lambda t, name: t.contiguous())
    monkeypatch.setattr(ops, "lib", lambda: pytest.fail("the library was reached"))
    c = torch.rand(2, 3, 4, 4)
    for s in (torch.rand(2, 4, 4, 4), torch.rand(3, 3, 4, 4), torch.rand(2, 3, 16), torch.rand(2, 3, 0, 4)):
        with pytest.raises(_lib.HipOpError, match="EFDM needs"):
            ops.efdm(c, s)
    with pytest.raises(_lib.HipOpError, match="EFDM needs"):
        ops.efdm(torch.rand(3, 4, 4), torch.rand(3, 4, 4))
    for x in (torch.rand(7), torch.rand(2, 0)):
        with pytest.raises(_lib.HipOpError, match="plane_sort needs"):
            ops.plane_sort(x)


def test_fake_kernels_give_shapes_and_dtypes():
    from arbitrarystyletransfer_amd import library  # noqa: F401
    o = torch.ops.ast_hip
    m = torch.device("meta")
    c = torch.empty(2, 16, 8, 12, device=m)
    for s in (torch.empty(2, 16, 5, 7, device=m), torch.empty(1, 16, 5, 7, device=m)):
        out = o.efdm(c, s, 0.5)
        assert out.shape == c.shape and out.dtype == torch.float32 and out.device.type == "meta"
    vals, idx = o.plane_sort(c)
    assert vals.shape == idx.shape == c.shape and vals.dtype == torch.float32 and idx.dtype == torch.int32
    vals, idx = o.plane_sort(torch.empty(5, 100, device=m))
    assert vals.shape == idx.shape == (5, 100)


def test_state_dict_keys_do_not_depend_on_the_transform():
    from arbitrarystyletransfer_amd import models
    a = models.AdaINStyleTransfer()
    e = models.AdaINStyleTransfer(transform="efdm")
    assert isinstance(a.adain, models.AdaIN) and isinstance(e.adain, models.EFDM)
    assert list(a.state_dict()) == list(e.state_dict()) and len(a.state_dict()) > 0
    for k, v in a.state_dict().items():
        assert torch.equal(v, e.state_dict()[k]), k
    e.load_state_dict(a.state_dict())


def test_statistics_methods_raise_under_efdm():
    from arbitrarystyletransfer_amd import models
    net = models.AdaINStyleTransfer(transform="efdm")
    img = torch.zeros(1, 3, 64, 64)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="efdm"):
            net.style_statistics(img)
        with pytest.raises(NotImplementedError, match="efdm"):
            net.stylize_with_stats(img, torch.zeros(512), torch.ones(512))
        with pytest.raises(NotImplementedError, match="efdm"):
            net.stylize_regions(img, img)


# ---- the restatement ---------------------------------------------------------------------------

def test_keys_follow_total_order():
    nan_neg = torch.tensor([-1], dtype=torch.int32).view(torch.float32)            # 0xffffffff
    nan_pos = torch.tensor([0x7FFFFFFF], dtype=torch.int32).view(torch.float32)
    seq = torch.cat([nan_neg, torch.tensor([float("-inf"), -2.0, -1e-40, -0.0, 0.0, 1e-40, 2.0, float("inf")]),
                     nan_pos])
    k = ER.keys(seq)
    assert bool((k[1:] > k[:-1]).all()), k.tolist()
    # the unsigned form of the kernel (flip all bits of a negative, else the sign bit) orders alike
    b = seq.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(b >= 2 ** 31, b ^ 0xFFFFFFFF, b ^ 0x80000000)
    assert bool((u[1:] > u[:-1]).all())
    assert torch.equal(u - 2 ** 31, k.to(torch.int64))


@pytest.mark.parametrize("cs,ss", [
    ((2, 2, 3, 5), (2, 2, 3, 5)),      # equal sizes
    ((1, 2, 4, 6), (1, 2, 3, 3)),      # Ms < Mc
    ((3, 1, 2, 5), (1, 1, 4, 7)),      # Ms > Mc, one style shared by the batch
])
def test_restatement_equals_brute_force_rank_count(cs, ss):
    c, s = ER.features(11, cs, specials=True), ER.features(12, ss, specials=True)
    assert (c == 0).sum() >= 4 and torch.isnan(c).any() and torch.isinf(s).any()
    assert bool((c.view(torch.int32) == -2 ** 31).any())   # a -0.0 among the +0.0 ties
    got, ref = ER.efdm_target(c, s), ER.brute_force_target(c, s)
    assert ER.bits_equal(got, ref)
    assert ER.bits_equal(ER.efdm(c, s, 1.0), ref)


def test_restatement_equals_the_papers_formulation():
    c, s = ER.features(21, (2, 3, 16, 16)), ER.features(22, (2, 3, 16, 16))
    assert 0.3 < float((c == 0).float().mean()) < 0.7
    assert ER.bits_equal(ER.efdm_target(c, s), ER.paper_efdm(c, s))


def test_restatement_plane_sort():
    x = ER.features(31, (3, 50), specials=True)
    vals, idx = ER.plane_sort(x)
    assert idx.dtype == torch.int32 and ER.bits_equal(vals, torch.gather(x, 1, idx.long()))
    k = torch.gather(ER.keys(x), 1, idx.long())
    assert bool((k[:, 1:] >= k[:, :-1]).all())
    tie = k[:, 1:] == k[:, :-1]
    assert bool(tie.any()) and bool((idx[:, 1:] > idx[:, :-1])[tie].all())      # ties in index order
    assert torch.isnan(vals[:, -1]).all() and bool((vals[:, 0] == float("-inf")).all())
    z = (vals == 0).nonzero()
    first_zero = vals[0, int(z[z[:, 0] == 0][0, 1])]
    assert first_zero.view(torch.int32).item() == -2 ** 31                       # -0.0 before every +0.0


def test_rank_mapping():
    for m in (1, 2, 7, 64, 1000):
        assert torch.equal(ER.rank_map(m, m), torch.arange(m))
    for mc, ms in ((1, 9), (9, 1), (960, 256), (256, 960), (4097, 4096), (5, 2 ** 31 - 1), (2 ** 20, 3)):
        j = ER.rank_map(mc, ms)
        assert int(j.min()) >= 0 and int(j.max()) <= ms - 1 and bool((j[1:] >= j[:-1]).all()), (mc, ms)
    # the largest product of the definition still fits a signed 64-bit integer
    assert (2 * (2 ** 31 - 2) + 1) * (2 ** 31 - 1) < 2 ** 63


def test_blend_in_fp32_is_far_below_the_op_tolerance():
    """The GPU tests hold the alpha = 0.3 blend to 2e-5 against the float64 blend of the bit-exact
    target; the same blend in float32 on the CPU sits four orders of magnitude under that."""
    worst = 0.0
    for name in ("64x64", "bigger_content", "chunked_sizes_differ"):
        c, s, _ = ER.case_inputs(name)
        worst = max(worst, ER.rel_inf(ER.efdm(c, s, 0.3, torch.float32), ER.efdm(c, s, 0.3, torch.float64)))
    print(f"fp32 blend vs float64: {worst:.2e}")
    assert worst <= 2e-7


@pytest.mark.parametrize("name", list(ER.CASES))
def test_case_inputs_are_what_the_gpu_tests_expect(name):
    c, s, chunk = ER.case_inputs(name)
    cs, ss, specials, _ = ER.CASES[name]
    assert tuple(c.shape) == cs and tuple(s.shape) == ss and c.dtype == s.dtype == torch.float32
    assert bool(torch.isnan(c).any()) == specials
    assert float((c == 0).float().mean()) > 0.3
    assert chunk == 0 or (chunk >= 64 and chunk & (chunk - 1) == 0)
