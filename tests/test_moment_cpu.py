"""CPU: the float64 statement of the moment-matching loss (tests/moment_ref.py), the condition on the
test inputs that its sign bar needs, and the host side of csrc/moment.hip through the C ABI (argument
checks and workspace queries; nothing is launched: no GPU needed)."""
import os
import re

import pytest
import torch

import moment_ref as R
from arbitrarystyletransfer_amd import _lib, library, losses, ops, train  # noqa: F401  (library registers the ops)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ast_hip.h")
NAMES = {"ast_moment_stats_workspace_bytes": 4, "ast_moment_stats_f32": 10, "ast_moment_loss_workspace_bytes": 4,
         "ast_moment_loss_f32": 17, "ast_moment_loss_backward_f32": 12}


@pytest.mark.parametrize("name", list(R.CASES))
def test_analytic_gradient_equals_autograd(name):
    x, y = R.case_inputs(name)
    leaf = x.double().requires_grad_(True)
    R.loss(leaf, y, weight=0.7).backward(torch.tensor(1.3, dtype=torch.float64))
    y_mean, y_cov = R.stats(y)
    want = R.gradient(x, y_mean, y_cov, weight=0.7, g=1.3)
    assert want.shape == x.shape
    assert R.rel_inf(want, leaf.grad) <= 1e-12
    assert y.grad is None


@pytest.mark.parametrize("name", list(R.CASES))
def test_inputs_leave_few_signs_unresolved(name):
    """The condition of the sign bar: at most UNRESOLVED_MAX of the C^2 entries lie inside the margin in
    float64, and fp32 CPU arithmetic flips none of the resolved ones."""
    x, y = R.case_inputs(name)
    n, c = x.shape[:2]
    y_mean, y_cov = R.stats(y)
    mu, cov = R.stats(x)
    ok = R.resolved(cov, y_cov)
    share = [1.0 - float(ok[b].double().mean()) for b in range(n)]
    print(f"{name}: unresolved share per sample {['%.4f' % s for s in share]}")
    assert max(share) <= R.UNRESOLVED_MAX
    ok_mu = R.resolved_mu(mu, y_mean)
    assert 1.0 - float(ok_mu.double().mean(dim=1).min()) <= R.UNRESOLVED_MAX
    s_mu64, s_cov64 = R.signs(x, y_mean, y_cov)
    y_mean32, y_cov32 = R.stats(y, torch.float32)
    s_mu32, s_cov32 = R.signs(x, y_mean32, y_cov32, torch.float32)
    assert torch.equal(s_cov32[ok], s_cov64[ok]) and torch.equal(s_mu32[ok_mu], s_mu64[ok_mu])
    assert torch.equal(s_cov64, s_cov64.transpose(1, 2))


def test_definition_on_a_hand_case():
    x = torch.tensor([[[[0.0, 2.0]], [[1.0, 1.0]]]])            # C = 2, M = 2: mu = (1, 1), Cov = [[2, 0], [0, 0]]
    y = torch.tensor([[[[1.0, 3.0, 5.0]], [[0.0, 0.0, 3.0]]]])  # mu = (3, 1), Cov = [[4, 3], [3, 3]]
    mean, cov = R.stats(x)
    assert mean.tolist() == [[1.0, 1.0]] and cov.tolist() == [[[2.0, 0.0], [0.0, 0.0]]]
    y_mean, y_cov = R.stats(y)
    assert y_mean.tolist() == [[3.0, 1.0]] and y_cov.tolist() == [[[4.0, 3.0], [3.0, 3.0]]]
    assert float(R.loss(x, y)) == (2.0 + 0.0) / 2 + (2.0 + 3.0 + 3.0 + 3.0) / 4
    s_mu, s_cov = R.signs(x, y_mean, y_cov)
    assert s_mu.tolist() == [[-1, 0]] and s_cov.tolist() == [[[-1, -1], [-1, -1]]]


def test_header_binding_and_surface():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name)
    assert "#define AST_MOMENT_MAX_C 1024" in open(HEADER).read() and ops.MOMENT_MAX_C == 1024
    assert library.OPS[library.OPS.index("cx_loss") + 1] == "moment_loss"
    assert hasattr(torch.ops.ast_hip, "moment_loss")
    assert "compute_moment_loss" in losses.__all__
    a = train.default_args()
    assert a.moment_lam == 0.0 and tuple(a.moment_taps) == ("relu_9", "relu_15")
    with pytest.raises(ValueError):
        train._tap_index("relu_99", "moment_taps")


def _al256(b):
    return (b + 255) & ~255


def test_workspace_queries():
    L = _lib.lib()
    tile = 4 * 64 * 64
    # (n, c, m, splits) -> splits used, tile pairs
    for (n, c, m, forced), (splits, pairs) in {
        (1, 64, 4096, 0): (8, 1), (2, 160, 143, 0): (3, 6), (2, 512, 64, 0): (1, 36), (3, 96, 2, 0): (1, 3),
        (1, 64, 4096, 1): (1, 1), (1, 64, 4096, 4): (4, 1), (1, 1, 2, 4): (1, 1), (1, 1024, 70, 3): (3, 136),
        (2, 160, 143, 4): (3, 6),   # 4 splits of 36 pixels round up to 64 each: three have pixels
    }.items():
        part = _al256(n * splits * pairs * tile)
        assert L.ast_moment_stats_workspace_bytes(n, c, m, forced) == part, (n, c, m, forced)
        assert L.ast_moment_loss_workspace_bytes(n, c, m, forced) == part + _al256(4 * n * pairs), (n, c, m, forced)
    for q in (L.ast_moment_stats_workspace_bytes, L.ast_moment_loss_workspace_bytes):
        assert q(0, 64, 16, 0) == -2 and q(1, 0, 16, 0) == -2 and q(1, 64, 1, 0) == -2 and q(32768, 64, 16, 0) == -2
        assert q(1, 64, 1 << 31, 0) == -2
        assert q(1, 1025, 16, 0) == -3 and q(1, 64, 16, -1) == -3


@pytest.mark.parametrize("call", [
    lambda L: L.ast_moment_stats_f32(None, 1, 1, 1, 8, 16, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, None, 1, 1, 8, 16, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, None, 1, 8, 16, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, 1, 1, 8, 16, 0, None, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, 1, 0, 8, 16, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, 1, 1, 8, 1, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, 1, 1, 1025, 16, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, 1, 1, 8, 16, -1, 1, 1 << 30, None),
    lambda L: L.ast_moment_stats_f32(1, 1, 1, 1, 8, 16, 0, 1, 16383, None),          # a short workspace
    lambda L: L.ast_moment_loss_f32(None, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, None, 1, 1, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, None, 1, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, None, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, None, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, None, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, None, 1, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, None, 1, 1, 8, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, None, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, 1, 3, 2, 8, 16, 1.0, 0, 1, 1 << 30, None),   # ns not in {1, n}
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 1, 1.0, 0, 1, 1 << 30, None),    # one pixel
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1025, 16, 1.0, 0, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, -2, 1, 1 << 30, None),
    lambda L: L.ast_moment_loss_f32(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 16, 1.0, 0, 1, 16384, None),     # a short workspace
    lambda L: L.ast_moment_loss_backward_f32(None, 1, 1, 1, None, 1, 1, 8, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, None, 1, 1, None, 1, 1, 8, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, None, 1, None, 1, 1, 8, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, 1, None, None, 1, 1, 8, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, 1, 1, None, None, 1, 8, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, 1, 1, None, 1, 0, 8, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, 1, 1, None, 1, 1, 0, 16, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, 1, 1, None, 1, 1, 8, 1, 1.0, 0, None),
    lambda L: L.ast_moment_loss_backward_f32(1, 1, 1, 1, None, 1, 1, 1025, 16, 1.0, 0, None),
])
def test_argument_errors_rejected_before_launch(call):
    assert call(_lib.lib()) < 0


def test_python_surface_rejects_bad_calls():
    x = torch.zeros(1, 8, 4, 4)
    for call in (lambda: ops.moment_stats(x), lambda: ops.moment_loss(x, torch.zeros(1, 8), torch.zeros(1, 8, 8)),
                 lambda: ops.moment_loss_backward(x, (x, x, x)),
                 lambda: losses.compute_moment_loss(x, x)):
        with pytest.raises(_lib.HipOpError):   # CPU tensors: there is no CPU path
            call()


def test_fake_kernel_gives_the_output_shapes():
    m = torch.device("meta")
    x = torch.empty(2, 16, 5, 7, device=m)
    out = torch.ops.ast_hip.moment_loss(x, torch.empty(1, 16, device=m), torch.empty(1, 16, 16, device=m), 1.0)
    assert [tuple(t.shape) for t in out] == [(), (2,), (2, 16), (2, 16), (2, 16, 16)]
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.float32, torch.int8, torch.int8]
