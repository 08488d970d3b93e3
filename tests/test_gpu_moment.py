"""GPU: the moment-matching style loss of csrc/moment.hip against its float64 statement
(tests/moment_ref.py, where the bars are stated)."""
import argparse
import gc

import pytest
import torch

import moment_ref as R
from arbitrarystyletransfer_amd import _lib, losses, ops, synth
from arbitrarystyletransfer_amd import library  # noqa: F401  (registers the ops)

pytestmark = pytest.mark.gpu

NAMES = list(R.CASES)
_CACHE = {}


def _case(name):
    """Inputs and float64 references of a case, computed once and left unchanged."""
    if name not in _CACHE:
        x, y = R.case_inputs(name)
        y_mean, y_cov = R.stats(y)
        mu, cov = R.stats(x)
        _CACHE[name] = dict(x=x, y=y, y_mean=y_mean, y_cov=y_cov, mu=mu, cov=cov,
                            terms=R.sample_terms(x, y_mean, y_cov), signs=R.signs(x, y_mean, y_cov),
                            ok=R.resolved(cov, y_cov), ok_mu=R.resolved_mu(mu, y_mean))
    return _CACHE[name]


def _same(a, b):
    """Bitwise equality (NaNs with equal bits are equal)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def _one(dev, v=1.0):
    return torch.tensor(v, device=dev, dtype=torch.float32)


def _forward(name, dev, weight=1.0, splits=0):
    c = _case(name)
    x, y = c["x"].to(dev), c["y"].to(dev)
    y_mean, y_cov = ops.moment_stats(y, _splits=splits)
    loss, state = ops.moment_loss(x, y_mean, y_cov, weight, _splits=splits)
    return x, y_mean, y_cov, loss, state


@pytest.mark.parametrize("name", NAMES)
def test_stats_against_float64(name, hip_device):
    c = _case(name)
    mean, cov = ops.moment_stats(c["y"].to(hip_device))
    e_mu = float((mean.double().cpu() - c["y_mean"]).abs().max()) / float(c["y_mean"].abs().max())
    e_cov = float((cov.double().cpu() - c["y_cov"]).abs().max()) / float(c["y_cov"].abs().max())
    print(f"{name}: mean {e_mu:.2e}, cov {e_cov:.2e} of the largest entry")
    assert e_mu <= R.OP_TOL and e_cov <= R.OP_TOL
    assert _same(cov, cov.transpose(1, 2).contiguous())


@pytest.mark.parametrize("name", NAMES)
def test_loss_and_signs_against_float64(name, hip_device):
    c = _case(name)
    weight = 0.7
    x, y_mean, y_cov, loss, (mean_x, sign_mu, sign_cov, sums) = _forward(name, hip_device, weight)
    want = weight * float(c["terms"].mean())
    err = abs(float(loss) - want) / want
    e_terms = float(((sums.double().cpu() - c["terms"]).abs() / c["terms"]).max())
    print(f"{name}: loss {float(loss):.7f} vs {want:.7f} ({err:.2e}); per-sample terms {e_terms:.2e}")
    assert err <= R.OP_TOL and e_terms <= R.OP_TOL
    assert float((mean_x.double().cpu() - c["mu"]).abs().max()) <= R.OP_TOL * float(c["mu"].abs().max())
    s_mu, s_cov = sign_mu.cpu(), sign_cov.cpu()
    assert s_cov.dtype == torch.int8 and s_mu.dtype == torch.int8
    assert bool(((s_cov >= -1) & (s_cov <= 1)).all()) and bool(((s_mu >= -1) & (s_mu <= 1)).all())
    assert torch.equal(s_cov, s_cov.transpose(1, 2))
    ok, ok_mu = c["ok"], c["ok_mu"]
    share = 1.0 - float(ok.double().mean(dim=(1, 2)).min())
    flips = int((s_cov[ok] != c["signs"][1][ok]).sum())
    print(f"{name}: {share:.4%} of C^2 inside the margin, {flips} resolved signs differ")
    assert share <= R.UNRESOLVED_MAX
    assert flips == 0 and torch.equal(s_mu[ok_mu], c["signs"][0][ok_mu])


@pytest.mark.parametrize("name", NAMES)
def test_backward_against_float64_at_the_kernels_signs(name, hip_device):
    c = _case(name)
    weight, g = 0.7, 1.3
    x, _, _, _, state = _forward(name, hip_device, weight)
    dx = ops.moment_loss_backward(x, state, _one(hip_device, g), weight)
    want = R.gradient(c["x"], c["y_mean"], c["y_cov"], weight, g, state[1].cpu(), state[2].cpu())
    err = R.rel_inf(dx.cpu(), want)
    print(f"{name}: gradient rel_inf {err:.2e}")
    assert dx.shape == x.shape and err <= R.OP_TOL
    # gscale None is 1; accumulate adds into the buffer
    d1 = ops.moment_loss_backward(x, state, None, weight)
    assert _same(d1, ops.moment_loss_backward(x, state, _one(hip_device), weight))
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(hip_device)
    out = base.clone()
    assert ops.moment_loss_backward(x, state, _one(hip_device, g), weight, out=out) is out
    # base + gradient with the gradient's last product possibly fused into the add: two roundings apart at most
    want_acc = base.double() + dx.double()
    assert float((out.double() - want_acc).abs().max()) <= 2 * 2.0 ** -24 * float(want_acc.abs().max() + dx.abs().max())


def test_equal_maps_give_zero(hip_device):
    x = _case("c160_tails")["x"].to(hip_device)
    mean, cov = ops.moment_stats(x)
    loss, (mean_x, sign_mu, sign_cov, sums) = ops.moment_loss(x, mean, cov)
    assert float(loss) == 0.0 and not bool(sign_mu.any()) and not bool(sign_cov.any()) and _same(mean_x, mean)
    assert not bool(ops.moment_loss_backward(x, (mean_x, sign_mu, sign_cov)).any())


def test_constant_channel_has_exact_statistics(hip_device):
    c = _case("c40_constant_channel")
    mean, cov = ops.moment_stats(c["x"].to(hip_device))
    assert bool((mean[:, 3] == 0.75).all()) and not bool(cov[:, 3].any()) and not bool(cov[:, :, 3].any())
    assert float(mean[0, 5]) == 0.0 and not bool(cov[0, 5].any())


def test_split_counts_agree(hip_device):
    name = "c64_pixel_splits"
    c = _case(name)
    runs = [_forward(name, hip_device, 1.0, s) for s in (1, 4, 0)]
    covs = [r[2].double().cpu() for r in runs]
    scale = float(c["y_cov"].abs().max())
    for cov in covs:
        assert float((cov - c["y_cov"]).abs().max()) <= R.OP_TOL * scale
    losses_ = [float(r[3]) for r in runs]
    print(f"splits 1 / 4 / auto: loss {losses_}")
    assert max(losses_) - min(losses_) <= R.OP_TOL * max(losses_)
    grads = [ops.moment_loss_backward(r[0], r[4]).cpu() for r in runs]
    want = [R.gradient(c["x"], c["y_mean"], c["y_cov"], 1.0, 1.0, r[4][1].cpu(), r[4][2].cpu()) for r in runs]
    assert max(R.rel_inf(a, b) for a, b in zip(grads, want)) <= R.OP_TOL


def test_run_twice_bitwise(hip_device):
    for name in ("c160_tails", "c64_pixel_splits", "c96_two_pixels"):
        runs = []
        for _ in range(2):
            x, y_mean, y_cov, loss, state = _forward(name, hip_device, 0.7)
            runs.append((y_mean, y_cov, loss.reshape(1)) + state + (ops.moment_loss_backward(x, state, None, 0.7),))
        assert all(_same(a, b) for a, b in zip(*runs)), name


def test_graph_replay_equals_eager(hip_device):
    c = _case("c160_tails")
    x, y = c["x"].to(hip_device), c["y"].to(hip_device)   # on the device before the capture

    def body():
        y_mean, y_cov = ops.moment_stats(y)
        loss, state = ops.moment_loss(x, y_mean, y_cov, 0.7)
        return (loss.reshape(1),) + state + (ops.moment_loss_backward(x, state, None, 0.7),)
    eager = body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            out = body()
    finally:
        gc.enable()
    for t in out:
        t.fill_(0)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(eager, out))


def test_nan_stays_inside_its_sample(hip_device):
    for name in ("c160_tails", "c512_shared_style"):
        c = _case(name)
        x = c["x"].clone().to(hip_device)
        y_mean, y_cov = ops.moment_stats(c["y"].to(hip_device))
        _, clean = ops.moment_loss(x, y_mean, y_cov)
        d_clean = ops.moment_loss_backward(x, clean)
        x[0, 7, 1, 2] = float("nan")
        loss, state = ops.moment_loss(x, y_mean, y_cov)
        dx = ops.moment_loss_backward(x, state)
        assert not bool(torch.isfinite(loss)) and not bool(torch.isfinite(state[3][0]))
        assert _same(state[3][1:], clean[3][1:])                    # sample 1's loss term, in bits
        assert all(_same(a[1:], b[1:]) for a, b in zip(state[:3], clean[:3]))
        assert _same(dx[1:], d_clean[1:]) and bool(torch.isfinite(dx[1:]).all())
        assert int(state[2][0, 7].abs().sum()) == 0 and int(state[1][0, 7]) == 0   # a NaN difference has sign 0


def test_autograd_paths_equal_the_kernels_bitwise(hip_device):
    name = "c160_tails"
    c = _case(name)
    x, y_mean, y_cov, loss, state = _forward(name, hip_device, 0.6)
    want = ops.moment_loss_backward(x, state, _one(hip_device, 2.0), 0.6)
    # the registered op: the same kernels, and its fake kernel's shapes
    res = torch.ops.ast_hip.moment_loss(x, y_mean, y_cov, 0.6)
    assert all(_same(a, b) for a, b in zip(res, (loss.reshape(()), state[3], state[0], state[1], state[2])))
    m = torch.device("meta")
    fake = torch.ops.ast_hip.moment_loss(x.to(m), y_mean.to(m), y_cov.to(m), 0.6)
    assert [(tuple(t.shape), t.dtype) for t in fake] == [(tuple(t.shape), t.dtype) for t in res]
    leaf2 = x.clone().requires_grad_(True)
    ym, yc = y_mean.clone().requires_grad_(True), y_cov.clone().requires_grad_(True)
    out = torch.ops.ast_hip.moment_loss(leaf2, ym, yc, 0.6)[0]
    (2.0 * out).backward()
    assert _same(out.detach().reshape(1), loss.reshape(1)) and _same(leaf2.grad, want)
    assert ym.grad is None and yc.grad is None                      # the target gets no gradient
    torch.library.opcheck(torch.ops.ast_hip.moment_loss, (x.clone().requires_grad_(True), y_mean, y_cov, 0.6),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    # losses.compute_moment_loss takes the maps; the style map gets no gradient
    y = c["y"].to(hip_device).requires_grad_(True)
    leaf3 = x.clone().requires_grad_(True)
    val = losses.compute_moment_loss(leaf3, y, 0.6)
    (2.0 * val).backward()
    assert _same(val.detach().reshape(1), loss.reshape(1)) and _same(leaf3.grad, want) and y.grad is None


def test_wrappers_reject_bad_inputs(hip_device):
    d = hip_device
    f = lambda *s: torch.zeros(*s, device=d)  # noqa: E731
    bad = [
        lambda: ops.moment_stats(f(1, 8, 1, 1)),                                         # one pixel
        lambda: ops.moment_stats(f(8, 2, 2)),                                            # not 4-D
        lambda: ops.moment_stats(f(1, 8, 2, 2).double()),                                # not float32
        lambda: ops.moment_stats(f(1, ops.MOMENT_MAX_C + 1, 1, 2)),                      # past the limit
        lambda: ops.moment_loss(f(2, 8, 2, 2), f(3, 8), f(3, 8, 8)),                     # a style batch neither N nor 1
        lambda: ops.moment_loss(f(2, 8, 2, 2), f(1, 9), f(1, 9, 9)),                     # C mismatch
        lambda: ops.moment_loss(f(2, 8, 2, 2), f(1, 8), f(1, 8, 8).double()),
        lambda: ops.moment_loss(f(2, 8, 2, 2), torch.zeros(1, 8), f(1, 8, 8)),           # statistics on the CPU
        lambda: ops.moment_loss_backward(f(1, 8, 2, 2), (f(1, 8), f(1, 8), f(1, 8, 8))),  # float signs
        lambda: ops.moment_loss_backward(f(1, 8, 2, 2), (f(1, 8), f(1, 8).to(torch.int8), f(1, 8, 8).to(torch.int8)),
                                         torch.tensor(1.0)),                             # the scalar on the CPU
        lambda: losses.compute_moment_loss(f(1, 8, 2, 2), f(1, 9, 2, 2)),
    ]
    for call in bad:
        with pytest.raises(_lib.HipOpError):
            call()


# ---- trainer ------------------------------------------------------------------------------------------

def _trainer(dev, drop=(), **kw):
    from arbitrarystyletransfer_amd.train import AdaINTrainer, default_args
    torch.manual_seed(1234)
    args = vars(default_args(batch_size=2, image_size=64, **kw))
    for k in drop:
        del args[k]
    return AdaINTrainer(argparse.Namespace(**args), device=dev)


def test_trainer_without_the_term_is_the_parents_step(hip_device):
    """moment_lam = 0 (the default) and arguments that do not know the key at all give the same step in
    bits: nothing of the term is launched."""
    c = torch.from_numpy(synth.image(4321, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(4322, (2, 3, 64, 64))).to(hip_device)
    a, b = _trainer(hip_device), _trainer(hip_device, drop=("moment_lam", "moment_taps"))
    assert not hasattr(b.args, "moment_lam") and a.args.moment_lam == 0.0
    b.net.load_state_dict(a.net.state_dict())
    keys = list(a.train_dict)
    oa, ob = a.train_step(c, s, record=True), b.train_step(c, s, record=True)
    assert set(oa) == set(ob) and "moment_loss" not in oa
    assert list(a.train_dict) == list(b.train_dict) == keys
    assert all(_same(oa[k].detach().reshape(-1), ob[k].detach().reshape(-1)) for k in ("loss", "stylized", "grad_norm"))
    assert all(_same(p.detach(), q.detach()) for p, q in zip(a.params, b.params))


def test_trainer_term(hip_device):
    from arbitrarystyletransfer_amd import train
    c = torch.from_numpy(synth.image(4321, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(4322, (2, 3, 64, 64))).to(hip_device)
    base, tr = _trainer(hip_device), _trainer(hip_device, moment_lam=1.0)
    tr.net.load_state_dict(base.net.state_dict())
    out0 = base.compute_losses(c, s)
    out0["loss"].backward()
    g0 = [p.grad.clone() for p in base.params]
    out1 = tr.compute_losses(c, s)
    with torch.no_grad():
        taps, s_taps = tr.lossnet(c, s), tr.lossnet(out1["stylized"])
        want = sum(losses.compute_moment_loss(s_taps[i], taps[i][2:])
                   for i in (train._tap_index(k) for k in tr.args.moment_taps))
    assert _same(out1["moment_loss"].detach().reshape(1), want.reshape(1)) and float(want) > 0
    total = float(out0["loss"].detach()) + float(out1["moment_loss"].detach())
    assert abs(float(out1["loss"].detach()) - total) <= 1e-6 * abs(total)
    assert set(out1) - set(out0) == {"moment_loss"}
    out1["loss"].backward()
    g1 = [p.grad.clone() for p in tr.params]
    assert all(bool(torch.isfinite(g).all()) for g in g1)
    assert any(not _same(a, b) for a, b in zip(g0, g1))
