"""GPU: the self-similarity content loss (csrc/selfsim.hip: column sums, the pass over the tile pairs,
loss, GEMM backward) and its wrapper / autograd / registered-op / trainer surface, against
tests/selfsim_ref.py.

Bars (selfsim_ref.py derives them; none comes from the code under test): column sums within OP_TOL N of
float64; the loss and every per-sample value within OP_TOL = 2e-5; a sign may differ from the float64
sign only where |e64| <= 2 OP_TOL (q_x + q_c); t within OP_TOL of the float64 t at the GPU's signs; the
gradient within OP_TOL rel_inf of the float64 analytic gradient at the GPU's own sign planes. Everything
else is bit-for-bit.
"""
import functools
import gc

import pytest
import torch

import selfsim_ref as R
from arbitrarystyletransfer_amd import _lib, functional, library, losses, ops, synth  # noqa: F401  (registers the ops)

pytestmark = pytest.mark.gpu

OP_TOL = R.OP_TOL


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.case_inputs(name)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _mismatches(got, ref):
    return int((_bits(got) != _bits(ref)).sum())


def _flat(t):
    return t.cpu().reshape(t.shape[0], -1)


def _one(dev, v=1.0):
    return torch.tensor(v, device=dev)


def _npix(x):
    return x.shape[2] * x.shape[3]


# ---- the bars, per case ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_column_sums_against_float64(name, hip_device):
    x, c = _case(name)
    e = []
    for f in (x, c):
        fd = f.to(hip_device)
        r = ops.selfsim_colsum(fd, ops.cosine_norms(fd))
        assert tuple(r.shape) == (f.shape[0],) + tuple(f.shape[2:])
        e.append(float((_flat(r).double() - R.colsum(f)).abs().max()))
    print(f"selfsim_colsum {name}: |r - r64| x {e[0]:.2e}, c {e[1]:.2e} (bar {OP_TOL * _npix(x):.1e})")
    assert max(e) <= OP_TOL * _npix(x)


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_against_float64(name, hip_device):
    x, c = _case(name)
    n, npix = x.shape[0], _npix(x)
    loss, per, state = ops.selfsim_loss(x.to(hip_device), c.to(hip_device), 1.0)
    l64, per64 = R.loss(x, c)
    e_l = max(abs(float(loss) - float(l64)), float((per.cpu().double() - per64).abs().max()))
    pos, neg = state[5], state[6]
    assert pos.dtype == neg.dtype == torch.int64 and tuple(pos.shape) == tuple(neg.shape) == (n, npix, (npix + 63) // 64)
    assert int((pos & neg).ne(0).sum()) == 0
    s, stray = R.unpack_planes(pos, neg, npix)
    diagonal = int(s.diagonal(dim1=1, dim2=2).ne(0).sum())
    wrong, outside = R.check_signs(s, x, c)
    e_t = float((_flat(state[4]).double() - R.signed_sums(x, c, signs=s)).abs().max())
    print(f"selfsim_loss {name}: loss {float(loss):.6f} (float64 {float(l64):.6f}), error {e_l:.2e} (bar {OP_TOL:.0e}); "
          f"{wrong} of {n * npix * (npix - 1)} signs differ from float64, {outside} outside the margin; t error "
          f"{e_t:.2e}; {stray} bits past N, {diagonal} on the diagonal")
    assert e_l <= OP_TOL and outside == 0 and e_t <= OP_TOL and stray == 0 and diagonal == 0
    if name == "s8_one_pixel":
        assert float(loss) == 0.0 and int(pos.ne(0).sum()) == 0 and int(neg.ne(0).sum()) == 0
    half = ops.selfsim_loss(x.to(hip_device), c.to(hip_device), 0.5)[0]
    assert abs(float(half) - 0.5 * float(l64)) <= OP_TOL


@pytest.mark.parametrize("name", list(R.CASES))
def test_backward_against_float64(name, hip_device):
    x, c = _case(name)
    xd, cd = x.to(hip_device), c.to(hip_device)
    weight, g = 0.8, 1.5
    _, _, state = ops.selfsim_loss(xd, cd, weight)
    dx = ops.selfsim_loss_backward(xd, state, _one(hip_device, g), weight).cpu()
    s, _ = R.unpack_planes(state[5], state[6], _npix(x))
    ref = R.grad(x, c, weight, g, signs=s)
    assert tuple(dx.shape) == tuple(x.shape) and bool(torch.isfinite(dx).all())
    err = R.grad_error(dx, x, c, weight, g, signs=s)
    e_emu = R.grad_error(R.grad(x, c, weight, g, dtype=torch.float32, signs=s), x, c, weight, g, signs=s)
    print(f"selfsim_loss_backward {name}: rel_inf {err:.2e} (bar {OP_TOL:.0e}; the fp32 emulation: {e_emu:.2e}); "
          f"max |grad| {float(ref.abs().max()):.2e}, max |dx| {float(dx.abs().max()):.2e}")
    assert err <= OP_TOL
    if name == "s8_one_pixel":
        assert float(dx.abs().max()) == 0.0


# ---- equal maps, zero vectors, non-finite values ----------------------------------------------------------

def test_equal_maps_give_exactly_zero(hip_device):
    for name in ("s64_tiles", "s160_chunks"):
        x = _case(name)[0].to(hip_device)
        loss, per, state = ops.selfsim_loss(x, x.clone(), 1.0)
        dx = ops.selfsim_loss_backward(x, state, _one(hip_device), 1.0)
        got = [float(loss), float(per.abs().max()), int(state[5].ne(0).sum()), int(state[6].ne(0).sum()),
               float(state[4].abs().max()), float(dx.abs().max())]
        print(f"{name}, x == c: loss, per-sample, pos bits, neg bits, |t|, |dx| = {got}")
        assert got == [0.0, 0.0, 0, 0, 0.0, 0.0]


def test_zero_vectors(hip_device):
    x = R.features(12910, (1, 8, 9, 10)) + 0.01
    c = R.features(12911, (1, 8, 9, 10)) + 0.01
    x[:, :, 2, 3] = 0.0            # pixel 23 of x
    c[:, :, 7, 4] = 0.0            # pixel 74 of c, in the second tile
    xd, cd = x.to(hip_device), c.to(hip_device)
    u = ops.cosine_norms(xd)
    assert float(u[0, 2, 3]) == 0.0 and float(ops.cosine_norms(cd)[0, 7, 4]) == 0.0
    assert float(ops.selfsim_colsum(xd, u)[0, 2, 3]) == 89.0          # distance 1 from each of the other 89 pixels
    loss, per, state = ops.selfsim_loss(xd, cd, 1.0)
    dx = ops.selfsim_loss_backward(xd, state, _one(hip_device), 1.0)
    l64 = float(R.loss(x, c)[0])
    print(f"zero vectors: loss {float(loss):.6f} (float64 {l64:.6f}); max |dx| {float(dx.abs().max()):.2e}")
    assert abs(float(loss) - l64) <= OP_TOL and all(bool(torch.isfinite(t).all()) for t in state[:5])
    assert bool(torch.isfinite(dx).all()) and float(dx[0, :, 2, 3].abs().max()) == 0.0 and float(dx.abs().max()) > 0
    s, _ = R.unpack_planes(state[5], state[6], 90)
    assert R.rel_inf(dx.cpu(), R.grad(x, c, signs=s)) <= OP_TOL


def test_nan_stays_inside_its_sample(hip_device):
    x, c = (t.to(hip_device) for t in _case("s48_k_tails"))
    xn, cn = x.clone(), c.clone()
    xn[1, 5, 3, 4] = float("nan")
    cn[1, 7, 2, 2] = float("inf")
    a, b = ops.selfsim_loss(x, c, 1.0), ops.selfsim_loss(xn, cn, 1.0)
    da = ops.selfsim_loss_backward(x, a[2], _one(hip_device), 1.0)
    db = ops.selfsim_loss_backward(xn, b[2], _one(hip_device), 1.0)
    bad = [_mismatches(s[0], t[0]) for s, t in zip(a[2], b[2])] + [_mismatches(a[1][0], b[1][0]), _mismatches(da[0], db[0])]
    print(f"NaN / inf in sample 1: mismatches in sample 0 (state, per-sample loss, gradient): {bad}")
    assert not any(bad)


# ---- composition, autograd, determinism, graphs, the registered op -------------------------------------------

def test_stages_compose_to_the_whole_op_bitwise(hip_device):
    for name in ("s48_k_tails", "s32_many_tiles", "s512_model_c"):
        x, c = (t.to(hip_device) for t in _case(name))
        loss, per, state = ops.selfsim_loss(x, c, 0.9)
        u, v = ops.cosine_norms(x), ops.cosine_norms(c)
        rx, rc = ops.selfsim_colsum(x, u), ops.selfsim_colsum(c, v)
        sums, t, pos, neg = ops.selfsim_pairs(x, c, u, v, rx, rc)
        sl = ops.selfsim_total(sums, 0.9)
        bad = [_mismatches(a, b) for a, b in zip((u, v, rx, rc, t, pos, neg, sums, sl.reshape(1)),
                                                 tuple(state) + (per, loss.reshape(1)))]
        print(f"{name}: stages vs the whole op: {bad} mismatches")
        assert not any(bad)


def test_autograd_equals_the_backward_kernels_bitwise(hip_device):
    x, c = (t.to(hip_device) for t in _case("s64_tiles"))
    xg, cg = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    loss = losses.compute_selfsim_loss(xg, cg, 0.7)
    dx, dc = torch.autograd.grad(2.0 * loss, (xg, cg), allow_unused=True)
    want_loss, _, state = ops.selfsim_loss(x, c, 0.7)
    want = ops.selfsim_loss_backward(x, state, _one(hip_device, 2.0), 0.7)
    bad = [_mismatches(loss.reshape(1), want_loss.reshape(1)), _mismatches(dx, want)]
    print(f"compute_selfsim_loss vs ops: {bad} mismatches (loss, gradient)")
    assert bad == [0, 0] and dc is None and float(want.abs().max()) > 0


def _everything(x, c, one):
    loss, per, state = ops.selfsim_loss(x, c, 1.0)
    dx = ops.selfsim_loss_backward(x, state, one, 1.0)
    return (loss.reshape(1), per, dx) + tuple(state)


def test_run_twice_bitwise(hip_device):
    for name in ("s64_tiles", "s32_many_tiles", "s512_model_c"):
        x, c = (t.to(hip_device) for t in _case(name))
        a, b = (_everything(x, c, _one(hip_device)) for _ in range(2))
        bad = [_mismatches(s, t) for s, t in zip(a, b)]
        assert not any(bad), (name, bad)


def test_graph_replay_equals_eager(hip_device):
    x, c = (t.to(hip_device) for t in _case("s64_tiles"))
    one = _one(hip_device)
    eager = _everything(x, c, one)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            out = _everything(x, c, one)
    finally:
        gc.enable()
    for t in out:
        t.fill_(0) if t.dtype != torch.float32 else t.fill_(float("nan"))
    g.replay()
    g.replay()   # the accumulator's zero fill is captured too: a second replay gives the same loss
    torch.cuda.synchronize()
    bad = [_mismatches(s, t) for s, t in zip(eager, out)]
    print(f"graph replay vs eager: {bad} mismatches")
    assert not any(bad)


def test_registered_op_equals_ctypes_path_bitwise(hip_device):
    x, c = (t.to(hip_device) for t in _case("s160_chunks"))
    out = torch.ops.ast_hip.selfsim_loss(x, c, 0.6)
    loss, per, state = ops.selfsim_loss(x, c, 0.6)
    bad = [_mismatches(a, b) for a, b in zip(out, (loss.reshape(1), per) + tuple(state))]
    assert not any(bad), bad
    m = torch.device("meta")
    fake = torch.ops.ast_hip.selfsim_loss(x.to(m), c.to(m), 0.6)
    assert [(tuple(t.shape), t.dtype) for t in fake] == [(tuple(t.shape), t.dtype) for t in out]


def test_wrappers_reject_bad_inputs(hip_device):
    d = hip_device
    f = lambda *s: torch.zeros(*s, device=d)  # noqa: E731
    bad = [
        lambda: ops.selfsim_loss(torch.zeros(1, 8, 2, 2), f(1, 8, 2, 2)),               # a CPU tensor
        lambda: ops.selfsim_loss(f(1, 8, 2, 2), torch.zeros(1, 8, 2, 2)),
        lambda: ops.selfsim_loss(f(1, 8, 2, 2), f(1, 9, 2, 2)),                          # shape mismatches
        lambda: ops.selfsim_loss(f(1, 8, 2, 2), f(1, 8, 2, 3)),
        lambda: ops.selfsim_loss(f(2, 8, 2, 2), f(1, 8, 2, 2)),
        lambda: ops.selfsim_loss(f(8, 2, 2), f(8, 2, 2)),                                # not 4-D
        lambda: ops.selfsim_loss(f(1, 8, 2, 2).double(), f(1, 8, 2, 2)),                 # not float32
        lambda: ops.selfsim_loss(f(1, 8, 0, 2), f(1, 8, 0, 2)),                          # empty
        lambda: ops.selfsim_loss(f(1, ops.REMD_MAX_C + 1, 1, 1), f(1, ops.REMD_MAX_C + 1, 1, 1)),   # past the limits
        lambda: ops.selfsim_loss(f(1, 1, 1, ops.SELFSIM_MAX_PIXELS + 1), f(1, 1, 1, ops.SELFSIM_MAX_PIXELS + 1)),
        lambda: ops.selfsim_colsum(f(1, 8, 2, 2), f(1, 2, 3)),
        lambda: ops.selfsim_pairs(f(1, 8, 2, 2), f(1, 8, 2, 2), f(1, 2, 2), f(1, 2, 2), f(1, 2, 2), f(1, 2, 2).double()),
        lambda: losses.compute_selfsim_loss(f(1, 8, 2, 2), f(1, 8, 3, 2)),
    ]
    for call in bad:
        with pytest.raises(_lib.HipOpError):
            call()
    x, c = f(1, 8, 2, 2) + 1, f(1, 8, 2, 2) + 1
    _, _, state = ops.selfsim_loss(x, c)
    with pytest.raises(_lib.HipOpError):
        ops.selfsim_loss_backward(x, state, torch.tensor(1.0), 1.0)                     # the scalar on the CPU
    with pytest.raises(_lib.HipOpError):
        ops.selfsim_loss_backward(x, state[:5] + (state[5].int(), state[6]), _one(d), 1.0)   # a plane of the wrong dtype
    with pytest.raises(_lib.HipOpError):
        ops.selfsim_loss_backward(x, state[:6], _one(d), 1.0)


# ---- trainer ------------------------------------------------------------------------------------------

def _trainer(dev, **kw):
    from arbitrarystyletransfer_amd.train import AdaINTrainer, default_args
    torch.manual_seed(1234)
    return AdaINTrainer(default_args(batch_size=2, image_size=64, **kw), device=dev)


def test_trainer_term(hip_device):
    from arbitrarystyletransfer_amd import train
    assert train.default_args().selfsim_lam == 0.0
    c = torch.from_numpy(synth.image(4321, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(4322, (2, 3, 64, 64))).to(hip_device)
    base, tr, both = _trainer(hip_device), _trainer(hip_device, selfsim_lam=1.0), _trainer(hip_device, selfsim_lam=1.0,
                                                                                          remd_lam=1.0)
    tr.net.load_state_dict(base.net.state_dict())
    both.net.load_state_dict(base.net.state_dict())
    out0 = base.compute_losses(c, s)
    assert "selfsim_loss" not in out0
    out0["loss"].backward()
    g0 = [p.grad.clone() for p in base.params]
    out1 = tr.compute_losses(c, s)
    with torch.no_grad():
        taps, s_taps = tr.lossnet(c, s), tr.lossnet(out1["stylized"])
        want = sum(losses.compute_selfsim_loss(s_taps[i], taps[i][:2])
                   for i in (train._tap_index(k, "selfsim_taps") for k in tr.args.selfsim_taps))
    assert _mismatches(out1["selfsim_loss"].reshape(1), want.reshape(1)) == 0 and float(want) > 0
    total = float(out0["loss"].detach()) + 1.0 * float(out1["selfsim_loss"].detach())
    got = float(out1["loss"].detach())
    print(f"trainer: selfsim_loss {float(want):.6f}; loss {got:.6f} vs base + term {total:.6f}")
    assert abs(got - total) <= 1e-6 * abs(total)
    assert set(out1) - set(out0) == {"selfsim_loss"}
    out1["loss"].backward()
    g1 = [p.grad.clone() for p in tr.params]
    assert all(bool(torch.isfinite(g).all()) for g in g1)
    assert any(_mismatches(a, b) for a, b in zip(g0, g1))
    out2 = both.compute_losses(c, s)
    assert set(out2) - set(out0) == {"selfsim_loss", "remd_loss"}
    assert _mismatches(out2["selfsim_loss"].reshape(1), want.reshape(1)) == 0


def test_trainer_step_is_deterministic(hip_device):
    c = torch.from_numpy(synth.image(4321, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(4322, (2, 3, 64, 64))).to(hip_device)
    a, b = _trainer(hip_device, selfsim_lam=1.0), _trainer(hip_device, selfsim_lam=1.0)
    b.net.load_state_dict(a.net.state_dict())
    keys = list(a.train_dict)
    oa, ob = a.train_step(c, s, record=True), b.train_step(c, s, record=True)
    assert list(a.train_dict) == keys == ["content_loss", "style_loss", "lf_loss", "tv_loss", "org_img_loss"]
    bad = [_mismatches(oa[k].reshape(-1), ob[k].reshape(-1)) for k in ("loss", "selfsim_loss", "grad_norm")]
    bad += [_mismatches(p, q) for p, q in zip(a.params, b.params)]
    assert not any(bad), bad
