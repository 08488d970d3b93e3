"""GPU: the contextual loss (csrc/cx.hip: centring, the two soft passes over the match tile, value, the
recomputing backward) and its wrapper / autograd / registered-op / trainer surface, against tests/cx_ref.py.

Bars (cx_ref.py derives them; none comes from the code under test), with kappa the case's amplification
from an error in a distance to a relative error in a weight and OP_TOL = 2e-5: S and E within kappa OP_TOL
relative of float64; col_cx within 2 kappa OP_TOL relative of the float64 value at the returned index, that
value at least (1 - 4 kappa OP_TOL) of the float64 maximum; -log CX_b within 2 kappa OP_TOL; the gradient
within 4 kappa OP_TOL rel_inf of the float64 analytic gradient at the GPU's own indices. The centred maps and
the means are one subtraction and one mean: OP_TOL absolute. Everything else is bit for bit.
"""
import functools
import gc

import pytest
import torch

import cx_ref as X
from arbitrarystyletransfer_amd import _lib, functional, library, losses, ops, synth  # noqa: F401  (registers the ops)

pytestmark = pytest.mark.gpu

OP_TOL = X.OP_TOL


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


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _mismatches(got, ref):
    return int((_bits(got) != _bits(ref)).sum())


def _flat(t):
    return t.cpu().reshape(t.shape[0], -1)


def _one(dev, v=1.0):
    return torch.tensor(v, device=dev)


def _rel(got, ref):
    return float(((got.double() - ref) / ref).abs().max())


def _stages(x, y, h, center=True, splits=0):
    """Every stage through its own wrapper: a dict of device tensors."""
    if center:
        mu, xc, yc = ops.cx_center(x, y)
    else:
        mu, xc, yc = None, x, y
    u, v = ops.cosine_norms(xc), ops.cosine_norms(yc)
    rmin, ridx, _, _ = ops.cosine_match(xc, yc)
    S, E = ops.cx_rowsum(xc, yc, u, v, rmin, h, _splits=splits)
    ccx, cidx, cdist = ops.cx_colmax(xc, yc, u, v, rmin, S, h, _splits=splits)
    return dict(mu=mu, xc=xc, yc=yc, u=u, v=v, rmin=rmin, ridx=ridx, S=S, E=E, ccx=ccx, cidx=cidx, cdist=cdist)


# ---- the stages and the whole forward ---------------------------------------------------------------------

@pytest.mark.parametrize("name", X.ALL_CASES)
def test_stages_and_forward_against_float64(name, hip_device):
    x, y, h = _case(name)
    q, kap = _parts(name), _kappa(name)
    bar = kap * OP_TOL
    xd, yd = x.to(hip_device), y.to(hip_device)
    s = _stages(xd, yd, h)
    n, M, P = q["d"].shape
    e_c = max(float((s["xc"].cpu().double() - q["xc"]).abs().max()), float((s["yc"].cpu().double() - q["yc"]).abs().max()),
              float((s["mu"].cpu().double() - y.double().flatten(2).mean(dim=2)).abs().max()))
    e_s, e_e = _rel(_flat(s["S"]), q["S"]), _rel(_flat(s["E"]), q["E"])
    a = _flat(s["cidx"]).long()
    assert s["cidx"].dtype == torch.int32 and 0 <= int(a.min()) and int(a.max()) < M
    at = q["cx"].transpose(1, 2).gather(2, a[..., None])[..., 0]
    e_cx, short = _rel(_flat(s["ccx"]), at), float((at / q["c"]).min())
    d_at = q["d"].transpose(1, 2).gather(2, a[..., None])[..., 0]
    e_d = float((_flat(s["cdist"]).double() - d_at).abs().max())
    loss, cxb, state = ops.cx_loss(xd, yd, 0.9, h)
    e_l = float((-torch.log(cxb.cpu().double()) + torch.log(q["cxb"])).abs().max())
    want = 0.9 * float((-torch.log(q["cxb"])).mean())
    print(f"cx {name}: centring {e_c:.2e}, col_dist {e_d:.2e} (bar {OP_TOL:.0e}); S {e_s:.2e}, E {e_e:.2e} (bar {bar:.2e}); "
          f"col_cx {e_cx:.2e} (bar {2 * bar:.2e}); value at the index / maximum {short:.6f} (bar {1 - 4 * bar:.6f}); "
          f"-log CX {e_l:.2e} (bar {2 * bar:.2e}); loss {float(loss):.6f} (float64 {want:.6f})")
    assert e_c <= OP_TOL and e_d <= OP_TOL
    assert max(e_s, e_e) <= bar and e_cx <= 2 * bar and short >= 1 - 4 * bar and e_l <= 2 * bar
    assert abs(float(loss) - want) <= 0.9 * 2 * bar
    assert tuple(cxb.shape) == (n,) and tuple(state[8].shape) == (n,) + tuple(y.shape[2:])


@pytest.mark.parametrize("name", X.ALL_CASES)
def test_backward_against_float64(name, hip_device):
    x, y, h = _case(name)
    bar = 4 * _kappa(name) * OP_TOL
    xd, yd = x.to(hip_device), y.to(hip_device)
    weight, g = 0.8, 1.5
    _, _, state = ops.cx_loss(xd, yd, weight, h)
    dx = ops.cx_loss_backward(xd, yd, state, _one(hip_device, g), weight, h).cpu()
    index = (state[5].cpu(), state[9].cpu())
    ref = X.grad(x, y, weight, g, h, index=index)
    emu = X.grad(x, y, weight, g, h, torch.float32, index)
    err, e_emu = X.grad_err(dx, ref), X.grad_err(emu, ref)
    print(f"cx_loss_backward {name}: rel_inf {err:.2e} (bar {bar:.2e}; the fp32 emulation: {e_emu:.2e}); max |grad| "
          f"{float(ref.abs().max()):.2e}")
    assert tuple(dx.shape) == tuple(x.shape) and bool(torch.isfinite(dx).all()) and err <= bar


# ---- exact cases ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("center", [True, False])
def test_one_style_pixel_is_exact(center, hip_device):
    """P = 1: D(i, m_i) is the only distance of the row, so w / S is 1 only if the row pass reproduces row_min
    in bits."""
    x, y = X.features(12910, (1, 16, 5, 30)), X.features(12911, (1, 16, 1, 1))
    xd, yd = x.to(hip_device), y.to(hip_device)
    s = _stages(xd, yd, 0.5, center)
    loss, cxb, state = ops.cx_loss(xd, yd, 1.0, 0.5, center)
    dx = ops.cx_loss_backward(xd, yd, state, _one(hip_device), 1.0, 0.5).cpu()
    bar = 4 * X.kappa(x, y, 0.5, center) * OP_TOL
    print(f"one style pixel, center={center}: col_cx {s['ccx'].flatten().tolist()}, loss {float(loss)}, max |dx| "
          f"{float(dx.abs().max()):.2e} (bar {bar:.2e})")
    assert float(s["ccx"].flatten()[0]) == 1.0 and int(s["cidx"].flatten()[0]) == 0
    assert float(cxb[0]) == 1.0 and float(loss) == 0.0
    assert float(dx.abs().max()) <= bar


@pytest.mark.parametrize("splits", [1, 3])
def test_exact_ties_take_the_lowest_index(splits, hip_device):
    """Content pixels i and i + 90 are equal bit for bit and sit in different 64-pixel tiles and workgroups:
    their sums are equal in bits and the lower one wins every column."""
    by, bx = X.features(11910, (1, 16, 1, 100)), X.features(11911, (1, 16, 1, 90))
    y, x = torch.cat([by, by], dim=3), torch.cat([bx, bx], dim=3)
    s = _stages(x.to(hip_device), y.to(hip_device), 0.5, splits=splits)
    hi = int((s["cidx"] >= 90).sum())
    print(f"duplicates, {splits} split(s): {hi} column indices are the higher duplicate")
    assert hi == 0
    assert _mismatches(s["S"][..., :90], s["S"][..., 90:]) == 0 and _mismatches(s["E"][..., :90], s["E"][..., 90:]) == 0
    assert _mismatches(s["ccx"][..., :100], s["ccx"][..., 100:]) == 0


@pytest.mark.parametrize("name", ["c512_split_keys", "c160_tile_tails"])
def test_split_counts(name, hip_device):
    x, y, h = _case(name)
    q, bar = _parts(name), _kappa(name) * OP_TOL
    s = _stages(x.to(hip_device), y.to(hip_device), h)
    cols, errs = [], []
    for k in (1, 4, 0):
        S, E = ops.cx_rowsum(s["xc"], s["yc"], s["u"], s["v"], s["rmin"], h, _splits=k)
        errs += [_rel(_flat(S), q["S"]), _rel(_flat(E), q["E"])]
        cols.append(ops.cx_colmax(s["xc"], s["yc"], s["u"], s["v"], s["rmin"], s["S"], h, _splits=k))
    bad = [_mismatches(a, b) for other in cols[1:] for a, b in zip(cols[0], other)]
    print(f"{name}: colmax 1 split vs 4 vs the library's choice: {bad} mismatches; rowsum errors {['%.2e' % e for e in errs]} "
          f"(bar {bar:.2e})")
    assert bad == [0] * 6 and max(errs) <= bar


def test_inactive_rows_get_exactly_zero(hip_device):
    x, y, h = _case("c32_many_queries")
    xd, yd = x.to(hip_device), y.to(hip_device)
    _, _, state = ops.cx_loss(xd, yd, 1.0, h)
    dx = ops.cx_loss_backward(xd, yd, state, _one(hip_device), 1.0, h).cpu().flatten(2)
    chosen = torch.zeros(460, dtype=torch.bool)
    chosen[state[9].cpu().flatten().long()] = True
    print(f"c32_many_queries: {int((~chosen).sum())} of 460 rows chosen by no column")
    assert int((~chosen).sum()) >= 400
    assert float(dx[0][:, ~chosen].abs().max()) == 0.0 and float(dx[0][:, chosen].abs().min(dim=0).values.max()) > 0


def test_a_tile_without_an_active_row_is_skipped(hip_device):
    """Rows 128 .. 191, a whole 64-row tile, point away from every target pixel: no column chooses them, the
    dense pass skips the tile and its gradient is exactly zero; the other rows keep the bar."""
    x, y, h = _case("c32_many_queries")
    x = x.clone()
    xc, yc = X.center(x, y)
    away = -X.R.normalized(yc)[0].mean(dim=0)                                  # [C]
    mu = y.double().flatten(2).mean(dim=2)[0]
    rows = torch.arange(128, 192)
    x.flatten(2)[0][:, rows] = (mu[:, None] + away[:, None] * (1.0 + 0.01 * torch.arange(64.0))[None, :]).float()
    q, kap = X.parts(x, y, h), X.kappa(x, y, h)
    assert kap * OP_TOL <= X.KAPPA_TOL_MAX and not bool(((q["a"][0] >= 128) & (q["a"][0] < 192)).any())
    xd, yd = x.to(hip_device), y.to(hip_device)
    _, _, state = ops.cx_loss(xd, yd, 0.8, h)
    a = state[9].cpu().flatten().long()
    assert not bool(((a >= 128) & (a < 192)).any())
    dx = ops.cx_loss_backward(xd, yd, state, _one(hip_device, 1.5), 0.8, h).cpu()
    ref = X.grad(x, y, 0.8, 1.5, h, index=(state[5].cpu(), state[9].cpu()))
    err = X.grad_err(dx, ref)
    print(f"tile skip: rel_inf {err:.2e} (bar {4 * kap * OP_TOL:.2e})")
    assert float(dx.flatten(2)[0][:, rows].abs().max()) == 0.0 and err <= 4 * kap * OP_TOL


def test_zero_vectors(hip_device):
    x, y = X.features(11912, (1, 8, 9, 10)) + 0.01, X.features(11913, (1, 8, 7, 11)) + 0.01
    xd, yd = x.to(hip_device), y.to(hip_device)
    mu, _, _ = ops.cx_center(xd, yd)
    xd[0, :, 2, 3] = mu[0]                       # content pixel 23 equals mu: a zero vector after centring
    loss, cxb, state = ops.cx_loss(xd, yd, 1.0, 0.5)
    dx = ops.cx_loss_backward(xd, yd, state, _one(hip_device), 1.0, 0.5)
    assert float(state[2][0, 2, 3]) == 0.0 and float(state[4][0, 2, 3]) == 1.0     # u = 0, distance 1 to everything
    assert all(bool(torch.isfinite(t).all()) for t in (loss, cxb, dx) + tuple(state[2:]))
    assert float(dx[0, :, 2, 3].abs().max()) == 0.0 and float(dx.abs().max()) > 0
    xz, yz = x.to(hip_device), y.to(hip_device)
    xz[0, :, 4, 4] = 0.0
    yz[0, :, 6, 4] = 0.0                         # and without centring, on both sides
    loss, cxb, state = ops.cx_loss(xz, yz, 1.0, 0.5, center=False)
    dx = ops.cx_loss_backward(xz, yz, state, _one(hip_device), 1.0, 0.5)
    assert float(state[2][0, 4, 4]) == 0.0 and float(state[3][0, 6, 4]) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in (loss, cxb, dx) + tuple(state[2:]))
    assert float(dx[0, :, 4, 4].abs().max()) == 0.0


def test_nan_stays_inside_its_sample(hip_device):
    x, y, h = _case("c48_k_tails")
    x, y = x.to(hip_device), y.to(hip_device)
    xn, yn = x.clone(), y.clone()
    xn[1, 5, 3, 4] = float("nan")
    yn[1, 7, 2, 2] = float("inf")
    a, b = ops.cx_loss(x, y, 1.0, h), ops.cx_loss(xn, yn, 1.0, h)
    da = ops.cx_loss_backward(x, y, a[2], _one(hip_device), 1.0, h)
    db = ops.cx_loss_backward(xn, yn, b[2], _one(hip_device), 1.0, h)
    bad = [_mismatches(s[0], t[0]) for s, t in zip(a[2], b[2])] + [_mismatches(da[0], db[0]), _mismatches(a[1][:1], b[1][:1])]
    print(f"NaN / inf in sample 1: mismatches in sample 0 (state, gradient, CX): {bad}")
    assert not any(bad)
    cidx = b[2][9]
    assert int(cidx.min()) >= 0 and int(cidx.max()) < x.shape[2] * x.shape[3]      # a NaN never wins
    xr = x.clone()
    xr[1, :, 0, 0] = float("nan")                                                  # one NaN row of sample 1
    s = _stages(xr, y, h)
    assert int((s["cidx"][1] == 0).sum()) == 0 and bool(torch.isfinite(s["ccx"][1]).all())


def test_center_off_equals_hand_centred_maps_bitwise(hip_device):
    x, y, h = _case("c64_shared_style")
    x, y = x.to(hip_device), y.to(hip_device)
    mu, xc, yc = ops.cx_center(x, y)
    hx, hy = x - mu[:, :, None, None], y - mu[:, :, None, None]
    assert _mismatches(hx, xc) == 0 and _mismatches(hy, yc) == 0
    on, off = ops.cx_loss(x, y, 0.7, h, True), ops.cx_loss(hx, hy, 0.7, h, False)
    assert off[2][0].numel() == 0 and off[2][1].numel() == 0
    d_on = ops.cx_loss_backward(x, y, on[2], _one(hip_device), 0.7, h)
    d_off = ops.cx_loss_backward(hx, hy, off[2], _one(hip_device), 0.7, h)
    bad = [_mismatches(on[0].reshape(1), off[0].reshape(1)), _mismatches(on[1], off[1]), _mismatches(d_on, d_off)]
    bad += [_mismatches(s, t) for s, t in zip(on[2][2:], off[2][2:])]
    print(f"center on vs hand-centred maps with center off: {bad} mismatches")
    assert not any(bad)


def test_stages_compose_to_the_whole_op_bitwise(hip_device):
    for name in ("c48_k_tails", "c512_split_keys", "c160_tile_tails_h01"):
        x, y, h = _case(name)
        x, y = x.to(hip_device), y.to(hip_device)
        loss, cxb, state = ops.cx_loss(x, y, 0.9, h)
        s = _stages(x, y, h)
        sl, scx = ops.cx_value(s["ccx"], 0.9)
        got = tuple(s[k] for k in ("xc", "yc", "u", "v", "rmin", "ridx", "S", "E", "ccx", "cidx", "cdist")) + (scx,)
        bad = [_mismatches(a, b) for a, b in zip(got, state)] + [_mismatches(sl.reshape(1), loss.reshape(1)),
                                                                 _mismatches(scx, cxb)]
        print(f"{name}: stages vs the whole op: {bad} mismatches")
        assert not any(bad)


# ---- the paths above the C ABI -------------------------------------------------------------------------------

def test_autograd_paths_equal_the_ctypes_path_bitwise(hip_device):
    x, y, h = _case("c64_shared_style")
    x, y = x.to(hip_device), y.to(hip_device)
    want_loss, _, state = ops.cx_loss(x, y, 0.7, h)
    want = ops.cx_loss_backward(x, y, state, _one(hip_device, 2.0), 0.7, h)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    loss = losses.compute_contextual_loss(xg, yg, 0.7, h)
    (dx,) = torch.autograd.grad(2.0 * loss, xg)
    bad = [_mismatches(loss.reshape(1), want_loss.reshape(1)), _mismatches(dx, want)]
    print(f"compute_contextual_loss vs ops: {bad} mismatches (loss, gradient)")
    assert bad == [0, 0]


@pytest.mark.parametrize("center", [True, False])
def test_registered_op_equals_ctypes_path_bitwise(center, hip_device):
    x, y, h = _case("c160_tile_tails")
    x, y = x.to(hip_device), y.to(hip_device)
    out = torch.ops.ast_hip.cx_loss(x, y, 0.6, h, center)
    loss, _, state = ops.cx_loss(x, y, 0.6, h, center)
    bad = [_mismatches(a, b) for a, b in zip(out, (loss.reshape(1),) + tuple(state))]
    assert len(out) == 13 and not any(bad), bad
    m = torch.device("meta")
    fake = torch.ops.ast_hip.cx_loss(x.to(m), y.to(m), 0.6, h, center)
    assert [(tuple(t.shape), t.dtype) for t in fake] == [(tuple(t.shape), t.dtype) for t in out]
    xg = x.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(torch.ops.ast_hip.cx_loss(xg, y, 0.6, h, center)[0], xg)
    assert _mismatches(dx, ops.cx_loss_backward(x, y, state, _one(hip_device), 0.6, h)) == 0


def test_target_gets_no_gradient(hip_device):
    x, y, h = _case("c48_k_tails")
    x, y = (t.to(hip_device).requires_grad_(True) for t in (x, y))
    loss = losses.compute_contextual_loss(x, y)
    dx, dy = torch.autograd.grad(loss, (x, y), allow_unused=True)
    assert dy is None and dx is not None and float(dx.abs().max()) > 0
    small = X.features(11914, (2, 48, 3, 4)).to(hip_device)                  # a target of another size, a batch of 1
    assert bool(torch.isfinite(losses.compute_contextual_loss(x, small[:1])))


def _everything(x, y, h, one):
    loss, cxb, state = ops.cx_loss(x, y, 1.0, h)
    dx = ops.cx_loss_backward(x, y, state, one, 1.0, h)
    return (loss.reshape(1), cxb, dx) + tuple(state)


def test_run_twice_bitwise(hip_device):
    for name in ("c64_shared_style", "c32_many_queries", "c24_few_content", "c512_split_keys_h01"):
        x, y, h = _case(name)
        x, y = x.to(hip_device), y.to(hip_device)
        a, b = (_everything(x, y, h, _one(hip_device)) for _ in range(2))
        bad = [_mismatches(s, t) for s, t in zip(a, b)]
        assert not any(bad), (name, bad)


def test_graph_replay_equals_eager(hip_device):
    x, y, h = _case("c64_shared_style")
    x, y = x.to(hip_device), y.to(hip_device)
    one = _one(hip_device)
    eager = _everything(x, y, h, one)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            out = _everything(x, y, h, one)
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


def test_wrappers_reject_bad_inputs(hip_device):
    d = hip_device
    f = lambda *s: torch.zeros(*s, device=d)  # noqa: E731
    bad = [
        lambda: ops.cx_loss(torch.zeros(1, 8, 2, 2), f(1, 8, 2, 2)),                  # a CPU tensor
        lambda: ops.cx_loss(f(1, 8, 2, 2), torch.zeros(1, 8, 2, 2)),
        lambda: ops.cx_center(f(1, 8, 2, 2), f(1, 9, 2, 2)),                           # C mismatch
        lambda: ops.cx_loss(f(3, 8, 2, 2), f(2, 8, 2, 2)),                             # a target batch neither N nor 1
        lambda: ops.cx_loss(f(1, 8, 0, 2), f(1, 8, 2, 2)),                             # empty maps
        lambda: ops.cx_loss(f(1, 8, 2, 2), f(1, 8, 2, 0)),
        lambda: ops.cx_loss(f(8, 2, 2), f(1, 8, 2, 2)),                                # not 4-D
        lambda: ops.cx_loss(f(1, 8, 2, 2).double(), f(1, 8, 2, 2)),                    # not float32
        lambda: ops.cx_loss(f(1, ops.CX_MAX_C + 1, 1, 1), f(1, ops.CX_MAX_C + 1, 1, 1)),   # past the limits
        lambda: ops.cx_loss(f(1, 1, 1, 1), f(1, 1, 129, 128)),
        lambda: ops.cx_loss(f(1, 8, 2, 2), f(1, 8, 2, 2), h=0.0),                      # the bandwidth
        lambda: ops.cx_loss(f(1, 8, 2, 2), f(1, 8, 2, 2), h=-0.5),
        lambda: ops.cx_loss(f(1, 8, 2, 2), f(1, 8, 2, 2), h=float("inf")),
        lambda: ops.cx_loss(f(1, 8, 2, 2), f(1, 8, 2, 2), h=float("nan")),
        lambda: losses.compute_contextual_loss(f(1, 8, 2, 2), f(1, 9, 2, 2)),
        lambda: losses.compute_contextual_loss(f(1, 8, 2, 2), f(1, 8, 2, 2), h=0.0),
    ]
    for call in bad:
        with pytest.raises(_lib.HipOpError):
            call()
    x, y = f(1, 8, 2, 2) + 1, f(1, 8, 2, 2) + 1
    _, _, state = ops.cx_loss(x, y)
    with pytest.raises(_lib.HipOpError):
        ops.cx_loss_backward(x, y, state, torch.tensor(1.0), 1.0)                      # the scalar on the CPU
    with pytest.raises(_lib.HipOpError):
        ops.cx_loss_backward(x, y, state[:9] + (state[9].long(),) + state[10:], _one(d), 1.0)
    with pytest.raises(_lib.HipOpError):
        ops.cx_loss_backward(x, y, state[:11], _one(d), 1.0)
    with pytest.raises(_lib.HipOpError):
        ops.cx_loss_backward(x, y, state, _one(d), 1.0, h=0.0)
    # the C ABI itself: a short workspace and a bad bandwidth are refused before any launch
    L, p = _lib.lib(), _lib.ptr
    u, v = ops.cosine_norms(x), ops.cosine_norms(y)
    rmin = ops.cosine_match(x, y)[0]
    S, E, ws = torch.full_like(rmin, -7.0), torch.full_like(rmin, -7.0), torch.zeros(4096, device=d)
    nb = int(L.ast_cx_rowsum_workspace_bytes(1, 1, 4, 4, 0))
    assert L.ast_cx_rowsum_f32(p(x), p(y), p(u), p(v), p(rmin), p(S), p(E), 1, 1, 8, 4, 4, 0.5, 0, p(ws), nb - 1, None) == -2
    assert L.ast_cx_rowsum_f32(p(x), p(y), p(u), p(v), p(rmin), p(S), p(E), 1, 1, 8, 4, 4, 0.0, 0, p(ws), nb, None) == -3
    assert L.ast_cx_rowsum_f32(p(x), p(y), p(u), p(v), p(rmin), p(S), p(E), 1, 1, ops.CX_MAX_C + 1, 4, 4, 0.5, 0, p(ws), nb,
                               None) == -3
    torch.cuda.synchronize()
    assert float(S.max()) == -7.0 and float(E.max()) == -7.0                           # nothing was launched


# ---- trainer ------------------------------------------------------------------------------------------

def _trainer(dev, **kw):
    from arbitrarystyletransfer_amd.train import AdaINTrainer, default_args
    torch.manual_seed(1234)
    return AdaINTrainer(default_args(batch_size=2, image_size=64, **kw), device=dev)


def test_trainer_terms(hip_device):
    from arbitrarystyletransfer_amd import train
    a = train.default_args()
    assert a.cx_lam == 0.0 and a.cx_content_lam == 0.0
    c = torch.from_numpy(synth.image(4321, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(4322, (2, 3, 64, 64))).to(hip_device)
    base, tr, both = _trainer(hip_device), _trainer(hip_device, cx_lam=1.0), _trainer(hip_device, cx_lam=1.0,
                                                                                   cx_content_lam=0.5)
    tr.net.load_state_dict(base.net.state_dict())
    both.net.load_state_dict(base.net.state_dict())
    out0 = base.compute_losses(c, s)
    assert "cx_loss" not in out0 and "cx_content_loss" not in out0
    out0["loss"].backward()
    g0 = [p.grad.clone() for p in base.params]
    out1, out2 = tr.compute_losses(c, s), both.compute_losses(c, s)
    with torch.no_grad():
        taps, s_taps = tr.lossnet(c, s), tr.lossnet(out1["stylized"])
        want = sum(losses.compute_contextual_loss(s_taps[i], taps[i][2:]) for i in (train._tap_index(k) for k in a.cx_taps))
        want_c = sum(losses.compute_contextual_loss(s_taps[i], taps[i][:2])
                     for i in (train._tap_index(k) for k in a.cx_content_taps))
    assert _mismatches(out1["cx_loss"].reshape(1), want.reshape(1)) == 0 and float(want) > 0
    assert _mismatches(out2["cx_loss"].reshape(1), want.reshape(1)) == 0
    assert _mismatches(out2["cx_content_loss"].reshape(1), want_c.reshape(1)) == 0 and float(want_c) > 0
    t1 = float(out0["loss"].detach()) + float(want)
    t2 = t1 + 0.5 * float(want_c)
    g1v, g2v = float(out1["loss"].detach()), float(out2["loss"].detach())
    print(f"trainer: cx_loss {float(want):.6f}, cx_content_loss {float(want_c):.6f}; loss {g1v:.6f} vs base + term "
          f"{t1:.6f}; with the content term {g2v:.6f} vs {t2:.6f}")
    assert abs(g1v - t1) <= 1e-6 * abs(t1) and abs(g2v - t2) <= 1e-6 * abs(t2)
    assert set(out1) - set(out0) == {"cx_loss"} and set(out2) - set(out0) == {"cx_loss", "cx_content_loss"}
    out1["loss"].backward()
    out2["loss"].backward()
    g1, g2 = [p.grad.clone() for p in tr.params], [p.grad.clone() for p in both.params]
    assert all(bool(torch.isfinite(g).all()) for g in g1 + g2)
    assert any(_mismatches(a_, b_) for a_, b_ in zip(g0, g1)) and any(_mismatches(a_, b_) for a_, b_ in zip(g1, g2))


def test_trainer_step_is_deterministic(hip_device):
    c = torch.from_numpy(synth.image(4321, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(4322, (2, 3, 64, 64))).to(hip_device)
    kw = dict(cx_lam=1.0, cx_content_lam=0.5)
    a, b = _trainer(hip_device, **kw), _trainer(hip_device, **kw)
    b.net.load_state_dict(a.net.state_dict())
    keys = list(a.train_dict)
    oa, ob = a.train_step(c, s, record=True), b.train_step(c, s, record=True)
    assert list(a.train_dict) == keys == ["content_loss", "style_loss", "lf_loss", "tv_loss", "org_img_loss"]
    bad = [_mismatches(oa[k].reshape(-1), ob[k].reshape(-1)) for k in ("loss", "cx_loss", "cx_content_loss", "grad_norm")]
    bad += [_mismatches(p, q) for p, q in zip(a.params, b.params)]
    assert not any(bad), bad
