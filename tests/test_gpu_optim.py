"""GPU parity of csrc/optim.hip (clip_grad_norm_ + Adam, eager and graph-capturable) against the
float64 reference of tests/optim_ref.py, which tests/test_optim_cpu.py pins to torch's own Adam.

Tolerances (none is taken from what the kernels give):
 * gradient norm: rtol 1e-5 against float64. Every summand is non-negative and the longest fp32
   addition chain is 256 serial adds per thread plus 8 tree levels, then about one add and 8 tree
   levels in the finish kernel: <= ~273 * 2^-24 = 1.6e-5 relative on the sum, half that on the root.
 * parameters and moments after N steps: torch's fp32 Adam + clip_grad_norm_ on the CPU runs on the
   same inputs; with e_t = max|torch32 - ref64| the HIP result must satisfy
   max|hip - ref64| <= 2 * e_t + 2 * ulp32(max|ref64|). The kernel's arithmetic is torch's; the
   factor 2 and the 2 ulp allow for FMA contraction on the device. The maxima run over all tensors
   of a test together (a one-element tensor has no meaningful error statistic of its own); an update
   that leaks across a tensor boundary is wrong by ~lr, far outside the bound.
 * step_static against step(): the device computes the bias corrections in double as the host does,
   but one fp32 ulp on lr/bc1 and one on sqrt(bc2) move an update of size <= ~lr by <= 2.4e-7
   relative: rtol 2e-7 per parameter plus atol N * lr * 3e-7 for parameters near zero.
 * clipped gradients: g * coef with coef computed in float64 from the norm the device reports (fp32
   add, divide and multiply: 3 roundings of 2^-24 = 1.8e-7), rtol 2e-7.

Gradients are synth.uniform streams times a seeded choice of {1e-4, 1, 1e2} per element (dynamic
range); parameters are uniform in +-0.1."""
import copy
import functools

import numpy as np
import pytest
import torch

import optim_ref as OR
from arbitrarystyletransfer_amd import optim, synth

pytestmark = pytest.mark.gpu

# multi-chunk tensors between single-chunk ones: 1 + 1 + 1 + 2 + 1 + 3 + 1 + 1 + 1 = 12 chunks of 65536
T_EDGE = ((1,), (65535,), (65536,), (65537,), (3,), (131073,), (7, 5), (64, 3, 3, 3), (1,))
assert OR.nchunks([int(np.prod(s)) for s in T_EDGE]) == 12
SCALES = np.array([1e-4, 1.0, 1e2])
ADAIN = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-5)


def numel(shape):
    return int(np.prod(shape))


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def make_params(shapes, seed=40):
    return tuple(frozen((synth.uniform(seed + i, numel(s)) * 0.1).astype(np.float32).reshape(s))
                 for i, s in enumerate(shapes))


def make_grad(seed, shape):
    n = numel(shape)
    pick = np.minimum(((synth.uniform(seed + 500000, n) + 1.0) * 1.5).astype(np.int64), 2)
    return frozen((synth.uniform(seed, n) * SCALES[pick]).astype(np.float32).reshape(shape))


@functools.lru_cache(maxsize=None)
def make_grad_steps(shapes, nsteps, seed=1000):
    """nsteps gradient sets for `shapes` (shared, read-only)."""
    return tuple(tuple(make_grad(seed + 1000 * s + i, sh) for i, sh in enumerate(shapes)) for s in range(nsteps))


def one_group(shapes, **hyper):
    return [dict(idx=list(range(len(shapes))), **hyper)]


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def cat64(xs):
    return np.concatenate([np.asarray(x, np.float64).ravel() for x in xs])


def check_bound(what, hip, t32, ref):
    """max|hip - ref64| <= 2 * max|torch32 - ref64| + 2 * ulp32(max|ref64|), over all tensors."""
    assert [np.shape(x) for x in hip] == [np.shape(x) for x in ref] == [np.shape(x) for x in t32]
    h, t, r = cat64(hip), cat64(t32), cat64(ref)
    e_hip = float(np.max(np.abs(h - r)))
    e_t = float(np.max(np.abs(t - r)))
    bound = 2.0 * e_t + 2.0 * ulp32(np.max(np.abs(r)))
    print(f"{what}: e_hip={e_hip:.3e} e_t={e_t:.3e} bound={bound:.3e}")
    assert e_hip <= bound, (what, e_hip, e_t, bound)


def bits(t):
    """int32 view of a float32 tensor or array (bitwise comparisons; NaN-safe)."""
    if torch.is_tensor(t):
        return t.detach().contiguous().view(torch.int32).cpu().numpy()
    return np.ascontiguousarray(t, np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def group_args(ps, groups):
    return [dict(params=[ps[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"]) for g in groups]


def run_torch32(params, grad_steps, groups, max_norm, state=None):
    """torch.optim.Adam(foreach=False) + clip_grad_norm_ in fp32 on the CPU; returns the optimizer,
    its parameters and dict(params, exp_avg, exp_avg_sq) as numpy."""
    tp = [torch.from_numpy(p.copy()).requires_grad_() for p in params]
    opt = torch.optim.Adam(group_args(tp, groups), foreach=False)
    if state is not None:
        for p, m, v, s in zip(tp, *state):
            opt.state[p] = dict(step=torch.tensor(float(s)), exp_avg=torch.from_numpy(np.array(m, np.float32)),
                                exp_avg_sq=torch.from_numpy(np.array(v, np.float32)))
    torch32_steps(opt, tp, grad_steps, max_norm)
    return opt, tp, torch32_result(opt, tp)


def torch32_steps(opt, tp, grad_steps, max_norm, error_if_nonfinite=False):
    for step in grad_steps:
        for p, g in zip(tp, step):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(tp, max_norm, error_if_nonfinite=error_if_nonfinite)
        opt.step()


def torch32_result(opt, tp):
    st = lambda p, k: opt.state[p][k].numpy().copy() if k in opt.state[p] else np.zeros(p.shape, np.float32)  # noqa: E731
    return dict(params=[p.detach().numpy().copy() for p in tp], exp_avg=[st(p, "exp_avg") for p in tp],
                exp_avg_sq=[st(p, "exp_avg_sq") for p in tp])


def make_hip(dev, params, groups, max_norm, **kw):
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(p, np.float32)).to(dev)) for p in params]
    return ps, optim.FusedAdam(group_args(ps, groups), max_grad_norm=max_norm, **kw)


def set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else torch.from_numpy(g.copy()).to(p.device)


def hip_result(opt, ps):
    st = lambda p, k: opt.state[p][k].cpu().numpy() if k in opt.state[p] else np.zeros(p.shape, np.float32)  # noqa: E731
    return dict(params=[p.detach().cpu().numpy() for p in ps], exp_avg=[st(p, "exp_avg") for p in ps],
                exp_avg_sq=[st(p, "exp_avg_sq") for p in ps])


def check_all(what, hip, t32, ref):
    for k in ("params", "exp_avg", "exp_avg_sq"):
        check_bound(f"{what} {k}", hip[k], t32[k], ref[k])


def steps_of(opt, ps):
    return [float(opt.state[p]["step"]) for p in ps if "step" in opt.state[p]]


# ---- 1. eager step against float64 ---------------------------------------------------------------

ADAM_CASES = {
    "adain_ast": (2e-4, (0.9, 0.999), 1e-5, 2.0),
    "autoencoder_large_lr": (1e-2, (0.9, 0.99), 1e-7, 10.0),
    "lerp2_noclip": (2e-4, (0.3, 0.9), 1e-7, None),   # beta1 <= 0.5: second at::lerp form; null clip state
}


@pytest.mark.parametrize("case", sorted(ADAM_CASES))
def test_adam_vs_float64(case, hip_device):
    """Measured on an MI355X (50 steps, T_edge), parameters, e_hip / e_t: adain_ast 6.9e-8 / 6.9e-8,
    autoencoder_large_lr 1.3e-7 / 1.4e-7, lerp2_noclip 7.1e-8 / 7.1e-8 (the same element carries both
    maxima: the arithmetic is torch's). The moments' e_hip is at or below their e_t, with clipping
    more than ten times below (the device contracts to FMAs)."""
    lr, betas, eps, max_norm = ADAM_CASES[case]
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 50)
    groups = one_group(T_EDGE, lr=lr, betas=betas, eps=eps)
    ref = OR.run(params, grad_steps, groups, max_norm)
    _, _, t32 = run_torch32(params, grad_steps, groups, max_norm)
    ps, opt = make_hip(hip_device, params, groups, max_norm, error_if_nonfinite=True)
    for s, grads in enumerate(grad_steps):
        set_grads(ps, grads)
        opt.step()
        if max_norm is None:
            assert opt.last_grad_norm is None
        else:
            np.testing.assert_allclose(opt.last_grad_norm.item(), ref["norms"][s], rtol=1e-5)
    check_all(f"adam_vs_float64[{case}]", hip_result(opt, ps), t32, ref)   # every tensor downloaded whole
    assert steps_of(opt, ps) == [50.0] * len(ps)


def test_beta1_zero_exp_avg_is_the_gradient(hip_device):
    """at::lerp has two forms so that weight 1 returns its end point exactly: with beta1 = 0 the
    weight is 1 >= 0.5, and g - (g - m) * (1 - 1) is g bit for bit, while m + 1 * (g - m) is not
    (m and g differ by up to six orders of magnitude here). torch's exp_avg is then the clipped
    gradient itself; so must the kernel's be. Rounding-level bounds cannot tell the two forms apart;
    this can."""
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 3)
    groups = one_group(T_EDGE, lr=2e-4, betas=(0.0, 0.9), eps=1e-7)
    ref = OR.run(params, grad_steps, groups, 2.0)
    topt, tp, t32 = run_torch32(params, grad_steps, groups, 2.0)
    for p in tp:
        assert same_bits(topt.state[p]["exp_avg"], p.grad)
    ps, opt = make_hip(hip_device, params, groups, 2.0)
    for grads in grad_steps:
        set_grads(ps, grads)
        opt.step()
        for p in ps:
            assert same_bits(opt.state[p]["exp_avg"], p.grad)
    check_all("beta1_zero", hip_result(opt, ps), t32, ref)


# ---- 2. chunk edges --------------------------------------------------------------------------------

GUARD = 64
SENTINEL = 12345.678


class Guarded:
    """Parameters, gradients and moments of T_edge, each the contiguous interior of a larger device
    buffer with GUARD sentinel floats on either side (an out-of-range write of a few elements lands
    in a guard, inside the allocation)."""

    def __init__(self, dev, params, grads, groups, max_norm):
        self.bufs = []
        ps = [torch.nn.Parameter(self.alloc(dev, p)) for p in params]
        self.opt = optim.FusedAdam(group_args(ps, groups), max_grad_norm=max_norm)
        for p, g in zip(ps, grads):
            p.grad = None if g is None else self.alloc(dev, g)
            self.opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=self.alloc(dev, np.zeros(p.shape, np.float32)),
                                     exp_avg_sq=self.alloc(dev, np.zeros(p.shape, np.float32)))
        self.ps = ps

    def alloc(self, dev, arr):
        n = arr.size
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.float32)
        inner = buf[GUARD:GUARD + n]
        inner.copy_(torch.from_numpy(np.array(arr, np.float32).ravel()))
        self.bufs.append(buf)
        inner = inner.view(arr.shape)
        assert inner.is_contiguous() and inner.data_ptr() == buf.data_ptr() + 4 * GUARD
        return inner

    def assert_guards_intact(self):
        want = bits(np.full(GUARD, SENTINEL, np.float32))
        for k, buf in enumerate(self.bufs):
            assert np.array_equal(bits(buf[:GUARD]), want), f"buffer {k}: write before the tensor"
            assert np.array_equal(bits(buf[-GUARD:]), want), f"buffer {k}: write past the tensor"


def test_chunk_edges_touch_exactly_their_tensor(hip_device):
    params, grads = make_params(T_EDGE), make_grad_steps(T_EDGE, 1)[0]
    # eps 1e-8 and a clip coefficient of 1/2: the first Adam step moves an element by
    # lr * g / (|g| + eps), ~lr = 1e-2 unless |g| is within a few eps of zero
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    groups = one_group(T_EDGE, **hyper)
    max_norm = 0.5 * OR.total_norm(grads)
    ref = OR.run(params, [grads], groups, max_norm)
    for p0, p1 in zip(params, ref["params"]):   # the inputs make every element move by several fp32 ulps
        assert np.all(np.abs(p1 - p0) > 4 * np.spacing(np.abs(p0)))
    _, _, t32 = run_torch32(params, [grads], groups, max_norm)
    G = Guarded(hip_device, params, grads, groups, max_norm)
    G.opt.step()
    torch.cuda.synchronize()
    G.assert_guards_intact()
    got = hip_result(G.opt, G.ps)
    for i, (p0, g0) in enumerate(zip(params, grads)):
        assert np.all(got["params"][i] != p0), f"tensor {i}: parameter elements left unchanged"
        assert np.all(got["exp_avg"][i] != 0), f"tensor {i}: exp_avg elements left unchanged"
        assert np.all(got["exp_avg_sq"][i] > 0), f"tensor {i}: exp_avg_sq elements left unchanged"
        assert np.all(G.ps[i].grad.cpu().numpy() != g0), f"tensor {i}: gradient elements left unscaled"
        for k in ("params", "exp_avg", "exp_avg_sq"):   # first and last element on their own
            for j in (0, -1):
                assert got[k][i].ravel()[j] != (p0.ravel()[j] if k == "params" else 0.0), (i, k, j)
    check_all("chunk_edges", got, t32, ref)
    np.testing.assert_allclose(G.opt.last_grad_norm.item(), ref["norms"][0], rtol=1e-5)

    # the 65537-element tensor without a gradient: it and its moments stay as they are, the norm and
    # the other tensors are those of a run without it
    skip = T_EDGE.index((65537,))
    grads2 = [None if i == skip else g for i, g in enumerate(grads)]
    ref2 = OR.run(params, [grads2], groups, max_norm)
    _, _, t32_2 = run_torch32(params, [grads2], groups, max_norm)
    G2 = Guarded(hip_device, params, grads2, groups, max_norm)
    G2.opt.step()
    torch.cuda.synchronize()
    G2.assert_guards_intact()
    got2 = hip_result(G2.opt, G2.ps)
    assert same_bits(got2["params"][skip], params[skip])
    assert same_bits(got2["exp_avg"][skip], np.zeros(65537, np.float32))
    assert same_bits(got2["exp_avg_sq"][skip], np.zeros(65537, np.float32))
    assert float(G2.opt.state[G2.ps[skip]]["step"]) == 0.0
    np.testing.assert_allclose(G2.opt.last_grad_norm.item(), ref2["norms"][0], rtol=1e-5)
    assert ref2["norms"][0] < ref["norms"][0]
    for i, p0 in enumerate(params):
        if i != skip:
            assert np.all(got2["params"][i] != p0), f"tensor {i}: parameter elements left unchanged"
    check_all("chunk_edges_without_65537", got2, t32_2, ref2)


# ---- 3. many tensors -------------------------------------------------------------------------------

def test_many_small_tensors(hip_device):
    """257 tensors (binary search over many entries), 258 chunks (the finish kernel's threads 0 and 1
    fold two partial sums each)."""
    shapes = tuple((1 + i % 9,) for i in range(256))
    shapes = shapes[:128] + ((65537,),) + shapes[128:]
    assert len(shapes) == 257 and OR.nchunks([numel(s) for s in shapes]) == 258
    params, grad_steps = make_params(shapes, 7000), make_grad_steps(shapes, 3, 9000)
    groups = one_group(shapes, **ADAIN)
    ref = OR.run(params, grad_steps, groups, 2.0)
    _, _, t32 = run_torch32(params, grad_steps, groups, 2.0)
    ps, opt = make_hip(hip_device, params, groups, 2.0)
    for s, grads in enumerate(grad_steps):
        set_grads(ps, grads)
        opt.step()
        np.testing.assert_allclose(opt.last_grad_norm.item(), ref["norms"][s], rtol=1e-5)
    got = hip_result(opt, ps)
    check_all("many_small_tensors", got, t32, ref)
    # the small tensors on their own: the 65537-element one would otherwise dominate the statistics
    small = [i for i, s in enumerate(shapes) if s != (65537,)]
    for k in ("params", "exp_avg", "exp_avg_sq"):
        check_bound(f"many_small_tensors small {k}", [got[k][i] for i in small], [t32[k][i] for i in small],
                    [ref[k][i] for i in small])


# ---- 4. clip coefficient 1 -------------------------------------------------------------------------

def test_clip_inactive_leaves_gradients_bitwise(hip_device):
    params, grads = make_params(T_EDGE), make_grad_steps(T_EDGE, 1)[0]
    groups = one_group(T_EDGE, **ADAIN)
    norm = OR.total_norm(grads)
    ps, opt = make_hip(hip_device, params, groups, 10.0 * norm)
    set_grads(ps, grads)
    opt.step()
    np.testing.assert_allclose(opt.last_grad_norm.item(), norm, rtol=1e-5)
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad.cpu(), torch.from_numpy(g.copy()))
        assert same_bits(p.grad, g)

    max_norm = float(np.float32(norm / 4.0))   # what the C ABI's float argument holds
    ps, opt = make_hip(hip_device, params, groups, max_norm)
    set_grads(ps, grads)
    opt.step()
    norm_dev = opt.last_grad_norm.item()
    np.testing.assert_allclose(norm_dev, norm, rtol=1e-5)
    coef64 = OR.clip_coef(norm_dev, max_norm)
    assert 0.2 < coef64 < 0.3
    coef32 = np.float32(max_norm) / (np.float32(norm_dev) + np.float32(1e-6))   # the kernel's own expression
    for p, g in zip(ps, grads):
        got = p.grad.cpu().numpy()
        want32 = g * coef32
        assert np.all(np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)))
        np.testing.assert_allclose(got, g.astype(np.float64) * coef64, rtol=2e-7, atol=0)


# ---- 5. parameter groups ---------------------------------------------------------------------------

def test_param_groups_one_norm(hip_device):
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 5)
    none = T_EDGE.index((7, 5))
    grad_steps = [[None if i == none else g for i, g in enumerate(step)] for step in grad_steps]
    groups = [dict(idx=[0, 1, 2, 3, 4], lr=2e-4, betas=(0.9, 0.999), eps=1e-5),
              dict(idx=[5, 6, 7, 8], lr=1e-2, betas=(0.3, 0.9), eps=1e-7)]
    ref = OR.run(params, grad_steps, groups, 2.0)
    _, _, t32 = run_torch32(params, grad_steps, groups, 2.0)
    ps, opt = make_hip(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    for s, grads in enumerate(grad_steps):
        set_grads(ps, grads)
        opt.step()
        np.testing.assert_allclose(opt.last_grad_norm.item(), ref["norms"][s], rtol=1e-5)
        for k, g in enumerate(groups):   # neither group's own norm would pass for the total
            own = OR.total_norm([grads[i] for i in g["idx"]])
            assert abs(own - ref["norms"][s]) > 1e-3 * ref["norms"][s], k
    got = hip_result(opt, ps)
    check_all("param_groups", got, t32, ref)
    for g in groups:
        idx = g["idx"]
        check_bound(f"param_groups lr={g['lr']} params", [got["params"][i] for i in idx],
                    [t32["params"][i] for i in idx], [ref["params"][i] for i in idx])
    assert same_bits(got["params"][none], params[none]) and len(opt.state[ps[none]]) == 0
    assert steps_of(opt, ps) == [5.0] * 8


def test_intermittent_gradient_keeps_its_own_step_count(hip_device):
    """torch keeps one step count per parameter: one that had no gradient in some steps is stepped
    with its own bias corrections in the others, not with its group's."""
    shapes = ((5,), (65537,), (7, 5))
    params, grad_steps = make_params(shapes, 80), make_grad_steps(shapes, 4, 4000)
    grad_steps = [[None if i == 1 and s in (0, 2) else g for i, g in enumerate(step)]
                  for s, step in enumerate(grad_steps)]
    groups = one_group(shapes, **ADAIN)
    ref = OR.run(params, grad_steps, groups, 2.0)
    assert ref["step"] == [4, 2, 4]
    topt, tp, t32 = run_torch32(params, grad_steps, groups, 2.0)
    assert [float(topt.state[p]["step"]) for p in tp] == [4.0, 2.0, 4.0]
    ps, opt = make_hip(hip_device, params, groups, 2.0)
    for s, grads in enumerate(grad_steps):
        set_grads(ps, grads)
        opt.step()
        np.testing.assert_allclose(opt.last_grad_norm.item(), ref["norms"][s], rtol=1e-5)
    assert steps_of(opt, ps) == [4.0, 2.0, 4.0]
    check_all("intermittent_gradient", hip_result(opt, ps), t32, ref)
    # the capturable form holds one device step count per group and cannot express this
    with pytest.raises(RuntimeError):
        opt.prepare_static()


# ---- 6.-8. graph-capturable step ---------------------------------------------------------------------

def make_static(dev, params, groups, max_norm, state_dict=None, **kw):
    """A FusedAdam driven as train.StepGraph drives it, without a graph: prepare_static(), persistent
    gradient tensors, fill_static()."""
    ps, opt = make_hip(dev, params, groups, max_norm, **kw)
    if state_dict is not None:
        opt.load_state_dict(copy.deepcopy(state_dict))
    opt.prepare_static()
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt.fill_static()
    return ps, opt


def static_step(ps, opt, grads, after=True):
    """One replayed step: new gradients into the same storage, step_static(), host bookkeeping."""
    ptrs = [p.grad.data_ptr() for p in ps]
    for p, g in zip(ps, grads):
        p.grad.copy_(torch.from_numpy(g.copy()))
    opt.step_static()
    if after:
        opt.after_static_step()
    assert ptrs == [p.grad.data_ptr() for p in ps]


def sched_of(opt):
    return [s.cpu().numpy() for _, _, _, _, s in opt._static]


def assert_static_close(got, want, nsteps, lr):
    for k in ("params", "exp_avg", "exp_avg_sq"):
        for a, b in zip(got[k], want[k]):
            np.testing.assert_allclose(a, b, rtol=2e-7, atol=nsteps * lr * 3e-7, err_msg=k)


TWO_GROUPS = [dict(idx=[0, 1, 2, 3, 4], lr=2e-4, betas=(0.9, 0.999), eps=1e-5),
              dict(idx=[5, 6, 7, 8], lr=1e-3, betas=(0.3, 0.9), eps=1e-7)]


@pytest.mark.parametrize("ngroups", [1, 2])
def test_step_static_matches_step(ngroups, hip_device):
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 6)
    groups = one_group(T_EDGE, **ADAIN) if ngroups == 1 else TWO_GROUPS
    ref = OR.run(params, grad_steps[:3], groups, 2.0)   # the first three steps, for the norms
    ps_e, opt_e = make_hip(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    ps_s, opt_s = make_static(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    for s, grads in enumerate(grad_steps):
        if s == 3:
            before = opt_s.static_hyper()
            for opt in (opt_e, opt_s):
                for g in opt.param_groups:
                    g["lr"] = g["lr"] * 0.5
            assert opt_s.static_hyper() != before
            assert opt_s.static_hyper() == opt_e.static_hyper()
        set_grads(ps_e, grads)
        opt_e.step()
        static_step(ps_s, opt_s, grads)
        np.testing.assert_allclose(opt_s.last_grad_norm.item(), opt_e.last_grad_norm.item(), rtol=1e-5)
        if s < 3:
            np.testing.assert_allclose(opt_s.last_grad_norm.item(), ref["norms"][s], rtol=1e-5)
        for a, b in zip(ps_s, ps_e):   # both clipped their gradients in place
            np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=2e-7, atol=0)
    lr = max(g["lr"] for g in groups)
    assert_static_close(hip_result(opt_s, ps_s), hip_result(opt_e, ps_e), 6, lr)
    for sched in sched_of(opt_s):
        assert sched[0] == 6.0 and sched[1] == 0.0
    assert steps_of(opt_s, ps_s) == [6.0] * len(ps_s)
    assert steps_of(opt_e, ps_e) == [6.0] * len(ps_e)
    # the halved lr reached the device schedule: sched[2] = lr / (1 - beta1^6)
    for g, sched in zip(opt_s.param_groups, sched_of(opt_s)):
        np.testing.assert_allclose(sched[2], g["lr"] / (1.0 - g["betas"][0] ** 6), rtol=2e-7)
        np.testing.assert_allclose(sched[3], np.sqrt(1.0 - g["betas"][1] ** 6), rtol=2e-7)


def with_bad_element(grads, value):
    """`grads` with one element of the 65537-element tensor (in its second chunk) set to `value`."""
    k = T_EDGE.index((65537,))
    bad = [g for g in grads]
    b = grads[k].copy()
    b[65536] = value
    bad[k] = b
    return bad


def test_step_static_skips_nonfinite_and_resumes(hip_device):
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 5)
    groups = one_group(T_EDGE, **ADAIN)
    ps, opt = make_static(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    for grads in grad_steps[:2]:
        static_step(ps, opt, grads)
    assert sched_of(opt)[0][0] == 2.0
    before = hip_result(opt, ps)
    for value, grads in ((float("nan"), grad_steps[2]), (float("inf"), grad_steps[3])):
        bad = with_bad_element(grads, value)
        static_step(ps, opt, bad, after=False)   # StepGraph.run raises before after_static_step()
        norm = opt.last_grad_norm.item()
        assert norm != norm if value != value else norm == float("inf")
        sched = sched_of(opt)[0]
        assert sched[0] == 2.0 and sched[1] != 0.0
        after = hip_result(opt, ps)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            for a, b in zip(after[k], before[k]):
                assert same_bits(a, b), k
        for p, g in zip(ps, bad):   # the skip path must not scale the gradients either
            assert same_bits(p.grad, g)
        assert steps_of(opt, ps) == [2.0] * len(ps)
    static_step(ps, opt, grad_steps[4])
    sched = sched_of(opt)[0]
    assert sched[0] == 3.0 and sched[1] == 0.0
    assert steps_of(opt, ps) == [3.0] * len(ps)
    good = [grad_steps[0], grad_steps[1], grad_steps[4]]
    ps_e, opt_e = make_hip(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    for grads in good:
        set_grads(ps_e, grads)
        opt_e.step()
    assert_static_close(hip_result(opt, ps), hip_result(opt_e, ps_e), 3, ADAIN["lr"])
    ref = OR.run(params, good, groups, 2.0)
    _, _, t32 = run_torch32(params, good, groups, 2.0)
    check_all("static_resumes_after_skip", hip_result(opt, ps), t32, ref)


@pytest.mark.parametrize("path", ["static", "eager"])
def test_nonfinite_not_checked_steps_like_torch(path, hip_device):
    """error_if_nonfinite=False: a NaN gradient does not skip the step; the NaN norm gives a NaN
    coefficient, and gradients, moments and parameters turn NaN exactly where fp32 torch's do."""
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 2)
    groups = one_group(T_EDGE, **ADAIN)
    steps = [grad_steps[0], with_bad_element(grad_steps[1], float("nan"))]
    topt, tp, _ = run_torch32(params, steps, groups, 2.0)
    t32 = torch32_result(topt, tp)
    if path == "static":
        ps, opt = make_static(hip_device, params, groups, 2.0, error_if_nonfinite=False)
        for grads in steps:
            static_step(ps, opt, grads)
        sched = sched_of(opt)[0]
        assert sched[0] == 2.0 and sched[1] == 0.0
    else:
        ps, opt = make_hip(hip_device, params, groups, 2.0, error_if_nonfinite=False)
        for grads in steps:
            set_grads(ps, grads)
            opt.step()
    norm = opt.last_grad_norm.item()
    assert norm != norm
    got = hip_result(opt, ps)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        for a, b in zip(got[k], t32[k]):
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
    for p, q in zip(ps, tp):
        assert np.array_equal(np.isnan(p.grad.cpu().numpy()), np.isnan(q.grad.numpy()))
    assert all(np.isnan(a).all() for a in got["params"])   # torch: every gradient times the NaN coefficient
    assert steps_of(opt, ps) == [2.0] * len(ps)


def loaded_state(shapes, step):
    """Moments as a checkpoint at `step` would hold them (seeded), and the torch optimizer holding them."""
    ms = [frozen((synth.uniform(300 + i, numel(s)) * 1e-2).astype(np.float32).reshape(s)) for i, s in enumerate(shapes)]
    vs = [frozen(((synth.uniform(400 + i, numel(s)) * 1e-2) ** 2 + 1e-9).astype(np.float32).reshape(s))
          for i, s in enumerate(shapes)]
    return ms, vs, [step] * len(shapes)


def test_static_resumes_from_loaded_step(hip_device):
    params, grads = make_params(T_EDGE), make_grad_steps(T_EDGE, 1)[0]
    groups = one_group(T_EDGE, **ADAIN)
    state = loaded_state(T_EDGE, 1000)
    topt, tp, _ = run_torch32(params, [], groups, 2.0, state=state)
    sd = copy.deepcopy(topt.state_dict())
    ps_s, opt_s = make_static(hip_device, params, groups, 2.0, state_dict=sd, error_if_nonfinite=True)
    assert sched_of(opt_s)[0][0] == 1000.0
    ps_e, opt_e = make_hip(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    opt_e.load_state_dict(copy.deepcopy(sd))
    static_step(ps_s, opt_s, grads)
    set_grads(ps_e, grads)
    opt_e.step()
    sched = sched_of(opt_s)[0]
    assert sched[0] == 1001.0 and sched[1] == 0.0
    np.testing.assert_allclose(sched[2], ADAIN["lr"] / (1.0 - 0.9 ** 1001), rtol=2e-7)
    np.testing.assert_allclose(sched[3], np.sqrt(1.0 - 0.999 ** 1001), rtol=2e-7)
    assert steps_of(opt_s, ps_s) == steps_of(opt_e, ps_e) == [1001.0] * len(T_EDGE)
    assert_static_close(hip_result(opt_s, ps_s), hip_result(opt_e, ps_e), 1, ADAIN["lr"])
    ref = OR.run(params, [grads], groups, 2.0, state=state)
    assert ref["step"] == [1001] * len(T_EDGE)
    torch32_steps(topt, tp, [grads], 2.0)
    t32 = torch32_result(topt, tp)
    check_all("static_from_step_1000 static", hip_result(opt_s, ps_s), t32, ref)
    check_all("static_from_step_1000 eager", hip_result(opt_e, ps_e), t32, ref)


# ---- 9. checkpoints --------------------------------------------------------------------------------

def test_state_dict_interchanges_with_torch_adam(hip_device):
    shapes = ((1,), (65537,), (7, 5))
    params, grad_steps = make_params(shapes, 60), make_grad_steps(shapes, 6, 3000)
    groups = one_group(shapes, **ADAIN)
    ref = OR.run(params, grad_steps, groups, 2.0)

    # torch -> FusedAdam: three torch steps, its checkpoint into a FusedAdam built with other
    # hyper-parameters (the checkpoint's replace them), three more steps on each
    topt, tp, _ = run_torch32(params, grad_steps[:3], groups, 2.0)
    mid = [p.detach().numpy().copy() for p in tp]
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(hip_device)) for p in mid]
    opt = optim.FusedAdam(ps, lr=1e-3, max_grad_norm=2.0)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    assert opt.param_groups[0]["lr"] == ADAIN["lr"] and opt.param_groups[0]["eps"] == ADAIN["eps"]
    assert steps_of(opt, ps) == [3.0] * 3
    assert all(opt.state[p]["exp_avg"].device == p.device for p in ps)
    for grads in grad_steps[3:]:
        set_grads(ps, grads)
        opt.step()
    torch32_steps(topt, tp, grad_steps[3:], 2.0)
    t32 = torch32_result(topt, tp)   # six steps of torch's fp32 Adam
    check_all("torch_to_fused", hip_result(opt, ps), t32, ref)
    assert steps_of(opt, ps) == [6.0] * 3

    # FusedAdam -> torch: three FusedAdam steps, its checkpoint into torch.optim.Adam over CPU copies,
    # three more steps on each
    ps, opt = make_hip(hip_device, params, groups, 2.0)
    for grads in grad_steps[:3]:
        set_grads(ps, grads)
        opt.step()
    tp2 = [p.detach().cpu().clone().requires_grad_() for p in ps]
    topt2 = torch.optim.Adam(tp2, lr=1e-3, foreach=False)
    topt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert topt2.param_groups[0]["lr"] == ADAIN["lr"]
    for grads in grad_steps[3:]:
        set_grads(ps, grads)
        opt.step()
    torch32_steps(topt2, tp2, grad_steps[3:], 2.0)
    check_all("fused_to_torch", torch32_result(topt2, tp2), t32, ref)
    check_all("fused_six_steps", hip_result(opt, ps), t32, ref)
    assert [float(topt2.state[p]["step"]) for p in tp2] == [6.0] * 3

    want = set(torch.optim.Adam([torch.zeros(1, requires_grad=True)]).state_dict()["param_groups"][0])
    assert set(optim.FusedAdam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]) == want
    assert set(opt.state_dict()["param_groups"][0]) == want
    sd = opt.state_dict()["state"]
    assert sorted(sd) == [0, 1, 2] and all(sorted(v) == ["exp_avg", "exp_avg_sq", "step"] for v in sd.values())


# ---- 10. the standalone clip_grad_norm_ ------------------------------------------------------------

CLIP_SHAPES = ((1,), (65536,), (65537,), (35,))


def clip_pair(dev, grads):
    """Parameters holding `grads` on the device and on the CPU (None: no gradient)."""
    hip, cpu = [], []
    for g in grads:
        shape = (3,) if g is None else g.shape
        a, b = torch.nn.Parameter(torch.zeros(shape, device=dev)), torch.nn.Parameter(torch.zeros(shape))
        if g is not None:
            a.grad, b.grad = torch.from_numpy(g.copy()).to(dev), torch.from_numpy(g.copy())
        hip.append(a)
        cpu.append(b)
    return hip, cpu


def test_clip_grad_norm_function(hip_device):
    grads = list(make_grad_steps(CLIP_SHAPES, 1, 5000)[0])
    norm = OR.total_norm(grads)
    # clipping; a parameter without a gradient is ignored
    with_none = grads[:2] + [None] + grads[2:]
    hip, cpu = clip_pair(hip_device, with_none)
    max_norm = float(np.float32(norm / 3.0))
    got = optim.clip_grad_norm_(hip, max_norm)
    want = torch.nn.utils.clip_grad_norm_(cpu, max_norm)
    np.testing.assert_allclose(got.item(), norm, rtol=1e-5)
    np.testing.assert_allclose(got.item(), want.item(), rtol=1e-5)
    coef = OR.clip_coef(got.item(), max_norm)
    assert 0.3 < coef < 0.4
    for a, g in zip(hip, with_none):
        if g is None:
            assert a.grad is None
        else:
            np.testing.assert_allclose(a.grad.cpu().numpy(), g.astype(np.float64) * coef, rtol=2e-7, atol=0)
    # not clipping: bit-unchanged
    hip, _ = clip_pair(hip_device, grads)
    got = optim.clip_grad_norm_(hip, 10.0 * norm)
    np.testing.assert_allclose(got.item(), norm, rtol=1e-5)
    for a, g in zip(hip, grads):
        assert same_bits(a.grad, g)
    # a single tensor
    hip, _ = clip_pair(hip_device, [grads[2]])
    one = OR.total_norm([grads[2]])
    got = optim.clip_grad_norm_(hip[0], float(np.float32(one / 2.0)))
    np.testing.assert_allclose(got.item(), one, rtol=1e-5)
    np.testing.assert_allclose(hip[0].grad.cpu().numpy(),
                               grads[2].astype(np.float64) * OR.clip_coef(got.item(), float(np.float32(one / 2.0))),
                               rtol=2e-7, atol=0)
    # no gradients at all
    hip, _ = clip_pair(hip_device, [None, None])
    assert float(optim.clip_grad_norm_(hip, 1.0)) == 0.0
    assert float(optim.clip_grad_norm_([], 1.0)) == 0.0
    # only the L2 norm
    hip, _ = clip_pair(hip_device, grads)
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(hip, 1.0, norm_type=1)
    for a, g in zip(hip, grads):
        assert same_bits(a.grad, g)
    # non-finite gradients
    k = CLIP_SHAPES.index((65537,))
    for value in (float("nan"), float("inf")):
        bad = list(grads)
        b = grads[k].copy()
        b[65536] = value
        bad[k] = b
        hip, cpu = clip_pair(hip_device, bad)
        with pytest.raises(RuntimeError):
            optim.clip_grad_norm_(hip, 1.0, error_if_nonfinite=True)
        for a, g in zip(hip, bad):   # raised before any gradient changed
            assert same_bits(a.grad, g)
        got = optim.clip_grad_norm_(hip, 1.0, error_if_nonfinite=False)
        want = torch.nn.utils.clip_grad_norm_(cpu, 1.0, error_if_nonfinite=False)
        if value != value:
            assert got.item() != got.item() and want.item() != want.item()
            assert all(np.isnan(a.grad.cpu().numpy()).all() for a in hip)   # NaN coefficient
        else:
            assert got.item() == float("inf") and want.item() == float("inf")
            for i, a in enumerate(hip):   # coefficient 0: inf * 0 = NaN, everything else +-0
                out = a.grad.cpu().numpy()
                isnan = np.isnan(out)
                assert isnan.sum() == (1 if i == k else 0)
                assert np.all(out[~isnan] == 0.0)
            assert np.isnan(hip[k].grad.cpu().numpy()[65536])
        for a, b in zip(hip, cpu):
            assert np.array_equal(np.isnan(a.grad.cpu().numpy()), np.isnan(b.grad.numpy()))


# ---- 11. eager non-finite check ----------------------------------------------------------------------

@pytest.mark.parametrize("ngroups", [1, 2])
def test_eager_nonfinite_raises_before_any_change(ngroups, hip_device):
    params, grad_steps = make_params(T_EDGE), make_grad_steps(T_EDGE, 3)
    groups = one_group(T_EDGE, **ADAIN) if ngroups == 1 else TWO_GROUPS
    ps, opt = make_hip(hip_device, params, groups, 2.0, error_if_nonfinite=True)
    for grads in grad_steps[:2]:
        set_grads(ps, grads)
        opt.step()
    before = hip_result(opt, ps)
    for value in (float("nan"), float("inf"), float("-inf")):
        bad = with_bad_element(grad_steps[2], value)
        set_grads(ps, bad)
        with pytest.raises(RuntimeError):
            opt.step()
        after = hip_result(opt, ps)
        for k in ("params", "exp_avg", "exp_avg_sq"):
            for a, b in zip(after[k], before[k]):
                assert same_bits(a, b), k
        for p, g in zip(ps, bad):
            assert same_bits(p.grad, g)
        assert steps_of(opt, ps) == [2.0] * len(ps)
    set_grads(ps, grad_steps[2])   # and the next good step is the third
    opt.step()
    assert steps_of(opt, ps) == [3.0] * len(ps)
    ref = OR.run(params, grad_steps, groups, 2.0)
    _, _, t32 = run_torch32(params, grad_steps, groups, 2.0)
    check_all("eager_after_nonfinite", hip_result(opt, ps), t32, ref)
