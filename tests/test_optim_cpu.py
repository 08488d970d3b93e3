"""CPU checks around csrc/optim.hip: the float64 reference of tests/optim_ref.py against torch's own
float64 Adam + clip_grad_norm_ (so the GPU tests compare with torch's arithmetic and not with a
restatement of the kernel), the host-only table builder, and the argument checks of the four
launching entry points (each must return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as OR
from arbitrarystyletransfer_amd import _lib, synth

SHAPES = [(5,), (130,), (7, 5), (1,), (64,)]


def _grads(seed, shapes, nsteps):
    scales = np.array([1e-4, 1.0, 1e2])
    out = []
    for s in range(nsteps):
        step = []
        for i, sh in enumerate(shapes):
            n = int(np.prod(sh))
            u = synth.uniform(seed + 100 * s + i, n)
            pick = np.minimum(((synth.uniform(seed + 100 * s + i + 50, n) + 1.0) * 1.5).astype(np.int64), 2)
            step.append((u * scales[pick]).reshape(sh))
        out.append(step)
    return out


@pytest.mark.parametrize("betas0,betas1", [((0.9, 0.999), (0.3, 0.9)), ((0.3, 0.9), (0.9, 0.999))])
def test_reference_matches_torch_float64(betas0, betas1):
    params = [synth.uniform(10 + i, int(np.prod(sh))).reshape(sh) * 0.1 for i, sh in enumerate(SHAPES)]
    grad_steps = _grads(1000, SHAPES, 20)
    for step in grad_steps:
        step[3] = None   # a parameter that never has a gradient
    groups = [dict(idx=[0, 1], lr=2e-4, betas=betas0, eps=1e-5), dict(idx=[2, 3, 4], lr=1e-2, betas=betas1, eps=1e-7)]
    max_norm = 2.0
    ref = OR.run(params, grad_steps, groups, max_norm)

    tp = [torch.from_numpy(p.copy()).requires_grad_() for p in params]
    opt = torch.optim.Adam([dict(params=[tp[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"])
                            for g in groups], foreach=False)
    for s, step in enumerate(grad_steps):
        for p, g in zip(tp, step):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_(tp, max_norm, error_if_nonfinite=True)
        np.testing.assert_allclose(ref["norms"][s], norm.item(), rtol=1e-12)
        opt.step()
    for i, p in enumerate(tp):
        np.testing.assert_allclose(ref["params"][i], p.detach().numpy(), rtol=1e-12, atol=0)
        if i != 3:
            np.testing.assert_allclose(ref["exp_avg"][i], opt.state[p]["exp_avg"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(ref["exp_avg_sq"][i], opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
            assert ref["step"][i] == int(opt.state[p]["step"].item()) == 20
    assert ref["step"][3] == 0 and len(opt.state[tp[3]]) == 0
    np.testing.assert_array_equal(ref["params"][3], params[3])


def test_reference_clip_coef_nonfinite():
    """torch.clamp(max_norm / (norm + 1e-6), max=1.0) on the special values."""
    for norm in (0.0, 0.5, 2.0, 7.0, float("inf"), float("nan")):
        want = torch.clamp(torch.tensor(2.0, dtype=torch.float64) / (torch.tensor(norm, dtype=torch.float64) + 1e-6),
                           max=1.0).item()
        got = OR.clip_coef(norm, 2.0)
        assert (got != got and want != want) or got == want, (norm, got, want)
    assert OR.total_norm([None, None]) == 0.0
    assert OR.total_norm([np.array([3.0]), None, np.array([[4.0]])]) == 5.0
    assert OR.total_norm([np.array([1.0, float("inf")])]) == float("inf")
    n = OR.total_norm([np.array([1.0, float("nan")])])
    assert n != n


class _Entry(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_longlong), ("chunk0", ctypes.c_longlong)]


def _build(numels, null_param=None, null_grad=None, ntensors=None):
    L = _lib.lib()
    n = len(numels)
    table = (_Entry * max(n, 1))()
    fake = lambda base, null: (ctypes.c_void_p * max(n, 1))(  # noqa: E731
        *[0 if i == null else base + 0x1000 * (i + 1) for i in range(n)])
    p, g = fake(0x10000000, null_param), fake(0x20000000, null_grad)
    m, v = fake(0x30000000, None), fake(0x40000000, None)
    ret = L.ast_optim_build_table(ctypes.addressof(table), n if ntensors is None else ntensors, p, g, m, v,
                                  (ctypes.c_longlong * max(n, 1))(*numels))
    return ret, table, (p, g, m, v)


def test_build_table_layout():
    L = _lib.lib()
    numels = [1, 65535, 65536, 65537, 131072, 131073, 7, 1]
    assert L.ast_optim_table_bytes(len(numels)) == len(numels) * ctypes.sizeof(_Entry)
    assert ctypes.sizeof(_Entry) == 4 * ctypes.sizeof(ctypes.c_void_p) + 2 * ctypes.sizeof(ctypes.c_longlong)
    total, table, ptrs = _build(numels)
    running = 0
    for i, n in enumerate(numels):
        e = table[i]
        assert e.n == n
        assert e.chunk0 == running, (i, e.chunk0, running)
        assert (e.p, e.g, e.m, e.v) == tuple(a[i] for a in ptrs)
        running += (n + 65535) // 65536
    assert running == 1 + 1 + 1 + 2 + 2 + 3 + 1 + 1
    assert total == running
    assert total == sum(-(-n // 65536) for n in numels)   # FusedAdam.prepare_static's own formula
    assert total == OR.nchunks(numels)


def test_build_table_without_moments():
    """clip_grad_norm_ and the all-groups norm table pass no moment arrays: the entries hold null."""
    L = _lib.lib()
    numels = [3, 65537]
    table = (_Entry * 2)()
    p = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    assert L.ast_optim_build_table(ctypes.addressof(table), 2, p, p, None, None, (ctypes.c_longlong * 2)(*numels)) == 3
    assert [(e.m, e.v, e.n, e.chunk0) for e in table] == [(None, None, 3, 0), (None, None, 65537, 1)]


def test_build_table_rejects_bad_arguments():
    numels = [4, 65537, 9]
    assert _build(numels)[0] == 4
    assert _build(numels, null_param=1)[0] < 0
    assert _build(numels, null_grad=2)[0] < 0
    assert _build([4, 0, 9])[0] < 0
    assert _build([4, -1, 9])[0] < 0
    assert _build(numels, ntensors=0)[0] < 0
    assert _build(numels, ntensors=-1)[0] < 0
    L = _lib.lib()
    p = (ctypes.c_void_p * 1)(0x1000)
    assert L.ast_optim_build_table(None, 1, p, p, p, p, (ctypes.c_longlong * 1)(1)) < 0


TOO_MANY = 2 ** 31   # one more chunk than a launch grid holds

# (entry point, arguments): every pointer that must be non-null is the fake address 1, so a case that
# got past the checks would reach a launch (and return a hipError_t >= 0 on a host without a device)
ARG_ERRORS = {
    "norm_null_table": ("ast_grad_norm_f32", (None, 1, 1, 1, 2.0, 1, None)),
    "norm_null_partial": ("ast_grad_norm_f32", (1, 1, 1, None, 2.0, 1, None)),
    "norm_null_state": ("ast_grad_norm_f32", (1, 1, 1, 1, 2.0, None, None)),
    "norm_no_tensors": ("ast_grad_norm_f32", (1, 0, 1, 1, 2.0, 1, None)),
    "norm_negative_tensors": ("ast_grad_norm_f32", (1, -1, 1, 1, 2.0, 1, None)),
    "norm_no_chunks": ("ast_grad_norm_f32", (1, 1, 0, 1, 2.0, 1, None)),
    "norm_negative_chunks": ("ast_grad_norm_f32", (1, 1, -1, 1, 2.0, 1, None)),
    "norm_too_many_chunks": ("ast_grad_norm_f32", (1, 1, TOO_MANY, 1, 2.0, 1, None)),
    "scale_null_table": ("ast_grad_scale_f32", (None, 1, 1, 1, None)),
    "scale_null_state": ("ast_grad_scale_f32", (1, 1, 1, None, None)),
    "scale_no_tensors": ("ast_grad_scale_f32", (1, 0, 1, 1, None)),
    "scale_negative_tensors": ("ast_grad_scale_f32", (1, -1, 1, 1, None)),
    "scale_no_chunks": ("ast_grad_scale_f32", (1, 1, 0, 1, None)),
    "scale_negative_chunks": ("ast_grad_scale_f32", (1, 1, -1, 1, None)),
    "scale_too_many_chunks": ("ast_grad_scale_f32", (1, 1, TOO_MANY, 1, None)),
    "adam_null_table": ("ast_adam_step_f32", (None, 1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "adam_no_tensors": ("ast_adam_step_f32", (1, 0, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "adam_negative_tensors": ("ast_adam_step_f32", (1, -1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "adam_no_chunks": ("ast_adam_step_f32", (1, 1, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "adam_negative_chunks": ("ast_adam_step_f32", (1, 1, -1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "adam_too_many_chunks": ("ast_adam_step_f32", (1, 1, TOO_MANY, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "adam_step_zero": ("ast_adam_step_f32", (1, 1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0, None)),
    "adam_step_negative": ("ast_adam_step_f32", (1, 1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, -1, None)),
    "adam_null_table_no_clip": ("ast_adam_step_f32", (None, 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 1, None)),
    "sched_null_table": ("ast_adam_step_sched_f32", (None, 1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None)),
    "sched_null_sched": ("ast_adam_step_sched_f32", (1, 1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, None, 1, None)),
    "sched_null_sched_no_clip": ("ast_adam_step_sched_f32", (1, 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, None, 0, None)),
    "sched_no_tensors": ("ast_adam_step_sched_f32", (1, 0, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None)),
    "sched_negative_tensors": ("ast_adam_step_sched_f32", (1, -1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None)),
    "sched_no_chunks": ("ast_adam_step_sched_f32", (1, 1, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None)),
    "sched_negative_chunks": ("ast_adam_step_sched_f32", (1, 1, -1, 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None)),
    "sched_too_many_chunks": ("ast_adam_step_sched_f32", (1, 1, TOO_MANY, 1, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None)),
}


@pytest.mark.parametrize("case", sorted(ARG_ERRORS))
def test_optimizer_argument_errors_rejected_before_launch(case):
    name, args = ARG_ERRORS[case]
    assert getattr(_lib.lib(), name)(*args) < 0
