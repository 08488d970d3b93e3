"""Float64 restatement of the optimizer step (clip_grad_norm_ for the L2 norm + torch.optim.Adam
without amsgrad or weight decay) in plain numpy: the reference side of tests/test_optim_cpu.py
(which pins it to torch's own float64 Adam) and tests/test_gpu_optim.py.

Everything is float64; the bias corrections are Python doubles, as torch computes them. A
parameter whose gradient is None in a step is left out of the norm and is not stepped (its step
count stays), as in torch."""
import math

import numpy as np

CHUNK = 65536   # elements per workgroup of the kernels under test (layout checks only)


def total_norm(grads):
    """L2 norm over every array of `grads` (None entries are ignored); 0.0 for no gradients."""
    s = 0.0
    for g in grads:
        if g is not None:
            g = np.asarray(g, np.float64)
            s += float(np.sum(g * g))
    return math.sqrt(s)


def clip_coef(norm, max_norm):
    """torch: clamp(max_norm / (norm + 1e-6), max=1.0). A NaN norm gives NaN, an inf norm 0."""
    c = float(max_norm) / (float(norm) + 1e-6)
    if c != c:
        return float("nan")
    return min(1.0, c)


def adam_step(p, g, m, v, step, lr, b1, b2, eps):
    """One Adam update at (1-based) step count `step`; returns the new (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def run(params, grad_steps, groups, max_norm, state=None):
    """Drive len(grad_steps) optimizer steps.

    params:      list of arrays.
    grad_steps:  per step, a list with one gradient (or None) per parameter.
    groups:      list of dict(idx=[parameter indices], lr=, betas=(b1, b2), eps=).
    max_norm:    None for no clipping, else ONE norm over the gradients of all groups.
    state:       optional (exp_avg list, exp_avg_sq list, step list) to resume from.

    Returns dict(params, exp_avg, exp_avg_sq, step, norms, coefs, grads): the final tensors, the
    per-parameter step counts, per step the total norm and clip coefficient (None without
    clipping), and the last step's gradients as clip_grad_norm_ leaves them."""
    ps = [np.array(p, np.float64) for p in params]
    if state is None:
        ms = [np.zeros_like(p) for p in ps]
        vs = [np.zeros_like(p) for p in ps]
        steps = [0] * len(ps)
    else:
        ms = [np.array(m, np.float64) for m in state[0]]
        vs = [np.array(v, np.float64) for v in state[1]]
        steps = [int(s) for s in state[2]]
    norms, coefs, grads = [], [], None
    for raw in grad_steps:
        grads = [None if g is None else np.array(g, np.float64) for g in raw]
        if max_norm is not None:
            norm = total_norm(grads)
            coef = clip_coef(norm, max_norm)
            grads = [None if g is None else g * coef for g in grads]
            norms.append(norm)
            coefs.append(coef)
        else:
            norms.append(None)
            coefs.append(None)
        for grp in groups:
            b1, b2 = grp["betas"]
            for i in grp["idx"]:
                if grads[i] is None:
                    continue
                steps[i] += 1
                ps[i], ms[i], vs[i] = adam_step(ps[i], grads[i], ms[i], vs[i], steps[i], grp["lr"], b1, b2,
                                                grp["eps"])
    return dict(params=ps, exp_avg=ms, exp_avg_sq=vs, step=steps, norms=norms, coefs=coefs, grads=grads)


def nchunks(numels):
    return sum(-(-int(n) // CHUNK) for n in numels)
