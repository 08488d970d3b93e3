"""Float64 references and derived error bounds for the stages of the inference MobileNet block
(expand + depthwise + SE pool, SE fold, gated pointwise conv, expand-as-GEMM), on the CPU.

Every reference is computed from the operands the kernel reads (the block plan's packed weights
read back, the stored input), so every bf16 operand is exact in float64. Every bound is derived
from the roundings a kernel may make, never measured:

  u   unit roundoff of the storage type: 2^-8 for bf16 (8 significand bits: half an ulp of a value
      just above a power of two), 2^-24 for fp32
  eps 2^-24, fp32 arithmetic and accumulation
  L   1.5, the Lipschitz constant of Hardswish: slope (2v + 3) / 6 on [-3, 3], which peaks at 1.5

Hidden map.   H64 = hs(w1 . x + b1), A = |w1| . |x| + |b1|
              eH  = u |H64| + L (cin + 2) eps A
              (fp32 dot product of cin terms plus bias: (cin + 2) eps A before the activation, times
              L after it; one storage rounding of the result. Ratio-1 blocks have no expand:
              H64 = x, or its nearest x2 upsample, and eH = 0.)
Depthwise D.  D64 = hs(dw(reflect(H64)) + bd), S = |wdw| (*) |H64| + |bd| with the same padding,
              dw_abs(e) = |wdw| (*) e
              |D - D64| <= u |D64| + L [(1 + u) dw_abs(eH) + u S + (k^2 + 2) eps S]
              (the hidden error through the taps, the taps rounded to the storage type (v5: bf16 MFMA
              operands; the (1 + u) is the rounded tap on the hidden error), the fp32 sum of k^2 taps
              plus bias, Hardswish, one storage rounding. v4 keeps hidden values and taps in fp32 and
              sits inside the same bound.)
Pool vs f64.  |pool - sum_pixels D64| <= sum_pixels bound_D
Pool vs the kernel's own D (the tight one: a miscounted tile, row or column moves the sum by ~1/W):
              |pool - sum D_gpu| <= u sum|D_gpu| + (ho wo) eps sum|D_gpu|
              (the pool adds the values before their storage rounding; fp32 sum of ho wo terms)
SE fold.      from the kernel's own pool: gate64 = clamp(fc2 relu(fc1 pool / hw + b) + b, 0, 1),
              wg64 = w2 gate64; G the same expression without clamps on absolute values
              |wg - wg64| <= u |wg64| + |w2| gamma G,  gamma = (hid + red + 8) eps
              wg rows cout..cout_pad and columns hid..hid_pad are exactly 0
Pointwise.    from the kernel's own D and wg: out64 = wg . D + b2 (+ res)
              |out - out64| <= u |out64| + (hid + 3) eps (|wg| . |D| + |b2| + |res|)
Expand GEMM.  |out - H64| <= eH with cin = c1 + c2

Every check is per element, no element exempt, no quantiles. A check returns max(err / bound) and,
when an element is outside, a message with its index, channel, tile coordinates and err / bound.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
L_HS = 1.5
U_BF16 = 2.0 ** -8
U_FP32 = 2.0 ** -24
TILE = (32, 28)   # rows x columns of the v5 / v4 output tile, for the failure message only


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: U_BF16, torch.float32: U_FP32}[dtype]


def f64(t):
    return None if t is None else t.detach().to("cpu").double()


def hs(v):
    return v * torch.clamp(v / 6.0 + 0.5, 0.0, 1.0)


def upsample2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


# -- the stage references ----------------------------------------------------------------------
def hidden_ref(x, w1, b1, u):
    """(H64, eH) of the expand: x [n, cin, h, w], w1 [hid, cin], b1 [hid], all float64."""
    cin = x.shape[1]
    pre = torch.einsum("oc,nchw->nohw", w1, x) + b1.view(1, -1, 1, 1)
    a = torch.einsum("oc,nchw->nohw", w1.abs(), x.abs()) + b1.abs().view(1, -1, 1, 1)
    h64 = hs(pre)
    return h64, u * h64.abs() + L_HS * (cin + 2) * EPS * a


def _dw(hmap, wd, bias, k, s):
    p = (k - 1) // 2
    c = hmap.shape[1]
    return F.conv2d(F.pad(hmap, (p, p, p, p), mode="reflect"), wd.reshape(c, 1, k, k), bias, stride=s, groups=c)


def dw_ref(h64, eh, wd, bd, k, s, u):
    """(D64, bound_D) of the depthwise conv + Hardswish on the hidden map h64 with error eh."""
    d64 = hs(_dw(h64, wd, bd, k, s))
    sabs = _dw(h64.abs(), wd.abs(), bd.abs(), k, s)
    through = _dw(eh, wd.abs(), None, k, s) if eh is not None else torch.zeros_like(d64)
    bound = u * d64.abs() + L_HS * ((1 + u) * through + u * sabs + (k * k + 2) * EPS * sabs)
    return d64, bound


def pool_vs_own_d(d_gpu, u):
    dg = f64(d_gpu)
    ho, wo = dg.shape[2:]
    sabs = dg.abs().sum(dim=(2, 3))
    return dg.sum(dim=(2, 3)), (u + ho * wo * EPS) * sabs


def se_fold_ref(pool, hw, fc1w, fc1b, fc2w, fc2b, w2, u):
    """(wg64 [n, cout, hid], bound) from the pool sums [n, hid] (all float64)."""
    hid, red = fc1w.shape[1], fc1w.shape[0]
    mean = pool / hw
    gate = torch.clamp(torch.relu(mean @ fc1w.T + fc1b) @ fc2w.T + fc2b, 0.0, 1.0)
    g_abs = (mean.abs() @ fc1w.abs().T + fc1b.abs()) @ fc2w.abs().T + fc2b.abs()
    wg64 = w2.unsqueeze(0) * gate.unsqueeze(1)
    gamma = (hid + red + 8) * EPS
    return wg64, u * wg64.abs() + w2.abs().unsqueeze(0) * (gamma * g_abs).unsqueeze(1)


def pw_ref(d_gpu, wg_gpu, b2, res, cout, hid, u):
    """(out64, bound) of the gated pointwise conv from the stored D [n, hid, h, w] and
    wg [n, cout_pad, hid_pad]; res (float64, at the output's size) or None."""
    dg, wg = f64(d_gpu), f64(wg_gpu)[:, :cout, :hid]
    out = torch.einsum("nok,nkhw->nohw", wg, dg)
    mag = torch.einsum("nok,nkhw->nohw", wg.abs(), dg.abs())
    if b2 is not None:
        out = out + b2.view(1, -1, 1, 1)
        mag = mag + b2.abs().view(1, -1, 1, 1)
    if res is not None:
        out = out + res
        mag = mag + res.abs()
    return out, u * out.abs() + (hid + 3) * EPS * mag


# -- the per-element check ---------------------------------------------------------------------
def check(name, got, ref, bound):
    """(max err / bound, message or None): every element of |got - ref| against bound. An element
    with bound 0 must be exact; a non-finite value is outside. The message names the worst element:
    its index, channel and tile coordinates."""
    got = f64(got)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).double())
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
    worst = float(ratio.max())
    if worst <= 1.0:
        return worst, None
    flat = int(ratio.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), ratio.shape))
    where = f"index {idx}"
    if len(idx) >= 2:
        where += f", channel {idx[1]}"
    if len(idx) == 4:
        where += f", tile (band {idx[2] // TILE[0]}, strip {idx[3] // TILE[1]}) row {idx[2] % TILE[0]} col {idx[3] % TILE[1]}"
    n_out = int((ratio > 1.0).sum())
    return worst, (f"{name}: {n_out} of {ratio.numel()} elements outside the bound; worst at {where}: got "
                   f"{float(got[idx]):.9g}, ref {float(ref[idx]):.9g}, err {float(err[idx]):.3e}, bound "
                   f"{float(bound[idx]):.3e}, err/bound {worst:.3g}")


def check_zero_padding(wg, cout, hid):
    """(0 or inf, message or None): the padding rows and columns of wg are exactly 0."""
    w = f64(wg)
    bad = int(torch.count_nonzero(w[:, cout:, :])) + int(torch.count_nonzero(w[:, :cout, hid:]))
    if bad == 0:
        return 0.0, None
    nz = torch.nonzero(torch.cat((w[:, :, hid:].flatten(), w[:, cout:, :hid].flatten())))
    return math.inf, f"wg padding: {bad} non-zero entries in rows {cout}.. or columns {hid}.. (first flat index {int(nz[0])})"


# -- a block's operands and the whole chain of checks ------------------------------------------
def operands(x, w1, b1, wd, bd, fc1w, fc1b, fc2w, fc2b, w2, b2, k, s, up, identity, u):
    """The block's operands in float64. x is the (concatenated) stored input; w1/b1 None for a
    ratio-1 block; wd [hid, k*k]; b2 None without a BatchNorm after the pointwise conv."""
    return SimpleNamespace(x=f64(x), w1=f64(w1), b1=f64(b1), wd=f64(wd), bd=f64(bd), fc1w=f64(fc1w), fc1b=f64(fc1b),
                           fc2w=f64(fc2w), fc2b=f64(fc2b), w2=f64(w2), b2=f64(b2), k=k, s=s, up=up,
                           identity=identity, u=u, hid=int(wd.shape[0]), cout=int(w2.shape[0]))


def operands_from_plan(blk, p, x, x2, up, dtype):
    """operands() from DepthWiseConv._plan: the tensors the kernels read, read back."""
    cin = blk.inp
    xs = x if x2 is None else torch.cat((x, x2), 1)
    w1 = None if p.w1p is None else p.w1p[:blk.hidden_dim, :cin]
    return operands(xs, w1, p.b1, p.wd, p.bd, p.fc1w, p.fc1b, p.fc2w, p.fc2b, p.w2, p.b2, blk.kernel_size,
                    blk.stride, up, blk.identity, unit_roundoff(dtype))


def stage_report(op, d, pool, wg, out, hmid=None, d_own=None):
    """Every stage check of one block run: {stage: (max err/bound, message or None)}.

    d, pool, wg, out are what the kernels (or a restatement of them) produced. hmid, when given, is
    the stored output of the expand GEMM; the depthwise reference then starts from it (a ratio-1
    depthwise on a stored map). d_own, when given, replaces d in the pool-vs-own-D check."""
    rep = {}
    u = op.u
    cached = getattr(op, "_dref", None) if hmid is None else None
    if cached is not None:   # the float64 reference of D is computed once per block
        d64, bd_ = cached
    else:
        if op.w1 is not None:
            h64, eh = hidden_ref(op.x, op.w1, op.b1, u)
            if hmid is not None:
                rep["expand_gemm"] = check("expand GEMM H", hmid, h64, eh)
                h64, eh = f64(hmid), None
        else:
            h64, eh = (upsample2(op.x) if op.up == 2 else op.x), None
        d64, bd_ = dw_ref(h64, eh, op.wd.reshape(op.hid, -1), op.bd, op.k, op.s, u)
        if hmid is None:
            op._dref = (d64, bd_)
    rep["D"] = check("depthwise D", d, d64, bd_)
    rep["pool_f64"] = check("pool vs float64", pool, d64.sum(dim=(2, 3)), bd_.sum(dim=(2, 3)))
    rep["pool_own_D"] = check("pool vs own D", pool, *pool_vs_own_d(d if d_own is None else d_own, u))
    hw = d64.shape[2] * d64.shape[3]
    wg64, bw = se_fold_ref(f64(pool), hw, op.fc1w, op.fc1b, op.fc2w, op.fc2b, op.w2, u)
    rep["wg"] = check("SE fold wg", f64(wg)[:, :op.cout, :op.hid], wg64, bw)
    rep["wg_padding"] = check_zero_padding(wg, op.cout, op.hid)
    res = None
    if op.identity:
        res = upsample2(op.x) if op.up == 2 else op.x
    rep["out"] = check("pointwise out", out, *pw_ref(d, wg, op.b2, res, op.cout, op.hid, u))
    return rep


def failures(rep):
    return [msg for _, msg in rep.values() if msg is not None]


def assert_stages(rep, label=""):
    bad = failures(rep)
    assert not bad, f"{label}\n  " + "\n  ".join(bad)


def ratios(rep):
    return {k: v[0] for k, v in rep.items()}
