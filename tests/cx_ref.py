"""CPU restatement of the contextual loss (include/ast_hip.h, csrc/cx.hip; Mechrez, Talmi, Zelnik-Manor,
ECCV 2018).

Definition. x [N, C, H, W] is the stylised map, the differentiable side; y [Ns, C, Hs, Ws] the target, Ns = N,
or 1 for a target shared by the batch; it is data. M = H W, P = Hs Ws; h > 0 the bandwidth; eps = EPS.
    centring (default on)   mu[c] = mean_j y[c, j];  xc = x - mu, yc = y - mu; off: xc = x, yc = y
    u_i, v_j, D(i, j)       those of remd_ref.py on (xc, yc): D = 1 - u_i v_j <xc_i, yc_j>, a zero vector at
                            distance 1 from everything; no clamp
    row side                r_i = min_j D(i, j), m_i its arg-min; k_i = 1 / (r_i + eps)
                            w(i, j) = exp((1 - D(i, j) k_i) / h);  S_i = sum_j w(i, j);  E_i = sum_j w(i, j) D(i, j)
    column side             CX(i, j) = w(i, j) / S_i;  c_j = max_i CX(i, j), a_j its arg-max: the lowest index on
                            equal values, a NaN never wins, (-inf, 0) without a winner
    loss                    CX_b = (1 / P) sum_j c_j;  L = weight / N * sum_b -log CX_b
    gradient, to x only, g the upstream scalar, xh_i = u_i xc_i, yh_j = v_j yc_j, J_i = { j : a_j = i }:
        A_i = sum_{J_i} w(i, j);  B_i = sum_{J_i} w(i, j) D(i, j);  T_i = B_i / S_i - A_i E_i / S_i^2
        G_i = (k_i / (h S_i)) (sum_{J_i} w(i, j) yh_j - (A_i / S_i) sum_j w(i, j) yh_j) - (k_i^2 T_i / h) yh_{m_i}
        dx_i = -(g weight / (N P CX_b)) u_i (G_i - xh_i <xh_i, G_i>);  0 for an empty J_i and for u_i = 0

The implementation is the dense PyTorch formulation: centre, normalise, bmm, min, divide, exp, sum, divide,
max, log. `dtype=torch.float64` is the reference, `dtype=torch.float32` the emulation. Every function takes
an optional `index=(row_index, col_index)` so that a value or a gradient can be evaluated at given indices.

Bars (all from the project and the float64 reference, none from the code under test). OP_TOL = 2e-5 is the
project's single-op bar on a distance. An error e in D(i, j) and in r_i moves the exponent (1 - D k) / h by at
most (1 + k max_j D) k e / h, so per case
    kappa = max_i (1 + k_i max_j D(i, j)) k_i / h          (float64)
is the amplification from an error in D to a relative error in w.
    S, E, w        relative <= kappa OP_TOL
    col_cx         relative <= 2 kappa OP_TOL against the float64 value at the returned index (a ratio w / S)
    index          the float64 value at the returned index >= (1 - 4 kappa OP_TOL) x the float64 maximum
    -log CX_b      absolute <= 2 kappa OP_TOL
    gradient       rel_inf <= 4 kappa OP_TOL against the float64 analytic gradient at the tested indices (two
                   ratios, each with an uncertain numerator and denominator)
    inputs         in float64 alone: kappa OP_TOL <= KAPPA_TOL_MAX = 1e-3; the share of columns whose runner-up
                   lies within 4 kappa OP_TOL relative of the winner, and remd_ref.near_tie_fraction of the rows
                   of the centred maps, at most NEAR_TIE_MAX = 2 %; the float32 emulation's gradient error at
                   the float64 indices at most a quarter of the gradient bar
"""
import torch

import remd_ref as R
from remd_ref import OP_TOL, features, rel_inf  # noqa: F401  (re-exported)

EPS = 1e-5
NEAR_TIE_MAX = 0.02
KAPPA_TOL_MAX = 1e-3

# name -> (remd_ref case, C, h): the shapes and seeds of remd_ref.CASES at h = 0.5, c8_row_col at C = 16 (at
# C = 8 its kappa OP_TOL is 2.4e-3), and h = 0.1 on the two cases that keep the conditions there.
CASES = {name: (name, R.CASES[name][2], 0.5) for name in R.CASES if name != "c8_row_col"}
CASES["c16_row_col"] = ("c8_row_col", 16, 0.5)
CASES["c512_split_keys_h01"] = ("c512_split_keys", 512, 0.1)
CASES["c160_tile_tails_h01"] = ("c160_tile_tails", 160, 0.1)

# Two more for the backward's dense pass, which takes one more path per 128 channels up to 512 and splits the
# channels over the grid past that (the cases above have C <= 128, 160 and 512):
# name -> (n, ns, C, (H, W), (Hs, Ws), seed, h)
EXTRA = {
    "c320_three_blocks": (1, 1, 320, (6, 11), (8, 9), 12130, 0.5),    # three channel blocks; two tiles a side
    "c520_two_groups": (2, 1, 520, (5, 14), (7, 10), 12110, 0.5),      # two channel groups, the second one 8 wide
}
ALL_CASES = list(CASES) + list(EXTRA)


def case_inputs(name):
    """(x, y, h) of a named case."""
    if name in EXTRA:
        n, ns, c, (hh, ww), (hs, ws), seed, h = EXTRA[name]
    else:
        base, c, h = CASES[name]
        n, ns, _, (hh, ww), (hs, ws) = R.CASES[base]
        seed = 11000 + 10 * list(R.CASES).index(base)
    return features(seed, (n, c, hh, ww)), features(seed + 1, (ns, c, hs, ws)), h


def center(x, y, dtype=torch.float64, on=True):
    """(xc, yc) in `dtype`: both maps minus y's channel means."""
    xf, yf = x.to(dtype), y.to(dtype)
    if not on:
        return xf, yf
    mu = yf.flatten(2).mean(dim=2)[:, :, None, None]
    return xf - mu, yf - mu


def argmax_last(v):
    """(max, index) along the last axis: the first maximum; NaN never wins; (-inf, 0) without a winner."""
    m, i = R.argmin_last(-v)
    return -m, i


def parts(x, y, h=0.5, dtype=torch.float64, index=None, center_on=True):
    """A dict of everything the loss is made of, in `dtype`: d [n, M, P], r, m, k, w, S, E, cx [n, M, P],
    c, a [n, P], cxb [n]. With index = (row_index, col_index), r and c are taken at those indices."""
    xc, yc = center(x, y, dtype, center_on)
    d = R.distances(xc, yc, dtype)
    n = d.shape[0]
    if index is None:
        r, m = R.argmin_last(d)
    else:
        m = index[0].reshape(n, -1).long()
        r = d.gather(2, m[..., None])[..., 0]
    k = 1.0 / (r + EPS)
    w = torch.exp((1.0 - d * k[..., None]) / h)
    S, E = w.sum(dim=2), (w * d).sum(dim=2)
    cx = w / S[..., None]
    if index is None:
        c, a = argmax_last(cx.transpose(1, 2))
    else:
        a = index[1].reshape(n, -1).long()
        c = cx.transpose(1, 2).gather(2, a[..., None])[..., 0]
    return dict(xc=xc, yc=yc, d=d, r=r, m=m, k=k, w=w, S=S, E=E, cx=cx, c=c, a=a, cxb=c.mean(dim=1))


def loss(x, y, weight=1.0, h=0.5, dtype=torch.float64, index=None, center_on=True):
    """(loss, per-sample CX_b [n]) in `dtype`."""
    p = parts(x, y, h, dtype, index, center_on)
    return weight * (-torch.log(p["cxb"])).mean(), p["cxb"]


def loss_dense(x, y, weight=1.0, h=0.5, center_on=True):
    """The float64 loss as a differentiable function of x through torch.autograd."""
    xc, yc = center(x, y.detach(), torch.float64, center_on)
    d = R.distances(xc, yc, torch.float64)
    k = 1.0 / (d.min(dim=2).values + EPS)
    w = torch.exp((1.0 - d * k[..., None]) / h)
    cx = w / w.sum(dim=2, keepdim=True)
    return weight * (-torch.log(cx.max(dim=1).values.mean(dim=1))).mean()


def grad(x, y, weight=1.0, g=1.0, h=0.5, dtype=torch.float64, index=None, center_on=True):
    """The analytic gradient [n, C, H, W] in `dtype`, written from the formulas above, the minima and maxima
    taken at `index` when given."""
    q = parts(x, y, h, dtype, index, center_on)
    n, ch = x.shape[:2]
    u = R.inv_norms(q["xc"], dtype)                                         # [n, M]
    xh = R.normalized(q["xc"], dtype)                                       # [n, M, C]
    yh = R.normalized(q["yc"], dtype).expand(n, -1, -1)                     # [n, P, C]
    d, w, S, E, k, m, a = (q[t] for t in ("d", "w", "S", "E", "k", "m", "a"))
    M, P = d.shape[1:]
    ind = (a[:, None, :] == torch.arange(M)[None, :, None]).to(dtype)       # [n, M, P]: a_j == i
    A, B = (ind * w).sum(dim=2), (ind * w * d).sum(dim=2)
    T = B / S - A * E / (S * S)
    alpha, beta, tau = k / (h * S), A / S, k * k * T / h
    ym = torch.gather(yh, 1, m[..., None].expand(-1, -1, ch))               # yh_{m_i}
    G = alpha[..., None] * (torch.bmm(ind * w, yh) - beta[..., None] * torch.bmm(w, yh)) - tau[..., None] * ym
    active = (ind.sum(dim=2) > 0) & (u > 0)
    G = torch.where(active[..., None], G, torch.zeros_like(G))
    scale = -(g * weight / (n * P * q["cxb"]))[:, None, None]
    out = scale * u[..., None] * (G - xh * (xh * G).sum(dim=2, keepdim=True))
    out = torch.where(active[..., None], out, torch.zeros_like(out))
    return out.transpose(1, 2).reshape(n, ch, *x.shape[2:])


# ---- the checks of the bars ---------------------------------------------------------------------------

def kappa(x, y, h, center_on=True):
    """max_i (1 + k_i max_j D(i, j)) k_i / h in float64."""
    q = parts(x, y, h, torch.float64, None, center_on)
    return float(((1.0 + q["k"] * q["d"].max(dim=2).values) * q["k"] / h).max())


def col_near_tie_fraction(cx, tol):
    """The share of columns of cx [n, M, P] whose runner-up lies within `tol` relative of the winner."""
    if cx.shape[1] < 2:
        return 0.0
    top = cx.transpose(1, 2).topk(2, dim=2).values
    return float(((top[..., 0] - top[..., 1]) <= tol * top[..., 0]).double().mean())


def grad_err(got, ref):
    """rel_inf(got, ref); where the reference gradient is zero -- exactly, or as float64 rounding noise below
    1e-12 at inputs of scale 1 (a target of one pixel: CX = 1 whatever x is) -- the absolute error."""
    top = float(ref.double().abs().max())
    return rel_inf(got, ref) if top > 1e-12 else float((got.double() - ref.double()).abs().max())


def active_fraction(a, M):
    """The share of rows that some column chose."""
    return sum(len(set(s.tolist())) for s in a) / float(a.shape[0] * M)
