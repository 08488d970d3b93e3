"""CPU restatement of the relaxed earth mover's distance style loss (include/ast_hip.h, csrc/remd.hip).

Definition. x [N, C, H, W] is the stylised map, the differentiable side; y [Ns, C, Hs, Ws] the style map,
Ns = N, or 1 for a style shared by the batch. M = H W, P = Hs Ws; pixel i of x and pixel j of y are
C-vectors.
    u_i = 1 / ||x_i||_2, v_j = 1 / ||y_j||_2, exactly 0 when the squared norm is not positive
    s(i, j) = u_i v_j <x_i, y_j>,  D(i, j) = 1 - s(i, j): a zero vector is at distance 1 from everything
    r_i = min_j D(i, j), a_i its arg-min;  c_j = min_i D(i, j), b_j its arg-min; the lowest index on equal
          values; a NaN never wins; a value replaces the running (+inf, 0) only when strictly less
    rbar_b = mean_i r_i, cbar_b = mean_j c_j;  L = weight / N * sum_b max(rbar_b, cbar_b), the row branch
          (ROW = 1) taken when rbar_b >= cbar_b, the column branch (COL = 2) otherwise
    gradient, to x only, with xh_i = u_i x_i, yh_j = v_j y_j and g the upstream scalar:
          row branch     dL/dx_i = -(g weight / (N M)) u_i (yh_a - (1 - r_i) xh_i),  a = a_i
          column branch  dL/dx_i = -(g weight / (N P)) u_i sum over { j : b_j = i } of (yh_j - (1 - c_j) xh_i)
          0 where u_i = 0 and, in the column branch, where no column chose i

The implementation is the dense PyTorch formulation: normalise, bmm, min along each axis.
`dtype=torch.float64` is the reference, `dtype=torch.float32` the emulation. Every function takes
optional `index=` and `branch=` so that a value or a gradient can be evaluated at given indices and a
given branch.

Bars (all from the project, none from the code under test). OP_TOL = 2e-5 is the single-op bar of
swap_ref.py, wct_ref.py and test_gpu_parity.py; distances lie in [0, 2], cosines in [-1, 1]: scale 1.
    value     |r_i - D64(i, a_i)| <= OP_TOL, and the same for columns
    index     D64(i, a_i) <= min_j D64(i, j) + 2 OP_TOL, and the same for columns: two distances each
              within OP_TOL of the truth can only swap order inside that margin
    loss      loss and both means within OP_TOL absolute of float64 at weight 1
    branch    equals the reference's branch
    gradient  rel_inf <= OP_TOL against the float64 analytic gradient at the tested indices and branch
    inputs    in the float64 reference alone: the share of rows (columns) whose runner-up lies within
              2 OP_TOL of the winner is at most NEAR_TIE_MAX = 2 % per case and axis; every sample's
              |rbar - cbar| is at least BRANCH_GAP_MIN = 10 OP_TOL, except in c8_one_pixel
"""
import torch

from swap_ref import OP_TOL, features, rel_inf  # noqa: F401  (re-exported)

NEAR_TIE_MAX = 0.02
BRANCH_GAP_MIN = 10 * OP_TOL
ROW, COL = 1, 2

# name -> (n, ns, C, (H, W), (Hs, Ws)): the smallest shapes at which the kernel can still go wrong
CASES = {
    "c8_one_pixel": (1, 1, 8, (1, 1), (1, 1)),            # one pair; rbar = cbar exactly: the equality rule, row branch
    "c8_row_col": (1, 1, 8, (1, 9), (5, 1)),              # one row against one column; content pixels no column chose
    "c48_k_tails": (2, 2, 48, (7, 9), (6, 11)),           # C not a multiple of 32; partial tiles on both sides
    "c64_shared_style": (2, 1, 64, (12, 13), (11, 15)),   # ns = 1; several tiles on both sides
    "c160_tile_tails": (1, 1, 160, (9, 8), (19, 21)),     # several style tiles with a tail; three channel chunks
    "c32_many_queries": (1, 1, 32, (20, 23), (6, 7)),     # 8 content tiles: the column partials merge across tiles
    "c512_split_keys": (1, 1, 512, (8, 8), (32, 32)),     # the model's C; the library splits the style side
    "c24_few_content": (1, 1, 24, (2, 2), (17, 18)),      # 4 content pixels, 306 style pixels: long inverse lists
}


def case_inputs(name):
    """(x, y) of a named case."""
    n, ns, c, (h, w), (hs, ws) = CASES[name]
    seed = 11000 + 10 * list(CASES).index(name)
    return features(seed, (n, c, h, w)), features(seed + 1, (ns, c, hs, ws))


def inv_norms(x, dtype=torch.float64):
    """[n, pixels]: 1 / ||pixel||, 0 unless the squared norm is positive."""
    f = x.to(dtype).flatten(2)
    sq = (f * f).sum(dim=1)
    return torch.where(sq > 0, sq.clamp_min(torch.finfo(dtype).tiny).rsqrt(), torch.zeros_like(sq))


def normalized(x, dtype=torch.float64):
    """[n, pixels, C]: the unit vectors, a zero vector staying zero."""
    f = x.to(dtype).flatten(2)
    return (f * inv_norms(x, dtype)[:, None, :]).transpose(1, 2)


def distances(x, y, dtype=torch.float64):
    """D [n, M, P]; y's batch of 1 is shared."""
    xh, yh = normalized(x, dtype), normalized(y, dtype)
    return 1.0 - torch.bmm(xh, yh.expand(xh.shape[0], -1, -1).transpose(1, 2))


def argmin_last(d):
    """(min, index) along the last axis: the first minimum; NaN never wins; (+inf, 0) if nothing is below
    +inf."""
    clean = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    idx = clean.argmin(dim=-1)
    # torch's argmin returns the first of equal minima on the CPU; make it certain
    first = (clean == clean.gather(-1, idx[..., None])).int().argmax(dim=-1)
    return clean.gather(-1, first[..., None])[..., 0], first


def match(x, y, dtype=torch.float64, index=None):
    """(row_min [n, M], row_index, col_min [n, P], col_index). With index = (row_index, col_index) the
    minima are the distances at those indices."""
    d = distances(x, y, dtype)
    if index is None:
        r, a = argmin_last(d)
        c, b = argmin_last(d.transpose(1, 2))
    else:
        a, b = (t.reshape(d.shape[0], -1).long() for t in index)
        r = d.gather(2, a[..., None])[..., 0]
        c = d.transpose(1, 2).gather(2, b[..., None])[..., 0]
    return r, a, c, b


def means_branch(r, c, branch=None):
    """(row_mean [n], col_mean [n], branch [n]): ROW where row_mean >= col_mean, else COL; `branch`
    (an int or a tensor [n]) overrides."""
    rm, cm = r.mean(dim=1), c.mean(dim=1)
    nat = torch.where(rm >= cm, torch.full_like(rm, ROW), torch.full_like(rm, COL)).long()
    if branch is None:
        br = nat
    elif isinstance(branch, int):
        br = nat if branch == 0 else torch.full_like(nat, branch)
    else:
        br = branch.long().reshape(-1)
    return rm, cm, br


def loss(x, y, weight=1.0, dtype=torch.float64, index=None, branch=None):
    """(loss, row_mean, col_mean, branch) in `dtype`."""
    r, _, c, _ = match(x, y, dtype, index)
    rm, cm, br = means_branch(r, c, branch)
    return weight * torch.where(br == ROW, rm, cm).mean(), rm, cm, br


def loss_dense(x, y, weight=1.0, branch=None):
    """The float64 loss as a differentiable function of x through torch.autograd: normalise, bmm, min."""
    d = distances(x, y, torch.float64)
    r, c = d.min(dim=2).values, d.min(dim=1).values
    rm, cm, br = means_branch(r.detach(), c.detach(), branch)
    return weight * torch.where(br == ROW, r.mean(dim=1), c.mean(dim=1)).mean()


def grad(x, y, weight=1.0, g=1.0, dtype=torch.float64, index=None, branch=None):
    """The analytic gradient [n, C, H, W] in `dtype`, written from the formulas above; the minima are
    evaluated at `index` and the branch is `branch` when given."""
    n, ch = x.shape[:2]
    u = inv_norms(x, dtype)                                   # [n, M]
    xh, yh = normalized(x, dtype), normalized(y, dtype)       # [n, M, C], [ns, P, C]
    yh = yh.expand(n, -1, -1)
    r, a, c, b = match(x, y, dtype, index)
    _, _, br = means_branch(r, c, branch)
    m, p = r.shape[1], c.shape[1]
    out = torch.zeros_like(xh)
    for s in range(n):
        if int(br[s]) == ROW:
            t = yh[s][a[s]] - (1.0 - r[s])[:, None] * xh[s]
            out[s] = -(g * weight / (n * m)) * u[s][:, None] * t
        else:
            acc = torch.zeros_like(xh[s])
            acc.index_add_(0, b[s], yh[s])                                   # sum of yh_j over the list of i
            coef = torch.zeros(m, dtype=dtype).index_add_(0, b[s], 1.0 - c[s])   # sum of (1 - c_j)
            out[s] = -(g * weight / (n * p)) * u[s][:, None] * (acc - coef[:, None] * xh[s])
    return out.transpose(1, 2).reshape(n, ch, *x.shape[2:])


# ---- the checks of the bars ---------------------------------------------------------------------------

def near_tie_fraction(d):
    """The share of rows of d [n, R, K] whose runner-up lies within 2 OP_TOL of the winner."""
    if d.shape[2] < 2:
        return 0.0
    low = (-d).topk(2, dim=2).values
    return float(((low[..., 0] - low[..., 1]) <= 2 * OP_TOL).double().mean())


def check_axis(vmin, vidx, d64):
    """(value error, worst index shortfall) of the minima (vmin, vidx) [n, R] along the last axis of the
    float64 distances d64 [n, R, K]: the value bar asks the first <= OP_TOL, the index rule the second
    <= 2 OP_TOL."""
    n, rws, _ = d64.shape
    at = d64.gather(2, vidx.reshape(n, rws, 1).long())[..., 0]
    e_val = float((vmin.reshape(n, rws).double() - at).abs().max())
    shortfall = float((at - d64.min(dim=2).values).max())
    return e_val, shortfall
