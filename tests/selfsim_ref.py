"""CPU restatement of the self-similarity content loss (include/ast_hip.h, csrc/selfsim.hip).

Definition. x [n, C, H, W] is the stylised map, the differentiable side; c the content map of the same
shape; N = H W pixels per sample. Per sample, for either map f:
    u_i = 1 / ||f_i||_2, exactly 0 unless the squared norm is positive;  fh_i = u_i f_i
    D_f(i, j) = 1 - <fh_i, fh_j> for i != j, D_f(i, i) = 0: a zero vector is at distance 1 from every other pixel
    r_f(j) = sum_i D_f(i, j);  q_f(j) = 1 / r_f(j) when r_f(j) is positive and finite, else 0
    e(i, j) = D_x(i, j) q_x(j) - D_c(i, j) q_c(j);  s(i, j) = sign e(i, j), 0 for e == 0, NaN and the diagonal
    L_b = (1 / N) sum_{i != j} |e(i, j)|;  L = weight / n * sum_b L_b
    t(j) = q_x(j) sum_{k != j} s(k, j) D_x(k, j)
    gradient, to x only, with g the upstream scalar:
        W(m, j) = (s(m, j) - t(j)) q_x(j) + (s(j, m) - t(m)) q_x(m)        (m != j)
        G_m = sum_{j != m} W(m, j) xh_j;  dxh_m = -(g weight / (n N)) G_m
        dx_m = u_m (dxh_m - xh_m <xh_m, dxh_m>), 0 where u_m = 0

The implementation is the dense PyTorch formulation: normalise, bmm, column-normalise, abs, sum.
`dtype=torch.float64` is the reference, `dtype=torch.float32` the emulation. `grad` and `signed_sums`
take `signs=` so that they can be evaluated at given signs (the kernel's planes, unpacked), t being
recomputed from them.

Bars (all from the project, none from the code under test). OP_TOL = 2e-5 is the single-op bar of
swap_ref.py, remd_ref.py and test_gpu_parity.py; distances lie in [0, 2]: scale 1.
    column sums  |r - r64| <= OP_TOL N: a sum of N distances each within OP_TOL
    loss         |L - L64| <= OP_TOL for the loss and every per-sample value (L lies in [0, 2])
    signs        where a sign differs from the float64 sign, |e64(i, j)| <= 2 OP_TOL (q_x(j) + q_c(j)): each
                 D within OP_TOL of the truth moves e by at most OP_TOL (q_x + q_c)
    t            |t - t64| <= OP_TOL against the float64 t at the tested signs (|t| <= 1)
    gradient     rel_inf <= OP_TOL against the float64 analytic gradient at the tested signs; where that
                 gradient is exactly 0 (one pixel: q = 0; two pixels: every term cancels), max |dx| <= OP_TOL
                 times the largest sum of the magnitudes of an element's terms (grad_error)
    inputs       in the float64 reference alone: the share of off-diagonal pairs inside the sign margin is
                 at most NEAR_TIE_MAX = 2 % per case (the two degenerate cases exempt); no zero vector
"""
import torch

from swap_ref import OP_TOL, features, rel_inf  # noqa: F401  (re-exported)

NEAR_TIE_MAX = 0.02
DEGENERATE = ("s8_one_pixel", "s8_two_pixels")

# name -> (n, C, (H, W)): the smallest shapes at which the kernels can still go wrong
CASES = {
    "s8_one_pixel": (1, 8, (1, 1)),          # q = 0: loss 0, gradient 0, empty planes
    "s8_two_pixels": (1, 8, (1, 2)),         # every normalised column is (0, 1) on both sides: loss ~ 0
    "s48_k_tails": (2, 48, (7, 9)),          # N = 63, one partial tile, C not a multiple of 32, two samples
    "s64_tiles": (2, 64, (12, 13)),          # N = 156: three tiles with a tail, six triangle pairs
    "s160_chunks": (1, 160, (9, 8)),         # three channel chunks, two tiles
    "s32_many_tiles": (1, 32, (20, 23)),     # N = 460: 36 tile pairs, 8-word plane rows, t merged over 8 tiles
    "s512_model_c": (1, 512, (16, 16)),      # the model's C, and channel chunks in the backward
    "s24_row": (1, 24, (1, 130)),            # a one-row map
    "s40_near_content": (1, 40, (10, 11)),   # x = c (1 + 0.05 features): small e, the training regime
}


def case_inputs(name):
    """(x, c) of a named case."""
    n, ch, (h, w) = CASES[name]
    seed = 12000 + 10 * list(CASES).index(name)
    c = features(seed + 1, (n, ch, h, w))
    if name == "s40_near_content":
        return c * (1.0 + 0.05 * features(seed + 2, (n, ch, h, w))), c
    return features(seed, (n, ch, h, w)), c


def inv_norms(x, dtype=torch.float64):
    """[n, N]: 1 / ||pixel||, 0 unless the squared norm is positive."""
    f = x.to(dtype).flatten(2)
    sq = (f * f).sum(dim=1)
    return torch.where(sq > 0, sq.clamp_min(torch.finfo(dtype).tiny).rsqrt(), torch.zeros_like(sq))


def unit(x, dtype=torch.float64):
    """[n, N, C]: the unit vectors, a zero vector staying zero."""
    f = x.to(dtype).flatten(2)
    return (f * inv_norms(x, dtype)[:, None, :]).transpose(1, 2)


def distances(x, dtype=torch.float64):
    """D [n, N, N]: the cosine distances inside a map, 0 on the diagonal."""
    xh = unit(x, dtype)
    d = 1.0 - torch.bmm(xh, xh.transpose(1, 2))
    return d * (1.0 - torch.eye(d.shape[1], dtype=d.dtype))


def inv_colsum(r):
    ok = (r > 0) & torch.isfinite(r)
    return torch.where(ok, 1.0 / torch.where(ok, r, torch.ones_like(r)), torch.zeros_like(r))


def colsum(x, dtype=torch.float64):
    """r [n, N] by its definition: the sum of the distances of a column."""
    return distances(x, dtype).sum(dim=1)


def colsum_fast(x, dtype=torch.float64):
    """r [n, N] in the form the kernel uses: (N - 1) - (<fh_j, S> - ||fh_j||^2), S the sum of the unit vectors."""
    xh = unit(x, dtype)
    s = xh.sum(dim=1, keepdim=True)
    return (xh.shape[1] - 1) - ((xh * s).sum(dim=2) - (xh * xh).sum(dim=2))


def differences(x, c, dtype=torch.float64):
    """(e [n, N, N], D_x, q_x [n, N], q_c)."""
    dx, dc = distances(x, dtype), distances(c, dtype)
    qx, qc = inv_colsum(dx.sum(dim=1)), inv_colsum(dc.sum(dim=1))
    return dx * qx[:, None, :] - dc * qc[:, None, :], dx, qx, qc


def sign_of(e):
    """+1 / -1 / 0; NaN gives 0; the diagonal of e is 0 already."""
    return (e > 0).to(e.dtype) - (e < 0).to(e.dtype)


def loss(x, c, weight=1.0, dtype=torch.float64):
    """(loss, per_sample [n]) in `dtype`."""
    e = differences(x, c, dtype)[0]
    per = e.abs().sum(dim=(1, 2)) / e.shape[1]
    return weight * per.mean(), per


def loss_dense(x, c, weight=1.0):
    """The float64 loss as a differentiable function of x through torch.autograd."""
    return loss(x, c.detach(), weight)[0]


def signed_sums(x, c, dtype=torch.float64, signs=None):
    """t [n, N] at `signs` [n, N, N] (the natural ones of `dtype` when None)."""
    e, dx, qx, _ = differences(x, c, dtype)
    s = sign_of(e) if signs is None else signs.to(dtype)
    return qx * (s * dx).sum(dim=1)


def grad(x, c, weight=1.0, g=1.0, dtype=torch.float64, signs=None):
    """The analytic gradient [n, C, H, W] in `dtype`, written from the formulas above, at `signs`."""
    n, ch = x.shape[:2]
    e, dx, qx, _ = differences(x, c, dtype)
    s = sign_of(e) if signs is None else signs.to(dtype)
    npix = e.shape[1]
    t = qx * (s * dx).sum(dim=1)                                  # [n, N]
    a = (s - t[:, None, :]) * qx[:, None, :]                      # A(m, j) = (s(m, j) - t(j)) q(j)
    w = (a + a.transpose(1, 2)) * (1.0 - torch.eye(npix, dtype=e.dtype))
    u, xh = inv_norms(x, dtype), unit(x, dtype)                   # [n, N], [n, N, C]
    dxh = -(g * weight / (n * npix)) * torch.bmm(w, xh)
    out = u[..., None] * (dxh - xh * (xh * dxh).sum(dim=2, keepdim=True))
    return out.transpose(1, 2).reshape(n, ch, *x.shape[2:])


def grad_term_scale(x, c, weight=1.0, g=1.0, signs=None):
    """The largest sum of the magnitudes of the terms a gradient element adds up, in float64: the formulas of
    `grad` with |s| + |t| for s - t and |xh| for xh. Where every term cancels (two pixels: t(j) = s(i, j)
    exactly, so W = 0 and the gradient is 0) this, not the gradient's own size, is the scale of its rounding
    error."""
    n = x.shape[0]
    e, dx, qx, _ = differences(x, c)
    s = sign_of(e) if signs is None else signs.double()
    npix = e.shape[1]
    t = qx * (s * dx).sum(dim=1)
    a = (s.abs() + t.abs()[:, None, :]) * qx[:, None, :]
    w = (a + a.transpose(1, 2)) * (1.0 - torch.eye(npix, dtype=e.dtype))
    u, xh = inv_norms(x), unit(x).abs()
    dxh = abs(g * weight / (n * npix)) * torch.bmm(w, xh)
    return float((u[..., None] * (dxh + xh * (xh * dxh).sum(dim=2, keepdim=True))).max())


def grad_error(got, x, c, weight=1.0, g=1.0, signs=None):
    """rel_inf of `got` against the float64 analytic gradient at `signs`; where that gradient is exactly 0
    (the two degenerate cases), max |got| over grad_term_scale, and 0 for an all-zero `got`."""
    ref = grad(x, c, weight, g, signs=signs)
    if float(ref.abs().max()) > 0:
        return rel_inf(got, ref)
    worst = float(got.double().abs().max())
    scale = grad_term_scale(x, c, weight, g, signs)
    return 0.0 if worst == 0.0 else worst / scale if scale > 0 else float("inf")


def unpack_planes(pos, neg, npix):
    """s [n, N, N] float64 (+1 / -1 / 0) from the int64 planes [n, N, ceil(N / 64)], with every bit past N
    returned too: (s, stray) where stray counts the set bits at or past column N."""
    def bits(p):
        p = p.cpu()
        k = torch.arange(64, dtype=torch.int64)
        return ((p[..., None] >> k) & 1).reshape(p.shape[0], p.shape[1], -1)
    bp, bn = bits(pos), bits(neg)
    stray = int(bp[..., npix:].sum() + bn[..., npix:].sum())
    return (bp[..., :npix] - bn[..., :npix]).double(), stray


# ---- the checks of the bars ---------------------------------------------------------------------------

def sign_margin(qx, qc):
    """[n, 1, N]: inside it two values each computed from distances within OP_TOL of the truth may differ in sign."""
    return 2 * OP_TOL * (qx + qc)[:, None, :]


def near_tie_fraction(x, c):
    """The share of off-diagonal pairs whose float64 |e| lies inside the sign margin."""
    e, _, qx, qc = differences(x, c)
    npix = e.shape[1]
    if npix < 2:
        return 0.0
    off = ~torch.eye(npix, dtype=torch.bool)
    return float((e.abs() <= sign_margin(qx, qc))[:, off].double().mean())


def check_signs(s, x, c):
    """(mismatches against the float64 signs, how many of them lie outside the sign margin)."""
    e, _, qx, qc = differences(x, c)
    bad = s.double() != sign_of(e)
    return int(bad.sum()), int((bad & (e.abs() > sign_margin(qx, qc))).sum())
