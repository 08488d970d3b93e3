"""CPU restatement of the moment-matching style loss (include/ast_hip.h, csrc/moment.hip): the l_m of
STROTSS (Kolkin et al., CVPR 2019), its `moment_loss`.

Definition. x [N, C, H, W] is the stylised map, the differentiable side, M = H W; y [Ns, C, Hs, Ws] the
style map, Ns = N, or 1 for a style shared by the batch, P = Hs Ws, of any size. Per sample b:
    mu_x = mean over the pixels;  Cov_x = (X - mu_x)(X - mu_x)^T / (M - 1), with no ridge; likewise for y
    L_b = (1 / C) sum_c |mu_x - mu_y|_c + (1 / C^2) sum_ij |Cov_x - Cov_y|_ij
    L = weight / N * sum_b L_b
    gradient, to x only (the target is detached), with g the upstream scalar, s_mu = sign(mu_x - mu_y),
    S = sign(Cov_x - Cov_y), sign(0) = 0:
          dL/dX[b, c, m] = g weight / N (s_mu[c] / (C M) + 2 / (C^2 (M - 1)) sum_k S[c, k] (X[k, m] - mu_x[k]))
    (S is symmetric; the centring projection drops out because the rows of X - mu_x sum to zero).

`dtype=torch.float64` is the reference. `gradient` takes optional signs, so that it can be evaluated at
given ones: the loss is not differentiable where a difference is zero, and an entry whose difference is
below the arithmetic's resolution may get either sign; the gradient is then checked at the signs the
kernel chose and the signs themselves wherever the difference is resolved.

Bars (all from the project, none from the code under test). OP_TOL = 2e-5 is the single-op bar of
swap_ref.py, remd_ref.py and wct_ref.py for an fp32-MFMA reduction against float64.
    statistics  |Cov - Cov64| <= OP_TOL max|Cov64|, |mu - mu64| <= OP_TOL max|mu64|
    loss        relative error <= OP_TOL (a sum of absolute values: no cancellation)
    signs       sign_cov equals sign64 wherever |Cov_x - Cov_y| > OP_TOL max(max|Cov_x|, max|Cov_y|): two
                covariances each within the statistics bar move their difference by at most that much in
                each direction, so beyond it the sign is decided; sign_mu likewise with the means
    inputs      in the float64 reference alone: the entries inside that margin are at most
                UNRESOLVED_MAX = 0.5 % of C^2 per case (a condition on the seeds, checked by the CPU test)
    gradient    rel_inf <= OP_TOL against the float64 analytic gradient at the kernel's own signs
"""
import torch

from swap_ref import OP_TOL, features, rel_inf  # noqa: F401  (re-exported)

UNRESOLVED_MAX = 0.005

# name -> (n, ns, C, (H, W), (Hs, Ws)): the smallest shapes at which the kernel can still go wrong
CASES = {
    "c160_tails": (2, 2, 160, (13, 11), (9, 15)),         # channel and pixel tails; three tile rows
    "c512_shared_style": (2, 1, 512, (8, 8), (8, 8)),     # ns = 1; the model's C, 36 tile pairs
    "c64_pixel_splits": (1, 1, 64, (64, 64), (32, 32)),   # the library splits the pixels 8 ways
    "c96_two_pixels": (3, 1, 96, (1, 2), (5, 7)),         # M = 2: the smallest map
    "c40_constant_channel": (2, 2, 40, (6, 7), (5, 5)),   # channel 3 of x constant: zero variance
    "c1_single_channel": (2, 1, 1, (4, 5), (3, 3)),       # C = 1
}


def case_inputs(name):
    """(x, y) of a named case: ReLU of a normal draw, fixed seeds."""
    n, ns, c, (h, w), (hs, ws) = CASES[name]
    seed = 15000 + 10 * list(CASES).index(name)
    x, y = features(seed, (n, c, h, w)), features(seed + 1, (ns, c, hs, ws))
    if name == "c40_constant_channel":
        x[:, 3] = 0.75        # constant in x: its covariance row and column are exactly 0
        x[0, 5] = 0.0         # a dead channel in one sample only
    return x, y


def stats(y, dtype=torch.float64):
    """(mean [N, C], cov [N, C, C]) over the pixels, unbiased, no ridge."""
    v = y.to(dtype).flatten(2)
    mean = v.mean(dim=2)
    d = v - mean[:, :, None]
    return mean, d @ d.transpose(1, 2) / (v.shape[2] - 1)


def sample_terms(x, y_mean, y_cov, dtype=torch.float64):
    """L_b [N]."""
    mean, cov = stats(x, dtype)
    return (mean - y_mean.to(dtype)).abs().mean(dim=1) + (cov - y_cov.to(dtype)).abs().mean(dim=(1, 2))


def loss(x, y, weight=1.0, dtype=torch.float64):
    """The loss from the two maps (the PyTorch formulation: mean, bmm, abs().mean())."""
    y_mean, y_cov = stats(y.detach(), dtype)
    return weight * sample_terms(x, y_mean, y_cov, dtype).mean()


def signs(x, y_mean, y_cov, dtype=torch.float64):
    """(sign_mu [N, C], sign_cov [N, C, C]) as int8, sign(0) = 0."""
    mean, cov = stats(x, dtype)
    return (torch.sign(mean - y_mean.to(dtype)).to(torch.int8), torch.sign(cov - y_cov.to(dtype)).to(torch.int8))


def gradient(x, y_mean, y_cov, weight=1.0, g=1.0, sign_mu=None, sign_cov=None, dtype=torch.float64):
    """The analytic dL/dx [N, C, H, W], at the given signs when passed, else at the reference's own."""
    n, c = x.shape[:2]
    v = x.to(dtype).flatten(2)
    m = v.shape[2]
    if sign_mu is None or sign_cov is None:
        sign_mu, sign_cov = signs(x, y_mean, y_cov, dtype)
    centred = v - v.mean(dim=2, keepdim=True)
    dx = sign_mu.to(dtype)[:, :, None] / (c * m) + 2.0 / (c * c * (m - 1)) * (sign_cov.to(dtype) @ centred)
    return (g * weight / n * dx).reshape(x.shape)


def resolved(cov_x, cov_y):
    """Mask [N, C, C] of the entries whose sign is decided: |Cov_x - Cov_y| > OP_TOL max(|Cov_x|, |Cov_y|)."""
    scale = max(float(cov_x.abs().max()), float(cov_y.abs().max()))
    return (cov_x - cov_y).abs() > OP_TOL * scale


def resolved_mu(mu_x, mu_y):
    scale = max(float(mu_x.abs().max()), float(mu_y.abs().max()))
    return (mu_x - mu_y).abs() > OP_TOL * scale
