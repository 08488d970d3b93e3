"""CPU restatement of the whitening and colouring transform (include/ast_hip.h, csrc/wct.hip).

Definition. content x [n, C, hc, wc], style s [ns, C, hs, ws], ns in {n, 1}; per sample, the map viewed
as C x M (M >= 2):
    mu    = per-channel mean
    Sigma = (X - mu)(X - mu)^T / (M - 1) + eps I,   eps = eps_rel * max(tr / C, 1e-20),
            tr the trace of the unregularised covariance (two-pass centring)
    T     = Sigma_s^(1/2) Sigma_c^(-1/2)   (symmetric roots)
    t     = T (x - mu_c) + mu_s,           out = alpha t + (1 - alpha) x

Two implementations:
  * wct(...)           float64, roots by torch.linalg.eigh: the reference;
  * wct_emulated(...)  float32 torch matmuls running exactly the library's coupled Newton-Schulz
                       iteration  A = Sigma / ||Sigma||_F, Y0 = A, Z0 = I, P = 1.5 I - 0.5 Z Y,
                       Y <- Y P, Z <- P Z,  Sigma^(1/2) = Y sqrt(||Sigma||_F), Sigma^(-1/2) = Z / sqrt(||Sigma||_F)
                       for a fixed count. Its distance from the reference, e_cpu, is what the method
                       costs in fp32 on a given input; the GPU bars are multiples of it.
The mean is x0 + mean(x - x0) with x0 the plane's first element, in both: a constant plane then has
exactly its value as mean, a zero trace and eps = eps_rel * 1e-20.
"""
import math

import torch

TRACE_FLOOR = 1e-20
OP_TOL = 2e-5          # the single-op bar of test_gpu_parity.py / test_gpu_efdm.py
FP32_BAR = 1e-3        # README: fp32 paths against the float64 oracle
E_CPU_MAX = 2.5e-4     # the emulation's own error on every named case: 4 * e_cpu stays under FP32_BAR

# name -> (n, ns, C, (hc, wc), (hs, ws)): the smallest shapes at which the kernels can still go wrong
CASES = {
    "c8_odd_planes": (1, 1, 8, (5, 7), (6, 6)),            # C below one MFMA tile; odd M, unaligned planes
    "c48_k_tails": (2, 2, 48, (9, 11), (7, 13)),           # C no multiple of 32; K tails of the split covariance
    "c64_shared_style": (2, 1, 64, (8, 12), (10, 8)),      # ns = 1: zero batch stride
    "c32_rank_deficient": (1, 1, 32, (4, 5), (5, 7)),      # Mc < C: the ridge carries the content covariance
    "c160_tile_tails": (1, 1, 160, (16, 16), (16, 16)),    # several tiles per side with a tail
    "c512_model": (1, 1, 512, (16, 16), (16, 16)),         # the model's C
}


def default_iters(c, eps_rel=1e-3):
    return math.ceil(math.log(c / eps_rel) / math.log(2.25)) + 5


def features(seed, shape):
    """Feature maps like a ReLU layer's: ReLU of a rank-max(C/8, 2) mixture of Gaussian sources plus a
    per-channel offset; every fifth channel (0, 5, 10, ...) is dead (all zero). float32 [n, C, h, w]."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    r = max(c // 8, 2)
    mix = torch.randn(c, r, generator=g, dtype=torch.float64) / math.sqrt(r)
    off = 0.5 * torch.randn(c, 1, generator=g, dtype=torch.float64)
    src = torch.randn(n, r, h * w, generator=g, dtype=torch.float64)
    x = torch.relu(mix @ src + off)
    x[:, ::5] = 0.0
    return x.reshape(n, c, h, w).float()


def case_inputs(name):
    n, ns, c, (hc, wc), (hs, ws) = CASES[name]
    seed = 7000 + 10 * list(CASES).index(name)
    return features(seed, (n, c, hc, wc)), features(seed + 1, (ns, c, hs, ws))


def rel_inf(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def mean_cov(x, eps_rel, dtype=torch.float64):
    """(mean [n, C], cov [n, C, C] with the ridge, eps [n]) of x [n, C, ...] in `dtype`."""
    n, c = x.shape[:2]
    v = x.reshape(n, c, -1).to(dtype)
    m = v.shape[2]
    x0 = v[:, :, :1]
    mu = x0 + (v - x0).mean(dim=2, keepdim=True)
    d = v - mu
    cov = d @ d.transpose(1, 2) / (m - 1)
    tr = cov.diagonal(dim1=1, dim2=2).sum(dim=1)
    eps = eps_rel * torch.clamp(tr / c, min=TRACE_FLOOR)
    return mu[:, :, 0], cov + eps[:, None, None] * torch.eye(c, dtype=dtype), eps


def eigh_roots(cov):
    """(cov^(1/2), cov^(-1/2)), symmetric, by eigendecomposition (float64)."""
    w, v = torch.linalg.eigh(cov.double())
    return (v * w.sqrt()[..., None, :]) @ v.transpose(-1, -2), (v / w.sqrt()[..., None, :]) @ v.transpose(-1, -2)


def frobenius(cov):
    """||cov||_F per matrix as max|c| * sqrt(sum (c / max|c|)^2): safe for a 1e-23 ridge in fp32."""
    m = cov.abs().amax(dim=(-1, -2), keepdim=True)
    return (m * ((cov / m) ** 2).sum(dim=(-1, -2), keepdim=True).sqrt())


def newton_schulz_roots(cov, iters):
    """The library's iteration in cov's dtype (float32: the emulation)."""
    c = cov.shape[-1]
    eye = torch.eye(c, dtype=cov.dtype)
    nrm = frobenius(cov)
    y, z = cov / nrm, eye.expand_as(cov).clone()
    for _ in range(iters):
        p = 1.5 * eye - 0.5 * (z @ y)
        y, z = y @ p, p @ z
    return y * nrm.sqrt(), z / nrm.sqrt()


def _apply(x, s_root, c_iroot, mu_c, mu_s, alpha):
    n, c = x.shape[:2]
    v = x.reshape(n, c, -1).to(s_root.dtype)
    t = (s_root @ c_iroot) @ (v - mu_c[:, :, None]) + mu_s[:, :, None]
    return (alpha * t + (1.0 - alpha) * v).reshape(x.shape)


def wct(content, style, alpha=1.0, eps_rel=1e-3):
    """The float64 reference (eps_rel is not range-checked here)."""
    mu_c, cov_c, _ = mean_cov(content, eps_rel)
    mu_s, cov_s, _ = mean_cov(style, eps_rel)
    return _apply(content, eigh_roots(cov_s)[0], eigh_roots(cov_c)[1], mu_c, mu_s, alpha)


def wct_emulated(content, style, alpha=1.0, eps_rel=1e-3, iters=0):
    """float32 throughout, roots by the Newton-Schulz iteration: what the library computes, up to the
    order of its sums."""
    iters = iters or default_iters(content.shape[1], eps_rel)
    mu_c, cov_c, _ = mean_cov(content, eps_rel, torch.float32)
    mu_s, cov_s, _ = mean_cov(style, eps_rel, torch.float32)
    return _apply(content, newton_schulz_roots(cov_s, iters)[0], newton_schulz_roots(cov_c, iters)[1], mu_c, mu_s,
                  float(alpha))


def root_errors(cov, root, iroot):
    """(rel_inf of Y Y against cov, rel_inf of Z cov Z against I), evaluated in float64."""
    s, y, z = cov.double(), root.double(), iroot.double()
    eye = torch.eye(s.shape[-1], dtype=torch.float64).expand_as(s)
    return rel_inf(y @ y, s), rel_inf(z @ s @ z, eye)
