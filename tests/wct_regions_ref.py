"""CPU restatement of the regional whitening and colouring transform (include/ast_hip.h, csrc/wct.hip).

Definition. content x [n, C, h, w]; labels uint8 [n, h, w] (label k < K: region k; any label >= K, 255
by convention: pass-through, in no statistic); styles s [S, C, hs, ws] shared by the batch, optionally
with style_labels [S, hs, ws]; mix [n or 1, K, S], non-negative, rows summing to 1.
    region (b, k)   the M_k pixels labelled k, in ascending pixel index, as a C x M_k map; mu and Sigma
                    are wct_ref.mean_cov of that map; M_k < 2: the region is invalid
    style side      wct_ref.mean_cov of the whole style map, or (style_labels) of style s's own region k
    U_k             the styles with mix[b, k, s] != 0 (the others are never read)
    C_k, m_k        sum over U_k, ascending s, of w_s Sigma_s^(1/2) and of w_s mu_s
    T_k             C_k Sigma_(c,k)^(-1/2);   t = T_k (x - mu_(c,k)) + m_k;   out = alpha t + (1 - alpha) x
    pass-through    out = x where label >= K, in an invalid content region, and in a region one of
                    whose used styles has an invalid region k
Two implementations, region by region with boolean masks (deliberately not the library's binned form):
  * wct_regions(...)           float64, roots by eigendecomposition: the reference;
  * wct_regions_emulated(...)  float32, roots by wct_ref.newton_schulz_roots: what the library computes up
                               to the order of its sums; its distance from the reference is e_cpu.
"""
import torch

import wct_ref as WR

PASS = 255

# name -> n, C, (h, w), K, S, (hs, ws), the pixel count of every region per content sample (the rest of
# the plane is labelled 255), the same per style (None: no style labels), and the named mixes. The
# smallest shapes at which the kernels can still go wrong; the label maps are random scatters of exactly
# these counts, so no region is a band or a box.
CASES = {
    # C below one tile, odd plane, both regions under one 32-pixel K chunk
    "c8_odd_planes": dict(n=1, c=8, hw=(5, 7), k=2, s=2, shw=(6, 6), counts=[(19, 11)], style_counts=None,
                          mixes={"eye": [[1, 0], [0, 1]], "blend": [[.25, .75], [.5, .5]]}),
    # maps differ per sample; no region size is a multiple of 32; region 0 spans two covariance splits
    # (M_k > 64), regions 1 and 2 one
    "c48_two_splits": dict(n=2, c=48, hw=(9, 11), k=3, s=3, shw=(7, 13), counts=[(67, 17, 9), (70, 13, 11)],
                           style_counts=None, mixes={"eye": [[1, 0, 0], [0, 1, 0], [0, 0, 1]]}),
    # a zero weight in every row; shared and per-sample mixes
    "c64_mixes": dict(n=2, c=64, hw=(8, 12), k=2, s=3, shw=(10, 8), counts=[(50, 39), (45, 44)], style_counts=None,
                      mixes={"shared": [[.3, .7, 0], [0, .5, .5]],
                             "per_sample": [[[.3, .7, 0], [0, .5, .5]], [[1, 0, 0], [.2, .3, .5]]]}),
    # M_k < C (the ridge carries the covariance), an empty region and a one-pixel region
    "c32_small_regions": dict(n=1, c=32, hw=(4, 5), k=3, s=3, shw=(5, 7), counts=[(14, 0, 1)], style_counts=None,
                              mixes={"eye": [[1, 0, 0], [0, 1, 0], [0, 0, 1]]}),
    # style labels; style 1 lacks region 1: unused there ("absent_unused", region 1 is transformed) or used
    # ("absent_used", region 1 passes through)
    "c160_style_labels": dict(n=1, c=160, hw=(16, 16), k=2, s=2, shw=(16, 16), counts=[(140, 100)],
                              style_counts=[(120, 110), (230, 0)],
                              mixes={"absent_unused": [[.5, .5], [1, 0]], "absent_used": [[.5, .5], [.6, .4]]}),
    # the model's C
    "c512_model": dict(n=1, c=512, hw=(16, 16), k=2, s=2, shw=(16, 16), counts=[(150, 90)], style_counts=None,
                       mixes={"blend": [[1, 0], [.25, .75]]}),
}


def scatter_labels(seed, hw, counts):
    """uint8 [len(counts), h, w]: map i has exactly counts[i][k] pixels labelled k, scattered at random, and
    255 elsewhere (every case leaves some)."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    out = torch.full((len(counts), h * w), PASS, dtype=torch.uint8)
    for i, cnt in enumerate(counts):
        assert sum(cnt) < h * w
        order = torch.randperm(h * w, generator=g)
        pos = 0
        for k, m in enumerate(cnt):
            out[i, order[pos:pos + m]] = k
            pos += m
    return out.reshape(len(counts), h, w)


def case_inputs(name):
    """(content, labels, styles, style_labels or None) of a named case."""
    d = CASES[name]
    seed = 9000 + 10 * list(CASES).index(name)
    content = WR.features(seed, (d["n"], d["c"]) + d["hw"])
    styles = WR.features(seed + 1, (d["s"], d["c"]) + d["shw"])
    labels = scatter_labels(seed + 2, d["hw"], d["counts"])
    style_labels = None if d["style_counts"] is None else scatter_labels(seed + 3, d["shw"], d["style_counts"])
    return content, labels, styles, style_labels


def case_mix(name, variant):
    """The named mix as float64 [1 or n, K, S] (rows sum to 1 as written)."""
    m = torch.tensor(CASES[name]["mixes"][variant], dtype=torch.float64)
    return m.unsqueeze(0) if m.dim() == 2 else m


def variants():
    return [(name, v) for name, d in CASES.items() for v in d["mixes"]]


def region_index(labels, b, k):
    """The pixel indices of region k of map b, ascending."""
    return torch.nonzero(labels[b].reshape(-1) == k).reshape(-1)


def _regions(content, labels, styles, mix, style_labels, alpha, eps_rel, dtype, roots):
    """out (in `dtype`) and valid [n, K] (bool). roots(cov) -> (cov^(1/2), cov^(-1/2))."""
    n, c = content.shape[:2]
    k_regions, s_styles = mix.shape[1], mix.shape[2]
    x = content.reshape(n, c, -1).to(dtype)
    sv = styles.reshape(s_styles, c, -1)
    out = x.clone()
    valid = torch.zeros((n, k_regions), dtype=torch.bool)
    style_cache = {}

    def style_stats(s, k):
        key = (s, k if style_labels is not None else -1)
        if key not in style_cache:
            if style_labels is None:
                smap = sv[s:s + 1]
            else:
                smap = sv[s:s + 1][:, :, style_labels[s].reshape(-1) == k]
            if smap.shape[2] < 2:
                style_cache[key] = None
            else:
                mu, cov, _ = WR.mean_cov(smap, eps_rel, dtype)
                style_cache[key] = (mu[0], roots(cov)[0][0].to(dtype))
        return style_cache[key]

    for b in range(n):
        w_b = mix[b if mix.shape[0] > 1 else 0]
        for k in range(k_regions):
            mask = labels[b].reshape(-1) == k
            used = [s for s in range(s_styles) if float(w_b[k, s]) != 0.0]
            if int(mask.sum()) < 2 or not used:
                continue
            stats = [style_stats(s, k) for s in used]
            if any(st is None for st in stats):
                continue
            valid[b, k] = True
            xk = x[b:b + 1][:, :, mask]
            mu_c, cov_c, _ = WR.mean_cov(xk, eps_rel, dtype)
            c_iroot = roots(cov_c)[1][0].to(dtype)
            colour = sum(w_b[k, s].to(dtype) * st[1] for s, st in zip(used, stats))
            m_k = sum(w_b[k, s].to(dtype) * st[0] for s, st in zip(used, stats))
            t = (colour @ c_iroot) @ (xk[0] - mu_c[0][:, None]) + m_k[:, None]
            out[b][:, mask] = alpha * t + (1.0 - alpha) * xk[0]
    return out.reshape(content.shape), valid


def wct_regions(content, labels, styles, mix, style_labels=None, alpha=1.0, eps_rel=1e-3):
    """The float64 reference: (out, valid [n, K])."""
    return _regions(content, labels, styles, mix, style_labels, alpha, eps_rel, torch.float64, WR.eigh_roots)


def wct_regions_emulated(content, labels, styles, mix, style_labels=None, alpha=1.0, eps_rel=1e-3, iters=0):
    """float32 throughout, roots by the library's Newton-Schulz iteration: (out, valid [n, K])."""
    iters = iters or WR.default_iters(content.shape[1], eps_rel)
    return _regions(content, labels, styles, mix, style_labels, float(alpha), eps_rel, torch.float32,
                    lambda cov: WR.newton_schulz_roots(cov, iters))


def region_errors(got, ref, labels, valid):
    """{(b, k): rel_inf over the pixels of valid region (b, k)}."""
    n, c = ref.shape[:2]
    g, r = got.reshape(n, c, -1), ref.reshape(n, c, -1)
    out = {}
    for b in range(n):
        for k in range(valid.shape[1]):
            if valid[b, k]:
                idx = region_index(labels, b, k)
                out[(b, k)] = WR.rel_inf(g[b][:, idx], r[b][:, idx])
    return out


def passthrough_mask(labels, valid):
    """bool [n, h, w]: the pixels that must equal the content in bits."""
    m = torch.ones(labels.shape, dtype=torch.bool)
    for b in range(labels.shape[0]):
        for k in range(valid.shape[1]):
            if valid[b, k]:
                m[b] &= labels[b] != k
    return m
