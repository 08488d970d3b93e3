"""CPU restatement of the feature k-means and the label mode filter (include/ast_hip.h, csrc/kmeans.hip).

Definition. A bank is x [B, C, H, W]; point g = b HW + p is the C-vector at pixel p of map b and all
B HW points are clustered together. Centroids are c [K, C], 1 <= K <= 8.
    d(g, k)   = sum over channels of (x - c)^2
    assign    label(g) = the k of least d, the lowest k on equal distances; a distance replaces the
                running (+inf, 255) only when strictly smaller, so a NaN never wins and a point
                without a winner gets 255 and belongs to no cluster
    update    c_k = (sum of the points labelled k) / count_k; a cluster of count 0 keeps its centroid
    seed      "maximin": m = the mean of all points; seed 0 = the g of largest d(g, m); seed j = the g
                of largest dmin(g) = min over the earlier seeds of d(g, seed); ties to the lowest g
    lloyd     centroids = the points at the seeds (or `init`); `iters` rounds of assign, update; one
                final assign: the returned labels and counts belong to the returned centroids
    mode      `passes` rounds of a 3x3 majority vote over a uint8 map, the window clipped at the
                borders: only labels < K vote, the most frequent wins; on a tie the centre's own label
                if it is among the tied, else the lowest; a centre >= K passes through
The implementation here is the matrix form, deliberately not the kernel's tile form: the points as a
[P, C] matrix, distances by broadcasting, sums by index_add_. `dtype=torch.float64` is the reference,
`dtype=torch.float32` the emulation (the same computation in fp32).

Bars (all from the project, none from the code under test). OP_TOL = 2e-5 is the single-op bar of
swap_ref.py / wct_ref.py; NEAR_TIE_MAX = 2 % that of swap_ref.py. E = max_g ||x_g||^2 + max_k ||c_k||^2
bounds every distance of a case (d <= 2 E), so it is the scale of a distance's error.
    assign  d64(g, label(g)) <= min_k d64(g, k) + 2 OP_TOL E for every point: two distances each within
            OP_TOL E of the truth can swap order only inside that margin
    inputs  in the float64 reference alone, at most NEAR_TIE_MAX of a case's points may have a
            runner-up inside that margin (asserted in test_kmeans_cpu.py; the worst random case here
            is c64_tiles with 0.19 %, the others have none)
    update  given labels, against float64 from the same labels: rel_inf <= OP_TOL, counts exact
    seed    conditioned on the earlier seeds, dmin64(returned seed) >= max_g dmin64(g) - 2 OP_TOL E
    lloyd   on the planted inputs (K Gaussian centres 4 randn(K, C) plus unit noise, in uneven stripes)
            the clusters are far apart against the noise: in float64 the runner-up's distance exceeds
            the winner's by at least PLANTED_MARGIN * max ||x||^2 in every round of every case (the
            least here is 0.74, case c20_k3), four orders of magnitude above OP_TOL, so fp32 labels
            must equal the float64 ones exactly, and the centroids then agree to OP_TOL
    mode    exact
"""
import torch

OP_TOL = 2e-5
NEAR_TIE_MAX = 0.02
PLANTED_MARGIN = 0.38    # asserted in test_kmeans_cpu.py, which prints the least over the cases and rounds

# name -> (B, C, (H, W), K): the smallest shapes at which the kernel can still go wrong
CASES = {
    "c8_one_pixel": (1, 8, (1, 1), 1),        # one pixel, one cluster
    "c20_k3": (1, 20, (7, 9), 3),             # C tail, 63 points
    "c24_k2": (2, 24, (5, 13), 2),
    "c48_k8": (3, 48, (9, 10), 8),            # three maps, a tile tail per map
    "c130_k7": (1, 130, (8, 9), 7),
    "c64_tiles": (2, 64, (40, 40), 5),        # 3200 points: many tiles, more than one level of partials
    "c512_k8": (1, 512, (12, 12), 8),         # the model's C
}
# one more: at C = 1024 the kernel's tile has 16 pixels for every K (at C = 512 for K > 4 only)
EXTRA_CASES = {
    "c1024_narrow_tile": (1, 1024, (5, 9), 8),
}
ALL_CASES = {**CASES, **EXTRA_CASES}


def features(seed, shape):
    """relu(randn): float32, as swap_ref.features."""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(*shape, generator=g, dtype=torch.float64)).float()


def case_inputs(name):
    """(x [B, C, H, W], centroids [K, C]) of a named case, both relu(randn)."""
    b, c, (h, w), k = ALL_CASES[name]
    seed = 12000 + 10 * list(ALL_CASES).index(name)
    return features(seed, (b, c, h, w)), features(seed + 1, (k, c))


def planted_inputs(name):
    """(x [B, C, H, W], planted labels uint8 [B, H, W]) of a named case: K Gaussian centres
    4 randn(K, C) plus unit noise; cluster j takes a run of consecutive points g whose length is
    proportional to j + 1 (at least one point), so the stripes are uneven and cross map borders."""
    b, c, (h, w), k = ALL_CASES[name]
    g = torch.Generator().manual_seed(12500 + 10 * list(ALL_CASES).index(name))
    p = b * h * w
    centres = 4.0 * torch.randn(k, c, generator=g, dtype=torch.float64)
    edges = [0]
    tot = k * (k + 1) // 2
    for j in range(k):
        edges.append(max(edges[-1] + 1, round(p * ((j + 1) * (j + 2) // 2) / tot)))
    edges[-1] = p
    lab = torch.zeros(p, dtype=torch.long)
    for j in range(k):
        lab[edges[j]:edges[j + 1]] = j
    pts = centres[lab] + torch.randn(p, c, generator=g, dtype=torch.float64)
    return from_points(pts.float(), b, h, w), lab.to(torch.uint8).reshape(b, h, w)


def rel_inf(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def points(x, dtype=torch.float64):
    """[B, C, H, W] -> [B HW, C], point g = b HW + p."""
    b, c = x.shape[:2]
    return x.to(dtype).reshape(b, c, -1).permute(0, 2, 1).reshape(-1, c)


def from_points(pts, b, h, w):
    return pts.reshape(b, h * w, -1).permute(0, 2, 1).reshape(b, -1, h, w).contiguous()


def dist(x, cen, dtype=torch.float64):
    """d(g, k) [P, K]."""
    return ((points(x, dtype)[:, None, :] - cen.to(dtype)[None]) ** 2).sum(dim=2)


def scale(x, cen):
    """E = max ||x_g||^2 + max ||c_k||^2 in float64."""
    return float((points(x) ** 2).sum(1).max() + (cen.double() ** 2).sum(1).max())


def argmin_rows(d):
    """label [P] (long, 255 where nothing wins) of distances [P, K]: the first minimum; a NaN or +inf
    never wins."""
    clean = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    lab = clean.argmin(dim=1)      # the first of equal minima
    none = torch.isinf(clean.gather(1, lab[:, None])[:, 0]) & (clean.gather(1, lab[:, None])[:, 0] > 0)
    return torch.where(none, torch.full_like(lab, 255), lab)


def assign(x, cen, dtype=torch.float64):
    """labels uint8 [B, H, W]."""
    b, _, h, w = x.shape
    return argmin_rows(dist(x, cen, dtype)).to(torch.uint8).reshape(b, h, w)


def update(x, labels, prev, dtype=torch.float64):
    """(centroids [K, C] in `dtype`, counts int32 [K]) from given labels; prev for the empty clusters."""
    k, c = prev.shape
    pts, lab = points(x, dtype), labels.reshape(-1).long()
    keep = lab < k
    sums = torch.zeros(k, c, dtype=dtype).index_add_(0, lab[keep], pts[keep])
    counts = torch.bincount(lab[keep], minlength=k)
    cen = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None].to(dtype), prev.to(dtype))
    return cen, counts.to(torch.int32)


def dmin_given(x, earlier, dtype=torch.float64):
    """dmin(g) [P] before the next seed: d(g, mean) when no seed is there yet, else the least distance
    to the points at the indices `earlier`."""
    pts = points(x, dtype)
    if len(earlier) == 0:
        return ((pts - pts.mean(dim=0, keepdim=True)) ** 2).sum(1)
    return ((pts[:, None, :] - pts[list(earlier)][None]) ** 2).sum(2).min(dim=1).values


def seed(x, k, dtype=torch.float64):
    """The k maximin seeds (a list of point indices)."""
    out = []
    for _ in range(k):
        out.append(int(dmin_given(x, out, dtype).argmax()))   # the first of equal maxima
    return out


def lloyd(x, k, iters, init=None, dtype=torch.float64, trace=None):
    """(centroids [K, C], labels uint8 [B, H, W], counts int32 [K]). `trace`, a list, receives per round
    (the final assignment included) the tuple (inertia, least runner-up margin), both float64."""
    cen = (points(x, dtype)[seed(x, k, dtype)] if init is None else init.to(dtype)).clone()
    for r in range(iters + 1):
        lab = assign(x, cen, dtype)
        if trace is not None:
            d = dist(x, cen)
            top = d.topk(min(2, k), dim=1, largest=False).values
            at = d.gather(1, lab.reshape(-1, 1).long().clamp(max=k - 1))[:, 0]
            trace.append((float(at.sum()), float((top[:, -1] - top[:, 0]).min()) if k > 1 else float("inf")))
        if r < iters:
            cen = update(x, lab, cen, dtype)[0]
    counts = torch.bincount(lab.reshape(-1).long()[lab.reshape(-1) < k], minlength=k).to(torch.int32)
    return cen, lab, counts


def mode_filter(labels, k, passes=1):
    """uint8 [N, H, W] -> the same after `passes` rounds of the 3x3 vote (plain loops: it is the definition)."""
    cur = labels.clone()
    n, h, w = cur.shape
    for _ in range(passes):
        nxt = cur.clone()
        for b in range(n):
            for y in range(h):
                for x in range(w):
                    own = int(cur[b, y, x])
                    if own >= k:
                        continue
                    votes = [0] * k
                    for yy in range(max(y - 1, 0), min(y + 2, h)):
                        for xx in range(max(x - 1, 0), min(x + 2, w)):
                            l = int(cur[b, yy, xx])
                            if l < k:
                                votes[l] += 1
                    top = max(votes)
                    nxt[b, y, x] = own if votes[own] == top else votes.index(top)
        cur = nxt
    return cur


def label_maps(seed_, shape, k, holes=True):
    """Random uint8 maps with labels 0..k-1 and, with `holes`, a few 255."""
    g = torch.Generator().manual_seed(seed_)
    m = torch.randint(0, k, shape, generator=g, dtype=torch.int64)
    if holes:
        m = torch.where(torch.rand(shape, generator=g) < 0.1, torch.full_like(m, 255), m)
    return m.to(torch.uint8)


# ---- the checks of the bars ---------------------------------------------------------------------------

def near_tie_fraction(x, cen):
    """The share of points whose runner-up lies within 2 OP_TOL E of the winner (float64 alone)."""
    if cen.shape[0] < 2:
        return 0.0
    top = dist(x, cen).topk(2, dim=1, largest=False).values
    return float(((top[:, 1] - top[:, 0]) <= 2 * OP_TOL * scale(x, cen)).double().mean())


def check_assign(labels, x, cen):
    """(worst shortfall / E, number of labels equal to the float64 argmin, points) of labels against the
    float64 distances: the assign bar asks the first <= 2 OP_TOL."""
    d = dist(x, cen)
    lab = labels.reshape(-1).long()
    assert int(lab.max()) < cen.shape[0], "a finite point got no cluster"
    at = d.gather(1, lab[:, None])[:, 0]
    short = float((at - d.min(dim=1).values).max()) / scale(x, cen)
    return short, int((lab == argmin_rows(d)).sum()), lab.numel()


def check_seeds(seeds, x):
    """The worst, over the steps, of (max dmin64 - dmin64(seed_j)) / E, each step conditioned on the given
    earlier seeds; E = 2 max ||x||^2 (a seed is a point, the mean lies inside their hull)."""
    e = 2.0 * float((points(x) ** 2).sum(1).max())
    worst = 0.0
    for j, s in enumerate(seeds):
        dm = dmin_given(x, [int(v) for v in seeds[:j]])
        worst = max(worst, float(dm.max() - dm[int(s)]) / e)
    return worst
