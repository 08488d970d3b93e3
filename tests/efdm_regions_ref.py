"""CPU restatement of regional exact feature distribution matching (include/ast_hip.h,
csrc/efdm_regions.hip) in plain torch, on tests/efdm_ref.py: the reference side of
tests/test_efdm_regions_cpu.py and tests/test_gpu_efdm_regions.py.

Definition. content c [n, C, h, w]; labels uint8 [n, h, w] (label k < K: region k; any label >= K, 255 by
convention: pass-through); styles [S, C, hs, ws] shared by the batch, optionally with style_labels
[S, hs, ws]; mix [n or 1, K, S], non-negative. Order and keys are those of efdm_ref (totalOrder of the
bits, ties in index order). For sample b, channel ch and region k:
    I_k, Mc_k       the pixels with labels[b] == k and their number; r(i) the stable rank of i among I_k
    J_sk, Ms_sk     all pixels of style s, or (style_labels) those with style_labels[s] == k
    S_sk            the values of plane (s, ch) on J_sk, ascending
    t_s[i]          S_sk[((2 r(i) + 1) * Ms_sk) // (2 * Mc_k)]
    t[i]            sum_s mix[b, k, s] * t_s[i] in ascending s, weights of exactly 0 skipped; with exactly
                    one non-zero weight t = t_s in bits (no multiply)
    out[i]          t[i] at alpha == 1, else c[i] + alpha * (t[i] - c[i])
    pass-through    out = c in bits where label >= K, and in a region one of whose used styles has
                    Ms_sk == 0
The restatement works region by region with boolean masks and one sort per region (deliberately not the
library's one sort per plane and label scan). dtype float32 reproduces the library's arithmetic (fp32
products, fp32 sums, nothing fused); float64 is the reference of the mixes and blends."""
import torch

import efdm_ref as ER
from wct_regions_ref import scatter_labels

PASS = 255
OP_TOL = 2e-5   # the project's single-op bar (test_gpu_efdm.py)

# name -> content shape, bank shape, K, specials, the pixel count of every region per content sample and
# per style (the rest of each map is labelled 255; the maps are random scatters of exactly these counts)
CASES = {
    # odd plane under one tile, specials planted in every plane
    "small_specials": dict(c=(2, 3, 5, 7), s=(2, 3, 5, 7), k=2, specials=True,
                           counts=[(17, 12), (20, 9)], style_counts=[(15, 14), (10, 20)]),
    # 8 wave tiles, LDS stages, the scan across waves; K not a multiple of S
    "64x64_scattered": dict(c=(2, 4, 64, 64), s=(3, 4, 64, 64), k=4, specials=False,
                            counts=[(1500, 1000, 900, 600), (2000, 700, 800, 500)],
                            style_counts=[(1100, 1000, 1000, 900), (900, 1200, 800, 1100), (1300, 700, 1100, 900)]),
    # the sizes differ, both ways
    "bigger_content": dict(c=(1, 2, 24, 40), s=(2, 2, 16, 16), k=3, specials=False,
                           counts=[(400, 300, 200)], style_counts=[(100, 80, 60), (90, 90, 70)]),
    "bigger_style": dict(c=(1, 2, 16, 16), s=(2, 2, 24, 40), k=3, specials=False,
                         counts=[(100, 80, 60)], style_counts=[(400, 300, 200), (350, 350, 200)]),
    # the 16384-element edge (LDS above 64 KB, 16 positions per thread in the scan), all 8 regions
    "at_fused_max": dict(c=(1, 2, 128, 128), s=(2, 2, 128, 128), k=8, specials=False,
                         counts=[(3000, 2500, 2200, 2000, 1900, 1800, 1500, 1400)],
                         style_counts=[(2900, 2600, 2100, 2100, 1800, 1900, 1400, 1500),
                                       (1400, 1500, 1800, 1900, 2000, 2200, 2500, 3000)]),
    # the first size past one 512-element tile
    "past_one_tile": dict(c=(1, 1, 1, 513), s=(2, 1, 1, 513), k=3, specials=False,
                          counts=[(200, 170, 130)], style_counts=[(180, 170, 150), (250, 130, 120)]),
}

# the mixes of the cases without specials that the float64 comparison runs (rows sum to 1 as written;
# a zero weight in most rows, a one-hot row among them)
MIXES = {
    "64x64_scattered": {"shared": [[.3, .7, 0], [0, .5, .5], [.2, .3, .5], [1, 0, 0]],
                        "per_sample": [[[.3, .7, 0], [0, .5, .5], [.2, .3, .5], [1, 0, 0]],
                                       [[0, 0, 1], [.6, 0, .4], [.5, .5, 0], [.1, .2, .7]]]},
    "bigger_content": {"shared": [[.25, .75], [.5, .5], [0, 1]]},
    "bigger_style": {"shared": [[.25, .75], [.5, .5], [0, 1]]},
}


def case_inputs(name):
    """(content, labels, styles, style_labels) of a named case (float32 / uint8 CPU tensors)."""
    d = CASES[name]
    seed = 5200 + 10 * list(CASES).index(name)
    content = ER.features(seed, d["c"], d["specials"])
    styles = ER.features(seed + 1, d["s"], d["specials"])
    labels = scatter_labels(seed + 2, d["c"][2:], d["counts"])
    style_labels = scatter_labels(seed + 3, d["s"][2:], d["style_counts"])
    return content, labels, styles, style_labels


def one_hot_mix(name, shift=0):
    """float32 [1, K, S]: region k takes style (k + shift) % S."""
    k, s = CASES[name]["k"], CASES[name]["s"][0]
    m = torch.zeros(1, k, s)
    for r in range(k):
        m[0, r, (r + shift) % s] = 1.0
    return m


def case_mix(name, variant):
    """The named mix as float32 [1 or n, K, S]."""
    m = torch.tensor(MIXES[name][variant], dtype=torch.float32)
    return m.unsqueeze(0) if m.dim() == 2 else m


def region_index(labels, b, k):
    """The pixel indices of region k of map b, ascending."""
    return torch.nonzero(labels[b].reshape(-1) == k).reshape(-1)


def region_sort(x, labels, regions):
    """The bank: (sorted [S, C, M] float32 in the order (min(label, K), key, index), count [S, K] int32).
    labels None: one region holds everything."""
    s, c = x.shape[:2]
    flat = x.reshape(s, c, -1)
    m = flat.shape[2]
    if labels is None:
        count = torch.zeros((s, regions), dtype=torch.int32)
        count[:, 0] = m
        return ER.plane_sort(flat.reshape(s * c, m))[0].reshape(s, c, m), count
    cls = labels.reshape(s, m).to(torch.int64).clamp_max(regions)
    count = torch.stack([(cls == k).sum(dim=1) for k in range(regions)], dim=1).to(torch.int32)
    by_key = torch.sort(ER.keys(flat), dim=2, stable=True).indices                      # [S, C, M]
    by_cls = torch.sort(torch.gather(cls[:, None].expand(s, c, m), 2, by_key), dim=2, stable=True).indices
    order = torch.gather(by_key, 2, by_cls)
    return torch.gather(flat.contiguous().view(torch.int32), 2, order).view(torch.float32), count


def efdm_regions(content, labels, styles, mix, style_labels=None, alpha=1.0, dtype=torch.float64):
    """(out, valid [n, K] bool). out is in `dtype`; where it is a copy (pass-through, or a one-hot row at
    alpha == 1) it holds the float32 value exactly. valid[b, k]: region k of sample b is matched (every
    used style has pixels of region k); an empty content region counts as matched."""
    n, c = content.shape[:2]
    k_regions, s_styles = int(mix.shape[1]), int(mix.shape[2])
    x = content.reshape(n, c, -1)
    sv = styles.reshape(s_styles, c, -1)
    out = x.to(dtype).clone()
    valid = torch.zeros((n, k_regions), dtype=torch.bool)
    sorted_style = {}

    def style_values(s, k):   # S_sk [C, Ms_sk] float32, ascending
        key = (s, k if style_labels is not None else -1)
        if key not in sorted_style:
            plane = sv[s] if style_labels is None else sv[s][:, style_labels[s].reshape(-1) == k]
            sorted_style[key] = ER.plane_sort(plane)[0] if plane.shape[1] else plane
        return sorted_style[key]

    for b in range(n):
        w_b = mix[b if mix.shape[0] > 1 else 0]
        for k in range(k_regions):
            idx = region_index(labels, b, k)
            used = [s for s in range(s_styles) if float(w_b[k, s]) != 0.0]
            banks = [style_values(s, k) for s in used]
            if any(sk.shape[1] == 0 for sk in banks):
                continue
            valid[b, k] = True
            mk = idx.numel()
            if mk == 0:
                continue
            xk = x[b][:, idx].contiguous()                                              # [C, Mc_k]
            order = torch.sort(ER.keys(xk), dim=1, stable=True).indices                 # order[ch, r] = element of rank r
            rank = torch.empty_like(order)
            rank.scatter_(1, order, torch.arange(mk).expand(c, -1).contiguous())
            t = torch.zeros((c, mk), dtype=dtype)
            for j, (s, sk) in enumerate(zip(used, banks)):
                t_s = torch.gather(sk[:, ER.rank_map(mk, sk.shape[1])], 1, rank)        # float32, copies
                if len(used) == 1:
                    t = t_s.to(dtype)
                elif j == 0:
                    t = w_b[k, s].to(dtype) * t_s.to(dtype)
                else:
                    t = t + w_b[k, s].to(dtype) * t_s.to(dtype)
            xk = xk.to(dtype)
            out[b][:, idx] = t if alpha == 1.0 else xk + alpha * (t - xk)
    return out.reshape(content.shape), valid


def brute_force(content, labels, styles, mix, style_labels=None):
    """The definition word for word at alpha == 1, O(M^2) per plane, in Python floats (float64): the rank
    is the number of (key_j, j) < (key_i, i) over the pixels j of i's own region. Pass-through pixels keep
    the content's value."""
    n, c = content.shape[:2]
    k_regions, s_styles = int(mix.shape[1]), int(mix.shape[2])
    out = content.double().clone()
    for b in range(n):
        lab = labels[b].reshape(-1).tolist()
        w_b = mix[b if mix.shape[0] > 1 else 0].double().tolist()
        for ch in range(c):
            xs = content[b, ch].reshape(-1)
            kc = ER.keys(xs).tolist()
            o = out[b, ch].view(-1)
            for k in range(k_regions):
                region = [i for i in range(len(lab)) if lab[i] == k]
                used = [s for s in range(s_styles) if w_b[k][s] != 0.0]
                banks = []
                for s in used:
                    sp = styles[s, ch].reshape(-1)
                    sl = None if style_labels is None else style_labels[s].reshape(-1).tolist()
                    ks, vs = ER.keys(sp).tolist(), sp.tolist()
                    js = [j for j in range(len(vs)) if sl is None or sl[j] == k]
                    banks.append([vs[j] for j in sorted(js, key=lambda j: (ks[j], j))])
                if any(len(bk) == 0 for bk in banks):
                    continue
                for i in region:
                    r = sum(1 for j in region if (kc[j], j) < (kc[i], i))
                    ts = [bk[((2 * r + 1) * len(bk)) // (2 * len(region))] for bk in banks]
                    if len(used) == 1:
                        o[i] = ts[0]
                    else:
                        t = w_b[k][used[0]] * ts[0]
                        for s, v in zip(used[1:], ts[1:]):
                            t = t + w_b[k][s] * v
                        o[i] = t
    return out


def passthrough_mask(labels, valid):
    """bool [n, h, w]: the pixels that must equal the content in bits."""
    m = torch.ones(labels.shape, dtype=torch.bool)
    for b in range(labels.shape[0]):
        for k in range(valid.shape[1]):
            if valid[b, k]:
                m[b] &= labels[b] != k
    return m
