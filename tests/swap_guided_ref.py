"""CPU restatement of guided style swap (include/ast_hip.h, csrc/swap.hip), built on swap_ref.py.

Definition. Content key ck and content c [n, C, H, W]; a bank of S >= 1 styles, keys sk and values sv
[S, C, Hs, Ws], shared by the batch. Ns = (Hs - 2)(Ws - 2); the global style patch is
j = s Ns + jy (Ws - 2) + jx. Classes, one per patch: cc uint8 [n, H - 2, W - 2], sc uint8
[S, Hs - 2, Ws - 2]; a class >= MAX_CLASSES = 64 takes no part.
    score(i, j) = swap_ref's score of content patch i against patch j - s Ns of style s
    index(i)    = the j of maximal score among the j with sc(j) == cc(i) < 64, the lowest global j on
                  equal scores; a NaN never wins; -1 (score -inf) without an admissible candidate or
                  with none above -inf
    out[y, x]   = (1 - alpha) c[y, x] + alpha / cnt(y, x) * sum of sv[s, jy + dy, jx + dx] over the
                  covering content patches (y - dy, x - dx) whose index is >= 0, ascending (dy, dx);
                  cnt counts those; c[y, x] itself where cnt = 0. An index >= S Ns is clamped.
`dtype=torch.float64` is the reference, `dtype=torch.float32` the emulation. The masked score matrix
[n, M, S Ns] (-inf where not admissible) is what the kernel never stores and the tests compare against.

Bars: swap_ref's, unchanged -- OP_TOL, the 2 * OP_TOL * S index shortfall, GATHER_TOL, NEAR_TIE_MAX; S is
the largest winning score of a case; score error and shortfall run over the matched patches.
"""
import torch
import torch.nn.functional as F

import swap_ref as SR

MAX_CLASSES = 64
OP_TOL, GATHER_TOL, NEAR_TIE_MAX = SR.OP_TOL, SR.GATHER_TOL, SR.NEAR_TIE_MAX

# name -> (row, n, S, C, (H, W), (Hs, Ws)); inputs are SR.features(9900 + 10 * row, ...) for the content and
# 9901 + 10 * row for the bank; the classes are in case_classes
CASES = {
    "g8_one_patch": (0, 1, 1, 8, (3, 3), (3, 3)),            # degenerate sizes, one class
    "g8_no_candidate": (0, 1, 1, 8, (3, 3), (3, 3)),         # the same inputs, cc = 0 against sc = 1: -1
    "g48_bands": (1, 2, 1, 48, (9, 11), (8, 13)),            # every tile mixes classes; C no multiple of 8 * 4
    "g64_bank_by_style": (2, 1, 3, 64, (20, 23), (11, 15)),  # tile skip, a style never visited, 2 tiles + tail per style
    "g32_sky_takes_sky": (3, 2, 2, 32, (12, 13), (10, 21)),  # per-sample content classes; excluded style patches
    "g160_missing_class": (4, 1, 2, 160, (9, 8), (19, 21)),  # -1 results, the cnt = 0 gather, a one-patch class
    "g512_split_bank": (5, 1, 2, 512, (10, 10), (34, 34)),   # the model's C; the shape that makes the library split
}


def case_inputs(name):
    """(content [n, C, H, W], bank [S, C, Hs, Ws]) of a named case."""
    row, n, s, c, (hc, wc), (hs, ws) = CASES[name]
    return SR.features(9900 + 10 * row, (n, c, hc, wc)), SR.features(9901 + 10 * row, (s, c, hs, ws))


def case_classes(name):
    """(cc uint8 [n, H - 2, W - 2], sc uint8 [S, Hs - 2, Ws - 2]) of a named case."""
    _, n, s, _, (hc, wc), (hs, ws) = CASES[name]
    cc = torch.zeros(n, hc - 2, wc - 2, dtype=torch.uint8)
    sc = torch.zeros(s, hs - 2, ws - 2, dtype=torch.uint8)
    if name == "g8_no_candidate":
        sc[:] = 1
    elif name == "g48_bands":
        cc[:, 2:5], cc[:, 5:7] = 1, 2                     # content rows 0-1 / 2-4 / 5-6
        sc[:, :, 4:8], sc[:, :, 8:11] = 1, 2              # style columns 0-3 / 4-7 / 8-10
    elif name == "g64_bank_by_style":
        cc[:, 9:18] = 1                                   # class 2 unused by the content
        for k in range(s):
            sc[k] = k
    elif name == "g32_sky_takes_sky":
        cc[:, 0:4] = 1
        cc[1, :, 0:5] = 2
        sc[0, 0:3] = 1
        sc[1, :, 10:] = 2
        sc[1, :, 0:3] = 255
    elif name == "g160_missing_class":
        cc[:, :, 0:2] = 3                                 # absent from the bank
        cc[:, 5:, 4:] = 255
        cc[:, 3, 3] = 1
        sc[1] = 1
        sc[0, :, 0:9] = 2
    elif name == "g512_split_bank":
        cc[:, 4:] = 1
        sc[1] = 1
        sc[0, 20:] = 1
    return cc, sc


def bank_scores(ck, sk, dtype=torch.float64):
    """score(i, j) for every content patch and every patch of the bank: [n, M, S * Ns]."""
    return torch.cat([SR.scores(ck, sk[s:s + 1], dtype) for s in range(sk.shape[0])], dim=2)


def admissible(cc, sc):
    """bool [n, M, S * Ns]: sc(j) == cc(i) < MAX_CLASSES."""
    n = cc.shape[0]
    a, b = cc.reshape(n, -1, 1).long(), sc.reshape(1, 1, -1).long()
    return (a == b) & (a < MAX_CLASSES)


def masked_scores(ck, sk, cc, sc, dtype=torch.float64):
    """bank_scores with -inf where the pair is not admissible."""
    s = bank_scores(ck, sk, dtype)
    return torch.where(admissible(cc, sc), s, torch.full_like(s, float("-inf")))


def argmax_rows(msc):
    """(index, score) [n, M] of masked scores: the first maximum, NaN never wins, (-1, -inf) where nothing
    is above -inf."""
    idx, best = SR.argmax_rows(msc)
    return torch.where(torch.isinf(best) & (best < 0), torch.full_like(idx, -1), idx), best


def match(ck, sk, cc, sc, dtype=torch.float64):
    """(index int64 [n, H - 2, W - 2], winning score) in `dtype`."""
    n, _, h, w = ck.shape
    idx, best = argmax_rows(masked_scores(ck, sk, cc, sc, dtype))
    return idx.reshape(n, h - 2, w - 2), best.reshape(n, h - 2, w - 2)


def gather(sv, index, content, alpha=1.0, dtype=torch.float64):
    """The reconstruction from given global indices [n, H - 2, W - 2]: negative = no match."""
    sv, content = sv.to(dtype), content.to(dtype)
    n, c, h, w = content.shape
    cols = torch.cat([F.unfold(sv[s][None], 3)[0] for s in range(sv.shape[0])], dim=1)     # [C * 9, S * Ns]
    out = []
    for b in range(n):
        ix = index[b].reshape(-1).long()
        ok = (ix >= 0).to(dtype)[None, None]                                              # [1, 1, M]
        sel = cols[:, ix.clamp(0, cols.shape[1] - 1)][None] * ok                          # [1, C * 9, M]
        tot = F.fold(sel, (h, w), 3)[0]
        cnt = F.fold(ok.expand(1, 9, -1).contiguous(), (h, w), 3)[0]                      # [1, H, W]
        mixed = (1.0 - alpha) * content[b] + alpha * (tot / cnt.clamp(min=1.0))
        out.append(torch.where(cnt > 0, mixed, content[b]))
    return torch.stack(out)


def style_swap_guided(content, styles, cc, sc, alpha=1.0, normalize_keys=False, dtype=torch.float64, index=None):
    """(out, index). With `index` given, the reconstruction uses it instead of the reference's own."""
    if index is None:
        ck, sk = (SR.normalize(content, dtype), SR.normalize(styles, dtype)) if normalize_keys else (content, styles)
        index = match(ck, sk, cc, sc, dtype)[0]
    return gather(styles, index, content, alpha, dtype), index


# ---- the checks of the bars ---------------------------------------------------------------------------

def top_scale(msc):
    """S: the largest winning score of the case (over the matched patches)."""
    best = argmax_rows(msc)[1]
    return float(best[torch.isfinite(best)].max())


def near_tie_fraction(msc):
    """The share of content patches whose admissible runner-up lies within 2 * OP_TOL * S of the winner."""
    if msc.shape[2] < 2 or not bool(torch.isfinite(argmax_rows(msc)[1]).any()):
        return 0.0
    clean = torch.where(torch.isnan(msc), torch.full_like(msc, float("-inf")), msc)
    top = clean.topk(2, dim=2).values
    gap = torch.where(torch.isfinite(top[..., 1]), top[..., 0] - top[..., 1], torch.full_like(top[..., 0], float("inf")))
    return float((gap <= 2 * OP_TOL * top_scale(msc)).double().mean())


def check_match(index, score, msc):
    """(score error / S, worst index shortfall / S, wrong-class count, unmatched disagreements) of a
    guided match against the float64 masked scores [n, M, S * Ns]. The first two run over the patches
    the reference matches; the third counts returned indices >= 0 that are not admissible; the fourth
    the patches where `index < 0` and "the reference has no candidate" disagree."""
    n, m, _ = msc.shape
    index, score = index.reshape(n, m).long(), score.reshape(n, m).double()
    ref_idx, ref_best = argmax_rows(msc)
    none = ref_idx < 0
    disagree = int(((index < 0) != none).sum())
    at = msc.gather(2, index.clamp(min=0)[..., None])[..., 0]
    wrong_class = int(((index >= 0) & torch.isinf(at) & (at < 0) & ~none).sum())
    both = (index >= 0) & ~none
    if not bool(both.any()):
        return 0.0, 0.0, wrong_class, disagree
    s = top_scale(msc)
    e_score = float((score - at)[both].abs().max()) / s
    shortfall = float((ref_best - at)[both].max()) / s
    return e_score, shortfall, wrong_class, disagree
