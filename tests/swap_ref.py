"""CPU restatement of style swap (include/ast_hip.h, csrc/swap.hip).

Definition. Content key ck [n, C, H, W], style key sk and style value sv [ns, C, Hs, Ws] (ns = n, or 1
for a style shared by the batch), content c [n, C, H, W]; every side at least 3. Content patch
i = y (W - 2) + x and style patch j = jy (Ws - 2) + jx are the C x 3 x 3 blocks with their top-left
corner at (y, x) / (jy, jx).
    score(i, j) = <ck patch i, sk patch j> / ||sk patch j||_2, exactly 0 for a style patch of zero norm
    index(i)    = the j of maximal score, the lowest j on equal scores; a NaN never wins; a score
                  replaces the running (-inf, 0) only when strictly greater, so index 0 (score -inf)
                  is returned when nothing wins. The content patch's own norm does not enter.
    out[y, x]   = (1 - alpha) c[y, x] + alpha / cnt(y, x) * sum of sv[jy + dy, jx + dx] over the (dy, dx)
                  in {0, 1, 2}^2 whose content patch (y - dy, x - dx) exists, (jy, jx) = index(y - dy,
                  x - dx), in ascending (dy, dx) order; cnt is the number of such terms (1..9).
With normalize=True the keys are the per-channel instance-normalised maps, (x - mean) / sqrt(unbiased
var + 1e-5), and the values the raw maps; otherwise the keys are the maps themselves.

The implementation here is the Chen & Schmidt form, deliberately not the kernel's tap-shift form:
the normalised style patches (F.unfold) are the filters of a conv2d over the content key, the
argmax runs over the filter axis, and the reconstruction is F.fold of the selected value patches
divided by the fold of ones. `dtype=torch.float64` is the reference, `dtype=torch.float32` the
emulation (the same computation in fp32).

Bars (all from the project, none from the code under test). OP_TOL = 2e-5 is the single-op bar of
wct_ref.py / test_gpu_parity.py; errors are rel_inf = max |got - ref| / max |ref|; S is the largest
winning score of a case.
    score   |score(i) - ref64(i, index(i))| <= OP_TOL * S for every content patch
    index   ref64(i, index(i)) >= max_j ref64(i, j) - 2 * OP_TOL * S for every content patch: two scores
            each within OP_TOL * S of the truth can swap order only inside that margin
    inputs  in the float64 reference alone, at most NEAR_TIE_MAX = 2 % of a case's content patches may
            have a runner-up inside that margin (asserted in test_swap_cpu.py)
    gather  given indices, against float64 from the same indices: GATHER_TOL = 1e-6 rel_inf (at most
            nine fp32 additions and one multiply: 9 * 2^-24 = 5.4e-7 of the summed magnitudes)
"""
import torch
import torch.nn.functional as F

OP_TOL = 2e-5
GATHER_TOL = 1e-6
NEAR_TIE_MAX = 0.02
NORM_EPS = 1e-5

# name -> (n, ns, C, (H, W), (Hs, Ws)): the smallest shapes at which the kernel can still go wrong
CASES = {
    "c8_one_patch": (1, 1, 8, (3, 3), (3, 3)),              # one patch on each side
    "c8_one_row": (1, 1, 8, (3, 9), (5, 3)),                # one row of content patches, one column of style patches
    "c48_k_tails": (2, 2, 48, (7, 9), (6, 11)),             # C not a multiple of 32; partial tiles on both sides
    "c64_shared_style": (2, 1, 64, (12, 13), (11, 15)),     # ns = 1; more than one tile of content and of style patches
    "c160_tile_tails": (1, 1, 160, (9, 8), (19, 21)),       # several style tiles with a tail
    "c32_many_queries": (1, 1, 32, (20, 23), (6, 7)),       # many content tiles, few style patches
    "c512_split_keys": (1, 1, 512, (10, 10), (34, 34)),     # the model's C; 1024 style patches against 64 content
}                                                           # patches: the shape that makes the library split


def features(seed, shape):
    """relu(randn): float32 [n, C, h, w]."""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(*shape, generator=g, dtype=torch.float64)).float()


def case_inputs(name):
    """(content, style) of a named case."""
    n, ns, c, (hc, wc), (hs, ws) = CASES[name]
    seed = 9000 + 10 * list(CASES).index(name)
    return features(seed, (n, c, hc, wc)), features(seed + 1, (ns, c, hs, ws))


def rel_inf(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def normalize(x, dtype=torch.float64):
    """Per-channel instance normalisation (x - mean) / sqrt(unbiased var + 1e-5) in `dtype`."""
    v = x.to(dtype)
    mean = v.mean(dim=(2, 3), keepdim=True)
    var = v.var(dim=(2, 3), keepdim=True, unbiased=True)
    return (v - mean) / (var + NORM_EPS).sqrt()


def scores(ck, sk, dtype=torch.float64):
    """score(i, j) for every pair: [n, M, Ns], as a conv of ck with the normalised style patches."""
    ck, sk = ck.to(dtype), sk.to(dtype)
    n, c = ck.shape[:2]
    out = []
    for b in range(n):
        s = sk[b if sk.shape[0] > 1 else 0][None]
        cols = F.unfold(s, 3)[0]                                        # [C * 9, Ns]
        nrm = cols.norm(dim=0, keepdim=True)
        filt = torch.where(nrm > 0, cols / nrm, torch.zeros_like(cols))
        filt = filt.t().reshape(-1, c, 3, 3)                            # [Ns, C, 3, 3]
        out.append(F.conv2d(ck[b][None], filt)[0].flatten(1).t())       # [M, Ns]
    return torch.stack(out)


def argmax_rows(sc):
    """(index, score) [n, M] of scores [n, M, Ns]: the first maximum; NaN never wins; (0, -inf) if
    nothing is above -inf."""
    clean = torch.where(torch.isnan(sc), torch.full_like(sc, float("-inf")), sc)
    idx = clean.argmax(dim=2)           # the first of equal maxima
    return idx, clean.gather(2, idx[..., None])[..., 0]


def match(ck, sk, dtype=torch.float64):
    """(index int64 [n, H - 2, W - 2], winning score) in `dtype`."""
    n, _, h, w = ck.shape
    idx, best = argmax_rows(scores(ck, sk, dtype))
    return idx.reshape(n, h - 2, w - 2), best.reshape(n, h - 2, w - 2)


def gather(sv, index, content, alpha=1.0, dtype=torch.float64):
    """The reconstruction from given indices [n, H - 2, W - 2]: fold of the selected value patches over
    the fold of ones, blended with the content."""
    sv, content = sv.to(dtype), content.to(dtype)
    n, c, h, w = content.shape
    out = []
    for b in range(n):
        cols = F.unfold(sv[b if sv.shape[0] > 1 else 0][None], 3)[0]    # [C * 9, Ns]
        sel = cols[:, index[b].reshape(-1).long()][None]               # [1, C * 9, M]
        tot = F.fold(sel, (h, w), 3)[0]
        cnt = F.fold(torch.ones_like(sel[:, :9]), (h, w), 3)[0]          # [1, H, W]
        out.append((1.0 - alpha) * content[b] + alpha * (tot / cnt))
    return torch.stack(out)


def style_swap(content, style, alpha=1.0, normalize_keys=False, dtype=torch.float64, index=None):
    """(out, index). With `index` given, the reconstruction uses it instead of the reference's own."""
    if index is None:
        ck, sk = (normalize(content, dtype), normalize(style, dtype)) if normalize_keys else (content, style)
        index = match(ck, sk, dtype)[0]
    return gather(style, index, content, alpha, dtype), index


# ---- the checks of the bars ---------------------------------------------------------------------------

def top_scale(ref_scores):
    """S: the largest winning score of the case."""
    return float(argmax_rows(ref_scores)[1].max())


def near_tie_fraction(ref_scores):
    """The share of content patches whose runner-up lies within 2 * OP_TOL * S of the winner (float64
    reference alone)."""
    if ref_scores.shape[2] < 2:
        return 0.0
    top = ref_scores.topk(2, dim=2).values
    return float(((top[..., 0] - top[..., 1]) <= 2 * OP_TOL * top_scale(ref_scores)).double().mean())


def check_match(index, score, ref_scores):
    """(score error / S, worst index shortfall / S) of a match against the float64 scores [n, M, Ns]:
    the score bar asks the first <= OP_TOL, the index rule the second <= 2 * OP_TOL."""
    n, m, _ = ref_scores.shape
    s = top_scale(ref_scores)
    at = ref_scores.gather(2, index.reshape(n, m, 1).long())[..., 0]
    e_score = float((score.reshape(n, m).double() - at).abs().max()) / s
    shortfall = float((argmax_rows(ref_scores)[1] - at).max()) / s
    return e_score, shortfall
