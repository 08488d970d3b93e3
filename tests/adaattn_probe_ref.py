"""Exact probes for the AdaAttN forward (csrc/adaattn.hip): three input constructions whose answer
is a closed form in float64, so the kernels are held to the few fp32 roundings of their epilogue
(and, in bf16, the rounding of the output) instead of to a whole-op bar on random data.

Shared by tests/test_adaattn_probe_cpu.py (the constructions' conditions, a bf16 emulation with
planted defects) and tests/test_gpu_adaattn_probes.py (the kernels).

Style maps and W_v, in every probe:
  * style entries are integers, |s| <= 3, and every (image, channel) plane sums to exactly 0 (so the
    bf16 path's style mean is exactly 0 and its centred V' is V); the one exception is the `mean`
    variant of the uniform probe, whose planes are such a plane plus +-1 (mean exact, Nk = 2^k);
  * style columns are pairwise distinct within an image;
  * W_v is a signed permutation with magnitudes 1..3: V = W_v s is a small integer (|V| <= 9),
    V and V^2 are exact in bf16 (asserted), and each V channel is one style channel.

uniform   W_k = 0: every logit is exactly 0, those of the zero-padded keys too, so only the tail
          mask separates keys from padding. out = sqrt(mean_k V^2 - (mean_k V)^2) IN(c) + mean_k V.
planted   style +-1 (one 0 per plane when Nk is odd), content[:, i] = style[:, pi(i)], W_q = W_k =
          g I: query i's own key wins by >= 128 nats (after the bf16 rounding of Q and K), which is
          past fp32's smallest denormal in log2 units: every other weight and every rescale factor
          of the online softmax is exactly 0 and out[:, i] == V[:, pi(i)], in fp32 and in bf16.
twin      match channels (a +-1 code shared by the two keys of a pair; W_q = W_k = g on them) and
          payload channels (ch % 8 == 7; zero-sum integers that differ between the twins; W_q = W_k
          = 0): the twins' K rows are bit-equal, each query weights its pair 1/2 and 1/2, and
          mean = (V_a + V_b) / 2, std = |V_a - V_b| / 2. Pairs are placed inside one 16-key group,
          across 32-key blocks, across key splits and on key Nk - 1.

Bounds. planted: equality. uniform and twin: |out - ref| <= slack in fp32 and <= ulp_bf16(ref) / 2
+ slack in bf16, slack = 2^-18 (std (|IN(c)| + rstd_c mean_q |c|) + |mean|): the sums over keys are
sums of exact small integers against weights that are exactly 1 or 0, so the only roundings are the
epilogue's fp32 operations (content statistics, 1 / l, the variance fma, sqrt, the final fma): fewer
than ten, each <= 2^-24 relative; 2^-18 leaves a factor of about eight over that count.
The rstd_c mean_q |c| term is the one departure from a purely relative slack 2^-18 (|std IN(c)| +
|mean|): the content mean is an fp32 sum, off by a few 2^-24 of mean_q |c| in ABSOLUTE terms, and
c - mean_c cancels for a pixel near its plane's mean, where that error is no longer small against
|IN(c)|. A correct fp32 emulation left 1 to 37 such elements per case (|ref| ~ 1e-6, up to 25 x the
relative slack) outside the purely relative form; the term is of the size of the relative one for a
typical pixel (both ~ 2^-18 std), so the bound stays some 2^-17 of std, against defects of >= 1e-3.
"""
import ctypes
import functools
import types

import numpy as np
import torch

LOG2E = 1.4426950408889634
SLACK = 2.0 ** -18
MARGIN_NATS = 128.0
EPS = 1e-5

# (n, C, hc, wc, hs, ws), waves of the bf16 launch, keys split in the bf16 launch, what it reaches
CASES = [
    ((512, 32, 3, 5, 5, 7), 8, False, "8-wave CT 1; Nk = 35; one query tile, mostly padding"),
    ((512, 64, 3, 5, 5, 7), 8, False, "8-wave CT 2"),
    ((512, 96, 2, 3, 3, 11), 8, False, "8-wave CT 3"),
    ((256, 128, 17, 16, 7, 10), 8, False, "8-wave CT 4; two query tiles, the second with 16 queries; tile remap"),
    ((512, 32, 2, 4, 10, 10), 8, False, "8-wave; four key blocks, 4 keys in the last"),
    ((256, 32, 3, 4, 33, 31), 4, False, "4-wave; Nk = 1023: 32 key blocks, no split"),
    ((1, 128, 32, 32, 33, 31), 4, True, "4-wave; keys split"),
    ((1, 64, 48, 40, 33, 35), 4, True, "4-wave; Nk = 1155, uneven last split"),
    ((2, 40, 20, 20, 12, 12), 4, True, "C not a multiple of 32 (five key blocks: split in two)"),
    ((2, 8, 17, 3, 3, 4), 4, False, "C = 8: one padded channel tile"),
]
# the uniform probe's `mean` variant: Nk a power of two (no padded key), style planes of mean +-1
MEAN_CASES = [
    ((512, 32, 3, 5, 4, 8), 8, False, "8-wave; Nk = 32, V mean added back by the attention epilogue"),
    ((2, 64, 9, 13, 8, 16), 4, True, "4-wave; Nk = 128, keys split: V mean added back by the merge"),
]


def case_id(case):
    n, c, hc, wc, hs, ws = case[0]
    return f"{n}x{c}-{hc}x{wc}-{hs}x{ws}"


def plan(dtype, shape):
    """ast_adaattn_plan as a namespace (waves, ksplit, kchunk, nqp, nkp); dtype 0 = fp32, 1 = bf16."""
    from arbitrarystyletransfer_amd import _lib
    out = [ctypes.c_int(0) for _ in range(5)]
    rc = _lib.lib().ast_adaattn_plan(dtype, *shape, *(ctypes.addressof(o) for o in out))
    assert rc == 0, (rc, dtype, shape)
    return types.SimpleNamespace(**{k: o.value for k, o in zip(("waves", "ksplit", "kchunk", "nqp", "nkp"), out)})


# ---------------------------------------------------------------------------------------------------
# number formats and bounds
# ---------------------------------------------------------------------------------------------------
def bf16_round(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def ulp_bf16(x):
    """Spacing of bf16 at |x| (float64 in, float64 out): 2^(floor(log2 |x|) - 7)."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    _, e = torch.frexp(a)           # a = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 8)


def bound(pr, dtype, relative_only=False):
    """Per-element bound of a uniform / twin probe for the output dtype (relative_only: with the
    purely relative slack, for the record)."""
    slack = pr.slack_rel if relative_only else pr.slack
    return slack if dtype == torch.float32 else ulp_bf16(pr.ref) / 2 + slack


def err_over_bound(out, pr, dtype, relative_only=False):
    """max and per-element |out - ref| / bound (bound > 0 wherever ref != 0; 0/0 counts as 0)."""
    err = (out.double().cpu() - pr.ref).abs()
    b = bound(pr, dtype, relative_only)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(ratio.max()), ratio


def slack_used(out, pr):
    """bf16 outputs: the largest (|out - ref| - ulp_bf16(ref) / 2) / slack, i.e. how much of the slack
    the fp32 value behind the rounded output needed (<= 0: none)."""
    err = (out.double().cpu() - pr.ref).abs() - ulp_bf16(pr.ref) / 2
    return float(torch.where(err <= 0, torch.zeros_like(err), err / pr.slack).max())


def _in64(x):
    """InstanceNorm2d (biased variance, eps 1e-5, no affine) over the last axis, float64."""
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + EPS)


def _assert_exact_v(v):
    assert torch.equal(bf16_round(v), v) and torch.equal(bf16_round(v * v), v * v), "V or V^2 is not exact in bf16"


def _assert_zero_sum(style):
    assert int(style.sum(-1).abs().max()) == 0, "a style plane does not sum to 0"


def _assert_distinct_columns(style):
    """Style columns pairwise distinct within each image (style: integer [n, C, Nk])."""
    cols = np.ascontiguousarray(style.permute(0, 2, 1).numpy().astype(np.int8))
    rows = cols.view(np.dtype((np.void, cols.shape[2]))).reshape(cols.shape[0], cols.shape[1])
    for b in range(rows.shape[0]):
        assert len(np.unique(rows[b])) == rows.shape[1], f"image {b}: two style columns are equal"


# ---------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------
def _signed_permutation(rng, c):
    w = np.zeros((c, c), np.float64)
    w[np.arange(c), rng.permutation(c)] = rng.choice([-1.0, 1.0], c) * rng.integers(1, 4, c)
    return torch.from_numpy(w)


def _zero_sum_planes(rng, n, c, nk, amax, nonzero=False):
    """Integer planes [n, C, Nk], |s| <= amax, each summing to 0: r, -r (and one 0 when Nk is odd),
    shuffled along the keys. nonzero: r is +-amax only."""
    half = nk // 2
    r = rng.integers(-amax, amax + 1, (n, c, half))
    if nonzero:
        r = amax * (2 * rng.integers(0, 2, (n, c, half)) - 1)
    base = np.concatenate([r, -r, np.zeros((n, c, nk - 2 * half), r.dtype)], -1)
    return torch.from_numpy(rng.permuted(base, axis=-1)).double()


def _per_image_shuffle(rng, base, n):
    """[C, N] -> [n, C, N]: every image sees the base with its own channel and column order (the
    pairwise distances between columns, checked once on the base, hold for every image)."""
    c, m = base.shape
    out = np.empty((n, c, m), base.dtype)
    for b in range(n):
        out[b] = base[rng.permutation(c)][:, rng.permutation(m)]
    return out


def _content_values(rng, shape):
    """Random bf16-exact content."""
    return bf16_round(torch.from_numpy(rng.standard_normal(shape) * 1.5 + 0.25)).double()


def margin_nats(content, style, wq, wk, winners):
    """The margin condition, float64: over every query and every non-winning key j,
    min (L_w - L_j - 2 * 2^-7 * max(B_w, B_j)),  L = q.k,  B = sum_ch |q_ch| |k_ch|
    with w the query's weakest winner. bf16 rounds Q and K to 2^-9 relative each (W = g I is exact),
    so a logit moves by at most 2^-8 B and a difference of two by 2^-7 max B: the term is twice that."""
    q = wq @ _in64(content)
    k = wk @ _in64(style)
    L = q.transpose(1, 2) @ k
    B = q.abs().transpose(1, 2) @ k.abs()
    lw = L.masked_fill(~winners, float("inf")).amin(-1, keepdim=True)
    bw = B.masked_fill(~winners, 0.0).amax(-1, keepdim=True)
    m = (lw - L - 2.0 ** -6 * torch.maximum(B, bw)).masked_fill(winners, float("inf"))
    return float(m.min())


def _pick_g(m1):
    """Smallest power of two g >= 4 with g^2 * (margin at g = 1) >= 128 nats."""
    assert m1 > 0, f"no margin at any scale ({m1})"
    g = 4
    while g * g * m1 < MARGIN_NATS:
        g *= 2
    assert g <= 64, (g, m1)
    return g


def _finish(shape, content, style, wq, wk, wv, mean, std, **extra):
    n, c, hc, wc, hs, ws = shape
    xn = _in64(content)
    ref = std * xn + mean
    cm = content.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((content - cm) ** 2).mean(-1, keepdim=True) + EPS)
    slack_rel = SLACK * ((std * xn).abs() + mean.abs())                               # purely relative
    slack = slack_rel + SLACK * std * rstd * content.abs().mean(-1, keepdim=True)    # + the content mean's error
    f32 = lambda t: t.to(torch.float32)
    assert torch.equal(bf16_round(content), content) and torch.equal(bf16_round(style), style)
    return types.SimpleNamespace(
        shape=shape, content=f32(content).reshape(n, c, hc, wc), style=f32(style).reshape(n, c, hs, ws),
        wq=f32(wq), wk=f32(wk), wv=f32(wv), ref=ref.reshape(n, c, hc, wc), slack=slack.reshape(n, c, hc, wc),
        slack_rel=slack_rel.reshape(n, c, hc, wc), **extra)


# ---------------------------------------------------------------------------------------------------
# the probes
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform(shape, with_mean=False, seed=11):
    n, c, hc, wc, hs, ws = shape
    nq, nk = hc * wc, hs * ws
    rng = np.random.default_rng(seed + 7 * c + nk)
    if with_mean:
        assert nk & (nk - 1) == 0, "the mean variant needs Nk = 2^k (plane means exact)"
        style = _zero_sum_planes(rng, n, c, nk, 2) + torch.from_numpy(rng.choice([-1.0, 1.0], (n, c, 1)))
        assert float(style.mean(-1).abs().min()) == 1.0
    else:
        style = _zero_sum_planes(rng, n, c, nk, 3)
        _assert_zero_sum(style)
    assert float(style.abs().max()) <= 3
    _assert_distinct_columns(style)
    wv = _signed_permutation(rng, c)
    v = wv @ style
    vc = wv @ (style - style.mean(-1, keepdim=True))    # what the bf16 path stores
    _assert_exact_v(v)
    _assert_exact_v(vc)
    content = _content_values(rng, (n, c, nq))
    wq = torch.from_numpy(rng.standard_normal((c, c)) * 0.3).float().double()
    wk = torch.zeros(c, c, dtype=torch.float64)
    mean = v.mean(-1, keepdim=True).expand(n, c, nq)
    std = torch.sqrt((v * v).mean(-1, keepdim=True) - v.mean(-1, keepdim=True) ** 2).expand(n, c, nq)
    return _finish(shape, content, style, wq, wk, wv, mean, std)


def planted_must_keys(nk):
    """Keys every planted map must cover: 0, Nk - 1 and the edges of the V slot shuffle's 4-key
    runs (positions 3, 4, 7, 8, 11, 12, 15, 16) of one 32-key block (the second where there is one)."""
    blk = 1 if nk >= 64 else 0
    must = [0, nk - 1] + [32 * blk + p for p in (3, 4, 7, 8, 11, 12, 15, 16)]
    return list(dict.fromkeys(k for k in must if k < nk))


@functools.lru_cache(maxsize=None)
def planted(shape, seed=23):
    n, c, hc, wc, hs, ws = shape
    nq, nk = hc * wc, hs * ws
    for attempt in range(32):
        rng = np.random.default_rng(seed + 7 * c + nk + 1000 * attempt)
        base = _zero_sum_planes(rng, 1, c, nk, 1, nonzero=True)[0].numpy()
        if len(np.unique(base.T, axis=0)) == nk:
            break
    style = torch.from_numpy(_per_image_shuffle(rng, base, n))
    _assert_zero_sum(style)
    _assert_distinct_columns(style)
    assert int(((style == 0).sum(-1) != nk % 2).sum()) == 0      # +-1, one 0 per plane when Nk is odd
    # pi: the must keys first, then every other key, dealt to the queries of the whole batch in turn
    must = planted_must_keys(nk)
    seq = np.array(must + [k for k in rng.permutation(nk) if k not in set(must)])
    pi = torch.from_numpy(seq[(np.arange(n)[:, None] * nq + np.arange(nq)[None, :]) % nk])   # [n, Nq]
    content = torch.gather(style, 2, pi[:, None, :].expand(n, c, nq))
    wv = _signed_permutation(rng, c)
    v = wv @ style
    _assert_exact_v(v)
    eye = torch.eye(c, dtype=torch.float64)
    winners = torch.zeros(n, nq, nk, dtype=torch.bool).scatter_(2, pi[:, :, None], True)
    g = _pick_g(margin_nats(content, style, eye, eye, winners))
    margin = margin_nats(content, style, g * eye, g * eye, winners)
    assert margin >= MARGIN_NATS, margin
    mean = torch.gather(v, 2, pi[:, None, :].expand(n, c, nq))
    covered = set(pi.flatten().tolist())
    assert set(must) <= covered and (len(covered) == nk or n * nq < nk)
    if nq >= nk:
        assert all(len(set(pi[b].tolist())) == nk for b in range(n))
    return _finish(shape, content, style, g * eye, g * eye, wv, mean, torch.zeros_like(mean), pi=pi, g=g, margin=margin,
                   must=must)


def twin_pairs(nk, kchunk_keys, rng):
    """(pairs [P, 2], singles): placed pairs first -- one inside a 16-key group (on two different 4-key
    runs of the V slot shuffle), one across 32-key blocks, one across the first two key splits
    (kchunk_keys = keys per split, 0 without a split) and one on key Nk - 1 (with key 5: another
    block when Nk > 32, the first and the last split when the keys are split) -- then the other keys
    paired at random. The number of pairs is even (so +-1 codes can balance); 0..3 keys stay single."""
    blk = 1 if nk >= 64 else 0
    placed = [(32 * blk + 3, 32 * blk + min(12, nk - 2)), (5, nk - 1)]
    if nk > 46:
        placed.append((10, 45))
    if kchunk_keys:
        placed.append((20, kchunk_keys + 7))
    used = [k for p in placed for k in p]
    assert len(set(used)) == len(used) and max(used) < nk, placed
    rest = [int(k) for k in rng.permutation(nk) if k not in set(used)]
    npairs = len(rest) // 2
    if (npairs + len(placed)) % 2:
        npairs -= 1
    singles = rest[2 * npairs:]
    pairs = placed + [(rest[2 * i], rest[2 * i + 1]) for i in range(npairs)]
    return np.array(pairs), singles, placed


def twin_placements(pairs, nk, kchunk_keys):
    """Which placements a pair list covers (the GPU test holds this against the planned kchunk)."""
    a, b = pairs[:, 0], pairs[:, 1]
    return {
        "same16": bool(np.any((a // 16 == b // 16) & (a % 16 // 4 != b % 16 // 4))),
        "blocks": bool(np.any(a // 32 != b // 32)),
        "splits": bool(kchunk_keys and np.any(a // kchunk_keys != b // kchunk_keys)),
        "adjacent_splits": bool(kchunk_keys and np.any(np.abs(a // kchunk_keys - b // kchunk_keys) == 1)),
        "last": bool(np.any((a == nk - 1) | (b == nk - 1))),
    }


@functools.lru_cache(maxsize=None)
def twin(shape, kchunk_keys=0, seed=37):
    n, c, hc, wc, hs, ws = shape
    nq, nk = hc * wc, hs * ws
    pay = np.array([ch for ch in range(c) if ch % 8 == 7])
    mat = np.array([ch for ch in range(c) if ch % 8 != 7])
    for attempt in range(64):
        rng = np.random.default_rng(seed + 7 * c + nk + 1000 * attempt)
        pairs, singles, placed = twin_pairs(nk, kchunk_keys, rng)
        npairs = len(pairs)
        base = rng.permuted(np.tile(np.repeat([1.0, -1.0], npairs // 2), (len(mat), 1)), axis=-1)   # [Cm, P] balanced
        if len(np.unique(base.T, axis=0)) == npairs:
            break
    code = _per_image_shuffle(rng, base, n)                         # [n, Cm, P]
    style = np.zeros((n, c, nk))
    style[:, mat[:, None], pairs[None, :, 0]] = code
    style[:, mat[:, None], pairs[None, :, 1]] = code
    # payload: (x, y), x != y, for half the pairs and (-x, -y) for the other half, pair order shuffled
    # per plane; the singles get 0 / (r, -r) / (0, r, -r): zero sum, twins differ in every channel
    x = rng.integers(-3, 4, (n, len(pay), npairs // 2))
    y = (x + 3 + rng.integers(1, 7, x.shape)) % 7 - 3
    xy = np.stack([np.concatenate([x, -x], -1), np.concatenate([y, -y], -1)], -1)     # [n, Cp, P, 2]
    xy = np.take_along_axis(xy, np.argsort(rng.random(xy.shape[:3]), -1)[..., None], 2)
    style[:, pay[:, None], pairs[None, :, 0]] = xy[..., 0]
    style[:, pay[:, None], pairs[None, :, 1]] = xy[..., 1]
    if len(singles) >= 2:
        r = rng.integers(1, 4, (n, len(pay)))
        style[:, pay, singles[-2]] = r
        style[:, pay, singles[-1]] = -r
    style = torch.from_numpy(style)
    _assert_zero_sum(style)
    assert float(style.abs().max()) <= 3
    _assert_distinct_columns(style)
    ia, ib = torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])
    assert torch.equal(style[:, mat][:, :, ia], style[:, mat][:, :, ib])            # twins: equal codes
    assert bool((style[:, pay][:, :, ia] != style[:, pay][:, :, ib]).all())         # and different payloads
    # targets: the placed pairs first, then the others, dealt to the queries of the whole batch in turn
    tgt = torch.from_numpy((np.arange(n)[:, None] * nq + np.arange(nq)[None, :]) % npairs)    # [n, Nq]
    assert n * nq >= len(placed)
    content = _content_values(rng, (n, c, nq))
    content[:, mat] = torch.gather(torch.from_numpy(code), 2, tgt[:, None, :].expand(n, len(mat), nq))
    ka, kb = ia[tgt], ib[tgt]                                                        # [n, Nq]
    winners = torch.zeros(n, nq, nk, dtype=torch.bool).scatter_(2, ka[:, :, None], True).scatter_(2, kb[:, :, None], True)
    sel = torch.zeros(c, dtype=torch.float64)
    sel[mat] = 1.0
    g = _pick_g(margin_nats(content, style, torch.diag(sel), torch.diag(sel), winners))
    wqk = g * torch.diag(sel)
    margin = margin_nats(content, style, wqk, wqk, winners)
    assert margin >= MARGIN_NATS, margin
    k = wqk @ _in64(style)
    assert torch.equal(k[:, :, ia], k[:, :, ib])                                     # the twins' K rows
    wv = _signed_permutation(rng, c)
    v = wv @ style
    _assert_exact_v(v)
    va = torch.gather(v, 2, ka[:, None, :].expand(n, c, nq))
    vb = torch.gather(v, 2, kb[:, None, :].expand(n, c, nq))
    return _finish(shape, content, style, wqk, wqk, wv, (va + vb) / 2, (va - vb).abs() / 2, pairs=pairs, placed=placed,
                   tgt=tgt, g=g, margin=margin, placements=twin_placements(pairs[tgt.unique().numpy()], nk, kchunk_keys))


# ---------------------------------------------------------------------------------------------------
# a plain torch emulation of the bf16 pipeline, with defects that can be planted
# ---------------------------------------------------------------------------------------------------
DEFECTS = ("pad", "drop", "vswap", "merge", "qtile")


def vswap_keys(nk):
    """The two keys the `vswap` defect exchanges in V (not in K): neighbours across a 4-key run."""
    blk = 1 if nk >= 64 else 0
    return 32 * blk + 3, 32 * blk + 4


def emulate_bf16(pr, pl, defect=None):
    """project_bf16_kernel, attend_bf16_kernel and attn_merge_kernel in torch on the CPU: Q, K, V,
    V^2 and P rounded to bf16, fp32 accumulation, the key splits of the plan `pl` merged as the
    merge kernel does. Returns bf16 [n, C, hc, wc].
      pad    one padded key (key Nk) counted by the softmax
      drop   the last key masked
      vswap  V and V^2 of two keys of one 16-key group exchanged, K left alone
      merge  split 1 merged with weight 1 instead of 2^(m_1 - M)
      qtile  query tile t reads the Q of tile t ^ 1"""
    assert defect is None or defect in DEFECTS
    n, c, hc, wc, hs, ws = pr.shape
    nq, nk = hc * wc, hs * ws
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    x, s = pr.content.reshape(n, c, nq), pr.style.reshape(n, c, nk)

    def stats(t):
        m = t.mean(-1, keepdim=True)
        return m, 1.0 / torch.sqrt(((t - m) ** 2).mean(-1, keepdim=True) + np.float32(EPS))
    cm, crs = stats(x)
    sm, srs = stats(s)
    q = bf(bf(pr.wq) @ bf((x - cm) * (crs * np.float32(LOG2E))))     # log2 units, as the kernel's Q
    k = bf(bf(pr.wk) @ bf((s - sm) * srs))
    vf = bf(pr.wv) @ bf(s - sm)
    v, v2 = bf(vf), bf(vf * vf)
    vm = pr.wv @ sm                                                   # [n, C, 1]
    pad = lambda t, m: torch.nn.functional.pad(t, (0, m - t.shape[-1]))
    q, k, v, v2 = pad(q, pl.nqp), pad(k, pl.nkp), pad(v, pl.nkp), pad(v2, pl.nkp)
    if defect == "qtile":
        t = pl.waves * 32
        tiles = torch.arange(pl.nqp // t)
        src = torch.where((tiles ^ 1) < len(tiles), tiles ^ 1, tiles)
        q = q.reshape(n, c, -1, t)[:, :, src].reshape(n, c, pl.nqp)
    if defect == "vswap":
        a, b = vswap_keys(nk)
        idx = torch.arange(pl.nkp)
        idx[a], idx[b] = b, a
        v, v2 = v[:, :, idx], v2[:, :, idx]
    q = q[:, :, :nq]
    sc = q.transpose(1, 2) @ k                                        # [n, Nq, Nkp]
    valid = nk + 1 if defect == "pad" else nk - 1 if defect == "drop" else nk
    sc[:, :, min(valid, pl.nkp):] = float("-inf")
    step = pl.kchunk * 32
    parts = []
    for sp in range(pl.ksplit):
        ssl = sc[:, :, sp * step:(sp + 1) * step]
        m = ssl.amax(-1, keepdim=True)
        p = torch.exp2(ssl - m)
        pb = bf(p)
        parts.append((m, p.sum(-1, keepdim=True), pb @ v[:, :, sp * step:(sp + 1) * step].transpose(1, 2),
                      pb @ v2[:, :, sp * step:(sp + 1) * step].transpose(1, 2)))
    M = torch.stack([p[0] for p in parts]).amax(0)
    L = O = O2 = 0.0
    for sp, (m, l, o, o2) in enumerate(parts):
        w = torch.ones_like(m) if (defect == "merge" and sp == 1) else torch.exp2(m - M)
        L, O, O2 = L + w * l, O + w * o, O2 + w * o2
    mean = (O * (1.0 / L)).transpose(1, 2)                            # [n, C, Nq]
    var = torch.relu((O2 * (1.0 / L)).transpose(1, 2) - mean * mean)
    out = torch.sqrt(var) * ((x - cm) * crs) + (mean + vm)
    return out.to(torch.bfloat16).reshape(n, c, hc, wc)
