"""CPU restatement of exact feature distribution matching (EFDM) and of the plane sort under it, in
plain torch: the reference side of tests/test_efdm_cpu.py and tests/test_gpu_efdm.py.

Order: IEEE-754 totalOrder of the float's bits, key = b < 0 ? -(b & 0x7fffffff) - 1 : b for the
int32 view b (so -0 < +0, negative NaNs first, positive NaNs last, equal keys = equal bits).
Rank: stable ascending (torch.sort(stable=True) on the integer keys). S: the style plane's values
in ascending key order. j(r) = ((2r + 1) * Ms) // (2 * Mc) in int64. out[i] = S[j(r(i))], bit for
bit at alpha == 1, else c + alpha * (t - c) in the dtype asked for."""
import torch

FUSED_MAX = 16384


def keys(x: torch.Tensor) -> torch.Tensor:
    """The signed totalOrder keys of a float32 tensor (int32, same shape)."""
    b = x.contiguous().view(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFFFFFF) - 1, b)


def rank_map(mc: int, ms: int) -> torch.Tensor:
    """j(r) for r = 0..mc-1 (int64)."""
    r = torch.arange(mc, dtype=torch.int64)
    return ((2 * r + 1) * ms) // (2 * mc)


def plane_sort(x: torch.Tensor):
    """x [P, M] float32 -> (values [P, M] float32 in ascending key order, int32 source indices)."""
    order = torch.sort(keys(x), dim=1, stable=True).indices
    vals = torch.gather(x.contiguous().view(torch.int32), 1, order).view(torch.float32)
    return vals, order.to(torch.int32)


def efdm_target(content: torch.Tensor, style: torch.Tensor) -> torch.Tensor:
    """t of the definition: float32 [N, C, Hc, Wc], every value a copy of a style value."""
    n, c = content.shape[:2]
    ns = style.shape[0]
    assert style.shape[1] == c and ns in (1, n)
    cf = content.reshape(n * c, -1)
    sf = style.expand(n, -1, -1, -1).reshape(n * c, -1)
    mc, ms = cf.shape[1], sf.shape[1]
    order = torch.sort(keys(cf), dim=1, stable=True).indices          # order[p, r] = element of rank r
    s_sorted = plane_sort(sf)[0].view(torch.int32)
    picked = s_sorted[:, rank_map(mc, ms)]                            # [P, Mc]: S[j(r)] by rank
    out = torch.empty_like(picked)
    out.scatter_(1, order, picked)
    return out.view(torch.float32).reshape(content.shape)


def efdm(content: torch.Tensor, style: torch.Tensor, alpha: float = 1.0, dtype=torch.float64) -> torch.Tensor:
    """alpha == 1: the target itself (float32 bits). Else c + alpha * (t - c) computed in `dtype`."""
    t = efdm_target(content, style)
    if alpha == 1.0:
        return t
    c = content.to(dtype)
    return c + alpha * (t.to(dtype) - c)


def brute_force_target(content: torch.Tensor, style: torch.Tensor) -> torch.Tensor:
    """The definition word for word, O(M^2) per plane: rank = number of (key_j, j) < (key_i, i)."""
    n, c = content.shape[:2]
    out = torch.empty(content.shape, dtype=torch.int32)
    for a in range(n):
        for ch in range(c):
            kc = keys(content[a, ch].reshape(-1)).tolist()
            sp = style[a if style.shape[0] == n else 0, ch].reshape(-1)
            ks = keys(sp).tolist()
            sb = sp.contiguous().view(torch.int32).tolist()
            s_sorted = [sb[j] for j in sorted(range(len(ks)), key=lambda j: (ks[j], j))]
            mc, ms = len(kc), len(ks)
            o = out[a, ch].view(-1)
            for i in range(mc):
                r = sum(1 for j in range(mc) if (kc[j], j) < (kc[i], i))
                o[i] = s_sorted[((2 * r + 1) * ms) // (2 * mc)]
    return out.view(torch.float32)


def paper_efdm(content: torch.Tensor, style: torch.Tensor) -> torch.Tensor:
    """Zhang et al.'s formulation for equal sizes: sort both planes as floats, send the style's
    sorted values through the inverse of the content's sorting permutation."""
    n, c = content.shape[:2]
    cf, sf = content.reshape(n, c, -1), style.reshape(n, c, -1)
    index_c = torch.sort(cf, dim=-1, stable=True).indices
    value_s = torch.sort(sf, dim=-1, stable=True).values
    inverse = index_c.argsort(-1)
    return value_s.gather(-1, inverse).reshape(content.shape)


def features(seed: int, shape, specials: bool = False) -> torch.Tensor:
    """A post-ReLU-like map: about half exact zeros, the rest positive; with `specials`, a -0.0,
    +inf, -inf and a NaN planted in every plane that has room for them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(shape, generator=g)).to(torch.float32)
    if specials:
        flat = x.view(-1, x.shape[-2] * x.shape[-1]) if x.dim() == 4 else x.view(x.shape[0], -1)
        m = flat.shape[1]
        for k, v in enumerate((-0.0, float("inf"), float("-inf"), float("nan"))):
            if m > k + 1:
                flat[:, ((m * (2 * k + 1)) // 9 + k) % m] = v
    return x


# name -> (content shape, style shape, specials, chunk); chunk 0 = the automatic path
CASES = {
    "small_specials": ((2, 3, 5, 7), (2, 3, 5, 7), True, 0),
    "64x64": ((2, 4, 64, 64), (2, 4, 64, 64), False, 0),
    "bigger_content": ((1, 2, 24, 40), (1, 2, 16, 16), False, 0),
    "bigger_style": ((1, 2, 16, 16), (1, 2, 24, 40), False, 0),
    "shared_style": ((3, 2, 9, 11), (1, 2, 9, 11), True, 0),
    "chunked_25x40": ((1, 2, 25, 40), (1, 2, 25, 40), True, 256),
    "chunked_4097": ((1, 1, 4097, 1), (1, 1, 4097, 1), True, 256),
    "chunked_sizes_differ": ((1, 2, 25, 40), (1, 2, 33, 21), False, 256),
    "at_fused_max": ((1, 2, 128, 128), (1, 2, 128, 128), False, 0),
    "past_fused_max": ((1, 1, 1, FUSED_MAX + 1), (1, 1, 1, FUSED_MAX + 1), False, 0),
}


def case_inputs(name: str):
    """(content, style, chunk) of a named case (float32 CPU tensors)."""
    cs, ss, specials, chunk = CASES[name]
    seed = 4100 + 2 * list(CASES).index(name)
    return features(seed, cs, specials), features(seed + 1, ss, specials), chunk


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rel_inf(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
