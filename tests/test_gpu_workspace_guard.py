"""No entry point writes past the workspace that its *_workspace_bytes query asks for.

Every C-ABI entry of efdm.hip, efdm_regions.hip, wct.hip, swap.hip, remd.hip and selfsim.hip that takes a
workspace is called through _lib.lib() on a uint8 buffer of `bytes` plus an equal-sized guard (at least
1 MiB), all of it 0xA5, with workspace_bytes = bytes exactly. After a synchronise every guard byte must
still be 0xA5, and the outputs must equal, bit for bit, those of the ops.* wrapper on the same inputs
(whose workspace comes from torch.empty: the outputs do not depend on what the workspace held).
The shapes are the smallest that populate every region: two tiles against three and six tile pairs for
the pixel matches, three style tiles with 1 and 3 splits for the swap, two channel tiles for the WCT,
the chunk-and-merge path for the sorts."""
import pytest
import torch

from arbitrarystyletransfer_amd import _lib, ops

pytestmark = pytest.mark.gpu

GUARD_MIN = 1 << 20
FILL = 0xA5


def _rand(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32)


def _labels(seed, regions, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, regions, shape, generator=g, dtype=torch.uint8)


def _same(a, b):
    """Bit for bit, NaN patterns included."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.reshape(-1), b.reshape(-1)
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return bool(torch.equal(a, b))


def _guarded(dev, query, qargs, entry, args):
    """entry(*args, workspace, bytes, stream) on a guarded workspace of exactly query(*qargs) bytes."""
    L = _lib.lib()
    nbytes = int(getattr(L, query)(*qargs))
    assert nbytes > 0, (query, qargs, nbytes)
    buf = torch.full((nbytes + max(nbytes, GUARD_MIN),), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    _lib.check(getattr(L, entry)(*args, buf.data_ptr(), nbytes, _lib.stream_ptr(dev)), entry)
    torch.cuda.synchronize(dev)
    touched = int((buf[nbytes:] != FILL).sum())
    assert touched == 0, f"{entry}{tuple(qargs)}: {touched} guard bytes written past {nbytes}"


def _p(*ts):
    return [t.data_ptr() for t in ts]


# ---- relaxed EMD: C = 8, n = 2, M = 70 (2 tiles), P = 130 (3 tiles) ----

@pytest.fixture(scope="module")
def remd_maps(hip_device):
    return _rand(11, 2, 8, 7, 10).to(hip_device), _rand(12, 2, 8, 10, 13).to(hip_device)


@pytest.mark.parametrize("splits", [1, 3])
def test_cosine_match(hip_device, remd_maps, splits):
    x, y = remd_maps
    n, c, m, p = 2, 8, 70, 130
    u, v = ops.cosine_norms(x), ops.cosine_norms(y)
    want = ops.cosine_match(x, y, _splits=splits)
    got = [torch.empty_like(t) for t in want]
    _guarded(hip_device, "ast_cosine_match_workspace_bytes", (n, n, m, p, splits), "ast_cosine_match_f32",
             _p(x, y, u, v, *got) + [n, n, c, m, p, splits])
    assert all(_same(a, b) for a, b in zip(got, want))


def test_remd_loss_and_backward(hip_device, remd_maps):
    x, y = remd_maps
    n, c, m, p = 2, 8, 70, 130
    # the column branch for every sample: the backward then fills its start, cursor and list regions
    loss, rmean, cmean, branch, state = ops.remd_loss(x, y, weight=0.7, _branch=2)
    got = [torch.empty_like(t) for t in state]
    g_rmean, g_cmean, g_branch = torch.empty_like(rmean), torch.empty_like(cmean), torch.empty_like(branch)
    acc = _lib.loss_accumulator(hip_device, pooled=False)
    _guarded(hip_device, "ast_remd_loss_workspace_bytes", (n, n, m, p), "ast_remd_loss_f32",
             _p(x, y, *got, g_rmean, g_cmean, g_branch, acc) + [n, n, c, m, p, 0.7, 2])
    assert all(_same(a, b) for a, b in zip(got, state))
    assert _same(g_rmean, rmean) and _same(g_cmean, cmean) and _same(g_branch, branch) and _same(acc[0], loss)

    grad = torch.ones((), device=hip_device)
    want = ops.remd_loss_backward(x, y, state, branch, grad, weight=0.7)
    dx = torch.empty_like(x)
    _guarded(hip_device, "ast_remd_loss_backward_workspace_bytes", (n, m, p), "ast_remd_loss_backward_f32",
             _p(x, y, *state, branch, grad, dx) + [n, n, c, m, p, 0.7])
    assert _same(dx, want)


# ---- self-similarity: C = 8, n = 2, N = 130 (3 tiles, 6 tile pairs) ----

def test_selfsim_entries(hip_device):
    x, cm = _rand(21, 2, 8, 10, 13).to(hip_device), _rand(22, 2, 8, 10, 13).to(hip_device)
    n, c, m = 2, 8, 130
    u, v = ops.cosine_norms(x), ops.cosine_norms(cm)
    rx, rc = ops.selfsim_colsum(x, u), ops.selfsim_colsum(cm, v)
    r = torch.empty_like(rx)
    _guarded(hip_device, "ast_selfsim_colsum_workspace_bytes", (n, c), "ast_selfsim_colsum_f32", _p(x, u, r) + [n, c, m])
    assert _same(r, rx)

    want = ops.selfsim_pairs(x, cm, u, v, rx, rc)
    got = [torch.empty_like(t) for t in want]
    _guarded(hip_device, "ast_selfsim_pairs_workspace_bytes", (n, m), "ast_selfsim_pairs_f32",
             _p(x, cm, u, v, rx, rc, *got) + [n, c, m])
    assert all(_same(a, b) for a, b in zip(got, want))

    loss, sums, state = ops.selfsim_loss(x, cm, weight=0.7)
    g_state, g_sums = [torch.empty_like(t) for t in state], torch.empty_like(sums)
    acc = _lib.loss_accumulator(hip_device, pooled=False)
    _guarded(hip_device, "ast_selfsim_loss_workspace_bytes", (n, c, m), "ast_selfsim_loss_f32",
             _p(x, cm, *g_state, g_sums, acc) + [n, c, m, 0.7])
    assert all(_same(a, b) for a, b in zip(g_state, state)) and _same(g_sums, sums) and _same(acc[0], loss)

    grad = torch.ones((), device=hip_device)
    want_dx = ops.selfsim_loss_backward(x, state, grad, weight=0.7)
    dx = torch.empty_like(x)
    iu, _, irx, _, t, pos, neg = state
    _guarded(hip_device, "ast_selfsim_loss_backward_workspace_bytes", (n, c, m), "ast_selfsim_loss_backward_f32",
             _p(x, iu, irx, t, pos, neg, grad, dx) + [n, c, m, 0.7])
    assert _same(dx, want_dx)


# ---- style swap: C = 8, content 12 x 12 (100 patches), style 14 x 14 (144 patches, 3 tiles) ----

@pytest.fixture(scope="module")
def swap_maps(hip_device):
    content, style = _rand(31, 2, 8, 12, 12).to(hip_device), _rand(32, 2, 8, 14, 14).to(hip_device)
    cc, sc = _labels(33, 2, 2, 10, 10).to(hip_device), _labels(34, 2, 2, 12, 12).to(hip_device)
    return content, style, cc, sc


SWAP_DIMS = (12, 12, 14, 14)


def _patch_norms(dev, style):
    ns, c = int(style.shape[0]), int(style.shape[1])
    inv = torch.empty((ns, 12, 12), device=dev, dtype=torch.float32)
    _guarded(dev, "ast_patch_norms_workspace_bytes", (ns, 14, 14), "ast_patch_norms_f32", _p(style, inv) + [ns, c, 14, 14])
    return inv


@pytest.mark.parametrize("splits", [1, 3])
def test_patch_match(hip_device, swap_maps, splits):
    content, style, _, _ = swap_maps
    inv = _patch_norms(hip_device, style)
    w_index, w_score = ops.patch_match(content, style, return_score=True, _splits=splits)
    index, score = torch.empty_like(w_index), torch.empty_like(w_score)
    _guarded(hip_device, "ast_patch_match_workspace_bytes", (2, 2, *SWAP_DIMS, splits), "ast_patch_match_ex_f32",
             _p(content, style, inv, index, score) + [2, 2, 8, *SWAP_DIMS, splits])
    assert _same(index, w_index) and _same(score, w_score)


def test_style_swap(hip_device, swap_maps):
    content, style, _, _ = swap_maps
    w_out, w_index = ops.style_swap(content, style, alpha=0.6, return_index=True)
    out, index = torch.empty_like(w_out), torch.empty_like(w_index)
    _guarded(hip_device, "ast_style_swap_workspace_bytes", (2, 2, *SWAP_DIMS), "ast_style_swap_f32",
             _p(content, style, style, content, out, index) + [None, 2, 2, 8, *SWAP_DIMS, 0.6])
    assert _same(out, w_out) and _same(index, w_index)


@pytest.mark.parametrize("splits", [1, 3])
def test_patch_match_guided(hip_device, swap_maps, splits):
    content, bank, cc, sc = swap_maps
    inv = _patch_norms(hip_device, bank)
    w_index, w_score = ops.patch_match_guided(content, bank, cc, sc, return_score=True, _splits=splits)
    index, score = torch.empty_like(w_index), torch.empty_like(w_score)
    _guarded(hip_device, "ast_patch_match_guided_workspace_bytes", (2, 2, *SWAP_DIMS, splits),
             "ast_patch_match_guided_ex_f32", _p(content, bank, inv, cc, sc, index, score) + [2, 2, 8, *SWAP_DIMS, splits, 0])
    assert _same(index, w_index) and _same(score, w_score)


def test_style_swap_guided(hip_device, swap_maps):
    content, bank, cc, sc = swap_maps
    w_out, w_index = ops.style_swap_guided(content, bank, cc, sc, alpha=0.6, return_index=True)
    out, index = torch.empty_like(w_out), torch.empty_like(w_index)
    _guarded(hip_device, "ast_style_swap_guided_workspace_bytes", (2, 2, *SWAP_DIMS), "ast_style_swap_guided_f32",
             _p(content, bank, bank, content, cc, sc, out, index) + [None, 2, 2, 8, *SWAP_DIMS, 0.6])
    assert _same(out, w_out) and _same(index, w_index)


# ---- WCT: c = 72 (2 tiles, 3 tile pairs), content 9 x 11, style 7 x 9, n = 2, ns = 1 ----

@pytest.fixture(scope="module")
def wct_maps(hip_device):
    return _rand(41, 2, 72, 9, 11).to(hip_device), _rand(42, 1, 72, 7, 9).to(hip_device)


def test_wct_stages_and_whole(hip_device, wct_maps):
    content, style = wct_maps
    n, ns, c, mc = 2, 1, 72, 99
    (mu_c, cov_c), (mu_s, cov_s) = ops.wct_cov(content), ops.wct_cov(style)
    mean, cov = torch.empty_like(mu_c), torch.empty_like(cov_c)
    _guarded(hip_device, "ast_wct_cov_workspace_bytes", (n, c, mc), "ast_wct_cov_f32",
             _p(content, mean, cov) + [n, c, mc, ops.WCT_EPS_REL])
    assert _same(mean, mu_c) and _same(cov, cov_c)

    covs = torch.cat([cov_c, cov_s])
    w_root, w_iroot = ops.wct_sqrt(covs)
    root, iroot = torch.empty_like(covs), torch.empty_like(covs)
    _guarded(hip_device, "ast_wct_sqrt_workspace_bytes", (n + ns, c), "ast_wct_sqrt_f32",
             _p(covs, root, iroot) + [n + ns, c, 0])
    assert _same(root, w_root) and _same(iroot, w_iroot)

    whole = ops.wct(content, style, alpha=0.6)
    s_root, c_iroot = root[n:].contiguous(), iroot[:n].contiguous()
    out = torch.empty_like(content)
    _guarded(hip_device, "ast_wct_apply_workspace_bytes", (n, c), "ast_wct_apply_f32",
             _p(content, mu_c, mu_s, s_root, c_iroot, out) + [n, ns, c, mc, 0.6])
    assert _same(out, whole)

    out = torch.empty_like(content)
    _guarded(hip_device, "ast_wct_workspace_bytes", (n, ns, c, mc, 63), "ast_wct_f32",
             _p(content, style, out) + [n, ns, c, 9, 11, 7, 9, 0.6, ops.WCT_EPS_REL, 0])
    assert _same(out, whole)


@pytest.mark.parametrize("style_regional", [0, 1])
def test_wct_regions(hip_device, wct_maps, style_regional):
    content, _ = wct_maps
    n, c, k, s = 2, 72, 3, 2
    styles = _rand(43, s, c, 7, 9).to(hip_device)
    labels, slabels = _labels(44, k, n, 9, 11).to(hip_device), _labels(45, k, s, 7, 9).to(hip_device)
    mix = torch.tensor([[[0.25, 0.75], [1.0, 0.0], [0.5, 0.5]]], device=hip_device)
    sl = slabels if style_regional else None

    w_mean, w_cov, w_count = ops.wct_region_cov(content, labels, k)
    mean, cov, count = torch.empty_like(w_mean), torch.empty_like(w_cov), torch.empty_like(w_count)
    _guarded(hip_device, "ast_wct_region_cov_workspace_bytes", (n, c, 9, 11, k), "ast_wct_region_cov_f32",
             _p(content, labels, mean, cov, count) + [n, c, 9, 11, k, ops.WCT_EPS_REL])
    assert _same(mean, w_mean) and _same(cov, w_cov) and _same(count, w_count)

    _, c_iroot = ops.wct_sqrt(w_cov.reshape(n * k, c, c))
    c_iroot = c_iroot.reshape(n, k, c, c)
    if style_regional:
        s_mean, s_cov, s_count = ops.wct_region_cov(styles, slabels, k)
        s_root = ops.wct_sqrt(s_cov.reshape(s * k, c, c))[0].reshape(s, k, c, c)
    else:
        (s_mean, s_cov), s_count = ops.wct_cov(styles), None
        s_root = ops.wct_sqrt(s_cov)[0]
    want = ops.wct_region_apply(content, labels, w_mean, c_iroot, s_mean, s_root, mix, s_count, alpha=0.6)
    out = torch.empty_like(content)
    _guarded(hip_device, "ast_wct_region_apply_workspace_bytes", (n, c, 9, 11, k), "ast_wct_region_apply_f32",
             _p(content, labels, w_mean, c_iroot, s_mean, s_root, mix) + [_lib.ptr(s_count), out.data_ptr(), n, c, 9, 11, k, s,
                                                                         1, style_regional, 0.6])
    assert _same(out, want)

    want = ops.wct_regions(content, labels, styles, mix, style_labels=sl, alpha=0.6)
    out = torch.empty_like(content)
    _guarded(hip_device, "ast_wct_regions_workspace_bytes", (n, c, 9, 11, k, s, 7, 9, style_regional), "ast_wct_regions_f32",
             _p(content, labels, styles) + [_lib.ptr(sl)] + _p(mix, out) + [n, c, 9, 11, k, s, 7, 9, 1, 0.6, ops.WCT_EPS_REL, 0])
    assert _same(out, want)


# ---- EFDM: the chunk-and-merge path (chunk 64), the plane sort with its index, the regional op ----

def test_efdm_general_path(hip_device):
    content, style = _rand(51, 2, 3, 9, 11).to(hip_device), _rand(52, 1, 3, 7, 9).to(hip_device)
    want = ops.efdm(content, style, alpha=0.6, _chunk=64)
    out = torch.empty_like(content)
    _guarded(hip_device, "ast_efdm_ex_workspace_bytes", (2, 1, 3, 99, 63, 64), "ast_efdm_ex_f32",
             _p(content, style, out) + [2, 1, 3, 9, 11, 7, 9, 0.6, 64])
    assert _same(out, want)


def test_plane_sort_with_index(hip_device):
    x = _rand(53, 6, 300).to(hip_device)
    w_vals, w_index = ops.plane_sort(x, return_index=True, _chunk=64)
    vals, index = torch.empty_like(w_vals), torch.empty_like(w_index)
    _guarded(hip_device, "ast_plane_sort_workspace_bytes", (6, 300, 1, 64), "ast_plane_sort_f32",
             _p(x, vals, index) + [6, 300, 64])
    assert _same(vals, w_vals) and _same(index, w_index)


@pytest.mark.parametrize("style_regional", [0, 1])
def test_efdm_regions(hip_device, style_regional):
    n, c, k, s = 2, 8, 3, 2
    content, styles = _rand(54, n, c, 9, 11).to(hip_device), _rand(55, s, c, 7, 9).to(hip_device)
    labels, slabels = _labels(56, k, n, 9, 11).to(hip_device), _labels(57, k, s, 7, 9).to(hip_device)
    mix = torch.tensor([[[0.25, 0.75], [1.0, 0.0], [0.5, 0.5]]], device=hip_device)
    sl = slabels if style_regional else None
    want = ops.efdm_regions(content, labels, styles, mix, style_labels=sl, alpha=0.6)
    out = torch.empty_like(content)
    _guarded(hip_device, "ast_efdm_regions_workspace_bytes", (n, c, 9, 11, k, s, 7, 9), "ast_efdm_regions_f32",
             _p(content, labels, styles) + [_lib.ptr(sl)] + _p(mix, out) + [n, c, 9, 11, k, s, 7, 9, 1, 0.6])
    assert _same(out, want)
