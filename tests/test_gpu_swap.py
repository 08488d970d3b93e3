"""GPU: style swap (csrc/swap.hip: the style patches' inverse norms, the fused match -- an implicit GEMM
on the fp32 MFMA with a running argmax, the scores never stored -- and the overlap-averaging gather)
and its wrapper / registered-op / model surface, against tests/swap_ref.py.

Bars (swap_ref.py derives them; none comes from the code under test): a returned score is within
OP_TOL * S of the float64 score of the returned index, S the case's largest winning score; the float64
score of the returned index is within 2 * OP_TOL * S of the float64 maximum, for every content patch;
the reconstruction from given indices is within 1e-6 rel_inf of float64 from the same indices. Every
test prints the numbers it asserts on."""
import functools
import gc

import pytest
import torch

import swap_ref as SR
from arbitrarystyletransfer_amd import _lib, library, models, ops, synth  # noqa: F401  (library registers the ops)

pytestmark = pytest.mark.gpu

OP_TOL, GATHER_TOL = SR.OP_TOL, SR.GATHER_TOL
ALPHAS = (1.0, 0.6)


@functools.lru_cache(maxsize=None)
def _case(name):
    return SR.case_inputs(name)


@functools.lru_cache(maxsize=None)
def _ref_scores(name):
    return SR.scores(*_case(name))


def _mismatches(got, ref):
    return int((got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)).sum())


# ---- match ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SR.CASES))
def test_patch_match_against_float64(name, hip_device):
    c, s = _case(name)
    idx, score = ops.patch_match(c.to(hip_device), s.to(hip_device), return_score=True)
    n, _, h, w = c.shape
    ns_patches = (s.shape[2] - 2) * (s.shape[3] - 2)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == tuple(score.shape) == (n, h - 2, w - 2)
    idx, score = idx.cpu(), score.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < ns_patches
    ref = _ref_scores(name)
    e_score, shortfall = SR.check_match(idx, score, ref)
    same = int((idx.reshape(n, -1) == SR.argmax_rows(ref)[0]).sum())
    print(f"patch_match {name}: score error {e_score:.2e} S (bar {OP_TOL:.0e}); index shortfall {shortfall:.2e} S "
          f"(bar {2 * OP_TOL:.0e}); {same} of {idx.numel()} indices are the reference argmax")
    assert e_score <= OP_TOL and shortfall <= 2 * OP_TOL


@pytest.mark.parametrize("offset", [(0, 0), (3, 2), (6, 7)])
def test_planted_crop_is_found(offset, hip_device):
    """The content is an exact crop of the style: every patch's best match is itself."""
    oy, ox = offset
    s = SR.features(9801, (1, 16, 12, 14))
    c = s[:, :, oy:oy + 6, ox:ox + 7].contiguous()
    out, idx = ops.style_swap(c.to(hip_device), s.to(hip_device), return_index=True)
    y, x = torch.meshgrid(torch.arange(4), torch.arange(5), indexing="ij")
    want = ((y + oy) * 12 + (x + ox)).int()
    wrong = int((idx[0].cpu() != want).sum())
    err = SR.rel_inf(out.cpu(), c)
    print(f"planted crop at {offset}: {wrong} wrong indices, swap vs the crop {err:.2e}")
    assert wrong == 0 and err <= OP_TOL


def test_swap_with_itself_is_the_identity(hip_device):
    x = SR.features(9802, (2, 24, 9, 10))
    out, idx = ops.style_swap(x.to(hip_device), x.to(hip_device), return_index=True)
    wrong = int((idx.cpu().reshape(2, -1) != torch.arange(7 * 8).int()).sum())
    err = SR.rel_inf(out.cpu(), x)
    print(f"style_swap(x, x): {wrong} indices off the identity, {err:.2e} from x")
    assert wrong == 0 and err <= OP_TOL


@pytest.mark.parametrize("splits", [1, 2, 5])
def test_exact_ties_take_the_lowest_index(splits, hip_device):
    """A style map of period 40 along x, 82 wide: style patches j and j + 40 are equal bit for bit and
    usually sit in different 64-patch tiles (and splits); the lower one must win every time."""
    base = SR.features(9803, (1, 16, 6, 40))
    s = torch.cat([base, base, base[..., :2]], dim=3)
    c = SR.features(9804, (1, 16, 8, 9))
    assert torch.equal(s[..., :42], s[..., 40:])
    idx, score = ops.patch_match(c.to(hip_device), s.to(hip_device), return_score=True, _splits=splits)
    jx = idx.cpu() % 80
    ref = SR.scores(c, s)
    e_score, shortfall = SR.check_match(idx.cpu(), score.cpu(), ref)
    print(f"periodic style, {splits} split(s): {int((jx >= 40).sum())} of {idx.numel()} indices are the higher "
          f"duplicate; score error {e_score:.2e} S, shortfall {shortfall:.2e} S")
    assert int((jx >= 40).sum()) == 0 and e_score <= OP_TOL and shortfall <= 2 * OP_TOL


def test_zero_patches(hip_device):
    """A zero style patch scores 0 and never wins over a positive score; an all-zero content patch
    ties everywhere at 0 and returns index 0."""
    s = SR.features(9805, (1, 8, 7, 20)) + 0.01
    s[:, :, :3, :5] = 0.0                      # style patches 0, 1, 2 are all zero
    s[:, :, 4:, 10:13] = 0.0                   # and patch 4 * 18 + 10 = 82, in the second tile
    c = SR.features(9806, (1, 8, 6, 6)) + 0.01
    c[:, :, :3, :3] = 0.0                      # content patch 0 is all zero
    idx, score = ops.patch_match(c.to(hip_device), s.to(hip_device), return_score=True)
    idx, score = idx.cpu().flatten(), score.cpu().flatten()
    zero = {0, 1, 2, 82}
    picked_zero = [int(j) for j in idx[1:] if int(j) in zero]
    print(f"zero patches: index of the zero content patch {int(idx[0])} (score {float(score[0])}); positive patches "
          f"that picked a zero style patch: {picked_zero}; smallest winning score {float(score[1:].min()):.3f}")
    assert int(idx[0]) == 0 and float(score[0]) == 0.0
    assert not picked_zero and float(score[1:].min()) > 0


@pytest.mark.parametrize("name", ["c512_split_keys", "c160_tile_tails"])
def test_split_counts_agree_bitwise(name, hip_device):
    c, s = (t.to(hip_device) for t in _case(name))
    i1, s1 = ops.patch_match(c, s, return_score=True, _splits=1)
    i4, s4 = ops.patch_match(c, s, return_score=True, _splits=4)
    i0, s0 = ops.patch_match(c, s, return_score=True)
    bad = [_mismatches(i1, i4), _mismatches(s1, s4), _mismatches(i1, i0), _mismatches(s1, s0)]
    print(f"{name}: 1 split vs 4 vs the library's choice: {bad} mismatches (index, score, index, score)")
    assert bad == [0, 0, 0, 0]


def test_library_splits_the_style_patches_of_a_small_batch():
    n, ns, _, (hc, wc), (hs, ws) = SR.CASES["c512_split_keys"]
    L = _lib.lib()
    auto, one = (L.ast_patch_match_workspace_bytes(n, ns, hc, wc, hs, ws, k) for k in (0, 1))
    print(f"c512_split_keys: workspace {auto} bytes at the library's split count, {one} at one split")
    assert auto > one > 0


# ---- gather and the whole op ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SR.CASES))
def test_gather_and_whole_op_against_float64(name, hip_device):
    c, s = _case(name)
    cd, sd = c.to(hip_device), s.to(hip_device)
    g = torch.Generator().manual_seed(77)
    rnd = torch.randint(0, (s.shape[2] - 2) * (s.shape[3] - 2), (c.shape[0], c.shape[2] - 2, c.shape[3] - 2), generator=g)
    res = []
    for alpha in ALPHAS:
        got = ops.patch_gather(sd, rnd.int().to(hip_device), cd, alpha=alpha).cpu()
        e_g = SR.rel_inf(got, SR.gather(s, rnd, c, alpha))
        out, idx = ops.style_swap(cd, sd, alpha=alpha, return_index=True)
        e_w = SR.rel_inf(out.cpu(), SR.gather(s, idx.cpu().long(), c, alpha))
        print(f"{name} alpha={alpha}: patch_gather on random indices {e_g:.2e}, style_swap vs the reference from its "
              f"own indices {e_w:.2e} (bar {GATHER_TOL:.0e})")
        res += [e_g, e_w]
    assert all(e <= GATHER_TOL for e in res), res


def test_alpha_zero_returns_the_content(hip_device):
    c, s = (t.to(hip_device) for t in _case("c48_k_tails"))
    bad = _mismatches(ops.style_swap(c, s, alpha=0.0), c)
    print(f"alpha = 0: {bad} values differ from the content")
    assert bad == 0


def test_normalized_keys(hip_device):
    """normalize=True matches on the instance-normalised maps (the reference normalises in float64 on
    the CPU) and reconstructs from the raw style features."""
    for name in ("c48_k_tails", "c64_shared_style"):
        c, s = _case(name)
        cd, sd = c.to(hip_device), s.to(hip_device)
        ref = SR.scores(SR.normalize(c), SR.normalize(s))
        idx, score = ops.patch_match(ops.mean_variance_norm(cd), ops.mean_variance_norm(sd), return_score=True)
        e_score, shortfall = SR.check_match(idx.cpu(), score.cpu(), ref)
        out, idx2 = ops.style_swap(cd, sd, alpha=0.6, normalize=True, return_index=True)
        e_out = SR.rel_inf(out.cpu(), SR.gather(s, idx2.cpu().long(), c, 0.6))
        differs = _mismatches(idx2, ops.patch_match(cd, sd))
        print(f"normalize=True {name}: score error {e_score:.2e} S, shortfall {shortfall:.2e} S, output {e_out:.2e}; "
              f"{differs} indices differ from the raw-key match")
        assert e_score <= OP_TOL and shortfall <= 2 * OP_TOL and e_out <= GATHER_TOL
        assert _mismatches(idx, idx2) == 0 and differs > 0


def test_stages_compose_to_the_whole_op(hip_device):
    """ast_style_swap_f32 is ast_patch_norms_f32, ast_patch_match_f32 and ast_patch_gather_f32, bit for
    bit -- with a per-sample style and with a shared one."""
    L = _lib.lib()
    st = _lib.stream_ptr(hip_device)
    for name in ("c48_k_tails", "c64_shared_style", "c512_split_keys"):
        c, s = (t.to(hip_device) for t in _case(name))
        n, ns, ch, (hc, wc), (hs, ws) = SR.CASES[name]
        whole, whole_idx = ops.style_swap(c, s, alpha=0.6, return_index=True)
        nb = L.ast_patch_norms_workspace_bytes(ns, hs, ws)
        mb = L.ast_patch_match_workspace_bytes(n, ns, hc, wc, hs, ws, 0)
        wn = torch.empty(nb, device=hip_device, dtype=torch.uint8)
        wm = torch.empty(mb, device=hip_device, dtype=torch.uint8)
        inv = torch.empty(ns, hs - 2, ws - 2, device=hip_device)
        idx = torch.empty(n, hc - 2, wc - 2, device=hip_device, dtype=torch.int32)
        out = torch.empty_like(c)
        _lib.check(L.ast_patch_norms_f32(s.data_ptr(), inv.data_ptr(), ns, ch, hs, ws, wn.data_ptr(), nb, st), "norms")
        _lib.check(L.ast_patch_match_f32(c.data_ptr(), s.data_ptr(), inv.data_ptr(), idx.data_ptr(), None, n, ns, ch,
                                         hc, wc, hs, ws, wm.data_ptr(), mb, st), "match")
        _lib.check(L.ast_patch_gather_f32(s.data_ptr(), idx.data_ptr(), c.data_ptr(), out.data_ptr(), n, ns, ch, hc, wc,
                                          hs, ws, 0.6, st), "gather")
        e_inv = SR.rel_inf(inv.cpu(), 1.0 / torch.nn.functional.unfold(s.cpu().double(), 3).norm(dim=1).reshape(inv.shape))
        bad = [_mismatches(idx, whole_idx), _mismatches(out, whole)]
        print(f"stages vs whole op, {name}: {bad} mismatches (index, output); inverse norms vs float64 {e_inv:.2e}")
        assert bad == [0, 0] and e_inv <= OP_TOL


@pytest.mark.parametrize("name", list(SR.CASES))
def test_run_twice_bitwise(name, hip_device):
    c, s = (t.to(hip_device) for t in _case(name))
    (o1, i1), (o2, i2) = (ops.style_swap(c, s, alpha=0.6, return_index=True) for _ in range(2))
    s1, s2 = (ops.patch_match(c, s, return_score=True)[1] for _ in range(2))
    bad = [_mismatches(o1, o2), _mismatches(i1, i2), _mismatches(s1, s2)]
    print(f"run to run, {name}: {bad} mismatches (output, index, score)")
    assert bad == [0, 0, 0]


def test_replays_from_a_hip_graph(hip_device):
    """One ops.style_swap call captured on a single stream (no parallel branches) and replayed on new
    inputs: the eager result's bits."""
    c, s = _case("c512_split_keys")
    c2, s2 = SR.features(9811, tuple(c.shape)), SR.features(9812, tuple(s.shape))
    sc, ss = c.to(hip_device), s.to(hip_device)
    eager = [ops.style_swap(a.to(hip_device), b.to(hip_device), alpha=0.6) for a, b in ((c, s), (c2, s2))]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            out = ops.style_swap(sc, ss, alpha=0.6)
    finally:
        gc.enable()
    bad = []
    for (a, b), ref in zip(((c, s), (c2, s2)), eager):
        sc.copy_(a)
        ss.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        bad.append(_mismatches(out, ref))
    print(f"graph replays vs eager: {bad} mismatches")
    assert bad == [0, 0]


@pytest.mark.parametrize("name", ["c48_k_tails", "c64_shared_style"])
def test_a_nan_stays_in_its_sample(name, hip_device):
    c, s = (t.to(hip_device) for t in _case(name))
    clean, clean_idx = ops.style_swap(c, s, alpha=0.6, return_index=True)
    poisoned = c.clone()
    poisoned[0, 3, 2, 1] = float("nan")
    out, idx = ops.style_swap(poisoned, s, alpha=0.6, return_index=True)
    bad = [_mismatches(out[1], clean[1]), _mismatches(idx[1], clean_idx[1])]
    print(f"NaN in sample 0, {name}: sample 1 differs in {bad} (output, index); sample 0 finite: "
          f"{bool(torch.isfinite(out[0]).all())}")
    assert bad == [0, 0] and not bool(torch.isfinite(out[0]).all())
    ns_patches = (s.shape[2] - 2) * (s.shape[3] - 2)
    assert int(idx.min()) >= 0 and int(idx.max()) < ns_patches


def test_wrappers_reject_bad_inputs(hip_device):
    c = torch.rand(1, 4, 5, 5, device=hip_device)
    idx = torch.zeros(1, 3, 3, device=hip_device, dtype=torch.int32)
    for bad in (c.double(), c.half()):
        with pytest.raises(_lib.HipOpError, match="float32"):
            ops.style_swap(bad, c)
        with pytest.raises(_lib.HipOpError, match="float32"):
            ops.patch_match(c, bad)
    with pytest.raises(_lib.HipOpError, match="equal C"):
        ops.style_swap(c, torch.rand(1, 3, 5, 5, device=hip_device))
    with pytest.raises(_lib.HipOpError, match="at least 3"):
        ops.style_swap(c[:, :, :2], c)
    with pytest.raises(_lib.HipOpError, match="style batch"):
        ops.patch_match(c, torch.rand(2, 4, 5, 5, device=hip_device))
    with pytest.raises(_lib.HipOpError, match="unsupported"):
        ops.style_swap(torch.rand(1, 1025, 3, 3, device=hip_device), torch.rand(1, 1025, 3, 3, device=hip_device))
    with pytest.raises(_lib.HipOpError, match="int32"):
        ops.patch_gather(c, idx.long(), c)
    with pytest.raises(_lib.HipOpError, match="int32"):
        ops.patch_gather(c, idx[:, :2], c)


# ---- registered op and model ---------------------------------------------------------------------------

def test_registered_op_matches_and_has_no_backward(hip_device):
    c, s = (t.to(hip_device) for t in _case("c64_shared_style"))
    bad = [_mismatches(torch.ops.ast_hip.style_swap(c, s, 0.6, nrm), ops.style_swap(c, s, alpha=0.6, normalize=nrm))
           for nrm in (False, True)]
    print(f"torch.ops.ast_hip.style_swap vs ops.style_swap: {bad} mismatches")
    assert bad == [0, 0]
    with pytest.raises(NotImplementedError):
        torch.ops.ast_hip.style_swap(c.clone().requires_grad_(), s, 0.6, False).sum().backward()


@pytest.fixture(scope="module")
def net(hip_device):
    return models.AdaINStyleTransfer(transform="wct").to(hip_device).eval()


@pytest.fixture(scope="module")
def imgs(hip_device):
    return (torch.from_numpy(synth.image(7601, (1, 3, 64, 64))).to(hip_device),
            torch.from_numpy(synth.image(7602, (1, 3, 64, 64))).to(hip_device))


def test_model_stylize_swap(net, imgs, hip_device):
    c, s = imgs
    with torch.no_grad():
        f_c, f_s = net.encode_pair(c, s)
        bad = [_mismatches(net.stylize_swap(c, s, alpha=a, normalize=nrm),
                           net.decoder(ops.style_swap(f_c, f_s, alpha=a, normalize=nrm)))
               for a in ALPHAS for nrm in (False, True)]
        y = net.stylize_swap(c, s)
        yc = net.stylize_swap(c, s, preserve_color=True)
        small = net.stylize_swap(c, s[:, :, :48, :40])                 # sizes may differ
        default = models.AdaINStyleTransfer().to(hip_device).eval()    # same seeds: same weights
        other = _mismatches(default.stylize_swap(c, s), y)
        t = models.StyleSwap()(f_c, f_s)
        err = SR.rel_inf(t.cpu(), SR.gather(f_s.cpu(), ops.patch_match(f_c, f_s).cpu().long(), f_c.cpu()))
        own = _mismatches(y, net(c, s))                                # the model's own transform (WCT) differs
    print(f"stylize_swap vs decoder(ops.style_swap(...)): {bad} mismatches; relu4_1 map {tuple(f_c.shape)}; "
          f"transform='wct' vs default model: {other} mismatches; StyleSwap vs float64 from its indices {err:.2e}")
    assert tuple(f_c.shape) == (1, 512, 8, 8) and y.shape == c.shape and bad == [0, 0, 0, 0] and other == 0
    assert bool(torch.isfinite(y).all()) and err <= GATHER_TOL and small.shape == c.shape
    assert yc.shape == c.shape and _mismatches(yc, ops.luma_transfer(y, c)) == 0
    assert own > 0


def test_model_compile_fullgraph_bit_identical(net, imgs):
    torch._dynamo.reset()
    c, s = imgs
    with torch.no_grad():
        ref = net.stylize_swap(c, s, 0.8, True)
        cm = torch.compile(net.stylize_swap, fullgraph=True, dynamic=False)
        out = cm(c, s, 0.8, True)
        out2 = cm(c, s, 0.8, True)
    torch.cuda.synchronize()
    bad = _mismatches(out, ref) + _mismatches(out2, ref)
    print(f"compiled stylize_swap vs eager: {bad} mismatches")
    assert bad == 0


def test_model_raises_under_grad(net, imgs):
    c, s = imgs
    with pytest.raises(NotImplementedError):
        net.stylize_swap(c.clone().requires_grad_(), s)
    with pytest.raises(NotImplementedError):
        net.stylize_swap(c, s)                                          # the parameters ask for a gradient
    f_c, f_s = (t.detach() for t in net.encode_pair(c, s))
    with pytest.raises(NotImplementedError):
        models.StyleSwap()(f_c.requires_grad_(), f_s)
