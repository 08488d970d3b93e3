"""GPU: exact feature distribution matching (csrc/efdm.hip: the fused kernel, the chunk-sort + merge
path, plane_sort), its autograd / registered-op / model / loss surface, against the CPU restatement
tests/efdm_ref.py, which test_efdm_cpu.py pins to a brute-force rank count.

At alpha = 1 every output is a copy of a style value, so parity is bit for bit (int32 views are
compared). The alpha blend is held to OP_TOL, the project's single-op bar (test_gpu_parity.py),
against the float64 blend of the bit-exact target; the same blend in float32 on the CPU sits at
3e-8 (test_efdm_cpu.py asserts 2e-7). Every test prints what it asserts on."""
import functools
import gc

import pytest
import torch

import efdm_ref as ER
from arbitrarystyletransfer_amd import _lib, library, losses, models, ops, synth  # noqa: F401  (library registers the ops)
from arbitrarystyletransfer_amd import functional as Fn

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5
# tests/test_gpu_hist.py:78-79 holds pixel_mse_loss (the sqdiff kernel) to 1e-5, value and gradient
SQDIFF_TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _case(name):
    return ER.case_inputs(name)


@functools.lru_cache(maxsize=None)
def _target(name):
    c, s, _ = _case(name)
    return ER.efdm_target(c, s)


def _mismatches(got, ref):
    return int((got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)).sum())


# ---- plane_sort --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sort_case(m):
    x = ER.features(5000 + m, (3, m), specials=True)
    return (x,) + ER.plane_sort(x)


@pytest.mark.parametrize("m,chunk", [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (1000, 0), (4096, 0), (4097, 0),
                                     (1000, 256), (4097, 256)])
def test_plane_sort_bit_equal(m, chunk, hip_device):
    x, ref_v, ref_i = _sort_case(m)
    vals, idx = ops.plane_sort(x.to(hip_device), return_index=True, _chunk=chunk)
    only = ops.plane_sort(x.to(hip_device), _chunk=chunk)
    bad_v, bad_i, bad_o = _mismatches(vals.cpu(), ref_v), int((idx.cpu() != ref_i).sum()), _mismatches(only.cpu(), ref_v)
    print(f"plane_sort M={m} chunk={chunk}: {bad_v} value, {bad_i} index, {bad_o} values-only mismatches of {3 * m}")
    assert idx.dtype == torch.int32 and vals.shape == idx.shape == (3, m)
    assert bad_v == 0 and bad_i == 0 and bad_o == 0


def test_plane_sort_of_a_feature_map_and_its_registered_op(hip_device):
    x = ER.features(5100, (2, 3, 9, 11), specials=True)
    ref_v, ref_i = ER.plane_sort(x.reshape(6, 99))
    vals, idx = torch.ops.ast_hip.plane_sort(x.to(hip_device))
    bad = _mismatches(vals.cpu().reshape(6, 99), ref_v) + int((idx.cpu().reshape(6, 99) != ref_i).sum())
    print(f"plane_sort op on (2,3,9,11): {bad} mismatches")
    assert vals.shape == idx.shape == x.shape and bad == 0


# ---- efdm, alpha = 1: bit for bit ----------------------------------------------------------------

@pytest.mark.parametrize("name", list(ER.CASES))
def test_efdm_bit_equal(name, hip_device):
    c, s, chunk = _case(name)
    got = ops.efdm(c.to(hip_device), s.to(hip_device), _chunk=chunk).cpu()
    bad = _mismatches(got, _target(name))
    print(f"efdm {name} chunk={chunk}: {bad} of {c.numel()} values differ in bits")
    assert got.shape == c.shape and bad == 0
    # every output plane is a sub-multiset of its style plane: values are copied, never computed
    sp = s.expand(c.shape[0], -1, -1, -1).reshape(c.shape[0] * c.shape[1], -1).view(torch.int32)
    for p, row in enumerate(got.reshape(sp.shape[0], -1).view(torch.int32)):
        assert bool(torch.isin(row, sp[p]).all()), (name, p)


def test_paths_agree(hip_device):
    """The same inputs through the fused kernel and through chunk sorts of 64 and 256: equal bits."""
    c, s, _ = _case("64x64")
    c, s = c.to(hip_device), s.to(hip_device)
    fused = ops.efdm(c, s)
    for chunk in (64, 256, 4096):
        bad = _mismatches(ops.efdm(c, s, _chunk=chunk), fused)
        print(f"fused vs chunk={chunk}: {bad} mismatches")
        assert bad == 0
    assert _mismatches(fused.cpu(), _target("64x64")) == 0


def test_constant_content_plane_ranks_by_index(hip_device):
    """All-equal content: rank = index, so the output is the sorted style plane itself."""
    s = ER.features(5200, (1, 2, 12, 12))
    c = torch.full((1, 2, 12, 12), 0.5)
    c[0, 1] = 0.0
    for chunk in (0, 64):
        got = ops.efdm(c.to(hip_device), s.to(hip_device), _chunk=chunk).cpu()
        ref = ER.plane_sort(s.reshape(2, 144))[0].reshape(1, 2, 12, 12)
        bad = _mismatches(got, ref) + _mismatches(got, ER.efdm_target(c, s))
        print(f"constant content, chunk={chunk}: {bad} mismatches")
        assert bad == 0


def _offset_view(t):
    """t's values in storage that starts one element past an aligned address."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("name", ["64x64", "chunked_25x40"])
def test_unaligned_bases(name, hip_device):
    c, s, chunk = _case(name)
    c, s = c.to(hip_device), s.to(hip_device)
    ref = ops.efdm(c, s, alpha=0.3, _chunk=chunk)
    cv, sv, ov = _offset_view(c), _offset_view(s), _offset_view(torch.zeros_like(c))
    assert cv.data_ptr() % 16 == 4 and sv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
    n, ch, hc, wc = c.shape
    L = _lib.lib()
    nbytes = L.ast_efdm_ex_workspace_bytes(n, s.shape[0], ch, hc * wc, s.shape[2] * s.shape[3], chunk)
    ws = torch.empty(max(1, nbytes), device=hip_device, dtype=torch.uint8)
    _lib.check(L.ast_efdm_ex_f32(cv.data_ptr(), sv.data_ptr(), ov.data_ptr(), n, s.shape[0], ch, hc, wc, s.shape[2],
                                 s.shape[3], 0.3, chunk, ws.data_ptr(), nbytes, _lib.stream_ptr(hip_device)), "efdm")
    bad = _mismatches(ov, ref) + _mismatches(ops.efdm(cv, sv, alpha=0.3, _chunk=chunk), ref)
    print(f"unaligned bases, {name}: {bad} mismatches")
    assert bad == 0


def test_plain_entry_point_is_the_automatic_path(hip_device):
    c, s, _ = _case("bigger_content")
    c, s = c.to(hip_device), s.to(hip_device)
    out = torch.empty_like(c)
    n, ch, hc, wc = c.shape
    assert _lib.lib().ast_efdm_workspace_bytes(n, n, ch, hc * wc, 256) == 0
    _lib.check(_lib.lib().ast_efdm_f32(c.data_ptr(), s.data_ptr(), out.data_ptr(), n, n, ch, hc, wc, 16, 16, 1.0,
                                       None, 0, _lib.stream_ptr(hip_device)), "efdm")
    bad = _mismatches(out.cpu(), _target("bigger_content"))
    print(f"ast_efdm_f32 with no workspace: {bad} mismatches")
    assert bad == 0


def test_wrappers_reject_other_dtypes_and_devices_mismatch(hip_device):
    c = torch.rand(1, 2, 4, 4, device=hip_device)
    for bad in (c.double(), c.half(), c.to(torch.bfloat16)):
        with pytest.raises(_lib.HipOpError, match="float32"):
            ops.efdm(bad, c)
        with pytest.raises(_lib.HipOpError, match="float32"):
            ops.efdm(c, bad)
        with pytest.raises(_lib.HipOpError, match="float32"):
            ops.plane_sort(bad)
    with pytest.raises(_lib.HipOpError, match="EFDM needs"):
        ops.efdm(c, torch.rand(1, 3, 4, 4, device=hip_device))
    with pytest.raises(_lib.HipOpError):
        ops.efdm(c, c, _chunk=100)


# ---- alpha blend ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["64x64", "bigger_content", "chunked_sizes_differ"])
def test_efdm_alpha_blend(name, hip_device):
    c, s, chunk = _case(name)
    ref = ER.efdm(c, s, 0.3, torch.float64)
    got = ops.efdm(c.to(hip_device), s.to(hip_device), alpha=0.3, _chunk=chunk).cpu()
    err = ER.rel_inf(got, ref)
    print(f"efdm alpha=0.3 {name}: rel_inf {err:.2e}")
    assert err <= OP_TOL


# ---- determinism -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["64x64", "chunked_4097"])
def test_run_to_run_determinism(name, hip_device):
    c, s, chunk = _case(name)
    c, s = c.to(hip_device), s.to(hip_device)
    a = ops.efdm(c, s, alpha=0.3, _chunk=chunk)
    b = ops.efdm(c, s, alpha=0.3, _chunk=chunk)
    bad = _mismatches(a, b)
    print(f"run to run, {name}: {bad} mismatches")
    assert bad == 0


# ---- autograd, registered op, compile, graph -------------------------------------------------------

def test_autograd_is_straight_through(hip_device):
    c, s, _ = _case("bigger_content")
    g = torch.randn(c.shape, generator=torch.Generator().manual_seed(5300)).to(hip_device)
    res = []
    for fn in (lambda a, b: Fn.EFDMFn.apply(a, b, 0.3), lambda a, b: torch.ops.ast_hip.efdm(a, b, 0.3),
               lambda a, b: models.EFDM()(a, b, alpha=0.3)):
        cs, ss = c.to(hip_device).requires_grad_(), s.to(hip_device).requires_grad_()
        out = fn(cs, ss)
        (out * g).sum().backward()
        print(f"grad mismatches {_mismatches(cs.grad, g)}, style grad {ss.grad}")
        assert _mismatches(cs.grad, g) == 0 and ss.grad is None
        res.append(out.detach())
    plain = ops.efdm(c.to(hip_device), s.to(hip_device), alpha=0.3)
    assert all(_mismatches(r, plain) == 0 for r in res)
    assert _mismatches(torch.ops.ast_hip.efdm(c.to(hip_device), s.to(hip_device), 1.0).cpu(),
                       _target("bigger_content")) == 0


def test_compile_fullgraph_efdm_module(hip_device):
    """As test_gpu_dispatch.py does for the AdaIN model: fullgraph raises on a graph break, and the
    compiled module (torch.ops.ast_hip.efdm) gives the eager path's bits."""
    torch._dynamo.reset()
    c, s, _ = _case("bigger_content")
    c, s = c.to(hip_device), s.to(hip_device)
    m = models.EFDM()
    with torch.no_grad():
        ref = m(c, s, 0.8)
        cm = torch.compile(m, fullgraph=True, dynamic=False)
        out = cm(c, s, 0.8)
    torch.cuda.synchronize()
    bad = _mismatches(out, ref)
    print(f"compiled EFDM vs eager: {bad} mismatches")
    assert bad == 0


def test_general_path_replays_from_a_hip_graph(hip_device):
    """One ops.efdm call on the chunk-sort + merge path captured the way train.StepGraph captures a
    step, replayed on new inputs: the eager result's bits."""
    c, s, chunk = _case("chunked_25x40")
    c2, s2 = ER.features(5400, tuple(c.shape)), ER.features(5401, tuple(s.shape))
    sc, ss = c.to(hip_device), s.to(hip_device)
    eager = [ops.efdm(a.to(hip_device), b.to(hip_device), alpha=0.3, _chunk=chunk) for a, b in ((c, s), (c2, s2))]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            out = ops.efdm(sc, ss, alpha=0.3, _chunk=chunk)
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


# ---- model -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets(hip_device):
    c = torch.from_numpy(synth.image(5501, (2, 3, 64, 64))).to(hip_device)
    s = torch.from_numpy(synth.image(5502, (2, 3, 64, 64))).to(hip_device)
    return dict(efdm=models.AdaINStyleTransfer(transform="efdm").to(hip_device).eval(),
                adain=models.AdaINStyleTransfer().to(hip_device).eval(), c=c, s=s)


def test_model_efdm_forward(nets):
    net, c, s = nets["efdm"], nets["c"], nets["s"]
    with torch.no_grad():
        f_c, f_s = net.encode_pair(c, s)
        t = net.adain(f_c, f_s)
        ref_t = ER.efdm_target(f_c.cpu(), f_s.cpu())
        bad_t = _mismatches(t.cpu(), ref_t)
        y = net(c, s)
        bad_y = _mismatches(y, net.decoder(ref_t.to(c.device)))
        y3 = net(c, s, alpha=0.3)
        bad_3 = _mismatches(y3, net.decoder(ops.efdm(f_c, f_s, alpha=0.3)))
        yc = net(c, s, preserve_color=True)
    print(f"model: transform {bad_t}, forward {bad_y}, alpha {bad_3} mismatches; relu4_1 map {tuple(f_c.shape)}")
    assert tuple(f_c.shape) == (2, 512, 8, 8) and y.shape == c.shape
    assert bad_t == 0 and bad_y == 0 and bad_3 == 0
    assert yc.shape == c.shape and bool(torch.isfinite(yc).all()) and _mismatches(yc, ops.luma_transfer(y, c)) == 0
    with torch.no_grad():
        for call in (lambda: net.style_statistics(s), lambda: net.stylize_with_stats(c, f_s[0, :, 0, 0], f_s[0, :, 0, 0]),
                     lambda: net.stylize_regions(c, s)):
            with pytest.raises(NotImplementedError):
                call()


def test_model_default_is_unchanged(nets):
    net, c, s = nets["adain"], nets["c"], nets["s"]
    with torch.no_grad():
        f_c, f_s = net.encode_pair(c, s)
        bad = [_mismatches(net(c, s, alpha=a), net.decoder(ops.adain(f_c, f_s, alpha=a))) for a in (1.0, 0.8)]
        bad.append(_mismatches(net.encoder(c)[0], nets["efdm"].encoder(c)[0]))
    print(f"default model vs decoder(ops.adain(...)): {bad} mismatches")
    assert isinstance(net.adain, models.AdaIN) and net.transform == "adain" and bad == [0, 0, 0]


def test_efdm_decoder_trains_through_the_model(nets, hip_device):
    """What AdaINTrainer does with self.net.adain(f_c, f_s): the gradient reaches the decoder, and
    the content features get the decoder's input gradient unchanged."""
    net = models.AdaINStyleTransfer(transform="efdm").to(hip_device)
    f_c, f_s = (t.detach().clone().requires_grad_() for t in nets["efdm"].encode_pair(nets["c"], nets["s"]))
    t = net.adain(f_c, f_s)
    t.retain_grad()
    net.decoder(t).square().mean().backward()
    w = net.decoder.convs()[0].weight
    print(f"decoder grad norm {float(w.grad.norm()):.3e}")
    assert f_s.grad is None and _mismatches(f_c.grad, t.grad) == 0 and float(w.grad.norm()) > 0


# ---- loss ------------------------------------------------------------------------------------------

def test_compute_efdm_loss(hip_device):
    f, s = ER.features(5600, (2, 8, 16, 16)) + 0.25, ER.features(5601, (2, 8, 16, 16))
    tgt = ER.efdm_target(f, s).double()
    ref = 2.5 * ((f.double() - tgt) ** 2).mean()
    ref_grad = 2.5 * 2.0 * (f.double() - tgt) / f.numel()
    fd, sd = f.to(hip_device).requires_grad_(), s.to(hip_device).requires_grad_()
    loss = losses.compute_efdm_loss(fd, sd, 2.5)
    loss.backward()
    loss = loss.detach()
    ev = abs(float(loss) - float(ref)) / float(ref)
    eg = ER.rel_inf(fd.grad.cpu(), ref_grad)
    print(f"efdm loss {float(loss):.6f} vs {float(ref):.6f}: rel {ev:.2e}; gradient rel_inf {eg:.2e}")
    assert ev <= SQDIFF_TOL and eg <= SQDIFF_TOL and sd.grad is None
    assert abs(float(losses.compute_efdm_loss(fd.detach(), sd.detach())) - float(ref) / 2.5) <= SQDIFF_TOL * float(ref)
