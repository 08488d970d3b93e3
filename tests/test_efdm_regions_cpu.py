"""CPU: the definition of regional EFDM (tests/efdm_regions_ref.py) against a brute-force rank count and
against efdm_ref, the fp32 mix against the float64 mix, the C ABI's declarations and argument checks, the
wrappers' host-side validation and the model wiring. No GPU needed: nothing is launched."""
import pytest
import torch

import efdm_ref as ER
import efdm_regions_ref as RR
from arbitrarystyletransfer_amd import _lib, library, models, ops  # noqa: F401  (library registers the ops)

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
OP_TOL = RR.OP_TOL


# ---- the definition and the cases --------------------------------------------------------------------

def _tiny():
    c = ER.features(5101, (2, 2, 4, 5), specials=True)
    s = ER.features(5102, (2, 2, 3, 6), specials=True)
    lab = RR.scatter_labels(5103, (4, 5), [(9, 7), (12, 5)])
    slab = RR.scatter_labels(5104, (3, 6), [(8, 6), (11, 0)])    # style 1 has no region 1
    return c, lab, s, slab


@pytest.mark.parametrize("with_style_labels", [False, True])
def test_reference_equals_the_brute_force_rank_count(with_style_labels):
    c, lab, s, slab = _tiny()
    slab = slab if with_style_labels else None
    eye = torch.eye(2).unsqueeze(0)
    got, valid = RR.efdm_regions(c, lab, s, eye, slab, dtype=torch.float32)
    want = RR.brute_force(c, lab, s, eye, slab).float()
    assert ER.bits_equal(got, want)
    assert valid.tolist() == ([[True, False]] * 2 if with_style_labels else [[True, True]] * 2)
    # a mix, no specials: the same sums in the same order, in float64
    c2, s2 = ER.features(5105, (2, 2, 4, 5)), ER.features(5106, (2, 2, 3, 6))
    mix = torch.tensor([[[.25, .75], [1.0, 0.0]], [[.5, .5], [0.0, 1.0]]])
    got, valid = RR.efdm_regions(c2, lab, s2, mix, slab)
    want = RR.brute_force(c2, lab, s2, mix, slab)
    assert torch.equal(got, want)
    keep = RR.passthrough_mask(lab, valid)[:, None].expand_as(c2)
    assert bool((got[keep] == c2.double()[keep]).all()) and not bool((got[~keep] == c2.double()[~keep]).all())


def test_one_region_one_style_is_plain_efdm_in_bits():
    for name in ("small_specials", "bigger_content", "bigger_style", "64x64"):
        c, s, _ = ER.case_inputs(name)
        s = s[:1]
        lab = torch.zeros((c.shape[0],) + tuple(c.shape[2:]), dtype=torch.uint8)
        got, valid = RR.efdm_regions(c, lab, s, torch.ones(1, 1, 1), dtype=torch.float32)
        assert bool(valid.all()) and ER.bits_equal(got, ER.efdm_target(c, s)), name
        for alpha in (0.6,):
            blend = RR.efdm_regions(c, lab, s, torch.ones(1, 1, 1), alpha=alpha)[0]
            if not bool(torch.isnan(c).any()):
                assert torch.equal(blend, ER.efdm(c, s, alpha)), name


def test_ranks_from_one_whole_plane_sort_equal_the_per_region_ranks():
    """What the kernel does: one stable sort of the whole plane, then the count of earlier sorted positions
    with the same label."""
    c, lab, _, _ = RR.case_inputs("small_specials")
    for b in range(c.shape[0]):
        flat = c[b].reshape(c.shape[1], -1)
        order = torch.sort(ER.keys(flat), dim=1, stable=True).indices
        for ch in range(flat.shape[0]):
            l_sorted = lab[b].reshape(-1)[order[ch]]
            for k in range(2):
                idx = RR.region_index(lab, b, k)
                per_region = torch.sort(ER.keys(flat[ch, idx]), stable=True).indices     # rank -> position in idx
                by_scan = order[ch][l_sorted == k]                                          # rank -> pixel
                assert torch.equal(idx[per_region], by_scan)


def test_cases_have_the_properties_they_are_named_for():
    for name, d in RR.CASES.items():
        c, lab, s, slab = RR.case_inputs(name)
        assert tuple(c.shape) == d["c"] and tuple(s.shape) == d["s"] and c.shape[1] == s.shape[1], name
        assert int((lab == RR.PASS).sum(dim=(1, 2)).min()) > 0 and int((slab == RR.PASS).sum(dim=(1, 2)).min()) > 0
        for b, cnt in enumerate(d["counts"]):
            assert [int((lab[b] == k).sum()) for k in range(d["k"])] == list(cnt) and min(cnt) > 0, name
        for i, cnt in enumerate(d["style_counts"]):
            assert [int((slab[i] == k).sum()) for k in range(d["k"])] == list(cnt) and min(cnt) > 0, name
        assert bool(torch.isnan(c).any()) == d["specials"], name
        assert c.shape[2] * c.shape[3] <= ER.FUSED_MAX and s.shape[2] * s.shape[3] <= ER.FUSED_MAX
    assert RR.CASES["at_fused_max"]["c"][2] * RR.CASES["at_fused_max"]["c"][3] == ER.FUSED_MAX
    for name, mixes in RR.MIXES.items():
        assert not RR.CASES[name]["specials"]
        for v in mixes:
            m = RR.case_mix(name, v)
            assert m.shape[1:] == (RR.CASES[name]["k"], RR.CASES[name]["s"][0]) and bool((m >= 0).all())
            assert float((m.double().sum(dim=2) - 1).abs().max()) <= 1e-6


def test_fp32_mix_against_the_float64_mix():
    """The library's arithmetic (fp32 products and sums) against the float64 reference: the precondition of
    the GPU bar OP_TOL."""
    worst = 0.0
    for name, mixes in RR.MIXES.items():
        c, lab, s, slab = RR.case_inputs(name)
        for v in mixes:
            for sl in (None, slab):
                for alpha in (1.0, 0.6):
                    mix = RR.case_mix(name, v)
                    ref, valid = RR.efdm_regions(c, lab, s, mix, sl, alpha)
                    f32, valid32 = RR.efdm_regions(c, lab, s, mix, sl, alpha, dtype=torch.float32)
                    e = ER.rel_inf(f32, ref)
                    print(f"{name}/{v} style_labels={sl is not None} alpha={alpha}: fp32 vs float64 {e:.2e}")
                    assert bool((valid == valid32).all()) and bool(valid.all())
                    worst = max(worst, e)
    print(f"worst {worst:.2e} (bar {OP_TOL:.0e})")
    assert worst <= OP_TOL


def test_a_zero_weight_style_is_never_read_by_the_reference():
    c, lab, s, slab = RR.case_inputs("bigger_content")
    s_nan = s.clone()
    s_nan[1] = float("nan")
    mix = torch.tensor([[[1.0, 0.0]] * 3])
    got = RR.efdm_regions(c, lab, s_nan, mix, slab, dtype=torch.float32)[0]
    one = RR.efdm_regions(c, lab, s[:1], mix[:, :, :1], slab[:1], dtype=torch.float32)[0]
    assert ER.bits_equal(got, one) and bool(torch.isfinite(got).all())


def test_region_sort_of_the_reference():
    c, lab, s, slab = RR.case_inputs("small_specials")
    bank, count = RR.region_sort(s, slab, 2)
    assert count.tolist() == [list(cnt) for cnt in RR.CASES["small_specials"]["style_counts"]]
    for i in range(s.shape[0]):
        pos = 0
        for k in (0, 1, RR.PASS):
            sel = s[i].reshape(s.shape[1], -1)[:, slab[i].reshape(-1) == k]
            assert ER.bits_equal(bank[i][:, pos:pos + sel.shape[1]], ER.plane_sort(sel)[0])
            pos += sel.shape[1]
        assert pos == 35
    plain, count = RR.region_sort(s, None, 3)
    assert ER.bits_equal(plain.reshape(6, 35), ER.plane_sort(s.reshape(6, 35))[0]) and count.tolist() == [[35, 0, 0]] * 2


# ---- C ABI ---------------------------------------------------------------------------------------------

def test_header_table_and_ops_agree():
    import test_capi
    d = test_capi.declared()
    for name, nargs in (("ast_efdm_region_sort_f32", 10), ("ast_efdm_regions_workspace_bytes", 8),
                        ("ast_efdm_regions_f32", 19)):
        assert d[name] == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name), name
    assert library.OPS[library.OPS.index("plane_sort") + 1] == "efdm_regions"
    assert hasattr(torch.ops.ast_hip, "efdm_regions")
    assert ops.MAX_REGIONS == 8 and ops.MAX_STYLE_ROWS == 64 and ops.EFDM_FUSED_MAX == ER.FUSED_MAX == 16384


P = 256   # a non-null "pointer": every call below must return before anything is launched or read
BIG = 1 << 40


def _sort(L, s=2, c=8, h=4, w=4, k=2, x=P, labels=P, out=P, count=P):
    return L.ast_efdm_region_sort_f32(x, labels, out, count, s, c, h, w, k, None)


def _whole(L, n=2, c=8, hc=4, wc=4, k=2, s=2, hs=4, ws_=4, mix_n=1, ws=P, nbytes=BIG, slab=None, labels=P, content=P,
           styles=P, mix=P, out=P):
    return L.ast_efdm_regions_f32(content, labels, styles, slab, mix, out, n, c, hc, wc, k, s, hs, ws_, mix_n, 1.0, ws,
                                  nbytes, None)


@pytest.mark.parametrize("want,call", [
    (E_SHAPE, lambda L: _sort(L, s=0)),
    (E_SHAPE, lambda L: _sort(L, c=0)),
    (E_SHAPE, lambda L: _sort(L, h=0)),
    (E_SHAPE, lambda L: _sort(L, k=0)),
    (E_SHAPE, lambda L: _sort(L, k=9)),
    (E_SHAPE, lambda L: _sort(L, s=1 << 16, c=1 << 15)),            # 2^31 planes
    (E_UNSUPPORTED, lambda L: _sort(L, h=1, w=16385)),
    (E_UNSUPPORTED, lambda L: _sort(L, h=129, w=128, labels=None)),
    (E_NULL, lambda L: _sort(L, x=None)),
    (E_NULL, lambda L: _sort(L, out=None)),
    (E_NULL, lambda L: _sort(L, count=None)),
    (E_SHAPE, lambda L: _whole(L, n=0)),
    (E_SHAPE, lambda L: _whole(L, c=0)),
    (E_SHAPE, lambda L: _whole(L, wc=0)),
    (E_SHAPE, lambda L: _whole(L, hs=0)),
    (E_SHAPE, lambda L: _whole(L, k=0)),
    (E_SHAPE, lambda L: _whole(L, k=9)),
    (E_SHAPE, lambda L: _whole(L, s=0)),
    (E_SHAPE, lambda L: _whole(L, s=65)),
    (E_SHAPE, lambda L: _whole(L, n=3, mix_n=2)),
    (E_SHAPE, lambda L: _whole(L, n=1 << 16, c=1 << 15)),           # 2^31 planes
    (E_SHAPE, lambda L: _whole(L, nbytes=256)),                     # the bank alone takes 1024 bytes
    (E_SHAPE, lambda L: _whole(L, nbytes=0)),
    (E_UNSUPPORTED, lambda L: _whole(L, hc=1, wc=16385)),
    (E_UNSUPPORTED, lambda L: _whole(L, hs=16385, ws_=1)),
    (E_UNSUPPORTED, lambda L: _whole(L, hs=16385, ws_=1, slab=P)),
    (E_UNSUPPORTED, lambda L: _whole(L, ws=P + 2)),                 # a workspace off 4-byte alignment
    (E_NULL, lambda L: _whole(L, content=None)),
    (E_NULL, lambda L: _whole(L, labels=None)),
    (E_NULL, lambda L: _whole(L, styles=None)),
    (E_NULL, lambda L: _whole(L, mix=None)),
    (E_NULL, lambda L: _whole(L, out=None)),
    (E_NULL, lambda L: _whole(L, ws=None)),
])
def test_bad_arguments_are_rejected_before_launch(want, call):
    assert call(_lib.lib()) == want


def test_workspace_query():
    q = _lib.lib().ast_efdm_regions_workspace_bytes
    assert q(2, 8, 4, 4, 2, 2, 4, 4) == 1024 + 256           # the bank [2, 8, 16] and count [2, 2], 256-byte units
    assert q(8, 512, 64, 64, 8, 4, 64, 64) == 4 * 4 * 512 * 4096 + 256
    assert q(1, 1, 128, 128, 8, 64, 128, 128) == 4 * 64 * 16384 + 2048
    assert q(0, 8, 4, 4, 2, 2, 4, 4) == q(2, 8, 4, 4, 0, 2, 4, 4) == q(2, 8, 4, 4, 9, 2, 4, 4) == E_SHAPE
    assert q(2, 8, 4, 4, 2, 65, 4, 4) == q(2, 8, 4, 4, 2, 0, 4, 4) == q(2, 8, 4, 0, 2, 2, 4, 4) == E_SHAPE
    assert q(2, 8, 129, 128, 2, 2, 4, 4) == q(2, 8, 4, 4, 2, 2, 1, 16385) == E_UNSUPPORTED


# ---- wrappers, registered op, model -----------------------------------------------------------------------

def test_cpu_tensors_are_rejected():
    x, lab = torch.rand(1, 4, 3, 3), torch.zeros(1, 3, 3, dtype=torch.uint8)
    mix = torch.ones(1, 1, 1)
    with pytest.raises(_lib.HipOpError):
        ops.efdm_regions(x, lab, x, mix)
    with pytest.raises(_lib.HipOpError):
        ops.efdm_region_sort(x, lab, 1)
    with pytest.raises(_lib.HipOpError):
        ops.efdm_region_sort(x, None, 1)
    with pytest.raises(_lib.HipOpError, match="regions must be"):
        ops.efdm_region_sort(x, lab, 9)
    with pytest.raises(_lib.HipOpError, match="uint8"):
        ops.efdm_regions(x, lab.int(), x, mix)


def test_meta_kernel_returns_the_content_shape():
    m = torch.device("meta")
    c, s = torch.empty(2, 16, 8, 12, device=m), torch.empty(3, 16, 5, 7, device=m)
    lab, mix = torch.empty(2, 8, 12, dtype=torch.uint8, device=m), torch.empty(1, 2, 3, device=m)
    for slab in (None, torch.empty(3, 5, 7, dtype=torch.uint8, device=m)):
        out = torch.ops.ast_hip.efdm_regions(c, lab, s, mix, slab, 0.6)
        assert out.shape == c.shape and out.dtype == c.dtype and out.device.type == "meta"


class _Relu41Stub(torch.nn.Module):
    """Stands in for the encoder on the CPU: a relu4_1-shaped map, so that the method reaches its label checks
    (which run after the encoder and before any launch)."""

    def forward(self, img):
        return [torch.zeros(img.shape[0], 512, img.shape[2] // 8, img.shape[3] // 8)]


@pytest.mark.parametrize("transform", ["adain", "efdm", "wct"])
def test_model_method_validates_on_the_host_and_raises_under_grad(transform):
    net = models.AdaINStyleTransfer(transform=transform)
    img = torch.zeros(1, 3, 32, 32)
    assert list(net.state_dict()) == list(models.AdaINStyleTransfer().state_dict())
    with pytest.raises(NotImplementedError, match="inference-only"):
        net.stylize_regions_efdm(img, img)
    with torch.no_grad():
        with pytest.raises(ValueError, match="content_img"):
            net.stylize_regions_efdm(img[0], img)
        with pytest.raises(ValueError, match="weights must be"):                     # region_weights
            net.stylize_regions_efdm(img, img, weights=[[1.0, 2.0]])
        with pytest.raises(ValueError, match="single region"):
            net.stylize_regions_efdm(img, img.expand(2, -1, -1, -1), weights=[[1.0, 0.0], [0.0, 1.0]])
        with pytest.raises(ValueError, match="sum to more than 0"):
            net.stylize_regions_efdm(img, img, weights=[[0.0]])
        with pytest.raises(ValueError, match="at most"):
            net.stylize_regions_efdm(img, img.expand(65, -1, -1, -1))
        with pytest.raises(ValueError, match="leave both None"):
            net.stylize_regions_efdm(img, img, labels=models.AutoRegions(2), weights=[[1.0], [1.0]])
        net.encoder = _Relu41Stub()
        lab = torch.zeros(1, 32, 32, dtype=torch.uint8)
        with pytest.raises(ValueError, match="labels must be at the image resolution"):   # _feature_labels
            net.stylize_regions_efdm(img, img, labels=lab[:, :5, :5])
        with pytest.raises(ValueError, match="labels has 2 maps"):
            net.stylize_regions_efdm(img, img, labels=lab.expand(2, -1, -1))
        with pytest.raises(ValueError, match="labels must be a uint8 tensor"):
            net.stylize_regions_efdm(img, img, labels=[[0]])
        with pytest.raises(ValueError, match="style_labels must be at the image resolution"):
            net.stylize_regions_efdm(img, img, labels=lab[:, :4, :4], style_labels=lab[:, :7])   # labels: relu4_1 size


def test_stylize_regions_still_raises_on_an_efdm_model():
    net = models.AdaINStyleTransfer(transform="efdm")
    img = torch.zeros(1, 3, 32, 32)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="stylize_regions_efdm"):
        net.stylize_regions(img, img)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="efdm") as e:
        net.style_statistics(img)
    assert "stylize_regions_efdm" not in str(e.value)
