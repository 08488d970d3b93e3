"""GPU: the colour-space kernels (csrc/color.hip) against the reference values of
tests/golden/color.npz and, beyond the fixture shapes, the float64 restatement tests/color_ref.py.

The forward bar is 8 x noise32, noise32 = max |reference in fp32 - reference in float64| of that
function and shape: a same-formula fp32 implementation carries that rounding noise, the device's
exp2 / log2 are a few ulp where the CPU's pow is about one, and a maximum over a few hundred
samples wanders by about 2x. It is tight enough that the modern sRGB matrix (off by 3.4e-6) fails.
Every test prints its measured ratio to the bar's noise.
"""
import numpy as np
import pytest
import torch

import color_ref as CR
from arbitrarystyletransfer_amd import functional as Fn
from arbitrarystyletransfer_amd import model_util, models, ops, synth

pytestmark = pytest.mark.gpu

TAGS = ("s99", "s128")
FACTOR = 8.0


def _ratio(got, ref64, noise, what):
    """max |got - ref64| / noise over the elements finite in ref64 (printed; the caller asserts)."""
    got = got.detach().double().cpu()
    fin = torch.isfinite(ref64)
    assert torch.isfinite(got[fin]).all(), what
    r = float((got[fin] - ref64[fin]).abs().max()) / float(noise)
    print(f"{what}: max err / noise32 = {r:.2f} (noise32 {float(noise):.2e})")
    return r


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", CR.MODES)
def test_forward_parity(golden, hip_device, tag, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"{tag}_{mode}_x"]).to(hip_device)
    y = getattr(model_util, mode)(x)
    assert y.dtype == torch.float32 and y.shape == x.shape
    r = _ratio(y, torch.from_numpy(g[f"{tag}_{mode}_ref64"]), g[f"{tag}_{mode}_noise32"], f"{mode} {tag}")
    assert r <= FACTOR


# 2 ------------------------------------------------------------------------------------------------
_LARGE = {}


def _large(mode):
    """(fp32 input, float64 restatement, fp32-restatement noise) at (2,3,20,52): HW = 1040, a
    multiple of 4 and more than one pass of a 256-thread block at four elements per thread."""
    if not _LARGE:
        _LARGE["rgb"] = torch.from_numpy(synth.image(911, (2, 3, 20, 52)))
    if mode not in _LARGE:
        x = CR.stage_input(mode, _LARGE["rgb"]).float().contiguous()
        y64 = CR.convert(mode, x.double())
        y32 = CR.convert(mode, x)
        assert y32.dtype == torch.float32
        _LARGE[mode] = (x, y64, float((y32.double() - y64).abs().max()))
    return _LARGE[mode]


@pytest.mark.parametrize("mode", CR.MODES)
def test_forward_larger_shape(hip_device, mode):
    x, y64, noise = _large(mode)
    y = ops.color_convert(x.to(hip_device), mode)
    assert _ratio(y, y64, noise, f"{mode} 2x3x20x52") <= FACTOR


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("rgb2xyz", "rgb2lab", "xyz2lab"))
def test_nan_in_kind(golden, hip_device, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"wide_{mode}_x"]).to(hip_device)
    y = ops.color_convert(x, mode)
    mask = torch.from_numpy(g[f"wide_{mode}_nan"])
    assert mask.any()
    assert torch.equal(torch.isnan(y).cpu(), mask)
    ref = torch.from_numpy(g[f"wide_{mode}_ref64"])
    assert _ratio(y, ref, g[f"wide_{mode}_noise32"], f"{mode} wide (finite part)") <= FACTOR


# 4 ------------------------------------------------------------------------------------------------
def _bf16_ulp(v):
    """One bf16 ulp at |v| (8 significand bits), elementwise, for fp32 v."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", CR.MODES)
def test_bf16(golden, hip_device, tag, mode):
    g = golden("color")
    xb = torch.from_numpy(g[f"{tag}_{mode}_x"]).to(hip_device).to(torch.bfloat16)
    y32 = ops.color_convert(xb.float(), mode)
    yb32 = ops.color_convert(xb, mode)
    assert yb32.dtype == torch.float32
    assert torch.equal(yb32, y32)
    yb = ops.color_convert(xb, mode, out_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16
    want = y32.to(torch.bfloat16).float()
    assert bool(((yb.float() - want).abs() <= _bf16_ulp(want)).all())


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("rgb2lab", "lab2rgb"))
def test_unaligned_base(golden, hip_device, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"s128_{mode}_x"]).to(hip_device)
    buf = torch.empty(x.numel() + 1, device=hip_device, dtype=torch.float32)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 != 0
    assert torch.equal(ops.color_convert(view, mode), ops.color_convert(x, mode))
    s = torch.from_numpy(g["luma_s128_s"]).to(hip_device)
    assert torch.equal(ops.luma_transfer(s, view), ops.luma_transfer(s, x))
    gr = torch.from_numpy(synth.image(941, tuple(x.shape))).to(hip_device) - 0.5
    assert torch.equal(ops.color_convert_backward(view, gr, mode), ops.color_convert_backward(x, gr, mode))


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_round_trip(golden, hip_device, tag):
    x = torch.from_numpy(golden("color")[f"{tag}_rgb2lab_x"]).to(hip_device)
    err = float((model_util.lab2rgb(model_util.rgb2lab(x)) - x).abs().max())
    print(f"round trip {tag}: {err:.2e}")
    assert err <= 1e-5


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("rgb2lab", "lab2rgb"))
def test_backward_fixture(golden, hip_device, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"grad_{mode}_x"]).to(hip_device).requires_grad_(True)
    cot = torch.from_numpy(g[f"grad_{mode}_g"]).to(hip_device)
    getattr(model_util, mode)(x).backward(cot)
    r = _ratio(x.grad, torch.from_numpy(g[f"grad_{mode}_g64"]), g[f"grad_{mode}_noise32"], f"grad {mode}")
    assert r <= FACTOR


@pytest.mark.parametrize("mode", CR.MODES)
def test_backward_all_modes(golden, hip_device, mode):
    """Against the restatement's vjp on (2,3,9,11); noise from its fp32 run, as in test 2."""
    g = golden("color")
    x = torch.from_numpy(g[f"s99_{mode}_x"])
    cot = torch.from_numpy(g["grad_rgb2lab_g"])
    ref64 = CR.vjp(mode, x.double(), cot.double())
    noise = float((CR.vjp(mode, x, cot).double() - ref64).abs().max())
    dx = ops.color_convert_backward(x.to(hip_device), cot.to(hip_device), mode)
    assert _ratio(dx, ref64, noise, f"vjp {mode}") <= FACTOR
    leaf = x.to(hip_device).requires_grad_(True)
    Fn.ColorConvertFn.apply(leaf, mode).backward(cot.to(hip_device))
    assert torch.equal(leaf.grad, dx)


@pytest.mark.parametrize("mode", CR.MODES)
def test_backward_finite_at_black(hip_device, mode):
    x = torch.zeros(1, 3, 4, 6, device=hip_device, requires_grad=True)
    getattr(model_util, mode)(x).sum().backward()
    assert torch.isfinite(x.grad).all()


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_luma_transfer(golden, hip_device, tag):
    g = golden("color")
    s, c = (torch.from_numpy(g[f"luma_{tag}_{k}"]).to(hip_device) for k in "sc")
    assert float(s.min()) < 0 and float(s.max()) > 1   # decoder-like: outside [0, 1]
    y = ops.luma_transfer(s, c)
    assert torch.isfinite(y).all()
    assert _ratio(y, torch.from_numpy(g[f"luma_{tag}_ref64"]), g[f"luma_{tag}_noise32"], f"luma {tag}") <= FACTOR
    err = float((ops.luma_transfer(s, s) - s.clamp(0, 1)).abs().max())
    print(f"luma_transfer(x, x) vs clamp01(x) {tag}: {err:.2e}")
    assert err <= 1e-5
    yb = ops.luma_transfer(s.to(torch.bfloat16), c.to(torch.bfloat16))
    want = ops.luma_transfer(s.to(torch.bfloat16).float(), c.to(torch.bfloat16).float()).to(torch.bfloat16).float()
    assert yb.dtype == torch.bfloat16 and bool(((yb.float() - want).abs() <= _bf16_ulp(want)).all())


# 9 ------------------------------------------------------------------------------------------------
def test_registered_ops(golden, hip_device):
    from arbitrarystyletransfer_amd import library  # noqa: F401  (registers the ast_hip::* custom ops)
    g = golden("color")
    A = torch.ops.ast_hip
    for tag in TAGS:
        x = torch.from_numpy(g[f"{tag}_rgb2lab_x"]).to(hip_device)
        for mode, code in ops.COLOR_MODES.items():
            y = A.color_convert(x, code, False)
            assert torch.equal(y, ops.color_convert(x, mode)) and torch.equal(y, A.color_convert(x, code, False))
        xb = x.to(torch.bfloat16)
        assert torch.equal(A.color_convert(xb, 4, True), ops.color_convert(xb, "rgb2lab", out_dtype=torch.bfloat16))
        s, c = (torch.from_numpy(g[f"luma_{tag}_{k}"]).to(hip_device) for k in "sc")
        y = A.luma_transfer(s, c)
        assert torch.equal(y, ops.luma_transfer(s, c)) and torch.equal(y, A.luma_transfer(s, c))
    x = torch.from_numpy(g["grad_rgb2lab_x"]).to(hip_device)
    torch.library.opcheck(A.color_convert, (x.clone().requires_grad_(True), 4, False))
    torch.library.opcheck(A.color_convert, (x.to(torch.bfloat16), 5, True))
    torch.library.opcheck(A.luma_transfer, (x, x.flip(0)))
    leaf = x.clone().requires_grad_(True)
    cot = torch.from_numpy(g["grad_rgb2lab_g"]).to(hip_device)
    torch.library.opcheck(A.color_convert_backward, (x, cot, 4))
    A.color_convert(leaf, 4, False).backward(cot)
    assert torch.equal(leaf.grad, ops.color_convert_backward(x, cot, "rgb2lab"))


def test_model_util_under_compile(golden, hip_device):
    """Traced, the drop-in functions route to torch.ops.ast_hip.color_convert: no graph break
    (fullgraph raises on one), the eager path's bits, and the registered backward."""
    g = golden("color")
    x = torch.from_numpy(g["grad_rgb2lab_x"]).to(hip_device)
    cot = torch.from_numpy(g["grad_rgb2lab_g"]).to(hip_device)
    torch._dynamo.reset()
    fn = torch.compile(lambda t: model_util.lab2rgb(model_util.rgb2lab(t)), fullgraph=True, backend="aot_eager")
    leaf = x.clone().requires_grad_(True)
    y = fn(leaf)
    y.backward(cot)
    ref = x.clone().requires_grad_(True)
    yr = model_util.lab2rgb(model_util.rgb2lab(ref))
    yr.backward(cot)
    assert torch.equal(y, yr) and torch.equal(leaf.grad, ref.grad)


# 10 -----------------------------------------------------------------------------------------------
def test_adain_preserve_color(hip_device):
    c = torch.from_numpy(synth.image(921, (1, 3, 32, 32))).to(hip_device)
    s = torch.from_numpy(synth.image(922, (1, 3, 32, 32))).to(hip_device)
    net = models.AdaINStyleTransfer().to(hip_device)
    with torch.no_grad():
        plain = net(c, s)
        f_c, f_s = net.encode_pair(c, s)
        parent = net.decoder(net.adain(f_c, f_s, alpha=1.0))   # the forward before the keyword
        assert torch.equal(net(c, s, preserve_color=False), parent) and torch.equal(plain, parent)
        kept = net(c, s, preserve_color=True)
        assert torch.equal(kept, ops.luma_transfer(plain, c))
        assert not torch.equal(kept, plain)
        m, sd = net.style_statistics(s)
        a = net.stylize_with_stats(c, m[0], sd[0], preserve_color=True)
        assert torch.equal(a, ops.luma_transfer(net.stylize_with_stats(c, m[0], sd[0]), c))
    with pytest.raises(NotImplementedError):
        net(c, s, preserve_color=True)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_ast_lab_io(hip_device, dtype):
    c = torch.from_numpy(synth.image(931, (1, 3, 64, 64))).to(hip_device).to(dtype)
    s = torch.from_numpy(synth.image(932, (1, 3, 64, 64))).to(hip_device).to(dtype)
    lab = models.AST(exporting=True, lab_io=True).load_live_init().to(hip_device).to(dtype).eval()
    rgb = models.AST(exporting=True).load_live_init().to(hip_device).to(dtype).eval()
    with torch.no_grad():
        got = lab(c, s)
        inner = rgb(ops.color_convert(c, "rgb2lab", out_dtype=dtype), ops.color_convert(s, "rgb2lab", out_dtype=dtype))
        want = ops.color_convert(inner, "lab2rgb", out_dtype=dtype)
        plain = rgb(c, s)
    assert got.dtype == dtype and torch.equal(got, want)
    assert torch.isfinite(got.float()).all() and not torch.equal(got, plain)
