"""CPU: the colour-space surface (model_util's six conversions and three constants, the models
re-exports, the C-ABI argument checks) and the float64 restatement tests/color_ref.py pinned to the
reference values of tests/golden/color.npz. Nothing is launched."""
import numpy as np
import pytest
import torch

import color_ref as CR
from arbitrarystyletransfer_amd import _lib

TAGS = ("s99", "s128")


def test_model_util_surface():
    """The reference's `from model_util import channel_stats, rgb2lab, lab2rgb` (models.py:4) and
    `from model_util import rgb2lab` (data_loader.py:11) work on the drop-in."""
    from arbitrarystyletransfer_amd import model_util, models
    for name in CR.MODES + ("channel_stats",):
        assert callable(getattr(model_util, name)), name
    assert (model_util.ab_norm, model_util.l_norm, model_util.l_cent) == (110, 100, 50)
    assert models.rgb2lab is model_util.rgb2lab and models.lab2rgb is model_util.lab2rgb


def test_mode_codes_match_header():
    import os
    import re
    from arbitrarystyletransfer_amd import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "ast_hip.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"AST_COLOR_(\w+)\s*=\s*(\d+)", header)}
    assert codes == ops.COLOR_MODES and set(codes) == set(CR.MODES)


@pytest.mark.parametrize("call", [
    lambda L: L.ast_color_convert_f32(None, 1, 1, 4, 0, None),
    lambda L: L.ast_color_convert_f32(1, None, 1, 4, 0, None),
    lambda L: L.ast_color_convert_f32(1, 1, 0, 4, 0, None),
    lambda L: L.ast_color_convert_f32(1, 1, 1, 0, 0, None),
    lambda L: L.ast_color_convert_f32(1, 1, 1, 4, 6, None),
    lambda L: L.ast_color_convert_f32(1, 1, 1, 4, -1, None),
    lambda L: L.ast_color_convert_bf16_f32(None, 1, 1, 4, 0, None),
    lambda L: L.ast_color_convert_bf16_f32(1, 1, 0, 4, 0, None),
    lambda L: L.ast_color_convert_bf16_f32(1, 1, 1, 0, 0, None),
    lambda L: L.ast_color_convert_bf16_f32(1, 1, 1, 4, 6, None),
    lambda L: L.ast_color_convert_bf16(1, None, 1, 4, 0, None),
    lambda L: L.ast_color_convert_bf16(1, 1, 0, 4, 0, None),
    lambda L: L.ast_color_convert_bf16(1, 1, 1, 0, 0, None),
    lambda L: L.ast_color_convert_bf16(1, 1, 1, 4, 6, None),
    lambda L: L.ast_color_convert_backward_f32(None, 1, 1, 1, 4, 0, None),
    lambda L: L.ast_color_convert_backward_f32(1, None, 1, 1, 4, 0, None),
    lambda L: L.ast_color_convert_backward_f32(1, 1, None, 1, 4, 0, None),
    lambda L: L.ast_color_convert_backward_f32(1, 1, 1, 0, 4, 0, None),
    lambda L: L.ast_color_convert_backward_f32(1, 1, 1, 1, 0, 0, None),
    lambda L: L.ast_color_convert_backward_f32(1, 1, 1, 1, 4, 6, None),
    lambda L: L.ast_luma_transfer_f32(None, 1, 1, 1, 4, None),
    lambda L: L.ast_luma_transfer_f32(1, None, 1, 1, 4, None),
    lambda L: L.ast_luma_transfer_f32(1, 1, None, 1, 4, None),
    lambda L: L.ast_luma_transfer_f32(1, 1, 1, 0, 4, None),
    lambda L: L.ast_luma_transfer_f32(1, 1, 1, 1, 0, None),
    lambda L: L.ast_luma_transfer_bf16(None, 1, 1, 1, 4, None),
    lambda L: L.ast_luma_transfer_bf16(1, 1, 1, 0, 4, None),
    lambda L: L.ast_luma_transfer_bf16(1, 1, 1, 1, 0, None),
])
def test_color_argument_errors_rejected_before_launch(call):
    assert call(_lib.lib()) < 0


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", CR.MODES)
def test_restatement_matches_reference_float64(golden, tag, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"{tag}_{mode}_x"]).double()
    ref = torch.from_numpy(g[f"{tag}_{mode}_ref64"])
    assert _rel(CR.convert(mode, x), ref) <= 1e-12


@pytest.mark.parametrize("mode", ("rgb2xyz", "rgb2lab", "xyz2lab"))
def test_restatement_nan_in_kind(golden, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"wide_{mode}_x"]).double()
    y = CR.convert(mode, x)
    mask = torch.from_numpy(g[f"wide_{mode}_nan"])
    assert torch.equal(torch.isnan(y), mask)
    ref = torch.from_numpy(g[f"wide_{mode}_ref64"])
    assert _rel(y[~mask], ref[~mask]) <= 1e-12


@pytest.mark.parametrize("mode", ("rgb2lab", "lab2rgb"))
def test_restatement_vjp_matches_reference_autograd(golden, mode):
    g = golden("color")
    x = torch.from_numpy(g[f"grad_{mode}_x"]).double()
    cot = torch.from_numpy(g[f"grad_{mode}_g"]).double()
    ref = torch.from_numpy(g[f"grad_{mode}_g64"])
    assert _rel(CR.vjp(mode, x, cot), ref) <= 1e-12


@pytest.mark.parametrize("mode", CR.MODES)
def test_restatement_vjp_is_the_autograd_of_the_restatement(golden, mode):
    """All six vjps, on the fixture's s99 input of each mode (away from the branch points)."""
    g = golden("color")
    x = torch.from_numpy(g[f"s99_{mode}_x"]).double().requires_grad_(True)
    cot = torch.from_numpy(g["grad_rgb2lab_g"]).double()
    CR.convert(mode, x).backward(cot)
    assert _rel(CR.vjp(mode, x.detach(), cot), x.grad) <= 1e-12


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_luma_transfer(golden, tag):
    g = golden("color")
    s, c = (torch.from_numpy(g[f"luma_{tag}_{k}"]).double() for k in "sc")
    assert _rel(CR.luma_transfer(s, c), torch.from_numpy(g[f"luma_{tag}_ref64"])) <= 1e-12


def test_lab_io_needs_exporting():
    from arbitrarystyletransfer_amd import models
    with pytest.raises(ValueError):
        models.AST(lab_io=True)
    assert models.AST(exporting=True, lab_io=True)._lab_io is True


def test_cpu_tensors_are_rejected():
    from arbitrarystyletransfer_amd import model_util, ops
    x = torch.rand(1, 3, 4, 4)
    with pytest.raises(_lib.HipOpError):
        model_util.rgb2lab(x)
    with pytest.raises(_lib.HipOpError):
        model_util.lab2rgb(x.requires_grad_(True))
    with pytest.raises(_lib.HipOpError):
        ops.luma_transfer(x, x)
    with pytest.raises(_lib.HipOpError):
        ops.color_convert_backward(x, x, "rgb2lab")
    with pytest.raises(_lib.HipOpError):
        ops.color_convert(x, "rgb2hsv")


def test_fixture_is_small():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color.npz")
    assert os.path.getsize(path) < 200 * 1024
    assert np.load(path)["wide_rgb2xyz_nan"].sum() == 246
