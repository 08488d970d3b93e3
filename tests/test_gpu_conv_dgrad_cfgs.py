"""Which conv configurations ast_conv3x3_dgrad_f32 takes: the configuration table records, per entry,
whether its kernel has the fused input-gradient epilogue and whether that includes the 2x2-sum
(nearest-upsample adjoint) form. Every configuration index is offered one small input gradient, with
and without the 2x2 sum; the set that launches is pinned, every other index must be refused with
AST_E_UNSUPPORTED before any launch, and every launch must give the input gradient.

The rule the table encodes: 24-35 (split-bf16 kernels) with and without the sum; 18-23 (direct
cin <= 4) and 42, 43 (cin <= 3 MFMA) without it only; everything else refused, 38-41 included. At
this shape the swapped conv reads 16 channels (one K chunk: the smallest the split-bf16 tiles take),
so 18-23, 42 and 43 refuse it in their launchers as well, and the set is 24-35 both times
(test_gpu_parity.py::test_conv3x3_cin3_dgrad_epilogue launches 42 and 43 on a 3-channel gradient).
With AST_CONV_M16 unset (its default, 1) the entry runs an offered 24-27 as 28-31, the same tiles on the
16x16x32 MFMA, so those four indices are launched twice over.

Tolerance: rel_inf <= 5e-5, the bar of tests/test_gpu_dgrad_fused.py, against
functional.conv_input_grad_same (and its 2x2 window sum for upsample 2)."""
import numpy as np
import pytest
import torch

from arbitrarystyletransfer_amd import functional as Fn
from arbitrarystyletransfer_amd import synth
from arbitrarystyletransfer_amd._lib import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
TOL = 5e-5
E_UNSUPPORTED = -3  # AST_E_UNSUPPORTED (include/ast_hip.h)
N, COUT, H, W, CIN = 1, 16, 8, 32, 64
ACCEPTED = {
    1: {24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35},
    2: {24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35},
}


def rel_inf(a, b):
    a = np.asarray(a.detach().cpu(), np.float64)
    b = np.asarray(b.detach().cpu(), np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


@pytest.fixture(scope="module")
def problem(hip_device):
    d = hip_device
    wt = torch.from_numpy(synth.conv_weight(91, COUT, CIN, 3)).to(d)
    dy = torch.from_numpy((synth.uniform(92, N * COUT * H * W) * 2 - 1).astype(np.float32).reshape(N, COUT, H, W)).to(d)
    raw = Fn.conv_input_grad_same(dy, wt)
    ref = {1: raw, 2: raw.reshape(N, CIN, H // 2, 2, W // 2, 2).sum((3, 5))}
    torch.cuda.synchronize()
    return dy, Fn._TF.get(wt), ref


@pytest.mark.parametrize("upsample", [1, 2])
def test_dgrad_configurations(upsample, problem, hip_device):
    dy, wtf, ref = problem
    ncfg = lib().ast_conv3x3_num_configs()
    assert max(ACCEPTED[upsample]) < ncfg
    took = set()
    for cfg in range(ncfg):
        dx = torch.full((N, CIN, H // upsample, W // upsample), float("nan"), device=hip_device)
        rc = lib().ast_conv3x3_dgrad_f32(cfg, ptr(dy), ptr(wtf), ptr(dx), None, None, None, N, COUT, H, W, CIN,
                                         upsample, stream_ptr(hip_device))
        torch.cuda.synchronize()
        if rc == 0:
            took.add(cfg)
            err = rel_inf(dx, ref[upsample])
            print(f"dgrad cfg {cfg} upsample {upsample}: rel_inf {err:.2e} (bar {TOL:.0e})")
            assert err <= TOL, (cfg, err)
        else:
            assert rc == E_UNSUPPORTED, (cfg, rc)
    assert took == ACCEPTED[upsample], sorted(took ^ ACCEPTED[upsample])
