"""CPU self-test of the stage bounds of tests/mb_stage_ref.py (no GPU): a torch restatement of the
bf16 inference block with the kernels' rounding points (bf16 hidden values and depthwise taps, fp32
accumulation, the SE pool summed before the output rounding, bf16 D, wg and out: the v5 pipeline of
csrc/mb_ed5.hip, the superset) stays inside every bound, and each injected fault leaves at least
one. This pins the sensitivity of the GPU stage tests (tests/test_gpu_mb_stages.py), which run the
same checks on the kernels' outputs.

The restatement is not the project's kernels; its err/bound figures are simulated ones.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import mb_stage_ref as S

BF = torch.bfloat16

SHAPES = {
    # name: cin, ratio, k, (n, h, w), up. All identity blocks (stride 1, cout == cin) so that the
    # residual fault applies; output widths > 28 (two strips) and <= 60; hid and cout off the padding
    # multiples (32 and 16) so that wg has padding rows and columns.
    "k5": (20, 3, 5, (1, 12, 32), 1),        # hid 60 (hid_pad 64), cout 20 (cout_pad 32)
    "k3": (24, 3, 3, (2, 10, 30), 1),        # hid 72 (hid_pad 96), cout 24 (cout_pad 32)
    "ratio1_up2": (24, 1, 3, (1, 6, 16), 2),  # output 12 x 32, residual upsampled
    "ratio1_up1": (24, 1, 3, (1, 12, 32), 1),
}

FAULTS = ["replicate_pad", "dup_col0", "zero_tap", "drop_dw_bias", "pool_no_last_col", "pool_no_last_strip",
          "zero_last_channel", "wg_padding_nonzero", "no_residual"]


def rnd(g, *shape, scale=1.0, shift=0.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale + shift


def make_block(name):
    cin, t, k, (n, h, w), up = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    hid, cout, red = cin * t, cin, 8
    x = (torch.rand(n, cin, h, w, generator=g) * 2 - 0.7).to(BF)
    w1 = b1 = None
    if t != 1:
        w1 = rnd(g, hid, cin, scale=math.sqrt(6.0 / cin)).to(BF)   # the packed expand weights are bf16
        b1 = rnd(g, hid, scale=0.3)
    wd = rnd(g, hid, k * k, scale=math.sqrt(6.0 / (k * k)))
    bd = rnd(g, hid, scale=0.2, shift=0.3)
    fc1w, fc1b = rnd(g, red, hid, scale=0.5 / math.sqrt(hid)), rnd(g, red, scale=0.1, shift=0.5)
    fc2w, fc2b = rnd(g, hid, red, scale=0.5 / math.sqrt(red)), rnd(g, hid, scale=0.1, shift=0.5)
    w2, b2 = rnd(g, cout, hid, scale=math.sqrt(6.0 / hid)), rnd(g, cout, scale=0.2)
    return S.operands(x, w1, b1, wd, bd, fc1w, fc1b, fc2w, fc2b, w2, b2, k, 1, up, True, S.U_BF16)


def hs32(v):
    return v * torch.clamp(v * (1.0 / 6.0) + 0.5, 0.0, 1.0)


def restate(op, fault=None):
    """The block in fp32 torch with the v5 rounding points; `fault` injects one defect."""
    f32 = lambda t: t.float()  # noqa: E731
    k, p = op.k, (op.k - 1) // 2
    hid, cout = op.hid, op.cout
    x = f32(op.x)
    if op.w1 is not None:
        h = hs32(torch.einsum("oc,nchw->nohw", f32(op.w1), x) + f32(op.b1).view(1, -1, 1, 1)).to(BF).float()
    else:
        h = S.upsample2(x) if op.up == 2 else x
    wd = f32(op.wd).to(BF).float().reshape(hid, 1, k, k).clone()
    bd = f32(op.bd).clone()
    if fault == "zero_tap":
        wd[-1, 0, p, p] = 0.0
    if fault == "drop_dw_bias":
        bd[-1] = 0.0
    hp = F.pad(h, (p, p, p, p), mode="replicate" if fault == "replicate_pad" else "reflect")
    dpre = hs32(F.conv2d(hp, wd, bd, groups=hid))
    if fault == "dup_col0":
        dpre[..., 0] = dpre[..., 1]
    if fault == "zero_last_channel":
        dpre[:, -1] = 0.0
    wo = dpre.shape[3]
    pooled = dpre
    if fault == "pool_no_last_col":
        pooled = dpre[..., :wo - 1]
    if fault == "pool_no_last_strip":
        pooled = dpre[..., :(wo - 1) // 28 * 28]
    pool = pooled.sum(dim=(2, 3))
    d = dpre.to(BF)
    mean = pool / float(dpre.shape[2] * wo)
    gate = torch.clamp(torch.relu(mean @ f32(op.fc1w).T + f32(op.fc1b)) @ f32(op.fc2w).T + f32(op.fc2b), 0.0, 1.0)
    hid_pad, cout_pad = (hid + 31) // 32 * 32, (cout + 15) // 16 * 16
    assert hid_pad > hid and cout_pad > cout
    wg = torch.zeros(x.shape[0], cout_pad, hid_pad)
    wg[:, :cout, :hid] = f32(op.w2).unsqueeze(0) * gate.unsqueeze(1)
    wg = wg.to(BF)
    if fault == "wg_padding_nonzero":
        wg[-1, cout_pad - 1, hid_pad - 1] = 2.0 ** -20
    out = torch.einsum("nok,nkhw->nohw", wg[:, :cout, :hid].float(), d.float()) + f32(op.b2).view(1, -1, 1, 1)
    if fault != "no_residual":
        out = out + (S.upsample2(x) if op.up == 2 else x)
    return d, pool, wg, out.to(BF)


@pytest.fixture(scope="module")
def blocks():
    return {name: make_block(name) for name in SHAPES}


@pytest.mark.parametrize("name", list(SHAPES))
def test_restatement_inside_every_bound(name, blocks):
    op = blocks[name]
    rep = S.stage_report(op, *restate(op))
    print(name, {k: f"{v:.3g}" for k, v in S.ratios(rep).items()})
    S.assert_stages(rep, name)
    # not vacuous: the roundings are there, so the restatement is not exact either
    assert S.ratios(rep)["D"] > 1e-3 and S.ratios(rep)["out"] > 1e-3


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_fault_breaks_a_bound(name, fault, blocks):
    op = blocks[name]
    good, bad = restate(op), restate(op, fault)
    if fault == "replicate_pad" and op.up == 2:
        # After a nearest x2 upsample rows (columns) 0 and 1 are copies of each other, so the
        # 1-pixel reflection (row 1) and the replication (row 0) pad with the same values: this
        # fault does not exist at this shape. ratio1_up1 is the ratio-1 shape that carries it.
        assert all(torch.equal(a, b) for a, b in zip(good, bad))
        return
    assert not all(torch.equal(a, b) for a, b in zip(good, bad)), "the fault changed nothing"
    rep = S.stage_report(op, *bad)
    broken = {k: v for k, v in S.ratios(rep).items() if not v <= 1.0}
    print(name, fault, {k: f"{v:.3g}" for k, v in broken.items()})
    assert broken, f"{fault} at {name} stayed inside every bound: {S.ratios(rep)}"
    assert S.failures(rep)


def test_check_reports_where():
    ref = torch.zeros(1, 3, 40, 60, dtype=torch.float64)
    got = ref.clone()
    got[0, 2, 33, 57] = 1.0
    worst, msg = S.check("probe", got, ref, torch.full_like(ref, 0.25))
    assert worst == 4.0
    assert "index (0, 2, 33, 57)" in msg and "channel 2" in msg and "band 1, strip 2" in msg and "err/bound 4" in msg
    got[0, 0, 0, 0] = float("nan")
    assert S.check("probe", got, ref, torch.full_like(ref, 0.25))[0] == math.inf
    # a zero bound demands exactness
    assert S.check("probe", ref, ref, torch.zeros_like(ref)) == (0.0, None)
    assert S.check("probe", ref + 1e-30, ref, torch.zeros_like(ref))[0] == math.inf
