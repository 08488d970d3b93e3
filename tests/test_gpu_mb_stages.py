"""Stage-level parity of the inference MobileNet block kernels (csrc/mobilenet.hip, mb_ed4.hip,
mb_ed5.hip): every stage of a block -- ast_mb_expand_dw (D and the SE-pool sums), ast_mb_se_fold
(wg), ast_mb_pw (out) and ast_mb_expand_gemm -- against a float64 reference of the same stage with
a derived per-element bound (tests/mb_stage_ref.py; self-tested without a GPU in
tests/test_mb_stage_bounds_cpu.py). The whole-block bars of test_gpu_mobilenet.py (2e-2 of max|ref|
after the SE gate and a sum over the hidden channels) stay as a sanity check; these are the parity
checks of the kernels.

The stage launches copy DepthWiseConv.run (mobilenetv2.py); the fused pair is not used, so D exists.
Every output buffer starts as NaN, so an element a kernel does not write is outside its bound.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mb_stage_ref as S
from arbitrarystyletransfer_amd import mobilenetv2 as M
from arbitrarystyletransfer_amd import synth
from arbitrarystyletransfer_amd._lib import check, lib, ptr, stream_ptr
from arbitrarystyletransfer_amd.mobilenetv2 import DTYPE_CODE, DepthWiseConv

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32

# name: (family, inp, oup, stride, ratio, k, use_norm, use_identity, (n, h, w), up, split)
# The family is the kernel the dispatch selects for bf16 (launch_ed4 in mb_ed4.hip, launch_ed5 in
# mb_ed5.hip, dispatch_ed in mobilenet.hip). Pool cases keep the output within 60 x 60, so that one
# lost row or column moves a pool sum by more than the pool-vs-own-D bound.
CASES = {
    # v5, expand_dw5_kernel<KS> (k5, stride 1, cin_pad <= 48, wo % 4 == 0); tiles of 32 rows x 28
    # columns, hidden channels in chunks of 32
    "v5_ks1_one_tile": ("v5", 16, 16, 1, 4, 5, True, True, (2, 32, 28), 1, False),       # KS 1, hid 64, exactly one tile
    "v5_ks2_hid60_37x60": ("v5", 20, 16, 1, 3, 5, False, True, (1, 37, 60), 1, False),   # KS 2, cin 20 < cin_pad 32; hid 60:
    #   a partial last chunk; ragged second band (5 rows); three strips, the last 4 columns wide
    "v5_ks2_5x8": ("v5", 24, 24, 1, 6, 5, False, True, (1, 5, 8), 1, False),             # KS 2, cin 24 < 32; smaller than a tile
    "v5_ks3_hid240": ("v5", 40, 24, 1, 6, 5, True, True, (1, 33, 40), 1, False),         # KS 3, cin 40 < 48; hid 240: a
    #   half-filled last chunk; 1-row second band
    "v5_ks3_hid160_37x60": ("v5", 40, 40, 1, 4, 5, False, True, (2, 37, 60), 1, False),  # KS 3, hid 160 = 5 chunks, residual
    # v4 k5 fallback, expand_dw4_kernel<5, KS> via launch_k<5>: what v5 refuses
    "v4k5_wo30": ("v4_k5", 40, 40, 1, 4, 5, True, True, (2, 20, 30), 1, False),          # wo % 4 != 0: scalar D stores
    "v4k5_cin96": ("v4_k5", 96, 80, 1, 4, 5, False, True, (1, 16, 16), 1, False),        # cin_pad 96 > 48, KS 6, hid 384
    # v4 k3, expand_dw4_kernel<3, KS> via launch_k<3> (bands of 31 rows, strips of 28 columns)
    "v4k3_hid120_wo40": ("v4_k3", 20, 20, 1, 6, 3, False, True, (2, 12, 40), 1, False),  # hid 120; wo % 8 == 0: the 4-strip
    #   workgroup form; ragged last strip (12 columns)
    "v4k3_35x57": ("v4_k3", 16, 16, 1, 6, 3, True, True, (1, 35, 57), 1, False),         # odd wo: scalar stores; 2 bands; 1-column last strip
    "v4k3_20x36": ("v4_k3", 16, 24, 1, 6, 3, True, True, (2, 20, 36), 1, False),         # wo % 4 == 0 only: 8-byte D pieces
    # v4 stride 2, expand_dw4s2_kernel<K, KS> via launch_s2<K> (even wo; bands of 32 rows, strips of 14)
    "v4s2_k3_odd_ho": ("v4_s2", 16, 24, 2, 6, 3, True, True, (1, 33, 40), 1, False),     # ho 17 (odd input height), wo 20
    "v4s2_k5_two_bands": ("v4_s2", 24, 40, 2, 6, 5, True, True, (1, 66, 120), 1, False),  # ho 33: two bands; wo 60: 5 strips
    # v3, expand_dw3_kernel<3>: k3, stride 1, cin_pad >= 80 on a map of at most 128^2 (launch_ed4 declines)
    "v3_96_288": ("v3", 96, 96, 1, 3, 3, True, True, (1, 10, 12), 1, False),
    # stride 2 with odd wo: launch_ed4 declines (4-byte D pieces), v3 and v2 are stride 1 only, so v1
    # (expand_dw_kernel via launch_ed<bf16, K, 2>)
    "v1_s2_k3_odd_wo": ("v1_s2_odd", 16, 24, 2, 6, 3, False, True, (1, 20, 30), 1, False),   # wo 15
    "v1_s2_k5_odd_wo": ("v1_s2_odd", 24, 40, 2, 6, 5, True, True, (1, 17, 26), 1, False),    # ho 9, wo 13
    # ratio-1 (no expand), expand_dw4_kernel<3, 2, ..., R1, UP> via launch_ks<3, 2, true, UP>
    "r1_up1": ("v4_ratio1", 24, 24, 1, 1, 3, False, True, (2, 12, 20), 1, False),
    "r1_up2": ("v4_ratio1", 40, 40, 1, 1, 3, False, True, (2, 16, 24), 2, False),         # out 32 x 48; residual upsampled in pw
    "r1_up2_odd": ("v4_ratio1", 24, 24, 1, 1, 3, False, True, (1, 9, 13), 2, False),      # out 18 x 26: scalar stores
    # ratio-1 with a split input: c1 != cin, so launch_ed4 is skipped and v2 runs (expand_dw2_kernel<3, 1, false>)
    "r1_split_v2": ("v2_ratio1_split", 48, 40, 1, 1, 3, False, False, (1, 9, 13), 1, True),
    # ada_out: ast_mb_expand_gemm (pw_kernel<bf16, 8> with Hardswish) on x1 128 + x2 128 -> 768, then
    # the ratio-1 depthwise on the stored hidden map (launch_ks<3, 2, true, 1>)
    "gemm_256_768": ("gemm+v4_ratio1", 256, 128, 1, 3, 3, False, False, (1, 10, 12), 1, True),
}

# fp32 runs v1 only (dispatch_ed<float>): expand_dw_kernel<float, ...>
FP32_CASES = ["v5_ks2_hid60_37x60", "v4s2_k3_odd_ho", "r1_up2"]

FORCED = [
    # (variable, value, what it selects, cases it redirects)
    ("AST_MB_ED5", "0", "v4_k5",   # the v4 k5 kernels instead of v5
     ["v5_ks1_one_tile", "v5_ks2_hid60_37x60", "v5_ks2_5x8", "v5_ks3_hid240", "v5_ks3_hid160_37x60"]),
    ("AST_MB_ED", "3", "v3",       # no v4/v5: v3 for the stride-1 expand blocks (k3 and k5), v1 for stride 2
     ["v4k3_hid120_wo40", "v4k3_35x57", "v5_ks2_hid60_37x60", "v5_ks3_hid240", "v4s2_k3_odd_ho"]),
    ("AST_MB_ED", "2", "v2",       # v2: k3 expand, k5 with cin_pad > 48, ratio-1 with and without upsample
     ["v4k3_hid120_wo40", "v4k3_35x57", "v4k5_cin96", "r1_up1", "r1_up2"]),
    ("AST_MB_ED", "1", "v1",       # v1 for everything
     ["v4k3_hid120_wo40", "v5_ks2_hid60_37x60", "v4s2_k5_two_bands", "r1_up2", "v3_96_288"]),
]


def _nan(shape, dev, dtype):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def run_stages(name, dev, dtype):
    """One block, stage by stage, the way DepthWiseConv.run launches it (without the fused pair).
    Returns (operands for the references, {D, pool, wg, out[, hmid]} on the CPU)."""
    _, inp, oup, s, t, k, norm, ident, (n, h, w), up, split = CASES[name]
    seed = 950 + inp + oup
    blk = synth.live_init_(DepthWiseConv(inp, oup, s, t, kernel_size=k, use_norm=norm, use_identity=ident), seed)
    blk = blk.eval().to(dev).to(dtype)
    x = (torch.from_numpy(synth.image(seed + 1, (n, inp, h, w)) * 2 - 0.7)).to(dev).to(dtype)
    x1, x2, c1 = x, None, inp
    if split:
        c1 = inp // 2
        x1, x2 = x[:, :c1].contiguous(), x[:, c1:].contiguous()
    dt, cin, hid, cout = dtype, inp, blk.hidden_dim, oup
    pad = (k - 1) // 2
    ho, wo = (h * up + 2 * pad - k) // s + 1, (w * up + 2 * pad - k) // s + 1
    p = blk._plan(dt, dev)
    st = stream_ptr(dev)
    got = {}
    d, pool = _nan((n, hid, ho, wo), dev, dt), _nan((n, hid), dev, F32)
    if (dt == BF and p.w1p is not None and p.cin_pad >= 256 and p.cin_pad % 32 == 0 and hid % 128 == 0
            and s == 1 and up == 1 and k == 3):
        hmid = _nan((n, hid, h, w), dev, dt)
        check(lib().ast_mb_expand_gemm(DTYPE_CODE[dt], ptr(x1), ptr(x2), c1, n, cin, h, w, ptr(p.w1p), ptr(p.b1), hid,
                                       p.cin_pad, ptr(hmid), st), "expand GEMM")
        check(M._expand_dw(dt, hmid, None, hid, n, hid, h, w, 1, None, None, hid, 0, p.wd, p.bd, k, s, d, pool, ho, wo,
                           st), "dw")
        got["hmid"] = hmid
    else:
        check(M._expand_dw(dt, x1, x2, c1, n, cin, h, w, up, p.w1p, p.b1, hid, p.cin_pad, p.wd, p.bd, k, s, d, pool,
                           ho, wo, st), "expand+dw")
    wg = _nan((n, p.cout_pad, p.hid_pad), dev, dt)
    check(lib().ast_mb_se_fold(DTYPE_CODE[dt], ptr(pool), n, hid, ho * wo, ptr(p.fc1w), ptr(p.fc1b), p.red,
                               ptr(p.fc2w), ptr(p.fc2b), ptr(p.w2), cout, p.cout_pad, p.hid_pad, ptr(wg), st), "SE fold")
    out = _nan((n, cout, ho, wo), dev, dt)
    res = x if blk.identity else None   # identity blocks: res = x; after an upsample res_up = 1
    check(lib().ast_mb_pw(DTYPE_CODE[dt], ptr(d), n, hid, p.hid_pad, ho, wo, ptr(wg), p.cout_pad * p.hid_pad, ptr(p.b2),
                          cout, p.cout_pad, ptr(res), 1 if (res is not None and up == 2) else 0, ptr(out), st), "pw")
    torch.cuda.synchronize()
    got.update(D=d, pool=pool, wg=wg, out=out)
    op = S.operands_from_plan(blk, p, x1, x2, up, dt)
    return op, {key: v.float().cpu() for key, v in got.items()}


def report(op, got):
    return S.stage_report(op, got["D"], got["pool"], got["wg"], got["out"], hmid=got.get("hmid"))


def show(tag, name, rep):
    """The measured max(err / bound) per stage: a record, not a threshold."""
    print(f"STAGE {tag} {name} " + " ".join(f"{key}={v:.3g}" for key, v in S.ratios(rep).items()))


_RUNS = {}


def default_run(name, dev):
    """The bf16 run of a case under the default dispatch, once per process."""
    if name not in _RUNS:
        _RUNS[name] = run_stages(name, dev, BF)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_stages_bf16(name, hip_device):
    op, got = default_run(name, hip_device)
    rep = report(op, got)
    show(CASES[name][0], name, rep)
    S.assert_stages(rep, name)
    assert ("expand_gemm" in rep) == name.startswith("gemm")


@pytest.mark.parametrize("name", FP32_CASES)
def test_stages_fp32(name, hip_device):
    """fp32 storage runs the v1 kernels only; the same bounds with u = 2^-24."""
    op, got = run_stages(name, hip_device, F32)
    assert op.u == S.U_FP32
    rep = report(op, got)
    show("v1_fp32", name, rep)
    S.assert_stages(rep, name)


def test_pool_only_pass_bitwise(hip_device):
    """The pool-only pass of the fused pair (ast_mb_expand_dw with d == NULL) gives the pool sums of
    the D-writing pass bit for bit, at the fused pair's shapes."""
    from test_gpu_mobilenet import FUSED_CASES
    for inp, oup, t, norm, (n, h, w) in FUSED_CASES:
        blk = synth.live_init_(DepthWiseConv(inp, oup, 1, t, kernel_size=3, use_norm=norm), 970 + inp + oup)
        blk = blk.eval().to(hip_device).to(BF)
        x = torch.from_numpy(synth.image(971 + inp, (n, inp, h, w)) * 2 - 0.7).to(hip_device).to(BF)
        p = blk._plan(BF, hip_device)
        hid = blk.hidden_dim
        assert blk._fused_ok(BF, inp, p.cin_pad, hid, oup, 3, 1, h, w)
        pools = []
        for d in (_nan((n, hid, h, w), hip_device, BF), None):
            pool = _nan((n, hid), hip_device, F32)
            check(M._expand_dw(BF, x, None, inp, n, inp, h, w, 1, p.w1p, p.b1, hid, p.cin_pad, p.wd, p.bd, 3, 1, d,
                               pool, h, w, stream_ptr(hip_device)), "expand+dw")
            pools.append(pool)
        torch.cuda.synchronize()
        assert torch.isfinite(pools[0]).all()
        assert torch.equal(pools[0], pools[1]), (inp, oup, n, h, w)


# -- forced kernel families: AST_MB_ED and AST_MB_ED5 are read once per process ------------------
_CHILD = ("import sys; sys.path.insert(0, 'tests'); import test_gpu_mb_stages as T; "
          "T.child_main(sys.argv[1], sys.argv[2:])")


def child_main(dst, names):
    dev = torch.device("cuda:0")
    arrays = {}
    for name in names:
        _, got = run_stages(name, dev, BF)
        for key, v in got.items():
            arrays[f"{name}/{key}"] = v.numpy()   # bf16 values are exact in float32
    np.savez(dst, **arrays)


def test_forced_families(hip_device, tmp_path):
    """Each forced setting in a fresh child (one at a time; the first failing child ends the loop):
    the kernels it redirects the cases to stay inside the same bounds. For AST_MB_ED5=0 the
    difference between the v5 and the v4 D over bound_D is printed per case (a record: both are
    only asserted to be inside the bound)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for var, val, family, names in FORCED:
        dst = tmp_path / f"{var}_{val}.npz"
        env = {key: v for key, v in os.environ.items() if key not in ("AST_MB_ED", "AST_MB_ED5")}
        env[var] = val
        subprocess.run([sys.executable, "-c", _CHILD, str(dst)] + names, cwd=root, check=True, timeout=240, env=env)
        z = np.load(dst)
        for name in names:
            op, own = default_run(name, hip_device)
            got = {key: torch.from_numpy(z[f"{name}/{key}"]) for key in ("D", "pool", "wg", "out")}
            rep = report(op, got)
            show(f"forced_{var}={val}_{family}", name, rep)
            S.assert_stages(rep, f"{var}={val} {name}")
            if var == "AST_MB_ED5":
                S.assert_stages(report(op, own), name)
                bound = op._dref[1]
                delta = float(((got["D"].double() - own["D"].double()).abs() / bound.clamp_min(1e-300)).max())
                print(f"STAGE v5_vs_v4_delta {name} D={delta:.3g}")
