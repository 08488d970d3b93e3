"""Throughput of style swap (csrc/swap.hip).

At C = 512, 64 x 64 content against 64 x 64 style -- the relu4_1 maps of a 512 x 512 image pair: 3844
patches a side, K = 4608, 136 GFLOP per sample in the match -- for n = 1 and n = 8: times the three
stages (ast_patch_norms_f32, ast_patch_match_f32 with the library's split count and with forced
ones, ast_patch_gather_f32), the whole ast_style_swap_f32, and beside it the plain PyTorch
formulation of the same result on the same device (conv2d with the normalised style patches as
filters, argmax, conv_transpose2d of the one-hot map with the style patches, over the overlap
counts), which writes and re-reads the n x 3844 x 3844 score matrix. HIP events, warm-up first, the median of
--steps intervals of several launches, as bench_wct.py; the device's clocks as rocm-smi reports
them are printed when the tool is there.

    python scripts/bench_swap.py > profiles/swap_bench.txt

Prints one JSON line at the end.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import swap_ref as SR  # noqa: E402
from arbitrarystyletransfer_amd import _lib, ops  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def timed(fn, warmup, steps, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / reps)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]   # median, min, max (ms)


def torch_swap(c, s):
    """The PyTorch-ROCm formulation, per sample: (out, index)."""
    outs, idxs = [], []
    ones = None
    for b in range(c.shape[0]):
        cols = F.unfold(s[b:b + 1], 3)[0]                                   # [C * 9, Ns]
        nrm = cols.norm(dim=0, keepdim=True)
        filt = torch.where(nrm > 0, cols / nrm, torch.zeros_like(cols)).t().reshape(-1, c.shape[1], 3, 3)
        sc = F.conv2d(c[b:b + 1], filt)                                      # [1, Ns, H - 2, W - 2]
        idx = sc.argmax(dim=1)
        hot = F.one_hot(idx, sc.shape[1]).permute(0, 3, 1, 2).to(c.dtype)   # [1, Ns, H - 2, W - 2]
        tot = F.conv_transpose2d(hot, cols.t().reshape(-1, c.shape[1], 3, 3))
        if ones is None:
            ones = F.conv_transpose2d(torch.ones_like(hot[:, :1]), torch.ones(1, 1, 3, 3, device=c.device))
        outs.append(tot / ones)
        idxs.append(idx)
    return torch.cat(outs), torch.cat(idxs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulation")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    if shutil.which("rocm-smi"):
        print(subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True).stdout.strip())
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    c_, h, w = 512, 64, 64
    for n in a.batches:
        x = SR.features(8201, (n, c_, h, w)).to(dev)
        s = SR.features(8202, (n, c_, h, w)).to(dev)
        m = (h - 2) * (w - 2)
        flops = 2.0 * n * m * m * 9 * c_
        print(f"n = {n}: ({n}, {c_}, {h}, {w}) fp32 content and style; {m} patches a side, {flops / 1e9:.0f} GFLOP in the match")
        r = {}

        nb = int(L.ast_patch_norms_workspace_bytes(n, h, w))
        wn = torch.empty(nb, device=dev, dtype=torch.uint8)
        inv = torch.empty(n, m, device=dev)
        t, lo, hi = timed(lambda: L.ast_patch_norms_f32(s.data_ptr(), inv.data_ptr(), n, c_, h, w, wn.data_ptr(), nb, st),
                          a.warmup, a.steps, 10)
        print(f"  patch_norms                {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
        r["norms_ms"] = t

        idx = torch.empty(n, m, device=dev, dtype=torch.int32)
        score = torch.empty(n, m, device=dev)
        for splits in (0, 1, 4, 8, 16, 32, 61):
            mb = int(L.ast_patch_match_workspace_bytes(n, n, h, w, h, w, splits))
            wm = torch.empty(mb, device=dev, dtype=torch.uint8)
            t, lo, hi = timed(lambda: L.ast_patch_match_ex_f32(x.data_ptr(), s.data_ptr(), inv.data_ptr(), idx.data_ptr(),
                                                               score.data_ptr(), n, n, c_, h, w, h, w, splits,
                                                               wm.data_ptr(), mb, st), a.warmup, a.steps, 3)
            tag = "library's splits" if splits == 0 else f"{splits} split(s)"
            print(f"  patch_match, {tag:17s}{t * 1e3:9.1f} us  {flops / t / 1e9:6.1f} TFLOP/s = "
                  f"{100 * flops / (t * 1e-3) / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
            r[f"match_splits{splits}_ms"] = t
            del wm
        r["match_tflops"] = flops / r["match_splits0_ms"] / 1e9

        out = torch.empty_like(x)
        t, lo, hi = timed(lambda: L.ast_patch_gather_f32(s.data_ptr(), idx.data_ptr(), x.data_ptr(), out.data_ptr(), n, n,
                                                         c_, h, w, h, w, 1.0, st), a.warmup, a.steps, 10)
        print(f"  patch_gather               {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
        r["gather_ms"] = t

        t, lo, hi = timed(lambda: ops.style_swap(x, s), a.warmup, a.steps, 3)
        stages = r["norms_ms"] + r["match_splits0_ms"] + r["gather_ms"]
        print(f"  ops.style_swap, whole op   {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); stages sum to "
              f"{stages * 1e3:.1f} us: norms {100 * r['norms_ms'] / stages:.1f} %, match "
              f"{100 * r['match_splits0_ms'] / stages:.1f} %, gather {100 * r['gather_ms'] / stages:.1f} %")
        r["style_swap_ms"] = t

        if not a.no_torch:
            ref_out, ref_idx = torch_swap(x, s)
            got, gidx = ops.style_swap(x, s, return_index=True)
            agree = float((ref_idx.reshape(n, -1) == gidx.reshape(n, -1)).float().mean())
            err = float((got - ref_out).abs().max() / ref_out.abs().max())
            t, lo, hi = timed(lambda: torch_swap(x, s), 2, max(3, a.steps // 3), 1)
            print(f"  PyTorch conv2d / argmax / conv_transpose2d {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); "
                  f"{100 * agree:.2f} % of the indices agree, outputs differ by {err:.2e}; "
                  f"{t / r['style_swap_ms']:.2f} x ops.style_swap")
            r["torch_ms"], r["index_agreement"], r["torch_over_swap"] = t, agree, t / r["style_swap_ms"]
            del ref_out, ref_idx
        res[f"n{n}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
