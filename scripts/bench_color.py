"""Throughput and error of the colour-space kernels (csrc/color.hip).

Times rgb2lab, lab2rgb and luma_transfer at (8,3,512,512) fp32 and (32,3,1024,1024) bf16 beside a
same-size torch.Tensor.copy_ in the same process (HIP events, warm-up first, as bench.py), and
reports algorithmic GB/s (bytes read + written) and the ratio to the copy's rate. Also prints the
max error of the fp32 kernels against the float64 restatement tests/color_ref.py on a
(2,3,64,64) image, so two builds can be compared (the transcendental A/B):

    python scripts/bench_color.py                                   # the in-tree library
    bash scripts/build_variants.sh color_libm "-DAST_COLOR_LIBM=1" color.hip
    AST_HIP_LIB=build_var/libast_hip_color_libm.so python scripts/bench_color.py

Prints one JSON line at the end.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import color_ref as CR  # noqa: E402
from arbitrarystyletransfer_amd import _lib, ops, synth  # noqa: E402


REPS = 10   # launches per timed interval: the interval is device time, not launch latency


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(REPS):
            fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / REPS)
    times.sort()
    return times[len(times) // 2]   # median, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "cases": [], "errors": {}}

    rgb = torch.from_numpy(synth.image(951, (2, 3, 64, 64)))
    for mode in CR.MODES:
        x = CR.stage_input(mode, rgb).float().contiguous()
        y64 = CR.convert(mode, x.double())
        noise = float((CR.convert(mode, x).double() - y64).abs().max())
        err = float((ops.color_convert(x.to(dev), mode).double().cpu() - y64).abs().max())
        res["errors"][mode] = {"max_abs_err": err, "cpu_fp32_noise": noise, "scale": float(y64.abs().max())}
        print(f"{mode:8s} max|gpu - f64| {err:.3e}   CPU fp32 noise {noise:.3e}   scale {float(y64.abs().max()):.3g}")

    for shape, dtype in (((8, 3, 512, 512), torch.float32), ((32, 3, 1024, 1024), torch.bfloat16)):
        x = torch.rand(shape, device=dev).to(dtype)
        lab = ops.color_convert(x, "rgb2lab", out_dtype=dtype)
        s = (torch.rand(shape, device=dev) * 1.6 - 0.3).to(dtype)
        dst = torch.empty_like(x)
        nbytes = x.numel() * x.element_size()
        t_copy = timed(lambda: dst.copy_(x), a.warmup, a.steps)
        copy_gbs = 2 * nbytes / t_copy / 1e6
        print(f"{tuple(shape)} {dtype}: copy_ {t_copy:.4f} ms  {copy_gbs:.0f} GB/s")
        # the C ABI directly, into a preallocated output: no allocator or wrapper time in the interval
        L, st, n, hw = _lib.lib(), _lib.stream_ptr(dev), shape[0], shape[2] * shape[3]
        conv = L.ast_color_convert_bf16 if dtype == torch.bfloat16 else L.ast_color_convert_f32
        luma = L.ast_luma_transfer_bf16 if dtype == torch.bfloat16 else L.ast_luma_transfer_f32
        px, pl, ps, pd = x.data_ptr(), lab.data_ptr(), s.data_ptr(), dst.data_ptr()
        for name, fn, nb in (
                ("rgb2lab", lambda: conv(px, pd, n, hw, ops.COLOR_MODES["rgb2lab"], st), 2 * nbytes),
                ("lab2rgb", lambda: conv(pl, pd, n, hw, ops.COLOR_MODES["lab2rgb"], st), 2 * nbytes),
                ("luma_transfer", lambda: luma(ps, px, pd, n, hw, st), 3 * nbytes)):
            t = timed(fn, a.warmup, a.steps)
            gbs = nb / t / 1e6
            res["cases"].append({"shape": list(shape), "dtype": str(dtype), "op": name, "ms": t, "gbs": gbs,
                                 "copy_ms": t_copy, "copy_gbs": copy_gbs, "ratio_to_copy": gbs / copy_gbs})
            print(f"  {name:14s} {t:.4f} ms  {gbs:.0f} GB/s  {gbs / copy_gbs:.2f} x copy")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
