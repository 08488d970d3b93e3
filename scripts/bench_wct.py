"""Throughput of the whitening and colouring transform (csrc/wct.hip).

At (8, 512, 64, 64) for both maps -- the relu4_1 maps of benchmark config 2 -- times ast_wct_cov_f32, one
Newton-Schulz iteration on the 16 covariances (the difference of two fixed iteration counts), the roots
at the default count, the apply stage, the whole ast_wct_f32 eagerly and replayed from a hipGraph (the
same kernels without the 57 launches' host cost), and ast_adain_f32 on the same tensors in the same
process (HIP events, warm-up first, the median of 30 intervals of 10 launches, as bench_efdm.py). Then the model
level: AdaINStyleTransfer(transform="wct") against the default at B = 8, 512 x 512.

    python scripts/bench_wct.py > profiles/wct_bench.txt

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
import wct_ref as WR  # noqa: E402
from arbitrarystyletransfer_amd import _lib, models, ops, synth  # noqa: E402

REPS = 10   # launches per timed interval: the interval is device time, not launch latency


def timed(fn, warmup, steps, reps=REPS):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    L, st = _lib.lib(), _lib.stream_ptr(dev)

    n, c, h, w = shape = (8, 512, 64, 64)
    m, b = h * w, 2 * n
    x = WR.features(8001, shape).to(dev)
    s = WR.features(8002, shape).to(dev)
    out = torch.empty_like(x)
    iters = ops.wct_default_iters(c, 1e-3)
    print(f"{shape} fp32 content and style; {b} covariances of {c} x {c}; {iters} Newton-Schulz iterations")

    t_adain, lo, hi = timed(lambda: L.ast_adain_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n, c, h, w, h, w, 1.0,
                                                    1, st), a.warmup, a.steps)
    print(f"  adain                      {t_adain * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["adain_ms"] = t_adain

    mean = torch.empty(b, c, device=dev)
    cov = torch.empty(b, c, c, device=dev)
    wsb = int(L.ast_wct_cov_workspace_bytes(n, c, m))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    t_cov, lo, hi = timed(lambda: L.ast_wct_cov_f32(x.data_ptr(), mean.data_ptr(), cov.data_ptr(), n, c, m, 1e-3,
                                                    ws.data_ptr(), wsb, st), a.warmup, a.steps)
    fl = n * c * (c + 64) * m   # upper-triangle tiles: 2 flop x about half of C x C x M
    print(f"  wct_cov, {n} maps            {t_cov * 1e3:9.1f} us  {fl / t_cov / 1e9:6.1f} TFLOP/s on the triangle's tiles, "
          f"{x.numel() * 4 / t_cov / 1e6:5.0f} GB/s of input  ({wsb / 1e6:.0f} MB workspace; min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["cov_ms"] = t_cov
    L.ast_wct_cov_f32(s.data_ptr(), mean[n:].data_ptr(), cov[n:].data_ptr(), n, c, m, 1e-3, ws.data_ptr(), wsb, st)
    del ws

    root, iroot = torch.empty_like(cov), torch.empty_like(cov)
    wsb = int(L.ast_wct_sqrt_workspace_bytes(b, c))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    t_it = {}
    for k in (2, 12, iters):
        t_it[k] = timed(lambda: L.ast_wct_sqrt_f32(cov.data_ptr(), root.data_ptr(), iroot.data_ptr(), b, c, k,
                                                   ws.data_ptr(), wsb, st), a.warmup, a.steps)
    t_one = (t_it[12][0] - t_it[2][0]) / 10
    fl = 3 * 2 * c ** 3 * b
    print(f"  one Newton-Schulz iteration {t_one * 1e3:9.1f} us  {fl / t_one / 1e9:6.1f} TFLOP/s  (3 products x {b} matrices, "
          f"2 launches; from {t_it[12][0]:.3f} ms at 12 and {t_it[2][0]:.3f} ms at 2 iterations)")
    t, lo, hi = t_it[iters]
    print(f"  wct_sqrt, {iters} iterations     {t * 1e3:9.1f} us  {fl * iters / t / 1e9:6.1f} TFLOP/s  ({wsb / 1e6:.0f} MB workspace; "
          f"min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["ns_iteration_ms"], res["sqrt_ms"], res["ns_tflops"] = t_one, t, fl / t_one / 1e9
    del ws

    wsb = int(L.ast_wct_apply_workspace_bytes(n, c))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    t_app, lo, hi = timed(lambda: L.ast_wct_apply_f32(x.data_ptr(), mean.data_ptr(), mean[n:].data_ptr(),
                                                      root[n:].data_ptr(), iroot.data_ptr(), out.data_ptr(), n, n, c, m,
                                                      1.0, ws.data_ptr(), wsb, st), a.warmup, a.steps)
    fl = 2 * n * c * c * (c + m)
    print(f"  wct_apply (T, then the GEMM){t_app * 1e3:9.1f} us  {fl / t_app / 1e9:6.1f} TFLOP/s  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["apply_ms"] = t_app
    del ws

    wsb = int(L.ast_wct_workspace_bytes(n, n, c, m, m))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)

    def whole():
        return L.ast_wct_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n, n, c, h, w, h, w, 1.0, 1e-3, 0,
                             ws.data_ptr(), wsb, st)
    t_wct, lo, hi = timed(whole, a.warmup, a.steps)
    print(f"  wct, whole op              {t_wct * 1e3:9.1f} us  {t_wct / t_adain:6.1f} x adain  ({wsb / 1e6:.0f} MB workspace; "
          f"min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); stages sum to {(2 * t_cov + t_it[iters][0] + t_app) * 1e3:.1f} us")
    res["wct_ms"], res["wct_to_adain"] = t_wct, t_wct / t_adain
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.ast_wct_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n, n, c, h, w, h, w, 1.0, 1e-3, 0, ws.data_ptr(), wsb,
                      _lib.stream_ptr(dev))
    t_g, lo, hi = timed(g.replay, a.warmup, a.steps)
    print(f"  wct, hipGraph replay       {t_g * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["wct_graph_ms"] = t_g
    del ws, g

    ci = torch.from_numpy(synth.image(8101, (8, 3, 512, 512))).to(dev)
    si = torch.from_numpy(synth.image(8102, (8, 3, 512, 512))).to(dev)
    t_model = {}
    for transform in ("adain", "wct"):
        net = models.AdaINStyleTransfer(weights="live", transform=transform).to(dev)
        with torch.no_grad():
            t_model[transform] = timed(lambda: net(ci, si), 2, max(5, a.steps // 3), reps=1)
    print("model forward, 8 x 3 x 512 x 512 content and style:")
    for transform, (t, lo, hi) in t_model.items():
        print(f"  transform={transform:6s}  {t:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    d = t_model["wct"][0] - t_model["adain"][0]
    print(f"  wct - adain = {d:.3f} ms, {100 * d / t_model['wct'][0]:.1f} % of the wct forward")
    res["model"] = {"adain_ms": t_model["adain"][0], "wct_ms": t_model["wct"][0], "added_ms": d}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
