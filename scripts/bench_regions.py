"""Throughput of regional multi-style AdaIN (csrc/adain_regions.hip).

Times ast_adain_regions_f32 at (8, 512, 64, 64) -- the relu4_1 map of benchmark config 2 -- for
K in {1, 2, 4, 8} regions beside ast_adain_stats_f32 and a same-size torch.Tensor.copy_ on the same
tensor in the same process (HIP events, warm-up first, the median of the timed intervals, as
bench_color.py), and region_stats at K = 8. Both AdaIN kernels read the plane from HBM once and
write it once; the label bytes are 1 / (4 C) of that. Then the model level:
AdaINStyleTransfer.stylize_regions with N = 8, 512 x 512, K = 2, S = 2 against forward with B = 8.

    python scripts/bench_regions.py > profiles/regions_bench.txt

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
import regions_ref as RR  # noqa: E402
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
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "op": [], "model": {}}
    L, st = _lib.lib(), _lib.stream_ptr(dev)

    n, c, h, w = shape = (8, 512, 64, 64)
    rows = 4
    x = RR.features(4001, shape).to(dev)
    out = torch.empty_like(x)
    mean, std = (t.to(dev) for t in RR.style_table(4002, rows, c))
    nbytes = 2 * x.numel() * 4
    t_copy, _, _ = timed(lambda: out.copy_(x), a.warmup, a.steps)
    print(f"{shape} fp32, {nbytes / 1e6:.1f} MB read + written per call")
    print(f"  copy_                {t_copy * 1e3:8.1f} us  {nbytes / t_copy / 1e6:6.0f} GB/s")
    t_stats, lo, hi = timed(lambda: L.ast_adain_stats_f32(x.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                                          out.data_ptr(), n, c, h, w, 0, 0.8, 1, st),
                            a.warmup, a.steps)
    print(f"  adain_stats          {t_stats * 1e3:8.1f} us  {nbytes / t_stats / 1e6:6.0f} GB/s  "
          f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["copy_ms"], res["adain_stats_ms"] = t_copy, t_stats
    for k in (1, 2, 4, 8):
        lab = RR.label_map(n, h, w, k, seed=RR.LABEL_SEED).to(dev)
        mix = RR.mix_weights(4003 + k, n, k, rows).to(dev)
        t, lo, hi = timed(lambda: L.ast_adain_regions_f32(x.data_ptr(), lab.data_ptr(), mean.data_ptr(),
                                                          std.data_ptr(), mix.data_ptr(), out.data_ptr(), n, c, h, w,
                                                          k, rows, k * rows, 0.8, 1, st), a.warmup, a.steps)
        nb = nbytes + lab.numel()   # the label map comes from HBM once; its re-reads by the C planes hit L2
        print(f"  adain_regions K={k}    {t * 1e3:8.1f} us  {nb / t / 1e6:6.0f} GB/s  {t / t_stats:5.2f} x adain_stats  "
              f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
        res["op"].append({"K": k, "ms": t, "min_ms": lo, "max_ms": hi, "gbs": nb / t / 1e6,
                          "ratio_to_adain_stats": t / t_stats})
    lab = RR.label_map(n, h, w, 8, seed=RR.LABEL_SEED).to(dev)
    rm = torch.empty((n, 8, c), device=dev)
    rs = torch.empty_like(rm)
    rc = torch.empty((n, 8), device=dev, dtype=torch.int32)
    t, lo, hi = timed(lambda: L.ast_region_stats_f32(x.data_ptr(), lab.data_ptr(), rm.data_ptr(), rs.data_ptr(),
                                                     rc.data_ptr(), n, c, h, w, 8, st), a.warmup, a.steps)
    print(f"  region_stats K=8     {t * 1e3:8.1f} us  {(nbytes // 2 + lab.numel()) / t / 1e6:6.0f} GB/s")
    res["region_stats_k8_ms"] = t

    net = models.AdaINStyleTransfer(weights="live").to(dev)
    ci = torch.from_numpy(synth.image(4101, (8, 3, 512, 512))).to(dev)
    si = torch.from_numpy(synth.image(4102, (8, 3, 512, 512))).to(dev)
    lab = torch.zeros((8, 512, 512), dtype=torch.uint8, device=dev)
    lab[:, :, 256:] = 1
    with torch.no_grad():
        t_fwd, lo_f, hi_f = timed(lambda: net(ci, si), 2, max(5, a.steps // 3), reps=1)
        t_reg, lo_r, hi_r = timed(lambda: net.stylize_regions(ci, si[:2], labels=lab, weights=[[0.7, 0.3], [0.2, 0.8]]),
                                  2, max(5, a.steps // 3), reps=1)
    print("model, 8 x 3 x 512 x 512 content:")
    print(f"  forward (8 styles)                 {t_fwd:8.3f} ms  (min {lo_f:.3f}, max {hi_f:.3f})")
    print(f"  stylize_regions (K=2, S=2 styles)  {t_reg:8.3f} ms  (min {lo_r:.3f}, max {hi_r:.3f})  "
          f"{t_reg / t_fwd:.2f} x forward")
    res["model"] = {"forward_ms": t_fwd, "stylize_regions_ms": t_reg, "ratio": t_reg / t_fwd}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
