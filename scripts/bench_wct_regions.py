"""Throughput of the regional whitening and colouring transform (csrc/wct.hip).

At (8, 512, 64, 64) -- the relu4_1 maps of benchmark config 2 -- with HIP events, warm, the variants
alternating inside each step (so clock and neighbour drift hit all of them alike), the median of the
steps with min and max:
  (1) ops.wct with one shared style against ops.wct_regions with K = 1, S = 1 in the same process: the
      difference is what the binning and the gather cost;
  (2) K = 1, 2, 4, 8 regions of equal area scattered at random over the plane, S = K styles, one-hot
      weights: the regional covariance, the roots of the n K + S matrices and the apply stage apart, and
      the whole op. The MFMA work of covariance and apply is the same at every K; the roots scale with
      the matrix count;
  (3) the model: stylize_regions_wct (K = 2, S = 2) against the forward of a transform="wct" model at
      B = 8, 512 x 512.

    python scripts/bench_wct_regions.py > profiles/wct_regions_bench.txt

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

REPS = 5   # launches per timed interval: the interval is device time, not launch latency


def alternating(fns, warmup, steps, reps=REPS):
    """{name: (median, min, max) ms per call}; every step times each variant once, in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) / reps)
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = (t[len(t) // 2], t[0], t[-1])
    return out


def equal_area_labels(seed, n, h, w, k):
    """uint8 [n, h, w]: k regions of h w / k pixels each, scattered at random (no pass-through pixels)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.empty(n, h * w, dtype=torch.uint8)
    for b in range(n):
        lab[b, torch.randperm(h * w, generator=g)] = (torch.arange(h * w) % k).to(torch.uint8)
    return lab.reshape(n, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    L, st = _lib.lib(), _lib.stream_ptr(dev)

    n, c, h, w = shape = (8, 512, 64, 64)
    x = WR.features(8001, shape).to(dev)
    styles = WR.features(8002, shape).to(dev)   # a bank of up to 8 styles
    out = torch.empty_like(x)
    iters = ops.wct_default_iters(c, 1e-3)
    print(f"{shape} fp32 content, styles of the same size; {iters} Newton-Schulz iterations; median (min, max) of "
          f"{a.steps} steps of {REPS} calls, variants alternating inside each step")

    # (1) K = 1 against the unmasked op
    lab1 = torch.zeros(n, h, w, device=dev, dtype=torch.uint8)
    one = torch.ones(1, 1, 1, device=dev)
    ws_a = torch.empty(int(L.ast_wct_workspace_bytes(n, 1, c, h * w, h * w)), device=dev, dtype=torch.uint8)
    ws_b = torch.empty(int(L.ast_wct_regions_workspace_bytes(n, c, h, w, 1, 1, h, w, 0)), device=dev, dtype=torch.uint8)
    t = alternating({
        "wct": lambda: L.ast_wct_f32(x.data_ptr(), styles.data_ptr(), out.data_ptr(), n, 1, c, h, w, h, w, 1.0, 1e-3, 0,
                                     ws_a.data_ptr(), ws_a.numel(), st),
        "regions": lambda: L.ast_wct_regions_f32(x.data_ptr(), lab1.data_ptr(), styles.data_ptr(), None, one.data_ptr(),
                                                 out.data_ptr(), n, c, h, w, 1, 1, h, w, 1, 1.0, 1e-3, 0, ws_b.data_ptr(),
                                                 ws_b.numel(), st)}, a.warmup, a.steps)
    print("(1) one region, one shared style: the whole op")
    for k, (m, lo, hi) in t.items():
        print(f"  {k:8s} {m * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    d = t["regions"][0] - t["wct"][0]
    print(f"  regions - wct = {d * 1e3:.1f} us ({100 * d / t['wct'][0]:.1f} %): the binning and the gathered loads")
    res["k1"] = {"wct_ms": t["wct"][0], "regions_ms": t["regions"][0]}
    del ws_a, ws_b

    # (2) K = 1, 2, 4, 8: the stages apart
    print("(2) K equal-area scattered regions, S = K styles, one-hot weights")
    print(f"  {'K':>2s} {'cov us':>22s} {'roots us':>22s} {'per matrix, iteration':>22s} {'apply us':>22s} "
          f"{'cov + apply':>12s} {'whole op us':>22s}")
    res["by_k"] = {}
    for k in (1, 2, 4, 8):
        lab = equal_area_labels(8100 + k, n, h, w, k).to(dev)
        s = styles[:k].contiguous()
        mix = torch.eye(k, device=dev).unsqueeze(0).contiguous()
        b = n * k + k
        mean = torch.empty(b, c, device=dev)
        cov = torch.empty(b, c, c, device=dev)
        count = torch.empty(n, k, device=dev, dtype=torch.int32)
        root, iroot = torch.empty_like(cov), torch.empty_like(cov)
        wc = torch.empty(int(L.ast_wct_region_cov_workspace_bytes(n, c, h, w, k)), device=dev, dtype=torch.uint8)
        wq = torch.empty(int(L.ast_wct_sqrt_workspace_bytes(b, c)), device=dev, dtype=torch.uint8)
        wa = torch.empty(int(L.ast_wct_region_apply_workspace_bytes(n, c, h, w, k)), device=dev, dtype=torch.uint8)
        ww = torch.empty(int(L.ast_wct_regions_workspace_bytes(n, c, h, w, k, k, h, w, 0)), device=dev, dtype=torch.uint8)
        wsc = torch.empty(int(L.ast_wct_cov_workspace_bytes(k, c, h * w)), device=dev, dtype=torch.uint8)
        _lib.check(L.ast_wct_cov_f32(s.data_ptr(), mean[n * k:].data_ptr(), cov[n * k:].data_ptr(), k, c, h * w, 1e-3,
                                     wsc.data_ptr(), wsc.numel(), st), "style cov")
        fns = {
            "cov": lambda: L.ast_wct_region_cov_f32(x.data_ptr(), lab.data_ptr(), mean.data_ptr(), cov.data_ptr(),
                                                    count.data_ptr(), n, c, h, w, k, 1e-3, wc.data_ptr(), wc.numel(), st),
            "roots": lambda: L.ast_wct_sqrt_f32(cov.data_ptr(), root.data_ptr(), iroot.data_ptr(), b, c, iters,
                                                wq.data_ptr(), wq.numel(), st),
            "apply": lambda: L.ast_wct_region_apply_f32(
                x.data_ptr(), lab.data_ptr(), mean.data_ptr(), iroot.data_ptr(), mean[n * k:].data_ptr(),
                root[n * k:].data_ptr(), mix.data_ptr(), None, out.data_ptr(), n, c, h, w, k, k, 1, 0, 1.0, wa.data_ptr(),
                wa.numel(), st),
            "whole": lambda: L.ast_wct_regions_f32(x.data_ptr(), lab.data_ptr(), s.data_ptr(), None, mix.data_ptr(),
                                                   out.data_ptr(), n, c, h, w, k, k, h, w, 1, 1.0, 1e-3, 0, ww.data_ptr(),
                                                   ww.numel(), st)}
        for fn in fns.values():
            _lib.check(fn(), "bench call")
        t = alternating(fns, a.warmup, a.steps)
        f = {key: f"{m * 1e3:8.1f} ({lo * 1e3:.0f}, {hi * 1e3:.0f})" for key, (m, lo, hi) in t.items()}
        per = t["roots"][0] / (b * iters)
        print(f"  {k:2d} {f['cov']:>22s} {f['roots']:>22s} {per * 1e3:17.2f} us x{b:3d} {f['apply']:>22s} "
              f"{(t['cov'][0] + t['apply'][0]) * 1e3:12.1f} {f['whole']:>22s}")
        res["by_k"][k] = {"cov_ms": t["cov"][0], "roots_ms": t["roots"][0], "apply_ms": t["apply"][0],
                          "whole_ms": t["whole"][0], "matrices": b, "cov_workspace_mb": wc.numel() / 1e6}
        del wc, wq, wa, ww, wsc, mean, cov, root, iroot
    r = res["by_k"]
    ratio = (r[8]["cov_ms"] + r[8]["apply_ms"]) / (r[1]["cov_ms"] + r[1]["apply_ms"])
    print(f"  cov + apply at K = 8 over K = 1: {ratio:.2f} x  (a select-masked form would run K = 8 times the products)")
    res["cov_apply_k8_over_k1"] = ratio

    # (3) the model
    ci = torch.from_numpy(synth.image(8101, (8, 3, 512, 512))).to(dev)
    si = torch.from_numpy(synth.image(8102, (8, 3, 512, 512))).to(dev)
    lab2 = equal_area_labels(8103, 8, 64, 64, 2).to(dev)
    net = models.AdaINStyleTransfer(weights="live", transform="wct").to(dev).eval()
    with torch.no_grad():
        t = alternating({"forward": lambda: net(ci, si),
                         "stylize_regions_wct": lambda: net.stylize_regions_wct(ci, si[:2], lab2)},
                        2, max(5, a.steps // 3), reps=1)
    print("(3) model, 8 x 3 x 512 x 512: forward of transform='wct' (8 styles of the batch) against stylize_regions_wct "
          "(K = 2, S = 2)")
    for k, (m, lo, hi) in t.items():
        print(f"  {k:20s} {m:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    res["model"] = {k: v[0] for k, v in t.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
