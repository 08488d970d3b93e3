"""Throughput of the feature k-means (csrc/kmeans.hip) and the cost of labels=AutoRegions.

1. ops.kmeans at C = 512 on banks of S maps of 64 x 64 and 128 x 128 (the relu4_1 maps of 512 x 512 and
   1024 x 1024 images), S in {1, 4}, K in {4, 8}, 10 rounds: the whole op with its maximin seeding,
   the op from given initial centroids with 10 rounds and with none -- their difference over 10 is the
   time of one round (the fused assign-and-accumulate launch plus the reduction), against the
   4 P C bytes of the bank it has to read --, the stages alone, and beside it the plain PyTorch
   formulation of the same rounds on the same device from the same initial centroids (cdist, argmin,
   index_add_, bincount, a where for the empty clusters), with the share of final labels that agree.
2. AdaINStyleTransfer.stylize_regions at 512 x 512, S = 4 styles, batch 1 and 8: labels=AutoRegions(4)
   against hand-made label maps of four regions for content and styles (the path that existed before),
   and auto_labels alone.
HIP events, warm-up first, the median of --steps intervals of several launches, as bench_swap.py; the
device's clocks as rocm-smi reports them are printed when the tool is there.

    python scripts/bench_kmeans.py > profiles/kmeans_bench.txt

Prints one JSON line at the end.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as R  # noqa: E402
from arbitrarystyletransfer_amd import _lib, models, ops, synth  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, the datasheet's


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


def torch_lloyd(x, init, iters):
    """The PyTorch-ROCm formulation of the same rounds: (centroids, labels [P])."""
    b, c = x.shape[:2]
    pts = x.flatten(2).permute(0, 2, 1).reshape(-1, c)
    cen = init.clone()
    k = cen.shape[0]
    for r in range(iters + 1):
        lab = torch.cdist(pts, cen).argmin(dim=1)
        if r < iters:
            sums = torch.zeros_like(cen).index_add_(0, lab, pts)
            cnt = torch.bincount(lab, minlength=k).unsqueeze(1)
            cen = torch.where(cnt > 0, sums / cnt.clamp(min=1), cen)
    return cen, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulation")
    ap.add_argument("--no-model", action="store_true", help="skip part 2")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    if shutil.which("rocm-smi"):
        print(subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True).stdout.strip())
    c_, it = 512, a.iters
    for side in (64, 128):
        for s in (1, 4):
            x = R.features(12801 + side + s, (s, c_, side, side)).to(dev)
            p = s * side * side
            bank = 4.0 * p * c_
            for k in (4, 8):
                r = {}
                init = x.flatten(2).permute(0, 2, 1).reshape(-1, c_)[ops.kmeans_seed(x, k).long()].contiguous()
                print(f"bank ({s}, {c_}, {side}, {side}) fp32 = {bank / 1e6:.1f} MB, {p} points, K = {k}, {it} rounds")
                t_all, lo, hi = timed(lambda: ops.kmeans(x, k, iters=it), a.warmup, a.steps, 3)
                print(f"  ops.kmeans, maximin seeds + rounds   {t_all * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                t_it, lo, hi = timed(lambda: ops.kmeans(x, k, iters=it, init=init), a.warmup, a.steps, 3)
                print(f"  ops.kmeans from init, {it} rounds      {t_it * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                t_0, lo, hi = timed(lambda: ops.kmeans(x, k, iters=0, init=init), a.warmup, a.steps, 10)
                print(f"  ops.kmeans from init, 0 rounds       {t_0 * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                per = (t_it - t_0) / it
                rate = bank / (per * 1e-3)
                print(f"  one round (fused launch + reduction) {per * 1e3:9.1f} us = {rate / 1e12:.2f} TB/s of the bank's bytes, "
                      f"{100 * rate / HBM_PEAK:.1f} % of the HBM peak")
                t_seed, lo, hi = timed(lambda: ops.kmeans_seed(x, k), a.warmup, a.steps, 3)
                print(f"  ops.kmeans_seed ({k + 1} reads of the bank) {t_seed * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                lab = ops.kmeans_assign(x, init)
                t_as, lo, hi = timed(lambda: ops.kmeans_assign(x, init), a.warmup, a.steps, 10)
                print(f"  ops.kmeans_assign                    {t_as * 1e3:9.1f} us = {bank / (t_as * 1e-3) / 1e12:.2f} TB/s  "
                      f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                t_up, lo, hi = timed(lambda: ops.kmeans_update(x, lab, init), a.warmup, a.steps, 10)
                print(f"  ops.kmeans_update                    {t_up * 1e3:9.1f} us = {bank / (t_up * 1e-3) / 1e12:.2f} TB/s  "
                      f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                r.update(kmeans_ms=t_all, rounds_ms=t_it, no_rounds_ms=t_0, round_ms=per, round_bytes_per_s=rate,
                         seed_ms=t_seed, assign_ms=t_as, update_ms=t_up)
                if not a.no_torch:
                    _, ref_lab = torch_lloyd(x, init, it)
                    got = ops.kmeans(x, k, iters=it, init=init)[1]
                    agree = float((ref_lab == got.flatten().long()).float().mean())
                    t, lo, hi = timed(lambda: torch_lloyd(x, init, it), 2, max(3, a.steps // 3), 1)
                    print(f"  PyTorch cdist / argmin / index_add_  {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); "
                          f"{100 * agree:.2f} % of the labels agree; {t / t_it:.2f} x ops.kmeans from init")
                    r.update(torch_ms=t, label_agreement=agree, torch_over_kmeans=t / t_it)
                res[f"{side}x{side}_s{s}_k{k}"] = r
            del x

    if not a.no_model:
        net = models.AdaINStyleTransfer(weights="live").to(dev).eval()
        auto = models.AutoRegions(4)
        sty = torch.from_numpy(synth.image(12861, (4, 3, 512, 512))).to(dev)
        yy, xx = torch.meshgrid(torch.arange(512), torch.arange(512), indexing="ij")
        hand = ((yy // 256) * 2 + xx // 256).to(torch.uint8).to(dev)          # four quadrants
        for n in (1, 8):
            img = torch.from_numpy(synth.image(12862, (n, 3, 512, 512))).to(dev)
            lab, slab = hand.expand(n, -1, -1).contiguous(), hand.expand(4, -1, -1).contiguous()
            with torch.no_grad():
                t_hand, lo, hi = timed(lambda: net.stylize_regions(img, sty, labels=lab, style_labels=slab), a.warmup,
                                       a.steps, 2)
                print(f"stylize_regions 512 x 512, batch {n}, 4 styles, hand labels   {t_hand:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")
                t_auto, lo, hi = timed(lambda: net.stylize_regions(img, sty, labels=auto), a.warmup, a.steps, 2)
                print(f"                                          labels=AutoRegions(4) {t_auto:8.3f} ms  (min {lo:.3f}, max {hi:.3f}); "
                      f"+{t_auto - t_hand:.3f} ms = +{100 * (t_auto / t_hand - 1):.1f} %")
                f_c, f_s = net.encoder(img)[0], net.encoder(sty)[0]
                t_lab, lo, hi = timed(lambda: models._auto_regions(f_c, f_s, auto), a.warmup, a.steps, 2)
                print(f"                                          the maps alone, from the features {t_lab:8.3f} ms  "
                      f"(min {lo:.3f}, max {hi:.3f})")
            res[f"regions_n{n}"] = dict(hand_ms=t_hand, auto_ms=t_auto, auto_labels_ms=t_lab)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
