"""Throughput of regional exact feature distribution matching (csrc/efdm_regions.hip).

Times ast_efdm_regions_f32 at content (8, 512, 64, 64) and a bank (S, 512, 64, 64) -- the relu4_1 maps
of 512 x 512 images -- for K in {1, 4, 8} scattered label maps, S in {1, 4} styles (every weight
non-zero, so every pixel gathers S values), with and without style labels; beside it the bank stage
alone (ast_efdm_region_sort_f32), ast_efdm_f32 on the same content with one shared style (the kernel
regional EFDM grew out of), and a PyTorch formulation that masks and sorts region by region. HIP
events, warm-up first, the median of 30 intervals of 10 launches with the min-to-max spread, one
process (as bench_efdm.py). Then the model level: stylize_regions_efdm against stylize_regions
(regional AdaIN) at B = 8, 512 x 512, four styles, K = 4.

    python scripts/bench_efdm_regions.py > profiles/efdm_regions_bench.txt

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
import efdm_ref as ER  # noqa: E402
from wct_regions_ref import scatter_labels  # noqa: E402
from arbitrarystyletransfer_amd import _lib, models, ops, synth  # noqa: E402

REPS = 10   # launches per timed interval: the interval is device time, not launch latency
COUNTS = {1: (4000,), 4: (1200, 1000, 1000, 800), 8: (500,) * 8}   # of 4096 pixels; the rest is labelled 255


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


def torch_regions(x, lab, bank, slab, mix, k_regions):
    """The masked formulation: one sort per (sample, region) of the content and per (style, region) of the
    bank, gathers through the inverse permutation. Float order (no specials in the benchmark's maps)."""
    n, c = x.shape[:2]
    xf, bf = x.flatten(2), bank.flatten(2)
    out = xf.clone()
    for b in range(n):
        for k in range(k_regions):
            idx = torch.nonzero(lab[b].flatten() == k).flatten()
            mk = idx.numel()
            if mk == 0:
                continue
            rank = xf[b][:, idx].argsort(dim=1, stable=True).argsort(dim=1)
            r = torch.arange(mk, device=x.device)
            t = torch.zeros((c, mk), device=x.device)
            for s in range(bank.shape[0]):
                vals = bf[s] if slab is None else bf[s][:, slab[s].flatten() == k]
                srt = vals.sort(dim=1).values
                t += mix[0, k, s] * srt[:, ((2 * r + 1) * srt.shape[1]) // (2 * mk)].gather(1, rank)
            out[b][:, idx] = t
    return out.view_as(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "configs": {}}
    L, st = _lib.lib(), _lib.stream_ptr(dev)

    n, c, h, w = shape = (8, 512, 64, 64)
    x = ER.features(6201, shape).to(dev)
    bank4 = ER.features(6202, (4, c, h, w)).to(dev)
    out = torch.empty_like(x)
    print(f"content {shape} fp32, {n * c} planes of {h * w}; bank (S, {c}, {h}, {w}); scattered labels, "
          f"{4096 - sum(COUNTS[4])} of 4096 pixels pass through; median of {a.steps} intervals of {REPS} launches")
    t_efdm, lo, hi = timed(lambda: L.ast_efdm_f32(x.data_ptr(), bank4.data_ptr(), out.data_ptr(), n, 1, c, h, w, h, w, 1.0,
                                                  None, 0, st), a.warmup, a.steps)
    print(f"  efdm, one shared style            {t_efdm * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["efdm_ms"] = t_efdm
    t_torch = {}
    for s_styles in (1, 4):
        bank = bank4[:s_styles].contiguous()
        g = torch.Generator().manual_seed(6210 + s_styles)
        for k in (1, 4, 8):
            lab = scatter_labels(6220 + k, (h, w), [COUNTS[k]] * n).to(dev)
            slab = scatter_labels(6230 + k, (h, w), [COUNTS[k]] * s_styles).to(dev)
            mix = torch.rand((1, k, s_styles), generator=g) + 0.1
            mix = (mix / mix.sum(dim=2, keepdim=True)).to(dev)
            wsb = int(L.ast_efdm_regions_workspace_bytes(n, c, h, w, k, s_styles, h, w))
            ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
            count = torch.empty((s_styles, k), device=dev, dtype=torch.int32)
            for sl in (None, slab):
                tag = f"K{k}_S{s_styles}_{'style_labels' if sl is not None else 'whole_styles'}"
                sp = 0 if sl is None else sl.data_ptr()
                t, lo, hi = timed(lambda: _lib.check(L.ast_efdm_regions_f32(
                    x.data_ptr(), lab.data_ptr(), bank.data_ptr(), sp, mix.data_ptr(), out.data_ptr(), n, c, h, w, k,
                    s_styles, h, w, 1, 1.0, ws.data_ptr(), wsb, st), tag), a.warmup, a.steps)
                tb, blo, bhi = timed(lambda: _lib.check(L.ast_efdm_region_sort_f32(
                    bank.data_ptr(), sp, ws.data_ptr(), count.data_ptr(), s_styles, c, h, w, k, st), tag), a.warmup, a.steps)
                print(f"  K={k} S={s_styles} {'style labels' if sl is not None else 'whole styles'}  {t * 1e3:9.1f} us  "
                      f"{t / t_efdm:5.2f} x efdm  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); bank sort alone {tb * 1e3:7.1f} us "
                      f"(min {blo * 1e3:.1f}, max {bhi * 1e3:.1f}), apply by difference {(t - tb) * 1e3:7.1f} us")
                res["configs"][tag] = {"ms": t, "min_ms": lo, "max_ms": hi, "bank_sort_ms": tb, "to_efdm": t / t_efdm}
                if k in (1, 4) and s_styles == 4:
                    got = out.clone()
                    t_torch[tag] = timed(lambda: torch_regions(x, lab, bank, sl, mix, k), 1, 3, reps=1)
                    err = ER.rel_inf(got.cpu(), torch_regions(x, lab, bank, sl, mix, k).cpu())
                    print(f"      PyTorch, masked sorts per region  {t_torch[tag][0]:9.3f} ms  {t_torch[tag][0] / t:6.1f} x the kernel  "
                          f"(min {t_torch[tag][1]:.3f}, max {t_torch[tag][2]:.3f}; results {err:.1e} apart)")
                    res["configs"][tag]["torch_ms"] = t_torch[tag][0]
            del ws

    ci = torch.from_numpy(synth.image(6301, (8, 3, 512, 512))).to(dev)
    si = torch.from_numpy(synth.image(6302, (4, 3, 512, 512))).to(dev)
    lab = scatter_labels(6303, (64, 64), [COUNTS[4]] * 8).to(dev)
    weights = [[.4, .3, .2, .1], [.1, .4, .3, .2], [.2, .1, .4, .3], [.3, .2, .1, .4]]
    net = models.AdaINStyleTransfer(weights="live").to(dev)
    t_model = {}
    with torch.no_grad():
        t_model["stylize_regions"] = timed(lambda: net.stylize_regions(ci, si, lab, weights), 2, max(5, a.steps // 3), reps=1)
        t_model["stylize_regions_efdm"] = timed(lambda: net.stylize_regions_efdm(ci, si, lab, weights), 2,
                                                max(5, a.steps // 3), reps=1)
    print("model, 8 x 3 x 512 x 512 content, 4 styles, K = 4 (labels at relu4_1 resolution):")
    for name, (t, lo, hi) in t_model.items():
        print(f"  {name:22s}  {t:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    d = t_model["stylize_regions_efdm"][0] - t_model["stylize_regions"][0]
    print(f"  stylize_regions_efdm - stylize_regions = {d:.3f} ms, {100 * d / t_model['stylize_regions_efdm'][0]:.1f} % of "
          f"stylize_regions_efdm")
    res["model"] = {k: v[0] for k, v in t_model.items()}
    res["model"]["added_ms"] = d
    print(json.dumps(res))


if __name__ == "__main__":
    main()
