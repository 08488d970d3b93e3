"""Timings of the pieces behind stylisation by optimisation (arbitrarystyletransfer_amd/strotss.py).

(a) The moment-matching loss (csrc/moment.hip) at x = y = (16, 512, 64, 64) and (16, 512, 32, 32), the
    relu4_1 and relu5_1 maps of a batch of 16 images of 512 x 512: the target statistics, the forward and
    the backward, with the peak device memory of forward + backward; beside them the PyTorch formulation
    on the same device in the same process (mean, bmm, abs().mean(), autograd backward) with its peak.
(b) The bilinear resize, its adjoint, lap_build and lap_collapse (csrc/pyramid.hip) on a 3 x 512 x 512
    image against F.interpolate with autograd.
(c) One stylizer iteration at each default scale for a 512 x 512 pair, called eagerly and replayed from
    the hipGraph, as the slope between two run lengths (set-up and capture drop out), and the whole
    default run.
HIP events around several launches for (a) and (b), warm-up first, the median of --steps intervals; (c) is
a host clock around runs that end in a device synchronise.

    python scripts/bench_strotss.py > profiles/strotss_bench.txt

Prints one JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import swap_ref as SR  # noqa: E402
from arbitrarystyletransfer_amd import ops, strotss, synth  # noqa: E402
from arbitrarystyletransfer_amd import functional as Fn  # noqa: E402

PEAK_F32_MFMA = 157.3e12
MOMENT_SHAPES = [(16, 512, 64, 64), (16, 512, 32, 32)]


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def torch_moment(x, y_mean, y_cov):
    v = x.flatten(2)
    mu = v.mean(dim=2)
    d = v - mu[:, :, None]
    cov = torch.bmm(d, d.transpose(1, 2)) / (v.shape[2] - 1)
    return ((mu - y_mean).abs().mean(dim=1) + (cov - y_cov).abs().mean(dim=(1, 2))).mean()


def torch_moment_fwd_bwd(x, y_mean, y_cov):
    xg = x.detach().requires_grad_(True)
    loss = torch_moment(xg, y_mean, y_cov)
    (dx,) = torch.autograd.grad(loss, xg)
    return loss.detach(), dx


def us(t):
    return t * 1e3


def bench_moment(shape, a, dev):
    n, c, h, w = shape
    m = h * w
    x, y = SR.features(9101, shape).to(dev), SR.features(9102, shape).to(dev)
    pairs = ((c + 63) // 64) * ((c + 63) // 64 + 1) // 2
    f_cov, f_bwd = 2.0 * n * pairs * 4096 * m, 2.0 * n * c * c * m
    rate = lambda f, t: f"{f / t / 1e9:6.1f} TFLOP/s = {100 * f / (t * 1e-3) / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak"  # noqa: E731
    r = {"x": list(shape)}
    print(f"moment loss, x = y = {shape}: {m} pixels, covariance {f_cov / 1e9:.1f} GFLOP (upper-triangle tiles), "
          f"backward {f_bwd / 1e9:.1f} GFLOP")
    t, lo, hi = timed(lambda: ops.moment_stats(y), a.warmup, a.steps, 5)
    print(f"  ops.moment_stats               {us(t):9.1f} us  {rate(f_cov, t)} (min {us(lo):.1f}, max {us(hi):.1f})")
    r["stats_ms"] = t
    y_mean, y_cov = ops.moment_stats(y)
    t, lo, hi = timed(lambda: ops.moment_loss(x, y_mean, y_cov), a.warmup, a.steps, 5)
    print(f"  ops.moment_loss, forward       {us(t):9.1f} us  {rate(f_cov, t)} (min {us(lo):.1f}, max {us(hi):.1f})")
    r["forward_ms"] = t
    loss, state = ops.moment_loss(x, y_mean, y_cov)
    t, lo, hi = timed(lambda: ops.moment_loss_backward(x, state), a.warmup, a.steps, 5)
    print(f"  ops.moment_loss_backward       {us(t):9.1f} us  {rate(f_bwd, t)} (min {us(lo):.1f}, max {us(hi):.1f})")
    r["backward_ms"] = t
    ours = r["forward_ms"] + r["backward_ms"]

    def ours_fwd_bwd():
        _, st = ops.moment_loss(x, y_mean, y_cov)
        return ops.moment_loss_backward(x, st)
    dx = ops.moment_loss_backward(x, state)
    peak = peak_of(ours_fwd_bwd)
    print(f"  peak device memory of forward + backward {peak / 2**20:.1f} MiB (dx {4 * x.numel() / 2**20:.0f} MiB, the "
          f"partial tiles, the int8 signs)")
    r["peak_bytes"] = peak
    tl, tdx = torch_moment_fwd_bwd(x, y_mean, y_cov)
    e_l = abs(float(tl) - float(loss)) / float(tl)
    e_g = float((dx - tdx).abs().max() / tdx.abs().max())
    del tdx, dx
    tpeak = peak_of(lambda: torch_moment_fwd_bwd(x, y_mean, y_cov))
    tf, _, _ = timed(lambda: torch_moment(x, y_mean, y_cov), a.warmup, a.steps, 3)
    t, lo, hi = timed(lambda: torch_moment_fwd_bwd(x, y_mean, y_cov), a.warmup, a.steps, 3)
    verdict = "the PyTorch formulation is FASTER" if t < ours else "ours is faster"
    print(f"  PyTorch formulation: forward {us(tf):.1f} us, forward + backward {us(t):.1f} us (min {us(lo):.1f}, max "
          f"{us(hi):.1f}), peak memory {tpeak / 2**20:.1f} MiB = {tpeak / peak:.2f} x ours; loss differs by {e_l:.2e} rel, "
          f"gradient by {e_g:.2e} rel_inf; {t / ours:.2f} x ours ({us(ours):.1f} us forward + backward): {verdict}")
    r.update(torch_forward_ms=tf, torch_fwd_bwd_ms=t, torch_peak_bytes=tpeak, torch_over_ours=t / ours)
    return r


def bench_pyramid(a, dev):
    x = torch.from_numpy(synth.image(9201, (1, 3, 512, 512))).to(dev)
    g = torch.randn(1, 3, 512, 512, device=dev)
    gh = torch.randn(1, 3, 256, 256, device=dev)
    small = ops.resize_bilinear(x, (256, 256))
    bw = lambda b, t: f"{b / (t * 1e-3) / 1e12:5.2f} TB/s"  # noqa: E731
    r = {}
    print("bilinear resize and Laplacian pyramid, 3 x 512 x 512 fp32 (algorithmic bytes: what is read plus what is written)")

    def interp(v, size):
        return F.interpolate(v, size=size, mode="bilinear", align_corners=False)

    def torch_adjoint(grad, src, size):
        leaf = src.detach().requires_grad_(True)
        (d,) = torch.autograd.grad(interp(leaf, size), leaf, grad)
        return d
    px = 3 * 512 * 512
    rows = [
        ("resize 512 -> 256", lambda: ops.resize_bilinear(x, (256, 256)), lambda: interp(x, (256, 256)), 4 * (px + px // 4)),
        ("resize 256 -> 512", lambda: ops.resize_bilinear(small, (512, 512)), lambda: interp(small, (512, 512)), 4 * (px + px // 4)),
        ("resize 256 -> 512 with add", lambda: ops.resize_bilinear(small, (512, 512), add=x, sign=-1.0),
         lambda: x - interp(small, (512, 512)), 4 * (2 * px + px // 4)),
        ("adjoint of 256 -> 512", lambda: ops.resize_bilinear_adjoint(g, (256, 256)),
         lambda: torch_adjoint(g, small, (512, 512)), 4 * (px + px // 4)),
        ("adjoint of 512 -> 256", lambda: ops.resize_bilinear_adjoint(gh, (512, 512)),
         lambda: torch_adjoint(gh, x, (256, 256)), 4 * (px + px // 4)),
    ]
    for name, ours_fn, torch_fn, nbytes in rows:
        t, lo, hi = timed(ours_fn, a.warmup, a.steps, 20)
        tt, tlo, thi = timed(torch_fn, a.warmup, a.steps, 20)
        verdict = "PyTorch is FASTER" if tt < t else "ours is faster"
        print(f"  {name:28s} {us(t):8.1f} us {bw(nbytes, t)} (min {us(lo):.1f}, max {us(hi):.1f}); PyTorch "
              f"{us(tt):8.1f} us (min {us(tlo):.1f}, max {us(thi):.1f}), {tt / t:.2f} x ours: {verdict}")
        r[name] = {"ms": t, "torch_ms": tt, "bytes": nbytes}

    def torch_build(v, levels):
        cur, pyr = v, []
        for _ in range(levels):
            sm = interp(cur, ops.lap_down_size(cur.shape[-2:]))
            pyr.append(cur - interp(sm, cur.shape[-2:]))
            cur = sm
        return pyr + [cur]

    def torch_collapse(pyr):
        cur = pyr[-1]
        for lvl in reversed(pyr[:-1]):
            cur = lvl + interp(cur, lvl.shape[-2:])
        return cur
    pyr = ops.lap_build(x, 5)
    leaves = [p.clone().requires_grad_(True) for p in pyr]

    def ours_collapse_bwd():
        return torch.autograd.grad(Fn.LapCollapseFn.apply(*leaves), leaves, g)

    def torch_collapse_bwd():
        return torch.autograd.grad(torch_collapse(leaves), leaves, g)
    for name, ours_fn, torch_fn in (("lap_build, 5 levels", lambda: ops.lap_build(x, 5), lambda: torch_build(x, 5)),
                                    ("lap_collapse, 5 levels", lambda: ops.lap_collapse(pyr), lambda: torch_collapse(pyr)),
                                    ("collapse forward + backward", ours_collapse_bwd, torch_collapse_bwd)):
        t, lo, hi = timed(ours_fn, a.warmup, a.steps, 10)
        tt, tlo, thi = timed(torch_fn, a.warmup, a.steps, 10)
        verdict = "PyTorch is FASTER" if tt < t else "ours is faster"
        print(f"  {name:28s} {us(t):8.1f} us (min {us(lo):.1f}, max {us(hi):.1f}); PyTorch {us(tt):8.1f} us (min "
              f"{us(tlo):.1f}, max {us(thi):.1f}), {tt / t:.2f} x ours: {verdict}")
        r[name] = {"ms": t, "torch_ms": tt}
    return r


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench_stylizer(a, dev):
    st = strotss.StrotssStylizer(device=dev)
    c = torch.from_numpy(synth.image(9301, (1, 3, 512, 512))).to(dev)
    s = torch.from_numpy(synth.image(9302, (1, 3, 512, 512))).to(dev)
    r = {}
    print("stylizer, a 512 x 512 pair, default taps, weights and levels; per iteration = (run of 3k - run of k) / 2k, "
          f"k = {a.iters}, the median of {a.runs} pairs of runs")
    for scale in strotss.DEFAULT_SCALES:
        row = {}
        for graph in (False, True):
            st.stylize(c, s, scales=(scale,), iters=2, graph=graph)   # warm-up: code objects, packs, the allocator
            slopes = sorted((wall(lambda: st.stylize(c, s, scales=(scale,), iters=3 * a.iters, graph=graph))
                             - wall(lambda: st.stylize(c, s, scales=(scale,), iters=a.iters, graph=graph))) / (2 * a.iters)
                            for _ in range(a.runs))
            row["replayed" if graph else "eager"] = slopes[len(slopes) // 2]
            row[("replayed" if graph else "eager") + "_minmax"] = (slopes[0], slopes[-1])
        print(f"  scale {scale:4d}: eager {row['eager']:7.3f} ms / iteration (min {row['eager_minmax'][0]:.3f}, max "
              f"{row['eager_minmax'][1]:.3f}), replayed {row['replayed']:7.3f} ms (min {row['replayed_minmax'][0]:.3f}, max "
              f"{row['replayed_minmax'][1]:.3f}): {row['eager'] / row['replayed']:.2f} x")
        r[f"scale{scale}"] = row
    for graph in (True, False):
        runs = sorted(wall(lambda: st.stylize(c, s, graph=graph)) for _ in range(a.runs))
        name = "replayed" if graph else "eager"
        print(f"  the whole default run (scales {strotss.DEFAULT_SCALES}, 200 iterations each), {name}: "
              f"{runs[len(runs) // 2] / 1e3:.2f} s (min {runs[0] / 1e3:.2f}, max {runs[-1] / 1e3:.2f})")
        r[f"default_run_{name}_ms"] = runs[len(runs) // 2]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20, help="k of the stylizer's run lengths k and 3k")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    try:
        res["shader_clock_mhz"] = int(torch.cuda.clock_rate())
        print(f"{res['device']}; shader clock at start {res['shader_clock_mhz']} MHz")
    except Exception as e:   # not every installation can read it
        print(f"{res['device']}; shader clock not readable ({type(e).__name__})")
    for i, shape in enumerate(MOMENT_SHAPES):
        res[f"moment{i}"] = bench_moment(shape, a, dev)
    res["pyramid"] = bench_pyramid(a, dev)
    res["stylizer"] = bench_stylizer(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
