"""Throughput and memory of the contextual loss (csrc/cx.hip).

Three shapes at C = 512: x and y both (16, 512, 64, 64) -- the relu4_1 maps of a batch of 16 images of
512 x 512: 4096 pixels a side, 17 GFLOP per sample and pass --, both (16, 512, 32, 32), and x
(16, 512, 64, 64) against one shared y (1, 512, 64, 64). For each: every stage through its C-ABI entry
(centring, inverse norms, the match, the row sums, the column maxima, the value), the two soft passes as
multiples of the match, the whole forward (ops.cx_loss) and the backward (ops.cx_loss_backward), the
workspace bytes and the peak device memory of forward + backward; beside them the dense
PyTorch formulation on the same device in the same process (centre, normalise, bmm, min, divide, exp, sum,
divide, max, log, autograd backward), which stores several n x M x P tensors, with its peak memory. HIP
events, warm-up first, the median of --steps intervals of several launches, as bench_remd.py.

    python scripts/bench_cx.py > profiles/cx_bench.txt

The backward's other form (one block of 128 channels per workgroup: the distances recomputed per block) is
a build of csrc/cx.hip with -DCX_DENSE_BLOCKS=1, named by AST_HIP_LIB:

    AST_HIP_LIB=<that library> python scripts/bench_cx.py --no-torch --blocks 1 >> profiles/cx_bench.txt

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
import swap_ref as SR  # noqa: E402
from arbitrarystyletransfer_amd import _lib, ops  # noqa: E402

PEAK_F32_MFMA = 157.3e12
EPS = ops.CX_EPS

SHAPES = [((16, 512, 64, 64), (16, 512, 64, 64)), ((16, 512, 32, 32), (16, 512, 32, 32)),
          ((16, 512, 64, 64), (1, 512, 64, 64))]


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


def torch_cx(x, y, h):
    """The dense PyTorch-ROCm formulation: the loss as a differentiable function of x."""
    yf = y.flatten(2)
    mu = yf.mean(dim=2, keepdim=True)
    xh = torch.nn.functional.normalize(x.flatten(2) - mu, dim=1, eps=0.0).transpose(1, 2)   # [n, M, C]
    yh = torch.nn.functional.normalize(yf - mu, dim=1, eps=0.0).expand(x.shape[0], -1, -1)
    d = 1.0 - torch.bmm(xh, yh)
    w = torch.exp((1.0 - d / (d.min(dim=2, keepdim=True).values + EPS)) / h)
    cx = w / w.sum(dim=2, keepdim=True)
    return (-torch.log(cx.max(dim=1).values.mean(dim=1))).mean()


def torch_fwd_bwd(x, y, h):
    xg = x.detach().requires_grad_(True)
    loss = torch_cx(xg, y, h)
    (dx,) = torch.autograd.grad(loss, xg)
    return loss.detach(), dx


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def bench_shape(xs, ys, a, dev):
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    x, y = SR.features(8401, xs).to(dev) + 1e-3, SR.features(8402, ys).to(dev) + 1e-3
    n, c, m, p, ns, h = xs[0], xs[1], xs[2] * xs[3], ys[2] * ys[3], ys[0], a.h
    flops = 2.0 * n * m * p * c
    r = {"flops_per_pass": flops}
    us = lambda t: t * 1e3  # noqa: E731
    rate = lambda f, t: f"{f / t / 1e9:6.1f} TFLOP/s = {100 * f / (t * 1e-3) / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak"  # noqa: E731
    print(f"x {xs} vs y {ys}: {m} x {p} pixels, {flops / 1e9:.0f} GFLOP per pass over the pairs, h = {h}")

    t, lo, hi = timed(lambda: ops.cx_center(x, y), a.warmup, a.steps, 5)
    print(f"  cx_center                      {us(t):9.1f} us  (min {us(lo):.1f}, max {us(hi):.1f})")
    r["center_ms"] = t
    _, xc, yc = ops.cx_center(x, y)
    t, lo, hi = timed(lambda: (ops.cosine_norms(xc), ops.cosine_norms(yc)), a.warmup, a.steps, 5)
    print(f"  inverse norms, both sides      {us(t):9.1f} us  (min {us(lo):.1f}, max {us(hi):.1f})")
    r["norms_ms"] = t
    u, v = ops.cosine_norms(xc), ops.cosine_norms(yc)
    rmin, ridx = torch.empty(n, m, device=dev), torch.empty(n, m, device=dev, dtype=torch.int32)
    cmin, cidx = torch.empty(n, p, device=dev), torch.empty(n, p, device=dev, dtype=torch.int32)
    wb = int(L.ast_cosine_match_workspace_bytes(n, ns, m, p, 0))
    ws = torch.empty(wb, device=dev, dtype=torch.uint8)
    t, lo, hi = timed(lambda: L.ast_cosine_match_f32(xc.data_ptr(), yc.data_ptr(), u.data_ptr(), v.data_ptr(), rmin.data_ptr(),
                                                     ridx.data_ptr(), cmin.data_ptr(), cidx.data_ptr(), n, ns, c, m, p, 0,
                                                     ws.data_ptr(), wb, st), a.warmup, a.steps, 3)
    print(f"  cosine_match                   {us(t):9.1f} us  {rate(flops, t)} (min {us(lo):.1f}, max {us(hi):.1f})")
    r["match_ms"] = tm = t
    S, E = torch.empty(n, m, device=dev), torch.empty(n, m, device=dev)
    wb = int(L.ast_cx_rowsum_workspace_bytes(n, ns, m, p, 0))
    ws = torch.empty(wb, device=dev, dtype=torch.uint8)
    t, lo, hi = timed(lambda: L.ast_cx_rowsum_f32(xc.data_ptr(), yc.data_ptr(), u.data_ptr(), v.data_ptr(), rmin.data_ptr(),
                                                  S.data_ptr(), E.data_ptr(), n, ns, c, m, p, h, 0, ws.data_ptr(), wb, st),
                      a.warmup, a.steps, 3)
    print(f"  cx_rowsum                      {us(t):9.1f} us  {rate(flops, t)}; {t / tm:.2f} x the match (min {us(lo):.1f}, "
          f"max {us(hi):.1f})")
    r["rowsum_ms"], r["rowsum_over_match"] = t, t / tm
    ccx, cdist = torch.empty(n, p, device=dev), torch.empty(n, p, device=dev)
    wb = int(L.ast_cx_colmax_workspace_bytes(n, ns, m, p))
    ws = torch.empty(wb, device=dev, dtype=torch.uint8)
    t, lo, hi = timed(lambda: L.ast_cx_colmax_f32(xc.data_ptr(), yc.data_ptr(), u.data_ptr(), v.data_ptr(), rmin.data_ptr(),
                                                  S.data_ptr(), ccx.data_ptr(), cidx.data_ptr(), cdist.data_ptr(), n, ns, c, m,
                                                  p, h, 0, ws.data_ptr(), wb, st), a.warmup, a.steps, 3)
    print(f"  cx_colmax                      {us(t):9.1f} us  {rate(flops, t)}; {t / tm:.2f} x the match; workspace "
          f"{wb / 2**20:.1f} MiB (min {us(lo):.1f}, max {us(hi):.1f})")
    r["colmax_ms"], r["colmax_over_match"], r["colmax_ws_bytes"] = t, t / tm, wb
    t, lo, hi = timed(lambda: ops.cx_value(ccx.reshape(n, 1, p)), a.warmup, a.steps, 5)
    print(f"  cx_value                       {us(t):9.1f} us  (min {us(lo):.1f}, max {us(hi):.1f})")
    r["value_ms"] = t
    del ws

    t, lo, hi = timed(lambda: ops.cx_loss(x, y, 1.0, h), a.warmup, a.steps, 3)
    print(f"  ops.cx_loss, whole forward     {us(t):9.1f} us  {rate(3 * flops, t)} (min {us(lo):.1f}, max {us(hi):.1f})")
    r["forward_ms"] = t
    one = torch.tensor(1.0, device=dev)
    loss, cxb, state = ops.cx_loss(x, y, 1.0, h)
    active = torch.zeros(n, m, device=dev, dtype=torch.bool)
    active.scatter_(1, state[9].reshape(n, p).long(), True)
    # the dense pass recomputes the distances once per group of a.blocks x 128 channels and multiplies c' once
    bflops = flops * ((c + 128 * a.blocks - 1) // (128 * a.blocks) + 1)
    t, lo, hi = timed(lambda: ops.cx_loss_backward(x, y, state, one, 1.0, h), a.warmup, a.steps, 3)
    print(f"  ops.cx_loss_backward           {us(t):9.1f} us  {rate(bflops, t)} at {bflops / flops:.0f} passes ({a.blocks} "
          f"block(s) of 128 channels per workgroup, library {os.path.basename(_lib.LIB_PATH)}); "
          f"{float(active.float().mean()):.2%} of the rows active (min {us(lo):.1f}, max {us(hi):.1f})")
    r["backward_ms"], r["backward_flops"] = t, bflops
    r["forward_ws_bytes"] = int(L.ast_cx_loss_workspace_bytes(n, ns, m, p))
    r["backward_ws_bytes"] = int(L.ast_cx_loss_backward_workspace_bytes(n, c, m, p))
    ours = r["forward_ms"] + r["backward_ms"]

    def ours_fwd_bwd():
        _, _, stt = ops.cx_loss(x, y, 1.0, h)
        return ops.cx_loss_backward(x, y, stt, one, 1.0, h)
    del state
    peak = peak_of(ours_fwd_bwd)
    formula = 4 * c * (n * m + ns * p) + r["backward_ws_bytes"] + 4 * n * c * m
    print(f"  workspaces: forward {r['forward_ws_bytes'] / 2**20:.1f} MiB, backward {r['backward_ws_bytes'] / 2**20:.1f} MiB; "
          f"peak device memory of forward + backward {peak / 2**20:.0f} MiB (the centred copies 4 C (n M + ns P) = "
          f"{4 * c * (n * m + ns * p) / 2**20:.0f} MiB, G and the lists {r['backward_ws_bytes'] / 2**20:.0f} MiB, dx "
          f"{4 * n * c * m / 2**20:.0f} MiB: {formula / 2**20:.0f} MiB)")
    r["peak_bytes"] = peak

    if not a.no_torch:
        loss, cxb, state = ops.cx_loss(x, y, 1.0, h)
        dx = ops.cx_loss_backward(x, y, state, one, 1.0, h)
        tl, tdx = torch_fwd_bwd(x, y, h)
        e_l = abs(float(tl) - float(loss))
        e_g = float((dx - tdx).abs().max() / tdx.abs().max())
        del tl, tdx, dx, state
        tpeak = peak_of(lambda: torch_fwd_bwd(x, y, h))
        t, lo, hi = timed(lambda: torch_fwd_bwd(x, y, h), 2, max(3, a.steps // 3), 1)
        tf, _, _ = timed(lambda: torch_cx(x, y, h), 1, max(3, a.steps // 3), 1)
        print(f"  dense PyTorch formulation: forward {us(tf):.1f} us, forward + backward {us(t):.1f} us (min {us(lo):.1f}, max "
              f"{us(hi):.1f}), peak memory {tpeak / 2**20:.0f} MiB = {tpeak / peak:.1f} x ours; loss differs by {e_l:.2e}, "
              f"gradient by {e_g:.2e} rel_inf (near-ties choose differently); {t / ours:.2f} x ours ({us(ours):.1f} us "
              f"forward + backward)")
        r.update(torch_forward_ms=tf, torch_fwd_bwd_ms=t, torch_peak_bytes=tpeak, torch_over_ours=t / ours)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--h", type=float, default=0.5)
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulation")
    ap.add_argument("--blocks", type=int, default=4, help="CX_DENSE_BLOCKS of the library under AST_HIP_LIB (for the FLOP "
                    "count of the backward only): 1 for a build with -DCX_DENSE_BLOCKS=1")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "h": a.h}
    for i, (xs, ys) in enumerate(SHAPES):
        res[f"shape{i}"] = dict(bench_shape(xs, ys, a, dev), x=list(xs), y=list(ys))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
