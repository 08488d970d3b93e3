"""Throughput of the self-similarity content loss (csrc/selfsim.hip).

Two shapes at C = 512: x and c both (16, 512, 64, 64) -- the relu4_1 maps of a batch of 16 images of
512 x 512: 4096 pixels, 17 GFLOP per sample in each of the forward's and the backward's GEMM --, and both
(16, 512, 32, 32). For each: the column sums, the pass over the tile pairs (ast_selfsim_pairs_f32, norms
and column sums given), the whole forward (ops.selfsim_loss) and the backward
(ops.selfsim_loss_backward), the workspaces and the sign planes; ops.cosine_match on the same shape in
the same process, the yardstick at equal FLOPs; sample 0 against the float64 reference of
tests/selfsim_ref.py on the CPU; and the plain PyTorch formulation on the same device
(normalise, bmm twice, column-normalise, abs().sum(), autograd backward), which stores the n x N x N
distance matrices, with its peak memory. Then the AdaINTrainer step at B = 16, 512 x 512, with
selfsim_lam = 1 and with selfsim_lam = 0 (the step as it was) in the same process. HIP events, warm-up
first, the median of --steps intervals of several launches, as bench_remd.py.

    python scripts/bench_selfsim.py > profiles/selfsim_bench.txt

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
import selfsim_ref as R  # noqa: E402
import swap_ref as SR  # noqa: E402
from arbitrarystyletransfer_amd import _lib, ops, synth  # noqa: E402

PEAK_F32_MFMA = 157.3e12

SHAPES = [(16, 512, 64, 64), (16, 512, 32, 32)]


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


def torch_selfsim(x, c):
    """The PyTorch-ROCm formulation: the loss as a differentiable function of x."""
    def columns(f):
        fh = torch.nn.functional.normalize(f.flatten(2), dim=1, eps=0.0)              # [n, C, N]
        d = 1.0 - torch.bmm(fh.transpose(1, 2), fh)
        d = d - torch.diag_embed(d.diagonal(dim1=1, dim2=2))                          # the diagonal is 0 by definition
        return d / d.sum(dim=1, keepdim=True)
    return ((columns(x) - columns(c)).abs().sum(dim=(1, 2)) / (x.shape[2] * x.shape[3])).mean()


def torch_fwd_bwd(x, c):
    xg = x.detach().requires_grad_(True)
    loss = torch_selfsim(xg, c)
    (dx,) = torch.autograd.grad(loss, xg)
    return loss.detach(), dx


def bench_shape(shape, a, dev):
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    x, c = SR.features(8401, shape).to(dev) + 1e-3, SR.features(8402, shape).to(dev) + 1e-3
    n, ch, npix = shape[0], shape[1], shape[2] * shape[3]
    tiles = (npix + 63) // 64
    flops = 2.0 * n * npix * npix * ch
    r = {"flops": flops}
    print(f"x, c {shape}: {npix} pixels, {tiles * (tiles + 1) // 2} tile pairs, {flops / 1e9:.0f} GFLOP in the pairs pass "
          f"and again in the backward")
    u, v = ops.cosine_norms(x), ops.cosine_norms(c)
    t, lo, hi = timed(lambda: (ops.selfsim_colsum(x, u), ops.selfsim_colsum(c, v)), a.warmup, a.steps, 10)
    print(f"  column sums, both maps       {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    r["colsum_ms"] = t
    rx, rc = ops.selfsim_colsum(x, u), ops.selfsim_colsum(c, v)
    wb = int(L.ast_selfsim_pairs_workspace_bytes(n, npix))
    ws = torch.empty(wb, device=dev, dtype=torch.uint8)
    sums, tt = torch.empty(n, device=dev), torch.empty(n, npix, device=dev)
    pos = torch.empty(n, npix, tiles, device=dev, dtype=torch.int64)
    neg = torch.empty_like(pos)
    t, lo, hi = timed(lambda: L.ast_selfsim_pairs_f32(
        x.data_ptr(), c.data_ptr(), u.data_ptr(), v.data_ptr(), rx.data_ptr(), rc.data_ptr(), sums.data_ptr(),
        tt.data_ptr(), pos.data_ptr(), neg.data_ptr(), n, ch, npix, ws.data_ptr(), wb, st), a.warmup, a.steps, 3)
    planes = 2 * pos.numel() * 8
    print(f"  selfsim_pairs                {t * 1e3:9.1f} us  {flops / t / 1e9:6.1f} TFLOP/s = "
          f"{100 * flops / (t * 1e-3) / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak; workspace {wb / 2**20:.1f} MiB, sign "
          f"planes {planes / 2**20:.1f} MiB (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    r.update(pairs_ms=t, pairs_ws_bytes=wb, plane_bytes=planes, pairs_tflops=flops / t / 1e9)
    del ws

    t, lo, hi = timed(lambda: ops.cosine_match(x, c), a.warmup, a.steps, 3)
    tn, _, _ = timed(lambda: (ops.cosine_norms(x), ops.cosine_norms(c)), a.warmup, a.steps, 10)
    match = t - tn          # ops.cosine_match takes the norms itself
    print(f"  ops.cosine_match, same shape {match * 1e3:9.1f} us  {flops / match / 1e9:6.1f} TFLOP/s (the norms' "
          f"{tn * 1e3:.1f} us taken off): selfsim_pairs / cosine_match = {r['pairs_ms'] / match:.2f}")
    r.update(match_ms=match, norms_ms=tn, pairs_over_match=r["pairs_ms"] / match)

    t, lo, hi = timed(lambda: ops.selfsim_loss(x, c), a.warmup, a.steps, 3)
    print(f"  ops.selfsim_loss, forward    {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); "
          f"{t / match:.2f} x cosine_match")
    r["forward_ms"] = t
    one = torch.tensor(1.0, device=dev)
    loss, _, state = ops.selfsim_loss(x, c)
    t, lo, hi = timed(lambda: ops.selfsim_loss_backward(x, state, one), a.warmup, a.steps, 3)
    bwb = int(L.ast_selfsim_loss_backward_workspace_bytes(n, ch, npix))
    print(f"  ops.selfsim_loss_backward    {t * 1e3:9.1f} us  {flops / t / 1e9:6.1f} TFLOP/s; workspace {bwb / 2**20:.1f} MiB "
          f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    r.update(backward_ms=t, backward_ws_bytes=bwb, backward_tflops=flops / t / 1e9)
    ours = r["forward_ms"] + r["backward_ms"]

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _, _, st2 = ops.selfsim_loss(x, c)
    dx = ops.selfsim_loss_backward(x, st2, one)
    torch.cuda.synchronize()
    r["peak_bytes"] = torch.cuda.max_memory_allocated() - base
    print(f"  peak memory of forward + backward, state and workspaces included: {r['peak_bytes'] / 2**20:.0f} MiB")
    # sample 0 against the float64 reference on the CPU, the gradient at the kernel's own sign planes
    s0, _ = R.unpack_planes(st2[5][:1], st2[6][:1], npix)
    x0, c0 = x[:1].cpu(), c[:1].cpu()
    wrong, outside = R.check_signs(s0, x0, c0)
    e_p = abs(float(sums[0]) - float(R.loss(x0, c0)[1][0]))
    e_g = R.grad_error(dx[:1].cpu() * n, x0, c0, signs=s0)
    print(f"  sample 0 against float64: per-sample loss differs by {e_p:.2e}; {wrong} of {npix * (npix - 1)} signs differ, "
          f"{outside} outside the margin; gradient at the kernel's own signs rel_inf {e_g:.2e}")
    r.update(loss_err64=e_p, signs_differ=wrong, grad_rel_inf64=e_g)
    del st2, s0

    if not a.no_torch:
        tl, tdx = torch_fwd_bwd(x, c)
        e_l = abs(float(tl) - float(loss))
        e_g = float((dx - tdx).abs().max() / tdx.abs().max())
        del tl, tdx
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t, lo, hi = timed(lambda: torch_fwd_bwd(x, c), 2, max(3, a.steps // 3), 1)
        peak = torch.cuda.max_memory_allocated() - base
        tf, _, _ = timed(lambda: torch_selfsim(x, c), 1, max(3, a.steps // 3), 1)
        print(f"  PyTorch normalise / bmm x 2 / column-normalise / abs().sum() / autograd: forward {tf * 1e3:.1f} us, forward + "
              f"backward {t * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), peak memory {peak / 2**20:.0f} MiB; loss "
              f"differs by {e_l:.2e}, gradient by {e_g:.2e} rel_inf (signs of near-zero differences may differ); "
              f"{t / ours:.2f} x ours ({ours * 1e3:.1f} us forward + backward), {peak / r['peak_bytes']:.1f} x our peak memory")
        r.update(torch_forward_ms=tf, torch_fwd_bwd_ms=t, torch_peak_bytes=peak, torch_over_ours=t / ours,
                 torch_peak_over_ours=peak / r["peak_bytes"])
    return r


def bench_trainer(a, dev):
    from arbitrarystyletransfer_amd.train import AdaINTrainer, default_args
    b, s_ = 16, 512
    c = torch.from_numpy(synth.image(8411, (b, 3, s_, s_))).to(dev)
    s = torch.from_numpy(synth.image(8412, (b, 3, s_, s_))).to(dev)
    r = {}
    for lam in (0.0, 1.0):
        tr = AdaINTrainer(default_args(batch_size=b, image_size=s_, selfsim_lam=lam), device=dev)
        t, lo, hi = timed(lambda: tr.train_step(c, s), 2, max(3, a.steps // 3), 1)
        print(f"AdaINTrainer.train_step B = {b}, {s_} x {s_}, selfsim_lam = {lam}: {t:.2f} ms  (min {lo:.2f}, max {hi:.2f})")
        r[f"train_step_selfsim_lam{lam:g}_ms"] = t
        del tr
    r["train_step_ratio"] = r["train_step_selfsim_lam1_ms"] / r["train_step_selfsim_lam0_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch formulation")
    ap.add_argument("--no-trainer", action="store_true", help="skip the trainer step")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    for i, shape in enumerate(SHAPES):
        res[f"shape{i}"] = dict(bench_shape(shape, a, dev), shape=list(shape))
    if not a.no_trainer:
        res["trainer"] = bench_trainer(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
