"""Throughput of the relaxed-EMD style loss (csrc/remd.hip).

Three shapes at C = 512: x and y both (16, 512, 64, 64) -- the relu4_1 maps of a batch of 16 images of
512 x 512: 4096 pixels a side, 17 GFLOP per sample in the match --, both (16, 512, 32, 32), and x
(16, 512, 64, 64) against one shared y (1, 512, 64, 64). For each: the match (ast_cosine_match_f32, the
inverse norms given), the whole forward (ops.remd_loss) and the backward (ops.remd_loss_backward, under
the natural branch and under each forced one), the workspace bytes, and beside them the plain PyTorch
formulation on the same device (normalise, bmm, two mins, autograd backward), which stores the
n x M x P distance matrix, with its peak memory. Then the AdaINTrainer step at B = 16, 512 x 512, with
remd_lam = 1 and with remd_lam = 0 (the step as it was) in the same process. HIP events, warm-up
first, the median of --steps intervals of several launches, as bench_swap.py.

    python scripts/bench_remd.py > profiles/remd_bench.txt

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
from arbitrarystyletransfer_amd import _lib, ops, synth  # noqa: E402

PEAK_F32_MFMA = 157.3e12

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


def torch_remd(x, y):
    """The PyTorch-ROCm formulation: the loss as a differentiable function of x."""
    xh = torch.nn.functional.normalize(x.flatten(2), dim=1, eps=0.0).transpose(1, 2)   # [n, M, C]
    yh = torch.nn.functional.normalize(y.flatten(2), dim=1, eps=0.0).expand(x.shape[0], -1, -1)
    d = 1.0 - torch.bmm(xh, yh)
    return torch.maximum(d.min(dim=2).values.mean(dim=1), d.min(dim=1).values.mean(dim=1)).mean()


def torch_fwd_bwd(x, y):
    xg = x.detach().requires_grad_(True)
    loss = torch_remd(xg, y)
    (dx,) = torch.autograd.grad(loss, xg)
    return loss.detach(), dx


def torch_choices(x, y, ridx, cidx):
    """What the PyTorch formulation chose: the branch per sample (1 rows, 2 columns), its arg-mins [n, M]
    and [n, P], and by how much its own distance at our indices exceeds its minimum (rows, columns)."""
    with torch.no_grad():
        xh = torch.nn.functional.normalize(x.flatten(2), dim=1, eps=0.0).transpose(1, 2)
        yh = torch.nn.functional.normalize(y.flatten(2), dim=1, eps=0.0).expand(x.shape[0], -1, -1)
        d = 1.0 - torch.bmm(xh, yh)
        r, c = d.min(dim=2), d.min(dim=1)
        gap_r = d.gather(2, ridx.long()[..., None])[..., 0] - r.values
        gap_c = d.gather(1, cidx.long()[:, None, :])[:, 0] - c.values
        branch = torch.where(r.values.mean(dim=1) >= c.values.mean(dim=1), 1, 2)
    return branch, r.indices, c.indices, gap_r, gap_c


def bench_shape(xs, ys, a, dev):
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    x, y = SR.features(8301, xs).to(dev) + 1e-3, SR.features(8302, ys).to(dev) + 1e-3
    n, c, m, p, ns = xs[0], xs[1], xs[2] * xs[3], ys[2] * ys[3], ys[0]
    flops = 2.0 * n * m * p * c
    r = {"flops": flops}
    print(f"x {xs} vs y {ys}: {m} x {p} pixels, {flops / 1e9:.0f} GFLOP in the match")
    u, v = ops.cosine_norms(x), ops.cosine_norms(y)
    t, lo, hi = timed(lambda: (ops.cosine_norms(x), ops.cosine_norms(y)), a.warmup, a.steps, 10)
    print(f"  inverse norms, both sides    {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    r["norms_ms"] = t
    outs = [torch.empty(n, m, device=dev), torch.empty(n, m, device=dev, dtype=torch.int32),
            torch.empty(n, p, device=dev), torch.empty(n, p, device=dev, dtype=torch.int32)]
    for splits in (0, 1, 2, 4, 8, 16):
        wb = int(L.ast_cosine_match_workspace_bytes(n, ns, m, p, splits))
        ws = torch.empty(wb, device=dev, dtype=torch.uint8)
        t, lo, hi = timed(lambda: L.ast_cosine_match_f32(x.data_ptr(), y.data_ptr(), u.data_ptr(), v.data_ptr(),
                                                         *(o.data_ptr() for o in outs), n, ns, c, m, p, splits,
                                                         ws.data_ptr(), wb, st), a.warmup, a.steps, 3)
        tag = "library's splits" if splits == 0 else f"{splits} split(s)"
        print(f"  cosine_match, {tag:17s}{t * 1e3:9.1f} us  {flops / t / 1e9:6.1f} TFLOP/s = "
              f"{100 * flops / (t * 1e-3) / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak; workspace {wb / 2**20:.1f} MiB "
              f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
        r[f"match_splits{splits}_ms"], r[f"match_splits{splits}_ws_bytes"] = t, wb
        del ws
    r["match_tflops"] = flops / r["match_splits0_ms"] / 1e9
    # what a second, role-swapped launch of a rows-only kernel could at best cost: the same products again
    r["role_swapped_floor_ms"] = 2 * flops / PEAK_F32_MFMA * 1e3
    print(f"  two role-swapped launches cannot take less than 2 x FLOPs / peak = {r['role_swapped_floor_ms'] * 1e3:.1f} us")

    t, lo, hi = timed(lambda: ops.remd_loss(x, y), a.warmup, a.steps, 3)
    print(f"  ops.remd_loss, whole forward {t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    r["forward_ms"] = t
    one = torch.tensor(1.0, device=dev)
    for branch, tag in ((0, "natural"), (1, "rows"), (2, "columns")):
        _, _, _, br, state = ops.remd_loss(x, y, _branch=branch)
        t, lo, hi = timed(lambda: ops.remd_loss_backward(x, y, state, br, one), a.warmup, a.steps, 3)
        print(f"  ops.remd_loss_backward, {tag:8s}{t * 1e3:9.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); branches "
              f"taken: {int((br == 1).sum())} rows, {int((br == 2).sum())} columns")
        r[f"backward_{tag}_ms"] = t
    r["backward_ws_bytes"] = int(L.ast_remd_loss_backward_workspace_bytes(n, m, p))
    ours = r["forward_ms"] + r["backward_natural_ms"]

    if not a.no_torch:
        loss, _, _, br, state = ops.remd_loss(x, y)
        dx = ops.remd_loss_backward(x, y, state, br, one)
        tl, tdx = torch_fwd_bwd(x, y)
        e_l = abs(float(tl) - float(loss))
        # Among thousands of candidates a few pixels have a runner-up within fp32 rounding of the winner,
        # and the two formulations may then choose differently; such a pixel's gradient is another vector
        # altogether. The gradients are compared at the pixels where both made the same choices.
        ridx, cidx = state[3].reshape(n, m), state[5].reshape(n, p)
        tbr, ta, tb, gap_r, gap_c = torch_choices(x, y, ridx, cidx)
        rows, cols = (tbr == 1)[:, None], (tbr == 2)[:, None]
        off = (ridx != ta) & rows                                       # [n, M]: pixels whose gradient may differ
        dcol = (cidx != tb) & cols
        for idx in (cidx.long(), tb):   # the content pixels that either formulation's differing columns chose
            off |= torch.zeros(n, m, device=dev, dtype=torch.int32).scatter_add_(1, idx, dcol.int()) > 0
        off |= (tbr != br)[:, None]
        keep = (~off).reshape(n, 1, *xs[2:]).expand_as(dx)
        e_g = float(((dx - tdx).abs() * keep).max() / tdx.abs().max())
        print(f"  choices: {int((tbr == br).sum())} of {n} branches, all but {int((ridx != ta).sum())} of {n * m} row and "
              f"{int((cidx != tb).sum())} of {n * p} column arg-mins agree; where they differ PyTorch's own distance at "
              f"our index is within {max(float(gap_r.max()), float(gap_c.max())):.2e} of its minimum; {int(off.sum())} "
              f"pixels left out of the gradient comparison")
        del tl, tdx, ta, tb, gap_r, gap_c
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t, lo, hi = timed(lambda: torch_fwd_bwd(x, y), 2, max(3, a.steps // 3), 1)
        peak = torch.cuda.max_memory_allocated() - base
        tf, _, _ = timed(lambda: torch_remd(x, y), 1, max(3, a.steps // 3), 1)
        print(f"  PyTorch normalise / bmm / min / autograd: forward {tf * 1e3:.1f} us, forward + backward {t * 1e3:.1f} us "
              f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), peak memory {peak / 2**20:.0f} MiB; loss differs by {e_l:.2e}, "
              f"gradient (same choices) by {e_g:.2e}; {t / ours:.2f} x ours ({ours * 1e3:.1f} us forward + backward)")
        r.update(torch_forward_ms=tf, torch_fwd_bwd_ms=t, torch_peak_bytes=peak, torch_over_ours=t / ours)
    return r


def bench_trainer(a, dev):
    from arbitrarystyletransfer_amd.train import AdaINTrainer, default_args
    b, s_ = 16, 512
    c = torch.from_numpy(synth.image(8311, (b, 3, s_, s_))).to(dev)
    s = torch.from_numpy(synth.image(8312, (b, 3, s_, s_))).to(dev)
    r = {}
    for lam in (0.0, 1.0):
        tr = AdaINTrainer(default_args(batch_size=b, image_size=s_, remd_lam=lam), device=dev)
        t, lo, hi = timed(lambda: tr.train_step(c, s), 2, max(3, a.steps // 3), 1)
        print(f"AdaINTrainer.train_step B = {b}, {s_} x {s_}, remd_lam = {lam}: {t:.2f} ms  (min {lo:.2f}, max {hi:.2f})")
        r[f"train_step_remd_lam{lam:g}_ms"] = t
        del tr
    r["train_step_ratio"] = r["train_step_remd_lam1_ms"] / r["train_step_remd_lam0_ms"]
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
    for i, (xs, ys) in enumerate(SHAPES):
        res[f"shape{i}"] = dict(bench_shape(xs, ys, a, dev), x=list(xs), y=list(ys))
    if not a.no_trainer:
        res["trainer"] = bench_trainer(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
