"""Throughput of exact feature distribution matching and the plane sort (csrc/efdm.hip).

Times ast_efdm_f32 at (8, 512, 64, 64) for both maps -- the relu4_1 maps of benchmark config 2, the
fused path -- beside ast_adain_f32 and a same-size torch.Tensor.copy_ on the same tensors in the
same process (HIP events, warm-up first, the median of the timed intervals, as bench_regions.py);
the same shape forced through the chunk-sort + merge path; plane_sort at one general-path shape,
(8, 64, 512, 512), the relu1_1 tap of a 512 x 512 batch; and the model level:
AdaINStyleTransfer(transform="efdm") against the default at B = 8, 512 x 512.

    python scripts/bench_efdm.py > profiles/efdm_bench.txt

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
    x = ER.features(6001, shape).to(dev)
    s = ER.features(6002, shape).to(dev)
    out = torch.empty_like(x)
    nbytes = 3 * x.numel() * 4   # read c, read s, write out
    t_copy, _, _ = timed(lambda: out.copy_(x), a.warmup, a.steps)
    print(f"{shape} fp32 content and style, {n * c} planes of {h * w}; {nbytes / 1e6:.1f} MB read + written per call")
    print(f"  copy_ (2/3 of the bytes)  {t_copy * 1e3:9.1f} us")
    t_adain, lo, hi = timed(lambda: L.ast_adain_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n, c, h, w, h, w, 1.0,
                                                    1, st), a.warmup, a.steps)
    print(f"  adain                     {t_adain * 1e3:9.1f} us  {nbytes / t_adain / 1e6:6.0f} GB/s  "
          f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["copy_ms"], res["adain_ms"] = t_copy, t_adain
    for alpha in (1.0, 0.8):
        t, lo, hi = timed(lambda: L.ast_efdm_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n, n, c, h, w, h, w, alpha,
                                                 None, 0, st), a.warmup, a.steps)
        print(f"  efdm fused, alpha={alpha}     {t * 1e3:9.1f} us  {nbytes / t / 1e6:6.0f} GB/s  {t / t_adain:6.2f} x adain  "
              f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
        res[f"efdm_fused_alpha{alpha}_ms"] = t
    res["efdm_to_adain"] = res["efdm_fused_alpha1.0_ms"] / t_adain
    chunk = 1024
    wsb = int(L.ast_efdm_ex_workspace_bytes(n, n, c, h * w, h * w, chunk))
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    t, lo, hi = timed(lambda: L.ast_efdm_ex_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n, n, c, h, w, h, w, 1.0,
                                                chunk, ws.data_ptr(), wsb, st), a.warmup, max(5, a.steps // 3), reps=2)
    print(f"  efdm general, chunk={chunk} {t * 1e3:9.1f} us  ({wsb / 1e6:.0f} MB workspace, 2 merge passes)  "
          f"{t / t_adain:6.2f} x adain  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    res["efdm_general_chunk1024_ms"] = t
    del ws

    pshape = (8, 64, 512, 512)
    xp = ER.features(6003, pshape).to(dev)
    vals = torch.empty_like(xp)
    idx = torch.empty(pshape, device=dev, dtype=torch.int32)
    planes, m = pshape[0] * pshape[1], pshape[2] * pshape[3]
    print(f"plane_sort {pshape}: {planes} planes of {m} (general path, chunks of 4096, 6 merge passes)")
    for want in (0, 1):
        wsb = int(L.ast_plane_sort_workspace_bytes(planes, m, want, 0))
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
        t, lo, hi = timed(lambda: L.ast_plane_sort_f32(xp.data_ptr(), vals.data_ptr(), idx.data_ptr() if want else None,
                                                       planes, m, 0, ws.data_ptr(), wsb, st), 2, max(5, a.steps // 3),
                          reps=1)
        print(f"  {'values + indices' if want else 'values only     '}  {t:9.3f} ms  {planes * m / t / 1e6:7.2f} G keys/s  "
              f"({wsb / 1e9:.2f} GB workspace; min {lo:.3f}, max {hi:.3f})")
        res["plane_sort_idx_ms" if want else "plane_sort_ms"] = t
        del ws
    del xp, vals, idx

    ci = torch.from_numpy(synth.image(6101, (8, 3, 512, 512))).to(dev)
    si = torch.from_numpy(synth.image(6102, (8, 3, 512, 512))).to(dev)
    t_model = {}
    for transform in ("adain", "efdm"):
        net = models.AdaINStyleTransfer(weights="live", transform=transform).to(dev)
        with torch.no_grad():
            t_model[transform] = timed(lambda: net(ci, si), 2, max(5, a.steps // 3), reps=1)
    print("model forward, 8 x 3 x 512 x 512 content and style:")
    for transform, (t, lo, hi) in t_model.items():
        print(f"  transform={transform:6s}  {t:8.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    d = t_model["efdm"][0] - t_model["adain"][0]
    print(f"  efdm - adain = {d:.3f} ms, {100 * d / t_model['efdm'][0]:.1f} % of the efdm forward")
    res["model"] = {"adain_ms": t_model["adain"][0], "efdm_ms": t_model["efdm"][0], "added_ms": d}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
