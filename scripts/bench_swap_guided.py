"""Cost of guidance in the style-swap match (csrc/swap.hip): ast_patch_match_guided_ex_f32 against
ast_patch_match_ex_f32.

At C = 512 and 64 x 64 maps -- 3844 patches, 61 tiles of 64, a side -- for n = 1 and n = 8:
  (a) one class and a bank of one style against the unguided match: the same work, so the difference
      is what guidance itself costs (the class compare in the fold, the mask reads, the mask pre-kernel)
  (b) K = 2 and K = 4 horizontal bands on both sides, with the tile skip and without it
  (c) a bank of S = 4 styles, the content's quadrants as classes and region k -> style k, against the
      one-class match over the same bank and against four separate unguided matches
Beside every time stands the number of (content tile, bank tile) visits, counted on the host from the
same class-presence masks the kernel builds, and the time per visit, to be set against the unguided
kernel's time per tile pair of the same run. The inverse norms are computed once outside the timed
region. HIP events, warm-up first; the variants of a group alternate inside every step, so they see the
same clocks and the same neighbours; the median of --steps intervals of --reps launches each, with the
minimum and maximum as the spread.

    python scripts/bench_swap_guided.py > profiles/swap_guided_bench.txt

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

MT = 64   # patches per tile


def alternate(fns, warmup, steps, reps):
    """{name: (median, min, max) ms per launch}; inside a step every variant runs once, in turn."""
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


def tile_masks(cls):
    """Per map, the class-presence mask (a Python int) of every 64-patch tile of cls uint8 [B, h, w]."""
    flat = cls.reshape(cls.shape[0], -1).tolist()
    res = []
    for row in flat:
        masks = []
        for t in range(0, len(row), MT):
            m = 0
            for v in set(row[t:t + MT]):
                if v < ops.SWAP_MAX_CLASSES:
                    m |= 1 << v
            masks.append(m)
        res.append(masks)
    return res


def visits(cc, sc, skip=True):
    """(content tile, bank tile) pairs the guided kernel multiplies."""
    cm, bm = tile_masks(cc), [m for style in tile_masks(sc) for m in style]
    if not skip:
        return len(cm) * len(cm[0]) * len(bm)
    return sum(1 for sample in cm for a in sample for b in bm if a & b)


def bands(b, h, w, k):
    """uint8 [b, h, w]: k horizontal bands of patch rows."""
    rows = (torch.arange(h) * k // h).to(torch.uint8)
    return rows.view(1, h, 1).expand(b, h, w).contiguous()


def quadrants(b, h, w):
    y = (torch.arange(h) >= h // 2).to(torch.uint8).view(1, h, 1)
    x = (torch.arange(w) >= w // 2).to(torch.uint8).view(1, 1, w)
    return (2 * y + x).expand(b, h, w).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
    c_, h, w, S = 512, 64, 64, 4
    ph, pw = h - 2, w - 2
    m = ph * pw
    tiles = (m + MT - 1) // MT
    bank = SR.features(8302, (S, c_, h, w)).to(dev)
    inv = torch.empty(S, m, device=dev)
    nb = int(L.ast_patch_norms_workspace_bytes(S, h, w))
    wn = torch.empty(nb, device=dev, dtype=torch.uint8)
    _lib.check(L.ast_patch_norms_f32(bank.data_ptr(), inv.data_ptr(), S, c_, h, w, wn.data_ptr(), nb, st), "norms")

    for n in a.batches:
        x = SR.features(8301, (n, c_, h, w)).to(dev)
        idx = torch.empty(n, m, device=dev, dtype=torch.int32)
        score = torch.empty(n, m, device=dev)
        keep = []   # class maps and workspaces stay alive while their launches are timed

        def unguided(style):
            mb = int(L.ast_patch_match_workspace_bytes(n, 1, h, w, h, w, 0))
            wm = torch.empty(mb, device=dev, dtype=torch.uint8)
            keep.append(wm)
            sp, ip = bank[style].data_ptr(), inv[style].data_ptr()
            return lambda: L.ast_patch_match_ex_f32(x.data_ptr(), sp, ip, idx.data_ptr(), score.data_ptr(), n, 1, c_, h,
                                                    w, h, w, 0, wm.data_ptr(), mb, st)

        def guided(s, cc, sc, skip=True):
            ccd, scd = cc.to(dev), sc.to(dev)
            mb = int(L.ast_patch_match_guided_workspace_bytes(n, s, h, w, h, w, 0))
            wm = torch.empty(mb, device=dev, dtype=torch.uint8)
            keep.extend([ccd, scd, wm])
            flags = 0 if skip else 1
            return lambda: L.ast_patch_match_guided_ex_f32(x.data_ptr(), bank.data_ptr(), inv.data_ptr(), ccd.data_ptr(),
                                                           scd.data_ptr(), idx.data_ptr(), score.data_ptr(), n, s, c_, h,
                                                           w, h, w, 0, flags, wm.data_ptr(), mb, st)

        zc, zs1, zs4 = (torch.zeros(b, ph, pw, dtype=torch.uint8) for b in (n, 1, S))
        by_style = torch.arange(S, dtype=torch.uint8).view(S, 1, 1).expand(S, ph, pw).contiguous()
        four = [unguided(k) for k in range(S)]
        groups = {
            "(a) one class, one style": {
                "unguided ast_patch_match_ex_f32": (unguided(0), n * tiles * tiles),
                "guided, one class": (guided(1, zc, zs1), visits(zc, zs1)),
            },
            "(b) horizontal bands on both sides, one style": {
                "unguided ast_patch_match_ex_f32": (unguided(0), n * tiles * tiles),
                **{f"guided, K = {k}, skip {'on' if skip else 'off'}":
                   (guided(1, bands(n, ph, pw, k), bands(1, ph, pw, k), skip),
                    visits(bands(n, ph, pw, k), bands(1, ph, pw, k), skip)) for k in (2, 4) for skip in (True, False)},
            },
            "(c) bank of 4 styles, content quadrant k -> style k": {
                "guided, quadrant classes": (guided(S, quadrants(n, ph, pw), by_style),
                                             visits(quadrants(n, ph, pw), by_style)),
                "guided, one class over the bank": (guided(S, zc, zs4), visits(zc, zs4)),
                "four unguided matches, one per style": (lambda: [f() for f in four], S * n * tiles * tiles),
            },
        }
        print(f"n = {n}: content ({n}, {c_}, {h}, {w}), bank of up to {S} styles ({c_}, {h}, {w}); {m} patches = {tiles} "
              f"tiles a map; {a.steps} steps of {a.reps} launches, variants alternating")
        r = {}
        for title, group in groups.items():
            print(f"  {title}")
            t = alternate({k: f for k, (f, _) in group.items()}, a.warmup, a.steps, a.reps)
            for k, (_, v) in group.items():
                med, lo, hi = t[k]
                print(f"    {k:40s}{med * 1e3:10.1f} us  (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}); {v:7d} tile visits, "
                      f"{med * 1e6 / v:7.1f} ns per visit")
                r[f"{title[:3]} {k}"] = {"ms": med, "min_ms": lo, "max_ms": hi, "visits": v}
        res[f"n{n}"] = r
        del keep, four, groups
    print(json.dumps(res))


if __name__ == "__main__":
    main()
