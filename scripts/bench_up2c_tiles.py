#!/usr/bin/env python3
"""Launch times of the two forms of the collapsed upsampled conv (conv3x3_up2c_kernel: 8 waves, one
workgroup per CU / 4 waves, two per CU) over batch sizes of the three decoder layers -- the
measurement behind the selection rule of launch_up2c.
python scripts/bench_up2c_tiles.py [REPS]
Per shape: workgroups of either form, median launch time of REPS rounds (each round: 20 launches
of one form between two events, the forms alternating), the ratio, and the form auto takes."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from arbitrarystyletransfer_amd import ops, synth  # noqa: E402
from arbitrarystyletransfer_amd._lib import lib  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda")
cdiv = lambda a, b: -(-a // b)  # noqa: E731
print(f"{'n x cin x h x w -> cout':28s} {'wg8':>6s} {'wg4':>6s} {'t8 us':>9s} {'t4 us':>9s} {'t4/t8':>7s}  auto")
for cin, hw in ((256, 64), (128, 128), (64, 256)):
    wp = ops.pack_conv3x3(torch.from_numpy(synth.conv_weight(6, cin, cin, 3)).to(dev), up2c=True)
    b = torch.from_numpy(synth.conv_bias(7, cin)).to(dev)
    for n in (1, 2, 4, 8):
        x = torch.from_numpy(synth.image(5, (n, cin, hw, hw))).to(dev)
        t = {8: [], 4: []}
        for r in range(reps + 1):
            for tile in ((8, 4) if r % 2 == 0 else (4, 8)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    ops.conv3x3(x, wp, b, cin, upsample=2, pad_mode="reflect", _up2c_tile=tile)
                e1.record()
                e1.synchronize()
                if r:  # round 0 warms up
                    t[tile].append(e0.elapsed_time(e1) * 1e3 / 20)
        m8, m4 = statistics.median(t[8]), statistics.median(t[4])
        tiles = lambda th: (cdiv(n * cdiv(2 * hw, 32) * cdiv(2 * hw, th), 8) * 8) * cdiv(cin, 32)  # noqa: E731
        sep = "4 < 8" if max(t[4]) < min(t[8]) else ("8 < 4" if max(t[8]) < min(t[4]) else "overlap")
        print(f"{n:2d} x {cin:3d} x {hw:3d} x {hw:3d} -> {cin:3d}   {tiles(32):6d} {tiles(16):6d} {m8:9.1f} {m4:9.1f} "
              f"{m4 / m8:7.3f}  {lib().ast_conv3x3_up2c_variant(n, cin, hw, hw, cin)}  ({sep})", flush=True)
        del x
