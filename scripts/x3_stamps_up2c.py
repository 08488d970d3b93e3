#!/usr/bin/env python3
"""Phase timing of the collapsed upsampled conv (conv3x3_up2c_kernel, both forms) from in-kernel
clock stamps, at the phase boundaries scripts/x3_stamps.py reads for the 9-tap kernel.

Diagnostic only: needs the X3_STAMP build (bash scripts/build_variants.sh stamp "-DX3_STAMP=1"
conv_up2c.hip), selected through AST_HIP_LIB. The stamps never reach an output.
python scripts/x3_stamps_up2c.py OUTDIR TILE [n cin h_in w_in cout]     (TILE = 8 | 4)
Writes OUTDIR/up2c_stamps_t<TILE>_<shape>.npz (raw records) and prints the per-phase summary
(python scripts/x3_stamps_up2c.py FILE.npz prints it again from the records)."""
import ctypes
import os
import sys
import time

import numpy as np

MFMA_PER_CHUNK = 192  # per wave: 16 phase-taps x 2 source rows x 2 channel tiles x 3 products
MFMA_CYC = 16         # v_mfma_f32_16x16x32_bf16 issue cycles on one SIMD


def summary(rec):
    waves = rec[(rec[:, :, 196] == 0x57a3) & (rec[:, :, 197] != 0)]
    if len(waves) == 0:
        print("no up2c records")
        return
    nch, form = int(waves[0, 195]), int(waves[0, 197])
    wm, slabs = form // 16, form % 16
    st = waves[:, :192].astype(np.int64)
    d = lambda a, b: ((st[:, b] - st[:, a]) % (1 << 32)).astype(float)  # noqa: E731
    med = lambda v: float(np.median(v))  # noqa: E731
    total = d(0, 3 + 4 * nch)
    mf = np.stack([d(2 + 4 * k, 3 + 4 * k) for k in range(nch)], 1)
    nk = range(nch - 1)
    zero = np.zeros((len(st), 1))
    b1 = np.stack([d(3 + 4 * k, 4 + 4 * k) for k in nk], 1) if nch > 1 else zero
    sto = np.stack([d(4 + 4 * k, 5 + 4 * k) for k in nk], 1) if nch > 1 else zero
    per = np.stack([d(2 + 4 * k, 6 + 4 * k) for k in nk], 1) if nch > 1 else zero
    parts = {"prologue (slab DMA, gather, split, A write, barrier)": d(0, 1),
             "MFMA phases (next chunk's gather" + (", slab DMA" if slabs == 2 else "") + " issued inside)": mf.sum(1),
             "split + barrier 1": b1.sum(1),
             ("A write + barrier 2" if slabs == 2 else "slab DMA + A write + landing + barrier 2"): sto.sum(1),
             "last MFMAs to epilogue (barrier)": d(3 + 4 * (nch - 1), 2 + 4 * nch),
             "epilogue (staged stores, to vmcnt 0)": d(2 + 4 * nch, 3 + 4 * nch)}
    tot = med(total)
    print(f"{wm} waves, {slabs} slab buffer(s); {len(st)} waves of {len(st) // wm} workgroups, {nch} K chunks; "
          f"cycles per wave (median over waves):")
    for k, v in parts.items():
        print(f"  {k:58s} {med(v):9.0f}  {med(v) / tot:6.1%}")
    print(f"  {'total (workgroup resident)':58s} {tot:9.0f}")
    print(f"  per chunk: MFMA phase {med(mf):.0f} (p10 {np.percentile(mf, 10):.0f}, p90 {np.percentile(mf, 90):.0f}; "
          f"{MFMA_PER_CHUNK} MFMAs alone on a SIMD: {MFMA_PER_CHUNK * MFMA_CYC}, two waves sharing it: "
          f"{2 * MFMA_PER_CHUNK * MFMA_CYC}); split + barrier 1 {med(b1):.0f}; store phase {med(sto):.0f}; "
          f"chunk period {med(per):.0f}")
    if slabs == 1 and nch > 1:
        land = np.stack([d(120 + k, 5 + 4 * k) for k in nk], 1)
        issue = np.stack([d(4 + 4 * k, 120 + k) for k in nk], 1)
        print(f"  single slab buffer: DMA issue + A write {med(issue):.0f}, exposed landing wait + barrier 2 "
              f"{med(land):.0f} (p90 {np.percentile(land, 90):.0f}) per chunk")
    fixed = tot - (nch - 1) * med(per) - med(mf)
    print(f"  fit: block = {fixed:.0f} + {nch} x {med(per):.0f} cycles (prologue + last-chunk tail + epilogue = {fixed:.0f})")
    hw = waves[:, 192]
    cu = (hw >> 8) & 0xff | (waves[:, 193] & 0xf) << 8  # HW_ID's CU, SH and SE fields, and the XCC
    first = waves[:, 0].astype(np.int64)
    ncu = len(np.unique(cu))
    print(f"  recorded workgroups ran on {ncu} distinct (XCC, SE, CU) ids; SIMD ids of the first workgroup's waves: "
          f"{list(((hw >> 4) & 3)[:wm])}; entry-stamp spread over workgroups {int(first.max() - first.min())} (clock wraps ignored)")


def main():
    if sys.argv[1].endswith(".npz"):
        summary(np.load(sys.argv[1])["rec"])
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.environ.setdefault("AST_HIP_LIB", os.path.join(root, "build_var", "libast_hip_stamp.so"))
    sys.path.insert(0, root)
    import torch
    from arbitrarystyletransfer_amd import _lib, ops, synth

    out, tile = sys.argv[1], int(sys.argv[2])
    n, cin, h, w, cout = (int(v) for v in sys.argv[3:8]) if len(sys.argv) > 3 else (8, 64, 256, 256, 64)
    dev = torch.device("cuda")
    fn = _lib.lib().ast_dbg_x3_stamps
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    x = torch.from_numpy(synth.image(5, (n, cin, h, w))).to(dev)
    wp = ops.pack_conv3x3(torch.from_numpy(synth.conv_weight(6, cout, cin, 3)).to(dev), up2c=True)
    b = torch.from_numpy(synth.conv_bias(7, cout)).to(dev)

    def run():
        ops.conv3x3(x, wp, b, cout, upsample=2, pad_mode="reflect", _up2c_tile=tile)

    t0 = time.time()
    while time.time() - t0 < 1.5:  # back-to-back launches so the clock settles
        for _ in range(10):
            run()
        torch.cuda.synchronize()
    _lib.check(fn(None, 0, 1), "stamp clear")
    run()
    torch.cuda.synchronize()
    nwg, nrec = 2048, 200
    buf = np.zeros(nwg * 16 * nrec, dtype=np.uint32)
    _lib.check(fn(buf.ctypes.data, buf.nbytes, 0), "stamp read")
    tag = f"t{tile}_{n}x{cin}x{h}x{w}_{cout}"
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, f"up2c_stamps_{tag}.npz"), rec=buf.reshape(nwg, 16, nrec))
    print(tag)
    summary(buf.reshape(nwg, 16, nrec))


if __name__ == "__main__":
    main()
