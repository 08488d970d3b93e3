#!/usr/bin/env python3
"""Step boundaries of the software-pipelined MFMA loops, read from the compiler's assembly.

python scripts/x3_boundaries.py FILE.s [KERNEL_SUBSTRING]
FILE.s: a kernel source compiled with the Makefile's flags plus --cuda-device-only -S. For every
kernel whose name holds KERNEL_SUBSTRING (default conv3x3_x3_kernel), between its first and last
v_mfma: the number of MFMAs and of LDS reads, every LDS wait (s_waitcnt lgkmcnt(N)) with the
instructions around it -- M an MFMA, r a ds_read, wN the wait, . anything else -- and how many
lgkmcnt(0) waits come within two instructions of a ds_read (a step that opens by waiting out a read
issued just before it). Registers, scratch and occupancy are the compiler's own figures."""
import collections
import re
import sys


def kernels(path, sub):
    name, body, info = None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body, info = m.group(1), [], {}
            continue
        if name is None:
            continue
        s = line.strip()
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", s)
        if m:
            info[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                if sub in name:
                    yield name, body, info
                name = None
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        body.append(s.split(";")[0].strip())


def code(s):
    if s.startswith("v_mfma"):
        return "M"
    if s.startswith("ds_read"):
        return "r"
    m = re.search(r"lgkmcnt\((\d+)\)", s) if s.startswith("s_waitcnt") else None
    return f"w{m.group(1)}" if m else "."


def main():
    path, sub = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "conv3x3_x3_kernel")
    for name, body, info in kernels(path, sub):
        c = [code(s) for s in body]
        mf = [i for i, k in enumerate(c) if k == "M"]
        if not mf:
            continue
        lo, hi = mf[0], mf[-1]
        pats, bad = collections.Counter(), 0
        for i in range(lo, hi + 1):
            if c[i][0] != "w":
                continue
            # MFMAs issued since the last read that the wait covers
            j, since = i - 1, 0
            while j >= lo and c[j] != "r":
                since += c[j] == "M"
                j -= 1
            pats[" ".join(c[max(lo, i - 3):i + 3]) + f"   [{since} MFMA since the last read]"] += 1
            bad += c[i] == "w0" and "r" in c[max(lo, i - 2):i]
        targs = re.search(r"kernelI(.*?)EEv", name)
        print(f"{sub}<{targs.group(1).replace('Li', ',').replace('ELb', ',b').replace('E', '').lstrip(',') if targs else name}>: "
              f"VGPRs {info.get('NumVgprs')} AGPRs {info.get('NumAgprs')} scratch {info.get('ScratchSize')} "
              f"occupancy {info.get('Occupancy')}; MFMA phase: {len(mf)} MFMA, {c[lo:hi + 1].count('r')} ds_read, "
              f"lgkmcnt(0) within two instructions of a ds_read: {bad}")
        for p, n in sorted(pats.items(), key=lambda kv: -kv[1]):
            print(f"    {n:3d} x  {p}")


if __name__ == "__main__":
    main()
