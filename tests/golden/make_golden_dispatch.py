"""Writes tests/golden/dispatch_floats.json: what the *_workspace_floats queries of mobilenet.hip,
conv3x3_bwd.hip, losses.hip and mbtrain.hip return over a table of argument tuples, with nothing set and
under every forced expand+depthwise family. ast_mb_expand_dw_workspace_floats and
ast_conv3x3_wgrad_workspace_floats run the plan of the launch itself (the kernel family, its tile grid
and its split count), so a row that moves means that the dispatch of that shape moved.
tests/test_dispatch_queries_cpu.py holds the library to the file row by row.

Run with the library of the commit to record built (AST_HIP_LIB may point at another build of it):
  python tests/golden/make_golden_dispatch.py [--commit SHA]
No GPU is needed: the queries are host code. The switches are read once per process, so every forced
setting is recorded in a fresh child process (`--rows-for KEY` prints that setting's values).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ED = "ast_mb_expand_dw_workspace_floats"
# the settings tests/test_gpu_mb_stages.py forces (its FORCED table), as "VAR=value"; "" is nothing set
SETTINGS = ["", "AST_MB_ED=1", "AST_MB_ED=2", "AST_MB_ED=3", "AST_MB_ED5=0"]


def ed_args(case, fp32):
    """The query tuple of a test_gpu_mb_stages case, formed as its run_stages and DepthWiseConv._plan form it:
    (dtype, has_x2, c1, n, cin, h, w, up, expand, hid, cin_pad, k, stride, ho, wo)."""
    _, inp, _oup, s, t, k, _norm, _ident, (n, h, w), up, split = case
    hid = round(inp * t)
    pad = (k - 1) // 2
    ho, wo = (h * up + 2 * pad - k) // s + 1, (w * up + 2 * pad - k) // s + 1
    expand = t != 1
    align = 4 if fp32 else 16
    cin_pad = (inp + align - 1) // align * align if expand else 0
    dtype = 0 if fp32 else 1
    if not fp32 and expand and cin_pad >= 256 and cin_pad % 32 == 0 and hid % 128 == 0 and s == 1 and up == 1 and k == 3:
        # ada_out: the expand GEMM writes the hidden map, the ratio-1 depthwise follows
        return (dtype, 0, hid, n, hid, h, w, 1, 0, hid, 0, k, s, ho, wo)
    return (dtype, int(split), inp // 2 if split else inp, n, inp, h, w, up, int(expand), hid, cin_pad, k, s, ho, wo)


def ed_table():
    import test_gpu_mb_stages as T
    rows = [(f"bf16/{name}", ed_args(case, False)) for name, case in T.CASES.items()]
    rows += [(f"fp32/{name}", ed_args(T.CASES[name], True)) for name in T.FP32_CASES]
    rows += [  # rejected: the query answers 0
        ("rejected/k7", (1, 0, 16, 1, 16, 12, 12, 1, 1, 96, 16, 7, 1, 12, 12)),
        ("rejected/stride3", (1, 0, 16, 1, 16, 12, 12, 1, 1, 96, 16, 3, 3, 4, 4)),
        ("rejected/wrong_ho", (1, 0, 16, 1, 16, 12, 12, 1, 1, 96, 16, 3, 1, 11, 12)),
        ("rejected/cin_pad_unaligned", (1, 0, 20, 1, 20, 12, 12, 1, 1, 120, 20, 3, 1, 12, 12)),
        ("rejected/ratio1_hid_ne_cin", (1, 0, 24, 1, 24, 12, 12, 1, 0, 48, 0, 3, 1, 12, 12)),
        ("rejected/dtype2", (2, 0, 16, 1, 16, 12, 12, 1, 1, 96, 16, 3, 1, 12, 12)),
    ]
    return rows


# The other queries, with nothing set (no switch reaches them).
OTHER = {
    # (n, cin, h_in, w_in, cout, upsample): the Cout <= 3 MFMA plan (output width % 16 == 0), the small-Cout
    # VALU plan (Cout <= 4, or Cout and Cin <= 16), the general plan, and the aligned shapes (Cin, Cout % 64
    # == 0, W % 32 == 0) whose launch takes the split-bf16 kernel on the general plan's grid
    "ast_conv3x3_wgrad_workspace_floats": [
        (2, 64, 32, 32, 3, 1), (2, 64, 16, 16, 3, 2), (8, 64, 256, 256, 3, 1),
        (2, 64, 9, 13, 3, 1), (2, 5, 7, 9, 4, 1), (1, 16, 9, 13, 16, 2), (2, 3, 12, 20, 16, 1),
        (2, 16, 40, 70, 3, 1), (2, 40, 12, 20, 70, 1), (1, 40, 12, 20, 70, 2), (8, 96, 64, 64, 130, 1),
        (2, 64, 6, 32, 64, 1), (1, 128, 4, 16, 64, 2), (8, 128, 128, 128, 64, 1), (8, 512, 32, 32, 512, 1),
        (0, 64, 32, 32, 3, 1), (2, 64, 32, 32, 3, 3),
    ],
    # (n, c, hw)
    "ast_gram_workspace_floats": [(8, 64, 65536), (8, 128, 16384), (8, 256, 4096), (8, 512, 1024), (1, 64, 262144),
                                  (2, 70, 1000), (1, 3, 100), (0, 64, 4096)],
    # (M, N, batch, ksplit, sCb)
    "ast_mbt_gemm_workspace_floats": [(96, 4096, 1, 1, 0), (96, 16, 1, 8, 0), (96, 16, 4, 1, 0), (96, 16, 4, 1, 1536),
                                      (96, 16, 4, 3, 1536), (0, 16, 1, 1, 0)],
    # (planes, hw)
    "ast_plane_stats_workspace_floats": [(512, 65536), (64, 8192), (64, 8193), (3, 100), (0, 100)],
}


def values(setting):
    from arbitrarystyletransfer_amd import _lib
    lib = _lib.lib()
    out = [int(getattr(lib, ED)(*args)) for _, args in ed_table()]
    if not setting:
        out += [int(getattr(lib, q)(*args)) for q, tuples in OTHER.items() for args in tuples]
    return out


def child_values(setting):
    """values(setting) of a fresh process with only that switch set."""
    env = {k: v for k, v in os.environ.items() if k not in ("AST_MB_ED", "AST_MB_ED5")}
    if setting:
        var, val = setting.split("=")
        env[var] = val
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-for", setting], check=True,
                       capture_output=True, text=True, env=env, cwd=REPO)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the loaded library was built from (default: HEAD)")
    ap.add_argument("--rows-for", default=None, metavar="SETTING", help="print this process's values as JSON and exit")
    a = ap.parse_args()
    if a.rows_for is not None:
        print(json.dumps(values(a.rows_for)))
        return
    commit = a.commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], check=True, capture_output=True,
                                        text=True).stdout.strip()
    rows = []
    for setting in SETTINGS:
        vals = child_values(setting)
        keys = [(ED, case, args) for case, args in ed_table()]
        if not setting:
            keys += [(q, None, args) for q, tuples in OTHER.items() for args in tuples]
        assert len(keys) == len(vals)
        rows += [{"query": q, "setting": setting, "case": case, "args": list(args), "floats": v}
                 for (q, case, args), v in zip(keys, vals)]
    path = os.path.join(HERE, "dispatch_floats.json")
    with open(path, "w") as f:
        f.write("{\n \"recorded_at_commit\": %s,\n \"rows\": [\n" % json.dumps(commit))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]\n}\n")
    zero = sum(r["floats"] == 0 for r in rows)
    print(f"wrote {path}: {len(rows)} rows, {zero} of them 0, library {os.environ.get('AST_HIP_LIB') or 'in tree'}")


if __name__ == "__main__":
    main()
