"""Writes tests/golden/workspace_bytes.json: what every *_workspace_bytes query of efdm.hip,
efdm_regions.hip, wct.hip, swap.hip, remd.hip and selfsim.hip returns over a table of argument tuples,
error codes included. tests/test_workspace_queries_cpu.py holds the library to it row by row, so a
change of a workspace layout that moves a size shows up as a changed row.

Run with the library of the commit to record built (AST_HIP_LIB may point at another build of it):
  python tests/golden/make_golden_workspace.py [--commit SHA]
No GPU is needed: the queries are host code.
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
from arbitrarystyletransfer_amd import _lib  # noqa: E402

# query -> argument tuples, in the order of include/ast_hip.h
TABLE = {
    # (n, ns, c, mc, ms): in LDS up to 16384 elements a plane (no workspace), the general path beyond
    "ast_efdm_workspace_bytes": [(2, 2, 8, 4096, 4096), (2, 1, 8, 16385, 300), (1, 1, 3, 100, 70000), (2, 3, 8, 64, 64)],
    # (..., chunk): a chunk forces the general path
    "ast_efdm_ex_workspace_bytes": [(2, 1, 8, 300, 200, 64), (2, 2, 5, 99, 130, 128), (2, 2, 8, 300, 200, 0),
                                    (2, 2, 8, 300, 200, 96)],
    # (planes, m, want_index, chunk)
    "ast_plane_sort_workspace_bytes": [(6, 300, 0, 64), (6, 300, 1, 64), (3, 20000, 0, 0), (3, 20000, 1, 0),
                                       (6, 300, 1, 0), (0, 300, 1, 64)],
    # (n, c, hc, wc, regions, styles, hs, ws)
    "ast_efdm_regions_workspace_bytes": [(2, 8, 9, 11, 3, 2, 7, 9), (1, 64, 32, 32, 8, 1, 64, 64),
                                         (2, 8, 9, 11, 9, 2, 7, 9), (2, 8, 9, 11, 3, 2, 129, 128)],
    # (n, c, m): the split count peaks at 449..512 pixels and dips beyond
    "ast_wct_cov_workspace_bytes": [(2, 72, 448), (2, 72, 449), (2, 72, 512), (2, 72, 513), (1, 512, 4096), (2, 72, 1)],
    # (b, c)
    "ast_wct_sqrt_workspace_bytes": [(3, 72), (1, 1), (32, 512), (3, 1025)],
    "ast_wct_apply_workspace_bytes": [(2, 72), (1, 3), (0, 72)],
    # (n, ns, c, mc, ms)
    "ast_wct_workspace_bytes": [(2, 1, 72, 99, 63), (2, 2, 72, 448, 449), (2, 1, 72, 512, 513), (3, 3, 64, 513, 448),
                                (1, 1, 512, 4096, 4096), (8, 1, 3, 65536, 449), (2, 3, 72, 99, 63)],
    # (n, c, h, w, regions)
    "ast_wct_region_cov_workspace_bytes": [(2, 72, 16, 28, 3), (2, 72, 449, 1, 3), (2, 72, 16, 32, 1), (2, 72, 27, 19, 8),
                                           (1, 512, 64, 64, 4), (2, 72, 9, 11, 9)],
    "ast_wct_region_apply_workspace_bytes": [(2, 72, 9, 11, 3), (2, 72, 27, 19, 8), (1, 512, 64, 64, 4), (2, 72, 0, 11, 3)],
    # (n, c, hc, wc, regions, styles, hs, ws, style_regional)
    "ast_wct_regions_workspace_bytes": [(2, 72, 9, 11, 3, 2, 7, 9, 0), (2, 72, 9, 11, 3, 2, 7, 9, 1),
                                        (2, 72, 16, 28, 3, 2, 449, 1, 0), (2, 72, 16, 28, 3, 2, 449, 1, 1),
                                        (1, 64, 16, 32, 8, 3, 27, 19, 0), (1, 64, 16, 32, 8, 3, 27, 19, 1),
                                        (1, 512, 64, 64, 4, 1, 64, 64, 0), (1, 512, 64, 64, 4, 1, 64, 64, 1),
                                        (2, 72, 9, 11, 3, 65, 7, 9, 0)],
    # (ns, hs, ws)
    "ast_patch_norms_workspace_bytes": [(1, 64, 64), (3, 14, 14), (2, 3, 3), (1, 2, 64)],
    # (n, ns, hc, wc, hs, ws, splits): the library's own choice (splits 0) is many splits at n = 1 of
    # 64 x 64 and one at n = 128
    "ast_patch_match_workspace_bytes": [(1, 1, 64, 64, 64, 64, 0), (1, 1, 64, 64, 64, 64, 1), (1, 1, 64, 64, 64, 64, 3),
                                        (128, 128, 64, 64, 64, 64, 0), (128, 1, 64, 64, 64, 64, 3), (8, 8, 64, 64, 64, 64, 0),
                                        (2, 1, 12, 12, 14, 14, 0), (2, 2, 12, 12, 14, 14, 1), (2, 2, 12, 12, 14, 14, 3),
                                        (2, 2, 12, 12, 14, 14, 100), (2, 2, 12, 12, 14, 14, -1), (2, 3, 12, 12, 14, 14, 0)],
    # (n, ns, hc, wc, hs, ws)
    "ast_style_swap_workspace_bytes": [(1, 1, 64, 64, 64, 64), (128, 128, 64, 64, 64, 64), (128, 1, 64, 64, 64, 64),
                                       (2, 1, 12, 12, 14, 14), (2, 2, 5, 4, 40, 50), (128, 1, 12, 12, 64, 64),
                                       (2, 2, 12, 2, 14, 14)],
    # (n, s, hc, wc, hs, ws, splits)
    "ast_patch_match_guided_workspace_bytes": [(1, 1, 64, 64, 64, 64, 0), (1, 3, 64, 64, 64, 64, 0),
                                               (128, 1, 64, 64, 64, 64, 0), (128, 3, 64, 64, 64, 64, 0),
                                               (2, 1, 12, 12, 14, 14, 1), (2, 3, 12, 12, 14, 14, 1),
                                               (2, 1, 12, 12, 14, 14, 3), (2, 3, 12, 12, 14, 14, 3),
                                               (2, 2, 12, 12, 14, 14, 0), (2, 0, 12, 12, 14, 14, 0)],
    # (n, s, hc, wc, hs, ws)
    "ast_style_swap_guided_workspace_bytes": [(1, 1, 64, 64, 64, 64), (1, 3, 64, 64, 64, 64), (128, 1, 64, 64, 64, 64),
                                              (128, 3, 64, 64, 64, 64), (2, 2, 12, 12, 14, 14), (128, 3, 12, 12, 64, 64),
                                              (2, 2, 12, 12, 14, 2)],
    # (n, ns, m, p, splits): the library's own choice is 4 splits at 32 x 32 and 2 at 64 x 64, n = 16
    "ast_cosine_match_workspace_bytes": [(16, 16, 1024, 1024, 0), (16, 16, 1024, 1024, 1), (16, 16, 1024, 1024, 3),
                                         (16, 1, 4096, 4096, 0), (16, 16, 4096, 4096, 1), (16, 1, 4096, 4096, 3),
                                         (1, 1, 4096, 1024, 0), (1, 1, 100, 200, 0), (2, 2, 70, 130, 1), (2, 1, 70, 130, 3),
                                         (2, 2, 70, 130, 100), (2, 2, 70, 130, -1), (2, 2, 0, 130, 0)],
    # (n, ns, m, p)
    "ast_remd_loss_workspace_bytes": [(16, 16, 1024, 1024), (16, 1, 4096, 4096), (1, 1, 4096, 1024), (2, 1, 70, 130),
                                      (1, 1, 1024, 16384), (2, 3, 70, 130)],
    # (n, m, p)
    "ast_remd_loss_backward_workspace_bytes": [(16, 1024, 1024), (2, 70, 130), (1, 63, 1), (2, 70, 4194305)],
    # (n, c)
    "ast_selfsim_colsum_workspace_bytes": [(2, 8), (16, 512), (2, 1025), (0, 8)],
    # (n, pixels)
    "ast_selfsim_pairs_workspace_bytes": [(2, 130), (16, 4096), (1, 64), (1, 65), (2, 16385)],
    # (n, c, pixels)
    "ast_selfsim_loss_workspace_bytes": [(2, 8, 130), (16, 512, 4096), (1, 3, 64), (2, 0, 130)],
    "ast_selfsim_loss_backward_workspace_bytes": [(2, 8, 130), (16, 512, 4096), (1, 3, 65), (70000, 8, 130)],
}


def rows():
    lib = _lib.lib()
    return [{"query": name, "args": list(args), "bytes": int(getattr(lib, name)(*args))}
            for name, tuples in TABLE.items() for args in tuples]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the loaded library was built from (default: HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], check=True, capture_output=True,
                                        text=True).stdout.strip()
    out = {"recorded_at_commit": commit, "rows": rows()}
    path = os.path.join(HERE, "workspace_bytes.json")
    with open(path, "w") as f:
        f.write("{\n \"recorded_at_commit\": %s,\n \"rows\": [\n" % json.dumps(commit))
        f.write(",\n".join("  " + json.dumps(r) for r in out["rows"]))
        f.write("\n ]\n}\n")
    neg = sum(r["bytes"] < 0 for r in out["rows"])
    print(f"wrote {path}: {len(out['rows'])} rows, {neg} of them error codes, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
