"""Writes tests/golden/cx_workspace_bytes.json: what every *_workspace_bytes query of cx.hip returns over a
table of argument tuples, error codes included. tests/test_cx_cpu.py holds the library to it row by row,
so a change of a workspace layout that moves a size shows up as a changed row. The table of the other
ops (workspace_bytes.json, make_golden_workspace.py) stays as it is.

Run with the library built:
  python tests/golden/make_golden_cx_workspace.py
No GPU is needed: the queries are host code.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from arbitrarystyletransfer_amd import _lib  # noqa: E402

# (n, ns, m, p): one pixel, the test cases' shapes, the bench shapes, the limits, then the rejected ones
PAIRS = [(1, 1, 1, 1), (1, 1, 9, 5), (2, 2, 63, 66), (2, 1, 156, 165), (1, 1, 72, 399), (1, 1, 460, 42), (1, 1, 64, 1024),
         (1, 1, 4, 306), (16, 16, 4096, 4096), (16, 1, 4096, 4096), (16, 16, 1024, 1024), (4, 4, 16384, 16384),
         (65535, 1, 1, 1),
         (2, 3, 4, 4), (0, 1, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 16385, 4), (1, 1, 4, 16385), (65536, 1, 4, 4),
         (1, 0, 4, 4)]
SPLITS = (0, 1, 4, 100, -1)                 # the library's choice, forced counts, one past the tiles, a bad one
CHANNELS = (1, 48, 512, 1024, 1025, 0)


def table():
    lib = _lib.lib()
    q = lambda name, args: {"args": list(args), "bytes": int(getattr(lib, name)(*args))}  # noqa: E731
    return {
        # (n, ns, m, p, splits)
        "ast_cx_rowsum_workspace_bytes": [q("ast_cx_rowsum_workspace_bytes", a + (s,)) for a in PAIRS for s in SPLITS],
        # (n, ns, m, p)
        "ast_cx_colmax_workspace_bytes": [q("ast_cx_colmax_workspace_bytes", a) for a in PAIRS],
        "ast_cx_loss_workspace_bytes": [q("ast_cx_loss_workspace_bytes", a) for a in PAIRS],
        # (n, c, m, p)
        "ast_cx_loss_backward_workspace_bytes": [q("ast_cx_loss_backward_workspace_bytes", (n, c, m, p))
                                                 for n, _, m, p in PAIRS for c in CHANNELS],
    }


def main():
    t = table()
    path = os.path.join(HERE, "cx_workspace_bytes.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(' "%s": [\n' % k + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]"
                                   for k, v in t.items()) + "\n}\n")
    rows = [r for v in t.values() for r in v]
    print(f"wrote {path}: {len(rows)} rows, {sum(r['bytes'] < 0 for r in rows)} of them error codes, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
