"""Every *_workspace_bytes query of the EFDM, WCT, swap, rEMD and self-similarity ops, pinned to the
values recorded in tests/golden/workspace_bytes.json (tests/golden/make_golden_workspace.py), error
codes included. The queries are host code: no GPU is needed. A workspace layout and its query are one
function in csrc, so a row that moves means that a layout moved."""
import json
import os

import pytest

from arbitrarystyletransfer_amd import _lib

PATH = os.path.join(os.path.dirname(__file__), "golden", "workspace_bytes.json")
with open(PATH) as f:
    GOLDEN = json.load(f)
ROWS = GOLDEN["rows"]


def test_table_covers_every_query():
    queries = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")
               and n.split("_")[1] in ("efdm", "plane", "wct", "patch", "style", "cosine", "remd", "selfsim")}
    assert len(queries) == 23
    assert {r["query"] for r in ROWS} == queries
    assert len(ROWS) >= 60
    for q in queries:  # an accepted and a rejected tuple each
        vals = [r["bytes"] for r in ROWS if r["query"] == q]
        assert min(vals) < 0 <= max(vals), q


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r["query"][4:-16] + "-" + "x".join(str(a) for a in r["args"]))
def test_query_returns_recorded_value(row):
    got = int(getattr(_lib.lib(), row["query"])(*row["args"]))
    assert got == row["bytes"], (row, got, GOLDEN["recorded_at_commit"])
