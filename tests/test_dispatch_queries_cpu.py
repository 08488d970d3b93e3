"""The dispatch of the expand+depthwise stage and of the 3x3 weight gradient, pinned through their
workspace queries to the values recorded in tests/golden/dispatch_floats.json
(tests/golden/make_golden_dispatch.py): ast_mb_expand_dw_workspace_floats and
ast_conv3x3_wgrad_workspace_floats run the plan of the launch itself, so a shape that moves to another
kernel family or tile grid moves its row. Every case of tests/test_gpu_mb_stages.py is a row, with
nothing set and, in fresh child processes (the switches are read once per process), under each setting
that test forces. ast_gram_, ast_mbt_gemm_ and ast_plane_stats_workspace_floats are pinned beside them.
The queries are host code: no GPU is needed."""
import json
import os
import subprocess
import sys

import pytest

from arbitrarystyletransfer_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "dispatch_floats.json")
with open(PATH) as f:
    GOLDEN = json.load(f)
ROWS = GOLDEN["rows"]
ED = "ast_mb_expand_dw_workspace_floats"
SETTINGS = ["", "AST_MB_ED=1", "AST_MB_ED=2", "AST_MB_ED=3", "AST_MB_ED5=0"]


def _rows(setting):
    return [r for r in ROWS if r["setting"] == setting]


def test_table_covers_the_stage_cases_and_every_query():
    import test_gpu_mb_stages as T
    assert {s for _, _, _, names in T.FORCED for s in names} <= set(T.CASES)
    assert {f"{var}={val}" for var, val, _, _ in T.FORCED} == set(SETTINGS[1:])
    want = {f"bf16/{n}" for n in T.CASES} | {f"fp32/{n}" for n in T.FP32_CASES}
    for setting in SETTINGS:
        ed = [r for r in _rows(setting) if r["query"] == ED]
        accepted = {r["case"] for r in ed if not r["case"].startswith("rejected/")}
        assert accepted == want, setting
        assert sum(r["case"].startswith("rejected/") for r in ed) >= 3
        for r in ed:  # every accepted row was planned by a kernel family at the recorded commit
            assert (r["floats"] == 0) == r["case"].startswith("rejected/"), r
    assert {r["setting"] for r in ROWS} == set(SETTINGS)
    others = {r["query"] for r in _rows("")} - {ED}
    assert others == {"ast_conv3x3_wgrad_workspace_floats", "ast_gram_workspace_floats", "ast_mbt_gemm_workspace_floats",
                      "ast_plane_stats_workspace_floats"}
    wg = [r["args"] for r in ROWS if r["query"] == "ast_conv3x3_wgrad_workspace_floats"]
    for up in (1, 2):  # the Cout <= 3 MFMA plan, the small-Cout plan, the general plan, the aligned shapes
        assert any(a[4] <= 3 and a[3] * up % 16 == 0 and a[5] == up for a in wg)
        assert any((a[4] == 4 or (a[4] <= 16 and a[1] <= 16)) and a[5] == up for a in wg)
        assert any(a[4] > 16 and a[4] % 64 and a[5] == up for a in wg)
        assert any(a[4] % 64 == 0 and a[1] % 64 == 0 and a[3] * up % 32 == 0 and a[5] == up for a in wg)


@pytest.mark.parametrize("row", _rows(""), ids=lambda r: r["query"][4:-17] + "-" + (r["case"] or "x".join(map(str, r["args"]))))
def test_query_returns_recorded_value(row):
    got = int(getattr(_lib.lib(), row["query"])(*row["args"]))
    assert got == row["floats"], (row, got, GOLDEN["recorded_at_commit"])


_CHILD = ("import json, sys; from arbitrarystyletransfer_amd import _lib; "
          "print(json.dumps([int(getattr(_lib.lib(), q)(*a)) for q, a in json.loads(sys.argv[1])]))")


@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_forced_family_returns_recorded_values(setting):
    rows = _rows(setting)
    env = {k: v for k, v in os.environ.items() if k not in ("AST_MB_ED", "AST_MB_ED5")}
    var, val = setting.split("=")
    env[var] = val
    calls = json.dumps([[r["query"], r["args"]] for r in rows])
    out = subprocess.run([sys.executable, "-c", _CHILD, calls], cwd=os.path.dirname(HERE), check=True,
                         capture_output=True, text=True, timeout=120, env=env).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert got == [r["floats"] for r in rows], [(r["case"], r["floats"], g) for r, g in zip(rows, got) if g != r["floats"]]
