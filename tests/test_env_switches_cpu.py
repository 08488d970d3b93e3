"""Every AST_* environment switch the package still reads is accounted for. The C side reads a switch
only through ast_env::get (csrc/env.h, the one getenv of the library), the Python side through
os.environ.get. The names found in csrc/*.hip, csrc/*.h and the package's *.py must equal the lists
below; every C-side name must also be named by a file under tests/ or by a script outside
scripts/debug/ (a switch that only a debug script knows is a settled A/B measurement: retire it and
the code only it reaches), and every name must appear in DESIGN.md, whose table of the remaining
switches says what each selects."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "arbitrarystyletransfer_amd")

C_SWITCHES = {"AST_MB_ED", "AST_MB_ED5", "AST_ATTN_KSPLIT", "AST_UP2C_TILE", "AST_MBGEMM_VEC", "AST_CONV_M16"}
PY_SWITCHES = {"AST_HIP_LIB", "AST_ADAATTN_FLASH", "AST_MB_EDPW", "AST_MBGEMM_AUTOSPLIT", "AST_MBT_FUSE", "AST_CONV_TUNING",
               "AST_CONV_UP2C", "AST_CONV_PACK"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc():
    return sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")))


def test_c_side_reads_exactly_the_listed_switches_once_each():
    reads = []
    for path in _csrc():
        text = _read(path)
        reads += re.findall(r'ast_env::get\(\s*"(AST_[A-Z0-9_]+)"', text)
        # no reader beside env.h's: neither a literal name nor a variable handed to getenv
        if os.path.basename(path) != "env.h":
            assert "getenv" not in text, path
    assert re.findall(r"getenv\(([^)]*)\)", _read(os.path.join(PKG, "csrc", "env.h"))) == ["name"]
    assert sorted(reads) == sorted(C_SWITCHES), sorted(reads)  # equal as lists: one reader per switch


def test_python_side_reads_exactly_the_listed_switches():
    reads = set()
    for path in glob.glob(os.path.join(PKG, "*.py")):
        text = _read(path)
        reads |= set(re.findall(r'os\.environ\.get\(\s*"(AST_[A-Z0-9_]+)"', text))
        for other in re.findall(r'os\.(?:getenv\(|environ\[)\s*"(AST_[A-Z0-9_]+)"', text):
            raise AssertionError(f"{path}: {other} is read by another form than os.environ.get")
    assert reads == PY_SWITCHES, sorted(reads ^ PY_SWITCHES)


def test_every_c_switch_is_named_by_a_test_or_a_script():
    me = os.path.abspath(__file__)
    files = [p for p in glob.glob(os.path.join(REPO, "tests", "**", "*"), recursive=True) if os.path.isfile(p)]
    files += [p for p in glob.glob(os.path.join(REPO, "scripts", "**", "*"), recursive=True)
              if os.path.isfile(p) and os.sep + "debug" + os.sep not in p[len(REPO):]]
    texts = []
    for p in files:
        if os.path.abspath(p) == me or not p.endswith((".py", ".sh")):
            continue
        texts.append(_read(p))
    for name in sorted(C_SWITCHES):
        assert any(re.search(name + r"\b", t) for t in texts), name


def test_every_switch_is_in_design_md():
    design = _read(os.path.join(REPO, "DESIGN.md"))
    for name in sorted(C_SWITCHES | PY_SWITCHES):
        assert re.search(r"`" + name + r"`", design), name
