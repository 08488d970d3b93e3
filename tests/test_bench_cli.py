"""CPU: bench.py's command line (--full, --dump-outputs) and the output dump (no GPU: nothing is
launched, the dump is exercised on CPU tensors)."""
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_extras(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs, a.mode) == (7, 2, False, None, "fwd")
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_float32_named_files(tmp_path):
    out = {"loss": torch.tensor(1.5, dtype=torch.float64), "img": torch.arange(24.0).reshape(2, 3, 4).bfloat16(),
           "_private": torch.zeros(3), "note": "not a tensor"}
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["img.npy", "loss.npy"]
    img = np.load(tmp_path / "d" / "img.npy")
    assert img.dtype == np.float32 and img.shape == (2, 3, 4)
    np.testing.assert_array_equal(img.ravel(), np.arange(24, dtype=np.float32))
    assert float(np.load(tmp_path / "d" / "loss.npy")) == 1.5
    bench.dump_outputs(str(tmp_path / "d"), {"img": torch.zeros(2)}, rank=1, world=2)
    assert (tmp_path / "d" / "img.rank1.npy").exists()


def test_dump_outputs_samples_large_outputs_the_same_way(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)   # two files: 500 float32 each
    x = torch.arange(10000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": x.reshape(100, 100), "small": x[:10]})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (500,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and 0 <= a[0] and a[-1] < 10000   # sorted positions of the flat output
    assert np.load(tmp_path / "a" / "small.npy").shape == (10,)
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= 4000 + 2 * 128   # payload within the limit (+ the .npy headers)
