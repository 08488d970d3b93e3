"""Writes tests/golden/color.npz: inputs and expected outputs of the reference's colour helpers.

It imports the reference's own model_util.py (torch-only, imports as is) from AST_REFERENCE_DIR and
runs its six functions on synthetic images; only input and output tensors are written, no
reference source. Run in the build container:  python tests/golden/make_golden_color.py

Keys (tag: s99 = (2,3,9,11), HW odd, scalar path, N > 1; s128 = (1,3,8,16), the vector path):
  {tag}_{fn}_x         fp32 input of fn: x, rgb2xyz(x), xyz2lab(rgb2xyz(x)) or rgb2lab(x)
  {tag}_{fn}_ref64     the reference run in float64 on that input
  {tag}_{fn}_noise32   max |reference in fp32 - ref64|
  wide_{fn}_x / _out32 / _nan / _ref64 / _noise32   for rgb2xyz, rgb2lab, xyz2lab on (2,3,9,11):
                       x*1.6 - 0.3 (xyz2lab: the s99 input with one X and one Y negative), the
                       reference's fp32 output, its NaN mask; noise32 over the finite elements
  grad_{fn}_x / _g / _g32 / _g64 / _noise32         rgb2lab and lab2rgb input gradients for a fixed
                       cotangent g, inputs from x clamped to >= 0.02 (the reference's autograd is
                       finite there)
  luma_{tag}_s / _c / _ref64 / _noise32             luma_transfer composed from the reference
                       functions: lab2rgb(cat(L(rgb2lab(clamp01(s))), ab(rgb2lab(clamp01(c)))))
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AST_REFERENCE_DIR", "/root/reference")
sys.path.insert(0, REPO)
from arbitrarystyletransfer_amd import synth  # noqa: E402

FNS = ("rgb2xyz", "xyz2rgb", "xyz2lab", "lab2xyz", "rgb2lab", "lab2rgb")
SHAPES = {"s99": ((2, 3, 9, 11), 901), "s128": ((1, 3, 8, 16), 902)}


def load_reference():
    path = os.path.join(REF, "model_util.py")
    if not os.path.exists(path):
        raise SystemExit(f"reference not found at {REF}; golden vectors are generated in the build container only")
    spec = importlib.util.spec_from_file_location("ref_model_util", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stage_input(R, fn, x):
    if fn in ("rgb2xyz", "rgb2lab"):
        return x
    if fn in ("xyz2rgb", "xyz2lab"):
        return R.rgb2xyz(x)
    if fn == "lab2xyz":
        return R.xyz2lab(R.rgb2xyz(x))
    return R.rgb2lab(x)


def noise(a32, a64):
    d = (a32.double() - a64).abs()
    return np.float64(d[torch.isfinite(d)].max().item())


def main():
    R = load_reference()
    out = {}
    for tag, (shape, seed) in SHAPES.items():
        x = torch.from_numpy(synth.image(seed, shape))
        for fn in FNS:
            xin = stage_input(R, fn, x).float().contiguous()
            f = getattr(R, fn)
            y32, y64 = f(xin), f(xin.double())
            assert y32.dtype == torch.float32 and y64.dtype == torch.float64
            assert torch.isfinite(y64).all(), (tag, fn)
            out[f"{tag}_{fn}_x"] = xin.numpy()
            out[f"{tag}_{fn}_ref64"] = y64.numpy()
            out[f"{tag}_{fn}_noise32"] = noise(y32, y64)
            print(f"{tag} {fn}: noise32 {out[f'{tag}_{fn}_noise32']:.2e}  scale {y64.abs().max().item():.3g}")

    shape, seed = SHAPES["s99"]
    x = torch.from_numpy(synth.image(seed, shape))
    wide = x * 1.6 - 0.3
    xyz = R.rgb2xyz(x).float().clone()
    xyz[0, 0, 2, 3] = -0.01   # one negative X: poisons a alone
    xyz[1, 1, 4, 5] = -0.02   # one negative Y: poisons L, a and b
    for fn, xin in (("rgb2xyz", wide), ("rgb2lab", wide), ("xyz2lab", xyz)):
        f = getattr(R, fn)
        y32, y64 = f(xin), f(xin.double())
        assert torch.equal(torch.isnan(y32), torch.isnan(y64)), fn
        out[f"wide_{fn}_x"] = xin.numpy()
        out[f"wide_{fn}_out32"] = y32.numpy()
        out[f"wide_{fn}_nan"] = torch.isnan(y32).numpy()
        out[f"wide_{fn}_ref64"] = y64.numpy()
        out[f"wide_{fn}_noise32"] = noise(y32, y64)
        print(f"wide {fn}: {(xin < -0.055).sum().item()} of {xin.numel()} inputs below -0.055, "
              f"{torch.isnan(y32).sum().item()} of {y32.numel()} outputs NaN, "
              f"noise32 {out[f'wide_{fn}_noise32']:.2e}")

    g = torch.from_numpy(synth.image(903, shape)) - 0.5
    xc = x.clamp(min=0.02)
    for fn, xin in (("rgb2lab", xc), ("lab2rgb", R.rgb2lab(xc).float())):
        f = getattr(R, fn)
        grads = []
        for dt in (torch.float32, torch.float64):
            leaf = xin.to(dt).clone().requires_grad_(True)
            f(leaf).backward(g.to(dt))
            assert torch.isfinite(leaf.grad).all(), (fn, dt)
            grads.append(leaf.grad)
        out[f"grad_{fn}_x"] = xin.numpy()
        out[f"grad_{fn}_g"] = g.numpy()
        out[f"grad_{fn}_g32"] = grads[0].numpy()
        out[f"grad_{fn}_g64"] = grads[1].numpy()
        out[f"grad_{fn}_noise32"] = noise(grads[0], grads[1])
        print(f"grad {fn}: noise32 {out[f'grad_{fn}_noise32']:.2e}  scale {grads[1].abs().max().item():.3g}")

    def luma(s, c):
        ls, lc = R.rgb2lab(s.clamp(0, 1)), R.rgb2lab(c.clamp(0, 1))
        return R.lab2rgb(torch.cat([ls[:, :1], lc[:, 1:]], dim=1))

    for tag, (shape, seed) in SHAPES.items():
        s = torch.from_numpy(synth.image(seed + 10, shape)) * 1.6 - 0.3   # decoder-like: outside [0, 1]
        c = torch.from_numpy(synth.image(seed + 20, shape)) * 1.2 - 0.1
        y32, y64 = luma(s, c), luma(s.double(), c.double())
        assert torch.isfinite(y64).all()
        out[f"luma_{tag}_s"] = s.numpy()
        out[f"luma_{tag}_c"] = c.numpy()
        out[f"luma_{tag}_ref64"] = y64.numpy()
        out[f"luma_{tag}_noise32"] = noise(y32, y64)
        print(f"luma {tag}: noise32 {out[f'luma_{tag}_noise32']:.2e}")

    path = os.path.join(HERE, "color.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
