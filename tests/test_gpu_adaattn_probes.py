"""GPU: the AdaAttN forward against the exact probes of tests/adaattn_probe_ref.py, in fp32 and bf16,
on shapes that reach every form of the attention launch: attend_bf16_kernel<1..4, 8> (the 8-wave
kernel of large batches), the 4-wave kernel over many key blocks without a split, the key splits
with attn_merge_kernel, and the fp32 kernels on the same shapes. Every test first asserts, through
ast_adaattn_plan, that its case is launched as the table says, so a retune of the split or of the
8-wave threshold cannot silently move a case off the kernel it was written for.

  uniform  pins the tail mask (a padded key has the same logit as a real one) and the V mean add-back
  planted  pins where each key's V ends up (the V slot shuffle, the ragged last block, key splits,
           query tiles): out[:, i] == V[:, pi(i)] in bits, twice, and through ops.adaattn
  twin     pins accumulation across 16-key groups, key blocks and key splits and the merge weights

The calls go to the C ABI with an output full of NaN and a workspace full of 0xFF bytes (NaN in
either dtype): whatever the kernels read they must have written.

Bounds (adaattn_probe_ref.py): planted exact; uniform and twin |out - ref| <= slack (fp32) and
<= ulp_bf16(ref) / 2 + slack (bf16). Largest err / bound measured on an MI355X, over all cases (each
test prints its own; the module prints these maxima as it finishes):
  uniform  fp32 0.056   bf16 0.9987 (the half ulp of the output; 0.028 of the slack used beyond it)
  twin     fp32 0.035   bf16 0.9984 (0.006 of the slack used)
  planted  0 elements differ in either dtype on every case (margins 223 .. 1528 nats, g = 4 or 8)
With the purely relative slack 2^-18 (|std IN(c)| + |mean|), i.e. without the term for the content
mean's absolute fp32 error, the same outputs miss on isolated pixels that sit on their plane's mean:
fp32 uniform up to 16384 x (7102 of 8.9 M elements at 256 x 128 x 17 x 16, 3 .. 549 elsewhere), fp32
twin up to 10 x (14 elements), bf16 uniform up to 25 x (36 elements). That term is why it is there.
Two value-only mutants of attend_bf16_kernel were run once against this file and the whole-op bars
of test_gpu_adaattn.py: one padded key counted by the softmax fails test_uniform[*-bf16] on all ten
ragged cases and passes every whole-op bar; V slots stored in the wrong order fails all three probes.
"""
import numpy as np
import pytest
import torch

import adaattn_probe_ref as P
from arbitrarystyletransfer_amd import _lib, ops, synth
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16)}
ALL_CASES = P.CASES + P.MEAN_CASES
WORST = {}   # (probe, dtype) -> largest err / bound, printed as the module's tests finish


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print()
    for (kind, what), r in sorted(WORST.items()):
        print(f"adaattn probe {kind:8s} {what + (':' if ' ' in what else ' err / bound:'):26s} largest = {r:.4f}")


def forward(dev, code, content, style, wq, wk, wv):
    """ast_adaattn_fwd into a NaN-filled output, from a workspace of 0xFF bytes."""
    L = _lib.lib()
    n, c, hc, wc = content.shape
    hs, ws = style.shape[2:]
    content, style = content.contiguous(), style.contiguous()
    w = [t.to(dev, torch.float32).contiguous() for t in (wq, wk, wv)]
    out = torch.full_like(content, float("nan"))
    nbytes = L.ast_adaattn_workspace_bytes(code, n, c, hc, wc, hs, ws)
    wsb = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    _lib.check(L.ast_adaattn_fwd(code, _lib.ptr(content), _lib.ptr(style), _lib.ptr(w[0]), _lib.ptr(w[1]), _lib.ptr(w[2]),
                                 _lib.ptr(out), _lib.ptr(wsb), nbytes, n, c, hc, wc, hs, ws, _lib.stream_ptr(dev)),
               "adaattn")
    torch.cuda.synchronize(dev)
    return out


def run_probe(dev, pr, dt, images=slice(None)):
    code, dtype = DTYPES[dt]
    return forward(dev, code, pr.content[images].to(dev, dtype), pr.style[images].to(dev, dtype), pr.wq, pr.wk, pr.wv)


def assert_plan(case, dt):
    """The launch is the one the table names (fp32: always 4 waves; its split is its own)."""
    shape, waves, split, _ = case
    pl = P.plan(DTYPES[dt][0], shape)
    if dt == "bf16":
        assert pl.waves == waves and (pl.ksplit > 1) == split, (shape, vars(pl))
    else:
        assert pl.waves == 4, (shape, vars(pl))
    return pl


def held_to_bound(out, pr, kind, dt):
    assert bool(torch.isfinite(out).all()), "the output kept a NaN it was filled with (or made one)"
    worst, ratio = P.err_over_bound(out, pr, DTYPES[dt][1])
    rel_only, r2 = P.err_over_bound(out, pr, DTYPES[dt][1], relative_only=True)
    used = P.slack_used(out, pr) if dt == "bf16" else worst
    print(f"adaattn probe {kind} {dt} {pr.shape}: err / bound = {worst:.4f}, slack used {used:.4f}; with the purely "
          f"relative slack {rel_only:.4f} ({int((r2 > 1).sum())} elements over)")
    for key, val in (((kind, dt), worst), ((kind, dt + " slack used"), used), ((kind, dt + " relative slack only"), rel_only)):
        WORST[key] = max(WORST.get(key, 0.0), val)
    assert worst <= 1.0, (kind, dt, pr.shape, worst, int((ratio > 1).sum()))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ALL_CASES, ids=[P.case_id(c) for c in ALL_CASES])
def test_uniform(case, dt, hip_device):
    assert_plan(case, dt)
    pr = P.uniform(case[0], with_mean=case in P.MEAN_CASES)
    held_to_bound(run_probe(hip_device, pr, dt), pr, "uniform", dt)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_planted_key(case, dt, hip_device):
    assert_plan(case, dt)
    pr = P.planted(case[0])
    out = run_probe(hip_device, pr, dt)
    assert bool(torch.isfinite(out).all())
    wrong = int((out.double().cpu() != pr.ref).sum())
    print(f"adaattn probe planted {dt} {pr.shape}: g = {pr.g}, margin {pr.margin:.0f} nats, {wrong} elements differ")
    assert wrong == 0, (dt, pr.shape, wrong)
    assert torch.equal(run_probe(hip_device, pr, dt), out)
    dtype = DTYPES[dt][1]
    again = ops.adaattn(pr.content.to(hip_device, dtype), pr.style.to(hip_device, dtype),
                        *(t.to(hip_device) for t in (pr.wq, pr.wk, pr.wv)))
    assert torch.equal(again, out)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_twin_keys(case, dt, hip_device):
    pl = assert_plan(case, dt)
    (n, c, hc, wc, hs, ws) = case[0]
    nk, step = hs * ws, pl.kchunk * 32 if pl.ksplit > 1 else 0
    pr = P.twin(case[0], step)
    # the pairs the queries aim at, held against the planned split: they really straddle one
    aimed = pr.pairs[pr.tgt.unique().numpy()]
    got = P.twin_placements(aimed, nk, step)
    assert got == {"same16": True, "blocks": nk > 32, "splits": pl.ksplit > 1, "adjacent_splits": pl.ksplit > 1,
                   "last": True}, (case[0], vars(pl), got)
    if pl.ksplit > 1:
        a, b = aimed[:, 0] // step, aimed[:, 1] // step
        assert max(a.max(), b.max()) == pl.ksplit - 1 and bool(np.any((a == 0) & (b == pl.ksplit - 1)))
    held_to_bound(run_probe(hip_device, pr, dt), pr, "twin", dt)


@pytest.mark.parametrize("case", [c for c in P.CASES if c[1] == 8], ids=[P.case_id(c) for c in P.CASES if c[1] == 8])
def test_8_wave_and_4_wave_kernels_agree(case, hip_device):
    """One image of a large batch alone is launched on the 4-wave kernel, inside its batch on the
    8-wave kernel: on the planted probe both give the same bits."""
    shape = case[0]
    assert P.plan(1, shape).waves == 8 and P.plan(1, (1,) + shape[1:]).waves == 4
    pr = P.planted(shape)
    batch = run_probe(hip_device, pr, "bf16")
    for b in (0, shape[0] // 2 + 1, shape[0] - 1):
        alone = run_probe(hip_device, pr, "bf16", slice(b, b + 1))
        assert torch.equal(alone[0], batch[b]), (shape, b)
        assert bool((alone[0].double().cpu() == pr.ref[b]).all())


@pytest.mark.parametrize("shape", [(512, 128, 3, 5, 5, 7), (256, 64, 17, 16, 7, 10)])
def test_8_wave_random_data_vs_oracle(shape, hip_device):
    """The 8-wave kernel at the bar of test_gpu_adaattn.test_adaattn_bf16_vs_oracle: rel_inf <= 2e-2
    against the fp32 oracle on the same bf16-rounded inputs (bf16 Q / K / V / P rounding)."""
    n, c, hc, wc, hs, ws = shape
    assert P.plan(1, shape).waves == 8
    x = synth.uniform(4000 + c, n * c * hc * wc).astype(np.float32).reshape(n, c, hc, wc) * 2.0 - 0.3
    y = synth.uniform(4001 + c, n * c * hs * ws).astype(np.float32).reshape(n, c, hs, ws) * 1.5
    w = [torch.from_numpy(synth.conv_weight(4002 + c + i, c, c, 1).reshape(c, c)) for i in range(3)]
    w[0], w[1] = w[0] * 0.15, w[1] * 0.15
    xb, yb = (torch.from_numpy(t).to(torch.bfloat16) for t in (x, y))
    out = forward(hip_device, 1, xb.to(hip_device), yb.to(hip_device), *w)
    assert out.dtype == torch.bfloat16 and bool(torch.isfinite(out).all())
    ref = R.adaattn(xb.float(), yb.float(), *w).double()
    err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"adaattn 8-wave random {shape}: rel_inf = {err:.3e}")
    assert err <= 2e-2, (shape, err)
