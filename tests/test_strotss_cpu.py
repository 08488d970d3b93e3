"""CPU: the schedule of the optimisation-based stylizer (arbitrarystyletransfer_amd/strotss.py) -- scale
sizes, skipped scales, the level cap, the content weights and the pixel-limit check are pure functions."""
import inspect

import pytest

from arbitrarystyletransfer_amd import _lib, models, ops, strotss


def test_scale_size_keeps_aspect_on_multiples_of_16():
    S = strotss.scale_size
    assert S((512, 512), 64) == (64, 64) and S((512, 512), 512) == (512, 512)
    assert S((64, 48), 64) == (64, 48) and S((64, 48), 32) == (32, 32)       # 24 rounds half up to 32
    assert S((80, 64), 32) == (32, 32) and S((80, 64), 64) == (64, 48)       # 25.6 -> 32, 51.2 -> 48
    assert S((333, 517), 256) == (160, 256) and S((517, 333), 256) == (256, 160)   # 164.9 -> 160
    assert S((333, 517), 4096) == (336, 512)                                 # never above the image's own size (517 -> 512)
    assert S((1000, 37), 128) == (128, 16) and S((37, 1000), 128) == (16, 128)     # 4.7 -> the minimum side
    assert S((7, 9), 64) == (16, 16)                                         # a tiny image still gets 16
    assert S((99, 101), 100) == (96, 96) and S((101, 99), 101) == (96, 96)
    for size in ((333, 517), (64, 48), (1, 1), (4095, 17)):
        for s in (1, 15, 16, 17, 63, 64, 100, 511, 512, 513):
            h, w = S(size, s)
            assert h % 16 == 0 and w % 16 == 0 and h >= 16 and w >= 16
            assert max(h, w) <= max(16, 16 * ((min(s, max(size)) + 8) // 16))
    with pytest.raises(ValueError):
        S((0, 4), 64)
    with pytest.raises(ValueError):
        S((4, 4), 0)


def test_schedule_skips_repeated_sizes_and_keeps_the_scale_index():
    sched = strotss.scale_schedule((64, 48), (32, 64))
    assert sched == [(0, (32, 32)), (1, (64, 48))]
    assert strotss.scale_schedule((100, 100), (64, 128, 256, 512)) == [(0, (64, 64)), (1, (96, 96))]
    assert strotss.scale_schedule((333, 517), strotss.DEFAULT_SCALES) == [
        (0, (48, 64)), (1, (80, 128)), (2, (160, 256)), (3, (336, 512))]
    assert strotss.scale_schedule((20, 20), (8, 16, 24)) == [(0, (16, 16))]
    assert strotss.scale_schedule((40, 40), (16, 16, 40)) == [(0, (16, 16)), (2, (48, 48))]
    assert strotss.DEFAULT_SCALES == (64, 128, 256, 512)


def test_level_cap():
    assert strotss.level_cap((512, 512), 5) == 5 and strotss.level_cap((16, 16), 5) == 4
    assert strotss.level_cap((16, 512), 9) == 4 and strotss.level_cap((48, 32), 5) == 5
    assert strotss.level_cap((37, 50), 7) == 5 and strotss.level_cap((1, 9), 3) == 0
    assert strotss.level_cap((64, 64), 0) == 0
    for size in ((37, 50), (16, 16), (333, 517)):       # the coarsest level keeps a side of at least one real pixel
        n = strotss.level_cap(size, 99)
        assert min(size) >> n >= 1 and min(size) >> (n + 1) == 0
    with pytest.raises(ValueError):
        strotss.level_cap((8, 8), -1)


def test_content_weight_halves_per_scale():
    assert [strotss.content_weight_at(16.0, k) for k in range(4)] == [16.0, 8.0, 4.0, 2.0]
    assert strotss.content_weight_at(3.0, 2) == 0.75 and strotss.content_weight_at(0.0, 3) == 0.0


def test_tap_strides_and_limits():
    assert [strotss.tap_stride(t) for t in ("conv_1", "conv_3", "conv_5", "conv_9", "relu_9", "conv_13", "relu_15")] == [
        1, 2, 4, 8, 8, 16, 16]
    sched = strotss.scale_schedule((2048, 2048), (512, 1024, 2048))
    sizes = [(64, 64)] * 3
    strotss.check_limits(sched[:2], sizes, ("relu_9", "relu_15"), ("relu_9",), True, True)    # 128^2 = 16384: the limit itself
    with pytest.raises(_lib.HipOpError, match="self-similarity tap relu_9"):
        strotss.check_limits(sched, sizes, ("relu_9", "relu_15"), ("relu_9",), True, True)    # 256^2 at relu_9
    strotss.check_limits(sched, sizes, ("relu_9",), ("relu_9",), False, True)                 # the term is off
    strotss.check_limits(sched, sizes, ("relu_15",), ("relu_9",), True, True)                 # 128^2 at relu_15
    with pytest.raises(_lib.HipOpError, match="relaxed-EMD tap conv_1"):
        strotss.check_limits(sched[:1], [(4096, 4096)], ("relu_15",), ("conv_1",), True, True)
    assert ops.SELFSIM_MAX_PIXELS == 16384


def test_public_surface():
    sig = inspect.signature(strotss.StrotssStylizer.stylize)
    want = dict(init=None, scales=(64, 128, 256, 512), iters=200, lr=2e-3, content_weight=16.0, levels=5,
                remd_taps=("relu_9", "relu_15"), moment_taps=("relu_9", "relu_15"), selfsim_taps=("relu_9", "relu_15"),
                remd_lam=1.0, moment_lam=1.0, graph=True, return_history=False, clamp=False)
    got = {k: p.default for k, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
    assert got == want
    assert list(inspect.signature(strotss.StrotssStylizer.__init__).parameters) == ["self", "lossnet", "device"]
    assert list(inspect.signature(models.AdaINStyleTransfer.refine).parameters)[:4] == [
        "self", "content_img", "style_img", "stylizer"]
