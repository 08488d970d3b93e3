"""CPU: the host-only part of the conv C ABI -- the number of configurations and the sizes of the
weight packs -- pinned to literals recorded from the build before the conv source was split into
one translation unit per kernel family (no GPU needed: nothing is launched)."""
import pytest

from arbitrarystyletransfer_amd import _lib


def test_num_configs():
    assert _lib.lib().ast_conv3x3_num_configs() == 44


@pytest.mark.parametrize("cout,cin,packed,up2c", [
    (64, 3, 18432, 24576),
    (3, 64, 92160, 98304),
    (128, 40, 129024, 147456),
    (512, 512, 5898240, 6291456),
])
def test_pack_sizes(cout, cin, packed, up2c):
    L = _lib.lib()
    assert L.ast_conv3x3_packed_numel(cout, cin) == packed
    assert L.ast_conv3x3_up2c_numel(cout, cin) == up2c
