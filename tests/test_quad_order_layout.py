"""CPU check of the quadrant table's layout arithmetic (nnrt_fit_quad_order_blocks: the static grid of the pixel launch
when it reads the per-frame quadrant table): equal to the restatement, a whole number of workgroups per XCD band, and
enough entries for every split of the quadrants into working and idle ones."""
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


def np_blocks(Q):
    return 8 * (((Q + 7) // 8 + 1 + 3) // 4)


@pytest.mark.parametrize("Q", [1, 4, 31, 32, 33, 4800, 19200])
def test_quad_order_blocks(lib, Q):
    blocks = lib.nnrt_fit_quad_order_blocks(Q)
    assert blocks == np_blocks(Q) and blocks % 8 == 0
    per_band = 4 * blocks // 8   # entries of one band
    # a band holds its eighth of the working and its eighth of the idle quadrants: the largest band of every split fits,
    # with less than two workgroups of padding beyond the even share
    splits = range(Q + 1) if Q <= 4800 else list(range(0, Q + 1, 7)) + [Q]
    for W in splits:
        I = Q - W
        need = max(((x + 1) * W // 8 - x * W // 8) + ((x + 1) * I // 8 - x * I // 8) for x in range(8))
        assert need <= per_band
    assert per_band - (Q + 7) // 8 < 8
    assert 4 * blocks >= Q
    assert lib.nnrt_fit_quad_order_blocks(0) == 0
