"""nnrt_voxel_grid_ray_cast without a GPU: the entry point is exported and bound, and it refuses null and out-of-range
arguments on the host before the grid is read or any device work starts (tests/test_native_abi.py shows the pattern: a
made-up non-null address stands in for a handle the checks never reach)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def native():
    import os
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_ray_cast_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    assert "nnrt_voxel_grid_ray_cast" in native.exported_symbols()
    K = np.array([[80.0, 0.0, 31.5], [0.0, 80.0, 23.5], [0.0, 0.0, 1.0]])
    fake = 0x7f0000000000   # never dereferenced: every call below is refused by a check that comes before the grid is read

    def call(grid=fake, k=K, range_map=fake + 0x1000, coords=fake + 0x2000, count=4, width=64, height=48, mask=1, depth_scale=1000.0,
             depth_min=0.1, depth_max=3.0, f=8, depth=fake + 0x3000):
        st = lib.nnrt_voxel_grid_ray_cast(ctypes.c_void_p(grid), ctypes.c_void_p(coords), count, native.ptr(k), None, width, height, mask,
                                          depth_scale, depth_min, depth_max, 3.0, 8.0, f, ctypes.c_void_p(range_map), ctypes.c_void_p(depth),
                                          None, None, None, None)
        return st, lib.nnrt_last_error()

    for kw, text in ((dict(grid=None), b"null grid"), (dict(k=None), b"null intrinsic"), (dict(range_map=None), b"null range"),
                     (dict(coords=None), b"null block coordinates"), (dict(count=-1), b"null block coordinates"),
                     (dict(width=0), b"width and height"), (dict(height=-3), b"width and height"), (dict(f=0), b"range_map_down_factor"),
                     (dict(depth_min=-0.5), b"depth limits"), (dict(depth_min=3.0), b"depth limits"), (dict(depth_min=float("nan")), b"depth limits"),
                     (dict(depth_scale=0.0), b"depth_scale"), (dict(mask=32), b"attribute_mask"), (dict(depth=None), b"null depth map"),
                     (dict(mask=2), b"null vertex map"), (dict(mask=4), b"null normal map"), (dict(mask=8), b"null color map")):
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    with pytest.raises(native.NnrtError):
        native.check(call(grid=None)[0])
