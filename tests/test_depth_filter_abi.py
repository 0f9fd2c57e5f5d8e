"""nnrt_filter_depth and nnrt_bilateral_filter_depth without a GPU: both are exported and bound, and they refuse null and
out-of-range arguments on the host before any device work, naming the argument (tests/test_ray_cast_abi.py shows the
pattern: made-up non-null addresses stand in for images the checks never reach). Empty images are no error."""
import ctypes

import numpy as np
import pytest

FAKE = 0x7f0000000000   # never dereferenced
UINT16, FLOAT32 = 1, 0


@pytest.fixture(scope="module")
def native():
    import os
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_median_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    assert "nnrt_filter_depth" in native.exported_symbols()

    def call(d_in=FAKE, height=48, width=64, radius=1, preserve_zero=0, d_out=FAKE + 0x10000):
        st = lib.nnrt_filter_depth(ctypes.c_void_p(d_in), height, width, radius, preserve_zero, ctypes.c_void_p(d_out), None)
        return st, lib.nnrt_last_error()

    for kw, text in ((dict(radius=-1), b"radius"), (dict(radius=9), b"radius"), (dict(height=-1), b"height or width"),
                     (dict(width=-2), b"height or width"), (dict(d_in=None), b"null d_in"), (dict(d_out=None), b"null d_out"),
                     (dict(d_out=FAKE), b"d_out must not be d_in"), (dict(height=0, radius=9), b"radius")):
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    for kw in (dict(height=0), dict(width=0), dict(height=0, width=0, d_in=None, d_out=None), dict(width=0, d_in=None, d_out=None, radius=8)):
        assert call(**kw)[0] == 0, kw
    with pytest.raises(native.NnrtError):
        native.check(call(radius=-1)[0])


def test_bilateral_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    assert "nnrt_bilateral_filter_depth" in native.exported_symbols()
    spatial = np.ones(9, np.float32)
    weights = np.ones(4, np.float32)

    def call(d_in=FAKE, dtype=UINT16, height=48, width=64, radius=1, spatial=spatial, weights=weights, count=4, index_scale=1.0,
             depth_scale=1000.0, d_out=FAKE + 0x10000):
        st = lib.nnrt_bilateral_filter_depth(ctypes.c_void_p(d_in), dtype, height, width, radius, native.ptr(spatial), native.ptr(weights), count,
                                             index_scale, depth_scale, ctypes.c_void_p(d_out), None)
        return st, lib.nnrt_last_error()

    def with_entry(table, index, value):
        t = table.copy()
        t[index] = value
        return t

    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(radius=-1), b"radius"), (dict(radius=9), b"radius"), (dict(count=0), b"range_weight_count"),
                     (dict(count=4097), b"range_weight_count"), (dict(count=-5), b"range_weight_count"),
                     (dict(depth_scale=0.0), b"depth_scale"), (dict(depth_scale=-1.0), b"depth_scale"), (dict(depth_scale=nan), b"depth_scale"),
                     (dict(depth_scale=inf), b"depth_scale"), (dict(index_scale=0.0), b"range_index_scale"),
                     (dict(index_scale=-2.0), b"range_index_scale"), (dict(index_scale=nan), b"range_index_scale"),
                     (dict(index_scale=inf), b"range_index_scale"), (dict(spatial=None), b"null h_spatial_weights"),
                     (dict(weights=None), b"null h_range_weights"), (dict(dtype=2), b"in_dtype"), (dict(dtype=-1), b"in_dtype"),
                     (dict(height=-1), b"height or width"), (dict(width=-1), b"height or width"), (dict(d_in=None), b"null d_in"),
                     (dict(d_out=None), b"null d_out"), (dict(spatial=with_entry(spatial, 8, -0.5)), b"h_spatial_weights"),
                     (dict(spatial=with_entry(spatial, 0, nan)), b"h_spatial_weights"), (dict(weights=with_entry(weights, 3, inf)), b"h_range_weights"),
                     (dict(weights=with_entry(weights, 1, -1e-30)), b"h_range_weights"),
                     (dict(height=0, weights=None), b"null h_range_weights"), (dict(width=0, radius=9), b"radius")):
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    # entries past the tables' stated sizes are not read: radius 0 takes one spatial weight, count 1 one range weight
    assert call(height=0, radius=0, spatial=with_entry(spatial, 1, nan), count=1, weights=with_entry(weights, 1, nan))[0] == 0
    for kw in (dict(height=0), dict(width=0, dtype=FLOAT32), dict(height=0, width=0, d_in=None, d_out=None), dict(height=0, radius=8, spatial=np.ones(289, np.float32))):
        assert call(**kw)[0] == 0, kw
    with pytest.raises(native.NnrtError):
        native.check(call(count=0)[0])
