"""nnrt_intensity_from_rgb8, nnrt_intensity_halve and nnrt_rigid_align_hybrid without a GPU: declared in the header,
exported by the library and bound, and bad arguments are refused on the host before any device work, naming the
argument (tests/test_depth_filter_abi.py shows the pattern: made-up non-null addresses stand in for device arrays the
checks never reach)."""
import ctypes
import os

import numpy as np
import pytest

FAKE = 0x7f0000000000   # never dereferenced
NAMES = ("nnrt_intensity_from_rgb8", "nnrt_intensity_halve", "nnrt_rigid_align_hybrid")


@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_declared_exported_and_bound(native):
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nnrt_mi355x.h")).read()
    lib = native.lib()
    for name in NAMES:
        assert f"nnrt_status {name}(" in header
        assert name in native.exported_symbols()
        assert getattr(lib, name).restype is ctypes.c_int32
    from dynamicfuion_python_amd.nnrt import alignment, image_proc
    assert callable(alignment.align_rigid_hybrid) and callable(image_proc.intensity_from_rgb8) and callable(image_proc.halve_intensity)


def test_image_entry_points_refuse_bad_arguments_on_the_host(native):
    lib = native.lib()

    def call(fn, d_in=FAKE, height=48, width=64, d_out=FAKE + 0x100000):
        st = fn(ctypes.c_void_p(d_in), height, width, ctypes.c_void_p(d_out), None)
        return st, lib.nnrt_last_error()

    for fn, name in ((lib.nnrt_intensity_from_rgb8, b"d_rgb"), (lib.nnrt_intensity_halve, b"d_in")):
        for kw, text in ((dict(height=-1), b"height or width"), (dict(width=-2), b"height or width"), (dict(d_in=None), b"null " + name),
                         (dict(d_out=None), b"null d_out"), (dict(d_out=FAKE), b"overlap"), (dict(d_out=FAKE + 64), b"overlap"),
                         (dict(d_out=FAKE - 16), b"overlap")):
            st, msg = call(fn, **kw)
            assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (name, kw, st, msg)
        for kw in (dict(height=0), dict(width=0), dict(height=0, width=0, d_in=None, d_out=None)):
            assert call(fn, **kw)[0] == 0, kw
    with pytest.raises(native.NnrtError):
        native.check(call(lib.nnrt_intensity_halve, height=-1)[0])


def test_rigid_align_hybrid_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    T = np.eye(4)
    T_out, log, status = np.zeros((4, 4)), np.zeros((3, 4)), ctypes.c_int32(7)
    nan, inf = float("nan"), float("inf")

    def call(points=FAKE, normals=FAKE + 0x1000, colors=FAKE + 0x2000, V=100, tp=FAKE + 0x3000, tn=FAKE + 0x4000, ti=FAKE + 0x5000, H=48, W=64,
             fx=50.0, T_init=T, iterations=3, tau=0.07, cos=0.5, minimum=50, weight=0.1, threshold=0.0, T_out=T_out, log=log, rows=3,
             status=status):
        st = lib.nnrt_rigid_align_hybrid(ctypes.c_void_p(points), ctypes.c_void_p(normals), ctypes.c_void_p(colors), V, ctypes.c_void_p(tp),
                                         ctypes.c_void_p(tn), ctypes.c_void_p(ti), H, W, fx, 50.0, 32.0, 24.0, native.ptr(T_init), iterations, tau,
                                         cos, 0, minimum, weight, threshold, native.ptr(T_out), native.ptr(log), rows,
                                         ctypes.byref(status) if status is not None else None, None)
        return st, lib.nnrt_last_error()

    bad_T = T.copy()
    bad_T[1, 2] = nan
    for kw, text in ((dict(V=-1), b"points"), (dict(points=None), b"points: null"), (dict(normals=None), b"normals: null"),
                     (dict(colors=None), b"colors: null"), (dict(tp=None), b"target_points: null"), (dict(tn=None), b"target_normals: null"),
                     (dict(ti=None), b"target_intensity: null"), (dict(H=0), b"height and width"), (dict(W=-3), b"height and width"),
                     (dict(fx=nan), b"intrinsics"), (dict(T_init=None), b"T_init"), (dict(T_init=bad_T), b"T_init"),
                     (dict(iterations=0), b"iterations"), (dict(tau=0.0), b"distance_threshold"), (dict(tau=inf), b"distance_threshold"),
                     (dict(cos=nan), b"normal_agreement_cos"), (dict(minimum=-1), b"minimum_correspondence_count"),
                     (dict(weight=0.0), b"photometric_weight"), (dict(weight=-1.0), b"photometric_weight"), (dict(weight=nan), b"photometric_weight"),
                     (dict(weight=inf), b"photometric_weight"), (dict(threshold=nan), b"photometric_residual_threshold"),
                     (dict(T_out=None), b"T_out"), (dict(log=None), b"log: null"), (dict(rows=2), b"log: room for 2 rows"),
                     (dict(status=None), b"status"), (dict(log=T_out), b"overlap"), (dict(log=T, T_init=T), b"overlap")):
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    assert status.value == 7 and not T_out.any() and not log.any()   # a refused call writes nothing
    # no vertices: an ordinary result without a launch (and without a device), whatever the device pointers are
    T0 = T.copy()
    T0[0, 3] = 0.25
    log[:] = 5.0
    for threshold in (0.0, -1.0, 0.05):
        st, _ = call(V=0, points=None, normals=None, colors=None, tp=None, tn=None, ti=None, T_init=T0, threshold=threshold)
        assert st == 0 and status.value == 1 and np.array_equal(T_out, T0) and not log.any()
    with pytest.raises(native.NnrtError):
        native.check(call(weight=0.0)[0])
