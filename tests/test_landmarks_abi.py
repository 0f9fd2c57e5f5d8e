"""nnrt_fitter_set_landmarks, nnrt_fitter_get_landmark_distances and nnrt_fitter_landmark_info without a GPU: declared in
the header, exported by the library and bound, and their range and null refusals come before anything touches a device or
the fitter (made-up non-null addresses stand in for device arrays the checks never reach)."""
import ctypes
import os

import numpy as np
import pytest

FAKE = 0x7f0000000000   # never dereferenced
NAMES = ("nnrt_fitter_set_landmarks", "nnrt_fitter_get_landmark_distances", "nnrt_fitter_landmark_info")


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
    from dynamicfuion_python_amd.nnrt import alignment
    for method in ("set_landmarks", "clear_landmarks", "landmark_distances", "landmark_info"):
        assert callable(getattr(alignment.DeformableMeshToImageFitter, method))
    assert callable(alignment.landmarks_from_pixel_matches)


def test_python_surface_carries_the_term(native):
    import dataclasses
    import inspect
    from dynamicfuion_python_amd.alignment.render_based.rendering_alignment_optimizer import RenderingAlignmentOptimizer, RenderingAlignmentParameters
    from dynamicfuion_python_amd.fusion.pipeline import FrameResult, FusionPipeline
    p = RenderingAlignmentParameters()
    assert p.landmark_term_weight == 1.0 and p.landmark_cutoff == 0.0
    assert inspect.signature(RenderingAlignmentOptimizer.optimize_graph).parameters["landmarks"].default is None
    assert inspect.signature(FusionPipeline.__init__).parameters["landmark_provider"].default is None
    fields = {f.name: f.default for f in dataclasses.fields(FrameResult)}
    assert fields["landmark_count"] == 0 and fields["landmark_active_count"] == 0 and fields["landmark_rmse"] == 0.0


def test_set_landmarks_refuses_bad_ranges_before_the_fitter(native):
    lib = native.lib()
    nan, inf = float("nan"), float("inf")

    def call(ft=None, idx=FAKE, targets=FAKE + 0x1000, weights=None, count=3, term_weight=1.0, cutoff=0.0):
        st = lib.nnrt_fitter_set_landmarks(ctypes.c_void_p(ft), ctypes.c_void_p(idx), ctypes.c_void_p(targets), ctypes.c_void_p(weights), count,
                                           term_weight, cutoff, None)
        return st, lib.nnrt_last_error()

    # the ranges are checked with a null fitter and with a stand-in one alike: before anything else
    for ft in (None, FAKE + 0x100000):
        for kw, text in ((dict(count=-1), b"count"), (dict(count=1 << 24), b"count"), (dict(term_weight=0.0), b"term_weight"),
                         (dict(term_weight=-1.0), b"term_weight"), (dict(term_weight=nan), b"term_weight"), (dict(term_weight=inf), b"term_weight"),
                         (dict(cutoff=nan), b"cutoff"), (dict(cutoff=inf), b"cutoff"), (dict(cutoff=-inf), b"cutoff"),
                         (dict(idx=None), b"null d_vertex_indices"), (dict(targets=None), b"null d_vertex_indices or d_targets")):
            st, msg = call(ft=ft, **kw)
            assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    # in range, and then the null fitter is what is refused (a clear too)
    for kw in (dict(), dict(cutoff=-1.0), dict(count=0, idx=None, targets=None)):
        st, msg = call(**kw)
        assert st == 1 and b"null pointer" in msg, (kw, msg)
    with pytest.raises(native.NnrtError):
        native.check(call(term_weight=0.0)[0])


def test_read_backs_refuse_null_arguments(native):
    lib = native.lib()
    out = np.full(8, -1.0, np.float32)
    info = np.full(4, -1, np.int64)
    assert lib.nnrt_fitter_get_landmark_distances(None, native.ptr(out), 2, None) == 1
    assert b"null" in lib.nnrt_last_error()
    assert lib.nnrt_fitter_get_landmark_distances(ctypes.c_void_p(FAKE), None, 2, None) == 1
    assert b"null" in lib.nnrt_last_error()
    assert lib.nnrt_fitter_landmark_info(None, native.ptr(info), 4) == 1
    assert b"null" in lib.nnrt_last_error()
    assert lib.nnrt_fitter_landmark_info(ctypes.c_void_p(FAKE), None, 4) == 1
    assert b"null" in lib.nnrt_last_error()
    for count in (3, 0, -1):   # before the fitter is read
        assert lib.nnrt_fitter_landmark_info(ctypes.c_void_p(FAKE), native.ptr(info), count) == 1
        assert b"out_count" in lib.nnrt_last_error()
    assert (out == -1).all() and (info == -1).all()
