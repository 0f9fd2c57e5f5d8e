"""nnrt_shade_pixels and nnrt_compare_depth_to_raster without a GPU: both are exported and bound, and they refuse bad
arguments on the host before any device work, naming the argument (made-up non-null addresses stand in for arrays the
checks never reach, as in tests/test_depth_filter_abi.py). Empty images are no error."""
import ctypes

import numpy as np
import pytest

FAKE = 0x7f0000000000   # never dereferenced
STEP = 0x10000000       # spacing of the made-up arrays: far more than any of them spans at 48 x 64
FACES, BARY, DIST, TRI, COLORS, NORMALS, OUT, DEPTHS, FRAME = (FAKE + i * STEP for i in range(9))
VERTEX_COLOR, FLAT_EDGE, HEADLIGHT = 0, 1, 2
FLOAT32, UINT16 = 0, 1


@pytest.fixture(scope="module")
def native():
    import os
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


class Record(ctypes.Structure):
    _fields_ = [("both", ctypes.c_int64), ("model_only", ctypes.c_int64), ("frame_only", ctypes.c_int64), ("inliers", ctypes.c_int64),
                ("sum_abs", ctypes.c_double), ("sum_sq", ctypes.c_double), ("max_abs", ctypes.c_float), ("reserved", ctypes.c_int32)]


def test_shade_pixels_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    assert "nnrt_shade_pixels" in native.exported_symbols()
    white = np.ones(3, np.float32)

    def call(mode=VERTEX_COLOR, faces=FACES, bary=BARY, dist=DIST, height=48, width=64, k=1, tri=TRI, face_count=10, colors=COLORS,
             normals=NORMALS, vertex_count=12, color=white, line_width=2.0, ambient=0.1, out=OUT):
        st = lib.nnrt_shade_pixels(mode, ctypes.c_void_p(faces), ctypes.c_void_p(bary), ctypes.c_void_p(dist), height, width, k,
                                   ctypes.c_void_p(tri), face_count, ctypes.c_void_p(colors), ctypes.c_void_p(normals), vertex_count,
                                   native.ptr(color), line_width, ambient, ctypes.c_void_p(out), None)
        return st, lib.nnrt_last_error()

    nan = float("nan")
    cases = [(dict(mode=3), b"mode"), (dict(mode=-1), b"mode"), (dict(height=-1), b"height or width"), (dict(width=-2), b"height or width"),
             (dict(k=0), b"faces_per_pixel"), (dict(k=-3), b"faces_per_pixel"), (dict(face_count=-1), b"face_count"),
             (dict(vertex_count=-1), b"vertex_count"),
             (dict(mode=FLAT_EDGE, line_width=0.0), b"pixel_line_width"), (dict(mode=FLAT_EDGE, line_width=-1.0), b"pixel_line_width"),
             (dict(mode=FLAT_EDGE, line_width=nan), b"pixel_line_width"),
             (dict(mode=HEADLIGHT, ambient=-0.01), b"ambient"), (dict(mode=HEADLIGHT, ambient=1.5), b"ambient"),
             (dict(mode=HEADLIGHT, ambient=nan), b"ambient"),
             (dict(mode=FLAT_EDGE, color=None), b"null h_color"), (dict(mode=HEADLIGHT, color=None), b"null h_color"),
             (dict(colors=None), b"null d_vertex_colors"), (dict(mode=HEADLIGHT, normals=None), b"null d_vertex_normals"),
             (dict(tri=None), b"null d_triangle_indices"), (dict(mode=HEADLIGHT, tri=None), b"null d_triangle_indices"),
             (dict(faces=None), b"null d_pixel_face_indices"), (dict(bary=None), b"null d_pixel_barycentric_coordinates"),
             (dict(mode=HEADLIGHT, bary=None), b"null d_pixel_barycentric_coordinates"),
             (dict(mode=FLAT_EDGE, dist=None), b"null d_pixel_face_distances"), (dict(out=None), b"null d_out_pixels"),
             # the output inside an input: the first and the last byte of each
             (dict(out=FACES), b"d_out_pixels must not overlap"), (dict(out=FACES + 8 * 48 * 64 - 1), b"d_out_pixels must not overlap"),
             (dict(out=BARY + 4), b"d_out_pixels must not overlap"), (dict(mode=FLAT_EDGE, out=DIST), b"d_out_pixels must not overlap"),
             (dict(out=TRI + 8), b"d_out_pixels must not overlap"), (dict(out=COLORS), b"d_out_pixels must not overlap"),
             (dict(mode=HEADLIGHT, out=NORMALS + 12 * 12 - 1), b"d_out_pixels must not overlap"),
             (dict(out=FACES - 3 * 48 * 64 + 1), b"d_out_pixels must not overlap"),
             # value checks come before the empty-image return
             (dict(height=0, mode=7), b"mode"), (dict(width=0, k=0), b"faces_per_pixel"),
             (dict(height=0, mode=FLAT_EDGE, line_width=0.0), b"pixel_line_width"), (dict(width=0, colors=None), b"null d_vertex_colors")]
    for kw, text in cases:
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    # empty images launch nothing; arrays a mode does not read may be null; so may mesh arrays of a mesh without faces or vertices
    for kw in (dict(height=0), dict(width=0), dict(height=0, width=0, faces=None, bary=None, dist=None, out=None),
               dict(height=0, mode=FLAT_EDGE, tri=None, colors=None, normals=None, bary=None),
               dict(width=0, mode=HEADLIGHT, colors=None, dist=None), dict(height=0, color=None, normals=None, dist=None),
               dict(width=0, tri=None, face_count=0, colors=None, vertex_count=0)):
        assert call(**kw)[0] == 0, kw
    with pytest.raises(native.NnrtError, match="mode"):
        native.check(call(mode=9)[0])


def test_compare_depth_to_raster_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()
    assert "nnrt_compare_depth_to_raster" in native.exported_symbols()
    record = Record()

    def call(faces=FACES, depths=DEPTHS, height=48, width=64, k=1, frame=FRAME, dtype=UINT16, scale=1000.0, depth_max=3.0, threshold=0.01,
             out=OUT, statistics=record):
        where = None if statistics is None else ctypes.byref(statistics)
        st = lib.nnrt_compare_depth_to_raster(ctypes.c_void_p(faces), ctypes.c_void_p(depths), height, width, k, ctypes.c_void_p(frame), dtype,
                                              scale, depth_max, threshold, ctypes.c_void_p(out), where, None)
        return st, lib.nnrt_last_error()

    nan, inf = float("nan"), float("inf")
    cases = [(dict(statistics=None), b"null h_out_statistics"), (dict(height=-1), b"height or width"), (dict(width=-1), b"height or width"),
             (dict(k=0), b"faces_per_pixel"), (dict(dtype=2), b"depth_dtype"), (dict(dtype=-1), b"depth_dtype"),
             (dict(scale=0.0), b"depth_scale"), (dict(scale=-1000.0), b"depth_scale"), (dict(scale=nan), b"depth_scale"),
             (dict(scale=inf), b"depth_scale"), (dict(depth_max=nan), b"depth_max"), (dict(threshold=-0.001), b"inlier_threshold"),
             (dict(threshold=nan), b"inlier_threshold"),
             (dict(faces=None), b"null d_pixel_face_indices"), (dict(depths=None), b"null d_pixel_depths"), (dict(frame=None), b"null d_depth"),
             (dict(out=None), b"null d_out_difference"),
             (dict(out=FACES), b"d_out_difference must not overlap"), (dict(out=DEPTHS + 4 * 48 * 64 - 1), b"d_out_difference must not overlap"),
             (dict(out=FRAME), b"d_out_difference must not overlap"), (dict(out=FRAME + 2 * 48 * 64 - 1), b"d_out_difference must not overlap"),
             (dict(dtype=FLOAT32, out=FRAME + 4 * 48 * 64 - 1), b"d_out_difference must not overlap"),
             (dict(k=3, out=FACES + 3 * 8 * 48 * 64 - 1), b"d_out_difference must not overlap"),
             (dict(height=0, scale=0.0), b"depth_scale"), (dict(width=0, dtype=5), b"depth_dtype")]
    for kw, text in cases:
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    # a uint16 frame ends where it ends: one byte past it is no overlap
    assert call(out=FRAME + 2 * 48 * 64, height=0)[0] == 0
    # empty images launch nothing and the statistics are all zero
    for kw in (dict(height=0), dict(width=0, dtype=FLOAT32), dict(height=0, width=0, faces=None, depths=None, frame=None, out=None),
               dict(height=0, depth_max=inf, threshold=0.0)):
        for name, _ in Record._fields_:
            setattr(record, name, 7)
        assert call(**kw)[0] == 0, kw
        assert all(getattr(record, name) == 0 for name, _ in Record._fields_), kw
    with pytest.raises(native.NnrtError, match="depth_scale"):
        native.check(call(scale=0.0)[0])


def test_ndc_extraction_in_a_convention_refuses_an_unknown_one(native):
    lib = native.lib()
    assert "nnrt_get_meshes_ndc_face_vertices_and_clip_mask_in_convention" in native.exported_symbols()
    K = np.array([500.0, 0, 320, 0, 500, 240, 0, 0, 1])
    counts = np.zeros(1, np.int64)
    sets = (ctypes.c_void_p * 1)(None)
    for convention, status in ((0, 0), (1, 0), (2, 1), (-1, 1)):
        st = lib.nnrt_get_meshes_ndc_face_vertices_and_clip_mask_in_convention(sets, sets, native.ptr(counts), 0, native.ptr(K), 480, 640, 0.0,
                                                                               float("inf"), convention, None, None, None)
        assert st == status, convention
        if status:
            assert b"ndc_convention" in lib.nnrt_last_error()
