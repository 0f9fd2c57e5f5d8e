"""The motion images and the flow comparison without a GPU: load_flow_with_mask on DeepDeform's two flow
formats, the stated divergence from the reference's scene-flow mask, nnrt_motion_pixels / nnrt_flow_error and the record's
layout in the library, their refusal of bad arguments on the host before any device work (made-up non-null addresses stand
in for arrays the checks never reach, as in tests/test_shading_abi.py), FlowAgreement's ratios, the restatement on a
hand-written case, and the pipeline's refusal of a flow provider without motion images."""
import ctypes
import math

import numpy as np
import pytest

import _motion_util as MU

F32 = np.float32
FAKE = 0x7f0000000000   # never dereferenced
STEP = 0x10000000       # spacing of the made-up arrays: far more than any of them spans at 48 x 64
FACES, BARY, TRI, SOURCE, TARGET, POINTS, SCENE, OPTICAL, MASK, PREDICTED, PREDICTED_MASK, TRUTH, TRUTH_MASK, ERROR = (
    FAKE + i * STEP for i in range(14))


@pytest.fixture(scope="module")
def native():
    import os
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


# ---- data/io.py ----------------------------------------------------------------------------------------------------------
def flow_file(tmp_path, name, channels, holes):
    """A [C, H, W] flow saved with save_flow; holes: {(v, u): (channel, value)}."""
    from dynamicfuion_python_amd.data import io as dio
    flow = np.random.default_rng(channels).normal(size=(channels, 6, 9)).astype(F32)
    for (v, u), (c, value) in holes.items():
        flow[c, v, u] = value
    path = str(tmp_path / name)
    dio.save_flow(path, flow)
    return path, flow


@pytest.mark.parametrize("name,channels", [("pair.sflow", 3), ("pair.oflow", 2)])
def test_load_flow_with_mask_round_trips_both_formats(tmp_path, name, channels):
    from dynamicfuion_python_amd.data import io as dio
    holes = {(0, 0): (0, np.nan), (2, 3): (1, -np.inf), (5, 8): (channels - 1, np.inf)}
    path, written = flow_file(tmp_path, name, channels, holes)
    flow, mask = dio.load_flow_with_mask(path)
    assert flow.dtype == np.float32 and flow.shape == (6, 9, channels) and flow.flags["C_CONTIGUOUS"] and flow.flags["WRITEABLE"]
    assert mask.dtype == bool and mask.shape == (6, 9)
    want = np.ones((6, 9), bool)
    for pixel in holes:
        want[pixel] = False
    assert np.array_equal(mask, want)
    assert np.array_equal(flow[mask], np.moveaxis(written, 0, -1)[mask])   # the file's values, channel-last
    assert np.all(flow[~mask] == 0) and np.isfinite(flow).all()            # every channel of a masked pixel is zeroed


def test_scene_flow_mask_tests_the_z_channel_unlike_the_reference(tmp_path):
    from dynamicfuion_python_amd.data import io as dio
    pixels = [(1, 1), (4, 7)]
    path, written = flow_file(tmp_path, "z.sflow", 3, {pixel: (2, -np.inf) for pixel in pixels})
    flow, mask = dio.load_flow_with_mask(path)
    finite = np.isfinite(np.moveaxis(written, 0, -1))
    # the reference's call: the third argument of np.logical_and is out=, so z is never tested and those pixels stay valid
    reference = np.logical_and(finite[..., 0], finite[..., 1], finite[..., 2].copy())
    assert all(reference[pixel] for pixel in pixels) and reference.all()
    assert not any(mask[pixel] for pixel in pixels) and mask.sum() == mask.size - len(pixels)
    assert all(np.all(flow[pixel] == 0) for pixel in pixels)


def test_load_flow_with_mask_refuses_what_load_flow_refuses(tmp_path):
    from dynamicfuion_python_amd.data import io as dio
    with pytest.raises(ValueError):
        dio.load_flow_with_mask(str(tmp_path / "x.png"))


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_the_record_has_the_documented_layout(native):
    from dynamicfuion_python_amd.nnrt import rendering
    assert "nnrt_motion_pixels" in native.exported_symbols() and "nnrt_flow_error" in native.exported_symbols()
    lib = native.lib()
    assert lib.nnrt_motion_pixels.restype is ctypes.c_int32 and len(lib.nnrt_motion_pixels.argtypes) == 19
    assert lib.nnrt_flow_error.restype is ctypes.c_int32 and len(lib.nnrt_flow_error.argtypes) == 11
    record = rendering._FlowAgreementRecord
    assert ctypes.sizeof(record) == 56
    offsets = {name: getattr(record, name).offset for name, _ in record._fields_}
    assert offsets == {"both": 0, "predicted_only": 8, "truth_only": 16, "inliers": 24, "sum_epe": 32, "sum_sq": 40, "max_epe": 48, "reserved": 52}
    # the library fills the whole record: an empty image zeroes every field
    filled = record(*([7] * 8))
    assert lib.nnrt_flow_error(None, None, None, None, 0, 5, 3, 0.1, None, ctypes.byref(filled), None) == 0
    assert all(getattr(filled, name) == 0 for name, _ in record._fields_)


def test_motion_pixels_refuses_bad_arguments_on_the_host(native):
    lib = native.lib()

    def call(faces=FACES, bary=BARY, height=48, width=64, k=1, tri=TRI, face_count=10, source=SOURCE, target=TARGET, vertex_count=12,
             fx=500.0, fy=500.0, cx=32.0, cy=24.0, points=POINTS, scene=SCENE, optical=OPTICAL, mask=MASK):
        p = ctypes.c_void_p
        st = lib.nnrt_motion_pixels(p(faces), p(bary), height, width, k, p(tri), face_count, p(source), p(target), vertex_count, fx, fy, cx, cy,
                                    p(points), p(scene), p(optical), p(mask), None)
        return st, lib.nnrt_last_error()

    nan, inf = float("nan"), float("inf")
    cases = [(dict(height=-1), b"height or width"), (dict(width=-2), b"height or width"), (dict(k=0), b"faces_per_pixel"),
             (dict(k=-1), b"faces_per_pixel"), (dict(face_count=-1), b"face_count"), (dict(vertex_count=-1), b"vertex_count"),
             (dict(fx=nan), b"fx, fy, cx and cy"), (dict(fy=inf), b"fx, fy, cx and cy"), (dict(cx=-inf), b"fx, fy, cx and cy"),
             (dict(cy=nan), b"fx, fy, cx and cy"),
             (dict(tri=None), b"null d_triangle_indices"), (dict(source=None), b"null d_source_positions"),
             (dict(target=None), b"null d_target_positions"), (dict(faces=None), b"null d_pixel_face_indices"),
             (dict(bary=None), b"null d_pixel_barycentric_coordinates"), (dict(points=None), b"null d_out_source_points"),
             (dict(scene=None), b"null d_out_scene_flow"), (dict(optical=None), b"null d_out_optical_flow"), (dict(mask=None), b"null d_out_mask"),
             # an output inside an input: the first and the last byte
             (dict(points=FACES), b"must not overlap an input"), (dict(mask=FACES + 8 * 48 * 64 - 1), b"must not overlap an input"),
             (dict(scene=BARY + 4), b"must not overlap an input"), (dict(optical=TRI + 8), b"must not overlap an input"),
             (dict(mask=SOURCE + 12 * 12 - 1), b"must not overlap an input"), (dict(points=TARGET), b"must not overlap an input"),
             (dict(k=2, mask=FACES + 2 * 8 * 48 * 64 - 1), b"must not overlap an input"),
             # an output inside another
             (dict(scene=POINTS), b"must not overlap each other"), (dict(mask=OPTICAL + 8 * 48 * 64 - 1), b"must not overlap each other"),
             (dict(optical=SCENE + 12 * 48 * 64 - 4), b"must not overlap each other"),
             # value checks come before the empty-image return
             (dict(height=0, k=0), b"faces_per_pixel"), (dict(width=0, fx=nan), b"fx, fy, cx and cy"), (dict(height=0, tri=None), b"null d_triangle_indices")]
    for kw, text in cases:
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    # an array ends where it ends: one byte past it is no overlap (checked on an empty image, which launches nothing)
    for kw in (dict(height=0), dict(width=0), dict(height=0, width=0, faces=None, bary=None, points=None, scene=None, optical=None, mask=None),
               dict(height=0, tri=None, face_count=0, source=None, target=None, vertex_count=0)):
        assert call(**kw)[0] == 0, kw
    with pytest.raises(native.NnrtError, match="faces_per_pixel"):
        native.check(call(k=0)[0])


def test_flow_error_refuses_bad_arguments_on_the_host(native):
    from dynamicfuion_python_amd.nnrt import rendering
    lib = native.lib()
    record = rendering._FlowAgreementRecord()

    def call(predicted=PREDICTED, predicted_mask=PREDICTED_MASK, truth=TRUTH, truth_mask=TRUTH_MASK, height=48, width=64, channels=3,
             threshold=0.01, out=ERROR, statistics=record):
        p = ctypes.c_void_p
        where = None if statistics is None else ctypes.byref(statistics)
        st = lib.nnrt_flow_error(p(predicted), p(predicted_mask), p(truth), p(truth_mask), height, width, channels, threshold, p(out), where, None)
        return st, lib.nnrt_last_error()

    nan = float("nan")
    cases = [(dict(statistics=None), b"null h_out_statistics"), (dict(height=-1), b"height or width"), (dict(width=-1), b"height or width"),
             (dict(channels=1), b"channels"), (dict(channels=4), b"channels"), (dict(channels=0), b"channels"),
             (dict(threshold=-0.001), b"inlier_threshold"), (dict(threshold=nan), b"inlier_threshold"),
             (dict(predicted=None), b"null d_predicted"), (dict(predicted_mask=None), b"null d_predicted_mask"), (dict(truth=None), b"null d_truth"),
             (dict(out=None), b"null d_out_error"),
             (dict(out=PREDICTED), b"d_out_error must not overlap"), (dict(out=PREDICTED + 12 * 48 * 64 - 1), b"d_out_error must not overlap"),
             (dict(out=TRUTH + 4), b"d_out_error must not overlap"), (dict(out=PREDICTED_MASK + 48 * 64 - 1), b"d_out_error must not overlap"),
             (dict(out=TRUTH_MASK), b"d_out_error must not overlap"),
             (dict(height=0, channels=5), b"channels"), (dict(width=0, threshold=-1.0), b"inlier_threshold")]
    for kw, text in cases:
        st, msg = call(**kw)
        assert st == 1 and msg.startswith(b"invalid argument") and text in msg, (kw, st, msg)
    # a two-channel image ends where it ends: one byte past it is no overlap with C = 2 (an empty image launches nothing)
    for kw in (dict(height=0), dict(width=0, channels=2), dict(height=0, truth_mask=None),
               dict(height=0, width=0, predicted=None, predicted_mask=None, truth=None, truth_mask=None, out=None), dict(height=0, threshold=0.0)):
        for name, _ in record._fields_:
            setattr(record, name, 7)
        assert call(**kw)[0] == 0, kw
        assert all(getattr(record, name) == 0 for name, _ in record._fields_), kw
    with pytest.raises(native.NnrtError, match="channels"):
        native.check(call(channels=1)[0])


# ---- Python ------------------------------------------------------------------------------------------------------------
def test_flow_agreement_ratios_on_a_hand_written_case():
    from dynamicfuion_python_amd.nnrt.rendering import FlowAgreement
    a = FlowAgreement(both=4, predicted_only=2, truth_only=1, inliers=3, sum_epe=2.0, sum_sq=1.5, max_epe=1.0)
    assert a.mean_epe == 0.5 and a.rmse == math.sqrt(1.5 / 4) and a.inlier_ratio == 0.75
    empty = FlowAgreement()
    assert (empty.mean_epe, empty.rmse, empty.inlier_ratio) == (0.0, 0.0, 0.0)


def test_the_restatement_on_a_hand_written_case():
    """One triangle that moves 0.5 m along z: known points, flows and errors."""
    faces = np.array([[[0], [-1]]], np.int64)                 # 1 x 2 pixels, the second background
    bary = np.array([[[[0.5, 0.25, 0.25]], [[0.0, 0.0, 0.0]]]], F32)
    source = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], F32)
    target = source + F32([0.0, 0.0, 1.0])
    K = np.array([[100.0, 0.0, 8.0], [0.0, 100.0, 4.0], [0.0, 0.0, 1.0]])
    m = MU.motion_images(faces, bary, np.array([[0, 1, 2]]), source, target, K)
    assert np.array_equal(m["mask"], [[True, False]])
    assert np.array_equal(m["source_points"][0], np.array([[0.25, 0.25, 1.0], [0, 0, 0]], F32))
    assert np.array_equal(m["scene_flow"][0], np.array([[0, 0, 1.0], [0, 0, 0]], F32))
    assert np.array_equal(m["optical_flow"][0], np.array([[-12.5, -12.5], [0, 0]], F32))   # (33, 29) -> (20.5, 16.5)
    assert np.array_equal(m["optical_flow64"][0, 0], [-12.5, -12.5]) and m["optical_flow_scale"][0, 0] == 33.0
    behind = MU.motion_images(faces, bary, np.array([[0, 1, 2]]), source, source - F32([0, 0, 1.0]), K)   # the target at z = 0
    assert not behind["mask"].any() and not behind["scene_flow"].any() and not behind["source_points"].any()
    truth = np.array([[[0.0, 0.0, 1.0], [3.0, 4.0, 0.0]], [[0.0, 3.0, 5.0], [np.nan, 0.0, 0.0]]], F32)
    predicted = np.array([[[3.0, 4.0, 1.0], [0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]], F32)
    record, image = MU.flow_error(predicted, [[1, 0], [1, 1]], truth, None, 5.0)
    assert record == {"both": 2, "predicted_only": 1, "truth_only": 1, "inliers": 2, "sum_epe": 10.0, "sum_sq": 50.0, "max_epe": 5.0}
    assert np.array_equal(np.isnan(image), [[False, True], [False, True]]) and image[0, 0] == 5.0 and image[1, 0] == 5.0
    masked, _ = MU.flow_error(predicted, [[1, 0], [1, 1]], truth, [[0, 1], [1, 1]], 4.0)
    assert (masked["both"], masked["predicted_only"], masked["truth_only"], masked["inliers"]) == (1, 2, 1, 0)


def test_a_flow_provider_needs_motion_images():
    from dynamicfuion_python_amd import fusion as F
    assert F.FusionParameters().motion_images is False
    with pytest.raises(ValueError, match="motion_images"):
        F.FusionPipeline(None, F.FusionParameters(motion_images=False), flow_truth_provider=lambda pipeline, frame: None)
    with pytest.raises(ValueError, match="motion_images"):
        F.FusionPipeline(None, flow_truth_provider=lambda pipeline, frame: None)
    result = F.FrameResult(0)
    for name in ("motion_pixel_count", "scene_flow_count", "scene_flow_epe_mean", "scene_flow_rmse", "optical_flow_count",
                 "optical_flow_epe_mean", "optical_flow_rmse"):
        assert getattr(result, name) == 0, name
