"""GPU tests of the sparse feature tracker (csrc/feature_track.hip) against the numpy restatement of
tests/_feature_track_util.py, whose input sets tests/test_feature_track_cpu.py holds clear of every decision threshold: status
has to be equal without exception. Then the fusion loop with FusionParameters.landmark_tracking on a plate that slides in
its own plane."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _feature_track_util as U   # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ip():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd.nnrt import image_proc
    return image_proc


def _host(x):
    return x.detach().cpu().numpy()


# ---- scores -----------------------------------------------------------------------------------------------------------------
SCORE_SIZES = [(72, 40), (16, 16)]


@pytest.mark.parametrize("r", [1, 3, 7])
def test_scores(ip, r):
    """Images of multiples of 1/256: gradients, products and the float64 sums are exact in any order, so the score differs
    from the restatement's by the final rounding to float at most. 2 r + 3 on a side has exactly one scored pixel."""
    for W, H in SCORE_SIZES + [(2 * r + 3, 2 * r + 3)]:
        img = U.lattice_image(W, H, seed=W + r)
        want = U.corner_scores(img, r)
        got = _host(ip.corner_scores(img, r))
        border = np.ones((H, W), bool)
        border[r + 1:H - r - 1, r + 1:W - r - 1] = False
        assert (got[border] == 0).all() and (want[border] == 0).all()
        scored = int((~border).sum())
        assert scored == max(W - 2 * r - 2, 0) * max(H - 2 * r - 2, 0)
        if (W, H) == (2 * r + 3, 2 * r + 3):
            assert scored == 1
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        bar = 2.0 ** -23 * np.maximum(np.abs(got), np.abs(want)).astype(np.float64)
        print(f"r = {r}, {W} x {H}: {scored} scored pixels, max score {want.max():.4g}, worst error / bar {float((err / np.maximum(bar, 1e-300)).max()):.3g}")
        assert (err <= bar).all()
        if scored:
            assert want.max() > 0
    flat = np.full((40, 72), 0.375, F32)
    assert (_host(ip.corner_scores(flat, r)) == 0).all()
    assert ip.select_features(ip.corner_scores(flat, r), 64).shape == (0, 2)


# ---- selection ----------------------------------------------------------------------------------------------------------------
def _plateau():
    """A score image with a plateau of equal values and equal isolated peaks: ties go to the lower pixel index."""
    s = np.zeros((40, 72), F32)
    s[10:14, 20:26] = 0.5
    s[30, 5] = s[30, 60] = s[5, 60] = 0.75
    s[20, 40] = 0.25
    return s


@pytest.mark.parametrize("m", [0, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_selection(ip, m, masked):
    images = [U.corner_scores(U.lattice_image(W, H, seed=W), 1) for W, H in SCORE_SIZES] + [_plateau()]
    for scores in images:
        H, W = scores.shape
        mask = None
        if masked:
            mask = (np.random.default_rng(3).uniform(size=(H, W)) < 0.6).astype(np.uint8)
        everything = U.select_features(scores, H * W, 0.05, m, mask)
        assert len(everything) >= 1
        for max_count in (1, 64, 65, len(everything) + 7):
            want = U.select_features(scores, max_count, 0.05, m, mask)
            got = ip.select_features(scores, max_count, 0.05, m, mask)
            again = ip.select_features(torch.from_numpy(scores).cuda(), max_count, 0.05, m, None if mask is None else torch.from_numpy(mask).cuda())
            assert got.dtype == torch.float32 and np.array_equal(_host(got), want), (W, H, m, masked, max_count)
            assert torch.equal(got, again)
        print(f"{W} x {H}, m = {m}, {'masked' if masked else 'no mask'}: {len(everything)} candidates")


# ---- the tracker ----------------------------------------------------------------------------------------------------------------
def _gpu_track(ip, data, **extra):
    options = dict(data["options"], **extra)
    fb = options.pop("forward_backward_threshold", None)
    out = ip.track_features(data["pyr_a"], data["pyr_b"], data["points"], data["r"], U.ITERATIONS, forward_backward_threshold=fb, **options)
    return tuple(_host(x) for x in out)


def _compare(label, got, want, points):
    q, status, residual = got
    wq, wstatus, wresidual, _ = want
    assert np.isfinite(q).all() and np.isfinite(residual).all()
    assert np.array_equal(status, wstatus), (label, status.tolist(), wstatus.tolist())
    tracked = status == U.TRACKED
    lost = ~tracked
    assert np.array_equal(q[lost], points[lost])   # a lost feature keeps its input point
    e_pos = float(np.abs(q[tracked] - wq[tracked]).max()) if tracked.any() else 0.0
    e_res = float(np.abs(residual - wresidual).max()) if len(residual) else 0.0
    print(f"{label}: {int(tracked.sum())} of {len(status)} tracked, status counts {np.bincount(status, minlength=6).tolist()}; "
          f"position max |difference| {e_pos:.3g} px (bar 1e-3), residual {e_res:.3g} (bar 1e-5)")
    assert e_pos <= 1e-3 and e_res <= 1e-5
    return e_pos


@pytest.mark.parametrize("case", U.TRACK_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_tracker(ip, case):
    data = U.track_case(*case)
    got = _gpu_track(ip, data)
    _compare(str(case), got, data["want"], data["points"])
    again = _gpu_track(ip, data)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two runs differ"


def test_tracker_no_features(ip):
    data = U.track_case(*U.TRACK_CASES[0])
    q, status, residual = ip.track_features(data["pyr_a"], data["pyr_b"], np.zeros((0, 2), F32), 3, 10, forward_backward_threshold=0.5)
    assert q.shape == (0, 2) and status.shape == (0,) and residual.shape == (0,) and status.dtype == torch.uint8


@pytest.mark.parametrize("name", U.SPECIAL_CASES)
def test_tracker_causes_of_loss(ip, name):
    data = U.special_case(name)
    got = _gpu_track(ip, data)
    _compare(name, got, data["want"], data["points"])
    for row, code in data["expect"].items():
        assert got[1][row] == code
    assert (got[1] == U.TRACKED).any()
    again = _gpu_track(ip, data)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two runs differ"


def test_intensity_pyramid(ip):
    img = U.texture(17, 13)
    got = ip.intensity_pyramid(img, 3)
    want = U.pyramid(img, 3)
    assert [tuple(g.shape) for g in got] == [w.shape for w in want]
    assert all(np.array_equal(_host(g), w) for g, w in zip(got, want))
    with pytest.raises(ValueError):
        ip.intensity_pyramid(img, 5)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
PH, PW, PFX, STEP = 96, 128, 116.0, 0.01   # the camera and slide of tests/test_gpu_landmarks.py::test_pipeline_landmark_provider
PZ = 1.2


def _write_sliding_plate(directory, frames=3):
    """test_pipeline_landmark_provider's plate (z = 1.2 m, |x - k STEP| < 0.35, |y| < 0.25 in frame k) with colour frames whose
    texture is fixed to the plate: plate coordinates (x - k STEP, y) in metres index the analytic texture at PFX / PZ pixels
    per metre, so the pattern moves STEP metres (0.97 px) per frame with the plate. Off the plate the image is black."""
    from PIL import Image
    u, v = np.meshgrid(np.arange(PW, dtype=np.float64), np.arange(PH, dtype=np.float64))
    x, y = (u - PW / 2) * PZ / PFX, (v - PH / 2) * PZ / PFX
    for k in range(frames):
        on = (np.abs(x - k * STEP) < 0.35) & (np.abs(y) < 0.25)
        d = np.where(on, 1200, 0).astype(np.uint16)
        Image.fromarray(d).save(str(directory / f"depth_{k:04d}.png"))
        grey = U._f((x - k * STEP) * PFX / PZ + PW / 2, y * PFX / PZ + PH / 2)
        rgb = np.where(on[..., None], np.clip(np.round(grey * 255.0), 0, 255)[..., None].repeat(3, axis=2), 0).astype(np.uint8)
        Image.fromarray(rgb).save(str(directory / f"rgb_{k:04d}.png"))
    rows = [[PFX, 0, PW / 2, 0], [0, PFX, PH / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    (directory / "camera_intrinsics.txt").write_text("\n".join(" ".join(repr(float(c)) for c in row) for row in rows) + "\n")


def test_pipeline_landmark_tracking(ip, tmp_path):
    """The sliding plate of the landmark term's loop test, followed from its colour frames alone: with
    FusionParameters(landmark_tracking=...) and no provider the mean node translation along the slide is within one pixel's
    footprint (z / fx = 10.3 mm) of 10 and 20 mm after frames 1 and 2; without it the graph does not see the slide."""
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    from dynamicfuion_python_amd.nnrt import alignment as A
    _write_sliding_plate(tmp_path)
    tracking = A.FeatureTracking(max_features=256, quality=0.01, nms_radius=3, window_radius=5, levels=2, max_iterations=10, epsilon=0.0,
                                 min_eigen_threshold=1e-6, max_residual=0.05, forward_backward_threshold=0.5, weight=1.0)

    def run(tracking, **kw):
        seq = dfr.FrameSequenceDataset(base_dataset_type=dfr.DatasetType.CUSTOM, custom_frame_directory=str(tmp_path)).load()
        params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH,
                                    mesh_extraction_weight_thresholding_mode=F.MeshExtractionWeightThresholdingMode.CONSTANT,
                                    mesh_extraction_weight_threshold=0, coupled_data_term=True, landmark_tracking=tracking)
        params.alignment.max_iteration_count = 4
        params.alignment.guard_zero_rotation = True
        params.alignment.penalty_form = A.PenaltyForm.IRLS
        pipe = F.FusionPipeline(seq, params, **kw)
        translations = []
        while seq.has_more_frames():
            pipe.process_frame(seq.get_next_frame())
            translations.append(pipe.active_graph.get_node_translations(True).copy())
        return pipe, translations

    with pytest.raises(ValueError, match="landmark_provider.*landmark_tracking"):
        run(tracking, landmark_provider=lambda *a: None)
    plain, t_plain = run(None)
    assert plain.feature_tracker is None and plain.landmark_provider is None
    for k, r in enumerate(plain.results):
        assert (r.landmark_count, r.tracked_feature_count) == (0, 0)
        assert np.abs(t_plain[k][:, 0]).max() < 1e-7
    pipe, t = run(tracking)
    footprint = PZ / PFX
    assert [r.tracked for r in pipe.results] == [False, True, True] and pipe.results[0].tracked_feature_count == 0
    for k in (1, 2):
        r = pipe.results[k]
        mean_x = float(t[k][:, 0].mean())
        print(f"frame {k}: {r.tracked_feature_count} features selected, {r.landmark_count} landmarks ({r.landmark_active_count} active, rmse "
              f"{r.landmark_rmse:.4g} m); mean node t.x {mean_x:.4g} m (truth {k * STEP:.3g}, bar {footprint:.3g})")
        assert r.tracked_feature_count >= r.landmark_count > 0
        assert abs(mean_x - k * STEP) < footprint
