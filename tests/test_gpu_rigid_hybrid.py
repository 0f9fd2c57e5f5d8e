"""The hybrid (geometric + photometric) rigid alignment on the GPU (csrc/rigid_align.hip k_rigid_accumulate<true>,
csrc/photometric.hip) against its CPU restatement (tests/_rigid_hybrid_util.py) on textured analytic scenes,
and its switch in the fusion loop.

Parity tolerances are tests/test_gpu_rigid_align.py's, for the same reason: the float32 terms and their float64 products
are the restatement's exactly, only the order of the float64 sums differs (about V * 2^-53 relative), and the 6 x 6 solve
is well conditioned (asserted). Each one-iteration comparison first asserts on the CPU that no vertex stands within 1e-4
of a decision boundary, the photometric ones (floor, tap border, residual threshold) included."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _rigid_align_util as U  # noqa: E402
import _rigid_hybrid_util as HY  # noqa: E402

DD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepdeform")

# |GPU pose - restatement pose| (largest entry) after the hybrid (6, 3, 1) schedule at 160 x 120, V = 19481, as measured
# once on an MI355X; the test allows 10 x this, capped at 1e-6
FULL_SCHEDULE_MEASURED_DIFFERENCE = 1.11e-16
FULL_SCHEDULE_BOUND = 1e-6 if FULL_SCHEDULE_MEASURED_DIFFERENCE is None else min(10 * FULL_SCHEDULE_MEASURED_DIFFERENCE, 1e-6)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd.nnrt import alignment
    return alignment


@pytest.fixture(scope="module")
def IP(A):
    from dynamicfuion_python_amd.nnrt import image_proc
    return image_proc


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (1, 64), (7, 65), (61, 83)])
def test_intensity_from_rgb8(IP, shape):
    rgb = np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 256, shape + (3,), dtype=np.uint8)
    rgb.reshape(-1, 3)[0] = (255, 255, 255)
    got = IP.intensity_from_rgb8(rgb)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert np.array_equal(got.cpu().numpy(), HY.intensity_from_rgb8(rgb))
    assert np.array_equal(IP.intensity_from_rgb8(torch.from_numpy(rgb)).cpu().numpy(), got.cpu().numpy())


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 3), (3, 3), (5, 8), (61, 83)])
def test_halve_intensity(IP, shape):
    image = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape, dtype=np.float32)
    got = IP.halve_intensity(image)
    assert tuple(got.shape) == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), HY.halve_intensity(image))


def _one_iteration_parity(A, p, n, c, tp, tn, color, K, minimum=50, **kw):
    ti = HY.intensity_from_rgb8(color)
    T_r, log_r, status_r, margins, conds = HY.run_level_hybrid(p, n, c, tp, tn, ti, K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.eye(4), 1,
                                                               minimum_correspondence_count=minimum, **kw)
    assert U.margins_exceed(margins, 1e-4), {k: v for k, v in margins[0].items() if k != "per_vertex"}
    got = A.align_rigid_hybrid(p, n, c, tp, color, K, iteration_counts=(1,), minimum_correspondence_count=minimum, target_normals=tn, **kw)
    print(f"V {len(p)}: counts {got.log[0, [0, 2]]} / {log_r[0, [0, 2]]}, sum r^2 rel "
          f"{abs(got.log[0, 1] - log_r[0, 1]) / max(log_r[0, 1], 1e-300):.3g}, sum rI^2 rel "
          f"{abs(got.log[0, 3] - log_r[0, 3]) / max(log_r[0, 3], 1e-300):.3g}, pose abs {np.abs(got.transformation - T_r).max():.3g}, cond "
          f"{conds[0]:.3g}, status {got.status} / {status_r}")
    assert got.log.shape == (1, 4) and got.log[0, 0] == log_r[0, 0] and got.log[0, 2] == log_r[0, 2]
    assert got.correspondence_count == int(log_r[0, 0]) and got.photometric_count == int(log_r[0, 2])
    assert got.status == status_r
    assert abs(got.log[0, 1] - log_r[0, 1]) <= 1e-9 * log_r[0, 1] and abs(got.log[0, 3] - log_r[0, 3]) <= 1e-9 * log_r[0, 3]
    if status_r == 0:
        assert conds[0] < 1e6
        assert np.abs(got.transformation - T_r).max() <= 1e-9
    else:
        assert np.array_equal(got.transformation, np.eye(4))
    assert np.array_equal(got.transformation[3], [0, 0, 0, 1])
    return got, log_r


def test_one_iteration_parity(A):
    K, tp, tn, color, p, n, c = HY.scene(61, 83, 67, 45)
    assert len(p) == 3015
    got, _ = _one_iteration_parity(A, p, n, c, tp, tn, color, K)
    assert got.status == 0 and got.levels == ((1, 61, 83, 1),)
    assert 2000 < got.photometric_count <= got.correspondence_count
    assert got.photometric_rmse == np.sqrt(got.log[0, 3] / got.photometric_count) and got.inlier_rmse == np.sqrt(got.log[0, 1] / got.correspondence_count)
    # the photometric rows are in the system: the geometric call lands elsewhere
    geometric = A.align_rigid_point_to_plane(p, n, tp, K, iteration_counts=(1,), target_normals=tn)
    assert np.array_equal(geometric.log[0], got.log[0, :2]) and np.abs(geometric.transformation - got.transformation).max() > 1e-6


@pytest.fixture(scope="module")
def dense():
    """A 331 x 241 textured grid over the 83 x 61 image, its vertices that clear every first-iteration boundary by 1e-4, shuffled."""
    K, tp, tn, color, _, _, _ = HY.scene(61, 83, 67, 45)
    p, n = U.model(331, 241, HY.T_GT)
    c = HY.model_colors(331, 241)
    clear = np.flatnonzero(HY.clear_vertices_hybrid(p, n, c, tp, tn, HY.intensity_from_rgb8(color), K, np.eye(4)))
    order = np.random.default_rng(7).permutation(clear)
    return K, tp, tn, color, p[order], n[order], c[order]


@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 257, 256 * 256 + 1])
def test_reduction_tails(A, dense, V):
    """Partial waves, partial workgroups, one workgroup more than a wave, and a second grid-stride round, with 31 sums per
    lane. One vertex gives two rows: a singular system, DEGENERATE by the pivot test. The first five vertices hold four
    correspondences, eight rows: solvable (the restatement says so, cond(A) about 100)."""
    K, tp, tn, color, p, n, c = dense
    got, log_r = _one_iteration_parity(A, p[:V], n[:V], c[:V], tp, tn, color, K, minimum=1)
    assert got.status == (A.DEGENERATE if V < 5 else 0)
    assert log_r[0, 0] > 0.5 * V and log_r[0, 2] > 0.5 * V


def test_threshold_bites(A):
    """A residual threshold between two populated |rI|, at least 1e-3 relative from either: the photometric count drops to
    the restatement's, the geometric count stays."""
    K, tp, tn, color, p, n, c = HY.scene(61, 83, 67, 45)
    ti = HY.intensity_from_rgb8(color)
    _, keep, _ = U.accumulate(p, n, tp, tn, K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.eye(4))
    kept, _, rI, _, _ = HY.photometric_terms(p, c, tp, ti, K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.eye(4), keep)
    magnitudes = np.sort(np.abs(rI[kept]).astype(np.float64))
    k = len(magnitudes) // 2
    while (magnitudes[k + 1] - magnitudes[k]) < 4e-3 * magnitudes[k]:
        k += 1
    threshold = float(np.float32(0.5 * (magnitudes[k] + magnitudes[k + 1])))
    everything, _ = _one_iteration_parity(A, p, n, c, tp, tn, color, K)
    limited, log_r = _one_iteration_parity(A, p, n, c, tp, tn, color, K, photometric_residual_threshold=threshold)
    print(f"threshold {threshold:.6g}: {limited.photometric_count} of {everything.photometric_count} photometric rows")
    assert limited.photometric_count == k + 1 == int(log_r[0, 2]) and 0 < limited.photometric_count < everything.photometric_count
    assert limited.correspondence_count == everything.correspondence_count and limited.log[0, 1] == everything.log[0, 1]
    # a threshold <= 0 is no threshold
    off = A.align_rigid_hybrid(p, n, c, tp, color, K, iteration_counts=(1,), target_normals=tn, photometric_residual_threshold=-1.0)
    assert np.array_equal(off.log, everything.log) and np.array_equal(off.transformation, everything.transformation)


def test_nan_colours_give_the_geometric_result(A):
    K, tp, _, color, p, n, c = HY.scene(61, 83, 67, 45)
    hybrid = A.align_rigid_hybrid(p, n, np.full_like(c, np.nan), tp, color, K, iteration_counts=(2, 2, 1))
    geometric = A.align_rigid_point_to_plane(p, n, tp, K, iteration_counts=(2, 2, 1))
    assert hybrid.status == geometric.status == 0 and hybrid.levels == geometric.levels == ((4, 16, 21, 2), (2, 31, 42, 2), (1, 61, 83, 1))
    assert np.array_equal(hybrid.transformation, geometric.transformation)
    assert hybrid.log.shape == (5, 4) and np.array_equal(hybrid.log[:, :2], geometric.log) and not hybrid.log[:, 2:].any()
    assert hybrid.photometric_count == 0 and hybrid.photometric_rmse == 0.0 and hybrid.correspondence_count == geometric.correspondence_count


def test_tap_validity(A):
    """Rows 28..30 of the target points zeroed (normals and colours kept): a vertex whose own pixel lies in the band loses
    both rows, one whose taps touch the band keeps its geometric row only."""
    K, tp, tn, color, p, n, c = HY.scene(61, 83, 67, 45)
    banded = tp.copy()
    banded[28:31] = 0
    ti = HY.intensity_from_rgb8(color)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    _, keep_full, kept_full, _ = HY.accumulate_hybrid(p, n, c, tp, tn, ti, fx, fy, cx, cy, np.eye(4))
    _, keep, kept, _ = HY.accumulate_hybrid(p, n, c, banded, tn, ti, fx, fy, cx, cy, np.eye(4))
    _, _, _, _, (u, v) = HY.photometric_terms(p, c, banded, ti, fx, fy, cx, cy, np.eye(4), keep)
    own_row, tap_row = np.floor(v + np.float32(0.5)), np.floor(v)
    own_in_band = (own_row >= 28) & (own_row <= 30)
    taps_touch_band = (tap_row + 1 >= 28) & (tap_row <= 30)
    assert np.array_equal(keep, keep_full & ~own_in_band) and np.array_equal(kept, kept_full & ~taps_touch_band)
    assert (keep & taps_touch_band).sum() > 30 and not (kept & taps_touch_band).any()   # geometric rows without a photometric one
    got, log_r = _one_iteration_parity(A, p, n, c, banded, tn, color, K)
    assert got.correspondence_count == keep.sum() < keep_full.sum() and got.photometric_count == kept.sum() < kept_full.sum()
    assert got.correspondence_count - got.photometric_count > (keep_full.sum() - kept_full.sum()) + 30


def test_full_schedule_parity_ground_truth_and_determinism(A):
    K, tp, _, color, p, n, c = HY.scene(120, 160, 161, 121)
    T_r, log_r, status_r = HY.full_schedule()
    got = A.align_rigid_hybrid(p, n, c, tp, color, K)
    difference = np.abs(got.transformation - T_r).max()
    r, t = U.pose_errors(got.transformation, HY.T_GT)
    r0, t0 = U.pose_errors(np.eye(4), HY.T_GT)
    print(f"hybrid full schedule: |GPU - restatement| {difference:.3g}; GPU vs ground truth {r:.6g} rad, {t:.6g} m; counts "
          f"{got.log[:, 0]} / {log_r[:, 0]}, photometric {got.log[:, 2]} / {log_r[:, 2]}")
    assert got.status == status_r == 0 and got.log.shape == (10, 4)
    assert got.levels == ((4, 30, 40, 6), (2, 60, 80, 3), (1, 120, 160, 1))
    assert np.array_equal(got.log[:, 0], log_r[:, 0]) and np.array_equal(got.log[:, 2], log_r[:, 2])
    assert difference <= FULL_SCHEDULE_BOUND
    assert r <= 2 * HY.GT_ROTATION_ERROR and t <= 2 * HY.GT_TRANSLATION_ERROR
    assert r < r0 / 5 and t < t0 / 5
    again = A.align_rigid_hybrid(p, n, c, tp, color, K)
    assert np.array_equal(again.transformation, got.transformation) and np.array_equal(again.log, got.log)


def test_flat_plane(A):
    """A textured plane moved in its own plane: one iteration matches the restatement on the vertices that clear every
    boundary; the full hybrid schedule recovers the motion, the geometric call on the same inputs does not."""
    K, tp, tn, color, p, n, c = HY.plane_scene(61, 83, 67, 45)
    clear = HY.clear_vertices_hybrid(p, n, c, tp, tn, HY.intensity_from_rgb8(color), K, np.eye(4))
    assert clear.sum() > 2900
    got, _ = _one_iteration_parity(A, p[clear], n[clear], c[clear], tp, tn, color, K)
    assert got.status == 0 and got.photometric_count > 2500
    K, tp, _, color, p, n, c = HY.plane_scene(120, 160, 161, 121)
    r0, t0 = HY.in_plane_errors(np.eye(4))
    hybrid = A.align_rigid_hybrid(p, n, c, tp, color, K)
    geometric = A.align_rigid_point_to_plane(p, n, tp, K)
    (r_h, t_h), (r_g, t_g) = HY.in_plane_errors(hybrid.transformation), HY.in_plane_errors(geometric.transformation)
    print(f"plane, from {r0:.6g} rad / {t0:.6g} m: hybrid status {hybrid.status}, {r_h:.6g} rad / {t_h:.6g} m; geometric status "
          f"{geometric.status}, {r_g:.6g} rad / {t_g:.6g} m")
    assert hybrid.status == 0 and r_h < r0 / 5 and t_h < t0 / 5
    assert r_h <= 2 * HY.PLANE_HYBRID_ROTATION_ERROR and t_h <= 2 * HY.PLANE_HYBRID_TRANSLATION_ERROR
    assert not (r_g < r0 / 5 and t_g < t0 / 5)
    assert geometric.status == A.DEGENERATE or t_g > 0.9 * t0


def _run_pair(**fields):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=DD, frame_indices=[300, 600])
    params = F.FusionParameters(rigid_alignment=True, **fields)
    params.alignment.max_iteration_count = 1
    pipe = F.FusionPipeline(seq, params)
    pipe.process_frame(seq.get_next_frame())
    return pipe.process_frame(seq.get_next_frame())


@pytest.fixture(scope="module")
def geometric_pair(A):
    return _run_pair()


def test_fusion_pipeline_with_photometric_weight(A, geometric_pair):
    """The committed seq017 frames 300 -> 600 with the hybrid rigid step."""
    res = _run_pair(rigid_alignment_photometric_weight=0.1)
    E = res.extrinsics
    print(f"seq017 300 -> 600 hybrid: {res.rigid_correspondence_count} correspondences (geometric {geometric_pair.rigid_correspondence_count}), "
          f"RMSE {res.rigid_inlier_rmse:.4g} m (geometric {geometric_pair.rigid_inlier_rmse:.4g} m), {res.rigid_photometric_count} photometric "
          f"rows, intensity RMSE {res.rigid_photometric_rmse:.4g}, extrinsics\n{E}")
    assert res.tracked and res.rigid_photometric_count > 0 and np.isfinite(res.rigid_photometric_rmse) and res.rigid_photometric_rmse > 0
    assert res.rigid_photometric_count <= res.rigid_correspondence_count
    assert np.isfinite(E).all() and np.array_equal(E[3], [0, 0, 0, 1]) and not np.array_equal(E, np.eye(4))   # status 0: the pose was taken
    assert np.abs(E[:3, :3].T @ E[:3, :3] - np.eye(3)).max() < 1e-9
    assert abs(res.rigid_correspondence_count - geometric_pair.rigid_correspondence_count) <= 0.05 * geometric_pair.rigid_correspondence_count
    assert geometric_pair.rigid_photometric_count == 0 and geometric_pair.rigid_photometric_rmse == 0.0
    assert not np.array_equal(E, geometric_pair.extrinsics)


def test_fusion_pipeline_weight_zero_is_the_geometric_loop(A, geometric_pair):
    res = _run_pair(rigid_alignment_photometric_weight=0.0, rigid_alignment_photometric_residual_threshold=0.05)
    assert np.array_equal(res.extrinsics, geometric_pair.extrinsics)
    assert res.rigid_correspondence_count == geometric_pair.rigid_correspondence_count and res.rigid_inlier_rmse == geometric_pair.rigid_inlier_rmse
    assert res.rigid_photometric_count == 0
