"""Rigid frame-to-model alignment on the GPU (csrc/rigid_align.hip) against the CPU restatement
(tests/_rigid_align_util.py) on an analytic scene, and its wiring into the fusion loop.

Parity tolerances: the float32 terms and their float64 products are the restatement's exactly; only the order of the
float64 sums differs (about V * 2^-53 relative), and the 6 x 6 solve is well conditioned on this scene (asserted). Each
one-iteration comparison first asserts on the CPU that no vertex stands within 1e-4 of a decision boundary."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _rigid_align_util as U  # noqa: E402
from _util import FIXTURES, read_ply, transform_mesh  # noqa: E402

DD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepdeform")

# |GPU pose - restatement pose| (largest entry) after the (6, 3, 1) schedule at 160 x 120, V = 19481, as measured once
# on an MI355X; the test allows 10 x this, capped at 1e-6
FULL_SCHEDULE_MEASURED_DIFFERENCE = 3.33e-16
FULL_SCHEDULE_BOUND = 1e-6 if FULL_SCHEDULE_MEASURED_DIFFERENCE is None else min(10 * FULL_SCHEDULE_MEASURED_DIFFERENCE, 1e-6)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd.nnrt import alignment
    return alignment


def _one_iteration_parity(A, p, n, tp, tn, K, minimum=50, **kw):
    T_r, log_r, status_r, margins, conds = U.run_level(p, n, tp, tn, K[0, 0], K[1, 1], K[0, 2], K[1, 2], np.eye(4), 1,
                                                       minimum_correspondence_count=minimum, **kw)
    assert U.margins_exceed(margins, 1e-4), {k: v for k, v in margins[0].items() if k != "per_vertex"}
    got = A.align_rigid_point_to_plane(p, n, tp, K, iteration_counts=(1,), minimum_correspondence_count=minimum, target_normals=tn, **kw)
    print(f"V {len(p)}: count {got.correspondence_count} / {int(log_r[0, 0])}, sum r^2 rel "
          f"{abs(got.log[0, 1] - log_r[0, 1]) / max(log_r[0, 1], 1e-300):.3g}, pose abs {np.abs(got.transformation - T_r).max():.3g}, cond "
          f"{conds[0]:.3g}, status {got.status} / {status_r}")
    assert got.correspondence_count == int(log_r[0, 0]) and got.log.shape == (1, 2) and got.log[0, 0] == log_r[0, 0]
    assert got.status == status_r
    assert abs(got.log[0, 1] - log_r[0, 1]) <= 1e-9 * log_r[0, 1]
    if status_r == 0:
        assert conds[0] < 1e6
        assert np.abs(got.transformation - T_r).max() <= 1e-9
    else:
        assert np.array_equal(got.transformation, np.eye(4))
    assert np.array_equal(got.transformation[3], [0, 0, 0, 1])
    return got, log_r


def test_one_iteration_parity(A):
    K, tp, tn, p, n = U.scene(61, 83, 67, 45)
    assert len(p) == 3015
    got, _ = _one_iteration_parity(A, p, n, tp, tn, K)
    assert got.status == 0 and got.levels == ((1, 61, 83, 1),)
    assert got.fitness == got.correspondence_count / 3015 and got.correspondence_count > 2000
    assert got.inlier_rmse == np.sqrt(got.log[0, 1] / got.correspondence_count)
    # the level's own normals (no target_normals) are the restatement's
    again = A.align_rigid_point_to_plane(p, n, tp, K, iteration_counts=(1,))
    assert np.array_equal(again.transformation, got.transformation) and np.array_equal(again.log, got.log)


@pytest.fixture(scope="module")
def dense():
    """A 331 x 241 grid over the 83 x 61 image, its vertices that clear every first-iteration boundary by 1e-4, shuffled."""
    K, tp, tn, _, _ = U.scene(61, 83, 67, 45)
    p, n = U.model(331, 241, U.T_GT)
    clear = np.flatnonzero(U.clear_vertices(p, n, tp, tn, K, np.eye(4)))
    order = np.random.default_rng(7).permutation(clear)
    return K, tp, tn, p[order], n[order]


@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 257, 256 * 256 + 1])
def test_reduction_tails(A, dense, V):
    """Partial waves, partial workgroups, one workgroup more than a wave, and more vertices than the grid's 256 x 256
    lanes (a second grid-stride round). Fewer than 6 vertices: a singular system, DEGENERATE by the pivot test."""
    K, tp, tn, p, n = dense
    got, log_r = _one_iteration_parity(A, p[:V], n[:V], tp, tn, K, minimum=1)
    assert got.status == (A.DEGENERATE if V < 6 else 0)
    assert log_r[0, 0] > 0.5 * V


def test_full_schedule_parity_ground_truth_and_determinism(A):
    K, tp, _, p, n = U.scene(120, 160, 161, 121)
    T_r, log_r, status_r = U.full_schedule()
    got = A.align_rigid_point_to_plane(p, n, tp, K)
    difference = np.abs(got.transformation - T_r).max()
    r, t = U.pose_errors(got.transformation, U.T_GT)
    r0, t0 = U.pose_errors(np.eye(4), U.T_GT)
    print(f"full schedule: |GPU - restatement| {difference:.3g}; GPU vs ground truth {r:.6g} rad, {t:.6g} m; counts {got.log[:, 0]} / {log_r[:, 0]}")
    assert got.status == status_r == 0 and got.log.shape == (10, 2)
    assert got.levels == ((4, 30, 40, 6), (2, 60, 80, 3), (1, 120, 160, 1))
    assert difference <= FULL_SCHEDULE_BOUND
    # ground truth: twice the restatement's own errors, and below a fifth of the initial ones
    assert r <= 2 * U.GT_ROTATION_ERROR and t <= 2 * U.GT_TRANSLATION_ERROR
    assert r < r0 / 5 and t < t0 / 5
    # determinism: bit-identical
    again = A.align_rigid_point_to_plane(p, n, tp, K)
    assert np.array_equal(again.transformation, got.transformation) and np.array_equal(again.log, got.log)


@pytest.mark.parametrize("case", ["zero_target", "nan_normals", "behind_camera", "no_vertices"])
def test_degenerate_inputs(A, case):
    K, tp, _, p, n = U.scene(61, 83, 67, 45)
    if case == "zero_target":
        tp = np.zeros_like(tp)
    elif case == "nan_normals":
        n = np.full_like(n, np.nan)
    elif case == "behind_camera":
        p = p * np.float32([1, 1, -1])
    else:
        p, n = p[:0], n[:0]
    T0 = U.pose((0, 1, 0), 0.5, (0.001, 0, 0))
    got = A.align_rigid_point_to_plane(p, n, tp, K, initial_transformation=T0)
    assert got.status == A.DEGENERATE and np.array_equal(got.transformation, T0)
    assert got.correspondence_count == 0 and got.fitness == 0.0 and got.inlier_rmse == 0.0
    assert got.log.shape == (10, 2) and np.isfinite(got.log).all() and not got.log.any()


def test_thresholds_bite(A):
    """A second sheet 0.2 m behind the first, front-facing: nothing of it at 0.07 m, all that projects into the image at
    0.5 m. Vertices within 1e-4 of a boundary at either threshold are left out beforehand."""
    K, tp, tn, _, _ = U.scene(61, 83, 67, 45)
    front, back = U.model(41, 31, U.T_GT), U.model(41, 31, U.T_GT, z_offset=0.2)
    p, n = np.concatenate([front[0], back[0]]), np.concatenate([front[1], back[1]])
    clear = U.clear_vertices(p, n, tp, tn, K, np.eye(4)) & U.clear_vertices(p, n, tp, tn, K, np.eye(4), distance_threshold=0.5)
    is_back = (np.arange(len(p)) >= len(front[0]))[clear]
    p, n = p[clear], n[clear]
    assert is_back.sum() > 1000 and (~is_back).sum() > 1000
    narrow, log_n = _one_iteration_parity(A, p, n, tp, tn, K)
    wide, log_w = _one_iteration_parity(A, p, n, tp, tn, K, distance_threshold=0.5)
    only_front, _ = _one_iteration_parity(A, p[~is_back], n[~is_back], tp, tn, K)
    assert narrow.correspondence_count == only_front.correspondence_count   # the sums' order differs with V: not bit-equal
    assert abs(narrow.log[0, 1] - only_front.log[0, 1]) <= 1e-9 * only_front.log[0, 1]
    assert wide.correspondence_count > narrow.correspondence_count + 900
    # the normal-agreement and back-face tests bite too: a model facing away is dropped by culling alone
    flipped = A.align_rigid_point_to_plane(p[~is_back], -n[~is_back], tp, K, iteration_counts=(1,), target_normals=tn)
    assert np.array_equal(flipped.log, only_front.log)   # |m . g|: orientation-agnostic
    culled = A.align_rigid_point_to_plane(p[~is_back], -n[~is_back], tp, K, iteration_counts=(1,), target_normals=tn, cull_back_faces=True)
    assert culled.correspondence_count == 0 and culled.status == A.DEGENERATE
    kept = A.align_rigid_point_to_plane(p[~is_back], n[~is_back], tp, K, iteration_counts=(1,), target_normals=tn, cull_back_faces=True)
    assert np.array_equal(kept.log, only_front.log)
    strict = A.align_rigid_point_to_plane(p[~is_back], n[~is_back], tp, K, iteration_counts=(1,), target_normals=tn, normal_agreement_cos=0.999)
    assert 0 < strict.correspondence_count < only_front.correspondence_count


def test_fusion_pipeline_with_rigid_alignment(A):
    """The committed seq017 frames 300 -> 600 with the switch on: the loop completes, the extrinsics are a rigid motion."""
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=DD, frame_indices=[300, 600])
    params = F.FusionParameters(rigid_alignment=True)
    params.alignment.max_iteration_count = 1
    pipe = F.FusionPipeline(seq, params)
    first = pipe.process_frame(seq.get_next_frame())
    assert first.rigid_correspondence_count == 0 and np.array_equal(first.extrinsics, np.eye(4))
    res = pipe.process_frame(seq.get_next_frame())
    E = res.extrinsics
    print(f"seq017 300 -> 600: {res.rigid_correspondence_count} correspondences, RMSE {res.rigid_inlier_rmse:.4g} m, extrinsics\n{E}")
    assert res.tracked and res.rigid_correspondence_count > 0 and np.isfinite(res.rigid_inlier_rmse)
    assert E.shape == (4, 4) and np.isfinite(E).all() and np.array_equal(E[3], [0, 0, 0, 1])
    assert np.abs(E[:3, :3].T @ E[:3, :3] - np.eye(3)).max() < 1e-9 and np.linalg.det(E[:3, :3]) > 0
    assert E is not pipe.extrinsics and np.array_equal(E, pipe.extrinsics)


def test_optimize_graph_applies_the_extrinsics(oracle_mod):
    """The 25-node plane fixture (cpp/tests/test_deformable_mesh_fitter_advanced.cpp:55-128) seen from a moved camera:
    the mesh is stored in world coordinates (E^-1 of its camera-frame position), the target is the mesh itself. With
    extrinsics=E the fit finds nothing to do: node translations within the one-node plane test's tolerance of zero
    (tests/test_oracle_kats.py, atol 5e-5). Without it the fit sees the mesh displaced."""
    from dynamicfuion_python_amd.alignment.render_based.rendering_alignment_optimizer import (PenaltyFunction, RenderingAlignmentOptimizer,
                                                                                         RenderingAlignmentParameters)
    from dynamicfuion_python_amd.nnrt import geometry as G
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    flip = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 1.2], [0, 0, 0, 1.]])
    P, Nn, Fc = read_ply(os.path.join(FIXTURES, "plane_skin_25_nodes_source.ply"))
    P, Nn = transform_mesh(P, Nn, flip)
    nodes = np.load(os.path.join(FIXTURES, "nodes_25-node_plane.npy")).astype(np.float64)
    nodes = (nodes @ flip[:3, :3].T + flip[:3, 3]).astype(np.float32)
    K = np.array([[100.0, 0, 50], [0, 100.0, 50], [0, 0, 1]])
    fndc, fm = oracle_mod.extract_face_ndc(P, Fc, K, 100, 100, 0.0, 10.0)
    _, dep, _, _ = oracle_mod.rasterize(fndc, fm, 100, 100, 0.0, 1, -1, -1, True, False, True)
    target, _ = oracle_mod.unproject(np.where(dep[..., 0] > 0, dep[..., 0], 0).astype(np.float32), K, 1.0, 10.0)
    E = U.pose((1.0, -2.0, 0.5), 1.0, (0.004, -0.003, 0.01))
    Ei = np.linalg.inv(E)
    world = G.TriangleMesh((P.astype(np.float64) @ Ei[:3, :3].T + Ei[:3, 3]).astype(np.float32),
                           (Nn.astype(np.float64) @ Ei[:3, :3].T).astype(np.float32), Fc)
    params = RenderingAlignmentParameters(data_term_penalty_function=PenaltyFunction.SQUARE,
                                          regularization_term_penalty_function=PenaltyFunction.SQUARE, max_iteration_count=1)
    translations = {}
    for name, extrinsics in (("with", E), ("without", None)):
        wf = G.HierarchicalGraphWarpField(nodes, 0.1, False, 4, 0, G.WarpNodeCoverageComputationMethod.MINIMAL_K_NEIGHBOR_NODE_DISTANCE, 1)
        optimizer = RenderingAlignmentOptimizer((100, 100), None, K, params)
        if extrinsics is None:
            optimizer.optimize_graph(wf, world, target)
        else:
            optimizer.optimize_graph(wf, world, target, extrinsics=extrinsics)
        translations[name] = wf.get_node_translations(True)
        print(f"{name} extrinsics: max |t| {np.abs(translations[name]).max():.3g}")
    assert np.allclose(translations["with"], 0.0, rtol=0.0, atol=5e-5)
    assert np.abs(translations["without"]).max() > 1e-3
