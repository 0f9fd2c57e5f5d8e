"""CPU checks of the rigid frame-to-model alignment: the restatement's exponential map against closed
forms, its convergence on the analytic scene, the Python entry point's argument validation (no device needed) and the
defaults of the fusion loop's new switches."""
import inspect

import numpy as np
import pytest

import _rigid_align_util as U


def _expm_series(xi):
    """exp of the 4 x 4 twist matrix by its power series (|xi| < 1: 30 terms are exact to float64)."""
    M = np.zeros((4, 4))
    M[:3, :3] = U.hat(xi[:3])
    M[:3, 3] = xi[3:]
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 30):
        term = term @ M / k
        out = out + term
    return out


def test_exponential_map_closed_forms():
    v = np.array([0.3, -0.2, 0.5])
    T = U.se3_exp(np.concatenate([np.zeros(3), v]))          # w = 0: a pure translation
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], v)
    w = np.array([3e-10, -4e-10, 0.0])                         # tiny w: the series branch; R = I + K, t = v + w x v / 2 to 1e-19
    T = U.se3_exp(np.concatenate([w, v]))
    assert np.abs(T[:3, :3] - (np.eye(3) + U.hat(w))).max() < 1e-18
    assert np.abs(T[:3, 3] - (v + 0.5 * np.cross(w, v))).max() < 1e-18
    for w in (np.array([0.2, -0.5, 0.3]), np.array([2e-8, 1e-8, -1e-8]), np.array([1e-4, 2e-4, 0.0])):   # generic, and both sides of 1e-8
        T = U.se3_exp(np.concatenate([w, v]))
        assert np.abs(T - _expm_series(np.concatenate([w, v]))).max() < 1e-15
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() < 1e-15
    assert np.array_equal(U.se3_exp(np.zeros(6)), np.eye(4))


def test_restatement_converges_to_the_ground_truth():
    """The (6, 3, 1) schedule at 160 x 120 from the identity: the errors the GPU test's bounds are twice of."""
    T, log, status = U.full_schedule()
    r0, t0 = U.pose_errors(np.eye(4), U.T_GT)
    r, t = U.pose_errors(T, U.T_GT)
    print(f"rotation error {r0:.6g} -> {r:.6g} rad, translation error {t0:.6g} -> {t:.6g} m, last row {log[-1]}")
    assert status == 0 and log.shape == (10, 2)
    assert r < r0 / 5 and t < t0 / 5
    assert r <= U.GT_ROTATION_ERROR and t <= U.GT_TRANSLATION_ERROR   # the figures recorded for the GPU test
    assert log[-1, 0] > 0.9 * 161 * 121 and log[-1, 1] < log[0, 1] / 100


def test_degenerate_systems_keep_the_pose():
    K, tp, tn, p, n = U.scene(61, 83, 67, 45)
    T0 = U.pose((0, 1, 0), 0.5, (0.001, 0, 0))
    for pts, nrm, target in ((p, n, np.zeros_like(tp)), (p, np.full_like(n, np.nan), tp), (p * np.float32([1, 1, -1]), n, tp),
                             (p[:0], n[:0], tp), (p[:3], n[:3], tp)):
        T, log, status, _, _ = U.run_level(pts, nrm, target, U.ordered_normals(target), K[0, 0], K[1, 1], K[0, 2], K[1, 2], T0, 2,
                                           minimum_correspondence_count=1)
        assert status == U.DEGENERATE and np.array_equal(T, T0) and np.isfinite(log).all()


def test_argument_validation_needs_no_device():
    from dynamicfuion_python_amd.nnrt import alignment as A
    K, tp, tn, p, n = U.scene(61, 83, 67, 45)
    good = dict(points=p, normals=n, target_points=tp, intrinsic_matrix=K)
    bad = [("points", dict(points=p.astype(np.float64))), ("points", dict(points=p[:, :2])), ("normals", dict(normals=n[:-1])),
           ("normals", dict(normals=n.reshape(-1))), ("target_points", dict(target_points=tp.reshape(-1, 3))),
           ("target_points", dict(target_points=tp.astype(np.float64))), ("target_normals", dict(target_normals=tn[:-1])),
           ("intrinsic_matrix", dict(intrinsic_matrix=np.eye(4))), ("initial_transformation", dict(initial_transformation=np.eye(3))),
           ("initial_transformation", dict(initial_transformation=np.full((4, 4), np.nan))), ("iteration_counts", dict(iteration_counts=())),
           ("iteration_counts", dict(iteration_counts=(0, 0))), ("iteration_counts", dict(iteration_counts=(2, -1))),
           ("iteration_counts", dict(iteration_counts=(1.5,))), ("distance_threshold", dict(distance_threshold=0.0)),
           ("distance_threshold", dict(distance_threshold=float("inf"))), ("normal_agreement_cos", dict(normal_agreement_cos=float("nan"))),
           ("minimum_correspondence_count", dict(minimum_correspondence_count=-1))]
    for name, change in bad:
        with pytest.raises(ValueError, match=name):
            A.align_rigid_point_to_plane(**{**good, **change})
    assert A.DEGENERATE == U.DEGENERATE == 1
    fields = [f for f in A.RigidAlignmentResult.__dataclass_fields__]
    assert fields == ["transformation", "correspondence_count", "fitness", "inlier_rmse", "status", "log", "levels"]


def test_native_entry_point_refuses_bad_arguments():
    import ctypes
    from dynamicfuion_python_amd import _native as N
    lib = N.lib()
    T, out, log, st = np.eye(4), np.zeros((4, 4)), np.zeros((3, 2)), ctypes.c_int32(7)
    d = ctypes.c_void_p(0x7f0000000000)   # never dereferenced: every call below is refused, or has no vertex

    def call(V=8, H=4, W=4, T=T, iterations=3, tau=0.07, capacity=3, points=d, target=d):
        return lib.nnrt_rigid_align_point_to_plane(points, d, V, target, d, H, W, 4.0, 4.0, 2.0, 2.0, N.ptr(T), iterations, tau, 0.5, 0, 50,
                                                   N.ptr(out), N.ptr(log), capacity, ctypes.byref(st), None)
    for kwargs, message in ((dict(capacity=2), b"log: room for 2 rows"), (dict(points=None), b"points: null"), (dict(target=None), b"target_points"),
                            (dict(H=0), b"target_points"), (dict(iterations=0), b"iterations"), (dict(tau=-1.0), b"distance_threshold"),
                            (dict(V=-1), b"points"), (dict(T=np.full((4, 4), np.inf)), b"T_init")):
        assert call(**kwargs) == 1 and message in lib.nnrt_last_error(), kwargs
    T0 = U.pose((0, 1, 0), 0.5, (0.001, 0, 0))
    assert call(V=0, T=T0, points=None) == 0   # no vertex: an ordinary result, nothing launched
    assert st.value == 1 and np.array_equal(out, T0) and not log.any()


def test_fusion_switch_defaults():
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.alignment.render_based.rendering_alignment_optimizer import RenderingAlignmentOptimizer
    p = F.FusionParameters()
    assert p.rigid_alignment is False and tuple(p.rigid_alignment_iteration_counts) == (6, 3, 1)
    assert p.rigid_alignment_distance_threshold == 0.07 and p.rigid_alignment_normal_agreement_cos == 0.5
    parameters = inspect.signature(RenderingAlignmentOptimizer.optimize_graph).parameters
    assert list(parameters)[-1] == "extrinsics" and parameters["extrinsics"].default is None
    r = F.pipeline.FrameResult(0)
    assert r.rigid_correspondence_count == 0 and r.rigid_inlier_rmse == 0.0 and r.extrinsics is None
