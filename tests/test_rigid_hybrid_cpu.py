"""The hybrid rigid alignment without a GPU: the restatement's photometric Jacobian against finite
differences, what the photometric term buys on a plane, its neutrality under NaN colours, and the argument checks of
nnrt.alignment.align_rigid_hybrid that precede any device work."""
import numpy as np
import pytest

import _rigid_align_util as U
import _rigid_hybrid_util as HY


def test_image_kernel_restatements():
    rgb = np.zeros((2, 3, 3), np.uint8)
    rgb[0, 0], rgb[0, 1], rgb[0, 2], rgb[1, 0] = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
    I = HY.intensity_from_rgb8(rgb)
    assert I.dtype == np.float32 and np.allclose(I[0], [0.299, 0.587, 0.114], atol=1e-6) and abs(I[1, 0] - 1.0) < 1e-6 and I[1, 1] == 0
    ramp = np.add.outer(3.0 * np.arange(5), np.arange(8)).astype(np.float32)   # linear: the binomial mean returns the centre inside
    half = HY.halve_intensity(ramp)
    assert half.shape == (3, 4) and np.array_equal(half[1:-1, 1:], ramp[2:-2:2, 2::2])
    corner = ramp[[0, 0, 1]][:, [0, 0, 1]].astype(np.float64)   # indices clamped at the border
    assert half[0, 0] == np.array([0.25, 0.5, 0.25]) @ corner @ np.array([0.25, 0.5, 0.25])
    assert HY.halve_intensity(np.float32([[7.0]])).tolist() == [[7.0]]


def test_photometric_jacobian_against_finite_differences():
    """JI (weight 1) against central differences of a float64 copy of rI(xi) at vertices at least 0.01 pixels off a cell
    boundary. Tolerance: the truncation error h^2 / 6 |f'''| with |f'''| <= 96 D + 192 D^2, D = f rho / z_min (I is
    bilinear inside a cell with |Iu|, |Iv| <= 1 and |Iuv| <= 2 for intensities in [0, 1]; the n-th derivative of a pixel
    coordinate along a unit twist is at most n! 2^n D), the float64 rounding 2^-52 / h of the difference, and 64 float32
    roundings of the largest row entry."""
    K, tp, tn, color, p, n, c = HY.scene(61, 83, 67, 45)
    ti = HY.intensity_from_rgb8(color)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    T = np.eye(4)
    _, keep, _ = U.accumulate(p, n, tp, tn, fx, fy, cx, cy, T)
    kept, JI, rI, reach, _ = HY.photometric_terms(p, c, tp, ti, fx, fy, cx, cy, T, keep, photometric_weight=1.0)
    chosen = np.flatnonzero(kept & (reach["floor"] > 0.01))[::37]
    assert len(chosen) > 50
    h = 1e-6
    q = p[chosen].astype(np.float64)
    D = max(fx, fy) * max(np.linalg.norm(q, axis=1).max(), 1.0) / q[:, 2].min()
    tolerance = h * h / 6 * (96 * D + 192 * D * D) + 2.0 ** -52 / h + 64 * 2.0 ** -24 * np.abs(JI[chosen]).max()
    worst = 0.0
    for i in chosen:
        r0 = HY.photometric_residual_f64(np.zeros(6), p[i], c[i], ti, fx, fy, cx, cy, T)
        assert abs(r0 - rI[i]) < 1e-5
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            d = (HY.photometric_residual_f64(e, p[i], c[i], ti, fx, fy, cx, cy, T) -
                 HY.photometric_residual_f64(-e, p[i], c[i], ti, fx, fy, cx, cy, T)) / (2 * h)
            worst = max(worst, abs(d - float(JI[i, k])))
    print(f"{len(chosen)} vertices: max |JI - central difference| {worst:.3g}, tolerance {tolerance:.3g}, max |JI| {np.abs(JI[chosen]).max():.3g}")
    assert tolerance < 1e-3 * np.abs(JI[chosen]).max()   # the bound means something
    assert worst <= tolerance


def test_plane_needs_the_photometric_term():
    """A textured plane moved in its own plane (1 cm, 1 degree about its normal): point-to-plane sees nothing of it, the
    hybrid schedule recovers it."""
    r0, t0 = HY.in_plane_errors(np.eye(4))
    T_g, _, status_g = HY.plane_schedule(False)
    T_h, log_h, status_h = HY.plane_schedule(True)
    r_g, t_g = HY.in_plane_errors(T_g)
    r_h, t_h = HY.in_plane_errors(T_h)
    print(f"plane, from {r0:.6g} rad / {t0:.6g} m: geometric status {status_g}, {r_g:.6g} rad / {t_g:.6g} m; "
          f"hybrid status {status_h}, {r_h:.6g} rad / {t_h:.6g} m; photometric counts {log_h[:, 2]}")
    assert status_g == U.DEGENERATE or t_g > 0.9 * t0
    assert status_h == 0 and r_h < r0 / 5 and t_h < t0 / 5
    assert r_h <= HY.PLANE_HYBRID_ROTATION_ERROR and t_h <= HY.PLANE_HYBRID_TRANSLATION_ERROR
    assert abs(r_g - HY.PLANE_GEOMETRIC_ROTATION_ERROR) < 1e-3 and abs(t_g - HY.PLANE_GEOMETRIC_TRANSLATION_ERROR) < 1e-3


def test_full_schedule_reaches_the_ground_truth():
    T, log, status = HY.full_schedule()
    r, t = U.pose_errors(T, HY.T_GT)
    r0, t0 = U.pose_errors(np.eye(4), HY.T_GT)
    print(f"hybrid full schedule: {r:.6g} rad, {t:.6g} m from {r0:.6g} rad, {t0:.6g} m; log\n{log}")
    assert status == 0 and log.shape == (10, 4) and (log[:, 2] > 0).all() and (log[:, 2] <= log[:, 0]).all()
    assert r <= HY.GT_ROTATION_ERROR and t <= HY.GT_TRANSLATION_ERROR


def test_nan_colours_leave_the_geometric_alignment():
    K, tp, tn, color, p, n, c = HY.scene(61, 83, 67, 45)
    ti = HY.intensity_from_rgb8(color)
    nan = np.full_like(c, np.nan)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    sums_g, keep_g, _ = U.accumulate(p, n, tp, tn, fx, fy, cx, cy, np.eye(4))
    sums_h, keep_h, kept, _ = HY.accumulate_hybrid(p, n, nan, tp, tn, ti, fx, fy, cx, cy, np.eye(4))
    assert np.array_equal(sums_h[:29], sums_g) and sums_h[29] == 0 and sums_h[30] == 0 and not kept.any() and np.array_equal(keep_h, keep_g)
    T_g, log_g, status_g, _, _ = U.align(p, n, tp, K, iteration_counts=(2, 1))
    T_h, log_h, status_h, _, _ = HY.align_hybrid(p, n, nan, tp, color, K, iteration_counts=(2, 1))
    assert np.array_equal(T_h, T_g) and status_h == status_g and np.array_equal(log_h[:, :2], log_g) and not log_h[:, 2:].any()
    # with colours the sums do change
    sums_c, _, kept_c, _ = HY.accumulate_hybrid(p, n, c, tp, tn, ti, fx, fy, cx, cy, np.eye(4))
    assert kept_c.sum() > 2000 and sums_c[30] == kept_c.sum() and (sums_c[:27] != sums_g[:27]).any() and np.array_equal(sums_c[27:29], sums_g[27:])


def test_align_rigid_hybrid_refuses_bad_arguments_before_any_device_work():
    from dynamicfuion_python_amd.nnrt import alignment as A
    K, tp, _, color, p, n, c = HY.scene(61, 83, 67, 45)
    good = dict(points=p, normals=n, colors=c, target_points=tp, target_color=color, intrinsic_matrix=K)
    for change, text in ((dict(target_color=color[:-1]), "target_color"), (dict(target_color=color[:, :, :2]), "target_color"),
                         (dict(target_color=color.astype(np.float32)), "uint8"), (dict(target_color=color.astype(np.int16)), "uint8"),
                         (dict(photometric_weight=0.0), "photometric_weight"), (dict(photometric_weight=-0.1), "photometric_weight"),
                         (dict(photometric_weight=float("nan")), "photometric_weight"), (dict(photometric_weight=float("inf")), "photometric_weight"),
                         (dict(photometric_residual_threshold=float("nan")), "photometric_residual_threshold"),
                         (dict(colors=c[:-1]), "colors"), (dict(colors=c[:, :2]), "colors"), (dict(colors=c.astype(np.float64)), "colors"),
                         (dict(colors=c.reshape(-1)), "colors"),
                         # the geometric call's own checks hold too
                         (dict(normals=n[:-1]), "normals"), (dict(distance_threshold=0.0), "distance_threshold"),
                         (dict(iteration_counts=()), "iteration_counts")):
        with pytest.raises(ValueError, match=text):
            A.align_rigid_hybrid(**{**good, **change})
    result = A.RigidAlignmentResult(np.eye(4), 0, 0.0, 0.0, 0, np.zeros((1, 2)), ())   # the earlier construction still works
    assert result.photometric_count == 0 and result.photometric_rmse == 0.0
    hybrid = A.HybridRigidAlignmentResult(np.eye(4), 9, 0.5, 0.1, 0, np.zeros((1, 4)), (), photometric_count=7, photometric_rmse=0.02)
    assert isinstance(hybrid, A.RigidAlignmentResult) and hybrid.photometric_count == 7 and hybrid.photometric_rmse == 0.02
    assert [f for f in A.HybridRigidAlignmentResult.__dataclass_fields__][-2:] == ["photometric_count", "photometric_rmse"]
