"""CPU restatement of the rigid frame-to-model alignment (csrc/rigid_align.hip) and an analytic scene for it.

The per-vertex terms are float32 in the kernel's operation order (numpy's element-wise float32 arithmetic rounds every
product, sum and quotient once, like the kernel built with -ffp-contract=off); residual and Jacobian row are widened to
float64, where the product of two floats is exact, and summed exactly (math.fsum: the correctly rounded sum, the same on
every machine); the 6 x 6 solve and the pose update are float64. The GPU's sums differ from these by their rounding
alone, about V * 2^-53 relative.

Every iteration also reports how far the nearest vertex stayed from each decision boundary, so a test can assert that no
decision of the comparison hangs on the last bit."""
import functools
import math

import numpy as np

from dynamicfuion_python_amd import synthetic as S

f32 = np.float32
DEGENERATE = 1


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """exp of the twist xi = (w, v) as a 4 x 4 matrix: R = I + a K + b K^2, t = (I + b K + c K^2) v, K = hat(w); the
    coefficients' series below |w| = 1e-8 (the kernel's formulas)."""
    xi = np.asarray(xi, np.float64)
    w, v = xi[:3], xi[3:]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    if th < 1e-8:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        s, h = math.sin(th), math.sin(0.5 * th)
        a, b, c = s / th, 2.0 * h * h / th2, (th - s) / (th2 * th)
    K = hat(w)
    K2 = K @ K
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * K2
    T[:3, 3] = (np.eye(3) + b * K + c * K2) @ v
    return T


def ordered_normals(points_hw3):
    """k_ordered_point_cloud_normals (csrc/normals.hip) in float32: normalize((right - left) x (top - bottom)), flipped to
    n.z <= 0, zero on the border."""
    p = np.asarray(points_hw3, f32)
    H, W = p.shape[:2]
    out = np.zeros_like(p)
    if H < 3 or W < 3:
        return out
    dh = p[1:-1, 2:] - p[1:-1, :-2]
    dv = p[:-2, 1:-1] - p[2:, 1:-1]
    n = np.stack([dh[..., 1] * dv[..., 2] - dh[..., 2] * dv[..., 1], dh[..., 2] * dv[..., 0] - dh[..., 0] * dv[..., 2],
                  dh[..., 0] * dv[..., 1] - dh[..., 1] * dv[..., 0]], -1).astype(f32)
    n2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(n2)
        n = np.where((n2 > 0)[..., None], n / s[..., None], n).astype(f32)
    n = np.where((n[..., 2] > 0)[..., None], -n, n)
    out[1:-1, 1:-1] = n
    return out


def accumulate(points, normals, target_points, target_normals, fx, fy, cx, cy, T, distance_threshold=0.07, normal_agreement_cos=0.5,
               cull_back_faces=False):
    """One k_rigid_accumulate: (sums [29] float64, kept [V] bool, margins dict). Margins: the smallest distance of any
    vertex that reached a test from that test's boundary -- `round` and `border` in pixels, `tau` and `cos` relative,
    `z` in metres (inf where no vertex reached the test); `per_vertex` is each vertex's own smallest margin."""
    p, n = np.asarray(points, f32), np.asarray(normals, f32)
    tp, tn = np.asarray(target_points, f32), np.asarray(target_normals, f32)
    H, W = tp.shape[:2]
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    R = np.asarray(T, np.float64)[:3, :].astype(f32)
    tau2 = f32(distance_threshold) * f32(distance_threshold)
    c = f32(normal_agreement_cos)
    V = len(p)
    reach = {k: np.full(V, np.inf) for k in ("round", "border", "tau", "cos", "z")}   # per vertex; inf: never reached the test
    with np.errstate(all="ignore"):
        q = np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + R[i, 3] for i in range(3)], -1)
        m = np.stack([(R[i, 0] * n[:, 0] + R[i, 1] * n[:, 1]) + R[i, 2] * n[:, 2] for i in range(3)], -1)
        finite = np.isfinite(q).all(1)
        keep = finite & (q[:, 2] > 0)
        reach["z"][finite] = np.abs(q[finite, 2])
        u = fx * (q[:, 0] / q[:, 2]) + cx
        v = fy * (q[:, 1] / q[:, 2]) + cy
        uf, vf = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        for a, dim in ((u, W), (v, H)):
            a = a.astype(np.float64) + 0.5
            at = keep & np.isfinite(a)
            reach["round"][at] = np.minimum(reach["round"][at], np.abs(a - np.round(a))[at])
            reach["border"][at] = np.minimum(reach["border"][at], np.minimum(np.abs(a), np.abs(a - dim))[at])
        keep &= (uf >= 0) & (uf < f32(W)) & (vf >= 0) & (vf < f32(H))
        ui = np.where(keep, uf, 0).astype(np.int64)
        vi = np.where(keep, vf, 0).astype(np.int64)
        d, g = tp[vi, ui], tn[vi, ui]
        keep &= np.isfinite(d).all(1) & np.isfinite(g).all(1) & (d[:, 2] > 0) & (g != 0).any(1)
        e = q - d
        ee = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        reach["tau"][keep] = (np.abs(ee.astype(np.float64) - float(tau2)) / float(tau2))[keep]
        keep &= ~(ee > tau2)
        mg = np.abs((m[:, 0] * g[:, 0] + m[:, 1] * g[:, 1]) + m[:, 2] * g[:, 2])
        if c > 0:
            at = keep & np.isfinite(mg)
            reach["cos"][at] = (np.abs(mg.astype(np.float64) - float(c)) / float(c))[at]
            keep &= mg >= c
        if cull_back_faces:
            keep &= ~((m[:, 0] * q[:, 0] + m[:, 1] * q[:, 1]) + m[:, 2] * q[:, 2] >= 0)
        r = (g[:, 0] * e[:, 0] + g[:, 1] * e[:, 1]) + g[:, 2] * e[:, 2]
        J = np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2], q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0],
                      g[:, 0], g[:, 1], g[:, 2]], -1)
        keep &= np.isfinite(r) & np.isfinite(J).all(1)
    margins = {k: float(a.min()) if V else np.inf for k, a in reach.items()}
    margins["per_vertex"] = np.minimum.reduce(list(reach.values())) if V else np.zeros(0)
    Jd, rd = J[keep].astype(np.float64), r[keep].astype(np.float64)
    sums = np.zeros(29)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            sums[k] = math.fsum(Jd[:, a] * Jd[:, b])
            k += 1
    for a in range(6):
        sums[21 + a] = math.fsum(Jd[:, a] * rd)
    sums[27] = math.fsum(rd * rd)
    sums[28] = float(keep.sum())
    return sums, keep, margins


def normal_matrix(sums):
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[k]
            k += 1
    return A


def solve_update(sums, T, minimum_correspondence_count=50):
    """k_rigid_solve_update: (T_new, degenerate)."""
    A, x = normal_matrix(sums), -sums[21:27].copy()
    ok = sums[28] >= minimum_correspondence_count
    floor_pivot = 1e-12 * max(0.0, A.diagonal().max())
    L = A.copy()
    for j in range(6):
        if not ok:
            break
        s = L[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (s > floor_pivot) or not (s > 0.0):
            ok = False
            break
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (L[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    if ok:
        for i in range(6):
            x[i] = (x[i] - (L[i, :i] * x[:i]).sum()) / L[i, i]
        for i in range(5, -1, -1):
            x[i] = (x[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
        T_new = se3_exp(x) @ np.asarray(T, np.float64)
        T_new[3] = [0.0, 0.0, 0.0, 1.0]
        ok = bool(np.isfinite(T_new).all())
    return (T_new, False) if ok else (np.array(T, np.float64), True)


def run_level(points, normals, target_points, target_normals, fx, fy, cx, cy, T, iterations, distance_threshold=0.07,
              normal_agreement_cos=0.5, cull_back_faces=False, minimum_correspondence_count=50):
    """nnrt_rigid_align_point_to_plane: (T, log [iterations, 2], status, per-iteration margins, per-iteration cond(A))."""
    T = np.array(T, np.float64)
    log = np.zeros((iterations, 2))
    status, margins, conds = 0, [], []
    if len(points) == 0:
        return T, log, DEGENERATE, margins, conds
    for it in range(iterations):
        sums, _, mg = accumulate(points, normals, target_points, target_normals, fx, fy, cx, cy, T, distance_threshold, normal_agreement_cos,
                                 cull_back_faces)
        log[it] = sums[28], sums[27]
        margins.append(mg)
        A = normal_matrix(sums)
        conds.append(float(np.linalg.cond(A)) if np.isfinite(A).all() and A.any() else np.inf)
        T, degenerate = solve_update(sums, T, minimum_correspondence_count)
        status |= DEGENERATE if degenerate else 0
    return T, log, status, margins, conds


def align(points, normals, target_points, K, T0=None, iteration_counts=(6, 3, 1), distance_threshold=0.07, normal_agreement_cos=0.5,
          cull_back_faces=False, minimum_correspondence_count=50, target_normals=None):
    """nnrt.alignment.align_rigid_point_to_plane: (T, log, status, margins, conds)."""
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    K = np.asarray(K, np.float64)
    tp = np.asarray(target_points, f32)
    logs, status, margins, conds = [], 0, [], []
    for k, iterations in enumerate(iteration_counts):
        level = len(iteration_counts) - 1 - k
        if iterations == 0:
            continue
        s = 1 << level
        tpl = np.ascontiguousarray(tp[::s, ::s])
        tnl = np.asarray(target_normals, f32) if (level == 0 and target_normals is not None) else ordered_normals(tpl)
        T, log, st, mg, cd = run_level(points, normals, tpl, tnl, K[0, 0] / s, K[1, 1] / s, K[0, 2] / s, K[1, 2] / s, T, iterations,
                                       distance_threshold, normal_agreement_cos, cull_back_faces, minimum_correspondence_count)
        logs.append(log)
        status |= st
        margins += mg
        conds += cd
    return T, np.concatenate(logs, 0), status, margins, conds


def margins_exceed(margins, bound=1e-4):
    return all(v > bound for mg in margins for k, v in mg.items() if k != "per_vertex")


# ---------------------------------------------------------------------------------------------------------------------
# the analytic scene
# ---------------------------------------------------------------------------------------------------------------------
def pose(axis, degrees, translation):
    axis = np.asarray(axis, np.float64)
    return se3_exp(np.concatenate([np.radians(degrees) * axis / np.linalg.norm(axis), np.zeros(3)])) + np.block(
        [[np.zeros((3, 3)), np.asarray(translation, np.float64).reshape(3, 1)], [np.zeros((1, 4))]])


def intrinsics(H, W):
    return np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], np.float64)


def live_point_image(H, W, K, z_offset=0.0):
    """The height field z = surface_z(x, y) + z_offset seen from the live camera: per pixel the fixed point of
    z = surface_z(x_ray z, y_ray z) + z_offset in float64 (the surface varies slowly: the map contracts by ~0.3 per
    step), zero where the point leaves X_EXTENT x Y_EXTENT. [H, W, 3] float32."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xr, yr = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    z = np.full((H, W), 1.2 + z_offset)
    for _ in range(50):
        z = S.surface_z(xr * z, yr * z) + z_offset
    x, y = xr * z, yr * z
    inside = (x >= S.X_EXTENT[0]) & (x <= S.X_EXTENT[1]) & (y >= S.Y_EXTENT[0]) & (y <= S.Y_EXTENT[1])
    return np.where(inside[..., None], np.stack([x, y, z], -1), 0.0).astype(f32)


def model(cols, rows, T_gt, z_offset=0.0):
    """synthetic.grid_mesh vertices and normals (camera-facing), moved by T_gt^-1: T_gt maps them onto the live surface."""
    p, n, _ = S.grid_mesh(cols, rows)
    p = p.astype(np.float64)
    p[:, 2] += z_offset
    Ti = np.linalg.inv(T_gt)
    return (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32), (n.astype(np.float64) @ Ti[:3, :3].T).astype(f32)


def pose_errors(T, T_gt):
    """(rotation angle of R R_gt^T in radians, |t - t_gt|)."""
    dR = T[:3, :3] @ T_gt[:3, :3].T
    return float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))


def clear_vertices(points, normals, target_points, target_normals, K, T, bound=1e-4, **kw):
    """Mask of the vertices whose own first-iteration decisions all clear their boundaries by `bound` (any subset of them
    then does as a whole)."""
    _, _, mg = accumulate(points, normals, target_points, target_normals, K[0, 0], K[1, 1], K[0, 2], K[1, 2], T, **kw)
    return mg["per_vertex"] > bound


# the ground-truth motion of the tests: 2 degrees about a skew axis plus (1.515, -1, 2) cm; the 0.015 cm in x moves every
# vertex of the 67 x 45 grid at least 1e-4 pixels off a rounding boundary in the first iteration at 83 x 61
T_GT = pose((1.0, 2.0, -1.5), 2.0, (0.01515, -0.01, 0.02))

# pose_errors of the restatement's full_schedule() result against T_GT, as computed on the CPU
# (tests/test_rigid_align_cpu.py prints them): 1.0608e-06 rad and 3.2135e-06 m from 0.034907 rad and 0.027010 m
GT_ROTATION_ERROR = 1.07e-6
GT_TRANSLATION_ERROR = 3.22e-6


@functools.lru_cache(maxsize=None)
def scene(H, W, cols, rows):
    """(K, live point image, its ordered normals, model points, model normals) of T_GT; computed once, never modified."""
    K = intrinsics(H, W)
    tp = live_point_image(H, W, K)
    p, n = model(cols, rows, T_GT)
    return K, tp, ordered_normals(tp), p, n


@functools.lru_cache(maxsize=None)
def full_schedule():
    """The restatement's (6, 3, 1) schedule at 160 x 120 over the 161 x 121 grid from the identity: (T, log, status)."""
    K, tp, _, p, n = scene(120, 160, 161, 121)
    T, log, status, _, _ = align(p, n, tp, K)
    return T, log, status
