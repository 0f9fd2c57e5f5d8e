"""CPU restatement of the hybrid rigid alignment (csrc/rigid_align.hip k_rigid_accumulate<true>, csrc/photometric.hip,
DESIGN §26) on top of tests/_rigid_align_util.py, and textured analytic scenes for it.

As there: the per-vertex terms are float32 in the kernel's operation order, the scaled photometric row and residual are
widened to float64 (exact products) and summed with math.fsum together with the geometric products; solve and pose update
are _rigid_align_util's. Every iteration reports, besides that file's margins, how far the nearest vertex stayed from an
integer pixel coordinate (`floor`), from the tap border (`tap_border`) and from the residual threshold (`photo_threshold`)."""
import functools
import math

import numpy as np

import _rigid_align_util as U
from dynamicfuion_python_amd import synthetic as S

f32 = np.float32
SUMS = 31


# ---------------------------------------------------------------------------------------------------------------------
# the two image kernels
# ---------------------------------------------------------------------------------------------------------------------
def intensity_from_rgb8(rgb):
    """k_intensity_rgb8: ((0.299 R + 0.587 G) + 0.114 B) / 255 in float32."""
    c = np.asarray(rgb, np.uint8).astype(f32)
    return (((f32(0.299) * c[..., 0] + f32(0.587) * c[..., 1]) + f32(0.114) * c[..., 2]) / f32(255.0)).astype(f32)


def halve_intensity(image):
    """k_intensity_halve: 3 x 3 binomial mean centred on (2i, 2j), indices clamped; the three rows first, then the column."""
    a = np.asarray(image, f32)
    H, W = a.shape
    y1, x1 = 2 * np.arange((H + 1) // 2), 2 * np.arange((W + 1) // 2)
    y0, y2 = np.maximum(y1 - 1, 0), np.minimum(y1 + 1, H - 1)
    x0, x2 = np.maximum(x1 - 1, 0), np.minimum(x1 + 1, W - 1)
    h = [((a[y][:, x0] + f32(2.0) * a[y][:, x1]) + a[y][:, x2]) * f32(0.25) for y in (y0, y1, y2)]
    return (((h[0] + f32(2.0) * h[1]) + h[2]) * f32(0.25)).astype(f32)


def intensity_pyramid(rgb, levels):
    """[level 0, ..., level levels - 1], each from the next finer one."""
    out = [intensity_from_rgb8(rgb)]
    for _ in range(levels - 1):
        out.append(halve_intensity(out[-1]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one accumulate launch
# ---------------------------------------------------------------------------------------------------------------------
def photometric_terms(points, colors, target_points, target_intensity, fx, fy, cx, cy, T, keep, photometric_weight=0.1,
                      photometric_residual_threshold=0.0):
    """Steps P1-P6 for the vertices of `keep` (the kept geometric rows): (kept [V] bool, JI [V, 6] float32 scaled, rI [V]
    float32 unscaled, reach dict of per-vertex margins, (u, v) float32)."""
    p, col = np.asarray(points, f32), np.asarray(colors, f32)
    tp, ti = np.asarray(target_points, f32), np.asarray(target_intensity, f32)
    H, W = tp.shape[:2]
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    R = np.asarray(T, np.float64)[:3, :].astype(f32)
    w, thr = f32(photometric_weight), f32(photometric_residual_threshold)
    V = len(p)
    reach = {k: np.full(V, np.inf) for k in ("floor", "tap_border", "photo_threshold")}
    with np.errstate(all="ignore"):
        q = np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + R[i, 3] for i in range(3)], -1)
        u = fx * (q[:, 0] / q[:, 2]) + cx
        v = fy * (q[:, 1] / q[:, 2]) + cy
        # P1
        c = (f32(0.299) * col[:, 0] + f32(0.587) * col[:, 1]) + f32(0.114) * col[:, 2]
        kept = keep & np.isfinite(c)
        # P2
        u0f, v0f = np.floor(u), np.floor(v)
        for a, dim in ((u, W), (v, H)):
            a = a.astype(np.float64)
            reach["floor"][kept] = np.minimum(reach["floor"][kept], np.abs(a - np.round(a))[kept])
            reach["tap_border"][kept] = np.minimum(reach["tap_border"][kept], np.minimum(np.abs(a), np.abs(a - (dim - 1)))[kept])
        kept = kept & (u0f >= 0) & (u0f + f32(1) <= f32(W - 1)) & (v0f >= 0) & (v0f + f32(1) <= f32(H - 1))
        a, b = u - u0f, v - v0f
        u0 = np.where(kept, u0f, 0).astype(np.int64)
        v0 = np.where(kept, v0f, 0).astype(np.int64)
        u1, v1 = np.minimum(u0 + 1, W - 1), np.minimum(v0 + 1, H - 1)   # the clamp acts on dropped vertices only
        # P3
        taps = ((v0, u0), (v0, u1), (v1, u0), (v1, u1))
        for y, x in taps:
            z = tp[y, x, 2]
            kept = kept & np.isfinite(z) & (z > 0)
        I00, I01, I10, I11 = (ti[y, x] for y, x in taps)
        kept = kept & np.isfinite(I00) & np.isfinite(I01) & np.isfinite(I10) & np.isfinite(I11)
        # P4
        top = I00 + a * (I01 - I00)
        bot = I10 + a * (I11 - I10)
        Iuv = top + b * (bot - top)
        Iu = (I01 - I00) + b * ((I11 - I10) - (I01 - I00))
        Iv = bot - top
        # P5
        rI = Iuv - c
        if thr > 0:
            at = kept & np.isfinite(rI)
            reach["photo_threshold"][at] = (np.abs(np.abs(rI.astype(np.float64)) - float(thr)) / float(thr))[at]
            kept = kept & (np.abs(rI) <= thr)
        # P6
        qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
        gx = (Iu * fx) / qz
        gy = (Iv * fy) / qz
        gz = -(((Iu * fx) * qx + (Iv * fy) * qy) / (qz * qz))
        JI = np.stack([w * (qy * gz - qz * gy), w * (qz * gx - qx * gz), w * (qx * gy - qy * gx), w * gx, w * gy, w * gz], -1).astype(f32)
        kept = kept & np.isfinite(w * rI) & np.isfinite(JI).all(1)
    return kept, JI, rI.astype(f32), reach, (u, v)


def _geometric_rows(points, target_points, target_normals, fx, fy, cx, cy, T, keep):
    """Steps 1, 4, 5, 9 of the vertices U.accumulate kept: (J [n, 6], r [n]) float32, in vertex order."""
    p = np.asarray(points, f32)[keep]
    tp, tn = np.asarray(target_points, f32), np.asarray(target_normals, f32)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    R = np.asarray(T, np.float64)[:3, :].astype(f32)
    q = np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + R[i, 3] for i in range(3)], -1)
    u = fx * (q[:, 0] / q[:, 2]) + cx
    v = fy * (q[:, 1] / q[:, 2]) + cy
    ui, vi = np.floor(u + f32(0.5)).astype(np.int64), np.floor(v + f32(0.5)).astype(np.int64)
    d, g = tp[vi, ui], tn[vi, ui]
    e = q - d
    r = (g[:, 0] * e[:, 0] + g[:, 1] * e[:, 1]) + g[:, 2] * e[:, 2]
    J = np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2], q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0],
                  g[:, 0], g[:, 1], g[:, 2]], -1)
    return J.astype(f32), r.astype(f32)


def accumulate_hybrid(points, normals, colors, target_points, target_normals, target_intensity, fx, fy, cx, cy, T, distance_threshold=0.07,
                      normal_agreement_cos=0.5, cull_back_faces=False, photometric_weight=0.1, photometric_residual_threshold=0.0):
    """One k_rigid_accumulate<true>: (sums [31] float64, kept geometric [V] bool, kept photometric [V] bool, margins).
    Sums 0-26 take the geometric and the scaled photometric products, 27 and 28 stay geometric, 29 = sum rI^2 (unscaled),
    30 = the photometric count. Margins: U.accumulate's plus `floor`, `tap_border` (pixels) and `photo_threshold` (relative)."""
    sums_g, keep, margins = U.accumulate(points, normals, target_points, target_normals, fx, fy, cx, cy, T, distance_threshold,
                                         normal_agreement_cos, cull_back_faces)
    kept, JI, rI, reach, _ = photometric_terms(points, colors, target_points, target_intensity, fx, fy, cx, cy, T, keep, photometric_weight,
                                               photometric_residual_threshold)
    V = len(keep)
    for k, a in reach.items():
        margins[k] = float(a.min()) if V else np.inf
    margins["per_vertex"] = np.minimum.reduce([margins["per_vertex"]] + list(reach.values())) if V else np.zeros(0)
    J, r = _geometric_rows(points, target_points, target_normals, fx, fy, cx, cy, T, keep)
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    JId = JI[kept].astype(np.float64)
    rIw = (f32(photometric_weight) * rI[kept]).astype(f32).astype(np.float64)
    rIu = rI[kept].astype(np.float64)
    sums = np.zeros(SUMS)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            sums[k] = math.fsum(np.concatenate([Jd[:, a] * Jd[:, b], JId[:, a] * JId[:, b]]))
            k += 1
    for a in range(6):
        sums[21 + a] = math.fsum(np.concatenate([Jd[:, a] * rd, JId[:, a] * rIw]))
    sums[27] = math.fsum(rd * rd)
    sums[28] = float(keep.sum())
    sums[29] = math.fsum(rIu * rIu)
    sums[30] = float(kept.sum())
    assert sums[27] == sums_g[27] and sums[28] == sums_g[28]
    return sums, keep, kept, margins


def run_level_hybrid(points, normals, colors, target_points, target_normals, target_intensity, fx, fy, cx, cy, T, iterations,
                     distance_threshold=0.07, normal_agreement_cos=0.5, cull_back_faces=False, minimum_correspondence_count=50,
                     photometric_weight=0.1, photometric_residual_threshold=0.0):
    """nnrt_rigid_align_hybrid: (T, log [iterations, 4], status, per-iteration margins, per-iteration cond(A))."""
    T = np.array(T, np.float64)
    log = np.zeros((iterations, 4))
    status, margins, conds = 0, [], []
    if len(points) == 0:
        return T, log, U.DEGENERATE, margins, conds
    for it in range(iterations):
        sums, _, _, mg = accumulate_hybrid(points, normals, colors, target_points, target_normals, target_intensity, fx, fy, cx, cy, T,
                                           distance_threshold, normal_agreement_cos, cull_back_faces, photometric_weight,
                                           photometric_residual_threshold)
        log[it] = sums[28], sums[27], sums[30], sums[29]
        margins.append(mg)
        A = U.normal_matrix(sums)
        conds.append(float(np.linalg.cond(A)) if np.isfinite(A).all() and A.any() else np.inf)
        T, degenerate = U.solve_update(sums, T, minimum_correspondence_count)
        status |= U.DEGENERATE if degenerate else 0
    return T, log, status, margins, conds


def align_hybrid(points, normals, colors, target_points, target_color, K, T0=None, iteration_counts=(6, 3, 1), distance_threshold=0.07,
                 normal_agreement_cos=0.5, cull_back_faces=False, minimum_correspondence_count=50, target_normals=None, photometric_weight=0.1,
                 photometric_residual_threshold=0.0):
    """nnrt.alignment.align_rigid_hybrid: (T, log, status, margins, conds)."""
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    K = np.asarray(K, np.float64)
    tp = np.asarray(target_points, f32)
    pyramid = intensity_pyramid(target_color, len(iteration_counts))
    logs, status, margins, conds = [], 0, [], []
    for k, iterations in enumerate(iteration_counts):
        level = len(iteration_counts) - 1 - k
        if iterations == 0:
            continue
        s = 1 << level
        tpl = np.ascontiguousarray(tp[::s, ::s])
        tnl = np.asarray(target_normals, f32) if (level == 0 and target_normals is not None) else U.ordered_normals(tpl)
        T, log, st, mg, cd = run_level_hybrid(points, normals, colors, tpl, tnl, pyramid[level], K[0, 0] / s, K[1, 1] / s, K[0, 2] / s,
                                              K[1, 2] / s, T, iterations, distance_threshold, normal_agreement_cos, cull_back_faces,
                                              minimum_correspondence_count, photometric_weight, photometric_residual_threshold)
        logs.append(log)
        status |= st
        margins += mg
        conds += cd
    return T, np.concatenate(logs, 0), status, margins, conds


def clear_vertices_hybrid(points, normals, colors, target_points, target_normals, target_intensity, K, T, bound=1e-4, **kw):
    """Mask of the vertices whose own first-iteration decisions, photometric ones included, all clear their boundaries."""
    _, _, _, mg = accumulate_hybrid(points, normals, colors, target_points, target_normals, target_intensity, K[0, 0], K[1, 1], K[0, 2],
                                    K[1, 2], T, **kw)
    return mg["per_vertex"] > bound


# ---------------------------------------------------------------------------------------------------------------------
# a float64 copy of the sampler, for finite differences
# ---------------------------------------------------------------------------------------------------------------------
def photometric_residual_f64(xi, point, color, target_intensity, fx, fy, cx, cy, T):
    """rI of one vertex at the pose exp(xi^) T, in float64 throughout (its own floor; no validity tests)."""
    q = (U.se3_exp(xi) @ np.asarray(T, np.float64))[:3] @ np.append(np.asarray(point, np.float64), 1.0)
    u, v = fx * (q[0] / q[2]) + cx, fy * (q[1] / q[2]) + cy
    u0, v0 = int(math.floor(u)), int(math.floor(v))
    a, b = u - u0, v - v0
    ti = np.asarray(target_intensity, np.float64)
    top = ti[v0, u0] + a * (ti[v0, u0 + 1] - ti[v0, u0])
    bot = ti[v0 + 1, u0] + a * (ti[v0 + 1, u0 + 1] - ti[v0 + 1, u0])
    c = 0.299 * float(color[0]) + 0.587 * float(color[1]) + 0.114 * float(color[2])
    return (top + b * (bot - top)) - c


# ---------------------------------------------------------------------------------------------------------------------
# the textured scenes
# ---------------------------------------------------------------------------------------------------------------------
def texture(x, y):
    """A smooth RGB texture over the canonical surface's (x, y), float64 in [0.2, 0.8]; the three channels differ. The
    shortest period is 0.29 m: 8.7 pixels at the coarsest level the tests use (30 pixels per metre: 160 x 120, stride 4)."""
    r = 0.5 + 0.3 * np.sin(2 * np.pi * x / 0.37 + 0.4) * np.cos(2 * np.pi * y / 0.29)
    g = 0.5 + 0.3 * np.sin(2 * np.pi * (x + y) / 0.41 + 1.1)
    b = 0.5 + 0.3 * np.cos(2 * np.pi * (x - 0.7 * y) / 0.33)
    return np.stack([r, g, b], -1)


def live_color_image(target_points):
    """The texture at every live pixel's surface point (the live camera sees the canonical surface), quantized to uint8;
    zero where the point image holds no point."""
    tp = np.asarray(target_points, np.float64)
    rgb = np.rint(255.0 * texture(tp[..., 0], tp[..., 1]))
    return np.where((tp[..., 2] > 0)[..., None], rgb, 0).astype(np.uint8)


def model_colors(cols, rows):
    """The texture at synthetic.grid_mesh's vertices, [V, 3] float32 (not quantized)."""
    p, _, _ = S.grid_mesh(cols, rows)
    return texture(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)).astype(f32)


# the ground truth of the textured scene: U.T_GT with its translation moved by (0.01, 0.05, 0) cm, which moves every
# vertex of the 67 x 45 grid at least 2e-4 pixels off every rounding, floor and tap boundary in the first iteration at 83 x 61
T_GT = U.T_GT.copy()
T_GT[:3, 3] += (1e-4, 5e-4, 0.0)


@functools.lru_cache(maxsize=None)
def scene(H, W, cols, rows):
    """(K, live point image, its ordered normals, live colour image uint8, model points, normals, colours) of T_GT;
    computed once, never modified."""
    K = U.intrinsics(H, W)
    tp = U.live_point_image(H, W, K)
    p, n = U.model(cols, rows, T_GT)
    return K, tp, U.ordered_normals(tp), live_color_image(tp), p, n, model_colors(cols, rows)


# the flat plane: z = 1.2 over the same extent, normals (0, 0, -1); its ground truth is an in-plane motion, 1 cm along
# (0.8, 0.6, 0) and 1 degree about the plane's normal -- the motion point-to-plane cannot see
PLANE_Z = 1.2
T_GT_PLANE = U.pose((0.0, 0.0, 1.0), 1.0, (0.008, 0.006, 0.0))


def plane_point_image(H, W, K):
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = (u - K[0, 2]) / K[0, 0] * PLANE_Z, (v - K[1, 2]) / K[1, 1] * PLANE_Z
    inside = (x >= S.X_EXTENT[0]) & (x <= S.X_EXTENT[1]) & (y >= S.Y_EXTENT[0]) & (y <= S.Y_EXTENT[1])
    return np.where(inside[..., None], np.stack([x, y, np.full_like(x, PLANE_Z)], -1), 0.0).astype(f32)


@functools.lru_cache(maxsize=None)
def plane_scene(H, W, cols, rows):
    """As scene(), for the flat plane and T_GT_PLANE."""
    K = U.intrinsics(H, W)
    tp = plane_point_image(H, W, K)
    xs, ys = np.linspace(*S.X_EXTENT, cols), np.linspace(*S.Y_EXTENT, rows)
    X, Y = np.meshgrid(xs, ys)
    p = np.stack([X, Y, np.full_like(X, PLANE_Z)], -1).reshape(-1, 3)
    n = np.tile([0.0, 0.0, -1.0], (len(p), 1))
    Ti = np.linalg.inv(T_GT_PLANE)
    return (K, tp, U.ordered_normals(tp), live_color_image(tp), (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32), (n @ Ti[:3, :3].T).astype(f32),
            texture(p[:, 0], p[:, 1]).astype(f32))


def in_plane_errors(T):
    """(rotation error in radians, in-plane translation error in metres) of T against T_GT_PLANE."""
    r, _ = U.pose_errors(T, T_GT_PLANE)
    return r, float(np.linalg.norm((T[:3, 3] - T_GT_PLANE[:3, 3])[:2]))


@functools.lru_cache(maxsize=None)
def full_schedule():
    """The restatement's (6, 3, 1) hybrid schedule at 160 x 120 over the 161 x 121 textured grid from the identity."""
    K, tp, _, color, p, n, c = scene(120, 160, 161, 121)
    T, log, status, _, _ = align_hybrid(p, n, c, tp, color, K)
    return T, log, status


@functools.lru_cache(maxsize=None)
def plane_schedule(hybrid):
    """The (6, 3, 1) schedule on the 160 x 120 plane over its 161 x 121 grid, hybrid or geometric: (T, log, status)."""
    K, tp, _, color, p, n, c = plane_scene(120, 160, 161, 121)
    if hybrid:
        T, log, status, _, _ = align_hybrid(p, n, c, tp, color, K)
    else:
        T, log, status, _, _ = U.align(p, n, tp, K)
    return T, log, status


# pose_errors of full_schedule() against T_GT as computed on the CPU (tests/test_rigid_hybrid_cpu.py prints them):
# 2.8751e-06 rad and 4.1074e-06 m from 0.034907 rad and 0.026885 m
GT_ROTATION_ERROR = 2.88e-6
GT_TRANSLATION_ERROR = 4.11e-6

# in_plane_errors of plane_schedule() as computed on the CPU, from 0.017453 rad and 0.01 m: the hybrid restatement ends at
# 1.9164e-06 rad and 1.0540e-05 m; the geometric one ends DEGENERATE at 0.050288 rad and 0.011398 m (its system is
# singular up to rounding: the steps it does take are noise)
PLANE_HYBRID_ROTATION_ERROR = 1.92e-6
PLANE_HYBRID_TRANSLATION_ERROR = 1.06e-5
PLANE_GEOMETRIC_ROTATION_ERROR = 0.0503
PLANE_GEOMETRIC_TRANSLATION_ERROR = 0.0114
