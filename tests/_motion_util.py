"""numpy restatements of csrc/motion.hip, written from the definitions of DESIGN §32: the motion images of a mesh between
two states (float32 for the blends and the kernel's projection order, numpy rounding every float32 product and sum on its
own like the unfused build; float64 for the optical-flow yardstick) and the end-point-error statistics (float64)."""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24   # unit roundoff of float32


def _front(pixel_faces, triangles, vertex_count):
    """Slot-0 face per pixel, which pixels have one, and their faces' vertex indices [H, W, 3] (0 where there is none)."""
    face = np.asarray(pixel_faces)[..., 0]
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    drawn = (face >= 0) & (face < len(triangles))
    corners = np.zeros(face.shape + (3,), np.int64)
    if len(triangles):
        corners[drawn] = triangles[face[drawn]]
    drawn &= ((corners >= 0) & (corners < vertex_count)).all(-1)
    corners[~drawn] = 0
    return drawn, corners


def _blend(b, positions, corners):
    """(b0 P[i0] + b1 P[i1]) + b2 P[i2] in the dtype of b and positions."""
    return (b[..., 0, None] * positions[corners[..., 0]] + b[..., 1, None] * positions[corners[..., 1]]) + b[..., 2, None] * positions[corners[..., 2]]


def _project(p, fx, fy, cx, cy):
    """((fx x) / z + cx, (fy y) / z + cy) in the dtype of p and the intrinsics."""
    return np.stack([(fx * p[..., 0]) / p[..., 2] + cx, (fy * p[..., 1]) / p[..., 2] + cy], -1)


def motion_images(pixel_faces, barycentrics, triangles, source, target, K):
    """dict: source_points, scene_flow [H, W, 3] and optical_flow [H, W, 2] in float32 with the kernel's operation order, mask
    [H, W] bool; optical_flow64, the same quantity with the float32 blends widened and everything after them in float64,
    and optical_flow_scale, M = max(1, |pi(p_s)|, |pi(p_t)|, |cx|, |cy|) per pixel (both 0 / 1 where invalid)."""
    source = np.asarray(source, F32).reshape(-1, 3)
    target = np.asarray(target, F32).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    drawn, corners = _front(pixel_faces, triangles, len(source))
    b = np.asarray(barycentrics, F32)[..., 0, :]
    with np.errstate(all="ignore"):
        ps, pt = _blend(b, source, corners), _blend(b, target, corners)
        valid = drawn & (ps[..., 2] > 0) & (pt[..., 2] > 0)
        f = [F32(K[0, 0]), F32(K[1, 1]), F32(K[0, 2]), F32(K[1, 2])]
        flow32 = _project(pt, *f) - _project(ps, *f)
        wide = [float(v) for v in f]
        us, ut = _project(ps.astype(np.float64), *wide), _project(pt.astype(np.float64), *wide)
        flow64 = ut - us
        scale = np.maximum.reduce([np.ones(valid.shape), np.abs(us).max(-1), np.abs(ut).max(-1), np.full(valid.shape, abs(wide[2])),
                                   np.full(valid.shape, abs(wide[3]))])
    out = {"source_points": np.where(valid[..., None], ps, F32(0)).astype(F32), "scene_flow": np.where(valid[..., None], pt - ps, F32(0)).astype(F32),
           "optical_flow": np.where(valid[..., None], flow32, F32(0)).astype(F32), "mask": valid,
           "optical_flow64": np.where(valid[..., None], flow64, 0.0), "optical_flow_scale": np.where(valid, scale, 1.0)}
    return out


def optical_flow_bound(scale):
    """8 eps M per component: a projection u = ((f x) / z) + c takes three roundings, of f x, of the quotient q
    and of the sum; with u >= 0 and c >= 0 (a point that projects into the image of a camera whose principal point is in it)
    |q| = |u - c| <= max(u, c) <= M, so a projection is off by at most 3 eps M, two by 6 eps M, the subtraction of two
    values in [0, M] adds eps M, and the eighth covers the second-order terms. The tests keep both projections in the image."""
    return 8 * EPS * scale


def flow_error(predicted, predicted_mask, truth, truth_mask, inlier_threshold):
    """(record dict, error image float32): e = sqrt(sum_c d_c^2) in float64 over the float32 differences where both sides are
    valid, NaN elsewhere; the sums are numpy's float64 sums."""
    predicted, truth = np.asarray(predicted, F32), np.asarray(truth, F32)
    drawn = np.asarray(predicted_mask) != 0
    known = np.isfinite(truth).all(-1)
    if truth_mask is not None:
        known &= np.asarray(truth_mask) != 0
    both = drawn & known
    with np.errstate(invalid="ignore", over="ignore"):
        d = (predicted - truth).astype(np.float64)[both]
    squares = np.zeros(len(d))
    for c in range(d.shape[1]):
        squares = squares + d[:, c] * d[:, c]
    e = np.sqrt(squares)
    image = np.full(both.shape, np.nan, F32)
    image[both] = e.astype(F32)
    record = {"both": int(both.sum()), "predicted_only": int((drawn & ~known).sum()), "truth_only": int((known & ~drawn).sum()),
              "inliers": int((e <= float(F32(inlier_threshold))).sum()), "sum_epe": float(e.sum()), "sum_sq": float((e * e).sum()),
              "max_epe": float(e.astype(F32).max()) if len(e) else 0.0}
    return record, image
