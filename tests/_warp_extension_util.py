"""numpy restatement of csrc/warp_extension.hip, the checker of its two kernels.

The support ratio is float32 in the kernel's operation order: numpy's element-wise float32 arithmetic rounds every
product, sum, quotient and square root once, like the kernel built with -ffp-contract=off and correctly rounded
division and sqrt, so both outputs are compared bit for bit. The blend selects its nodes by those float32 squared distances
(ties must fall the same way) and is float64 from there on, with the polar factor from an SVD: the kernel's float32 sums,
its exp and its Newton iteration are measured against it."""
import numpy as np

f32 = np.float32
POLAR_MIN_DETERMINANT = 1e-3   # the kernel's "not safely positive"


def squared_distances(points, nodes):
    """[V, N] float32: ((dx*dx + dy*dy) + dz*dz), d = node - point (k_compute_anchors' expression)."""
    p, g = np.asarray(points, f32).reshape(-1, 1, 3), np.asarray(nodes, f32).reshape(1, -1, 3)
    with np.errstate(all="ignore"):
        d = g - p
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def vertex_support(points, nodes, node_coverage=0.05, node_coverage_weights=None):
    """(support_ratio [V] float32, nearest_node [V] int32). Fixed coverage: sqrt(min sq) / c. Variable (squared per-node
    coverages w): sqrt(min (sq * (1 / w))). The first minimum in node order wins; a key that is NaN never does."""
    points = np.asarray(points, f32).reshape(-1, 3)
    V, N = len(points), len(np.asarray(nodes).reshape(-1, 3))
    with np.errstate(all="ignore"):
        key = squared_distances(points, nodes)
        if node_coverage_weights is not None:
            key = key * (f32(1) / np.asarray(node_coverage_weights, f32).reshape(1, -1))
        best, nearest = np.full(V, np.inf, f32), np.full(V, -1, np.int32)
        if N:
            key = np.where(np.isnan(key), f32(np.inf), key)
            at = key.argmin(axis=1)   # the first occurrence: the lowest index
            best = key[np.arange(V), at]
            nearest = np.where(best < np.inf, at, -1).astype(np.int32)
        ratio = np.sqrt(best) if node_coverage_weights is not None else np.sqrt(best) / f32(node_coverage)
    finite = np.isfinite(points).all(axis=1)
    return np.where(finite, ratio, f32(0)).astype(f32), np.where(finite, nearest, -1).astype(np.int32)


def polar_rotation(B):
    """The rotation nearest to B (det B > 0): U V^T of its SVD."""
    U, _, Vt = np.linalg.svd(B)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    return R


def blend_node_transformations(points, nodes, node_rotations, node_translations, anchor_count=4, node_coverage=0.05):
    """(rotations [M, 3, 3], translations [M, 3], fallback_count), float64. Per point: the min(K, N) nearest nodes in
    ascending (float32 squared distance, index) order; w_k = exp(-d_k^2 / (2 c^2)) normalised; translation =
    sum_k w_k ((R_k (p - g_k) - (p - g_k)) + t_k), which is sum_k w_k (g_k + R_k (p - g_k) + t_k) - p for weights that
    sum to one; rotation = the polar factor of sum_k w_k R_k, or the nearest node's rotation where that sum's determinant
    is at most POLAR_MIN_DETERMINANT (counted)."""
    p32 = np.asarray(points, f32).reshape(-1, 3)
    g32 = np.asarray(nodes, f32).reshape(-1, 3)
    p, g = p32.astype(np.float64), g32.astype(np.float64)
    R = np.asarray(node_rotations, f32).reshape(-1, 3, 3).astype(np.float64)
    t = np.asarray(node_translations, f32).reshape(-1, 3).astype(np.float64)
    c = float(f32(node_coverage))
    sq = squared_distances(p32, g32)
    K = min(int(anchor_count), len(g))
    out_R, out_t, fallbacks = np.empty((len(p), 3, 3)), np.empty((len(p), 3)), 0
    for i in range(len(p)):
        slots = np.argsort(sq[i], kind="stable")[:K]
        d = p[i] - g[slots]
        d2 = (d * d).sum(axis=1)
        w = np.exp(-d2 / (2.0 * c * c))
        w = w / w.sum()
        Rd = np.einsum("kab,kb->ka", R[slots], d)
        out_t[i] = (w[:, None] * ((Rd - d) + t[slots])).sum(axis=0)
        B = (w[:, None, None] * R[slots]).sum(axis=0)
        if np.linalg.det(B) > POLAR_MIN_DETERMINANT:
            out_R[i] = polar_rotation(B)
        else:
            out_R[i] = R[slots[0]]
            fallbacks += 1
    return out_R, out_t, fallbacks


def rotations_about(axes, degrees):
    """[N, 3, 3] float64 Rodrigues rotations about `axes` [N, 3] by `degrees` [N]."""
    axes = np.asarray(axes, np.float64)
    axes = axes / np.linalg.norm(axes, axis=1, keepdims=True)
    th = np.radians(np.asarray(degrees, np.float64))
    Kx = np.zeros((len(axes), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -axes[:, 2], axes[:, 1], axes[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -axes[:, 0], -axes[:, 1], axes[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * (Kx @ Kx)


def random_motion(rng, count, max_degrees=60.0, max_translation=0.05):
    """(rotations [count, 3, 3] float32 up to max_degrees, translations [count, 3] float32)."""
    R = rotations_about(rng.normal(size=(count, 3)), rng.uniform(0.0, max_degrees, count))
    return R.astype(f32), rng.uniform(-max_translation, max_translation, (count, 3)).astype(f32)
