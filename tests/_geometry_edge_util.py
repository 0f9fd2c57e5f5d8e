"""Inputs and float64 references for the edge tests of csrc/geometry.hip's anchor search (k_compute_anchors<K>) and mesh
warp (launch_warp_mesh's three kernels). Plain numpy: nothing here touches a device.

The case lists below are shared by tests/test_geometry_edges_cpu.py (the oracle against float64 on these inputs) and
tests/test_gpu_geometry_edges.py (the kernels against the oracle, bit for bit), so both files see exactly the same inputs.

k_compute_anchors loads the nodes in batches of 64 (one batch ahead), walks full = N - N % 64 of them in groups of 8,
skips a group that no lane can use, and handles the last N % 64 nodes in a scalar tail: N = 64, 128, 192 have no tail,
N = 64 has one batch (no prefetch), N < 64 only the tail, N < K leaves slots empty (index -1, squared distance inf)."""
import numpy as np

from dynamicfuion_python_amd import synthetic

f32 = np.float32

LAYOUTS = ("uniform", "near_first", "near_last", "lattice", "duplicates")
# node coverage per layout: weights stay normal float32 numbers for every slot the K-NN keeps (lattice spacing is 1)
COVERAGE = {"uniform": 0.3, "near_first": 0.3, "near_last": 0.3, "lattice": 1.0, "duplicates": 0.3}

BATCH_N = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 192)   # V = 65, uniform, every K in ALL_K
ALL_K = (1, 2, 3, 4, 5, 6, 7, 8)
BATCH_V = 65
TAIL_V = (1, 63, 64, 65, 130)                            # N in TAIL_N, K = 4
TAIL_N = (64, 129)
SKIP_LAYOUTS = ("near_first", "near_last")               # N in SKIP_N, K in SKIP_K
SKIP_N = (128, 129)
SKIP_K = (1, 4, 8)
TIE_LAYOUTS = ("lattice", "duplicates")                  # N in TIE_N, K in TIE_K
TIE_N = (64, 128)
TIE_K = (1, 2, 4, 8)
FEW_N = (0, 1, 3)                                        # N < K, K in FEW_K
FEW_K = (4, 8)
THRESHOLD_N = 129
THRESHOLD_V = 130
# K -> coverage at which, over uniform points and nodes in (-1, 1)^3, some points keep 0, some 1..K-1 and some K slots
THRESHOLD_COVERAGE = {2: 0.12, 5: 0.17, 8: 0.2}
WARP_V = (1, 63, 65, 257, 1025)
WARP_N = 65
WARP_QUAD_K = (1, 2, 3, 4)     # k_warp_mesh_quad, or k_warp_mesh_vertex under NNRT_WARP_VERTEX=1
WARP_WIDE_K = (5, 6, 8)        # k_warp_mesh
WARP_INVALID = (0.0, 0.3)


def _seed(*parts):
    return int(np.random.SeedSequence([int(p) for p in parts]).generate_state(1)[0])


def anchor_case(N, V, seed, layout):
    """(points [V, 3], nodes [N, 3]) float32.
    uniform: both uniform in (-1, 1)^3.
    near_first / near_last: points uniform in (-0.1, 0.1)^3 (one tight cloud), nodes uniform in (-1, 1)^3 sorted by
        ascending / descending distance to the points' centroid. Ascending: the nearest nodes come first and the later
        groups of 8 are skipped by the __any test; descending: every node is nearer than those before, every group inserts.
    lattice: nodes on the 8 x 8 x 2 integer lattice (x fastest, z slowest: the first 64 are the layer z = 0), points at
        lattice cells' centres (cell + 0.5). Every squared distance is a multiple of 0.25 below 128, exact in float32, and
        each point has 8 (N = 128) or 4 (N = 64) nearest nodes at 0.75.
    duplicates: N / 2 nodes on the grid of multiples of 1/16 in [-1, 1), each appearing twice at seeded places; points at
        odd multiples of 1/32. Squared distances are multiples of 1/1024 below 12: exact in float32, a node and its copy tie."""
    rng = np.random.default_rng(_seed(seed, N, V, LAYOUTS.index(layout)))
    if layout == "uniform":
        points = rng.uniform(-1, 1, (V, 3))
        nodes = rng.uniform(-1, 1, (N, 3))
    elif layout in ("near_first", "near_last"):
        points = rng.uniform(-0.1, 0.1, (V, 3)).astype(f32)
        nodes = rng.uniform(-1, 1, (N, 3)).astype(f32)
        d = np.linalg.norm(nodes.astype(np.float64) - points.astype(np.float64).mean(axis=0), axis=1)
        order = np.argsort(d, kind="stable")
        nodes = nodes[order if layout == "near_first" else order[::-1]]
    elif layout == "lattice":
        if not 0 <= N <= 128:
            raise ValueError("the lattice has 128 nodes")
        z, y, x = np.meshgrid(np.arange(2), np.arange(8), np.arange(8), indexing="ij")
        nodes = np.stack([x, y, z], -1).reshape(-1, 3)[:N]
        points = np.stack([rng.integers(0, 7, V), rng.integers(0, 7, V), np.zeros(V, np.int64)], 1) + 0.5
    elif layout == "duplicates":
        if N % 2:
            raise ValueError("every node appears twice: N must be even")
        half = rng.integers(-16, 16, (N // 2, 3)) / 16.0
        nodes = np.concatenate([half, half])[rng.permutation(N)]
        points = (2 * rng.integers(-16, 16, (V, 3)) + 1) / 32.0
    else:
        raise ValueError(layout)
    return np.ascontiguousarray(points, f32).reshape(V, 3), np.ascontiguousarray(nodes, f32).reshape(N, 3)


def non_finite_cloud(seed=0):
    """(points [65, 3], nodes [129, 3], bad rows): the uniform case with a NaN coordinate in row 3 and +inf in row 40,
    ordinary points around them in the same wave."""
    points, nodes = anchor_case(129, 65, seed, "uniform")
    points = points.copy()
    points[3, 1] = np.nan
    points[40, 0] = np.inf
    return points, nodes, (3, 40)


def warp_extrinsics():
    """The rigid transform tests/test_gpu_parity.py::test_warp_bit_exact uses."""
    E = np.eye(4)
    E[:3, :3] = synthetic.rodrigues_np(np.array([[0.01, -0.02, 0.03]], f32))[0]
    E[:3, 3] = [0.01, -0.005, 0.02]
    return E


def warp_case(V, N, K, seed, invalid_share):
    """(points [V, 3], unit normals [V, 3], nodes [N, 3], rotations [N, 3, 3], translations [N, 3], anchors [V, K] int32,
    weights [V, K]) float32. Rotations: synthetic.rodrigues_np of axis-angle vectors with |w| <= 0.3; translations within
    0.05 per axis. Anchor indices lie in [0, N); invalid_share > 0 sets that seeded share of the slots to -1, row V // 2 to
    all -1 and (V >= 2) the row after it to slot 0 only. invalid_share = 0: every slot is valid. Weights are positive and
    sum to one over a row's valid slots; an invalid slot's weight is junk the warp must not read into its sums (inf or
    7.5: the thresholded anchor search leaves squared distances there). No index is ever outside [-1, N - 1]."""
    rng = np.random.default_rng(_seed(seed, V, N, K, round(1000 * invalid_share)))
    points = rng.uniform(-1, 1, (V, 3)).astype(f32)
    normals = rng.normal(size=(V, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32)
    nodes = rng.uniform(-1, 1, (N, 3)).astype(f32)
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    rotations = synthetic.rodrigues_np((axis * rng.uniform(0, 0.3, (N, 1))).astype(f32))
    translations = rng.uniform(-0.05, 0.05, (N, 3)).astype(f32)
    anchors = rng.integers(0, N, (V, K)).astype(np.int32)
    if invalid_share > 0:
        anchors[rng.random((V, K)) < invalid_share] = -1
        anchors[V // 2] = -1
        if V >= 2:
            row = (V // 2 + 1) % V
            anchors[row, 0] = rng.integers(0, N)
            anchors[row, 1:] = -1
    valid = anchors >= 0
    raw = np.where(valid, rng.uniform(0.1, 1.0, (V, K)), 0.0)
    total = raw.sum(axis=1, keepdims=True)
    weights = (raw / np.where(total > 0, total, 1.0)).astype(f32)
    v, k = np.indices((V, K))
    weights[~valid] = np.where((v + k) % 2 == 0, f32(np.inf), f32(7.5))[~valid]
    assert anchors.min() >= -1 and anchors.max() <= N - 1
    return points, normals, nodes, rotations, translations, anchors, weights


# ---- float64 restatements ---------------------------------------------------------------------------------------------
def squared_distances_f64(points, nodes):
    """[V, N] float64 squared distances of the float32 inputs (NaN / inf where a point is not finite)."""
    p = np.asarray(points, f32).astype(np.float64).reshape(-1, 1, 3)
    g = np.asarray(nodes, f32).astype(np.float64).reshape(1, -1, 3)
    with np.errstate(all="ignore"):
        d = g - p
        return (d * d).sum(axis=2)


def anchors_f64(points, nodes, K):
    """Brute-force K-NN in float64: [V, K] int32 node indices in ascending (distance, index) order, -1 where there are
    fewer than K nodes and in every slot of a point with a non-finite coordinate (no distance compares below inf)."""
    sq = squared_distances_f64(points, nodes)
    V, N = sq.shape
    out = np.full((V, K), -1, np.int32)
    finite = np.isfinite(np.asarray(points, f32).reshape(-1, 3)).all(axis=1)
    if N:
        order = np.argsort(np.where(np.isnan(sq), np.inf, sq), axis=1, kind="stable")[:, :K]
        out[:, :order.shape[1]] = order
    out[~finite] = -1
    return out


def weights_f64(points, nodes, anchors, coverage=None, node_weights=None, return_scale=False):
    """The unthresholded anchor weights of the given slots in float64: exp(-d^2 / (2 c^2)), c^2 the float32 coverage
    squared or the anchor node's float32 coverage weight, normalised over the row; an empty slot (-1) weighs 0. A row
    without any weight (no node, or every weight below float32's range) gets 1 / K in every slot, as the search gives it.
    return_scale: also the row's largest weight before normalisation."""
    sq = squared_distances_f64(points, nodes)
    anchors = np.asarray(anchors)
    V, K = anchors.shape
    w = np.zeros((V, K))
    for k in range(K if sq.shape[1] else 0):
        a = anchors[:, k]
        ok = a >= 0
        at = np.where(ok, a, 0)
        c2 = float(f32(coverage)) ** 2 if node_weights is None else np.asarray(node_weights, f32).astype(np.float64)[at]
        d2 = sq[np.arange(V), at]
        w[:, k] = np.where(ok, np.exp(-d2 / (2 * c2)), 0.0)
    # a row all of whose weights vanish in float32 (below half its smallest subnormal) sums to 0 there and gets 1 / K
    vanished = (w < 2.0 ** -150).all(axis=1)
    s = w.sum(axis=1, keepdims=True)
    out = w / np.where(s > 0, s, 1.0)
    out[vanished] = 1.0 / K
    return (out, w.max(axis=1)) if return_scale else out


def warp_f64(points, normals, nodes, rotations, translations, anchors, weights, extrinsics=None):
    """(positions, normals) [V, 3] float64: sum over the valid slots of w (g + R (E p - g) + t) and w R (E_R n)."""
    p = np.asarray(points, f32).astype(np.float64)
    n = np.asarray(normals, f32).astype(np.float64)
    g = np.asarray(nodes, f32).astype(np.float64)
    R = np.asarray(rotations, f32).astype(np.float64).reshape(-1, 3, 3)
    t = np.asarray(translations, f32).astype(np.float64)
    anchors = np.asarray(anchors)
    w = np.asarray(weights, f32).astype(np.float64)
    if extrinsics is not None:
        E = np.asarray(extrinsics, np.float64).astype(f32).astype(np.float64)   # the warp takes the transform as float32
        p = p @ E[:3, :3].T + E[:3, 3]
        n = n @ E[:3, :3].T
    out_p, out_n = np.zeros_like(p), np.zeros_like(n)
    for k in range(anchors.shape[1]):
        a = anchors[:, k]
        ok = a >= 0
        at = np.where(ok, a, 0)
        wk = np.where(ok, w[:, k], 0.0)[:, None]
        moved = g[at] + np.einsum("vab,vb->va", R[at], p - g[at]) + t[at]
        out_p += np.where(ok[:, None], wk * moved, 0.0)
        out_n += np.where(ok[:, None], wk * np.einsum("vab,vb->va", R[at], n), 0.0)
    return out_p, out_n


# ---- the cases both test files run --------------------------------------------------------------------------------------
def unthresholded_anchor_cases():
    """(layout, N, V, K) of every unthresholded anchor comparison: batch boundaries, wave tail, group skipping, ties, N < K."""
    cases = [("uniform", N, BATCH_V, K) for N in BATCH_N for K in ALL_K]
    cases += [("uniform", N, V, 4) for N in TAIL_N for V in TAIL_V]
    cases += [(layout, N, BATCH_V, K) for layout in SKIP_LAYOUTS for N in SKIP_N for K in SKIP_K]
    cases += [(layout, N, BATCH_V, K) for layout in TIE_LAYOUTS for N in TIE_N for K in TIE_K]
    cases += [("uniform", N, BATCH_V, K) for N in FEW_N for K in FEW_K]
    return cases


def warp_cases():
    """(V, K, invalid_share, extrinsics or None) of every warp comparison."""
    E = warp_extrinsics()
    return [(V, K, share, e) for V in WARP_V for K in WARP_QUAD_K + WARP_WIDE_K for share in WARP_INVALID for e in (None, E)]


def valid_counts(anchors):
    return (np.asarray(anchors) >= 0).sum(axis=1)
