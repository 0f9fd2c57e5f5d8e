"""numpy restatement of the uniform-grid point index (csrc/spatial_grid.hip): grid cells, cell means,
closest-to-mean and medoid samples, the two-stage radius samplers and brute-force K nearest neighbours, in the float32
expressions the kernels use. Shared by tests/test_spatial_index_cpu.py and tests/test_gpu_spatial_index.py."""
import numpy as np

F32 = np.float32


def cells_of(points, cell_size, offset=(0., 0., 0.)):
    """(member lists, one per occupied cell, cells ordered by their first member index; members ascending)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    keys = np.floor(p / F32(cell_size) + np.asarray(offset, F32))
    assert keys.dtype == F32
    if len(p) == 0:
        return []
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(first, kind="stable")   # unique cell -> rank by first member
    members = [np.flatnonzero(inverse == u) for u in order]
    return members


def mean_grid(points, cell_size, offset=(0., 0., 0.)):
    p = np.asarray(points, F32).reshape(-1, 3)
    rows = [p[m].astype(np.float64).mean(axis=0).astype(F32) for m in cells_of(p, cell_size, offset)]
    return np.array(rows, F32).reshape(-1, 3)


def _sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def closest_to_mean_grid(points, cell_size, offset=(0., 0., 0.)):
    p = np.asarray(points, F32).reshape(-1, 3)
    out = []
    for m in cells_of(p, cell_size, offset):
        mean = p[m].astype(np.float64).mean(axis=0).astype(F32)
        d = _sq(p[m] - mean)
        assert d.dtype == F32
        out.append(m[int(np.argmin(d))])   # the first smallest: ties to the lower index
    return np.sort(np.array(out, np.int64))


def median_grid(points, cell_size, offset=(0., 0., 0.)):
    """The medoid of every cell: sum_a = sequential float32 sum over the members b, ascending, of sqrt of the squared
    distance; the first member with the smallest sum below FLT_MAX, else the cell's first member."""
    p = np.asarray(points, F32).reshape(-1, 3)
    fmax = np.finfo(F32).max
    out = []
    for m in cells_of(p, cell_size, offset):
        q = p[m]
        dist = np.sqrt(_sq(q[None, :, :] - q[:, None, :]))   # [a, b] = |p_b - p_a|
        assert dist.dtype == F32
        sums = np.zeros(len(m), F32)
        for b in range(len(m)):
            sums = sums + dist[:, b]
        best, best_i = fmax, m[0]
        for a in range(len(m)):
            if sums[a] < best:
                best, best_i = sums[a], m[a]
        out.append(best_i)
    return np.sort(np.array(out, np.int64))


def extended_cell(radius):
    r = F32(radius)
    return np.sqrt(F32(2) * (r * r)) * F32(2)


def fast_mean_radius(points, radius):
    cell = extended_cell(radius)
    return mean_grid(mean_grid(points, cell), cell, (0.5, 0.5, 0.5))


def fast_median_radius(points, radius):
    p = np.asarray(points, F32).reshape(-1, 3)
    cell = extended_cell(radius)
    stage_1 = median_grid(p, cell)
    stage_2 = median_grid(p[stage_1], cell, (0.5, 0.5, 0.5))
    return stage_1[stage_2]


def knn(points, queries, k):
    """(indices [Q, k] int32, distances [Q, k] float32) by brute force, rows ordered by (squared distance, index);
    -1 / +inf past the point count."""
    p = np.asarray(points, F32).reshape(-1, 3)
    q = np.asarray(queries, F32).reshape(-1, 3)
    idx = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), np.inf, F32)
    ids = np.arange(len(p))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(len(q)):
            d2 = _sq(p - q[s])
            assert d2.dtype == F32
            order = np.lexsort((ids, d2))[:k]
            idx[s, :len(order)] = order
            dist[s, :len(order)] = np.sqrt(d2[order])
    return idx, dist


def ulp_distance(a, b):
    """Elementwise distance in float32 units in the last place between two finite float32 arrays."""
    def ordered(x):
        bits = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(bits < 0, np.int64(-2 ** 31) - bits, bits)   # -0.0 and +0.0 coincide
    return np.abs(ordered(a) - ordered(b))
