"""Sequential restatement of the reference's graph node selection (cpp/cpu/graph_proc.cpp:27-155) in numpy, the checker
of csrc/graph_sampling.hip. float32 throughout; the squared distance is ((dx*dx + dy*dy) + dz*dz), unfused."""
import numpy as np


def erosion_mask(vertex_count, faces, iteration_count, min_neighbors):
    """bool (V,): faces start alive; each iteration counts the alive faces touching every vertex and kills the alive
    faces with a vertex whose count is below min_neighbors; a vertex survives iff an alive face touches it."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    alive = faces
    for _ in range(iteration_count):
        counts = np.bincount(alive.reshape(-1), minlength=vertex_count)
        alive = alive[(counts[alive] >= min_neighbors).all(axis=1)]
    mask = np.zeros(vertex_count, bool)
    mask[alive.reshape(-1)] = True
    return mask


def within(a, b, coverage):
    """The reference's coverage predicate between point(s) a and b, as float32 arithmetic."""
    d = np.asarray(a, np.float32) - np.asarray(b, np.float32)
    c = np.float32(coverage)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= c * c


def candidates(points, mask=None, order=None):
    """Vertex indices in priority order: ascending or `order`, masked-out and non-finite vertices dropped."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    seq = np.arange(len(points)) if order is None else np.asarray(order, np.int64)
    keep = np.isfinite(points[seq]).all(axis=1)
    if mask is not None:
        keep &= np.asarray(mask, bool).reshape(-1)[seq]
    return seq[keep]


def sample_nodes(points, coverage, mask=None, order=None):
    """int64 node vertex indices in acceptance order: a candidate becomes a node iff no earlier node is within coverage."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    nodes = np.empty((len(points), 3), np.float32)
    picked = []
    for v in candidates(points, mask, order):
        n = len(picked)
        if n and within(nodes[:n], points[v], coverage).any():
            continue
        nodes[n] = points[v]
        picked.append(v)
    return np.asarray(picked, np.int64)
