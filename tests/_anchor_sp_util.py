"""CPU restatement of the shortest-path anchor computation (DESIGN.md "Shortest-path anchors"), in plain numpy float32, one
point at a time: a 40-entry list with drop-when-full and a minimum pop (key, then node index). Returns the popped keys
and the number of dropped inserts too, so the tests can assert that every row's keys are distinct (the index tie rule
then decides nothing) and that a case really fills the queue."""
import numpy as np

QUEUE_CAPACITY = 40
F = np.float32


def _sq(a, b):
    dx, dy, dz = F(a[0] - b[0]), F(a[1] - b[1]), F(a[2] - b[2])
    return F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))


def shortest_path_anchors(points, nodes, edges, K, coverage=None, node_weights=None):
    """anchors [V,K] int32, weights [V,K] float32, popped keys (one float32 list per point, every pop including the
    skipped ones), dropped inserts per point [V], and per point the number of times another node's entry sat in the queue
    with the popped key (a tie the index rule decided; 0 wherever the result does not depend on the rule)."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 3)
    edges = np.asarray(edges, np.int32)
    assert edges.ndim == 2 and edges.shape[0] == len(nodes)
    V, N = len(points), len(nodes)
    anchors = np.full((V, K), -1, np.int32)
    weights = np.zeros((V, K), np.float32)
    popped, dropped, ties = [], np.zeros(V, np.int64), np.zeros(V, np.int64)
    for v in range(V):
        p = points[v]
        if N:
            d = p[None, :] - nodes
            sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]   # float32, unfused
        found, dist, queue, keys = [], [], [], []

        def insert(key, node):
            if len(queue) < QUEUE_CAPACITY:
                queue.append((key, node))
            else:
                dropped[v] += 1

        while len(found) < K:
            seed = -1
            if N:
                candidates = sq.copy()
                candidates[found] = np.inf
                j = int(np.argmin(candidates))   # the first minimum: strict <, the lowest index wins a tie
                if candidates[j] < np.inf:
                    best, seed = candidates[j], j
            if seed < 0:
                break
            insert(np.sqrt(F(best)), seed)
            while queue and len(found) < K:
                at = min(range(len(queue)), key=lambda e: (queue[e][0], queue[e][1]))
                key, node = queue.pop(at)
                keys.append(key)
                ties[v] += sum(1 for (ke, ne) in queue if ke == key and ne != node)
                if node in found:
                    continue
                found.append(node)
                dist.append(key)
                if len(found) == K:
                    break
                for t in edges[node]:
                    if t >= 0:
                        insert(F(key + np.sqrt(_sq(nodes[t], nodes[node]))), int(t))
        popped.append(keys)
        w = np.zeros(K, np.float32)
        total = F(0)
        for k, (node, dk) in enumerate(zip(found, dist)):
            c2 = F(node_weights[node]) if node_weights is not None else F(F(coverage) * F(coverage))
            x = F(-F(dk * dk) / F(F(2) * c2))
            w[k] = F(np.exp(np.float64(x)))
            total = F(total + w[k])
        anchors[v, :len(found)] = found
        weights[v] = w / total if total > 0 else F(1) / F(K)
    return anchors, weights, popped, dropped, ties


def keys_distinct(popped):
    """Every point's popped keys are pairwise distinct."""
    return all(len(set(np.asarray(k, np.float32).tolist())) == len(k) for k in popped)


def knn_edge_rows(nodes, D):
    """[N,D] int32 rows of each node's D Euclidean-nearest other nodes (float64 distances, stable order), -1 padded."""
    nodes = np.asarray(nodes, np.float64)
    N = len(nodes)
    rows = np.full((N, D), -1, np.int32)
    for i in range(N):
        d = np.linalg.norm(nodes - nodes[i], axis=1)
        d[i] = np.inf
        order = np.argsort(d, kind="stable")[:min(D, N - 1)]
        rows[i, :len(order)] = order
    return rows


def jittered_grid(nx, ny, spacing, seed, z=0.0, jitter=0.3):
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    g = np.stack([gx.ravel(), gy.ravel(), np.zeros(nx * ny)], axis=1) * spacing
    g += rng.uniform(-jitter, jitter, g.shape) * spacing * np.array([1.0, 1.0, 0.3])
    g[:, 2] += z
    return g.astype(np.float32)
