"""Sequential restatement of the reference's depth-image graph loops in numpy / heapq, the checker of csrc/depth_graph.hip:
compute_mesh_from_depth (cpp/cpu/image_proc.cpp:341-482), compute_edges_shortest_path (cpp/cpu/graph_proc.cpp:181-338),
node_and_edge_clean_up and compute_clusters (graph_proc.cpp:540-636). float32 throughout; an edge length is
sqrt((dx*dx + dy*dy) + dz*dz), unfused and correctly rounded, and a relaxation is d_u + length in float32."""
import heapq

import numpy as np

F32 = np.float32


def edge_length(a, b):
    d = np.asarray(a, F32) - np.asarray(b, F32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=F32)


def mesh_from_depth(point_image, max_triangle_edge_distance):
    """(vertices (V, 3) float32, vertex_pixels (V, 2) int32 as (x, y), faces (F, 3) int32) of the reference's loop; empty
    arrays when there is no valid triangle."""
    p = np.asarray(point_image, F32)
    H, W = p.shape[:2]
    limit = F32(max_triangle_edge_distance)
    vertices, pixels, faces = [], [], []
    index = {}
    if H >= 2 and W >= 2:
        # the three edge tests of both triangles of every cell at once; the numbering loop below stays sequential
        with np.errstate(invalid="ignore"):
            ok = p[..., 2] > 0
            e_down = edge_length(p[:-1, :], p[1:, :]) <= limit          # (x, y) - (x, y+1)
            e_right = edge_length(p[:, :-1], p[:, 1:]) <= limit         # (x, y) - (x+1, y)
            e_diag = edge_length(p[1:, :-1], p[:-1, 1:]) <= limit       # (x, y+1) - (x+1, y)
        a_ok = ok[:-1, :-1] & ok[1:, :-1] & ok[:-1, 1:] & e_down[:, :-1] & e_right[:-1, :] & e_diag
        b_ok = ok[1:, 1:] & ok[:-1, 1:] & ok[1:, :-1] & e_diag & e_down[:, 1:] & e_right[1:, :]

        def vertex(x, y):
            v = index.get((x, y))
            if v is None:
                v = index[(x, y)] = len(vertices)
                vertices.append(p[y, x])
                pixels.append((x, y))
            return v
        for y, x in zip(*np.nonzero(a_ok | b_ok)):   # row-major
            y, x = int(y), int(x)
            if a_ok[y, x]:
                faces.append((vertex(x, y), vertex(x, y + 1), vertex(x + 1, y)))
            if b_ok[y, x]:
                faces.append((vertex(x + 1, y + 1), vertex(x + 1, y), vertex(x, y + 1)))
    return (np.asarray(vertices, F32).reshape(-1, 3), np.asarray(pixels, np.int32).reshape(-1, 2), np.asarray(faces, np.int32).reshape(-1, 3))


def vertex_neighbors(vertex_count, faces):
    """CSR (starts, targets): per vertex the sorted other vertices of its faces (the reference's std::set<int> per vertex)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    pairs = np.concatenate([faces[:, [i, j]] for i in range(3) for j in range(3) if i != j]) if len(faces) else np.zeros((0, 2), np.int64)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    keys = np.unique(pairs[:, 0] * vertex_count + pairs[:, 1])
    sources, targets = keys // max(vertex_count, 1), keys % max(vertex_count, 1)
    return np.searchsorted(sources, np.arange(vertex_count + 1)), targets


def edges_shortest_path(vertices, faces, node_vertex_indices, max_neighbor_count, node_coverage, enforce_total_num_neighbors, vertex_mask=None,
                        rows=None):
    """(edges (N, K) int32, weights (N, K) float32, distances (N, K) float32, first) of the reference's Dijkstra per node
    (only the nodes in `rows` if given; the other rows stay default). first[i] lists the distances of the first K + 1
    other nodes reached from node i, had the loop not stopped at K: a test asserts that they are pairwise distinct, so the
    order of the row does not depend on how ties are broken."""
    vertices = np.asarray(vertices, F32).reshape(-1, 3)
    nodes = np.asarray(node_vertex_indices, np.int64).reshape(-1)
    V, N, K = len(vertices), len(nodes), int(max_neighbor_count)
    c = F32(node_coverage)
    radius = F32(2) * c
    mask = None if vertex_mask is None else np.asarray(vertex_mask, bool).reshape(-1)
    starts, targets = vertex_neighbors(V, faces)
    vertex_node = np.full(V, -1, np.int64)
    for i, v in enumerate(nodes):
        if v >= 0:
            vertex_node[v] = i
    edges = np.full((N, K), -1, np.int32)
    weights = np.zeros((N, K), F32)
    distances = np.zeros((N, K), F32)
    first = {}
    for i in (range(N) if rows is None else rows):
        if nodes[i] < 0:
            first[i] = []
            continue
        heap = [(F32(0), int(nodes[i]))]
        visited = set()
        found = []
        while heap and len(found) < K + 1:
            d, v = heapq.heappop(heap)
            if v in visited:
                continue
            visited.add(v)
            other = vertex_node[v]
            if other >= 0 and other != i:
                found.append((d, int(other)))
            near = targets[starts[v]:starts[v + 1]]
            for n, length in zip(near, edge_length(vertices[v], vertices[near])):
                if mask is not None and not mask[n]:
                    continue
                nd = F32(d + length)
                if enforce_total_num_neighbors or nd <= radius:
                    heapq.heappush(heap, (nd, int(n)))
        first[i] = [d for d, _ in found]
        found = found[:K]
        w = [np.exp(-(d * d) / (F32(2) * c * c), dtype=F32) for d, _ in found]
        total = F32(0)
        for x in w:
            total = F32(total + x)
        for k, (d, other) in enumerate(found):
            edges[i, k] = other
            distances[i, k] = d
            weights[i, k] = w[k] / total if total > 0 else w[k] / F32(len(found))
    return edges, weights, distances, first


def weights_from_distances(distances, counts, node_coverage):
    """The row weights in float64 from float32 distances: exp(-(d*d) / (2 c c)) over the row's sum."""
    d = np.asarray(distances, np.float64)
    c = float(F32(node_coverage))
    w = np.exp(-(d * d) / (2.0 * c * c))
    w[np.arange(d.shape[1])[None, :] >= np.asarray(counts)[:, None]] = 0.0
    total = w.sum(axis=1, keepdims=True)
    return np.divide(w, total, out=np.zeros_like(w), where=total > 0)


def node_and_edge_clean_up(graph_edges, valid_nodes_mask):
    """The reference's passes, in its visiting order: returns the new mask (N,) bool."""
    edges = np.asarray(graph_edges)
    valid = np.asarray(valid_nodes_mask, bool).reshape(-1).copy()
    removed = set()
    while True:
        newly = 0
        for i in range(len(edges)):
            if not valid[i]:
                continue
            live = 0
            for n in edges[i]:
                if n == -1:
                    break
                if int(n) not in removed:
                    live += 1
            if live <= 1:
                valid[i] = False
                removed.add(i)
                newly += 1
        if newly == 0:
            return valid


def compute_clusters(graph_edges):
    """(sizes list, clusters (N, 1) int32): the reference's traversal."""
    edges = np.asarray(graph_edges)
    N = len(edges)
    neighbors = [set() for _ in range(N)]
    for i in range(N):
        for n in edges[i]:
            if n == -1:
                break
            neighbors[i].add(int(n))
            neighbors[int(n)].add(i)
    ids = np.full(N, -1, np.int32)
    sizes = []
    for i in range(N):
        if ids[i] != -1:
            continue
        active = {i}
        size = 0
        while active:
            a = min(active)
            active.remove(a)
            if ids[a] == -1:
                ids[a] = len(sizes)
                size += 1
            active.update(n for n in neighbors[a] if ids[n] == -1)
        sizes.append(size)
    return sizes, ids.reshape(-1, 1)


def compact_graph(edges, weights, distances, valid):
    """create_graph_data.py:199-272: keep the valid nodes' rows, drop removed neighbours shifting left, re-index, and divide
    each row's weights by their float32 numpy sum."""
    valid = np.asarray(valid, bool).reshape(-1)
    mapping = np.where(valid, np.cumsum(valid) - 1, -1)
    edges, weights, distances = edges[valid].copy(), weights[valid].copy(), distances[valid].copy()
    if valid.all():
        return edges, weights, distances
    for i in range(len(edges)):
        row, w, d = edges[i].copy(), weights[i].copy(), distances[i].copy()
        edges[i], weights[i], distances[i] = -1, 0, 0
        k = 0
        for j, n in enumerate(row):
            if n != -1 and not valid[n]:
                continue
            edges[i, k] = -1 if n == -1 else mapping[n]
            weights[i, k] = w[j]
            distances[i, k] = d[j]
            k += 1
        weights[i] /= np.sum(weights[i])
    return edges, weights, distances
