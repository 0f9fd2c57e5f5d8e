"""Mirror of the reference's legacy graph_proc bindings at the top level of `nnrt` (cpp/pybind/nnrt_pybind.cpp:121-126 ->
cpp/cpu/graph_proc.cpp:27-155), computed on the GPU (csrc/graph_sampling.hip): the vertex erosion mask of a mesh and the
greedy node sampling that picks a motion graph's nodes from its vertices. Both accept numpy arrays or device tensors and
return device tensors; both return exactly what the reference's sequential loops return. Further down, the rest of the
depth-image graph (nnrt_pybind.cpp:143-153, :219-225 -> graph_proc.cpp:181-338, :540-636; csrc/depth_graph.hip): geodesic
edges on the GPU, node clean-up and clusters as host code in the library.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from ._overloads import Overloaded, is_tensor
from ._tensors import to_device


def _dev() -> torch.device:
    return torch.device("cuda", N.current_device())


def get_vertex_erosion_mask(vertex_positions, face_indices, iteration_count, min_neighbors) -> torch.Tensor:
    """get_vertex_erosion_mask (graph_proc.cpp:27-90): bool (V, 1), true where the vertex survives `iteration_count`
    rounds of removing every face that has a vertex touched by fewer than `min_neighbors` remaining faces. Only the
    vertex count of `vertex_positions` is used, as in the reference. A face index outside [0, V) raises NnrtError."""
    dev = _dev()
    vertex_count = int(vertex_positions.shape[0])
    faces = to_device(face_indices, torch.int64, dev).reshape(-1, 3)
    mask = torch.empty(vertex_count, dtype=torch.uint8, device=dev)
    N.check(N.lib().nnrt_get_vertex_erosion_mask(vertex_count, N.ptr(faces), faces.shape[0], int(iteration_count), int(min_neighbors),
                                                 N.ptr(mask), N.stream_ptr()))
    return mask.view(torch.bool).reshape(vertex_count, 1)


def shuffle_permutation(vertex_count: int, seed: int) -> torch.Tensor:
    """The priority order `sample_nodes(..., random_shuffle=True, seed=seed)` uses: int64 (V,), host tensor, from a seeded
    CPU `torch.Generator` (the same on every device)."""
    generator = torch.Generator(device="cpu")
    generator.manual_seed(int(seed))
    return torch.randperm(int(vertex_count), generator=generator, dtype=torch.int64)


def sample_node_indices(vertex_positions, vertex_mask=None, order=None, node_coverage: float = 0.05) -> Tuple[torch.Tensor, int]:
    """The C-ABI call behind sample_nodes: (int64 node vertex indices in acceptance order, rounds taken). `vertex_mask`
    (V,) or (V, 1) bool restricts the candidates, `order` (V,) int64 is a permutation giving the priority order; None
    means every vertex / ascending index."""
    dev = _dev()
    p = to_device(vertex_positions, torch.float32, dev).reshape(-1, 3)
    count = p.shape[0]
    m = None
    if vertex_mask is not None:
        m = to_device(vertex_mask, torch.bool, dev).reshape(-1).view(torch.uint8)
        if m.shape[0] != count:
            raise ValueError(f"vertex mask has {m.shape[0]} entries for {count} vertices")
    o = None
    if order is not None:
        o = to_device(order, torch.int64, dev).reshape(-1)
        if o.shape[0] != count:
            raise ValueError(f"order has {o.shape[0]} entries for {count} vertices")
    out = torch.empty(max(count, 1), dtype=torch.int64, device=dev)
    n = np.zeros(1, np.int64)
    rounds = np.zeros(1, np.int32)
    N.check(N.lib().nnrt_sample_nodes(N.ptr(p), count, N.ptr(m), N.ptr(o), float(node_coverage), N.ptr(out), out.shape[0], N.ptr(n),
                                      N.ptr(rounds), N.stream_ptr()))
    return out[: int(n[0])], int(rounds[0])


def sample_nodes(vertex_positions_in, vertex_erosion_mask_in, node_coverage, use_only_non_eroded_indices, random_shuffle,
                 seed: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """sample_nodes (graph_proc.cpp:92-155): (node_positions (n, 3) float32, node_vertex_indices (n, 1) int32). Vertices are
    visited in ascending index, or in a random permutation (`random_shuffle`); a vertex becomes a node iff no earlier node
    lies within `node_coverage` of it. The reference shuffles with std::random_device and cannot be reproduced; here the
    permutation is `shuffle_permutation(V, seed)`, and `seed=None` draws a fresh seed. Vertices with a non-finite
    coordinate are skipped (in the reference they always become nodes)."""
    dev = _dev()
    p = to_device(vertex_positions_in, torch.float32, dev).reshape(-1, 3)
    order = None
    if random_shuffle:
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little") >> 1
        order = shuffle_permutation(p.shape[0], seed)
    mask = vertex_erosion_mask_in if use_only_non_eroded_indices else None
    if use_only_non_eroded_indices and mask is None:
        raise ValueError("use_only_non_eroded_indices needs vertex_erosion_mask_in")
    indices, _ = sample_node_indices(p, mask, order, node_coverage)
    return p[indices], indices.to(torch.int32).reshape(-1, 1)


# ---- geodesic edges, clean-up and clusters of the depth-image graph (nnrt_pybind.cpp:143-153, :219-225; csrc/depth_graph.hip) ----
def _edges_shortest_path(vertex_positions_in, vertex_mask_in, face_indices_in, node_indices_in, max_neighbor_count, node_coverage,
                         enforce_total_num_neighbors):
    dev = _dev()
    vertices = to_device(vertex_positions_in, torch.float32, dev).reshape(-1, 3)
    vertex_count = vertices.shape[0]
    mask = None
    if vertex_mask_in is not None:
        mask = to_device(vertex_mask_in, torch.bool, dev).reshape(-1).view(torch.uint8)
        if mask.shape[0] != vertex_count:
            raise ValueError(f"vertex mask has {mask.shape[0]} entries for {vertex_count} vertices")
    faces = to_device(face_indices_in, torch.int32, dev).reshape(-1, 3)
    nodes = to_device(node_indices_in, torch.int32, dev).reshape(-1)
    node_count, K = nodes.shape[0], int(max_neighbor_count)
    edges = torch.empty((node_count, max(K, 0)), dtype=torch.int32, device=dev)
    weights = torch.empty((node_count, max(K, 0)), dtype=torch.float32, device=dev)
    distances = torch.empty((node_count, max(K, 0)), dtype=torch.float32, device=dev)
    N.check(N.lib().nnrt_compute_edges_shortest_path(N.ptr(vertices), vertex_count, N.ptr(mask), N.ptr(faces), faces.shape[0], N.ptr(nodes),
                                                     node_count, K, float(node_coverage), int(bool(enforce_total_num_neighbors)),
                                                     N.ptr(edges), N.ptr(weights), N.ptr(distances), None, N.stream_ptr()))
    return edges, weights, distances, None


compute_edges_shortest_path = Overloaded(
    "compute_edges_shortest_path",
    """compute_edges_shortest_path (graph_proc.cpp:181-338, both value-returning overloads): (graph_edges (N, K) int32,
    graph_edge_weights (N, K) float32, graph_edge_distances (N, K) float32, None), device tensors. Row i holds the other
    nodes reached from node i's vertex over the mesh edges, by ascending float32 shortest-path length (the reference's
    Dijkstra values, bit for bit), truncated to K; unused slots are -1 / 0 / 0. Nodes at equal distance are ordered by node
    index (the reference: by its heap's state). The fourth entry of the reference's tuple, the dense N x V
    node_to_vertex_distances that only the DeformNet pixel anchors read, is not produced: None. A face index outside
    [0, V), a node vertex index >= V and duplicate node vertex indices raise NnrtError; a negative node vertex index gives
    an all-default row.""")


@compute_edges_shortest_path.overload(lambda a: is_tensor(a["vertex_mask_in"]) and is_tensor(a["face_indices_in"]) and is_tensor(a["node_indices_in"]))
def _compute_edges_shortest_path_masked(vertex_positions_in, vertex_mask_in, face_indices_in, node_indices_in, max_neighbor_count, node_coverage,
                                        enforce_total_num_neighbors):
    return _edges_shortest_path(vertex_positions_in, vertex_mask_in, face_indices_in, node_indices_in, max_neighbor_count, node_coverage,
                                enforce_total_num_neighbors)


@compute_edges_shortest_path.overload(lambda a: is_tensor(a["face_indices_in"]) and is_tensor(a["node_indices_in"]))
def _compute_edges_shortest_path_all(vertex_positions_in, face_indices_in, node_indices_in, max_neighbor_count, node_coverage,
                                     enforce_total_num_neighbors):
    return _edges_shortest_path(vertex_positions_in, None, face_indices_in, node_indices_in, max_neighbor_count, node_coverage,
                                enforce_total_num_neighbors)


def _host_edges(graph_edges) -> np.ndarray:
    if isinstance(graph_edges, torch.Tensor):
        graph_edges = graph_edges.detach().cpu().numpy()
    e = np.ascontiguousarray(np.asarray(graph_edges), dtype=np.int32)
    if e.ndim != 2:
        raise ValueError(f"graph edges must be (N, K), got {e.shape}")
    return e


def node_and_edge_clean_up(graph_edges, valid_nodes_mask):
    """node_and_edge_clean_up (graph_proc.cpp:540-590): clears `valid_nodes_mask` (N, 1) or (N,) bool, in place, for every
    valid node of which at most one entry before its row's first -1 names a node not removed by this call, repeated to the
    fixed point (independent of the visiting order), and returns it. Host code in the library after one copy; a torch
    tensor (any device) or a numpy array is updated in place."""
    e = _host_edges(graph_edges)
    if isinstance(valid_nodes_mask, torch.Tensor):
        host = valid_nodes_mask.detach().to(device="cpu", dtype=torch.bool).reshape(-1).numpy().astype(np.uint8)
    else:
        host = np.asarray(valid_nodes_mask).reshape(-1).astype(np.uint8)
    if host.shape[0] != e.shape[0]:
        raise ValueError(f"valid nodes mask has {host.shape[0]} entries for {e.shape[0]} nodes")
    N.check(N.lib().nnrt_node_and_edge_clean_up(N.ptr(e), e.shape[0], e.shape[1], N.ptr(host)))
    if isinstance(valid_nodes_mask, torch.Tensor):
        valid_nodes_mask.copy_(torch.from_numpy(host).reshape(valid_nodes_mask.shape).to(valid_nodes_mask.dtype))
    else:
        valid_nodes_mask[...] = host.reshape(valid_nodes_mask.shape).astype(valid_nodes_mask.dtype)
    return valid_nodes_mask


def compute_clusters(graph_edges_in):
    """compute_clusters (graph_proc.cpp:592-636): (cluster sizes as a list, clusters (N, 1) int32): the components of the
    undirected graph over each row's entries up to its first -1, numbered by ascending lowest member. Host code in the
    library after one copy; `clusters` is a tensor on the input's device for a tensor input, else a numpy array."""
    e = _host_edges(graph_edges_in)
    clusters = np.full(e.shape[0], -1, np.int32)
    sizes = np.zeros(max(e.shape[0], 1), np.int32)
    count = np.zeros(1, np.int64)
    N.check(N.lib().nnrt_compute_clusters(N.ptr(e), e.shape[0], e.shape[1], N.ptr(clusters), N.ptr(sizes), N.ptr(count)))
    clusters = clusters.reshape(-1, 1)
    if isinstance(graph_edges_in, torch.Tensor):
        clusters = torch.from_numpy(clusters).to(graph_edges_in.device)
    return [int(s) for s in sizes[: int(count[0])]], clusters
