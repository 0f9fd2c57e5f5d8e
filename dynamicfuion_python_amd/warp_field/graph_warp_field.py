"""Motion graph from a mesh (reference warp_field/graph_warp_field.py:24-42): erode the mesh's border vertices, sample the
graph nodes greedily from the remaining vertices, build the warp field over them -- all on the GPU
(csrc/graph_sampling.hip, csrc/hierarchy.hip); and the graph from a masked depth image (reference
apps/create_graph_data.py:27-296): pixel-connected mesh, erosion, node sampling, geodesic edges, clean-up and clusters
(csrc/depth_graph.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import nnrt
from ..nnrt import geometry as G


def sample_graph_nodes_from_mesh(mesh: G.TriangleMesh, node_coverage: float = 0.05, erosion_iteration_count: int = 10,
                                 erosion_min_neighbor_count: int = 4) -> Tuple[torch.Tensor, torch.Tensor]:
    """graph_warp_field.py:28-37: (node_positions (n, 3) float32, node_vertex_indices (n, 1) int32) of the mesh's
    non-eroded vertices sampled in ascending vertex order (use_only_non_eroded_indices=True, random_shuffle=False)."""
    erosion_mask = nnrt.get_vertex_erosion_mask(mesh.vertex_positions, mesh.triangle_indices, erosion_iteration_count,
                                                erosion_min_neighbor_count)
    return nnrt.sample_nodes(mesh.vertex_positions, erosion_mask, node_coverage, use_only_non_eroded_indices=True, random_shuffle=False)


def build_deformation_graph_from_mesh(mesh: G.TriangleMesh, node_coverage: float = 0.05, erosion_iteration_count: int = 10,
                                      erosion_min_neighbor_count: int = 4, neighbor_count: int = 8, minimum_valid_anchor_count: int = 3, *,
                                      anchor_count: int = 4, layer_count: int = 2,
                                      device: Optional[int] = None) -> G.HierarchicalGraphWarpField:
    """build_deformation_graph_from_mesh (graph_warp_field.py:24-42) with the reference's name and leading arguments.
    `neighbor_count` is accepted and unused: the reference feeds it to its geodesic edge construction
    (compute_edges_shortest_path), while HierarchicalGraphWarpField derives its layers and edges from the node positions.
    Raises ValueError when the sampling yields no node (an empty or fully eroded mesh)."""
    if device is not None:
        with torch.cuda.device(int(device)):
            nodes, _ = sample_graph_nodes_from_mesh(mesh, node_coverage, erosion_iteration_count, erosion_min_neighbor_count)
    else:
        nodes, _ = sample_graph_nodes_from_mesh(mesh, node_coverage, erosion_iteration_count, erosion_min_neighbor_count)
    if nodes.shape[0] == 0:
        raise ValueError("no graph node was sampled: the mesh is empty or erodes to nothing "
                         f"({erosion_iteration_count} iterations, min_neighbors {erosion_min_neighbor_count})")
    return G.HierarchicalGraphWarpField(nodes, node_coverage=node_coverage, anchor_count=anchor_count,
                                        minimum_valid_anchor_count=minimum_valid_anchor_count, layer_count=layer_count, device=device)


def extend_warp_field(warp_field: G.HierarchicalGraphWarpField, canonical_mesh, make_warp_field, support_ratio_threshold: float = 1.0,
                      minimum_new_node_count: int = 1):
    """Extend the warp field over canonical surface its nodes do not support (DynamicFusion section 3.4; the reference has
    no counterpart): (warp_field, order, new_node_positions).

    The vertices of `canonical_mesh` (a TriangleMesh or a [V, 3] array) farther than support_ratio_threshold * node_coverage
    from every node are the candidates; new nodes are sampled among them greedily in ascending vertex index at spacing
    node_coverage (nnrt.graph_proc.sample_node_indices). Fewer than minimum_new_node_count of them (or none): the field is
    returned as it is, with the identity order and an empty (0, 3) tensor. Otherwise each new node takes the current field's
    own motion at its position (functional.blend_node_transformations over the field's anchor_count nearest nodes, original
    node order), `make_warp_field([old nodes; new nodes])` builds the new field -- it returns the field, or (field, order)
    with order[v] = the index in the nodes it was given of the field's node v when it re-orders them
    (FusionPipeline.make_warp_field, quirk A5) -- and the field's motion is set to [R_old; R_new][order], [t_old; t_new][order]:
    old nodes keep their motion exactly. new_node_positions (M, 3) is a device tensor in sampling order."""
    vertices = getattr(canonical_mesh, "vertex_positions", canonical_mesh)
    nodes = warp_field.get_node_positions()
    coverage = warp_field.node_coverage
    support_ratio, _ = G.compute_vertex_support(vertices, nodes, coverage)
    vertices = torch.as_tensor(vertices, device=support_ratio.device).to(torch.float32).reshape(-1, 3)
    indices, _ = nnrt.graph_proc.sample_node_indices(vertices, support_ratio > support_ratio_threshold, None, coverage)
    new_positions = vertices[indices]
    if indices.shape[0] < max(int(minimum_new_node_count), 1):
        return warp_field, np.arange(warp_field.node_count), new_positions[:0]
    rotations, translations = warp_field.get_node_rotations(), warp_field.get_node_translations()
    new_rotations, new_translations, _ = G.blend_node_transformations(new_positions, nodes, rotations, translations, warp_field.anchor_count,
                                                                      coverage)
    made = make_warp_field(np.concatenate([nodes, new_positions.cpu().numpy()]))
    extended, order = made if isinstance(made, tuple) else (made, np.arange(warp_field.node_count + indices.shape[0]))
    order = np.asarray(order, np.int64)
    extended.set_node_rotations(np.concatenate([rotations, new_rotations.cpu().numpy()])[order])
    extended.set_node_translations(np.concatenate([translations, new_translations.cpu().numpy()])[order])
    return extended, order, new_positions


@dataclass
class DepthImageGraph:
    """What build_graph_nodes_from_depth_image computes; device tensors, nodes in sampling order with the removed ones
    dropped."""
    vertices: torch.Tensor              # (V, 3) float32: the depth mesh
    vertex_pixels: torch.Tensor         # (V, 2) int32 as (x, y)
    faces: torch.Tensor                 # (F, 3) int32
    non_eroded_vertices: torch.Tensor   # (V, 1) bool
    node_positions: torch.Tensor        # (N, 3) float32
    node_vertex_indices: torch.Tensor   # (N, 1) int32
    edges: torch.Tensor                 # (N, K) int32, -1 in unused slots
    edge_weights: torch.Tensor          # (N, K) float32
    edge_distances: torch.Tensor        # (N, K) float32
    clusters: torch.Tensor              # (N, 1) int32
    cluster_sizes: List[int]


def build_graph_nodes_from_depth_image(depth, mask, intrinsic_matrix, max_triangle_distance: float = 0.05,
                                       depth_scale_reciprocal: float = 1000.0, erosion_num_iterations: int = 10,
                                       erosion_min_neighbors: int = 4, remove_nodes_with_too_few_neighbors: bool = True,
                                       use_only_valid_vertices: bool = True, sample_random_shuffle: bool = False, neighbor_count: int = 8,
                                       enforce_neighbor_count: bool = True, node_coverage: float = 0.05, **unsupported) -> DepthImageGraph:
    """build_graph_warp_field_from_depth_image (apps/create_graph_data.py:27-296) up to the graph itself, with the
    reference's keyword arguments and defaults (`scene_flow_path` is refused, `enable_visual_debugging` does not exist;
    `node_coverage` is honoured -- the reference overwrites it with its global setting). `depth` is an (H, W) integer depth
    image in 1 / depth_scale_reciprocal metres or a float32 one in metres, `mask` an (H, W) image that is non-zero on the
    object or None for a depth image that is masked already; numpy arrays or tensors. Steps :60-285: mask the depth,
    back-project, pixel-connected mesh, erosion mask, node sampling, geodesic edges over every vertex, clean-up of nodes
    with at most one neighbour, compaction and re-indexing of the rows (removed neighbours dropped, entries shifted left,
    weights renormalized), clusters. The pixel anchors (:183-187) are not computed. Raises ValueError for an empty mesh, a
    graph without nodes or a cluster of at most two nodes (the reference asserts, calls exit() or raises)."""
    if unsupported:
        if "scene_flow_path" in unsupported:
            raise ValueError("scene_flow_path is not supported: the graph is built from depth alone")
        raise TypeError(f"unexpected keyword arguments {sorted(unsupported)}")
    K = np.asarray(intrinsic_matrix, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if mask is not None:
        if isinstance(depth, torch.Tensor):
            keep = torch.as_tensor(mask, device=depth.device) > 0
            bits = depth.view(torch.int16) if depth.dtype == torch.uint16 else depth
            depth = torch.where(keep, bits, torch.zeros_like(bits)).view(depth.dtype)
        else:
            keep = (mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)) > 0
            depth = np.where(keep, depth, np.zeros_like(depth))
    point_image = nnrt.image_proc.backproject_depth(depth, fx, fy, cx, cy, depth_scale_reciprocal)
    vertices, vertex_pixels, faces = nnrt.compute_mesh_from_depth(point_image, max_triangle_distance)
    if vertices.shape[0] == 0:
        raise ValueError("the depth image yields no mesh: no triangle with three valid depths and edges within max_triangle_distance")
    non_eroded = nnrt.get_vertex_erosion_mask(vertices, faces, erosion_num_iterations, erosion_min_neighbors)
    node_positions, node_indices = nnrt.sample_nodes(vertices, non_eroded, node_coverage, use_only_valid_vertices, sample_random_shuffle)
    node_count = node_positions.shape[0]
    if node_count == 0:
        raise ValueError("no graph node was sampled from the depth image (the mesh erodes to nothing)")
    # :154-160: every vertex is visible
    edges, weights, distances, _ = nnrt.compute_edges_shortest_path(vertices, faces, node_indices, neighbor_count, node_coverage,
                                                                    enforce_neighbor_count)
    valid = torch.ones((node_count, 1), dtype=torch.bool, device=edges.device)
    if remove_nodes_with_too_few_neighbors:
        nnrt.node_and_edge_clean_up(edges, valid)
    keep = valid.reshape(-1)
    if not bool(keep.any()):
        raise ValueError("no graph node is left after removing the nodes with at most one neighbour")
    if not bool(keep.all()):
        # :221-272: rows of the kept nodes; entries naming a removed node dropped, the rest shifted left (a stable sort
        # on "dropped"), ids re-mapped, weights divided by their row sum
        new_id = torch.where(keep, torch.cumsum(keep.to(torch.int64), 0) - 1, torch.full_like(keep, -1, dtype=torch.int64))
        edges, weights, distances = edges[keep], weights[keep], distances[keep]
        named = edges >= 0
        dropped = named & ~keep[edges.clamp(min=0).to(torch.int64)]
        order = torch.sort(dropped.to(torch.int8), dim=1, stable=True).indices
        mapped = torch.where(named, new_id[edges.clamp(min=0).to(torch.int64)], torch.full_like(edges, -1, dtype=torch.int64))
        mapped = torch.where(dropped, torch.full_like(mapped, -1), mapped).to(torch.int32)
        weights = torch.where(dropped, torch.zeros_like(weights), weights)
        distances = torch.where(dropped, torch.zeros_like(distances), distances)
        edges = torch.gather(mapped, 1, order)
        weights = torch.gather(weights, 1, order)
        distances = torch.gather(distances, 1, order)
        sums = weights.sum(dim=1, keepdim=True)
        if not bool((sums > 0).all()):
            raise ValueError("weight sum for node anchors is not positive after removing nodes")
        weights = weights / sums
        node_positions, node_indices = node_positions[keep], node_indices[keep]
    cluster_sizes, clusters = nnrt.compute_clusters(edges)
    for i, size in enumerate(cluster_sizes):
        if size <= 2:
            members = torch.nonzero(clusters.reshape(-1) == i).reshape(-1).tolist()
            raise ValueError(f"cluster is too small: {size}, it only has nodes {members}")
    return DepthImageGraph(vertices, vertex_pixels, faces, non_eroded, node_positions, node_indices, edges, weights, distances, clusters,
                           cluster_sizes)
