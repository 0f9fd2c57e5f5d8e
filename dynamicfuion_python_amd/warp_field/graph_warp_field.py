"""Motion graph from a mesh (reference warp_field/graph_warp_field.py:24-42): erode the mesh's border vertices, sample the
graph nodes greedily from the remaining vertices, build the warp field over them -- all on the GPU
(csrc/graph_sampling.hip, csrc/hierarchy.hip).
"""
from __future__ import annotations

from typing import Optional, Tuple

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
