"""Mirror of the reference's legacy graph_proc bindings at the top level of `nnrt` (cpp/pybind/nnrt_pybind.cpp:121-126 ->
cpp/cpu/graph_proc.cpp:27-155), computed on the GPU (csrc/graph_sampling.hip): the vertex erosion mask of a mesh and the
greedy node sampling that picks a motion graph's nodes from its vertices. Both accept numpy arrays or device tensors and
return device tensors; both return exactly what the reference's sequential loops return.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native as N
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
