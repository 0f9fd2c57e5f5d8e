"""Shortest-path anchors, the parts that need no GPU: the mirror's signatures against the reference's, the CPU restatement
(tests/_anchor_sp_util.py) on the reference's own known-answer case, the fusion loop's refusals and its edge re-indexing."""
import json
import os

import numpy as np
import pytest

import _anchor_sp_util as U
from test_mirror_signatures import GOLDEN, _matches, _signatures

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_shortest_path_kat.npz")
NAMES = ("compute_anchors_and_weights_shortest_path_fixed_node_weight", "compute_anchors_and_weights_shortest_path_variable_node_weight")


@pytest.mark.parametrize("name", NAMES)
def test_mirror_signature_matches_reference(name):
    import dynamicfuion_python_amd.nnrt as nn
    with open(GOLDEN) as f:
        rows = [r for r in json.load(f) if r["module"] == "nnrt.geometry.functional" and r["name"] == name]
    assert len(rows) == 1 and rows[0]["args"]
    fn = getattr(nn.geometry.functional, name, None)
    assert fn is not None, f"nnrt.geometry.functional.{name} is missing from the mirror"
    assert any(_matches(p, rows[0]["args"]) for p in _signatures(fn, True)), rows[0]["args"]


def test_restatement_reproduces_the_reference_known_answer():
    """tests/test_compute_anchors.py:57-146 of the reference: 11 nodes in three components, 2 points, D = 4 with -1 padding,
    K = 8, coverage 1; two restarts per point."""
    k = np.load(KAT)
    assert k["nodes"].shape == (11, 3) and k["edges"].shape == (11, 4) and k["points"].shape == (2, 3)
    a, w, popped, dropped, ties = U.shortest_path_anchors(k["points"], k["nodes"], k["edges"], 8, coverage=1.0)
    assert U.keys_distinct(popped) and not ties.any() and not dropped.any()
    assert np.array_equal(a, k["anchors"])
    assert np.array_equal(k["anchors"], [[4, 3, 2, 1, 0, 5, 6, 9], [9, 8, 7, 10, 1, 2, 3, 4]])
    assert np.allclose(w, k["weights"])
    assert np.allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-6)


def test_restatement_queue_rules():
    """Drop-when-full, the index tie rule, unfilled slots and empty inputs, on hand-made graphs."""
    # a star: node 0 joined to 44 leaves, all at distance 1 from it -> the first expansion inserts 44 entries into a queue
    # that holds 40; equal keys pop the lower index first
    ang = np.linspace(0, 2 * np.pi, 44, endpoint=False)
    nodes = np.concatenate([[[0, 0, 0]], np.stack([np.cos(ang), np.sin(ang), np.zeros(44)], axis=1)]).astype(np.float32)
    nodes[1:] /= np.linalg.norm(nodes[1:], axis=1, keepdims=True).astype(np.float32)
    edges = np.full((45, 44), -1, np.int32)
    edges[0] = np.arange(1, 45)
    a, w, popped, dropped, ties = U.shortest_path_anchors(np.array([[0, 0, 0.5]], np.float32), nodes, edges, 3, coverage=1.0)
    assert a[0, 0] == 0 and dropped[0] == 4 and len(popped[0]) == 3
    # fewer reachable nodes than K: unfilled slots are -1 with weight 0
    a, w, _, _, _ = U.shortest_path_anchors(np.zeros((1, 3), np.float32), nodes[:3], np.full((3, 1), -1, np.int32), 4, coverage=1.0)
    assert sorted(a[0, :3]) == [0, 1, 2] and a[0, 3] == -1 and w[0, 3] == 0 and abs(w[0].sum() - 1) < 1e-6
    # no node at all: -1 everywhere, weights 1 / K
    a, w, _, _, _ = U.shortest_path_anchors(np.zeros((2, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 2), np.int32), 4, coverage=1.0)
    assert (a == -1).all() and (w == 0.25).all()
    # two nodes at equal distance from the seed: the lower index pops first, and the restatement reports the tie
    nodes = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float32)
    edges = np.array([[2, 1], [0, -1], [0, -1]], np.int32)
    a, _, popped, _, ties = U.shortest_path_anchors(np.array([[0, 0.25, 0]], np.float32), nodes, edges, 2, coverage=1.0)
    assert a.tolist() == [[0, 1]] and ties[0] == 1


@pytest.mark.parametrize("mode", ["FIRST_FRAME_EXTRACTED_MESH", "PROVIDED_NODES"])
def test_pipeline_refuses_shortest_path_without_edge_rows(mode):
    from dynamicfuion_python_amd import fusion as F
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode[mode],
                                anchor_computation_mode=F.AnchorComputationMode.SHORTEST_PATH)
    with pytest.raises(NotImplementedError, match="SHORTEST_PATH"):
        F.FusionPipeline(None, params, nodes=np.zeros((8, 3), np.float32))   # refused before the sequence or a device is touched
    assert F.FusionParameters().anchor_computation_mode == F.AnchorComputationMode.EUCLIDEAN


def test_edge_rows_follow_a_node_permutation():
    from dynamicfuion_python_amd.fusion.pipeline import remap_edges_to_node_order
    edges = np.array([[1, 2, -1], [0, -1, -1], [0, 3, -1], [2, -1, -1]], np.int32)
    order = np.array([2, 0, 3, 1])   # new node v is old node order[v]
    got = remap_edges_to_node_order(edges, order)
    assert got.dtype == np.int32 and got.shape == edges.shape
    # old 2 -> new 0, old 0 -> new 1, old 3 -> new 2, old 1 -> new 3
    assert got.tolist() == [[1, 2, -1], [3, 0, -1], [0, -1, -1], [1, -1, -1]]
    # the same graph: (new v, new t) is an edge iff (order[v], order[t]) was one
    old = {(i, int(t)) for i in range(4) for t in edges[i] if t >= 0}
    new = {(int(order[v]), int(order[t])) for v in range(4) for t in got[v] if t >= 0}
    assert old == new
    assert np.array_equal(remap_edges_to_node_order(edges, np.arange(4)), edges)
    with pytest.raises(ValueError):
        remap_edges_to_node_order(edges, np.array([0, 0, 1, 2]))
    with pytest.raises(ValueError):
        remap_edges_to_node_order(np.array([[4], [0], [0], [0]], np.int32), order)
