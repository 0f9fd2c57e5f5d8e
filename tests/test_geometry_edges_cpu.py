"""The CPU oracle's anchor search and mesh warp against float64 on exactly the inputs tests/test_gpu_geometry_edges.py
hands to the kernels (tests/_geometry_edge_util.py), so an error the oracle and the kernels shared could not hide behind
their bit-for-bit agreement. No device is touched."""
import numpy as np
import pytest

import _geometry_edge_util as U

f32 = np.float32

# measured here over every case of the respective test (the oracle's float32 against the float64 restatement); the tests
# assert four times these, the margin of the warp-extension blend errors
MEASURED_WEIGHT_REL = 6.072e-6
MEASURED_WARP_POSITION_ABS = 2.499e-7
MEASURED_WARP_NORMAL_ABS = 1.726e-7
# Per-node coverage weights are squared nearest-node distances, some of them tiny: far slots then weigh less than any
# normal float32, where a relative error means nothing. Slots whose float64 weight is below this are only required to be
# as small in the oracle; with the fixed coverage no slot is.
TINY_WEIGHT = 2.0 ** -100


def _sets_equal(a, b):
    return np.array_equal(np.sort(a, axis=1), np.sort(b, axis=1))


@pytest.mark.parametrize("layout", ["uniform", "near_first", "near_last"])
def test_oracle_anchor_sets_equal_float64_knn(oracle_mod, layout):
    """Random layouts: for every point of every case, with no exclusion, the oracle's K anchors are the float64 K nearest
    nodes as a set (N >= K), and exactly K - N slots are -1 where N < K."""
    cases = [c for c in U.unthresholded_anchor_cases() if c[0] == layout]
    assert cases
    for _, N, V, K in cases:
        points, nodes = U.anchor_case(N, V, 0, layout)
        a, _ = oracle_mod.compute_anchors(points, nodes, K, U.COVERAGE[layout])
        assert _sets_equal(a, U.anchors_f64(points, nodes, K)), (layout, N, V, K)
        assert np.array_equal(U.valid_counts(a), np.full(V, min(N, K))), (layout, N, V, K)


@pytest.mark.parametrize("layout", U.TIE_LAYOUTS)
def test_oracle_tied_distances_are_the_smallest(oracle_mod, layout):
    """Lattice and duplicates: squared distances are exact in float32 and tie, so the index choice is free but the
    multiset of the K chosen squared distances is the K smallest float64 distances. The layouts do tie: some point's
    K-th and (K + 1)-th distances are equal."""
    tied = 0
    for N in U.TIE_N:
        for K in U.TIE_K:
            points, nodes = U.anchor_case(N, U.BATCH_V, 0, layout)
            a, _ = oracle_mod.compute_anchors(points, nodes, K, U.COVERAGE[layout])
            sq = U.squared_distances_f64(points, nodes)
            assert (a >= 0).all()
            assert all(len(set(row)) == K for row in a.tolist()), "a node taken twice"
            chosen = np.sort(np.take_along_axis(sq, a.astype(np.int64), axis=1), axis=1)
            ordered = np.sort(sq, axis=1)
            assert np.array_equal(chosen, ordered[:, :K]), (layout, N, K)
            tied += int((ordered[:, K - 1] == ordered[:, K]).sum())
    assert tied > 0


def test_oracle_weights_against_float64(oracle_mod):
    """Unthresholded weights of every anchor case, fixed coverage and per-node coverage weights, against
    exp(-d^2 / (2 c^2)) normalised in float64 over the oracle's own slots (the duplicates layout with the fixed coverage
    only). Largest relative error over the valid slots, measured here: 6.072e-6 (5.666e-6 with the fixed coverage): the
    float32 squared distance's rounding times the exponent d^2 / (2 c^2), which reaches 60 in these clouds. Bound: four
    times that. Empty slots weigh exactly 0; a row whose weights all vanish in float32 holds exactly 1 / K."""
    worst = 0.0
    for layout, N, V, K in U.unthresholded_anchor_cases():
        points, nodes = U.anchor_case(N, V, 0, layout)
        coverage = U.COVERAGE[layout]
        for node_weights in (None, oracle_mod.node_coverage_weights(nodes, coverage) if N else np.zeros(0, f32)):
            if node_weights is not None and layout == "duplicates":
                continue   # a node's nearest other node is its copy: coverage weight 0, no Gaussian to compare
            a, w = oracle_mod.compute_anchors(points, nodes, K, coverage if node_weights is None else 0.0, node_weights=node_weights)
            ref, scale = U.weights_f64(points, nodes, a, coverage, node_weights, return_scale=True)
            ok = a >= 0
            vanished = scale < 2.0 ** -150       # no weight at all: 1 / K in every slot, exactly
            assert not vanished.any() or N == 0 or node_weights is not None
            assert np.array_equal(w[vanished], np.full((int(vanished.sum()), K), f32(1) / f32(K)))
            assert not ((scale >= 2.0 ** -150) & (scale < TINY_WEIGHT)).any(), "a row summed from subnormal weights: change the seed"
            ok &= ~vanished[:, None]
            assert np.array_equal(w[(a < 0) & ~vanished[:, None]], np.zeros(int(((a < 0) & ~vanished[:, None]).sum()), f32))
            tiny = ok & (ref < TINY_WEIGHT)
            assert (w[tiny] < 2 * TINY_WEIGHT).all()
            assert node_weights is not None or not tiny.any()
            ok &= ~tiny
            if ok.any():
                worst = max(worst, float((np.abs(w[ok] - ref[ok]) / ref[ok]).max()))
    print(f"oracle weights vs float64: largest relative error {worst:.4g}")
    assert worst <= 4 * MEASURED_WEIGHT_REL


def test_oracle_warp_against_float64(oracle_mod):
    """oracle.warp_mesh on every warp case (V, K, invalid share, extrinsics) against the float64 restatement. Measured
    here: positions 2.499e-7 absolute (coordinates within 1.8), normals 1.726e-7; bounds: four times those. A row whose
    slots are all -1 is exactly zero."""
    worst_p = worst_n = 0.0
    for V, K, share, E in U.warp_cases():
        case = U.warp_case(V, U.WARP_N, K, 0, share)
        p, n = oracle_mod.warp_mesh(*case, E)
        p64, n64 = U.warp_f64(*case, E)
        worst_p = max(worst_p, float(np.abs(p - p64).max()))
        worst_n = max(worst_n, float(np.abs(n - n64).max()))
        empty = (case[5] < 0).all(axis=1)
        assert empty.any() == (share > 0)
        assert not p[empty].any() and not n[empty].any()
    print(f"oracle warp vs float64: positions {worst_p:.4g}, normals {worst_n:.4g}")
    assert worst_p <= 4 * MEASURED_WARP_POSITION_ABS
    assert worst_n <= 4 * MEASURED_WARP_NORMAL_ABS


def test_warp_case_rows():
    """The builder's promises: indices in [-1, N - 1], the all-invalid row and the slot-0-only row, weights summing to one
    over the valid slots, rotations orthonormal within |w| <= 0.3, translations within 0.05."""
    for V, K in ((1, 4), (63, 1), (65, 3), (257, 8)):
        p, n, g, R, t, a, w = U.warp_case(V, U.WARP_N, K, 0, 0.3)
        assert a.dtype == np.int32 and a.min() >= -1 and a.max() <= U.WARP_N - 1
        assert (a[V // 2] == -1).all()
        if V >= 2:
            assert a[V // 2 + 1, 0] >= 0 and (a[V // 2 + 1, 1:] == -1).all()
        valid = a >= 0
        sums = np.where(valid, w, 0).sum(axis=1)
        assert np.allclose(sums[valid.any(axis=1)], 1.0, atol=1e-6) and (w[valid] > 0).all()
        assert np.isin(w[~valid], [np.inf, 7.5]).all()
        assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
        angle = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1))
        assert angle.max() <= 0.3 + 1e-3 and np.abs(t).max() <= 0.05
        a0 = U.warp_case(V, U.WARP_N, K, 0, 0.0)[5]
        assert a0.min() >= 0 and a0.max() <= U.WARP_N - 1


def test_threshold_populations(oracle_mod):
    """At each K's coverage some points keep no slot, some 1..K-1 and some all K, fixed and per-node coverage alike."""
    points, nodes = U.anchor_case(U.THRESHOLD_N, U.THRESHOLD_V, 0, "uniform")
    for K, coverage in U.THRESHOLD_COVERAGE.items():
        for node_weights in (None, oracle_mod.node_coverage_weights(nodes, coverage)):
            a, _ = oracle_mod.compute_anchors(points, nodes, K, coverage if node_weights is None else 0.0, node_weights=node_weights,
                                              minimum_valid_anchor_count=1)
            n = U.valid_counts(a)
            assert (n == 0).any() and ((n > 0) & (n < K)).any() and (n == K).any()


# ---- hand-derived rows ----------------------------------------------------------------------------------------------------
TWO_NODES = np.array([[0.25, 0, 0], [-0.25, 0, 0]], f32)   # both 0.25 from the origin: d^2 = 0.0625 exactly
ORIGIN = np.zeros((1, 3), f32)


def test_fewer_nodes_than_slots_unthresholded(oracle_mod):
    a, w = oracle_mod.compute_anchors(ORIGIN, TWO_NODES, 4, 0.25)
    assert a.tolist() == [[0, 1, -1, -1]]
    assert w.tolist() == [[0.5, 0.5, 0.0, 0.0]]   # exp(-inf) = 0 in the empty slots, two equal weights


def test_minimum_valid_above_valid_leaves_weights_unnormalised(oracle_mod):
    """c = d = 0.25: each of the two nodes weighs exp(-0.0625 / (2 * 0.0625)) = exp(-1/2); with three required and two
    valid the row is not normalised, and the empty slots keep the squared distance inf the search left there."""
    a, w = oracle_mod.compute_anchors(ORIGIN, TWO_NODES, 4, 0.25, minimum_valid_anchor_count=3)
    e = f32(np.exp(-0.5))
    assert a.tolist() == [[0, 1, -1, -1]]
    assert w.tolist() == [[e, e, np.inf, np.inf]]
    a, w = oracle_mod.compute_anchors(ORIGIN, TWO_NODES, 4, 0.25, minimum_valid_anchor_count=2)   # two suffice: normalised
    assert a.tolist() == [[0, 1, -1, -1]] and w.tolist() == [[0.5, 0.5, np.inf, np.inf]]
    a, w = oracle_mod.compute_anchors(ORIGIN, TWO_NODES, 4, 0.1, minimum_valid_anchor_count=1)    # 0.0625 > 4 * 0.01: none kept
    assert a.tolist() == [[-1, -1, -1, -1]] and w.tolist() == [[f32(0.0625), f32(0.0625), np.inf, np.inf]]


def test_non_finite_point_has_no_anchor(oracle_mod):
    for bad in (np.nan, np.inf, -np.inf):
        points = np.array([[0.1, bad, 0.0], [0.0, 0.0, 0.0]], f32)
        a, w = oracle_mod.compute_anchors(points, TWO_NODES, 2, 0.25)
        assert a.tolist() == [[-1, -1], [0, 1]]
        assert w.tolist() == [[0.5, 0.5], [0.5, 0.5]]   # no slot, sum 0: 1 / K
    assert U.anchors_f64(np.array([[np.nan, 0, 0]], f32), TWO_NODES, 2).tolist() == [[-1, -1]]


def test_no_nodes(oracle_mod):
    a, w = oracle_mod.compute_anchors(ORIGIN, np.zeros((0, 3), f32), 4, 0.25)
    assert a.tolist() == [[-1, -1, -1, -1]] and w.tolist() == [[0.25, 0.25, 0.25, 0.25]]
    a, w = oracle_mod.compute_anchors(ORIGIN, np.zeros((0, 3), f32), 4, 0.25, minimum_valid_anchor_count=1)
    assert a.tolist() == [[-1, -1, -1, -1]] and np.isposinf(w).all()


def test_float64_knn_restatement():
    """anchors_f64 on a case small enough to read: ascending (distance, index), -1 past the node count."""
    nodes = np.array([[3, 0, 0], [1, 0, 0], [-1, 0, 0], [2, 0, 0]], f32)
    assert U.anchors_f64(ORIGIN, nodes, 3).tolist() == [[1, 2, 3]]
    assert U.anchors_f64(ORIGIN, nodes, 6).tolist() == [[1, 2, 3, 0, -1, -1]]
    assert U.anchors_f64(ORIGIN, nodes[:0], 2).tolist() == [[-1, -1]]
