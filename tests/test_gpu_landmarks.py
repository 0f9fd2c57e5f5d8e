"""GPU tests of the fitter's landmark term (nnrt_fitter_set_landmarks) against the restatement of
tests/_landmark_util.py (validated in tests/test_landmarks_cpu.py). Scene S1 (96 x 128, 24 nodes) or smaller: the smallest
where a vertex has several anchor nodes, a node run crosses a group pass and a wave, and a pair run exists."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _landmark_util as LU   # noqa: E402
from _coupled_util import apply_update, coupled_system, data_system, identity_motion, solve_dense   # noqa: E402
from _util import scene_target   # noqa: E402

pytestmark = pytest.mark.gpu

LM = 0.001
F32 = np.float32


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd import _native
    _native.lib()
    from dynamicfuion_python_amd import nnrt
    return nnrt


@pytest.fixture(scope="module")
def scenes(oracle_mod):
    from dynamicfuion_python_amd import synthetic as S
    oracle_mod.set_fused_jacobians(False)
    s1 = S.make_scene("S1")
    arap = S.make_scene("S1_ARAP", hierarchy_builder=lambda n, c, l: oracle_mod.build_hierarchy(n, c, l))
    # a flat patch facing the camera at z = 1.2 (normals towards it), S1's nodes put on it
    pts = s1.points.copy()
    pts[:, 2] = 1.2
    nrm = np.tile(np.array([0.0, 0.0, -1.0], F32), (len(pts), 1))
    nodes = s1.nodes.copy()
    nodes[:, 2] = 1.2
    flat = dataclasses.replace(s1, name="flat", points=pts, normals=nrm, nodes=nodes)
    return dict(S1=(s1, scene_target(oracle_mod, s1)), S1_ARAP=(arap, scene_target(oracle_mod, arap)), flat=(flat, None))


def _fitter(nn, sc, coupled=False, anchor_count=4, graph=0, lm=LM, iterations=1, thresholded=False, **kw):
    """thresholded: a field that thresholds anchors by distance (coverage 0.12, at least two valid anchors), under which S1's
    vertices keep one to four slots and the others hold -1 (tests/test_gpu_geometry_edges.py's field)."""
    G, A = nn.geometry, nn.alignment
    if thresholded:
        wf = G.HierarchicalGraphWarpField(sc.nodes, 0.12, True, anchor_count, 2, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                          sc.layer_count)
    else:
        wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, anchor_count, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                          sc.layer_count)
    ft = A.DeformableMeshToImageFitter(iterations, [A.IterationMode.ALL], preconditioning_dampening_factor=lm, use_hip_graph=graph, **kw)
    ft.set_data_coupling(A.DataCoupling.COUPLED if coupled else A.DataCoupling.BLOCK_DIAGONAL)
    return wf, ft


def _mesh(nn, sc):
    return nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces)


def _motion(wf):
    return wf.get_node_rotations(True), wf.get_node_translations(True)


def _start(sc, wf, fraction=0.5):
    R0, t0 = sc.partial_motion(fraction)
    wf.set_node_rotations(R0)
    wf.set_node_translations(t0)
    return _motion(wf)


def _landmarks(sc, count, seed=5, spread=0.02):
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(sc.points), count, replace=False).astype(np.int32)
    targets = (sc.points[idx] + rng.normal(0, spread, (count, 3))).astype(F32)
    return idx, targets, rng.uniform(0.5, 2.0, count).astype(F32)


def _term(sc, ft, R, t, idx, targets, s, K=4, dtype=F32, E=None, **kw):
    a, w = ft.anchors(len(sc.points), K)
    return LU.landmark_term(sc.points, sc.nodes, R, t, a, w, idx, targets, s, dtype=dtype, extrinsics=E, **kw), a


def _exported(ft, N, coupled):
    """(H [N,6,6] without the damping, g [N,6], {pair: block}) of the last iteration."""
    if coupled:
        diag, pairs, blocks, rhs = ft.coupled_system()
        return diag - LM * np.eye(6, dtype=F32), rhs.reshape(N, 6), {tuple(p): b for p, b in zip(pairs.tolist(), blocks)}
    dg = ft.diagnostics()
    return dg["hessian"].reshape(N, 6, 6), dg["gradient"].reshape(N, 6), {}


def _run_term_alone(nn, sc, depth, coupled, idx, targets, s, K=4, thresholded=False, E=None, **kw):
    # (a node no landmark reaches solves to a zero update: the guard keeps its rotation)
    wf, ft = _fitter(nn, sc, coupled=coupled, anchor_count=K, guard_zero_rotation=True, thresholded=thresholded)
    R, t = _start(sc, wf)
    ft.set_landmarks(idx, targets, s, **kw)
    ft.prepare(wf, _mesh(nn, sc), depth, np.zeros(depth.shape, np.uint8), sc.K, E, 1.0)   # empty reference mask: no data term
    ft.iterate(wf, 0, 1)
    ft.check()
    return wf, ft, R, t


def _check_term(ft, want, N, coupled, label):
    H, g, blocks = _exported(ft, N, coupled)
    scale = np.abs(want["H"]).max()
    eH, eg = np.abs(H - want["H"]).max() / scale, np.abs(g - want["g"]).max() / scale
    eb = 0.0
    for ij, b in blocks.items():
        eb = max(eb, np.abs(b - want["pairs"].get(ij, np.zeros((6, 6)))).max() / scale)
    print(f"{label}: H {eH:.2g}, g {eg:.2g}, pair blocks {eb:.2g} of max |H| = {scale:.3g} (bar 1e-6)")
    assert scale > 0 and max(eH, eg, eb) < 1e-6
    if coupled:
        assert set(want["pairs"]) <= set(blocks), "a landmark pair outside the frame's pair list"
        assert all(np.abs(blocks[ij]).max() > 0 for ij in want["pairs"])


# ---- 1. the term alone ----------------------------------------------------------------------------------------------------
def _extrinsics():
    """A world -> camera matrix that is not the identity: 0.1 rad about (1, 2, 0.5) and a few centimetres."""
    E = np.eye(4)
    E[:3, :3] = LU._rodrigues(0.1 * np.array([1.0, 2.0, 0.5]) / np.linalg.norm([1.0, 2.0, 0.5]))
    E[:3, 3] = [0.02, -0.03, 0.04]
    return E


@pytest.mark.parametrize("extrinsics", [False, True])
@pytest.mark.parametrize("coupled", [False, True])
def test_term_alone(nn, scenes, coupled, extrinsics):
    """extrinsics: d comes from the warped vertex in camera space, J from the vertex as stored, as for the data term."""
    sc, depth = scenes["S1"]
    idx, targets, s = _landmarks(sc, 7)
    E = _extrinsics() if extrinsics else None
    if extrinsics:
        targets = (targets.astype(np.float64) @ E[:3, :3].T + E[:3, 3]).astype(F32)
    wf, ft, R, t = _run_term_alone(nn, sc, depth, coupled, idx, targets, s, term_weight=1.5, E=E)
    want, a = _term(sc, ft, R, t, idx, targets, s, term_weight=1.5, E=E)
    _check_term(ft, want, len(sc.nodes), coupled, f"7 landmarks alone, {'coupled' if coupled else 'block-diagonal'}{', extrinsics' if extrinsics else ''}")
    if extrinsics:   # the restatement without E is another system: the case does depend on them
        other, _ = _term(sc, ft, R, t, idx, targets, s, term_weight=1.5)
        assert np.abs(other["g"] - want["g"]).max() > 1e-3 * np.abs(want["H"]).max()
    d, active = ft.landmark_distances()
    assert active.all() and np.abs(d - want["d"]).max() < 1e-6
    info = ft.landmark_info()
    assoc = int((a[idx] >= 0).sum())
    assert info["count"] == 7 and info["associations"] == assoc and info["node_runs"] == len(np.unique(a[idx][a[idx] >= 0]))
    assert (info["pair_associations"] > 0) == coupled


# ---- 2. additivity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupled", [False, True])
def test_additivity(nn, scenes, coupled):
    sc, depth = scenes["S1"]
    N = len(sc.nodes)
    idx, targets, s = _landmarks(sc, 7)
    out = {}
    for which in ("data", "landmarks", "both"):
        wf, ft = _fitter(nn, sc, coupled=coupled)
        _start(sc, wf)
        if which != "data":
            ft.set_landmarks(idx, targets, s)
        mask = np.zeros(depth.shape, np.uint8) if which == "landmarks" else None
        ft.prepare(wf, _mesh(nn, sc), depth, mask, sc.K, None, 1.0)
        ft.iterate(wf, 0, 1)
        ft.check()
        out[which] = _exported(ft, N, coupled)
    scale = np.abs(out["both"][0]).max()
    eH = np.abs(out["both"][0] - (out["data"][0] + out["landmarks"][0])).max() / scale
    eg = np.abs(out["both"][1] - (out["data"][1] + out["landmarks"][1])).max() / scale
    eb = max([np.abs(out["both"][2][ij] - (out["data"][2][ij] + out["landmarks"][2][ij])).max() / scale for ij in out["both"][2]] + [0.0])
    print(f"data + landmarks against the two alone ({'coupled' if coupled else 'block-diagonal'}): H {eH:.2g}, g {eg:.2g}, pairs {eb:.2g}")
    assert max(eH, eg, eb) < 1e-6
    assert np.abs(out["landmarks"][0]).max() > 0 and np.abs(out["data"][0]).max() > 0


# ---- 3. shapes that can go wrong ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one", "run_of_65", "twice_on_a_vertex", "eight_anchors", "empty_slots"])
@pytest.mark.parametrize("coupled", [False, True])
def test_shapes(nn, scenes, shape, coupled):
    sc, depth = scenes["S1"]
    K, thresholded = 4, False
    rng = np.random.default_rng(11)
    if shape == "one":
        idx = np.array([len(sc.points) // 2 + 7], np.int32)
    elif shape == "run_of_65":
        # 65 vertices anchored to one node: its run crosses a group pass (8) and a wave (64)
        wf0, ft0 = _fitter(nn, sc)
        ft0.prepare(wf0, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        a0, _ = ft0.anchors(len(sc.points), K)
        node = int(np.bincount(a0[a0 >= 0]).argmax())
        idx = np.nonzero((a0 == node).any(axis=1))[0][:65].astype(np.int32)
        assert len(idx) == 65
    elif shape == "twice_on_a_vertex":
        idx = np.array([100, 731, 100], np.int32)
    elif shape == "empty_slots":
        # -1 anchor slots: three vertices each with one, two and three empty slots, and two with none. The sorted lists are
        # then shorter than L K (keys that sort last and end no run), and a vertex has fewer than K (K - 1) / 2 pairs.
        thresholded = True
        a0, _ = _anchors_of(nn, sc, depth, thresholded=True)
        empty = (a0 < 0).sum(axis=1)
        rows = {e: np.nonzero(empty == e)[0] for e in (1, 2, 3, 0)}
        assert all(len(r) >= 3 for r in rows.values())
        idx = np.concatenate([rows[e][np.linspace(0, len(rows[e]) - 1, 3 if e else 2).astype(int)] for e in (1, 2, 3, 0)]).astype(np.int32)
    else:
        # 8 anchor slots on the fewest nodes a warp field takes with them (anchor_count <= node_count)
        K = 8
        keep = np.array([0, 2, 5, 9, 12, 14, 18, 23])
        sc = dataclasses.replace(sc, nodes=sc.nodes[keep], gt_rotations=sc.gt_rotations[keep], gt_translations=sc.gt_translations[keep],
                                 gt_axis_angles=sc.gt_axis_angles[keep])
        idx = rng.choice(len(sc.points), 9, replace=False).astype(np.int32)
    targets = (sc.points[idx] + rng.normal(0, 0.02, (len(idx), 3))).astype(F32)
    s = rng.uniform(0.5, 2.0, len(idx)).astype(F32)
    wf, ft, R, t = _run_term_alone(nn, sc, depth, coupled, idx, targets, s, K=K, thresholded=thresholded)
    want, a = _term(sc, ft, R, t, idx, targets, s, K=K)
    if shape == "empty_slots":
        assert (a[idx] < 0).any() and set((a[idx] < 0).sum(axis=1).tolist()) == {0, 1, 2, 3}
        info = ft.landmark_info()
        assert info["associations"] == int((a[idx] >= 0).sum()) < len(idx) * K
        if coupled:
            valid = (a[idx] >= 0).sum(axis=1)
            assert info["pair_associations"] == int((valid * (valid - 1) // 2).sum()) < len(idx) * K * (K - 1) // 2
    if shape == "run_of_65":
        assert max(np.bincount(a[idx][a[idx] >= 0])) == 65
    if shape == "eight_anchors":
        print(f"eight anchors: {int((a[idx] < 0).sum())} empty slots among the landmarks' {a[idx].size}")
    _check_term(ft, want, len(sc.nodes), coupled, f"{shape}, {'coupled' if coupled else 'block-diagonal'}")
    assert ft.landmark_info()["associations"] == int((a[idx] >= 0).sum())


def test_gate_and_cost(nn, scenes):
    """A zero weight, a NaN target and a cutoff-dropped landmark among 7: each inactive, the rest summed as without them,
    and the cost (step control's record of the first iteration; the reference mask is empty) as the term states it."""
    A = nn.alignment
    sc, depth = scenes["S1"]
    idx, targets, s = _landmarks(sc, 7)
    wf, ft = _fitter(nn, sc, guard_zero_rotation=True)
    ft.set_step_control(A.StepControl())
    R, t = _start(sc, wf)
    probe = LU.landmark_term(sc.points, sc.nodes, R, t, *_anchors_of(nn, sc, depth), idx, targets, s, term_weight=2.0)
    dist = np.linalg.norm(probe["d"].astype(np.float64), axis=1)
    order = np.argsort(dist)
    far, cutoff = int(order[-1]), float(dist[order[-2]] + dist[order[-1]]) / 2
    off, nan = int(order[0]), int(order[1])
    s = s.copy()
    s[off] = 0.0
    targets = targets.copy()
    targets[nan, 2] = np.nan
    ft.set_landmarks(idx, targets, s, term_weight=2.0, cutoff=cutoff)
    ft.prepare(wf, _mesh(nn, sc), depth, np.zeros(depth.shape, np.uint8), sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    want, _ = _term(sc, ft, R, t, idx, targets, s, term_weight=2.0, cutoff=cutoff)
    d, active = ft.landmark_distances()
    expect = np.ones(7, bool)
    expect[[far, off, nan]] = False
    assert np.array_equal(active, expect) and np.array_equal(want["active"], expect) and want["dropped"][far]
    _check_term(ft, want, len(sc.nodes), False, "zero weight + NaN target + beyond the cutoff")
    cost = ft.step_history()[0].cost
    by_hand = sum(float(((2.0 * float(s[l]) * want["d"][l].astype(np.float64)) ** 2).sum()) for l in np.nonzero(expect)[0])
    by_hand += (2.0 * float(s[far]) * cutoff) ** 2
    print(f"cost {cost:.9g}; restatement {want['cost']:.9g}; by hand {by_hand:.9g}")
    assert abs(cost - want["cost"]) <= 1e-6 * want["cost"] and abs(cost - by_hand) <= 1e-5 * by_hand


def _anchors_of(nn, sc, depth, K=4, thresholded=False):
    wf, ft = _fitter(nn, sc, anchor_count=K, thresholded=thresholded)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    return ft.anchors(len(sc.points), K)


# ---- 4. what the depth term cannot see ------------------------------------------------------------------------------------------
def _gn_loop(O, sc, depth, a, w, idx, targets, iterations, tukey_c=None, landmarks=True):
    """The float64 restatement's Gauss-Newton loop: the coupled system of tests/_coupled_util.py plus the landmark term."""
    N = len(sc.nodes)
    R, t = identity_motion(N)
    for _ in range(iterations):
        sysm = coupled_system(O, sc, depth, R, t, lm=LM, tukey_c=tukey_c)
        if landmarks:
            sysm = LU.add_to_system(sysm, LU.landmark_term(sc.points, sc.nodes, R, t, a, w, idx, targets, None, dtype=np.float64))
        x, _ = solve_dense(sysm["diag"], sysm["pairs"], sysm["blocks"], sysm["rhs"])
        R, t = apply_update(R, t, x)
    return R, t


@pytest.mark.parametrize("case", ["slide", "beyond_the_cutoff"])
def test_what_the_depth_term_cannot_see(nn, oracle_mod, scenes, case):
    """A flat patch moved 3 cm in its own plane (the depth term's null space), or 5 cm along its normal under IRLS Tukey at
    0.01 (every pixel beyond the cutoff): the depth-only coupled fit leaves the node translations at 0, one landmark per
    node recovers the motion as the float64 restatement's loop does."""
    A = nn.alignment
    flat, _ = scenes["flat"]
    N = len(flat.nodes)
    move = np.array([0.03, 0.0, 0.0], F32) if case == "slide" else np.array([0.0, 0.0, 0.05], F32)
    gt_t = np.tile(move, (N, 1))
    sc = dataclasses.replace(flat, gt_rotations=identity_motion(N)[0], gt_translations=gt_t)
    depth = scene_target(oracle_mod, sc)
    kw, tukey_c = dict(guard_zero_rotation=True), None   # (a depth-only fit that sees nothing solves to a zero update)
    if case == "beyond_the_cutoff":
        tukey_c = 0.01
        kw.update(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=tukey_c, penalty_form=A.PenaltyForm.IRLS)
    iterations = 4
    # one landmark per node: the vertex nearest to it, the target where the motion takes it
    idx = np.array([int(np.argmin(np.linalg.norm(sc.points - g, axis=1))) for g in sc.nodes], np.int32)
    targets = (sc.points[idx] + move).astype(F32)
    out = {}
    for with_landmarks in (False, True):
        wf, ft = _fitter(nn, sc, coupled=True, iterations=iterations, **kw)
        if with_landmarks:
            ft.set_landmarks(idx, targets)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, iterations)
        ft.check()
        out[with_landmarks] = (_motion(wf)[1], ft.anchors(len(sc.points), 4))
    t_depth, t_lm = out[False][0], out[True][0]
    a, w = out[True][1]
    _, t_ref = _gn_loop(oracle_mod, sc, depth, a, w, idx, targets, iterations, tukey_c)
    along = move / np.linalg.norm(move)
    print(f"{case}: depth only max |t . move| {np.abs(t_depth @ along).max():.3g}; with landmarks mean t . move {float((t_lm @ along).mean()):.4g} "
          f"of {np.linalg.norm(move):.3g}; against the restatement's loop {np.abs(t_lm - t_ref).max():.3g}")
    assert np.abs(t_depth @ along).max() < 1e-4
    assert np.abs(t_lm - t_ref).max() < 1e-4
    assert float((t_lm @ along).mean()) > 0.8 * float(np.linalg.norm(move))


# ---- 5. step control, both objectives -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["SQUARE", "ROBUST"])
def test_step_control_costs(nn, oracle_mod, scenes, objective):
    A = nn.alignment
    sc, depth = scenes["S1"]
    idx, targets, s = _landmarks(sc, 7)
    iterations = 4
    wf, ft = _fitter(nn, sc, coupled=True, iterations=iterations, step_objective=A.StepObjective[objective])
    ft.set_step_control(A.StepControl())
    ft.set_landmarks(idx, targets, s, term_weight=3.0)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    a, w = ft.anchors(len(sc.points), 4)
    want = []
    for k in range(iterations):
        R, t = _motion(wf)   # the state iteration k starts from
        data = data_system(oracle_mod, sc, depth, R, t)["cost"]
        term = LU.landmark_term(sc.points, sc.nodes, R, t, a, w, idx, targets, s, term_weight=3.0)["cost"]
        want.append((data, term))
        ft.iterate(wf, k, 1)
    ft.check()
    costs = [r.cost for r in ft.step_history()]
    assert len(costs) == iterations
    for k, (c, (data, term)) in enumerate(zip(costs, want)):
        print(f"{objective} iteration {k}: cost {c:.9g} = data {data:.9g} + landmarks {term:.9g} ({abs(c - (data + term)) / (data + term):.2g})")
        assert term > 0 and abs(c - (data + term)) <= 1e-6 * (data + term)
    assert costs[-1] <= costs[0]


# ---- 6. graphs ------------------------------------------------------------------------------------------------------------------
def _fit(nn, sc, depth, graph, idx, targets, s, wf_ft=None, iterations=3, coupled=True):
    wf, ft = wf_ft or _fitter(nn, sc, coupled=coupled, graph=graph, iterations=iterations)
    I, z = identity_motion(len(sc.nodes))
    wf.set_node_rotations(I)
    wf.set_node_translations(z)
    if idx is not None:
        ft.set_landmarks(idx, targets, s)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, iterations)
    ft.check()
    return (wf, ft), _motion(wf), ft.diagnostics()


def _same(x, y):
    return np.array_equal(x[1][0], y[1][0]) and np.array_equal(x[1][1], y[1][1]) and all(
        np.array_equal(x[2][k], y[2][k], equal_nan=True) for k in x[2])


def test_graphs(nn, scenes):
    sc, depth = scenes["S1"]
    idx, targets, s = _landmarks(sc, 7)
    _, targets2, _ = _landmarks(sc, 7, spread=0.03)
    eager = _fit(nn, sc, depth, 0, idx, targets, s)
    graphed = _fit(nn, sc, depth, 2, idx, targets, s)
    assert graphed[0][1].graph_count == 1
    assert _same(eager, graphed), "eager and graph replay differ"
    assert _same(eager, _fit(nn, sc, depth, 0, idx, targets, s)), "two identical runs differ"
    # new targets, the same count: the captured graph stays, and the result is a fresh fitter's
    again = _fit(nn, sc, depth, 2, idx, targets2, s, wf_ft=graphed[0])
    assert again[0][1].graph_count == 1
    assert _same(again, _fit(nn, sc, depth, 2, idx, targets2, s))
    assert not np.array_equal(again[1][1], graphed[1][1])
    # a new count re-captures
    ft = graphed[0][1]
    ft.set_landmarks(idx[:5], targets[:5], s[:5])
    assert ft.graph_count == 0
    fewer = _fit(nn, sc, depth, 2, idx[:5], targets[:5], s[:5], wf_ft=graphed[0])
    assert fewer[0][1].graph_count == 1
    assert _same(fewer, _fit(nn, sc, depth, 0, idx[:5], targets[:5], s[:5]))


# ---- 7. off is off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,coupled", [("S1", False), ("S1_ARAP", False), ("S1", True)])
def test_off_is_off(nn, scenes, name, coupled):
    sc, depth = scenes[name]
    idx, targets, s = _landmarks(sc, 7)
    never = _fit(nn, sc, depth, 2, None, None, None, iterations=2, coupled=coupled)
    wf, ft = _fitter(nn, sc, coupled=coupled, graph=2, iterations=2)
    had = _fit(nn, sc, depth, 2, idx, targets, s, wf_ft=(wf, ft), iterations=2)
    assert not _same(never, had)
    ft.clear_landmarks()
    assert ft.landmark_info()["count"] == 0 and ft.graph_count == 0
    cleared = _fit(nn, sc, depth, 2, None, None, None, wf_ft=(wf, ft), iterations=2)
    assert _same(never, cleared)
    assert cleared[0][1].graph_count == never[0][1].graph_count and cleared[0][1].launch_plan() == never[0][1].launch_plan()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(nn, scenes):
    A = nn.alignment
    sc, depth = scenes["S1"]
    V = len(sc.points)
    idx, targets, s = _landmarks(sc, 7)
    for bad in (V, -1):
        wf, ft = _fitter(nn, sc)
        bad_idx = idx.copy()
        bad_idx[4] = bad
        ft.set_landmarks(bad_idx, targets, s)
        with pytest.raises(RuntimeError, match="landmark 4: vertex index outside"):
            ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        with pytest.raises(RuntimeError, match="prepare"):
            ft.iterate(wf, 0, 1)
    # a vertex no face references: one more vertex appended to the mesh
    lone = dataclasses.replace(sc, points=np.concatenate([sc.points, sc.points[:1] + F32(0.001)]), normals=np.concatenate([sc.normals, sc.normals[:1]]))
    wf, ft = _fitter(nn, lone)
    lone_idx = idx.copy()
    lone_idx[2] = V
    ft.set_landmarks(lone_idx, targets, s)
    with pytest.raises(RuntimeError, match="landmark 2: its vertex belongs to no face"):
        ft.prepare(wf, _mesh(nn, lone), depth, None, sc.K, None, 1.0)
    ft.set_landmarks(idx, targets, s)   # the same fitter takes a good set afterwards
    ft.prepare(wf, _mesh(nn, lone), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    # a count mismatch on read-back is refused, not written past
    from dynamicfuion_python_amd import _native as N
    out = np.full((9, 4), -1.0, F32)
    for count in (6, 8, 9):
        assert N.lib().nnrt_fitter_get_landmark_distances(ft._h, N.ptr(out), count, N.stream_ptr(None)) == 1
        assert b"count differs" in N.lib().nnrt_last_error()
    assert (out == -1).all()
    # another mode than ALL in the fitter's list
    ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL, A.IterationMode.TRANSLATION_ONLY])
    with pytest.raises(RuntimeError, match="IterationMode ALL only"):
        ft.set_landmarks(idx, targets, s)
    ft.clear_landmarks()
    with pytest.raises(RuntimeError, match="term_weight"):
        _fitter(nn, sc)[1].set_landmarks(idx, targets, s, term_weight=0.0)


# ---- 9. pipeline ----------------------------------------------------------------------------------------------------------------
PH, PW, PFX, STEP = 96, 128, 116.0, 0.01   # S1's camera; the plate slides STEP metres per frame


def _write_sliding_plate(directory, frames=3):
    """A flat plate at z = 1.2 m, |x - k STEP| < 0.35, |y| < 0.25 in frame k, as DatasetType.CUSTOM files: it slides in its own
    plane, so away from its two vertical edges every frame's depth is the same."""
    from PIL import Image
    u, v = np.meshgrid(np.arange(PW), np.arange(PH))
    x, y = (u - PW / 2) * 1.2 / PFX, (v - PH / 2) * 1.2 / PFX
    for k in range(frames):
        d = np.where((np.abs(x - k * STEP) < 0.35) & (np.abs(y) < 0.25), 1200, 0).astype(np.uint16)
        Image.fromarray(d).save(str(directory / f"depth_{k:04d}.png"))
        Image.fromarray(np.full((PH, PW, 3), 128, np.uint8)).save(str(directory / f"rgb_{k:04d}.png"))
    rows = [[PFX, 0, PW / 2, 0], [0, PFX, PH / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    (directory / "camera_intrinsics.txt").write_text("\n".join(" ".join(repr(float(c)) for c in row) for row in rows) + "\n")


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def test_pipeline_landmark_provider(nn, tmp_path):
    """Three synthetic frames of a plate that slides 1 cm per frame in its own plane, which the depth term cannot see, tracked
    with the real-sequence recipe (IRLS, coupled, zero-rotation guard), 4 iterations per frame. The ground-truth provider
    ties every 40th face's first vertex to where the slide takes it. Without a provider the graph stays where it was; with
    it the node translations follow the slide in both tracked frames and FrameResult carries the three fields. The
    landmark residual is linear in the translations, so a Gauss-Newton step at damping 0.001 removes nearly all of it: the
    distances the last of the 4 iterations starts from are held to a fifth of the 10 mm each frame begins with, the mean
    node translation to 1.5 mm of the truth."""
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    A = nn.alignment
    _write_sliding_plate(tmp_path)
    calls = []

    def provider(pipeline, frame, canonical, point_image):
        k = pipeline.processed_frames - 1   # 1, 2: the frame being tracked
        tri, pos = _host(canonical.triangle_indices), _host(canonical.vertex_positions)
        idx = np.unique(tri[::40, 0]).astype(np.int32)
        calls.append((k, len(idx), tuple(point_image.shape)))
        return idx, (pos[idx] + np.array([k * STEP, 0.0, 0.0])).astype(F32), None

    def run(**kw):
        seq = dfr.FrameSequenceDataset(base_dataset_type=dfr.DatasetType.CUSTOM, custom_frame_directory=str(tmp_path)).load()
        params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH,
                                    mesh_extraction_weight_thresholding_mode=F.MeshExtractionWeightThresholdingMode.CONSTANT,
                                    mesh_extraction_weight_threshold=0, coupled_data_term=True)
        params.alignment.max_iteration_count = 4
        params.alignment.guard_zero_rotation = True
        params.alignment.penalty_form = A.PenaltyForm.IRLS
        pipe = F.FusionPipeline(seq, params, **kw)
        translations = []
        while seq.has_more_frames():
            pipe.process_frame(seq.get_next_frame())
            translations.append(pipe.active_graph.get_node_translations(True).copy())
        return pipe.results, translations

    plain, t_plain = run()
    none, t_none = run(landmark_provider=lambda *a: None)
    with_lm, t_lm = run(landmark_provider=provider)
    assert len(plain) == len(with_lm) == 3 and [r.tracked for r in with_lm] == [False, True, True]
    assert [c[0] for c in calls] == [1, 2] and all(c[1] > 100 for c in calls)
    # no provider, or one that has nothing to say: no term, the same results, and a graph that has not seen the slide
    for r in plain + none + with_lm[:1]:
        assert (r.landmark_count, r.landmark_active_count, r.landmark_rmse) == (0, 0, 0.0)
    for a, b in zip(t_plain, t_none):
        assert np.array_equal(a, b, equal_nan=True)
    for k in (1, 2):
        r = with_lm[k]
        mean_x, blind_x = float(t_lm[k][:, 0].mean()), float(t_plain[k][:, 0].mean())
        print(f"frame {k}: {r.landmark_count} landmarks, {r.landmark_active_count} active, rmse {r.landmark_rmse:.4g} m; mean node t.x {mean_x:.4g} "
              f"(truth {k * STEP:.3g}; without landmarks {blind_x:.4g}); max |t.yz| {np.abs(t_lm[k][:, 1:]).max():.3g}")
        assert r.landmark_count == calls[k - 1][1] and r.landmark_active_count == r.landmark_count
        assert 0.0 < r.landmark_rmse < 0.2 * STEP
        assert abs(mean_x - k * STEP) < 1.5e-3
        assert abs(blind_x) < 1e-3
