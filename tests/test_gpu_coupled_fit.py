"""GPU tests of the fitter's coupled data term (nnrt_fitter_set_data_coupling) against the float64
assembly of tests/_coupled_util.py (validated in tests/test_coupled_cpu.py). Scenes: S1 (96 x 128, 24 nodes) and S1_ARAP
(48 nodes, 2 layers): the smallest where a face spans several nodes, an edge coincides with a data pair and a wave holds
pixels of different node sets."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _coupled_util import (apply_update, coupled_step, coupled_system, data_system, edge_pairs, face_pairs, gt_translations_virtual,   # noqa: E402
                           identity_motion, solve_dense, solve_float32, union_pairs)
from _util import rel_err, scene_target   # noqa: E402
from test_gpu_parity import nan_rel_err   # noqa: E402

pytestmark = pytest.mark.gpu

LM = 0.001


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
    oracle_mod.set_fused_jacobians(False)   # the reference CPU path's arithmetic, whatever the library build
    out = {}
    for name in ("S1", "S1_ARAP"):
        sc = S.make_scene(name, hierarchy_builder=lambda n, c, l: oracle_mod.build_hierarchy(n, c, l))
        out[name] = (sc, scene_target(oracle_mod, sc))
    return out


def _hg_bar():
    from dynamicfuion_python_amd import _native
    return 1e-5 if _native.jacobian_fma() else 1e-6


def _fitter(nn, sc, coupled=True, anchor_count=4, graph=0, lm=LM, iterations=1, **kw):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, anchor_count, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE,
                                      sc.layer_count)
    ft = A.DeformableMeshToImageFitter(iterations, [A.IterationMode.ALL], preconditioning_dampening_factor=lm, use_hip_graph=graph, **kw)
    if coupled is not None:
        ft.set_data_coupling(A.DataCoupling.COUPLED if coupled else A.DataCoupling.BLOCK_DIAGONAL)
    return wf, ft


def _mesh(nn, sc):
    return nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces)


def _motion(wf):
    return wf.get_node_rotations(True), wf.get_node_translations(True)


def _cost(dg):
    m = dg["residual_mask"]
    return float((dg["residuals"][m].astype(np.float64) ** 2).sum())


def _check_system(ft, want, bar, label):
    """The exported system against the float64 assembly `want`; returns the exported blocks."""
    diag, pairs, blocks, rhs = ft.coupled_system()
    assert np.array_equal(pairs, want["pairs"])
    errs = (nan_rel_err(blocks, want["blocks"]), nan_rel_err(diag, want["diag"]), nan_rel_err(rhs, want["rhs"]))
    print(f"{label}: {len(pairs)} pairs; off-diagonal {errs[0]:.2g}, diagonal {errs[1]:.2g}, rhs {errs[2]:.2g} (bar {bar:g})")
    assert max(errs) < bar, errs
    return diag, pairs, blocks, rhs


# ---- 1. structure -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1", "S1_ARAP"])
def test_pair_structure(nn, oracle_mod, scenes, name):
    sc, depth = scenes[name]
    wf, ft = _fitter(nn, sc)
    assert ft.data_coupling == nn.alignment.DataCoupling.COUPLED and ft.coupled_pair_count == 0
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    want = union_pairs(face_pairs(oracle_mod, sc), edge_pairs(sc))
    _, pairs, _, _ = ft.coupled_system()
    assert ft.coupled_pair_count == len(want) == len(pairs)
    assert np.array_equal(pairs, want)
    assert (pairs[:, 0] < pairs[:, 1]).all()
    assert len({tuple(p) for p in pairs.tolist()}) == len(pairs)
    if name == "S1":
        assert len(pairs) == 140
    else:
        assert len(want) > len(face_pairs(oracle_mod, sc)) or len(edge_pairs(sc)) > 0


# ---- 2. system parity, one iteration ----------------------------------------------------------------------------------
@pytest.mark.parametrize("start,anchor_count", [("identity", 4), ("partial", 4), ("identity", 8)])
def test_system_parity(nn, oracle_mod, scenes, start, anchor_count):
    sc, depth = scenes["S1"]
    wf, ft = _fitter(nn, sc, anchor_count=anchor_count)
    if start == "partial":
        R0, t0 = sc.partial_motion(0.5)
        wf.set_node_rotations(R0)
        wf.set_node_translations(t0)
    R, t = _motion(wf)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    want = coupled_system(oracle_mod, sc, depth, R, t, anchor_count=anchor_count, lm=LM)
    diag, pairs, blocks, rhs = _check_system(ft, want, _hg_bar(), f"S1 from {start}, K = {anchor_count}")
    # a pair the face table predicts but no contributing pixel touches holds an exactly zero block
    touched = want["data"]["touched"][pairs[:, 0], pairs[:, 1]]
    print(f"  {int((~touched).sum())} of {len(pairs)} pairs untouched")
    assert not blocks[~touched].any()
    assert blocks[touched].any()


def test_system_parity_at_image_edges(nn, oracle_mod, scenes):
    """test_system_parity's `identity, 4 anchors` case on S1 cropped to 74 x 102 about its centre: neither side is a multiple
    of 8, so the last quadrant of every row and column of the pair launch holds lanes outside the image, and the mesh
    overflows the crop, so the lanes beside them contribute."""
    import dataclasses
    s1, _ = scenes["S1"]
    H, W = 74, 102
    K = s1.K.copy()
    K[0, 2], K[1, 2] = W / 2, H / 2
    sc = dataclasses.replace(s1, H=H, W=W, K=K)
    depth = scene_target(oracle_mod, sc)
    wf, ft = _fitter(nn, sc)
    R, t = _motion(wf)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    want = coupled_system(oracle_mod, sc, depth, R, t, lm=LM)
    contributes = want["data"]["contributes"].reshape(H, W)
    assert contributes[:, W - W % 8:].any() and contributes[H - H % 8:].any(), "no contributing pixel in the partial quadrants"
    diag, pairs, blocks, rhs = _check_system(ft, want, _hg_bar(), f"S1 cropped to {H} x {W}")
    touched = want["data"]["touched"][pairs[:, 0], pairs[:, 1]]
    assert not blocks[~touched].any()
    assert blocks[touched].any()


# ---- 2b. the pair launch has no say in pass 1's outputs -------------------------------------------------------------------
@pytest.mark.parametrize("tukey", [False, True])
def test_pair_launch_leaves_pass_one_outputs(nn, oracle_mod, scenes, tukey):
    """One eager iteration from the same S1 start, block-diagonal and coupled: residuals, residual mask and pixel faces
    are pass 1's alone, bit for bit. With IRLS Tukey: the target and cutoff test_gpu_robust_step.py takes for S1_coupled."""
    import _robust_step_util as RU
    sc, depth = scenes["S1"]
    kw = {}
    if tukey:
        sc, depth, c, _ = RU.config_inputs(oracle_mod, scenes, "S1_coupled")
        kw = dict(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=c, penalty_form=nn.alignment.PenaltyForm.IRLS)
    out = []
    for coupled in (False, True):
        wf, ft = _fitter(nn, sc, coupled=coupled, **kw)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, 1)
        ft.check()
        out.append(ft.diagnostics())
    assert out[0]["residual_mask"].any() and (out[0]["pixel_faces"] >= 0).any()
    if tukey:   # some masked pixels lie beyond the cutoff: their stored residual is the exact 0 of a pixel without weight
        assert (out[0]["residuals"][out[0]["residual_mask"]] == 0).any()
    for key in ("residuals", "residual_mask", "pixel_faces"):
        assert np.array_equal(out[0][key], out[1][key], equal_nan=True), key


# ---- 3. system parity with ARAP and IRLS --------------------------------------------------------------------------------
@pytest.mark.parametrize("irls", [False, True])
def test_system_parity_arap(nn, oracle_mod, scenes, irls):
    A = nn.alignment
    sc, depth = scenes["S1_ARAP"]
    both = {tuple(p) for p in face_pairs(oracle_mod, sc).tolist()} & {tuple(p) for p in edge_pairs(sc).tolist()}
    assert both, "S1_ARAP has no pair that is both a data pair and an edge"
    kw, okw = {}, {}
    R0, t0 = sc.partial_motion(0.5)
    if irls:
        vi = sc.hierarchy["virtual_indices"]
        sq = coupled_system(oracle_mod, sc, depth, R0[vi], t0[vi], lm=LM)
        m = sq["data"]["residual_mask"]
        c = float(np.median(np.abs(sq["data"]["r"][m])))
        from _robust_util import arap_term
        delta = float(np.median(arap_term(oracle_mod, sc, R0[vi], t0[vi])["norms"]))
        kw = dict(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=c, use_huber_penalty_for_arap_term=True,
                  huber_penalty_constant=delta, penalty_form=A.PenaltyForm.IRLS)
        okw = dict(tukey_c=c, huber_delta=delta)
    wf, ft = _fitter(nn, sc, **kw)
    wf.set_node_rotations(R0)
    wf.set_node_translations(t0)
    R, t = _motion(wf)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    want = coupled_system(oracle_mod, sc, depth, R, t, lm=LM, **okw)
    diag, pairs, blocks, rhs = _check_system(ft, want, _hg_bar(), f"S1_ARAP at half the motion, {'IRLS' if irls else 'square'}")
    # one pair that is a data pair and an edge: its block is the sum of both parts
    i, j = sorted(both)[0]
    s = int(np.nonzero((pairs[:, 0] == i) & (pairs[:, 1] == j))[0][0])
    assert rel_err(blocks[s], want["blocks"][s]) < 1e-5


# ---- 4. solve -----------------------------------------------------------------------------------------------------------
def test_solve_and_update(nn, oracle_mod, scenes):
    sc, depth = scenes["S1"]
    N = len(sc.nodes)
    wf, ft = _fitter(nn, sc)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    dg = ft.diagnostics()
    diag, pairs, blocks, rhs = ft.coupled_system()
    x64, cond = solve_dense(diag, pairs, blocks, rhs)
    e_f32 = rel_err(solve_float32(diag, pairs, blocks, rhs), x64)
    x_g = dg["updates"][: 6 * N]
    e_g = rel_err(x_g, x64)
    print(f"S1 coupled solve: fp64 condition number {cond:.3g}; GPU {e_g:.2g}, float32 numpy Cholesky {e_f32:.2g} from the fp64 solution")
    assert e_g <= max(1e-4, e_f32)
    # the node motion after the step: t = 0 + dt, R = I Rodrigues(w) of those updates (RodriguesImpl.h:66-88, A10)
    x = np.asarray(x_g, np.float32).reshape(N, 6)
    R_g, t_g = _motion(wf)
    assert np.array_equal(t_g, np.float32(0) + x[:, 3:])
    dR = oracle_mod.rodrigues(np.ascontiguousarray(x[:, :3])).reshape(N, 3, 3)
    I3 = np.eye(3, dtype=np.float32)
    R_e = np.empty_like(dR)
    for r in range(3):
        for c in range(3):
            R_e[:, r, c] = (I3[r, 0] * dR[:, 0, c] + I3[r, 1] * dR[:, 1, c]) + I3[r, 2] * dR[:, 2, c]
    assert np.array_equal(R_g.reshape(N, 3, 3), R_e)


# ---- 5 + 6. trajectory and convergence --------------------------------------------------------------------------------
def _trajectory(nn, sc, depth, coupled, iterations=6):
    wf, ft = _fitter(nn, sc, coupled=coupled, iterations=iterations)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    states, costs, systems = [_motion(wf)], [], []
    for k in range(iterations):
        ft.iterate(wf, k, 1)
        dg = ft.diagnostics()
        costs.append(_cost(dg))
        if coupled:
            systems.append(ft.coupled_system() + (dg["updates"].copy(),))
        states.append(_motion(wf))
    return states, costs, systems


def test_synchronised_trajectory_and_convergence(nn, oracle_mod, scenes):
    """Six coupled iterations on S1 from the identity, lambda = 0.001. Each is compared with the restatement started
    from the GPU's own motion before it; the cost (sum r^2 over the residual mask, measured at the start of iteration k)
    and the final translation error are held to 2 x the restatement's own trajectory. Block-diagonal: the cost rises."""
    sc, depth = scenes["S1"]
    N = len(sc.nodes)
    gt = gt_translations_virtual(sc)
    states, costs, systems = _trajectory(nn, sc, depth, True)
    bar = _hg_bar()
    for k, (diag, pairs, blocks, rhs, upd) in enumerate(systems):
        R, t = states[k]
        want = coupled_system(oracle_mod, sc, depth, R, t, lm=LM)
        errs = (nan_rel_err(blocks, want["blocks"]), nan_rel_err(diag, want["diag"]), nan_rel_err(rhs, want["rhs"]))
        x64, cond = solve_dense(diag, pairs, blocks, rhs)
        e_f32 = rel_err(solve_float32(diag, pairs, blocks, rhs), x64)
        e_g = rel_err(upd[: 6 * N], x64)
        print(f"iteration {k + 1}: cost {costs[k]:.4g}; system {max(errs):.2g}; solve {e_g:.2g} (float32 numpy {e_f32:.2g}, cond {cond:.3g})")
        assert max(errs) < bar, (k, errs)
        assert e_g <= max(1e-4, e_f32), k
    # the restatement's own trajectory from the identity
    R, t = identity_motion(N)
    ref_costs = []
    for _ in range(6):
        R, t, sysm, _ = coupled_step(oracle_mod, sc, depth, R, t, lm=LM)
        ref_costs.append(sysm["data"]["cost"])
        if len(ref_costs) == 6:
            break
        if len(ref_costs) == 5:
            ref_err = float(np.linalg.norm(t - gt, axis=1).mean())
    gpu_err = float(np.linalg.norm(states[5][1] - gt, axis=1).mean())
    print("GPU cost at the start of iterations 1..6:        ", [f"{c:.4g}" for c in costs])
    print("restatement cost at the start of iterations 1..6:", [f"{c:.4g}" for c in ref_costs])
    print(f"mean |t - gt| after 5 steps: GPU {gpu_err:.4g}, restatement {ref_err:.4g}")
    for k in range(1, 6):
        assert costs[k] <= 2 * ref_costs[k], k
    assert gpu_err <= 2 * ref_err
    assert costs[5] < costs[0] / 50
    _, bd_costs, _ = _trajectory(nn, sc, depth, False, iterations=2)
    print("block-diagonal cost at the start of iterations 1..2:", [f"{c:.4g}" for c in bd_costs])
    assert bd_costs[1] > bd_costs[0]


# ---- 7. the default is untouched ----------------------------------------------------------------------------------------
def test_default_untouched(nn, scenes):
    sc, depth = scenes["S1"]
    A = nn.alignment

    def run(prep):
        wf, ft = _fitter(nn, sc, coupled=None, graph=2)
        prep(wf, ft)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, 1)
        ft.check()
        return ft.diagnostics(), _motion(wf), ft.graph_count, ft.launch_plan()

    def explicit(wf, ft):
        ft.set_data_coupling(A.DataCoupling.BLOCK_DIAGONAL)

    def there_and_back(wf, ft):
        ft.set_data_coupling(A.DataCoupling.COUPLED)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.set_data_coupling(A.DataCoupling.BLOCK_DIAGONAL)
        with pytest.raises(RuntimeError):   # the setter invalidated the prepared frame
            ft.iterate(wf, 0, 1)

    fresh = run(lambda wf, ft: None)
    for other in (run(explicit), run(there_and_back)):
        for key in fresh[0]:
            assert np.array_equal(fresh[0][key], other[0][key], equal_nan=True), key
        assert np.array_equal(fresh[1][0], other[1][0]) and np.array_equal(fresh[1][1], other[1][1])
        assert fresh[2] == other[2] and fresh[3] == other[3]


# ---- 8. graph replay ----------------------------------------------------------------------------------------------------
def test_graph_replay(nn, scenes):
    sc, depth = scenes["S1"]
    mesh = _mesh(nn, sc)
    wf_e, ft_e = _fitter(nn, sc, graph=0, iterations=3)
    ft_e.prepare(wf_e, mesh, depth, None, sc.K, None, 1.0)
    ft_e.iterate(wf_e, 0, 3)
    ft_e.check()
    R_e, t_e = _motion(wf_e)
    wf, ft = _fitter(nn, sc, graph=2, iterations=3)
    ft.prepare(wf, mesh, depth, None, sc.K, None, 1.0)
    ft.snapshot_motion(wf)
    ft.iterate(wf, 0, 3)
    ft.check()
    assert ft.graph_count == 1
    R_g, t_g = _motion(wf)
    ft.restore_motion(wf)
    ft.fit_from_snapshot(wf, 3)
    ft.check()
    R_s, t_s = _motion(wf)
    I3 = np.eye(3)
    errs = (rel_err(t_g, t_e), rel_err(R_g - I3, R_e - I3), rel_err(t_s, t_e), rel_err(R_s - I3, R_e - I3))
    print(f"3 coupled iterations, graph replay vs eager: t {errs[0]:.2g}, R - I {errs[1]:.2g}; from the snapshot: t {errs[2]:.2g}, R - I {errs[3]:.2g}")
    assert max(errs) <= 1e-4


# ---- 9. singular system, and the refusals ---------------------------------------------------------------------------------
def test_singular_system_is_reported(nn, oracle_mod, scenes):
    sc, depth = scenes["S1"]
    N = len(sc.nodes)
    d = data_system(oracle_mod, sc, depth)
    # the node with the fewest contributing pixels: zero the depth of every pixel whose face anchors to it
    pf, fn, fc = d["pixel_faces"], d["face_nodes"], d["face_counts"]
    has = np.zeros((len(fn), N), bool)
    for x in range(fn.shape[1]):
        ok = fc > x
        has[np.nonzero(ok)[0], fn[ok, x]] = True
    px = np.nonzero(d["contributes"] & (pf >= 0))[0]
    counts = has[pf[px]].sum(axis=0)
    node = int(np.argmin(np.where(counts > 0, counts, counts.max() + 1)))
    masked = depth.copy().reshape(-1)
    hit = np.nonzero(pf >= 0)[0]
    masked[hit[has[pf[hit], node]]] = 0.0
    masked = masked.reshape(depth.shape)
    d2 = data_system(oracle_mod, sc, masked)
    assert not d2["touched"][node].any() and d2["touched"].any()
    wf, ft = _fitter(nn, sc, lm=0.0)
    ft.prepare(wf, _mesh(nn, sc), masked, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    with pytest.raises(RuntimeError, match="positive-definite"):
        ft.check()
    wf, ft = _fitter(nn, sc, lm=LM, guard_zero_rotation=True)
    ft.prepare(wf, _mesh(nn, sc), masked, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()
    R, t = _motion(wf)
    assert np.isfinite(R).all() and np.isfinite(t).all()


def test_refusals(nn):
    A = nn.alignment
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL])
    with pytest.raises(RuntimeError, match="data_coupling"):
        ft.set_data_coupling(2)
    assert ft.data_coupling == A.DataCoupling.BLOCK_DIAGONAL
    ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL, A.IterationMode.TRANSLATION_ONLY])
    with pytest.raises(RuntimeError, match="data_coupling"):
        ft.set_data_coupling(A.DataCoupling.COUPLED)
    ft.set_data_coupling(A.DataCoupling.BLOCK_DIAGONAL)
