"""GPU tests of step control under the robust step objective (nnrt_fitter_set_step_objective, k_step_cost_robust; DESIGN.md
section 25) against the float64 restatement of tests/_robust_step_util.py (checked in tests/test_robust_step_cpu.py, which
holds every decision of CONFIGS_ROBUST to a 1e-2 margin). Scenes: S1 (96 x 128, 24 nodes; the cost sum takes three
workgroups) and S1_ARAP (48 nodes, 2 layers: the edges' Huber cost)."""
import dataclasses
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _robust_step_util as RU   # noqa: E402
import _step_control_util as U   # noqa: E402
from _coupled_util import data_system   # noqa: E402
from _robust_util import F32, patch_targets   # noqa: E402
from _util import scene_target   # noqa: E402

pytestmark = pytest.mark.gpu

# The cost of every iteration against the restatement's own trajectory, relative. Measured on the first run (DESIGN.md
# section 25): 5.3e-7 (S1 block-diagonal), 2.8e-6 (S1 coupled), 3.5e-5 (S1_ARAP arrowhead); the bar is ten times the largest
# and stays below the 1e-3 cap (itself below the 1e-2 decision margin, so the bar cannot hide a flipped decision).
COST_BAR = min(10 * 3.47e-5, 1e-3)


@pytest.fixture(scope="module", autouse=True)
def _collect_garbage():
    """The pipeline test's objects reference each other: collected here, so that the device memory they hold is returned
    before the next module's tests read nnrt_device_bytes_in_use."""
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


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
    out = {}
    for name in ("S1", "S1_ARAP"):
        sc = S.make_scene(name, hierarchy_builder=lambda n, c, l: oracle_mod.build_hierarchy(n, c, l))
        out[name] = (sc, scene_target(oracle_mod, sc))
    return out


@pytest.fixture(scope="module")
def inputs(oracle_mod, scenes):
    """(scene, target A, Tukey cutoff, Huber delta) of every configuration, computed once."""
    return {name: RU.config_inputs(oracle_mod, scenes, name) for name in RU.CONFIGS_ROBUST}


@pytest.fixture(scope="module")
def restated(oracle_mod, scenes):
    return {name: RU.run_config(oracle_mod, scenes, name) for name in RU.CONFIGS_ROBUST}


def _fitter(nn, sc, coupled, settings, iterations, threshold=1e-6, graph=0, lm=U.LM, robust=True, tukey_c=None, huber=None, irls=True,
            guard=True, **kw):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)
    if tukey_c is not None:
        kw.update(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=tukey_c)
    if huber is not None:
        kw.update(use_huber_penalty_for_arap_term=True, huber_penalty_constant=huber)
    ft = A.DeformableMeshToImageFitter(iterations, [A.IterationMode.ALL], minimal_update_threshold=threshold, preconditioning_dampening_factor=lm,
                                       use_hip_graph=graph, penalty_form=A.PenaltyForm.IRLS if irls else A.PenaltyForm.REFERENCE,
                                       guard_zero_rotation=guard,
                                       step_objective=A.StepObjective.ROBUST if robust else A.StepObjective.SQUARE, **kw)
    if coupled:
        ft.set_data_coupling(A.DataCoupling.COUPLED)
    if settings is not None:
        ft.set_step_control(A.StepControl(**settings))
    return wf, ft


def _config_fitter(nn, inputs, name, graph=0):
    _, coupled, settings, iterations, _, _ = RU.CONFIGS_ROBUST[name]
    sc, A, c, huber = inputs[name]
    wf, ft = _fitter(nn, sc, coupled, settings, iterations, graph=graph, tukey_c=c, huber=huber)
    ft.prepare(wf, _mesh(nn, sc), A, None, sc.K, None, 1.0)
    return wf, ft, iterations


def _mesh(nn, sc):
    return nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces)


def _motion(wf):
    return wf.get_node_rotations(True), wf.get_node_translations(True)


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def _rows(history):
    return [(r.iteration, r.cost, np.float32(r.lambda_used), int(r.decision), r.max_update) for r in history]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the raw residuals are pass 1's, bit for bit -----------------------------------------------------------------------
def test_raw_residuals_equal_pass_one_without_penalties(nn, scenes):
    """Both penalties off: the residual buffer holds r itself, and the robust cost is the square cost in the same order."""
    scene, coupled, settings, iterations, threshold = U.CONFIGS["S1_coupled"]
    sc, depth = scenes[scene]
    runs = []
    for robust in (True, False):
        wf, ft = _fitter(nn, sc, coupled, settings, 3, threshold, robust=robust, irls=False, guard=False)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        for first, count in ((0, 1), (1, 2)):   # at the identity, and at the state two iterations later
            ft.iterate(wf, first, count)
            if robust:
                dg, raw = ft.diagnostics(), ft.raw_residuals()
                assert dg["residual_mask"].sum() > 1000 and np.abs(raw[dg["residual_mask"]]).max() > 0
                assert np.array_equal(_bits(raw), _bits(dg["residuals"])), first
                assert not raw[~dg["residual_mask"]].any()
        ft.check()
        runs.append((_rows(ft.step_history()), _motion(wf)))
    assert [r[3] for r in runs[0][0]] == [U.START, U.ACCEPT, U.ACCEPT]   # the third iteration ran at a moved state
    assert runs[0][0] == runs[1][0]   # the cost history equals the SQUARE objective's, bit for bit
    assert _same(runs[0][1], runs[1][1])


def test_raw_residuals_equal_pass_one_under_tukey(nn, inputs):
    """Tukey IRLS on: s r formed in float32 from the raw residuals is the residual buffer where the pixel contributes."""
    sc, A, c, _ = inputs["S1_coupled"]
    _, coupled, settings, _, _, _ = RU.CONFIGS_ROBUST["S1_coupled"]
    wf, ft = _fitter(nn, sc, coupled, settings, 3, tukey_c=c)
    ft.prepare(wf, _mesh(nn, sc), A, None, sc.K, None, 1.0)
    c32 = F32(c)
    for first, count in ((0, 1), (1, 2)):
        ft.iterate(wf, first, count)
        dg, raw = ft.diagnostics(), ft.raw_residuals()
        mask = dg["residual_mask"]
        contributes = mask & (np.abs(raw) <= c32)
        assert 1000 < contributes.sum() < mask.sum()   # the patch is cut
        q = (raw / c32).astype(F32)
        s = (F32(1.0) - (q * q).astype(F32)).astype(F32)
        want = np.where(contributes, (s * raw).astype(F32), F32(0.0)).astype(F32)
        assert np.array_equal(_bits(want), _bits(dg["residuals"])), first
        assert not raw[~mask].any()
    ft.check()
    assert [int(r.decision) for r in ft.step_history()] == [U.START, U.ACCEPT, U.ACCEPT]


# ---- 2. the cost ----------------------------------------------------------------------------------------------------------
def test_cost_equals_the_host_sum(nn, inputs):
    """Iteration 0 on S1: the device's fixed-order fp64 sum against the host's, the polynomial in the header's literal form."""
    sc, A, c, _ = inputs["S1_block"]
    wf, ft, _ = _config_fitter(nn, inputs, "S1_block")
    ft.iterate(wf, 0, 1)
    raw, mask = ft.raw_residuals(), ft.diagnostics()["residual_mask"]
    r = raw[mask].astype(np.float64)
    cd = float(F32(c))
    inside = np.abs(raw[mask]) <= F32(c)
    term = np.where(inside, (cd * cd / 3.0) * (1.0 - (1.0 - (r / cd) ** 2) ** 3), cd * cd / 3.0)
    host, got = float(term.sum()), ft.step_history()[0].cost
    print(f"device {got!r} host {host!r} relative {abs(got - host) / host:.3g}; {inside.sum()} inside the cutoff, {(~inside).sum()} beyond")
    assert (~inside).sum() > 100 and inside.sum() > 1000
    assert abs(got - host) <= 1e-12 * host
    assert abs(got - RU.tukey_cost(raw, mask, c)) <= 1e-12 * host


# ---- 3. the state machine, iteration by iteration ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RU.CONFIGS_ROBUST))
def test_trajectory_equals_the_restatement(nn, inputs, restated, name):
    want = restated[name]
    wf, ft, iterations = _config_fitter(nn, inputs, name)
    ft.iterate(wf, 0, iterations)
    ft.check()
    got = ft.step_history()
    assert [r.iteration for r in got] == list(range(iterations))
    cost_err = max(abs(g.cost - w["cost"]) / w["cost"] for g, w in zip(got, want))
    print(f"{name}: decisions {[int(r.decision) for r in got]}")
    print(f"  lambda {[float(np.float32(r.lambda_used)) for r in got]}")
    print(f"  cost {[f'{r.cost:.6g}' for r in got]}")
    print(f"  cost vs the restatement's trajectory: {cost_err:.3g} relative (bar {COST_BAR:.3g})")
    assert [int(r.decision) for r in got] == [w["decision"] for w in want]
    assert [np.float32(r.lambda_used) for r in got] == [w["lambda_used"] for w in want]
    assert cost_err <= COST_BAR
    s = ft.step_summary()
    assert (s["iterations_used"], s["rejected_step_count"]) == (RU.summarize(want)[0], RU.summarize(want)[2])
    assert abs(s["final_cost"] - want[-1]["c_best"]) <= COST_BAR * want[-1]["c_best"]


# ---- 4. graph replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1_coupled", "S1_ARAP_arrowhead"])
def test_graph_replay_equals_eager(nn, inputs, name):
    runs = []
    for graph in (0, 2):
        wf, ft, iterations = _config_fitter(nn, inputs, name, graph=graph)
        ft.iterate(wf, 0, iterations)
        ft.check()
        runs.append((_rows(ft.step_history()), _motion(wf), ft.graph_count, ft.raw_residuals()))
    assert runs[0][0] == runs[1][0]   # cost, lambda, decision and max |update| of every iteration, bit for bit
    assert _same(runs[0][1], runs[1][1])
    assert (runs[0][2], runs[1][2]) == (0, 1)   # one iteration is still one captured sequence
    assert np.array_equal(_bits(runs[0][3]), _bits(runs[1][3]))


# ---- 5. the contrast -------------------------------------------------------------------------------------------------------
def test_robust_run_ends_closer_than_the_square_run(nn, inputs):
    name = "S1_coupled"
    _, coupled, settings, iterations, _, _ = RU.CONFIGS_ROBUST[name]
    sc, A, c, _ = inputs[name]
    wf, ft, _ = _config_fitter(nn, inputs, name)
    ft.iterate(wf, 0, iterations)
    ft.check()
    e_robust = RU.translation_error(sc, _motion(wf)[1])
    wf, ft = _fitter(nn, sc, coupled, settings, iterations, robust=False, irls=False)
    ft.prepare(wf, _mesh(nn, sc), A, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, iterations)
    ft.check()
    e_square = RU.translation_error(sc, _motion(wf)[1])
    print(f"RMS translation error: SQUARE {e_square:.4g} (decisions {[int(r.decision) for r in ft.step_history()]}), ROBUST {e_robust:.4g}")
    assert 2.0 * e_robust <= e_square


# ---- 6. a state or a residual that is not finite ---------------------------------------------------------------------------
def _mask_one_node(oracle_mod, sc, depth):
    """`depth` with every pixel zeroed whose face anchors to the node with the fewest contributing pixels (the setup of
    tests/test_gpu_step_control.py::test_held_iterations_error_bits_are_discarded): that node's data block and gradient
    are exactly zero."""
    N = len(sc.nodes)
    d = data_system(oracle_mod, sc, depth)
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
    return masked.reshape(depth.shape)


def test_nan_rotation_is_rejected(nn, oracle_mod, scenes):
    """S1 (no hierarchy), block-diagonal, one node's pixels masked out, no zero-rotation guard: that node's block is
    lambda I with a zero right-hand side, its rotation update is exactly 0 and Rodrigues makes its rotation NaN.
    The faces it moves are then not rendered and their pixels leave the mask, so every residual of that state is finite;
    its cost is NaN all the same, and the step is rejected at every damping up to lambda_max."""
    sc, depth = scenes["S1"]
    masked = _mask_one_node(oracle_mod, sc, depth)
    c = 1.5 * float(np.abs(data_system(oracle_mod, sc, masked)["r"]).max())
    wf, ft = _fitter(nn, sc, False, U.control(increase=10.0, decrease=0.5, lambda_max=0.1), 8, tukey_c=c, guard=False)
    ft.prepare(wf, _mesh(nn, sc), masked, None, sc.K, None, 1.0)
    start = _motion(wf)
    ft.iterate(wf, 0, 1)
    assert np.isnan(_motion(wf)[0]).any()   # the step from the identity leaves the NaN rotation
    ft.iterate(wf, 1, 7)
    got = ft.step_history()
    print("decisions", [int(r.decision) for r in got], "cost", [f"{r.cost:.4g}" for r in got])
    assert [int(r.decision) for r in got] == [U.START, U.REJECT, U.START, U.REJECT, U.START, U.REJECT_FINAL, U.HOLD, U.HOLD]
    assert all(np.isnan(got[k].cost) for k in (1, 3, 5)) and all(np.isfinite(got[k].cost) and got[k].cost > 0 for k in (0, 2, 4, 6, 7))
    raw = ft.raw_residuals()
    assert np.isfinite(raw).all()
    ft.check()
    assert _same(_motion(wf), start) and np.isfinite(_motion(wf)[0]).all()


def test_nan_residual_is_not_a_saturated_cost(nn, oracle_mod, scenes):
    """A masked-in pixel whose reference point is NaN (the point-cloud overload takes the caller's mask as given): r is NaN,
    the pixel carries no weight in the IRLS step, and the cost is NaN -- a reject -- not the finite c^2 / 3 of a pixel
    beyond the cutoff."""
    sc, depth = scenes["S1"]
    refp, refm = oracle_mod.unproject(depth, sc.K, 1.0, 10.0)
    dg = data_system(oracle_mod, sc, depth)
    p = int(np.nonzero(dg["residual_mask"])[0][100])
    c = 1.5 * float(np.abs(dg["r"]).max())
    histories = []
    for poison in (False, True):
        pts = np.ascontiguousarray(refp, np.float32).reshape(-1, 3).copy()
        if poison:
            pts[p, 2] = np.nan
        wf, ft = _fitter(nn, sc, True, U.control(increase=10.0, decrease=0.1, lambda_max=10.0), 2, tukey_c=c)
        ft.prepare_point_cloud(wf, _mesh(nn, sc), pts, refm.reshape(-1), sc.K, None, (sc.H, sc.W))
        ft.iterate(wf, 0, 2)
        ft.check()
        histories.append(ft.step_history())
        if poison:
            raw, mask = ft.raw_residuals(), ft.diagnostics()["residual_mask"]
            assert mask[p] and np.isnan(raw[p]) and np.isfinite(np.delete(raw, p)).all()
    clean, bad = histories
    print("clean", [(int(r.decision), r.cost) for r in clean], "poisoned", [(int(r.decision), r.cost) for r in bad])
    assert [int(r.decision) for r in clean] == [U.START, U.ACCEPT] and all(np.isfinite(r.cost) for r in clean)
    assert [int(r.decision) for r in bad] == [U.START, U.REJECT] and all(np.isnan(r.cost) for r in bad)


# ---- 7. the switch ---------------------------------------------------------------------------------------------------------
def test_default_objective_is_untouched(nn, scenes):
    """A step-controlled SQUARE fit is what it was: the objective left alone, set to SQUARE, or taken to ROBUST and back."""
    A = nn.alignment
    scene, coupled, settings, iterations, threshold = U.CONFIGS["S1_coupled"]
    sc, depth = scenes[scene]

    def run(prep):
        wf, ft = _fitter(nn, sc, coupled, settings, iterations, threshold, graph=2, robust=False, irls=False, guard=False)
        prep(ft)
        assert ft.step_objective == A.StepObjective.SQUARE
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, iterations)
        ft.check()
        with pytest.raises(RuntimeError, match="NNRT_STEP_OBJECTIVE_ROBUST"):
            ft.raw_residuals()
        return _rows(ft.step_history()), _motion(wf), ft.graph_count, ft.launch_plan(), ft.diagnostics()

    def there_and_back(ft):
        ft.set_step_objective(A.StepObjective.ROBUST)
        ft.set_step_objective(A.StepObjective.SQUARE)

    plain = run(lambda ft: None)
    for other in (run(lambda ft: ft.set_step_objective(A.StepObjective.SQUARE)), run(there_and_back)):
        assert plain[0] == other[0] and _same(plain[1], other[1])
        assert plain[2] == other[2] == 1 and plain[3] == other[3]
        for key in plain[4]:
            assert np.array_equal(plain[4][key], other[4][key], equal_nan=True), key
    assert U.ACCEPT in [r[3] for r in plain[0]]


def test_refusals_and_acceptances(nn):
    A = nn.alignment
    SQUARE, ROBUST, IRLS, REFERENCE = A.StepObjective.SQUARE, A.StepObjective.ROBUST, A.PenaltyForm.IRLS, A.PenaltyForm.REFERENCE
    modes = [A.IterationMode.ALL]
    # SQUARE: refused exactly as before, in both orders
    ft = A.DeformableMeshToImageFitter(1, modes, penalty_form=IRLS)
    assert ft.step_objective == SQUARE
    with pytest.raises(RuntimeError, match="SQUARE penalties only"):
        ft.set_step_control(A.StepControl())
    ft = A.DeformableMeshToImageFitter(1, modes)
    ft.set_step_control(A.StepControl())
    with pytest.raises(RuntimeError, match="IRLS is refused while step control is on"):
        ft.set_robust_options(IRLS, False)
    # ROBUST: accepted together, IRLS first ...
    ft = A.DeformableMeshToImageFitter(1, modes, use_tukey_penalty_for_data_term=True, penalty_form=IRLS, step_objective=ROBUST)
    ft.set_step_control(A.StepControl())
    assert (ft.step_objective, ft.robust_options[0], ft.step_control is not None) == (ROBUST, IRLS, True)
    # ... and back to SQUARE is refused while both are on
    with pytest.raises(RuntimeError, match="NNRT_STEP_OBJECTIVE_SQUARE is refused"):
        ft.set_step_objective(SQUARE)
    assert ft.step_objective == ROBUST
    ft.set_step_control(None)
    ft.set_step_objective(SQUARE)
    # ... or step control first
    ft = A.DeformableMeshToImageFitter(1, modes, use_huber_penalty_for_arap_term=True, penalty_form=IRLS)
    ft.set_robust_options(REFERENCE, True)
    with pytest.raises(RuntimeError, match="NNRT_PENALTY_REFERENCE and a penalty enabled"):   # A8 / A9 have no objective
        ft.set_step_objective(ROBUST)
    ft.set_step_control(A.StepControl())
    ft.set_robust_options(REFERENCE, False)
    with pytest.raises(RuntimeError, match="IRLS"):
        ft.set_robust_options(IRLS, False)   # still SQUARE
    ft.set_step_control(None)
    ft.set_robust_options(IRLS, False)
    ft.set_step_objective(ROBUST)
    ft.set_step_control(A.StepControl())
    with pytest.raises(RuntimeError, match="NNRT_PENALTY_REFERENCE with a penalty enabled"):
        ft.set_robust_options(REFERENCE, False)
    assert ft.robust_options == (IRLS, False)
    ft.set_robust_options(IRLS, True)   # under ROBUST with step control on
    # without a penalty enabled REFERENCE is a square term: ROBUST takes it
    ft = A.DeformableMeshToImageFitter(1, modes, step_objective=ROBUST)
    ft.set_step_control(A.StepControl())
    assert ft.robust_options[0] == REFERENCE
    ft.set_robust_options(IRLS, False)   # and IRLS after step control, the other order
    assert (ft.step_objective, ft.robust_options[0], ft.step_control is not None) == (ROBUST, IRLS, True)
    with pytest.raises(RuntimeError, match="objective must be"):
        ft.set_step_objective(2)
    from dynamicfuion_python_amd import _native as N
    out = np.zeros(4, np.float32)
    with pytest.raises(RuntimeError, match="prepared frame"):
        N.check(N.lib().nnrt_fitter_get_raw_residuals(ft._h, N.ptr(out), 4, None))


def test_switching_with_cached_graphs_equals_a_fresh_fitter(nn, scenes):
    A = nn.alignment
    scene, coupled, settings, iterations, threshold = U.CONFIGS["S1_coupled"]
    sc, depth = scenes[scene]
    wf, ft = _fitter(nn, sc, coupled, settings, iterations, threshold, graph=2, irls=False)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, iterations)
    fresh = _rows(ft.step_history()), _motion(wf), ft.raw_residuals()
    assert ft.graph_count == 1
    # the same fit through a fitter that ran it under the SQUARE objective first and holds that sequence's graph
    wf, ft = _fitter(nn, sc, coupled, settings, iterations, threshold, graph=2, robust=False, irls=False)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 3)
    assert ft.graph_count == 1 and len(ft.step_history()) == 3
    ft.set_step_objective(A.StepObjective.ROBUST)
    assert ft.graph_count == 0
    with pytest.raises(RuntimeError, match="prepare"):   # the state machine restarts in prepare()
        ft.iterate(wf, 3, 1)
    wf.reset_motion()
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    assert ft.step_history() == []
    ft.iterate(wf, 0, iterations)
    ft.check()
    assert ft.graph_count == 1
    assert _rows(ft.step_history()) == fresh[0] and _same(_motion(wf), fresh[1])
    assert np.array_equal(_bits(ft.raw_residuals()), _bits(fresh[2]))


# ---- 8. the pipeline -------------------------------------------------------------------------------------------------------
def test_pipeline_runs_the_real_sequence_recipe(nn):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.alignment.render_based.rendering_alignment_optimizer import PenaltyFunction
    from dynamicfuion_python_amd.data import frame as dfr
    A = nn.alignment
    dd = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepdeform")
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=dd, frame_indices=[300, 600])
    params = F.FusionParameters(step_control=A.StepControl(increase=10.0, decrease=0.5, lambda_max=1e4), coupled_data_term=True,
                                step_objective=A.StepObjective.ROBUST)
    params.alignment = dataclasses.replace(params.alignment, data_term_penalty_function=PenaltyFunction.TUKEY,
                                           regularization_term_penalty_function=PenaltyFunction.HUBER, penalty_form=A.PenaltyForm.IRLS,
                                           guard_zero_rotation=True, max_iteration_count=4)
    pipe = F.FusionPipeline(seq, params)
    pipe.process_frame(seq.get_next_frame())
    res = pipe.process_frame(seq.get_next_frame())
    fitter = pipe.optimizer.fitter
    assert fitter.step_objective == A.StepObjective.ROBUST and fitter.robust_options == (A.PenaltyForm.IRLS, True)
    history = fitter.step_history()
    print("decisions", [int(r.decision) for r in history], "cost", [f"{r.cost:.5g}" for r in history],
          "lambda", [float(np.float32(r.lambda_used)) for r in history])
    assert res.tracked and len(history) == 4
    assert 0 < res.final_cost <= history[0].cost
    assert np.isfinite(pipe.active_graph.get_node_translations(True)).all()
    assert np.isfinite(pipe.active_graph.get_node_rotations(True)).all()
