"""GPU tests of the fitter's on-device step control (nnrt_fitter_set_step_control) against the float64
restatement of tests/_step_control_util.py (checked in tests/test_step_control_cpu.py, which also holds every decision
of the configurations below to a 1e-2 margin). Scenes: S1 (96 x 128, 24 nodes: block-diagonal and coupled steps; its cost
sum takes three workgroups) and S1_ARAP (48 nodes, 2 layers: arrowhead and coupled steps, the edge residuals in the cost)."""
import ctypes
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _step_control_util as U   # noqa: E402
from _coupled_util import data_system   # noqa: E402
from _robust_util import arap_term   # noqa: E402
from _util import scene_target   # noqa: E402

pytestmark = pytest.mark.gpu

# The cost of every iteration against the restatement's own trajectory, relative. Measured: 2.2e-6
# (S1 block-diagonal), 1.4e-5 (S1 coupled), 4.8e-5 (S1_ARAP arrowhead), 1.4e-5 (S1_ARAP coupled); the bar is ten times the
# largest, and stays below the 1e-3 cap (itself below the 1e-2 decision margin, so the bar cannot hide a flipped decision).
COST_BAR = min(10 * 4.8e-5, 1e-3)


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
def restated(oracle_mod, scenes):
    """The restatement's run of every configuration, computed once."""
    out = {}
    for name, (scene, coupled, settings, iterations, threshold) in U.CONFIGS.items():
        sc, depth = scenes[scene]
        out[name] = U.run(oracle_mod, sc, depth, coupled, settings, iterations, minimal_update_threshold=threshold)
    return out


def _fitter(nn, sc, coupled, settings, iterations, threshold=1e-6, graph=0, lm=U.LM, **kw):
    G, A = nn.geometry, nn.alignment
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)
    ft = A.DeformableMeshToImageFitter(iterations, [A.IterationMode.ALL], minimal_update_threshold=threshold,
                                       preconditioning_dampening_factor=lm, use_hip_graph=graph, **kw)
    if coupled:
        ft.set_data_coupling(A.DataCoupling.COUPLED)
    if settings is not None:
        ft.set_step_control(A.StepControl(**settings))
    return wf, ft


def _mesh(nn, sc):
    return nn.geometry.TriangleMesh(sc.points, sc.normals, sc.faces)


def _motion(wf):
    return wf.get_node_rotations(True), wf.get_node_translations(True)


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def _as32(c):
    """A StepControl as the C struct holds it (float32 fields)."""
    return tuple(np.float32(v) for v in (c.initial_lambda, c.increase, c.decrease, c.lambda_min, c.lambda_max, c.relative_cost_tolerance)) + (c.poll_interval,)


def _rows(history):
    return [(r.iteration, r.cost, np.float32(r.lambda_used), int(r.decision), r.max_update) for r in history]


# ---- 1. the state machine, iteration by iteration ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CONFIGS))
def test_trajectory_equals_the_restatement(nn, oracle_mod, scenes, restated, name):
    scene, coupled, settings, iterations, threshold = U.CONFIGS[name]
    sc, depth = scenes[scene]
    want = restated[name]
    wf, ft = _fitter(nn, sc, coupled, settings, iterations, threshold)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    before, best, host_err, arap_err, edges_max = _motion(wf), None, 0.0, 0.0, 0.0
    for k in range(iterations):
        ft.iterate(wf, k, 1)
        rec = ft.step_history()[-1]
        after = _motion(wf)
        # the fixed-order fp64 sum against the host's sum of the same exported float32 residuals
        dg = ft.diagnostics()
        host = float((dg["residuals"][dg["residual_mask"]].astype(np.float64) ** 2).sum())
        if not sc.hierarchy:
            host_err = max(host_err, abs(rec.cost - host) / host)
        else:
            # the edge residuals are not exported: what the device's sum holds beyond the pixels' part (the chunk that
            # straddles the end of the image included) against the oracle's float32 edge residuals at the same motion
            edges = float((np.asarray(arap_term(oracle_mod, sc, before[0], before[1])["residuals"], np.float32).astype(np.float64) ** 2).sum())
            edges_max = max(edges_max, edges)
            arap_err = max(arap_err, abs((rec.cost - host) - edges) / rec.cost)
        if rec.decision in (U.START, U.ACCEPT):
            best = before   # the state this iteration started from
        if rec.decision in (U.HOLD, U.REJECT, U.REJECT_FINAL):
            assert _same(after, best), f"iteration {k}: the motion after a held iteration is not the best snapshot"
        else:
            assert not _same(after, before), k
        before = after
    ft.check()
    got = ft.step_history()
    assert [r.iteration for r in got] == list(range(iterations))
    print(f"{name}: decisions {[int(r.decision) for r in got]}")
    print(f"  lambda {[float(np.float32(r.lambda_used)) for r in got]}")
    cost_err = max(abs(g.cost - w["cost"]) / w["cost"] for g, w in zip(got, want))
    step_err = max(abs(g.max_update - w["max_update"]) / w["max_update"] for g, w in zip(got, want) if w["max_update"] > 0)
    print(f"  cost vs the restatement's trajectory: {cost_err:.3g} relative (bar {COST_BAR:.3g}); max |update| {step_err:.3g}; "
          f"device sum vs host sum of the exported residuals {host_err:.3g} (S1 only); the sum's ARAP part vs the oracle's edge "
          f"residuals {arap_err:.3g} of the cost (S1_ARAP only)")
    assert [int(r.decision) for r in got] == [w["decision"] for w in want]
    assert [np.float32(r.lambda_used) for r in got] == [w["lambda_used"] for w in want]
    assert host_err <= 1e-12   # the 1e-12 check proper: scenes without a hierarchy, whose whole sum the host can repeat
    assert arap_err <= COST_BAR and (edges_max > 0) == bool(sc.hierarchy)   # some rejected state has stretched edges
    assert cost_err <= COST_BAR
    s = ft.step_summary()
    assert (s["iterations_used"], s["rejected_step_count"]) == (U.summarize(want)[0], U.summarize(want)[2])
    assert abs(s["final_cost"] - want[-1]["c_best"]) <= COST_BAR * want[-1]["c_best"]


# ---- 2. error bits: a held iteration's are discarded, a stepping iteration's stay ------------------------------------------
def _mask_one_node(oracle_mod, sc, depth):
    """`depth` with every pixel zeroed whose face anchors to the node with the fewest contributing pixels: that node's
    data block and gradient are exactly zero."""
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


def test_held_iterations_error_bits_are_discarded(nn, oracle_mod, scenes):
    """S1_ARAP, arrowhead solve, ARAP weight 0, one node's pixels masked out, no zero-rotation guard. That node's block is
    lambda I with a zero right-hand side: its rotation update is exactly 0 and Rodrigues makes its rotation NaN (SURVEY
    A7), raising nothing. The next iteration starts from that state: 0 * NaN makes the node's edge terms NaN, so the cost
    is not a number (a reject) and the diagonal blocks k_arrow_prepare forms are not positive definite: the HELD
    iteration's solve raises the potrf bit. First without step control, to show that the second iteration is what raises
    it; then with it: every retry ends the same way up to lambda_max, and check() is clean."""
    sc, depth = scenes["S1_ARAP"]
    masked = _mask_one_node(oracle_mod, sc, depth)
    mesh = _mesh(nn, sc)
    wf, ft = _fitter(nn, sc, False, None, 2, lm=0.01, arap_term_weight=0.0)
    ft.prepare(wf, mesh, masked, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 1)
    ft.check()   # the stepping solve is clean
    assert np.isnan(_motion(wf)[0]).any()
    ft.iterate(wf, 1, 1)
    with pytest.raises(RuntimeError, match="positive-definite"):
        ft.check()   # the solve linearised at the NaN state is not
    wf, ft = _fitter(nn, sc, False, U.control(increase=10.0, decrease=0.5, lambda_max=0.1), 8, arap_term_weight=0.0)
    ft.prepare(wf, mesh, masked, None, sc.K, None, 1.0)
    start = _motion(wf)
    ft.iterate(wf, 0, 8)
    got = ft.step_history()
    print("decisions", [int(r.decision) for r in got], "cost", [f"{r.cost:.4g}" for r in got])
    assert [int(r.decision) for r in got] == [U.START, U.REJECT, U.START, U.REJECT, U.START, U.REJECT_FINAL, U.HOLD, U.HOLD]
    assert all(np.isnan(got[k].cost) for k in (1, 3, 5))   # the rejected states are the NaN ones: their held solves fail
    ft.check()   # and nothing of that is left
    assert _same(_motion(wf), start) and np.isfinite(_motion(wf)[0]).all()


def test_stepping_iterations_error_bits_survive(nn, oracle_mod, scenes):
    """S1, block-diagonal, lambda = 0 throughout (lambda_min 0), one node's pixels masked out: that node's block is zero
    and the potrf bit is raised by the solve of every STEPPING iteration, the first included. The holds that follow put
    the error word back as it stood at their decision, which holds that bit: check() reports it."""
    sc, depth = scenes["S1"]
    masked = _mask_one_node(oracle_mod, sc, depth)
    wf, ft = _fitter(nn, sc, False, U.control(lambda_min=0.0, lambda_max=1.0), 4, lm=0.0)
    ft.prepare(wf, _mesh(nn, sc), masked, None, sc.K, None, 1.0)
    ft.iterate(wf, 0, 4)
    got = ft.step_history()
    print("decisions", [int(r.decision) for r in got], "cost", [f"{r.cost:.4g}" for r in got])
    assert int(got[0].decision) == U.START and any(int(r.decision) in (U.REJECT, U.HOLD) for r in got[1:])
    with pytest.raises(RuntimeError, match="positive-definite"):
        ft.check()


# ---- 3. graph replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1_coupled", "S1_ARAP_arrowhead"])
def test_graph_replay_equals_eager(nn, scenes, name):
    scene, coupled, settings, iterations, threshold = U.CONFIGS[name]
    sc, depth = scenes[scene]
    runs = []
    for graph in (0, 2):
        wf, ft = _fitter(nn, sc, coupled, settings, iterations, threshold, graph=graph)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, iterations)
        ft.check()
        runs.append((_rows(ft.step_history()), _motion(wf), ft.graph_count))
    assert runs[0][0] == runs[1][0]   # cost, lambda, decision and max |update| of every iteration, bit for bit
    assert _same(runs[0][1], runs[1][1])
    assert (runs[0][2], runs[1][2]) == (0, 1)


# ---- 4. host early exit, and minimal_update_threshold ----------------------------------------------------------------------
def test_early_exit_and_update_threshold(nn, scenes):
    sc, depth = scenes["S1"]
    mesh, out = _mesh(nn, sc), []
    for poll in (0, 2):
        settings = U.control(increase=10.0, decrease=0.1, lambda_max=10.0, poll_interval=poll)
        wf, ft = _fitter(nn, sc, True, settings, 7, threshold=1e3)   # every update is below 1e3
        start = _motion(wf)
        ft.fit_to_image(wf, mesh, None, depth, None, sc.K, None, 1.0)
        got = ft.step_history()
        assert int(got[0].decision) == U.SMALL_UPDATE and 0 < got[0].max_update < 1e3
        assert all(int(r.decision) == U.HOLD for r in got[1:])
        assert _same(_motion(wf), start)   # done after the first step, on the starting state
        s = ft.step_summary()
        assert s["done"] and s["iterations_used"] == 1 <= 7
        out.append((_motion(wf), len(got)))
    assert _same(out[0][0], out[1][0])
    assert out[0][1] == 7 and out[1][1] == 2   # the polled fit stopped after its first two iterations


def test_early_exit_keeps_the_result(nn, scenes):
    """A fit that ends by rejection at lambda_max: polled every two iterations it returns the motion of the unpolled fit."""
    scene, coupled, settings, _, threshold = U.CONFIGS["S1_block"]
    sc, depth = scenes[scene]
    out = []
    for poll in (0, 2):
        wf, ft = _fitter(nn, sc, coupled, dict(settings, poll_interval=poll), 20, threshold)
        ft.fit_to_image(wf, _mesh(nn, sc), None, depth, None, sc.K, None, 1.0)
        s = ft.step_summary()
        out.append((_motion(wf), len(ft.step_history()), s))
        assert s["done"] and s["iterations_used"] <= 20
    assert _same(out[0][0], out[1][0])
    assert out[0][2] == out[1][2]
    assert out[1][1] < out[0][1] == 20


def test_native_fit_to_image_polls(nn, scenes):
    """nnrt_fitter_fit_to_image's own loop (the Python fit_to_image runs prepare() and iterate() itself): polled every two
    iterations it stops once the device reports done, on the motion of the unpolled call, and its check() is clean."""
    from dynamicfuion_python_amd import _native as N
    scene, coupled, settings, _, threshold = U.CONFIGS["S1_block"]
    sc, depth = scenes[scene]
    out = []
    for poll in (0, 2):
        wf, ft = _fitter(nn, sc, coupled, dict(settings, poll_interval=poll), 20, threshold)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)   # uploads the frame's inputs; the native call prepares again
        p, n, f, d, m, K, E, H, W = ft._frame
        N.check(N.lib().nnrt_fitter_fit_to_image(ft._h, wf.handle, N.ptr(p), N.ptr(n), p.shape[0], N.ptr(f), f.shape[0], N.ptr(d), N.ptr(m),
                                                 H, W, N.ptr(K), N.ptr(E), 1.0, N.stream_ptr(None)))
        out.append((_motion(wf), _rows(ft.step_history())))
    assert _same(out[0][0], out[1][0])
    assert len(out[0][1]) == 20 and len(out[1][1]) == 14   # done at iteration 12 (REJECT_FINAL), seen after iteration 13
    assert out[1][1] == out[0][1][:14]
    assert out[0][1][12][3] == U.REJECT_FINAL


# ---- 5. the default is untouched ----------------------------------------------------------------------------------------
def test_default_untouched(nn, scenes):
    from dynamicfuion_python_amd import _native
    sc, depth = scenes["S1"]
    A = nn.alignment

    def run(prep):
        gc.collect()
        torch.cuda.synchronize()
        bytes_before = _native.lib().nnrt_device_bytes_in_use()
        wf, ft = _fitter(nn, sc, False, None, 2, graph=2)
        prep(wf, ft)
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, 2)
        ft.check()
        out = ft.diagnostics(), _motion(wf), ft.graph_count, ft.launch_plan(), ft.step_history(), ft.step_control
        del ft, wf
        gc.collect()
        return out + (_native.lib().nnrt_device_bytes_in_use() - bytes_before,)

    def there_and_back(wf, ft):
        ft.set_step_control(A.StepControl())
        assert _as32(ft.step_control) == _as32(A.StepControl())
        ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
        ft.iterate(wf, 0, 1)
        assert len(ft.step_history()) == 1
        ft.set_step_control(None)
        with pytest.raises(RuntimeError):   # the setter invalidated the prepared frame
            ft.iterate(wf, 0, 1)
        wf.reset_motion()

    fresh = run(lambda wf, ft: None)
    other = run(there_and_back)
    for key in fresh[0]:
        assert np.array_equal(fresh[0][key], other[0][key], equal_nan=True), key
    assert _same(fresh[1], other[1])
    assert fresh[2] == other[2] == 1 and fresh[3] == other[3]
    assert fresh[4] == other[4] == [] and fresh[5] is None and other[5] is None
    assert fresh[6] == other[6] == 0


# ---- 6. the refusals ------------------------------------------------------------------------------------------------------
def test_refusals(nn, scenes):
    A = nn.alignment
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], penalty_form=A.PenaltyForm.IRLS)
    with pytest.raises(RuntimeError, match="IRLS"):
        ft.set_step_control(A.StepControl())
    assert ft.step_control is None
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL])
    ft.set_step_control(A.StepControl())
    with pytest.raises(RuntimeError, match="IRLS"):
        ft.set_robust_options(A.PenaltyForm.IRLS, False)
    assert ft.robust_options == (A.PenaltyForm.REFERENCE, False)
    ft.set_robust_options(A.PenaltyForm.REFERENCE, True)
    with pytest.raises(RuntimeError, match="increase"):
        ft.set_step_control(A.StepControl(increase=1.0))
    assert _as32(ft.step_control) == _as32(A.StepControl())
    ft = A.DeformableMeshToImageFitter(2, [A.IterationMode.ALL, A.IterationMode.TRANSLATION_ONLY])
    with pytest.raises(RuntimeError, match="ALL only"):
        ft.set_step_control(A.StepControl())
    # every iteration a restart: refused while the mode is on; and a history buffer that is too small
    sc, depth = scenes["S1"]
    wf, ft = _fitter(nn, sc, False, U.control(), 2)
    ft.prepare(wf, _mesh(nn, sc), depth, None, sc.K, None, 1.0)
    with pytest.raises(RuntimeError, match="step control"):
        ft.iterate_from_identity(wf, 0, 1)
    ft.iterate(wf, 0, 2)
    from dynamicfuion_python_amd import _native as N
    rec, n = (N.StepRecord * 2)(), ctypes.c_int64()
    rec[0].iteration = 77
    assert N.lib().nnrt_fitter_get_step_history(ft._h, rec, 1, ctypes.byref(n), None) == 1
    assert n.value == 2 and rec[0].iteration == 77   # refused, the count reported, nothing written
    assert N.lib().nnrt_fitter_get_step_history(ft._h, rec, 2, ctypes.byref(n), None) == 0 and rec[1].iteration == 1


# ---- 7. the pipeline -------------------------------------------------------------------------------------------------------
def test_pipeline_reports_the_fit(nn):
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    A = nn.alignment
    dd = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepdeform")
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=dd, frame_indices=[300, 600])
    params = F.FusionParameters(step_control=A.StepControl(increase=10.0, decrease=0.5, lambda_max=1e4), coupled_data_term=True)
    params.alignment.max_iteration_count = 4
    pipe = F.FusionPipeline(seq, params)
    first = pipe.process_frame(seq.get_next_frame())
    assert (first.iterations_used, first.final_cost, first.rejected_step_count) == (0, 0.0, 0)   # nothing was fitted
    res = pipe.process_frame(seq.get_next_frame())
    history = pipe.optimizer.fitter.step_history()
    print("decisions", [int(r.decision) for r in history], "cost", [f"{r.cost:.5g}" for r in history])
    assert res.tracked and len(history) == 4
    assert 1 <= res.iterations_used <= 4
    assert 0 < res.final_cost <= history[0].cost
    assert res.rejected_step_count == sum(int(r.decision) in (U.REJECT, U.REJECT_FINAL) for r in history)
    assert np.isfinite(pipe.active_graph.get_node_translations(True)).all()
