"""CPU checks of the fitter's step control (nnrt_fitter_set_step_control): the float64 restatement in
tests/_step_control_util.py keeps its invariants on S1 and S1_ARAP, every decision the GPU tests repeat has a margin the
GPU's float error cannot cross, and the switch exists through the C ABI and the Python layers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _step_control_util as U   # noqa: E402
from _coupled_util import data_system   # noqa: E402
from _util import scene_target   # noqa: E402


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
def histories(oracle_mod, scenes):
    """The restatement's run of every configuration the GPU tests use, and the two longer S1 runs of the invariants."""
    out = {}
    for name, (scene, coupled, settings, iterations, threshold) in U.CONFIGS.items():
        sc, depth = scenes[scene]
        out[name] = U.run(oracle_mod, sc, depth, coupled, settings, iterations, minimal_update_threshold=threshold)
    sc, depth = scenes["S1"]
    out["block_24"] = U.run(oracle_mod, sc, depth, False, U.control(increase=10.0, decrease=0.5, lambda_max=10.0), 24)
    out["coupled_10"] = U.run(oracle_mod, sc, depth, True, U.control(increase=10.0, decrease=0.1, lambda_max=10.0), 10)
    return out


# ---- the restatement's invariants -------------------------------------------------------------------------------------
def test_best_cost_never_rises(histories):
    for name, h in histories.items():
        best = [r["c_best"] for r in h]
        print(name, "decisions", [r["decision"] for r in h], "c_best", [f"{c:.4g}" for c in best])
        assert all(b <= a for a, b in zip(best, best[1:])), name
        assert h[0]["decision"] == U.START


def test_held_state_re_evaluates_to_the_best_cost(oracle_mod, scenes, histories):
    sc, depth = scenes["S1"]
    h = histories["block_24"]
    assert h[-1]["decision"] == U.HOLD and any(r["decision"] == U.REJECT_FINAL for r in h)
    R, t = h[-1]["state"]
    assert data_system(oracle_mod, sc, depth, R, t)["cost"] == h[-1]["c_best"]
    # every rejected and every held iteration leaves the best state
    for r in h:
        if r["decision"] in (U.HOLD, U.REJECT, U.REJECT_FINAL):
            assert r["state"][0] is r["best"][0] and r["state"][1] is r["best"][1]


def test_block_diagonal_ends_below_its_start(histories):
    h = histories["block_24"]
    print("block-diagonal, 24 iterations:", [f"{r['cost']:.4g}" for r in h])
    assert abs(h[0]["cost"] - 0.1521) < 1e-4
    assert h[-1]["c_best"] < h[0]["cost"]
    assert U.summarize(h)[2] >= 4   # the unguarded step is rejected until the damping holds it


def test_coupled_rejects_the_rising_step(histories):
    h = histories["coupled_10"]
    costs = [r["cost"] for r in h]
    print("coupled, 10 iterations:", [f"{c:.4g}" for c in costs], [r["decision"] for r in h])
    assert [r["decision"] for r in h[:7]] == [U.START] + [U.ACCEPT] * 5 + [U.REJECT]
    assert abs(costs[5] - 0.001319) < 2e-6 and abs(costs[6] - 0.001423) < 2e-6
    assert h[-1]["c_best"] == costs[5]
    R, t = h[6]["state"]
    assert R is h[5]["best"][0] or np.array_equal(R, h[6]["best"][0])


def test_decision_margins(histories):
    """Every accept / reject decision of a configuration the GPU repeats differs from the best cost by >= 1e-2 relative
    (the first and the retry iterations, where c = c_best by construction, take none)."""
    for name in U.CONFIGS:
        margins = U.decision_margins(histories[name])
        print(name, [(i, f"{m:.3g}") for i, m in margins])
        assert margins, name
        assert min(m for _, m in margins) >= U.DECISION_MARGIN, name
        assert not any(r["decision"] in (U.CONVERGED, U.SMALL_UPDATE) for r in histories[name]), name


def test_configurations_cover_the_state_machine(histories):
    seen = {name: {r["decision"] for r in histories[name]} for name in U.CONFIGS}
    assert {U.START, U.ACCEPT, U.REJECT, U.REJECT_FINAL, U.HOLD} <= seen["S1_block"]
    assert {U.START, U.ACCEPT, U.REJECT} <= seen["S1_coupled"]
    for name in ("S1_ARAP_arrowhead", "S1_ARAP_coupled"):
        assert {U.START, U.REJECT} <= seen[name]


def test_summary_matches_the_python_layer(histories):
    from dynamicfuion_python_amd.nnrt import alignment as A
    for name, h in histories.items():
        recs = [A.StepRecord(r["iteration"], r["cost"], float(r["lambda_used"]), A.StepDecision(r["decision"]), r["max_update"]) for r in h]
        s = A.summarize_step_history(recs)
        assert (s["iterations_used"], s["final_cost"], s["rejected_step_count"]) == U.summarize(h), name
        assert s["final_cost"] == h[-1]["c_best"] and s["iterations_used"] <= len(h)
    assert A.summarize_step_history([]) == dict(iterations_used=0, final_cost=0.0, rejected_step_count=0, done=False)


# ---- the switch through the layers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    return _native


NEW_SYMBOLS = ("nnrt_fitter_set_step_control", "nnrt_fitter_get_step_control", "nnrt_fitter_get_step_history")


def test_symbols_signatures_and_header(native):
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported
    lib = native.lib()
    c_int32, c_int64, c_void_p, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER
    assert list(lib.nnrt_fitter_set_step_control.argtypes) == [c_void_p, P(native.StepControlSettings)]
    assert list(lib.nnrt_fitter_get_step_control.argtypes) == [c_void_p, P(c_int32), P(native.StepControlSettings)]
    assert list(lib.nnrt_fitter_get_step_history.argtypes) == [c_void_p, P(native.StepRecord), c_int64, P(c_int64), c_void_p]
    assert [f[0] for f in native.StepControlSettings._fields_] == ["initial_lambda", "increase", "decrease", "lambda_min", "lambda_max",
                                                                    "relative_cost_tolerance", "poll_interval"]
    assert ctypes.sizeof(native.StepControlSettings) == 28 and ctypes.sizeof(native.StepRecord) == 24
    header = open(os.path.join(os.path.dirname(native.LIB_PATH), "..", "include", "nnrt_mi355x.h")).read()
    for name in NEW_SYMBOLS + ("nnrt_step_control", "nnrt_step_record"):
        assert name in header
    for i, name in enumerate(("HOLD", "START", "ACCEPT", "CONVERGED", "REJECT", "REJECT_FINAL", "SMALL_UPDATE")):
        assert f"#define NNRT_STEP_{name} {i}" in header
    assert f"#define NNRT_STEP_HISTORY_CAPACITY {native.STEP_HISTORY_CAPACITY}" in header
    # the limits are stated where the caller reads them
    assert "SQUARE penalties only" in header and "IterationMode ALL only" in header
    assert "setting NNRT_PENALTY_IRLS while step control is on, returns NNRT_ERROR_ARGUMENT" in header


def _settings(native, **kw):
    v = dict(initial_lambda=0.0, increase=10.0, decrease=0.5, lambda_min=1e-6, lambda_max=1.0, relative_cost_tolerance=1e-4, poll_interval=0)
    v.update(kw)
    return native.StepControlSettings(*[v[f[0]] for f in native.StepControlSettings._fields_])


def test_null_fitter_is_refused(native):
    lib = native.lib()
    on, n = ctypes.c_int32(7), ctypes.c_int64(7)
    good = _settings(native)
    assert lib.nnrt_fitter_set_step_control(None, ctypes.byref(good)) == 1   # NNRT_ERROR_ARGUMENT
    assert b"null pointer" in lib.nnrt_last_error()
    assert lib.nnrt_fitter_set_step_control(None, None) == 1
    assert lib.nnrt_fitter_get_step_control(None, ctypes.byref(on), None) == 1 and on.value == 7
    rec = (native.StepRecord * 4)()
    assert lib.nnrt_fitter_get_step_history(None, rec, 4, ctypes.byref(n), None) == 1 and n.value == 7


@pytest.mark.parametrize("field,value", [("increase", 1.0), ("increase", 0.5), ("increase", float("nan")), ("decrease", 0.0),
                                         ("decrease", 1.5), ("decrease", float("nan")), ("initial_lambda", -1.0),
                                         ("lambda_min", -1e-3), ("lambda_max", 0.0), ("lambda_max", float("inf")),
                                         ("relative_cost_tolerance", -1.0), ("poll_interval", -1)])
def test_out_of_range_settings_are_refused(native, field, value):
    """The ranges are checked before the handle, so the refusal names the field even here, without a device."""
    lib = native.lib()
    bad = _settings(native, **{field: value})
    assert lib.nnrt_fitter_set_step_control(None, ctypes.byref(bad)) == 1
    message = lib.nnrt_last_error().decode()
    assert "step control" in message and field.split("_")[0] in message, message


def test_lambda_min_above_lambda_max_is_refused(native):
    lib = native.lib()
    bad = _settings(native, lambda_min=2.0, lambda_max=1.0)
    assert lib.nnrt_fitter_set_step_control(None, ctypes.byref(bad)) == 1
    assert "lambda_min" in lib.nnrt_last_error().decode()


class _FakeFitter:
    """Stands in for the native fitter: records what the Python layers hand down."""
    made = []

    def __init__(self, *a, **kw):
        self.kw, self.control = kw, None
        _FakeFitter.made.append(self)

    def set_data_coupling(self, v):
        self.coupling = v

    def set_step_control(self, v):
        self.control = v


def test_parameters_reach_the_fitter(monkeypatch):
    import dataclasses
    from dynamicfuion_python_amd.alignment.render_based import rendering_alignment_optimizer as rao
    from dynamicfuion_python_amd.fusion import pipeline as P
    from dynamicfuion_python_amd.nnrt import alignment as A
    assert issubclass(A.StepDecision, int) and [d.value for d in A.StepDecision] == list(range(7))
    assert dataclasses.is_dataclass(A.StepControl)
    assert rao.RenderingAlignmentParameters().step_control is None
    assert P.FusionParameters().step_control is None
    r = P.FrameResult(0)
    assert (r.iterations_used, r.final_cost, r.rejected_step_count) == (0, 0.0, 0)
    monkeypatch.setattr(A, "DeformableMeshToImageFitter", _FakeFitter)
    K = np.array([[100.0, 0, 32], [0, 100.0, 24], [0, 0, 1]])
    _FakeFitter.made.clear()
    c1, c2 = A.StepControl(increase=4.0), A.StepControl(decrease=0.25, poll_interval=2)
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, rao.RenderingAlignmentParameters(step_control=c1))
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters(step_control=c2, coupled_data_term=True)))
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters()))
    assert [f.control for f in _FakeFitter.made] == [c1, c2, None]
    assert _FakeFitter.made[1].coupling == A.DataCoupling.COUPLED


def test_python_methods_exist():
    from dynamicfuion_python_amd.nnrt import alignment as A
    F = A.DeformableMeshToImageFitter
    assert callable(F.set_step_control) and callable(F.step_history) and callable(F.step_summary)
    assert isinstance(F.step_control, property)
