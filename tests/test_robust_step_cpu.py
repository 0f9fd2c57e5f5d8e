"""CPU checks of step control under the robust step objective (nnrt_fitter_set_step_objective): the
restated robust cost of tests/_robust_step_util.py keeps its limits, every decision the GPU tests repeat has a margin the
GPU's float error cannot cross, the robust run beats the square one on the outlier scene, and the switch exists through
the C ABI and the Python layers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _robust_step_util as RU   # noqa: E402
import _step_control_util as U   # noqa: E402
from _robust_util import F32, huber_scale, patch_targets   # noqa: E402
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
    return {name: RU.run_config(oracle_mod, scenes, name) for name in RU.CONFIGS_ROBUST}


# ---- the restated cost ------------------------------------------------------------------------------------------------
def test_robust_cost_tends_to_the_square_cost():
    rng = np.random.default_rng(0)
    r = rng.normal(0, 0.02, 4000).astype(F32)
    mask = rng.random(4000) < 0.8
    e = rng.normal(0, 0.1, (300, 3)).astype(F32)
    square = float((r[mask].astype(np.float64) ** 2).sum()) + float((e.astype(np.float64) ** 2).sum())
    assert RU.robust_cost(r, mask, None, e, None) == pytest.approx(square, rel=1e-14)
    got = RU.robust_cost(r, mask, 1e6, e, 1e6)
    print("c, delta = 1e6:", got, "square", square)
    assert abs(got - square) <= 1e-12 * square
    stored = (e * huber_scale(e, 0.05)[0][:, None]).astype(F32)   # as the kernel stores them under delta = 0.05
    assert RU.robust_cost(r, mask, 0.03, stored, 0.05) < square   # and finite constants cost less


def test_tukey_saturates_beyond_the_cutoff():
    c = F32(0.03)
    c23 = float(c) ** 2 / 3.0
    r = np.array([0.0, 0.03, -0.03, np.nextafter(c, F32(1)), 0.5, -7.0, 1e30], F32)
    one = [RU.tukey_cost(r[k:k + 1], [True], c) for k in range(len(r))]
    assert one[0] == 0.0
    assert one[1] == pytest.approx(c23, rel=1e-12) and one[2] == pytest.approx(c23, rel=1e-12)   # continuous at the cutoff
    assert one[3:] == [c23] * 4
    assert RU.tukey_cost(r, np.zeros(len(r), bool), c) == 0.0
    # the literal form of the polynomial, where it does not cancel
    q = 0.6
    assert RU.tukey_cost(np.array([q * float(c)], F32), [True], c) == pytest.approx(c23 * (1 - (1 - q * q) ** 3), rel=1e-6)
    # a masked-in residual that is not finite is not a saturated finite cost
    for bad in (np.nan, np.inf, -np.inf):
        assert np.isnan(RU.tukey_cost(np.array([0.01, bad], F32), [True, True], c))
        assert np.isnan(RU.tukey_cost(np.array([0.01, bad], F32), [True, True], None))
    assert RU.tukey_cost(np.array([0.01, np.nan], F32), [True, False], c) > 0


def test_huber_from_stored_equals_huber_from_raw():
    """The stored entries are sqrt(delta / n) e where the raw norm n exceeds delta (float32, as the kernel scales them):
    2 m^2 - delta^2 from them equals 2 delta n - delta^2 from the raw norms."""
    rng = np.random.default_rng(1)
    raw = (rng.normal(0, 1, (2000, 3)) * rng.choice([1e-3, 0.03, 0.3, 3.0], (2000, 1))).astype(F32)
    delta = 0.05
    s, n = huber_scale(raw, delta)
    stored = (raw * s[:, None]).astype(F32)
    n64 = np.linalg.norm(raw.astype(np.float64), axis=1)
    want = np.where(n64 <= delta, n64 ** 2, 2 * delta * n64 - delta ** 2)
    assert 100 < (n > F32(delta)).sum() < 1900
    got = np.array([RU.huber_cost(stored[k], delta) for k in range(len(raw))])
    err = np.abs(got - want) / want
    print("largest relative error per edge", err.max(), "of the sum", abs(got.sum() - want.sum()) / want.sum())
    assert err.max() <= 1e-6
    assert abs(RU.huber_cost(stored, delta) - want.sum()) <= 1e-6 * want.sum()


# ---- the configurations the GPU repeats ---------------------------------------------------------------------------------
def test_cutoff_separates_inliers_from_the_patch(oracle_mod, scenes):
    from _robust_util import data_term
    for name in RU.CONFIGS_ROBUST:
        sc, A, c, _ = RU.config_inputs(oracle_mod, scenes, name)
        patch = patch_targets(scenes[RU.CONFIGS_ROBUST[name][0]][1])[2].reshape(-1)
        dg = data_term(oracle_mod, sc, A)
        r, m = np.abs(dg["r"]), dg["residual_mask"]
        assert (m & patch).sum() > 100
        assert r[m & ~patch].max() < c < r[m & patch].min(), name


def test_decision_margins_robust(histories):
    for name, h in histories.items():
        margins = RU.decision_margins(h)
        print(name, "decisions", [r["decision"] for r in h], "cost", [f"{r['cost']:.5g}" for r in h], [(i, f"{m:.3g}") for i, m in margins])
        assert margins, name
        assert min(m for _, m in margins) >= RU.DECISION_MARGIN, name
        assert not any(r["decision"] in (RU.CONVERGED, RU.SMALL_UPDATE) for r in h), name
        best = [r["c_best"] for r in h]
        assert all(b <= a for a, b in zip(best, best[1:])) and h[0]["decision"] == RU.START, name


def test_configurations_show_accept_and_reject(histories):
    seen = set()
    for h in histories.values():
        seen |= {r["decision"] for r in h}
    assert {RU.START, RU.ACCEPT, RU.REJECT} <= seen


def test_huber_is_exceeded(histories):
    name = "S1_ARAP_arrowhead"
    delta = RU.CONFIGS_ROBUST[name][5]
    norms = [r["edge_norm_max"] for r in histories[name]]
    print("largest raw edge norm per iteration", [f"{n:.3g}" for n in norms])
    assert max(norms) > 2 * delta


def test_robust_run_ends_closer_than_the_square_run(oracle_mod, scenes, histories):
    """S1, target A, coupled, the same start and settings: under the SQUARE objective with SQUARE penalties the patch's
    0.5 m residuals dominate the cost; under ROBUST with Tukey IRLS they carry no weight. The robust run ends at least
    twice as close to the ground-truth translations."""
    name = "S1_coupled"
    _, coupled, settings, iterations, _, _ = RU.CONFIGS_ROBUST[name]
    sc, A, _, _ = RU.config_inputs(oracle_mod, scenes, name)
    square = U.run(oracle_mod, sc, A, coupled, settings, iterations)
    e_square = RU.translation_error(sc, square[-1]["state"][1])
    e_robust = RU.translation_error(sc, histories[name][-1]["state"][1])
    print(f"RMS translation error: start {RU.translation_error(sc, np.zeros((len(sc.nodes), 3))):.4g}, SQUARE {e_square:.4g} "
          f"(decisions {[r['decision'] for r in square]}), ROBUST {e_robust:.4g}")
    assert 2.0 * e_robust <= e_square


# ---- the switch through the layers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    return _native


NEW_SYMBOLS = ("nnrt_fitter_set_step_objective", "nnrt_fitter_get_step_objective", "nnrt_fitter_get_raw_residuals")


def test_symbols_signatures_and_header(native):
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= exported
    lib = native.lib()
    c_int32, c_int64, c_void_p, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER
    assert list(lib.nnrt_fitter_set_step_objective.argtypes) == [c_void_p, c_int32]
    assert list(lib.nnrt_fitter_get_step_objective.argtypes) == [c_void_p, P(c_int32)]
    assert list(lib.nnrt_fitter_get_raw_residuals.argtypes) == [c_void_p, c_void_p, c_int64, c_void_p]
    # the structs keep their layouts
    assert ctypes.sizeof(native.StepControlSettings) == 28 and ctypes.sizeof(native.StepRecord) == 24
    assert ctypes.sizeof(native.FitterParams) == 29 * 4
    header = open(os.path.join(os.path.dirname(native.LIB_PATH), "..", "include", "nnrt_mi355x.h")).read()
    for name in NEW_SYMBOLS:
        assert name in header
    assert "#define NNRT_STEP_OBJECTIVE_SQUARE 0" in header and "#define NNRT_STEP_OBJECTIVE_ROBUST 1" in header
    flat = " ".join(header.replace("\n *", " ").split())
    assert "SQUARE penalties only under NNRT_STEP_OBJECTIVE_SQUARE" in flat
    assert "Under NNRT_STEP_OBJECTIVE_SQUARE, enabling step control while NNRT_PENALTY_IRLS is set" in flat
    assert "setting NNRT_PENALTY_IRLS while step control is on, returns NNRT_ERROR_ARGUMENT" in header


def test_argument_refusals_without_a_device(native):
    lib = native.lib()
    v = ctypes.c_int32(7)
    assert lib.nnrt_fitter_set_step_objective(None, 0) == 1 and b"null pointer" in lib.nnrt_last_error()
    assert lib.nnrt_fitter_set_step_objective(None, 1) == 1 and b"null pointer" in lib.nnrt_last_error()
    for bad in (-1, 2, 7):   # the range is checked before the handle
        assert lib.nnrt_fitter_set_step_objective(None, bad) == 1
        assert b"objective" in lib.nnrt_last_error() and b"NNRT_STEP_OBJECTIVE_ROBUST" in lib.nnrt_last_error()
    assert lib.nnrt_fitter_get_step_objective(None, ctypes.byref(v)) == 1 and v.value == 7
    out = np.full(4, 5.0, np.float32)
    assert lib.nnrt_fitter_get_raw_residuals(None, native.ptr(out), 4, None) == 1 and (out == 5.0).all()


class _FakeFitter:
    made = []

    def __init__(self, *a, **kw):
        self.kw, self.control = kw, None
        _FakeFitter.made.append(self)

    def set_data_coupling(self, v):
        self.coupling = v

    def set_step_control(self, v):
        self.control = v


def test_parameters_reach_the_fitter(monkeypatch):
    from dynamicfuion_python_amd.alignment.render_based import rendering_alignment_optimizer as rao
    from dynamicfuion_python_amd.fusion import pipeline as P
    from dynamicfuion_python_amd.nnrt import alignment as A
    assert issubclass(A.StepObjective, int) and (A.StepObjective.SQUARE, A.StepObjective.ROBUST) == (0, 1)
    assert rao.RenderingAlignmentParameters().step_objective == A.StepObjective.SQUARE   # the default objective is SQUARE
    assert P.FusionParameters().step_objective is None
    monkeypatch.setattr(A, "DeformableMeshToImageFitter", _FakeFitter)
    K = np.array([[100.0, 0, 32], [0, 100.0, 24], [0, 0, 1]])
    _FakeFitter.made.clear()
    c = A.StepControl()
    robust = rao.RenderingAlignmentParameters(step_control=c, step_objective=A.StepObjective.ROBUST, penalty_form=A.PenaltyForm.IRLS)
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, robust)
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters(step_control=c, step_objective=A.StepObjective.ROBUST)))
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters(alignment=robust)))
    rao.RenderingAlignmentOptimizer((48, 64), 0, K, P.alignment_parameters(P.FusionParameters()))
    assert [f.kw["step_objective"] for f in _FakeFitter.made] == [A.StepObjective.ROBUST] * 3 + [A.StepObjective.SQUARE]
    assert [f.control for f in _FakeFitter.made] == [c, c, c, None]


def test_python_methods_exist():
    import inspect
    from dynamicfuion_python_amd.nnrt import alignment as A
    F = A.DeformableMeshToImageFitter
    assert callable(F.set_step_objective) and callable(F.raw_residuals)
    assert isinstance(F.step_objective, property)
    assert inspect.signature(F.__init__).parameters["step_objective"].default == A.StepObjective.SQUARE
    for text in (A.StepControl.__doc__, F.set_step_control.__doc__):
        assert "StepObjective" in text
