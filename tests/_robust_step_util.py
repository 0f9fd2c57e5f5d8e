"""A float64 restatement of step control under the robust step objective (nnrt_fitter_set_step_objective,
NNRT_STEP_OBJECTIVE_ROBUST): the state machine of tests/_step_control_util.py's run(), iteration for
iteration, over the IRLS assemblies of tests/_coupled_util.py / tests/_robust_util.py, comparing the robust cost instead of
the sum of squares. CONFIGS_ROBUST are the runs tests/test_gpu_robust_step.py repeats on the device
(tests/test_robust_step_cpu.py holds each of their decisions to the 1e-2 margin on the CPU first)."""
import numpy as np

from _coupled_util import apply_update, coupled_system, gt_translations_virtual, identity_motion, solve_dense
from _robust_util import F32, arap_term, data_term, patch_targets
from _step_control_util import (ACCEPT, CONVERGED, DECISION_MARGIN, DONE_DECISIONS, HOLD, LM, REJECT, REJECT_FINAL,   # noqa: F401
                                SMALL_UPDATE, START, control, decision_margins, summarize)

HUBER_DELTA = 0.05   # S1_ARAP: edges stretch beyond it from the first rejected state on (test_huber_is_exceeded)


def tukey_cost(r, mask, c=None):
    """The data term of the robust objective, float64: over the masked pixels r^2 without a cutoff; with cutoff c,
    (c^2 / 3)(1 - (1 - q^2)^3), q = r / c, where |r| <= c in float32 (formed as (c^2 / 3) q^2 (3 + q^2 (q^2 - 3)): the same
    polynomial without the cancellation at small q), c^2 / 3 beyond; NaN for a masked r that is not finite."""
    r32 = np.asarray(r, F32)[np.asarray(mask, bool)]
    r = r32.astype(np.float64)
    if c is None:
        term = r * r
    else:
        cd = float(F32(c))
        c23 = cd * cd / 3.0
        q2 = (r / cd) * (r / cd)
        with np.errstate(invalid="ignore", over="ignore"):
            term = np.where(np.abs(r32) <= F32(c), c23 * (q2 * (3.0 + q2 * (q2 - 3.0))), c23)
    term = np.where(np.isfinite(r32), term, np.nan)
    return float(term.sum())


def huber_cost(stored, delta=None):
    """The ARAP term of the robust objective from the STORED edge residuals [E,3] (scaled by sqrt(delta / n) where the raw
    norm n exceeds delta): m^2 = their float64 sum of squares; m^2 without Huber, else m^2 if m^2 <= delta^2, 2 m^2 - delta^2
    otherwise."""
    e = np.asarray(stored, F32).astype(np.float64).reshape(-1, 3)
    m2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    if delta is None:
        return float(m2.sum())
    d2 = float(F32(delta)) * float(F32(delta))
    with np.errstate(invalid="ignore"):
        return float(np.where(m2 <= d2, m2, 2.0 * m2 - d2).sum())


def robust_cost(r, mask, tukey_c=None, stored_edges=None, huber_delta=None):
    c = tukey_cost(r, mask, tukey_c)
    if stored_edges is not None and len(stored_edges):
        c += huber_cost(stored_edges, huber_delta)
    return c


def inlier_cutoff(O, sc, target, patch):
    """The Tukey cutoff of the configurations: 1.5 times the largest |r| at the identity outside the pushed patch, so every
    inlier starts inside the cutoff and the patch (0.5 m behind) outside it."""
    dg = data_term(O, sc, target)
    inl = dg["residual_mask"] & ~patch.reshape(-1)
    return 1.5 * float(np.abs(dg["r"][inl]).max())


def evaluate(O, sc, depth, R, t, coupled, tukey_c=None, huber_delta=None, arap_weight=200.0):
    """The robust cost at (R, t) and the undamped IRLS Gauss-Newton system there: (cost, diag, pairs, blocks, rhs, edge norms)."""
    sysm = coupled_system(O, sc, depth, R, t, tukey_c=tukey_c, lm=0.0, arap_weight=arap_weight, huber_delta=huber_delta)
    d = sysm["data"]
    stored, norms = None, np.zeros(0, F32)
    if sc.hierarchy:
        ar = arap_term(O, sc, R, t, arap_weight, huber_delta)
        stored, norms = ar["residuals"], ar["norms"]
    cost = robust_cost(d["r"], d["residual_mask"], tukey_c, stored, huber_delta)
    pairs, blocks = sysm["pairs"], sysm["blocks"]
    if not coupled and len(pairs):
        blocks = blocks - d["Hfull"][pairs[:, 0], pairs[:, 1]]   # what stays off the diagonal is the ARAP wings
    return cost, sysm["diag"], pairs, blocks, sysm["rhs"], norms


def run(O, sc, depth, coupled, settings, iterations, lm=LM, minimal_update_threshold=1e-6, tukey_c=None, huber_delta=None, start=None):
    """_step_control_util.run's state machine with the robust cost and the IRLS system; the records also carry
    `edge_norm_max` (the largest raw edge residual norm at the evaluated state; 0 without a hierarchy)."""
    N = len(sc.nodes)
    R, t = identity_motion(N) if start is None else start
    f = F32
    lam = f(settings["initial_lambda"]) if settings["initial_lambda"] > 0 else f(lm)
    lam = min(max(lam, f(settings["lambda_min"])), f(settings["lambda_max"]))
    inc, dec, lmin, lmax = f(settings["increase"]), f(settings["decrease"]), f(settings["lambda_min"]), f(settings["lambda_max"])
    tol = float(f(settings["relative_cost_tolerance"]))
    thr = f(minimal_update_threshold)
    c_best, best, retry, done = 0.0, (R, t), False, False
    memo, out = {}, []
    for it in range(iterations):
        key = (np.asarray(R).tobytes(), np.asarray(t).tobytes())
        if key not in memo:
            memo[key] = evaluate(O, sc, depth, R, t, coupled, tukey_c, huber_delta)
        c, diag0, pairs, blocks, rhs, norms = memo[key]
        if done:
            hold, decision = True, HOLD
        elif it == 0 or retry:
            c_best, best, retry, hold, decision = c, (R, t), False, False, START
        elif c <= c_best:
            best = (R, t)
            if (c_best - c) <= tol * c_best:
                done, hold, decision = True, True, CONVERGED
            else:
                lam, hold, decision = max(f(lam * dec), lmin), False, ACCEPT
            c_best = c
        else:
            decision = REJECT
            if lam >= lmax:
                done, decision = True, REJECT_FINAL
            lam, retry, hold = min(f(lam * inc), lmax), True, True
        m = 0.0
        if hold:
            R, t = best
        else:
            diag = diag0 + (float(lam) * np.eye(6) if lam > 0 else 0.0)
            x, _ = solve_dense(diag, pairs, blocks, rhs)
            m = float(np.abs(x).max()) if np.isfinite(x).all() else float("inf")
            if m < thr:
                done, decision = True, SMALL_UPDATE
                R, t = best
            else:
                R, t = apply_update(R, t, x)
        out.append(dict(iteration=it, cost=c, lambda_used=f(lam), decision=decision, max_update=m, c_best=c_best, state=(R, t), best=best,
                        edge_norm_max=float(norms.max()) if len(norms) else 0.0))
    return out


# name -> (scene, coupled, settings, iterations, tukey, huber delta or None): every run fits target A of patch_targets (a
# 12 x 12 patch pushed 0.5 m back) with the Tukey cutoff of inlier_cutoff when `tukey`; lambda settings chosen so that every
# decision keeps the 1e-2 margin (tests/test_robust_step_cpu.py::test_decision_margins_robust): S1_coupled's fifth decision
# has 4e-3 and S1_ARAP_arrowhead's fourteenth 7e-3, so those runs stop before them
CONFIGS_ROBUST = {
    "S1_block": ("S1", False, control(increase=10.0, decrease=0.5, lambda_max=10.0), 10, True, None),
    "S1_coupled": ("S1", True, control(increase=10.0, decrease=0.1, lambda_max=10.0), 4, True, None),
    "S1_ARAP_arrowhead": ("S1_ARAP", False, control(increase=10.0, decrease=0.5, lambda_max=1e5), 12, True, HUBER_DELTA),
}


def config_inputs(O, scenes, name):
    """(sc, target A, tukey cutoff or None, huber delta or None) of a configuration; scenes: name -> (scene, rendered depth)."""
    scene, _, _, _, tukey, huber = CONFIGS_ROBUST[name]
    sc, depth = scenes[scene]
    A, _, patch = patch_targets(depth)
    return sc, A, (inlier_cutoff(O, sc, A, patch) if tukey else None), huber


def run_config(O, scenes, name):
    _, coupled, settings, iterations, _, _ = CONFIGS_ROBUST[name]
    sc, A, c, huber = config_inputs(O, scenes, name)
    return run(O, sc, A, coupled, settings, iterations, tukey_c=c, huber_delta=huber)


def translation_error(sc, t):
    """RMS distance of node translations t (virtual order) to the scene's ground truth."""
    return float(np.sqrt(((np.asarray(t, np.float64) - gt_translations_virtual(sc)) ** 2).sum(axis=1).mean()))
