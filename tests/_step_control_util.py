"""A float64 restatement of the fitter's on-device step control (nnrt_fitter_set_step_control) over
the assemblies of tests/_coupled_util.py: the same state machine, iteration for iteration, with the damping updated in
float32 as the device updates it. run() returns one record per iteration; CONFIGS are the runs the GPU tests repeat on the
device (tests/test_step_control_cpu.py checks on the CPU that each of their decisions has a margin the GPU's float error
cannot cross)."""
import numpy as np

from _coupled_util import apply_update, coupled_system, data_system, identity_motion, solve_dense
from _robust_util import F32, arap_term

HOLD, START, ACCEPT, CONVERGED, REJECT, REJECT_FINAL, SMALL_UPDATE = range(7)
DONE_DECISIONS = (CONVERGED, REJECT_FINAL, SMALL_UPDATE)
LM = 0.001
DECISION_MARGIN = 1e-2


def control(initial_lambda=0.0, increase=10.0, decrease=0.5, lambda_min=1e-6, lambda_max=1.0, relative_cost_tolerance=0.0, poll_interval=0):
    return dict(initial_lambda=initial_lambda, increase=increase, decrease=decrease, lambda_min=lambda_min, lambda_max=lambda_max,
                relative_cost_tolerance=relative_cost_tolerance, poll_interval=poll_interval)


# name -> (scene, coupled, settings, iterations, minimal_update_threshold): the runs of tests/test_gpu_step_control.py
CONFIGS = {
    "S1_block": ("S1", False, control(increase=10.0, decrease=0.5, lambda_max=10.0), 14, 1e-6),
    "S1_coupled": ("S1", True, control(increase=10.0, decrease=0.1, lambda_max=10.0), 8, 1e-6),
    "S1_ARAP_arrowhead": ("S1_ARAP", False, control(increase=10.0, decrease=0.5, lambda_max=1e5), 12, 1e-6),
    "S1_ARAP_coupled": ("S1_ARAP", True, control(increase=10.0, decrease=0.1, lambda_max=1e5), 12, 1e-6),
}


def evaluate(O, sc, depth, R, t, coupled, lam, arap_weight=200.0):
    """The total cost at (R, t) and the Gauss-Newton system the fitter would solve there under damping `lam`:
    (cost, diag [N,6,6], pairs, blocks, rhs). Block-diagonal / arrowhead steps keep the data term's diagonal blocks only."""
    sysm = coupled_system(O, sc, depth, R, t, lm=float(lam), arap_weight=arap_weight)
    d = sysm["data"]
    cost = d["cost"]
    if sc.hierarchy:
        res = arap_term(O, sc, R, t, arap_weight)["residuals"]
        cost += float((np.asarray(res, F32).astype(np.float64) ** 2).sum())
    pairs, blocks = sysm["pairs"], sysm["blocks"]
    if not coupled and len(pairs):
        blocks = blocks - d["Hfull"][pairs[:, 0], pairs[:, 1]]   # what stays off the diagonal is the ARAP wings
    return cost, sysm["diag"], pairs, blocks, sysm["rhs"]


def run(O, sc, depth, coupled, settings, iterations, lm=LM, minimal_update_threshold=1e-6, start=None):
    """The state machine of include/nnrt_mi355x.h (nnrt_fitter_set_step_control) from the identity (or `start` = (R, t)):
    a list of dicts(iteration, cost, lambda_used, decision, max_update, c_best, state=(R, t) after the iteration, best)."""
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
            memo[key] = evaluate(O, sc, depth, R, t, coupled, 0.0)
        c, diag0, pairs, blocks, rhs = memo[key]
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
        out.append(dict(iteration=it, cost=c, lambda_used=f(lam), decision=decision, max_update=m, c_best=c_best, state=(R, t), best=best))
    return out


def decision_margins(history):
    """|c - c_best| / c_best of every accept / reject decision (c_best as it stood before the decision)."""
    out, prev = [], None
    for h in history:
        if h["decision"] in (ACCEPT, CONVERGED, REJECT, REJECT_FINAL):
            out.append((h["iteration"], abs(h["cost"] - prev) / prev))
        prev = h["c_best"]
    return out


def summarize(history):
    """(iterations_used, final_cost, rejected_step_count) as dynamicfuion_python_amd.nnrt.alignment.summarize_step_history."""
    used, done, final_cost, rejected = len(history), False, 0.0, 0
    for i, h in enumerate(history):
        if h["decision"] in (START, ACCEPT, CONVERGED):
            final_cost = h["cost"]
        if h["decision"] in (REJECT, REJECT_FINAL):
            rejected += 1
        if not done and (h["decision"] in DONE_DECISIONS or h["decision"] == HOLD):
            used, done = (i + 1 if h["decision"] != HOLD else i), True
    return used, final_cost, rejected
