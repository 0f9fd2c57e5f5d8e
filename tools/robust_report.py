"""What the fitter's robust options (set_robust_options) do on the bench scenes, and what the IRLS path costs.

  python tools/robust_report.py frames [C2_ARAP C5 ...]   a ten-iteration frame fit from the identity warp, one
      iteration at a time, with the defaults and with TUKEY / HUBER + PenaltyForm.IRLS + guard_zero_rotation: per
      iteration the nodes with a NaN rotation, whether the factorization failed (potrf), the corner's pivot / diag(S)
      ratio and the largest |update|
  python tools/robust_report.py stages [S1_ARAP C2 ...]   event-timed stage times (nnrt_fitter_iterate_timed) of the
      first iteration with the square penalties, the reference forms and the IRLS forms

One JSON line per measurement on stdout. The Tukey cutoff and the Huber constant are the parameter defaults
(0.01, 1e-4) unless --tukey / --huber give others."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import bench  # noqa: E402
from dynamicfuion_python_amd import synthetic as S  # noqa: E402
from dynamicfuion_python_amd._native import NnrtError  # noqa: E402
from dynamicfuion_python_amd.nnrt import alignment as A, geometry as G, rendering as Rr  # noqa: E402


def setup(name, **kw):
    sc = S.make_scene(name, hierarchy_builder=S.native_hierarchy_builder)
    depth = bench.render_target(sc, G, Rr)
    wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)
    ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=0, **kw)
    ft.prepare(wf, G.TriangleMesh(sc.points, sc.normals, sc.faces), depth, None, sc.K)
    return sc, wf, ft


def frames(name, iters, robust):
    sc, wf, ft = setup(name, **robust)
    N = len(sc.nodes)
    for k in range(iters):
        ft.iterate(wf, k, 1)
        failed = ""
        try:
            ft.check()
        except NnrtError as e:
            failed = str(e)
        R = wf.get_node_rotations(True)
        upd = ft.diagnostics()["updates"][: 6 * N]
        info = ft.refine_info()
        print(json.dumps(dict(scene=name, options="irls+guard" if robust else "default", iteration=k + 1,
                              nan_rotation_nodes=int(np.isnan(R).reshape(N, -1).any(1).sum()), nan_updates=int(np.isnan(upd).sum()),
                              max_abs_update=float(np.nanmax(np.abs(upd))) if np.isfinite(upd).any() else None, potrf_failed=bool(failed),
                              pivot_ratio=info["pivot_ratio"], refined=info["refined"], accepted=info["accepted"])), flush=True)
        if failed:
            break


def stages(name, label, kw, reps):
    sc, wf, ft = setup(name, **kw)
    wf.reset_motion()
    ft.iterate_timed(wf, 0, 1)   # untimed first call
    rows = []
    for _ in range(reps):
        wf.reset_motion()
        rows.append(ft.iterate_timed(wf, 0, 1))
    med = {k: round(float(np.median([r[k] for r in rows])) * 1000, 2) for k in rows[0]}
    print(json.dumps(dict(scene=name, penalties=label, stage_us=med, reps=reps)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("frames", "stages"))
    ap.add_argument("scenes", nargs="*")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tukey", type=float, default=0.01)
    ap.add_argument("--huber", type=float, default=1e-4)
    args = ap.parse_args()
    pen = dict(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=args.tukey, use_huber_penalty_for_arap_term=True,
               huber_penalty_constant=args.huber)
    irls = dict(pen, penalty_form=A.PenaltyForm.IRLS, guard_zero_rotation=True)
    if args.what == "frames":
        for name in args.scenes or ["C2_ARAP", "C5"]:
            frames(name, args.iterations, {})
            frames(name, args.iterations, irls)
    else:
        for name in args.scenes or ["S1_ARAP", "C2"]:
            for label, kw in (("square", {}), ("reference", pen), ("irls", dict(pen, penalty_form=A.PenaltyForm.IRLS))):
                stages(name, label, kw, args.reps)
