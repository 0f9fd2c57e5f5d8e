"""The per-iteration cost of step control's two launches (k_step_cost, k_step_select): the solve stage
and the whole iteration as nnrt_fitter_time_kernels measures them, with the mode off and on, on bench.py's workloads.
--objective robust measures k_step_cost_robust in k_step_cost's place, with the Tukey and Huber
penalties in their IRLS form in both runs, so that the difference is the two launches alone.

    python tools/step_control_cost.py [C2 C5 ...] [--coupled] [--objective square|robust]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C2", "C5"])
    ap.add_argument("--coupled", action="store_true", help="the coupled data term's iteration instead of the default one")
    ap.add_argument("--objective", choices=("square", "robust"), default="square", help="the step objective of the `on` run")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=7)
    args = ap.parse_args()
    import torch
    import bench
    from dynamicfuion_python_amd import synthetic as S
    from dynamicfuion_python_amd.nnrt import alignment as A
    from dynamicfuion_python_amd.nnrt import geometry as G
    from dynamicfuion_python_amd.nnrt import rendering as Rr
    for config in args.configs:
        sc = S.make_scene(config, seed=0, hierarchy_builder=S.native_hierarchy_builder)
        depth = bench.render_target(sc, G, Rr)
        mesh = G.TriangleMesh(sc.points, sc.normals, sc.faces)
        out = dict(config=config, pixels=sc.H * sc.W, nodes=len(sc.nodes), layers=sc.layer_count, coupled=args.coupled, objective=args.objective)
        robust = args.objective == "robust"
        # cutoffs wide enough that the penalties weigh every pixel and edge: the launches do their full work
        penalties = dict(use_tukey_penalty_for_data_term=True, tukey_penalty_cutoff_cm=0.05, use_huber_penalty_for_arap_term=True,
                         huber_penalty_constant=0.01, penalty_form=A.PenaltyForm.IRLS, guard_zero_rotation=True,
                         step_objective=A.StepObjective.ROBUST) if robust else {}
        for label, control in (("off", None), ("on", A.StepControl())):
            wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)
            ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=A.GRAPH_ALWAYS,
                                               **penalties)
            if args.coupled:
                ft.set_data_coupling(A.DataCoupling.COUPLED)
            ft.set_step_control(control)
            R_mid, t_mid = sc.partial_motion(0.5)
            wf.set_node_rotations(R_mid)
            wf.set_node_translations(t_mid)
            ft.prepare(wf, mesh, depth, None, sc.K)
            ft.snapshot_motion(wf)
            k = ft.time_kernels(wf, reps=args.reps, trials=args.trials)
            torch.cuda.synchronize()
            out[f"solve_us_{label}"] = round(1e3 * k["solve"], 2)
            out[f"iteration_us_{label}"] = round(1e3 * k["iteration"], 2)
        out["added_us"] = round(out["solve_us_on"] - out["solve_us_off"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
