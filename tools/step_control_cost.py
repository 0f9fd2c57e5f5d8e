"""The per-iteration cost of step control's two launches (k_step_cost, k_step_select): the solve stage
and the whole iteration as nnrt_fitter_time_kernels measures them, with the mode off and on, on bench.py's workloads.

    python tools/step_control_cost.py [C2 C5 ...] [--coupled]
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
        out = dict(config=config, pixels=sc.H * sc.W, nodes=len(sc.nodes), layers=sc.layer_count, coupled=args.coupled)
        for label, control in (("off", None), ("on", A.StepControl())):
            wf = G.HierarchicalGraphWarpField(sc.nodes, sc.coverage, False, 4, 0, G.WarpNodeCoverageComputationMethod.FIXED_NODE_COVERAGE, sc.layer_count)
            ft = A.DeformableMeshToImageFitter(1, [A.IterationMode.ALL], preconditioning_dampening_factor=0.001, use_hip_graph=A.GRAPH_ALWAYS)
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
