"""The motion images and the flow comparison (csrc/motion.hip) at 640 x 480 for a kernel trace: a grid mesh of
9,322 triangles over most of the image, moved by a few millimetres, rendered --reps times after --warmup, and its scene and
optical flow compared with a perturbed copy. Run it under the profiler, which gives the kernels' own times:
    rocprofv3 --kernel-trace --stats -d <out> -- python tools/motion_timing.py [--reps 20] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from dynamicfuion_python_amd import synthetic
    from dynamicfuion_python_amd.nnrt import geometry as G
    from dynamicfuion_python_amd.nnrt import rendering as R
    H, W = 480, 640
    K = np.array([[500.0, 0.0, 319.5], [0.0, 500.0, 239.5], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(0)
    points, _, faces = synthetic.grid_mesh(80, 60)
    moved = (points + rng.normal(0.0, 0.003, points.shape)).astype(np.float32)
    fragments, camera = R.rasterize_meshes(G.TriangleMesh(points, None, faces), K, (H, W), cull_back_faces=False, ndc_convention=R.NDC_CONSISTENT)
    source, triangles, target = camera[0].vertex_positions, camera[0].triangle_indices, torch.from_numpy(moved).cuda()
    covered = int((fragments[0][..., 0] >= 0).sum())
    print(f"{W} x {H}, {len(faces)} triangles, {covered} of {H * W} pixels covered", flush=True)
    for i in range(args.warmup + args.reps):
        motion = R.motion_from_fragments(fragments[0], fragments[2], triangles, source, target, K)
        if i == 0:
            scene_truth = motion.scene_flow + torch.from_numpy(rng.normal(0.0, 0.002, (H, W, 3)).astype(np.float32)).cuda()
            optical_truth = motion.optical_flow + torch.from_numpy(rng.normal(0.0, 0.5, (H, W, 2)).astype(np.float32)).cuda()
            known = torch.from_numpy(rng.random((H, W)) < 0.9).cuda()
        scene, _ = R.compare_flow(motion.scene_flow, motion.mask, scene_truth, known, inlier_threshold=0.005)
        optical, _ = R.compare_flow(motion.optical_flow, motion.mask, optical_truth, known, inlier_threshold=1.0)
    torch.cuda.synchronize()
    print(f"valid {int(motion.mask.sum())}; scene flow: both {scene.both}, mean EPE {scene.mean_epe * 1e3:.3f} mm; "
          f"optical flow: both {optical.both}, mean EPE {optical.mean_epe:.3f} px", flush=True)


if __name__ == "__main__":
    main()
