"""Device time of the shaders and the depth comparison (csrc/shading.hip) at 640 x 480, one face per pixel: a
two-triangle plane with colours and normals over most of the image, against a uint16 depth frame. HIP events around each
call (for the comparison: both launches, the read-back of the record and the stream synchronization), median / min / max of
--reps calls after --warmup.
    python tools/shading_timing.py [--reps 20] [--warmup 3]
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
    from dynamicfuion_python_amd.nnrt import geometry as G
    from dynamicfuion_python_amd.nnrt import rendering as R
    H, W = 480, 640
    K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(0)
    p = np.array([[-0.6, -0.45, 1.0], [0.55, -0.45, 1.0], [0.55, 0.4, 1.1], [-0.6, 0.4, 1.1]], np.float32)
    normals = np.concatenate([rng.uniform(-0.3, 0.3, (4, 2)), -np.ones((4, 1))], 1).astype(np.float32)
    mesh = G.TriangleMesh(p, normals, np.array([[0, 1, 2], [0, 2, 3]], np.int64), vertex_colors=rng.random((4, 3)).astype(np.float32))
    fragments, camera = R.rasterize_meshes(mesh, K, (H, W), blur_radius_pixels=1.0, cull_back_faces=False, ndc_convention=R.NDC_CONSISTENT)
    depth = rng.integers(900, 1200, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.1] = 0
    depth = torch.from_numpy(depth.view(np.int16)).cuda()
    covered = int((fragments[0][..., 0] >= 0).sum())
    print(f"{W} x {H}, {covered} of {H * W} pixels covered", flush=True)
    calls = (("k_shade_pixels VERTEX_COLOR", lambda: R.VertexColorShader().shade_meshes(*fragments, camera)),
             ("k_shade_pixels FLAT_EDGE", lambda: R.FlatEdgeShader(2.0, (1.0, 1.0, 1.0)).shade_meshes(*fragments)),
             ("k_shade_pixels HEADLIGHT", lambda: R.HeadlightShader().shade_meshes(*fragments, camera)),
             ("compare_depth_to_raster (two launches, read-back, synchronization)",
              lambda: R.compare_depth_to_raster(fragments[0], fragments[1], depth)))
    for name, fn in calls:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(stop))
        ms = np.array(ms)
        print(f"{name}: median {np.median(ms) * 1e3:.1f} us, min {ms.min() * 1e3:.1f} us, max {ms.max() * 1e3:.1f} us over {args.reps} calls",
              flush=True)


if __name__ == "__main__":
    main()
