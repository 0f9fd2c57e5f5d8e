"""Device time of the rigid alignment's iteration (k_rigid_accumulate + k_rigid_solve_update) at C2 size: the
synthetic.CONFIGS["C2"] mesh (77,361 vertices) against a 640 x 480 live point image. HIP events around whole
nnrt_rigid_align_point_to_plane calls of 1 and of 1 + --iterations iterations; the difference divided by --iterations is
one iteration's time on the stream (the call's allocation, copies and synchronization cancel). Per-kernel times: run
this under `rocprofv3 --kernel-trace --stats`.
    python tools/rigid_align_timing.py [--iterations 20] [--reps 20] [--warmup 3] [--hybrid]
--hybrid times nnrt_rigid_align_hybrid on the same input, textured, the same way, next to the geometric
call (the solve kernel is the same: the difference of the two iteration times is the accumulate kernel's), then the two
image kernels at 640 x 480 (HIP events around 100 launches) and whole default-schedule calls of both Python functions
(host time around the call, which synchronizes).
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hybrid", action="store_true")
    args = ap.parse_args()
    import torch
    import _rigid_align_util as U
    from dynamicfuion_python_amd import _native as N
    from dynamicfuion_python_amd.nnrt import geometry as G
    H, W = 480, 640
    K = U.intrinsics(H, W)
    dev = torch.device("cuda")
    points, normals = U.model(321, 241, U.T_GT)
    p, n = torch.as_tensor(points, device=dev).contiguous(), torch.as_tensor(normals, device=dev).contiguous()
    tp = torch.as_tensor(U.live_point_image(H, W, K), device=dev).contiguous()
    tn = G.compute_ordered_point_cloud_normals(tp.reshape(-1, 3), (H, W))
    V = p.shape[0]
    lib = N.lib()
    T, out, st = np.eye(4), np.zeros((4, 4)), ctypes.c_int32(0)

    def geometric_call(iterations):
        log = np.zeros((iterations, 2))
        N.check(lib.nnrt_rigid_align_point_to_plane(N.ptr(p), N.ptr(n), V, N.ptr(tp), N.ptr(tn), H, W, K[0, 0], K[1, 1], K[0, 2], K[1, 2], N.ptr(T),
                                                    iterations, 0.07, 0.5, 0, 50, N.ptr(out), N.ptr(log), iterations, ctypes.byref(st),
                                                    N.stream_ptr()))
        return log

    def timed(iterations, call=geometric_call):
        for _ in range(args.warmup):
            call(iterations)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call(iterations)
            stop.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(stop))
        return np.array(ms)

    def report(label, call):
        one, many = timed(1, call), timed(1 + args.iterations, call)
        for name, ms in (("call, 1 iteration", one), (f"call, {1 + args.iterations} iterations", many)):
            print(f"{label}{name}: median {np.median(ms) * 1e3:.1f} us, min {ms.min() * 1e3:.1f} us, max {ms.max() * 1e3:.1f} us over {args.reps} calls",
                  flush=True)
        per_iteration = (np.median(many) - np.median(one)) / args.iterations * 1e3
        print(f"{label}one iteration (accumulate + solve), from the medians: {per_iteration:.1f} us", flush=True)
        return per_iteration

    log = geometric_call(1)
    print(f"V {V}, {W} x {H}: {int(log[0, 0])} correspondences in the first iteration, status {st.value}", flush=True)
    geometric = report("", geometric_call)
    if not args.hybrid:
        return
    import time
    import _rigid_hybrid_util as HY
    from dynamicfuion_python_amd.nnrt import alignment as A
    from dynamicfuion_python_amd.nnrt import image_proc as IP
    color = torch.as_tensor(HY.live_color_image(tp.cpu().numpy()), device=dev).contiguous()
    c = torch.as_tensor(HY.model_colors(321, 241), device=dev).contiguous()
    ti = IP.intensity_from_rgb8(color)

    def hybrid_call(iterations):
        log = np.zeros((iterations, 4))
        N.check(lib.nnrt_rigid_align_hybrid(N.ptr(p), N.ptr(n), N.ptr(c), V, N.ptr(tp), N.ptr(tn), N.ptr(ti), H, W, K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                                            N.ptr(T), iterations, 0.07, 0.5, 0, 50, 0.1, 0.0, N.ptr(out), N.ptr(log), iterations, ctypes.byref(st),
                                            N.stream_ptr()))
        return log

    log = hybrid_call(1)
    print(f"hybrid: {int(log[0, 0])} correspondences, {int(log[0, 2])} photometric rows in the first iteration, status {st.value}", flush=True)
    hybrid = report("hybrid ", hybrid_call)
    print(f"k_rigid_accumulate, photometric build less geometric build, per dispatch: {hybrid - geometric:.1f} us", flush=True)
    launches = 100
    for name, kernel, image in (("k_intensity_rgb8", IP.intensity_from_rgb8, color), ("k_intensity_halve", IP.halve_intensity, ti)):
        for _ in range(args.warmup):
            kernel(image)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            kernel(image)
        stop.record()
        torch.cuda.synchronize()
        print(f"{name} at {W} x {H}: {start.elapsed_time(stop) / launches * 1e3:.1f} us per launch, back to back with its output's allocation "
              f"({launches} launches)", flush=True)
    for name, call in (("align_rigid_point_to_plane", lambda: A.align_rigid_point_to_plane(p, n, tp, K)),
                       ("align_rigid_hybrid", lambda: A.align_rigid_hybrid(p, n, c, tp, color, K))):
        for _ in range(args.warmup):
            call()
        seconds = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            seconds.append(time.perf_counter() - t0)
        print(f"{name}, default (6, 3, 1) schedule: median {np.median(seconds) * 1e3:.3f} ms per call, min {min(seconds) * 1e3:.3f} ms over "
              f"{args.reps} calls", flush=True)


if __name__ == "__main__":
    main()
