"""Device time of the two anchor computations on C2's canonical mesh (synthetic.CONFIGS["C2"]: 77,361 vertices, 1,500
nodes), K = 4: `nnrt_compute_anchors_and_weights` (k_compute_anchors) and `nnrt_compute_anchors_and_weights_shortest_path`
over K-NN edge rows of degree D = 8 (the call: edge check, its stream synchronization, and the kernel). HIP events around
each call, median / min / max of --reps calls after --warmup.
    python tools/anchor_timing.py [--reps 20] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import _anchor_sp_util as U
    from dynamicfuion_python_amd import _native as N
    from dynamicfuion_python_amd import synthetic as S
    sc = S.make_scene("C2")
    dev = torch.device("cuda")
    p = torch.as_tensor(sc.points, device=dev).contiguous()
    n = torch.as_tensor(sc.nodes, device=dev).contiguous()
    e = torch.as_tensor(U.knn_edge_rows(sc.nodes, 8), device=dev).contiguous()
    V, nodes = p.shape[0], n.shape[0]
    a = torch.empty((V, 4), dtype=torch.int32, device=dev)
    w = torch.empty((V, 4), dtype=torch.float32, device=dev)
    lib = N.lib()

    def euclidean():
        N.check(lib.nnrt_compute_anchors_and_weights(N.ptr(p), V, N.ptr(n), nodes, 4, sc.coverage, None, 0, N.ptr(a), N.ptr(w), N.stream_ptr()))

    def shortest_path():
        N.check(lib.nnrt_compute_anchors_and_weights_shortest_path(N.ptr(p), V, N.ptr(n), nodes, N.ptr(e), 8, 4, sc.coverage, None, N.ptr(a),
                                                                   N.ptr(w), N.stream_ptr()))

    print(f"V {V} N {nodes} D 8 K 4", flush=True)
    for name, fn in (("k_compute_anchors", euclidean), ("shortest-path call (edge check + kernel)", shortest_path)):
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
