"""Motion-graph node selection time (csrc/graph_sampling.hip: erosion mask + greedy node sampling) on the two meshes
DESIGN records: the seq017 canonical mesh the fusion loop extracts from frame 300 (tests/golden/deepdeform) and the dense
synthetic mesh (synthetic.CONFIGS["C3"]: 1501 x 1501 vertices, its node coverage). Per mesh one JSON line: sizes, node
count, rounds, the device time of erosion + sampling (HIP events around both calls, median / min / max of --reps
repetitions after --warmup), and the single-thread time of the numpy restatement (tests/_graph_util.py) with whether both
give the same nodes.
    python tools/graph_sampling_timing.py [--reps 20] [--warmup 3] [--skip-restatement] [seq017] [dense]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EROSION_ITERATIONS, EROSION_MIN_NEIGHBORS = 10, 4


def seq017_mesh():
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.data import frame as dfr
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL,
                                   base_directory=os.path.join(ROOT, "tests", "golden", "deepdeform"), frame_indices=[300])
    pipe = F.FusionPipeline(seq, F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH))
    pipe.process_frame(seq.get_next_frame())
    mesh = pipe.graph_source_mesh
    return mesh.vertex_positions, mesh.triangle_indices, pipe.parameters.node_coverage


def dense_mesh():
    import torch
    from dynamicfuion_python_amd import synthetic as S
    config = S.CONFIGS["C3"]
    points, _, faces = S.grid_mesh(config[3], config[4])
    return torch.from_numpy(points).cuda(), torch.from_numpy(faces).cuda(), config[7]


def measure(name, vertices, faces, coverage, reps, warmup, restatement):
    import torch
    import _graph_util as GU
    from dynamicfuion_python_amd import nnrt

    def run():
        mask = nnrt.get_vertex_erosion_mask(vertices, faces, EROSION_ITERATIONS, EROSION_MIN_NEIGHBORS)
        return mask, nnrt.graph_proc.sample_node_indices(vertices, mask, None, coverage)

    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        mask, (indices, rounds) = run()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    row = {"mesh": name, "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "coverage": coverage,
           "candidates": int(mask.sum()), "nodes": int(indices.shape[0]), "rounds": rounds, "reps": reps,
           "device_ms_median": round(float(np.median(times)), 3), "device_ms_min": round(min(times), 3), "device_ms_max": round(max(times), 3)}
    if restatement:
        v, f = vertices.cpu().numpy(), faces.cpu().numpy()
        t0 = time.perf_counter()
        eroded = GU.erosion_mask(len(v), f, EROSION_ITERATIONS, EROSION_MIN_NEIGHBORS)
        want = GU.sample_nodes(v, coverage, eroded)
        row["restatement_1thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["identical"] = bool(np.array_equal(indices.cpu().numpy(), want) and np.array_equal(mask.cpu().numpy()[:, 0], eroded))
    print(json.dumps(row), flush=True)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("meshes", nargs="*", default=["seq017", "dense"])
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--warmup", type=int, default=3)
    parser.add_argument("--skip-restatement", action="store_true")
    args = parser.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device is visible: nothing to time")
    for name in args.meshes:
        vertices, faces, coverage = {"seq017": seq017_mesh, "dense": dense_mesh}[name]()
        measure(name, vertices, faces, coverage, args.reps, args.warmup, not args.skip_restatement)


if __name__ == "__main__":
    main()
