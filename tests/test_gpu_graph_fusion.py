"""The fusion loop starting from depth frames alone: the committed seq017 frames 300 -> 600 (tests/golden/deepdeform) through
FusionPipeline with GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH. The motion graph's nodes are sampled on the GPU from
the first frame's mesh (csrc/graph_sampling.hip) and must be exactly the sequential restatement's (tests/_graph_util.py)
on the same mesh; frame 600 is then tracked and fused with that graph."""
import os

import numpy as np
import pytest

import _graph_util as GU

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepdeform")


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def test_fusion_pipeline_builds_its_graph_from_the_first_mesh():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible for a -m gpu test")
    from dynamicfuion_python_amd.data import frame as dfr
    from dynamicfuion_python_amd import fusion as F
    seq = dfr.FrameSequenceDataset(17, dfr.DataSplit.TEST, base_dataset_type=dfr.DatasetType.LOCAL, base_directory=DD,
                                   frame_indices=[300, 600])
    params = F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH)
    params.alignment.max_iteration_count = 1
    pipe = F.FusionPipeline(seq, params)
    pipe.process_frame(seq.get_next_frame())

    mesh = pipe.graph_source_mesh   # extracted at weight threshold 0
    vertices, faces = _np(mesh.vertex_positions), _np(mesh.triangle_indices)
    assert len(faces) > 50000
    threshold0 = pipe.volume.extract_triangle_mesh(0.0, -1)
    assert np.array_equal(_np(threshold0.vertex_positions), vertices) and np.array_equal(_np(threshold0.triangle_indices), faces)
    eroded = GU.erosion_mask(len(vertices), faces, 10, 4)
    want = GU.sample_nodes(vertices, params.node_coverage, eroded)
    assert 0 < eroded.sum() < len(vertices)
    assert np.array_equal(_np(pipe.sampled_node_vertex_indices)[:, 0], want)
    assert np.array_equal(_np(pipe.sampled_node_positions), vertices[want])   # before make_warp_field's re-ordering
    wf = pipe.active_graph
    assert wf.node_count == len(want)
    # make_warp_field only re-orders: the graph holds the same node set
    held = wf.get_node_positions()
    assert np.array_equal(held[np.lexsort(held.T)], vertices[want][np.lexsort(vertices[want].T)])

    res = pipe.process_frame(seq.get_next_frame())
    assert res.tracked
    t = wf.get_node_translations(True)
    assert np.isfinite(t).all() and np.abs(t).max() > 0
    assert not seq.has_more_frames()
