"""The shading restatements (tests/_shading_util.py) without a GPU: over the CPU oracle's rasterization they reproduce the
reference's two known-answer images byte for byte, which pins the arithmetic the kernels are tested against to reference
data; the byte clamp outside [0, 255]; join_triangle_meshes; the DepthAgreement ratios."""
import math

import numpy as np
import pytest

import _shading_util as SU

F32 = np.float32


def triangle_fragments(oracle_mod, blur):
    H, W = SU.TRIANGLE_SIZE
    ndc, mask = oracle_mod.extract_face_ndc(SU.TRIANGLE_VERTICES, SU.TRIANGLE_FACES, SU.TRIANGLE_K, H, W)
    return oracle_mod.rasterize(ndc, mask, H, W, blur_radius_pixels=blur, faces_per_pixel=1)


def test_vertex_color_restatement_reproduces_the_reference_image(oracle_mod):
    faces, _, bary, _ = triangle_fragments(oracle_mod, 0.0)
    image = SU.shade_vertex_color(faces, bary, SU.TRIANGLE_FACES, SU.TRIANGLE_COLORS)
    want = SU.golden_image("triangle_vertex_colors.png")
    assert image.shape == want.shape == (480, 640, 3)
    assert int((image != want).sum()) == 0
    assert int((faces[..., 0] >= 0).sum()) == SU.VERTEX_COLOR_COVERED


def test_flat_edge_restatement_reproduces_the_reference_image(oracle_mod):
    faces, _, _, dist = triangle_fragments(oracle_mod, 1.0)
    image = SU.shade_flat_edge(faces, dist, 2.0, (1.0, 1.0, 1.0))
    want = SU.golden_image("triangle.png")
    assert int((image != want).sum()) == 0
    assert int(image.any(-1).sum()) == SU.FLAT_EDGE_LIT


def test_byte_conversion_clamps_outside_0_255(oracle_mod):
    assert SU.to_byte(np.array([-3.0, -0.0, 0.0, 0.999, 1.0, 127.5, 254.999, 255.0, 255.5, 1e30, np.inf, -np.inf, np.nan], F32)).tolist() == \
        [0, 0, 0, 0, 1, 127, 254, 255, 255, 255, 255, 0, 0]
    # blur > 0 keeps fragments outside the face, whose barycentrics are unclipped (some negative, some above 1); with
    # colours below 0 and above 1 the products leave [0, 255] on both sides
    faces, _, bary, _ = triangle_fragments(oracle_mod, 6.0)
    covered = faces[..., 0] >= 0
    assert (bary[..., 0, :][covered] < 0).any() and (bary[..., 0, :][covered] > 1).any()
    colors = np.array([[-0.5, 2.0, 0.25], [1.5, -1.0, 0.5], [0.75, 0.5, 3.0]], F32)
    image = SU.shade_vertex_color(faces, bary, SU.TRIANGLE_FACES, colors)
    b = bary[..., 0, :].astype(F32)
    value = np.zeros(b.shape[:2] + (3,), F32)
    for k in range(3):
        value = value + b[..., k, None] * colors[k]
    value = value * F32(255)
    low, high = covered[..., None] & (value <= 0), covered[..., None] & (value >= 255)
    assert low.any() and high.any() and (covered[..., None] & ~low & ~high).any()
    assert (image[low] == 0).all() and (image[high] == 255).all()
    middle = covered[..., None] & ~low & ~high
    assert np.array_equal(image[middle], np.trunc(value[middle]).astype(np.uint8))
    assert (image[~covered] == 0).all()
    # the flat-edge and head-lit shaders clamp the same way
    _, _, _, dist = triangle_fragments(oracle_mod, 1.0)
    lit = SU.shade_flat_edge(faces * 0, np.zeros_like(dist), 2.0, (2.0, -1.0, 0.5))   # distance 0: factor 1
    assert (lit == np.array([255, 0, 127], np.uint8)).all()
    normals = np.array([[0, 0, -1]] * 3, F32)
    head = SU.shade_headlight(faces, bary, SU.TRIANGLE_FACES, normals, (3.0, -2.0, 0.5), 0.0)
    inside = covered & (bary[..., 0, :] > 0.01).all(-1)
    assert inside.any() and (head[inside] == np.array([255, 0, 127], np.uint8)).all()


def test_join_triangle_meshes_offsets_indices_and_drops_partial_attributes():
    import torch
    from dynamicfuion_python_amd.nnrt import geometry as G
    a = dict(vertex_positions=np.arange(9, dtype=F32).reshape(3, 3), triangle_indices=np.array([[0, 1, 2]]),
             vertex_normals=np.tile(F32([0, 0, -1]), (3, 1)), vertex_colors=np.full((3, 3), 0.25, F32))
    b = dict(vertex_positions=10 + np.arange(12, dtype=F32).reshape(4, 3), triangle_indices=np.array([[0, 1, 2], [2, 1, 3]]),
             vertex_normals=np.tile(F32([0, 1, 0]), (4, 1)), vertex_colors=None)
    c = dict(vertex_positions=np.zeros((0, 3), F32), triangle_indices=np.zeros((0, 3), np.int64), vertex_normals=np.zeros((0, 3), F32),
             vertex_colors=None)

    def mesh(d):
        return G.TriangleMesh(d["vertex_positions"], d["vertex_normals"], d["triangle_indices"], vertex_colors=d["vertex_colors"])

    for parts in ([a, b], [b, a], [a, c, b], [a, a]):
        want = SU.join(parts)
        for joined in (G.join_triangle_meshes([mesh(d) for d in parts]), G.functional.join_triangle_meshes(tuple(mesh(d) for d in parts))):
            assert joined.triangle_indices.dtype == torch.int64
            assert np.array_equal(joined.triangle_indices.numpy(), want["triangle_indices"])
            assert np.array_equal(joined.vertex_positions.numpy(), want["vertex_positions"])
            assert np.array_equal(joined.vertex_normals.numpy(), want["vertex_normals"])
            if want["vertex_colors"] is None:
                assert joined.vertex_colors is None
            else:
                assert np.array_equal(joined.vertex_colors.numpy(), want["vertex_colors"])
    assert SU.join([a, b])["triangle_indices"].tolist() == [[0, 1, 2], [3, 4, 5], [5, 4, 6]]
    assert SU.join([b, a])["triangle_indices"].tolist() == [[0, 1, 2], [2, 1, 3], [4, 5, 6]]
    assert SU.join([a, b])["vertex_colors"] is None and SU.join([a, a])["vertex_colors"].shape == (6, 3)
    without_normals = G.TriangleMesh(a["vertex_positions"], None, a["triangle_indices"])
    assert G.join_triangle_meshes([mesh(a), without_normals]).vertex_normals is None
    with pytest.raises(RuntimeError):
        G.join_triangle_meshes([])


def test_depth_agreement_ratios_on_a_hand_written_case():
    from dynamicfuion_python_amd.nnrt.rendering import DepthAgreement
    # 3 x 3: model depth 1.0 on the first two rows; frame (mm): row 0 = 1010, 1000, 0; row 1 = 990, 5000, 1030; row 2 = 1000, 0, 1000
    faces = np.array([[0, 0, 0], [1, 1, 1], [-1, -1, -1]], np.int64)[..., None]
    depths = np.where(faces >= 0, F32(1.0), F32(-1.0)).astype(F32)
    frame = np.array([[1010, 1000, 0], [990, 5000, 1030], [1000, 0, 1000]], np.uint16)
    record, difference = SU.compare_depth(faces, depths, frame, 1000.0, 3.0, 0.0101)
    assert (record["both"], record["model_only"], record["frame_only"], record["inliers"]) == (4, 2, 2, 3)
    d = [float(F32(1.0) - F32(v) / F32(1000.0)) for v in (1010, 1000, 990, 1030)]
    assert record["sum_abs"] == math.fsum(abs(v) for v in d) and record["sum_sq"] == math.fsum(v * v for v in d)
    assert record["max_abs"] == abs(d[3])
    assert np.array_equal(np.isnan(difference), np.array([[0, 0, 1], [0, 1, 0], [1, 1, 1]], bool))
    assert difference[0, 0] == F32(d[0]) and difference[1, 2] == F32(d[3])
    a = DepthAgreement(**record)
    assert a.mean_abs == record["sum_abs"] / 4 and a.rmse == math.sqrt(record["sum_sq"] / 4) and a.inlier_ratio == 0.75
    assert abs(a.mean_abs - 0.0125) < 1e-6 and abs(a.rmse - math.sqrt((1e-4 + 0 + 1e-4 + 9e-4) / 4)) < 1e-6
    assert a.rmse >= a.mean_abs >= 0
    empty = DepthAgreement()
    assert (empty.mean_abs, empty.rmse, empty.inlier_ratio) == (0.0, 0.0, 0.0)
    nothing, image = SU.compare_depth(np.full((2, 2, 1), -1, np.int64), np.zeros((2, 2, 1), F32), np.zeros((2, 2), np.uint16))
    assert nothing == dict(both=0, model_only=0, frame_only=0, inliers=0, sum_abs=0.0, sum_sq=0.0, max_abs=0.0) and np.isnan(image).all()
