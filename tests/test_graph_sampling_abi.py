"""CPU checks of the graph-sampling entry points (nnrt_get_vertex_erosion_mask, nnrt_sample_nodes): the host-side argument
checks fail with NNRT_ERROR_ARGUMENT and a message before anything is launched (pointers are never dereferenced, so
made-up device addresses serve), zero-size calls succeed, and the nnrt mirror binds both with the reference's parameter
names (cpp/pybind/nnrt_pybind.cpp:121-126)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

BASE = 0x7f0000000000
ARGUMENT = 1


@pytest.fixture(scope="module")
def native():
    from dynamicfuion_python_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def _p(offset):
    return ctypes.c_void_p(BASE + offset)


FACES, MASK, POINTS, ORDER, OUT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000


def _erosion(native, vertex_count=10, faces=_p(FACES), face_count=4, iterations=1, min_neighbors=4, out=_p(MASK)):
    lib = native.lib()
    st = lib.nnrt_get_vertex_erosion_mask(vertex_count, faces, face_count, iterations, min_neighbors, out, None)
    return st, lib.nnrt_last_error()


def _sample(native, points=_p(POINTS), count=10, mask=_p(MASK), order=_p(ORDER), coverage=0.05, out=_p(OUT), capacity=None, h_count=True,
            rounds=True):
    lib = native.lib()
    n = np.full(1, -1, np.int64)
    r = np.full(1, -1, np.int32)
    st = lib.nnrt_sample_nodes(points, count, mask, order, coverage, out, count if capacity is None else capacity,
                               native.ptr(n) if h_count else None, native.ptr(r) if rounds else None, None)
    return st, lib.nnrt_last_error(), int(n[0]), int(r[0])


@pytest.mark.parametrize("kwargs, message", [
    (dict(vertex_count=-1), b"vertex count"),
    (dict(face_count=-1), b"face count"),
    (dict(iterations=-1), b"iteration_count"),
    (dict(faces=None), b"null"),
    (dict(out=None), b"null"),
    (dict(out=_p(FACES + 8)), b"overlap"),
])
def test_erosion_mask_refuses_bad_arguments(native, kwargs, message):
    st, msg = _erosion(native, **kwargs)
    assert st == ARGUMENT
    assert msg.startswith(b"invalid argument") and message in msg


@pytest.mark.parametrize("kwargs, message", [
    (dict(points=None), b"null"),
    (dict(out=None), b"null"),
    (dict(h_count=False), b"null"),
    (dict(count=-1), b"point count"),
    (dict(coverage=0.0), b"node_coverage"),
    (dict(coverage=-0.05), b"node_coverage"),
    (dict(coverage=float("inf")), b"node_coverage"),
    (dict(coverage=float("nan")), b"node_coverage"),
    (dict(coverage=1e-30), b"node_coverage"),   # its square is not a normal float
    (dict(coverage=1e30), b"node_coverage"),    # its square overflows
    (dict(capacity=9), b"out_capacity"),
    (dict(out=_p(POINTS + 16)), b"overlap"),
    (dict(out=_p(MASK - 8)), b"overlap"),
    (dict(out=_p(ORDER + 8 * 9)), b"overlap"),
])
def test_sample_nodes_refuses_bad_arguments(native, kwargs, message):
    st, msg, _, _ = _sample(native, **kwargs)
    assert st == ARGUMENT
    assert msg.startswith(b"invalid argument") and message in msg


def test_zero_size_calls_succeed(native):
    assert _erosion(native, vertex_count=0, faces=None, face_count=0, out=None)[0] == 0
    assert _erosion(native, vertex_count=0, faces=None, face_count=0, iterations=10, out=None)[0] == 0
    st, _, n, r = _sample(native, points=None, count=0, mask=None, order=None, out=None)
    assert (st, n, r) == (0, 0, 0)
    st, _, n, _ = _sample(native, points=None, count=0, mask=None, order=None, out=None, rounds=False)   # h_out_rounds is nullable
    assert (st, n) == (0, 0)


def test_optional_inputs_pass_the_host_checks(native):
    """A null mask and a null order are valid (every vertex, ascending index): with them the overlap check still runs."""
    st, msg, _, _ = _sample(native, mask=None, order=None, out=_p(POINTS))
    assert st == ARGUMENT and b"overlap" in msg


def test_mirror_binds_the_reference_names():
    from dynamicfuion_python_amd import nnrt
    erosion = list(inspect.signature(nnrt.get_vertex_erosion_mask).parameters.values())
    assert [p.name for p in erosion] == ["vertex_positions", "face_indices", "iteration_count", "min_neighbors"]
    assert all(p.default is inspect.Parameter.empty for p in erosion)
    sample = list(inspect.signature(nnrt.sample_nodes).parameters.values())
    assert [p.name for p in sample] == ["vertex_positions_in", "vertex_erosion_mask_in", "node_coverage", "use_only_non_eroded_indices",
                                        "random_shuffle", "seed"]
    assert all(p.default is inspect.Parameter.empty for p in sample[:5]) and sample[5].default is None


def test_graph_builder_signature_and_pipeline_mode():
    from dynamicfuion_python_amd import fusion as F
    from dynamicfuion_python_amd.warp_field.graph_warp_field import build_deformation_graph_from_mesh
    params = list(inspect.signature(build_deformation_graph_from_mesh).parameters.values())
    assert [(p.name, p.default) for p in params[1:6]] == [("node_coverage", 0.05), ("erosion_iteration_count", 10),
                                                          ("erosion_min_neighbor_count", 4), ("neighbor_count", 8),
                                                          ("minimum_valid_anchor_count", 3)]
    assert params[0].name == "mesh" and all(p.kind == p.KEYWORD_ONLY for p in params[6:])
    assert {p.name: p.default for p in params[6:]} == {"anchor_count": 4, "layer_count": 2, "device": None}
    assert F.FusionParameters(graph_generation_mode=F.GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH).graph_erosion_iteration_count == 10
