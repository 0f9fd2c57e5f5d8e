"""Mirror of the reference `nnrt` module (cpp/pybind/nnrt_pybind.cpp:27-42) for the fitter hot path.

Submodules keep the reference names: nnrt.core.linalg, nnrt.geometry (+ .functional), nnrt.rendering (+ .functional),
and the new nnrt.alignment (DeformableMeshToImageFitter, IterationMode) that the reference never bound.
"""
from . import core, geometry, rendering, alignment, image_proc  # noqa: F401
from .image_proc import backproject_depth_ushort, backproject_depth_float  # noqa: F401  (nnrt_pybind.cpp:52-67)
from .image_proc import filter_depth  # noqa: F401  (nnrt_pybind.cpp:97-104)
from . import graph_proc  # noqa: F401
from .graph_proc import get_vertex_erosion_mask, sample_nodes  # noqa: F401  (nnrt_pybind.cpp:121-126)
from .image_proc import compute_mesh_from_depth  # noqa: F401  (nnrt_pybind.cpp:79-80)
from .graph_proc import compute_edges_shortest_path, node_and_edge_clean_up, compute_clusters  # noqa: F401  (:143-153, :219-225)
