"""Mirror of the reference's Python `warp_field` package slot: graph construction from a mesh (warp_field/graph_warp_field.py)."""
from .graph_warp_field import build_deformation_graph_from_mesh, extend_warp_field, sample_graph_nodes_from_mesh  # noqa: F401
