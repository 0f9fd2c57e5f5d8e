"""RenderingAlignmentOptimizer.optimize_graph (alignment/render_based/rendering_alignment_optimizer.py:50-70 in the
reference, a stub there) implemented over the MI355X DeformableMeshToImageFitter, with the reference's
RenderingAlignmentParameters (settings/rendering_alignment.py:26-40) mapped onto the fitter's penalty switches.

The reference slot extracts the canonical mesh from the TSDF (`tsdf.extract_surface_mesh(-1, 0)`), renders the warped
mesh and fits the graph to the target point cloud; here the whole loop is one fit_to_image call (point-cloud overload,
DeformableMeshToImageFitter.cpp:85-276) on the GPU. The graph (a HierarchicalGraphWarpField) is updated in place.
"""
from __future__ import annotations

import enum
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ...nnrt import alignment as A
from ...nnrt import geometry as G


class PenaltyFunction(enum.Enum):
    """settings/rendering_alignment.py:20-23"""
    SQUARE = 1
    TUKEY = 2
    HUBER = 3


@dataclass
class RenderingAlignmentParameters:
    """settings/rendering_alignment.py:26-40 defaults, plus the fitter's own constructor defaults."""
    data_term_penalty_function: PenaltyFunction = PenaltyFunction.TUKEY
    data_term_penalty_constant: float = 0.01
    regularization_term_penalty_function: PenaltyFunction = PenaltyFunction.HUBER
    regularization_term_penalty_constant: float = 0.0001
    max_iteration_count: int = 100
    iteration_mode_sequence: tuple = (A.IterationMode.ALL,)
    preconditioning_dampening_factor: float = 0.001
    arap_term_weight: float = 200.0
    max_depth: float = 10.0
    use_perspective_correction: bool = True
    # A.NDC_REFERENCE reproduces the reference's y-mirrored render placement (A11); A.NDC_CONSISTENT is what real depth
    # frames need (the fusion pipeline's default)
    ndc_convention: int = A.NDC_REFERENCE
    # The form of the TUKEY / HUBER penalties and the zero-rotation guard (DeformableMeshToImageFitter.set_robust_options).
    # The defaults are the reference's arithmetic (quirks A8 / A9, NaN rotations A7); real sequences want
    # PenaltyForm.IRLS and guard_zero_rotation=True.
    penalty_form: A.PenaltyForm = A.PenaltyForm.REFERENCE
    guard_zero_rotation: bool = False
    # The data term's coupling across nodes (DeformableMeshToImageFitter.set_data_coupling): the reference's
    # block-diagonal Hessian by default; real sequences want DataCoupling.COUPLED (IterationMode.ALL only).
    data_coupling: A.DataCoupling = A.DataCoupling.BLOCK_DIAGONAL
    # On-device step control (DeformableMeshToImageFitter.set_step_control): None (default) runs every
    # iteration with the fixed damping, as the reference does; an A.StepControl keeps a step only if the cost fell.
    # IterationMode.ALL only. Under step_objective = StepObjective.SQUARE (default) SQUARE penalties (or
    # PenaltyForm.REFERENCE) only; StepObjective.ROBUST compares the robust cost, so PenaltyForm.IRLS
    # and step control run together: what real sequences want.
    step_control: Optional[A.StepControl] = None
    step_objective: A.StepObjective = A.StepObjective.SQUARE
    # The landmark term (DeformableMeshToImageFitter.set_landmarks) of optimize_graph(landmarks=...):
    # the fitter-wide residual weight (1.0 is untuned on any real sequence) and the distance cutoff in metres (0: none).
    landmark_term_weight: float = 1.0
    landmark_cutoff: float = 0.0


def as_triangle_mesh(mesh) -> G.TriangleMesh:
    """Accept this package's TriangleMesh or an Open3D-tensor-style mesh (vertex['positions'], vertex['normals'],
    triangle['indices'], each convertible with .numpy())."""
    if isinstance(mesh, G.TriangleMesh):
        return mesh
    try:
        def arr(t):
            return t.numpy() if hasattr(t, "numpy") else np.asarray(t)
        return G.TriangleMesh(arr(mesh.vertex["positions"]), arr(mesh.vertex["normals"]), arr(mesh.triangle["indices"]).astype(np.int64))
    except (AttributeError, KeyError, TypeError) as e:
        raise TypeError("canonical mesh must be a TriangleMesh or provide vertex['positions'/'normals'] and triangle['indices']") from e


class RenderingAlignmentOptimizer:
    def __init__(self, image_size_hw: Tuple[int, int], device=None, intrinsic_matrix=None,
                 parameters: RenderingAlignmentParameters | None = None):
        self.image_size_hw = (int(image_size_hw[0]), int(image_size_hw[1]))
        self.intrinsic_matrix = np.asarray(intrinsic_matrix, np.float64).reshape(3, 3)
        self.parameters = parameters or RenderingAlignmentParameters()
        p = self.parameters
        dev = None if device is None else (device.index if isinstance(device, torch.device) else int(device))
        self.fitter = A.DeformableMeshToImageFitter(
            max_iteration_count=p.max_iteration_count, iteration_mode_sequence=list(p.iteration_mode_sequence),
            use_perspective_correction=p.use_perspective_correction, max_depth=p.max_depth,
            use_tukey_penalty_for_data_term=p.data_term_penalty_function == PenaltyFunction.TUKEY,
            tukey_penalty_cutoff_cm=p.data_term_penalty_constant, preconditioning_dampening_factor=p.preconditioning_dampening_factor,
            arap_term_weight=p.arap_term_weight,
            use_huber_penalty_for_arap_term=p.regularization_term_penalty_function == PenaltyFunction.HUBER,
            huber_penalty_constant=p.regularization_term_penalty_constant, device=dev, ndc_convention=p.ndc_convention,
            penalty_form=p.penalty_form, guard_zero_rotation=p.guard_zero_rotation, step_objective=A.StepObjective(p.step_objective))
        self.fitter.set_data_coupling(A.DataCoupling(p.data_coupling))
        self.last_step_summary = None   # DeformableMeshToImageFitter.step_summary() of the last optimize_graph (step control on)
        if p.step_control is not None:
            self.fitter.set_step_control(p.step_control)

    def set_anchor_graph(self, edges):
        """Anchor the canonical mesh along these edge rows ([N, D] int32, the graph's virtual node order, -1 = empty) in
        every later optimize_graph call (AnchorComputationMode.SHORTEST_PATH); None: Euclidean anchors."""
        self.fitter.set_anchor_graph(edges)

    def optimize_graph(self, graph: G.HierarchicalGraphWarpField, tsdf, target_points, target_rgb=None, landmarks=None, extrinsics=None):
        """tsdf: an object with extract_surface_mesh(-1, 0) (NonRigidSurfaceVoxelBlockGrid) or the canonical mesh
        itself; target_points: organized [H,W,3] / [H*W,3] camera-space points (z <= 0 or non-finite = no target);
        extrinsics: the 4 x 4 world -> camera matrix the fitter applies to the mesh (None: identity);
        landmarks: (vertex_indices, targets, weights | None) for this fit (A.landmarks_from_pixel_matches makes one from
        2-D matches), None or an empty set: no landmark term."""
        mesh = tsdf.extract_surface_mesh(-1, 0) if hasattr(tsdf, "extract_surface_mesh") else tsdf
        mesh = as_triangle_mesh(mesh)
        if landmarks is not None and not (isinstance(landmarks, (tuple, list)) and len(landmarks) in (2, 3)):
            raise TypeError("landmarks must be a (vertex_indices, targets, weights | None) tuple; pass extrinsics by keyword")
        if landmarks is not None and len(landmarks[0]) > 0:
            self.fitter.set_landmarks(landmarks[0], landmarks[1], landmarks[2] if len(landmarks) > 2 else None,
                                      self.parameters.landmark_term_weight, self.parameters.landmark_cutoff)
        else:
            self.fitter.clear_landmarks()
        H, W = self.image_size_hw
        pts = target_points.detach() if isinstance(target_points, torch.Tensor) else torch.as_tensor(np.asarray(target_points))
        pts = pts.to(torch.float32).reshape(H * W, 3)
        valid = torch.isfinite(pts).all(dim=1) & (pts[:, 2] > 0)
        pts = torch.where(valid[:, None], pts, torch.zeros_like(pts))
        self.fitter.fit_to_image(graph, mesh, target_rgb, pts, valid.to(torch.uint8), self.intrinsic_matrix, extrinsics, (H, W))
        # what step control made of the fit (None while it is off)
        self.last_step_summary = self.fitter.step_summary() if self.parameters.step_control is not None else None
        return graph
