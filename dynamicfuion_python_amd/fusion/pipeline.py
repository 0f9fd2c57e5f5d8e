"""DynamicFusion loop with a tracking-method switch (reference apps/fusion/pipeline.py:47-600).

The reference app always tracks with the DeformNet network (pipeline.py:356-365); the rendering-based optimizer it
prepared for the Gauss-Newton fitter is a stub (alignment/render_based/rendering_alignment_optimizer.py:50-70). Here the
switch `FusionParameters.tracking_method` selects

* `TrackingMethod.RENDERING` -- `RenderingAlignmentOptimizer` over the MI355X `DeformableMeshToImageFitter`: the canonical
  mesh extracted from the TSDF is fitted to each incoming depth frame on the GPU;
* `TrackingMethod.NEURAL` -- the reference's DeformNet path, which this build does not provide (raises).

Per frame, everything stays on the GPU: depth/colour upload, back-projection, ordered-point-cloud normals, the GN fit,
truncation-region block search, non-rigid TSDF integration and marching cubes. Graph generation samples the nodes from
the first frame's extracted mesh on the GPU (`GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH`), builds the reference's
default graph from the first masked depth image on the GPU (`FIRST_FRAME_DEPTH_IMAGE` together with
`FusionParameters.graph_from_depth_image=True`: pixel-connected mesh, erosion, node sampling, geodesic edges, clean-up,
clusters) -- both need nothing but depth frames --, uses the DeepDeformGraph file of the
first frame (`FIRST_FRAME_LOADED_GRAPH`) or nodes supplied by the caller.

Camera motion: with `FusionParameters.rigid_alignment=True` every tracked frame first aligns the previous frame's warped
mesh rigidly to the live point image on the GPU (`nnrt.alignment.align_rigid_point_to_plane`, DESIGN §17, or with
`rigid_alignment_photometric_weight > 0` the hybrid `align_rigid_hybrid`; the reference
calls Open3D's `rgbd_odometry_multi_scale` at pipeline.py:338-354 and drops its result) and hands the estimated
extrinsics to the fit and to the TSDF calls, so the warp field is left with the non-rigid residual. Off (the default),
the extrinsics stay the identity: a static camera.

Deviations: the mesh-extraction ramp counts processed frames, not frame-index differences (DeepDeform test
sequences ship sparse frames 300, 600, ...); the data and ARAP penalties default to SQUARE because the reference fitter's
Tukey and Huber branches carry quirks A8/A9 (real sequences should be run with the re-weighted forms instead, see
below); the fitter runs with NDC_CONSISTENT, because the reference's image -> NDC
mapping renders the mesh y-mirrored about cy (A11) and so fits a mirrored surface to a real depth frame.

`FusionParameters.anchor_computation_mode = AnchorComputationMode.SHORTEST_PATH` (reference pipeline.py:577-582) makes the
tracker anchor the canonical mesh along the motion graph's edges -- the DeepDeformGraph file's rows or the depth-image
graph's geodesic rows, re-indexed to the warp field's virtual node order -- instead of to the Euclidean-nearest nodes.
Only the fit uses these anchors: TSDF integration and `warp_mesh` keep the warp field's own Euclidean anchors, as in the
reference.

Real sequences: pass `FusionParameters(alignment=RenderingAlignmentParameters(data_term_penalty_function=
PenaltyFunction.TUKEY, regularization_term_penalty_function=PenaltyFunction.HUBER, penalty_form=PenaltyForm.IRLS,
guard_zero_rotation=True, ndc_convention=NDC_CONSISTENT, ...))`. With `PenaltyForm.IRLS` the penalties are iteratively
re-weighted least squares instead of the reference's branches: a masked-in pixel with point-to-plane residual r and
cutoff c contributes iff |r| <= c, and its residual and Jacobian row are scaled by s = 1 - (r / c)^2 (Tukey's biweight
(1 - (r / c)^2)^2 on the squared residual), so depth discontinuities, occlusion edges and sensor outliers carry no
weight; an ARAP edge's residual 3-vector r and its Jacobian terms are scaled by s = 1 if |r| <= delta else
sqrt(delta / |r|) (Huber's weight min(1, delta / |r|)). Hand-held sequences (DeepDeform's are) also want
`rigid_alignment=True`, and every real sequence wants `coupled_data_term=True`: the reference's block-diagonal data
Hessian overshoots from the second iteration on, the coupled step converges. Add `step_control=StepControl(...)` with `step_objective=StepObjective.ROBUST`
 so that a frame's fit cannot end at a higher robust cost than it began. `guard_zero_rotation=True` keeps the rotation of a node whose
rotation update is exactly zero (every node without pixels), where the reference's Rodrigues formula gives NaN (A7).
The defaults (`_default_alignment`) keep their values.
"""
from __future__ import annotations

import dataclasses
import enum
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from ..alignment.render_based.rendering_alignment_optimizer import (PenaltyFunction, RenderingAlignmentOptimizer,
                                                                     RenderingAlignmentParameters)
from ..data import camera as dcam
from ..data.frame import FrameSequenceDataset
from ..nnrt import geometry as G
from ..nnrt import image_proc
from ..nnrt import rendering
from ..nnrt.alignment import (NDC_CONSISTENT, DataCoupling, FeatureTracking, FeatureTrackLandmarks, StepControl, StepObjective,
                              align_rigid_hybrid, align_rigid_point_to_plane)
from ..warp_field.graph_warp_field import build_graph_nodes_from_depth_image, extend_warp_field, sample_graph_nodes_from_mesh


class TrackingMethod(enum.Enum):
    NEURAL = 0       # DeformNet (reference default); not part of this build
    RENDERING = 1    # DeformableMeshToImageFitter on the GPU


class TrackingSpanMode(enum.Enum):
    """settings/fusion.py: FIRST_TO_CURRENT keeps accumulating motion in one graph; PREVIOUS_TO_CURRENT restarts each
    fit from the previous frame's solution (identical for the GN fitter, which always starts from the graph's state)."""
    FIRST_TO_CURRENT = 0
    PREVIOUS_TO_CURRENT = 1


class GraphGenerationMode(enum.Enum):
    FIRST_FRAME_EXTRACTED_MESH = 0   # nodes sampled from the first frame's extracted mesh (build_deformation_graph_from_mesh)
    FIRST_FRAME_DEPTH_IMAGE = 1      # the reference's default: the graph of the first masked depth image (create_graph_data.py:27-296);
                                     # needs FusionParameters.graph_from_depth_image=True
    FIRST_FRAME_LOADED_GRAPH = 2     # DeepDeformGraph .bin files of the first frame
    PROVIDED_NODES = 3               # nodes handed to FusionPipeline(nodes=...)


class AnchorComputationMode(enum.Enum):
    """apps/fusion/pipeline.py AnchorComputationMode: how the tracker anchors canonical vertices to graph nodes."""
    EUCLIDEAN = 0
    SHORTEST_PATH = 1   # along the graph's edge rows: FIRST_FRAME_LOADED_GRAPH or FIRST_FRAME_DEPTH_IMAGE only


class MeshExtractionWeightThresholdingMode(enum.Enum):
    CONSTANT = 0
    RAMP_UP_TO_CONSTANT = 1


def _default_alignment() -> RenderingAlignmentParameters:
    return RenderingAlignmentParameters(data_term_penalty_function=PenaltyFunction.SQUARE,
                                        regularization_term_penalty_function=PenaltyFunction.SQUARE, max_iteration_count=10,
                                        ndc_convention=NDC_CONSISTENT)


@dataclass
class FusionParameters:
    """The subset of the reference's Parameters tree the loop reads (settings/tsdf.py, settings/fusion.py,
    settings/graph.py, settings/rendering_alignment.py)."""
    tracking_method: TrackingMethod = TrackingMethod.RENDERING
    tracking_span_mode: TrackingSpanMode = TrackingSpanMode.FIRST_TO_CURRENT
    graph_generation_mode: GraphGenerationMode = GraphGenerationMode.FIRST_FRAME_LOADED_GRAPH
    anchor_computation_mode: AnchorComputationMode = AnchorComputationMode.EUCLIDEAN
    mesh_extraction_weight_thresholding_mode: MeshExtractionWeightThresholdingMode = MeshExtractionWeightThresholdingMode.RAMP_UP_TO_CONSTANT
    mesh_extraction_weight_threshold: int = 10
    voxel_size: float = 0.005
    sdf_truncation_distance: float = 0.025
    block_resolution: int = 16
    initial_block_count: int = 1000
    depth_scale: float = 1000.0
    node_coverage: float = 0.05
    anchor_node_count: int = 4
    fusion_minimum_valid_anchor_count: int = 3
    graph_layer_count: int = 2   # the fitter's ARAP arrowhead configuration with reference parity (quirk A3)
    graph_erosion_iteration_count: int = 10    # FIRST_FRAME_EXTRACTED_MESH (pipeline.py:518)
    graph_erosion_min_neighbor_count: int = 4  # build_deformation_graph_from_mesh's default
    # FIRST_FRAME_DEPTH_IMAGE (settings/graph.py). The mode is opt-in: without graph_from_depth_image=True the pipeline
    # refuses it at construction, as it did before the depth-image builder existed.
    graph_from_depth_image: bool = False
    graph_max_triangle_distance: float = 0.05
    graph_depth_image_erosion_iteration_count: int = 4
    graph_depth_image_erosion_min_neighbor_count: int = 4
    graph_neighbor_count: int = 8
    graph_enforce_neighbor_count: bool = False
    graph_remove_nodes_with_too_few_neighbors: bool = True
    graph_use_only_valid_vertices: bool = True
    graph_sample_random_shuffle: bool = False
    # rigid frame-to-model alignment ahead of the non-rigid fit; off: the extrinsics stay the identity
    rigid_alignment: bool = False
    rigid_alignment_iteration_counts: tuple = (6, 3, 1)   # coarse to fine
    rigid_alignment_distance_threshold: float = 0.07
    rigid_alignment_normal_agreement_cos: float = 0.5
    # the hybrid alignment (align_rigid_hybrid): above 0, and where the previous warped mesh has vertex colours,
    # the rigid step adds a photometric term of this weight against the frame's colour image, which holds the directions
    # point-to-plane slides along. Metres per unit of intensity; 0.1 is 5 mm of assumed depth noise over 0.05 of assumed
    # intensity noise and has not been tuned on any sequence. 0 (the default): the geometric call, bit for bit as before.
    rigid_alignment_photometric_weight: float = 0.0
    rigid_alignment_photometric_residual_threshold: float = 0.0   # drop photometric rows with |rI| above this; <= 0: keep all
    # grow the motion graph over surface fused beyond its nodes' support, after every tracked frame (extend_warp_field,
    # DESIGN §18), and let non-rigid integration take newly seen surface into the model
    # (NonRigidSurfaceVoxelBlockGrid.set_non_rigid_surface_growth); off: the nodes are the first frame's for the whole run
    warp_field_extension: bool = False
    warp_field_extension_support_ratio: float = 1.0
    warp_field_extension_minimum_new_node_count: int = 1
    # depth filters ahead of tracking: with either radius positive, tracked frames back-project a filtered
    # copy of the depth for the rigid alignment, the fit and the normals; TSDF integration always takes the raw frame.
    # Median first (zero-skipping, holes kept), then the bilateral smoother on its result. Radii up to 8; 0: off.
    # depth_bilateral_spatial_sigma 0 means depth_bilateral_radius / 2. depth_bilateral_range_sigma is in sensor units:
    # 30 is KinectFusion's conventional 30 mm and has not been tuned on any sequence here.
    depth_median_radius: int = 0
    depth_bilateral_radius: int = 0
    depth_bilateral_spatial_sigma: float = 0.0
    depth_bilateral_range_sigma: float = 30.0
    # score every tracked frame: after the fit and before integration the freshly warped canonical mesh is
    # rasterized in the live camera and its depth compared with the raw depth frame; FrameResult.model_* hold the result.
    # Reads the graph and the canonical mesh only.
    model_agreement: bool = False
    model_agreement_inlier_threshold: float = 0.01   # metres
    alignment: RenderingAlignmentParameters = field(default_factory=_default_alignment)
    # the full Gauss-Newton step (DataCoupling.COUPLED) in place of the reference's block-diagonal data
    # Hessian; real sequences should turn it on. Overrides alignment.data_coupling when set.
    coupled_data_term: bool = False
    # on-device step control of the non-rigid fit (StepControl): a step is kept only if the cost fell, so a
    # frame's fit cannot end worse than it began. Overrides alignment.step_control when set.
    step_control: Optional[StepControl] = None
    # the cost step control compares (StepObjective): SQUARE allows SQUARE penalties only (this loop's
    # default); ROBUST goes with the TUKEY / HUBER penalties in PenaltyForm.IRLS. Overrides alignment.step_objective when set.
    step_objective: Optional[StepObjective] = None
    # landmarks from the colour frames (FeatureTracking): when set, and no landmark_provider is given, the
    # pipeline tracks sparse features from each colour frame to the next and feeds them to the fit's landmark term. None
    # (the default): nothing is launched or allocated for it.
    landmark_tracking: Optional[FeatureTracking] = None
    # the tracked model's own motion field: after every tracked frame's fit, the canonical mesh warped by the
    # graph as it was before the fit, in the previous frame's camera, and by the fitted graph in the new camera are
    # rendered to scene-flow and optical-flow images on the previous frame's pixel grid (FusionPipeline.last_motion), which
    # a flow_truth_provider's ground truth is scored against. Reads the graph and the canonical mesh only. Off (the
    # default): nothing is launched or allocated for it. No default of this project has been tuned with it yet.
    motion_images: bool = False


def alignment_parameters(p: FusionParameters) -> RenderingAlignmentParameters:
    """The optimizer's parameters for these fusion parameters: p.alignment, in DataCoupling.COUPLED mode when
    coupled_data_term is set and with step_control / step_objective where those are set."""
    a = dataclasses.replace(p.alignment, data_coupling=DataCoupling.COUPLED) if p.coupled_data_term else p.alignment
    if p.step_objective is not None:
        a = dataclasses.replace(a, step_objective=p.step_objective)
    return dataclasses.replace(a, step_control=p.step_control) if p.step_control is not None else a


@dataclass
class FrameResult:
    frame_index: int
    canonical_vertex_count: int = 0
    canonical_triangle_count: int = 0
    tracked: bool = False
    new_block_count: int = 0       # blocks activated for this frame
    active_block_count: int = 0    # blocks in the volume after integration
    seconds: float = 0.0
    rigid_correspondence_count: int = 0   # rigid alignment: correspondences and RMSE of its last iteration (0 when it did not run)
    rigid_inlier_rmse: float = 0.0
    rigid_photometric_count: int = 0      # hybrid rigid alignment: photometric rows and intensity RMSE of its last iteration
    rigid_photometric_rmse: float = 0.0
    extrinsics: Optional[np.ndarray] = None   # a copy of the world -> camera matrix this frame was tracked and fused with
    node_count: int = 0       # nodes of the motion graph after this frame
    new_node_count: int = 0   # of them, added by this frame's warp field extension
    depth_filtered: bool = False   # tracked against filtered depth (depth_median_radius / depth_bilateral_radius)
    # FusionParameters.model_agreement: the warped model's rasterized depth against the raw frame (0 when not measured):
    # pixels valid on both sides, on the model's only, on the frame's only; over the first, mean |difference| and RMS
    # difference in metres and the share within model_agreement_inlier_threshold
    model_overlap_count: int = 0
    model_only_count: int = 0
    frame_only_count: int = 0
    model_depth_mean_abs: float = 0.0
    model_depth_rmse: float = 0.0
    model_inlier_ratio: float = 0.0
    # FusionParameters.step_control (0 while it is off): iterations up to and including the one that stopped the fit, the
    # cost of the state the fit ended on, and the steps it rejected
    iterations_used: int = 0
    final_cost: float = 0.0
    rejected_step_count: int = 0
    # FusionPipeline(landmark_provider=...) (0 without one): the landmarks the provider gave for this frame, those active
    # at the state the fit's last iteration started from, and the RMS of their distances |warped vertex - target| (metres)
    landmark_count: int = 0
    landmark_active_count: int = 0
    landmark_rmse: float = 0.0
    # FusionParameters.landmark_tracking (0 without it): the features selected in the previous colour frame; landmark_count
    # counts those that survived tracking and the match filter
    tracked_feature_count: int = 0
    # FusionParameters.motion_images (0 without it): the pixels of the model's motion field that are valid; with a
    # FusionPipeline(flow_truth_provider=...) that gave scene flow (metres) / optical flow (pixels) for this frame, the
    # pixels valid in both the field and the truth and, over them, the mean and the RMS end-point error
    motion_pixel_count: int = 0
    scene_flow_count: int = 0
    scene_flow_epe_mean: float = 0.0
    scene_flow_rmse: float = 0.0
    optical_flow_count: int = 0
    optical_flow_epe_mean: float = 0.0
    optical_flow_rmse: float = 0.0


def remap_edges_to_node_order(edges, order) -> np.ndarray:
    """Edge rows [N, D] over nodes in their original order -> rows over the same nodes re-ordered by `order` (order[v] = the
    original index of new node v): row v is the row of node order[v] with every entry replaced by its new index; negative
    entries (empty) are kept as -1."""
    edges = np.asarray(edges, np.int32)
    order = np.asarray(order, np.int64)
    if edges.ndim != 2 or order.shape != (edges.shape[0],) or not np.array_equal(np.sort(order), np.arange(len(order))):
        raise ValueError(f"`order` must be a permutation of the {edges.shape[0] if edges.ndim == 2 else '?'} edge rows")
    if (edges >= len(order)).any():
        raise ValueError("edge entry outside [-1, node count)")
    inverse = np.empty(len(order), np.int32)
    inverse[order] = np.arange(len(order), dtype=np.int32)
    rows = edges[order]
    return np.ascontiguousarray(np.where(rows >= 0, inverse[np.maximum(rows, 0)], -1).astype(np.int32))


class FusionPipeline:
    def __init__(self, sequence: FrameSequenceDataset, parameters: Optional[FusionParameters] = None, nodes=None,
                 device: Optional[int] = None, landmark_provider=None, flow_truth_provider=None):
        """landmark_provider: a callable (pipeline, frame, canonical_mesh, point_image) -> (vertex_indices, targets,
        weights | None) | None, called for every tracked frame before its non-rigid fit: the sparse correspondences of the
        fit's landmark term (nnrt.alignment.landmarks_from_pixel_matches makes the tuple from 2-D
        matches). None: no landmark term, unless FusionParameters.landmark_tracking is set: the pipeline then owns a
        FeatureTrackLandmarks, hands it every frame's colour image and uses it as the provider. Both given: refused.

        flow_truth_provider: a callable (pipeline, frame) -> dict | None, called for every tracked frame after its motion
        field was rendered (FusionParameters.motion_images, which it needs): ground-truth flow from the previous frame to
        this one on the previous frame's pixel grid, under any of the keys "scene_flow" [H, W, 3] (metres),
        "scene_flow_mask" [H, W], "optical_flow" [H, W, 2] (pixels), "optical_flow_mask" [H, W]
        (data.io.load_flow_with_mask gives such pairs). The end-point errors go to the frame's FrameResult."""
        self.parameters = p = parameters or FusionParameters()
        if flow_truth_provider is not None and not p.motion_images:
            raise ValueError("flow_truth_provider needs FusionParameters.motion_images=True: the truth is scored against the rendered "
                             "motion field")
        self.flow_truth_provider = flow_truth_provider
        if landmark_provider is not None and p.landmark_tracking is not None:
            raise ValueError("both landmark_provider and FusionParameters.landmark_tracking are given: the pipeline takes landmarks from one "
                             "source; drop one of the two")
        self.feature_tracker = FeatureTrackLandmarks(p.landmark_tracking) if p.landmark_tracking is not None else None
        self.landmark_provider = landmark_provider if self.feature_tracker is None else self.feature_tracker
        if p.tracking_method == TrackingMethod.NEURAL:
            raise NotImplementedError("TrackingMethod.NEURAL (DeformNet) is not part of this build; use TrackingMethod.RENDERING")
        if p.graph_generation_mode == GraphGenerationMode.FIRST_FRAME_DEPTH_IMAGE and not p.graph_from_depth_image:
            raise NotImplementedError(f"graph generation mode {p.graph_generation_mode.name} runs only with "
                                      "FusionParameters.graph_from_depth_image=True (the depth-image graph builder on the GPU)")
        if p.anchor_computation_mode == AnchorComputationMode.SHORTEST_PATH and p.graph_generation_mode not in (
                GraphGenerationMode.FIRST_FRAME_LOADED_GRAPH, GraphGenerationMode.FIRST_FRAME_DEPTH_IMAGE):
            raise NotImplementedError(f"AnchorComputationMode.SHORTEST_PATH needs a graph with edge rows; graph generation mode "
                                      f"{p.graph_generation_mode.name} has none (use FIRST_FRAME_LOADED_GRAPH or FIRST_FRAME_DEPTH_IMAGE)")
        if p.warp_field_extension and p.anchor_computation_mode == AnchorComputationMode.SHORTEST_PATH:
            raise NotImplementedError("warp_field_extension adds nodes without edge rows, which AnchorComputationMode.SHORTEST_PATH "
                                      "anchors along; use AnchorComputationMode.EUCLIDEAN")
        if p.graph_generation_mode == GraphGenerationMode.PROVIDED_NODES and nodes is None:
            raise ValueError("GraphGenerationMode.PROVIDED_NODES needs nodes=")
        for name in ("depth_median_radius", "depth_bilateral_radius"):
            if not 0 <= getattr(p, name) <= 8:
                raise ValueError(f"FusionParameters.{name} must be in [0, 8], got {getattr(p, name)}")
        self.sequence = sequence if sequence._loaded else sequence.load()
        self.device = torch.cuda.current_device() if device is None else int(device)
        first = self.sequence.get_frame_at(self.sequence.start_frame_index)
        self.intrinsics, _ = dcam.load_open3d_intrinsics_from_text_4x4_matrix_and_image(self.sequence.get_intrinsics_path(),
                                                                                        first.get_depth_image_path())
        self.K = self.intrinsics.intrinsic_matrix
        self.fx, self.fy, self.cx, self.cy = dcam.extract_intrinsic_projection_parameters(self.intrinsics)
        self.extrinsics = np.eye(4)
        self.volume = G.NonRigidSurfaceVoxelBlockGrid(["tsdf", "weight", "color"], ["float32", "uint16", "uint16"], [1, 1, 3],
                                                      voxel_size=p.voxel_size, block_resolution=p.block_resolution,
                                                      block_count=p.initial_block_count, device=self.device)
        if p.warp_field_extension:
            # new nodes are sampled on fused surface: the model has to be able to take in surface it first sees while tracking
            self.volume.set_non_rigid_surface_growth(True)
        self.truncation_voxel_multiplier = p.sdf_truncation_distance / p.voxel_size
        self._provided_nodes = nodes
        self.active_graph: Optional[G.HierarchicalGraphWarpField] = None
        # FIRST_FRAME_EXTRACTED_MESH / FIRST_FRAME_DEPTH_IMAGE: the mesh the nodes were sampled from and the nodes in
        # sampling order (before make_warp_field's re-ordering; DEPTH_IMAGE: after the clean-up), device tensors
        self.graph_source_mesh = None
        self.sampled_node_positions = None
        self.sampled_node_vertex_indices = None
        # FIRST_FRAME_DEPTH_IMAGE: the DepthImageGraph, its edges / weights / distances and its clusters
        self.depth_image_graph = None
        self.geodesic_edges = None
        self.graph_clusters = None
        # make_warp_field: the index, in the nodes it was given, of each node of the warp field it returned; with
        # warp_field_extension, the index in [the first frame's nodes; the nodes added since, in the order they were added]
        self.node_order = None
        # SHORTEST_PATH: the graph's edge rows in the warp field's virtual node order, as handed to the optimizer
        self.anchor_graph_edges = None
        self.optimizer = RenderingAlignmentOptimizer((self.intrinsics.height, self.intrinsics.width), self.device, self.K,
                                                     alignment_parameters(p))
        self.canonical_mesh = None
        self.warped_mesh = None
        # the point image the last tracked frame was aligned and fitted to, and whose normals gated its integration
        self.tracking_point_image = None
        # FusionParameters.motion_images: the MotionImages of the last tracked frame, on the previous frame's pixel grid
        self.last_motion = None
        self.processed_frames = 0
        self.results: List[FrameResult] = []

    # -- helpers ------------------------------------------------------------------------------------------------
    def _load_frame(self, frame):
        depth = frame.load_depth_image_numpy()
        color = frame.load_color_image_rgb()
        if self.sequence.far_clipping_distance_mm > 0:
            far = depth > self.sequence.far_clipping_distance_mm
            depth[far] = 0
            color[far] = 0
        if self.sequence.has_masks():
            masked = frame.load_mask_image_numpy() < self.sequence.mask_lower_threshold
            depth[masked] = 0
            color[masked] = 0
        dev = torch.device("cuda", self.device)
        depth_t = torch.from_numpy(depth.view(np.int16)).to(dev).view(torch.uint16)
        color_t = torch.from_numpy(np.ascontiguousarray(color)).to(dev)
        return depth, depth_t, color_t

    def _depth_max(self) -> float:
        far = self.sequence.far_clipping_distance
        return far if far > 0 else 3.0

    def mesh_extraction_threshold(self) -> int:
        """pipeline.py:450-460, counting processed frames."""
        p = self.parameters
        if p.mesh_extraction_weight_thresholding_mode == MeshExtractionWeightThresholdingMode.CONSTANT:
            return p.mesh_extraction_weight_threshold
        return min(self.processed_frames - 1, p.mesh_extraction_weight_threshold)

    def _initialize_graph(self, depth=None):
        """`depth`: the first frame's depth on the device, masked and clipped (FIRST_FRAME_DEPTH_IMAGE)."""
        p = self.parameters
        edge_rows = None
        if p.graph_generation_mode == GraphGenerationMode.FIRST_FRAME_LOADED_GRAPH:
            name = self.sequence.get_current_graph_name()
            if name is None:
                raise ValueError("no DeepDeformGraph file starts at the first frame")
            nodes, edge_rows = self.sequence.load_graph_data(name)[:2]
        elif p.graph_generation_mode == GraphGenerationMode.FIRST_FRAME_EXTRACTED_MESH:
            # pipeline.py:514-520: the mesh at weight threshold 0, erosion_iteration_count = 10
            self.graph_source_mesh = self.volume.extract_triangle_mesh(0.0, -1)
            self.sampled_node_positions, self.sampled_node_vertex_indices = sample_graph_nodes_from_mesh(
                self.graph_source_mesh, p.node_coverage, p.graph_erosion_iteration_count, p.graph_erosion_min_neighbor_count)
            if self.sampled_node_positions.shape[0] == 0:
                raise ValueError("no graph node was sampled from the first frame's mesh (empty or fully eroded)")
            nodes = self.sampled_node_positions.cpu().numpy()
        elif p.graph_generation_mode == GraphGenerationMode.FIRST_FRAME_DEPTH_IMAGE:
            # pipeline.py:522-540 with settings/graph.py; the warp field's own edges come from the hierarchy
            g = build_graph_nodes_from_depth_image(
                depth, None, self.K, max_triangle_distance=p.graph_max_triangle_distance, depth_scale_reciprocal=p.depth_scale,
                erosion_num_iterations=p.graph_depth_image_erosion_iteration_count,
                erosion_min_neighbors=p.graph_depth_image_erosion_min_neighbor_count,
                remove_nodes_with_too_few_neighbors=p.graph_remove_nodes_with_too_few_neighbors,
                use_only_valid_vertices=p.graph_use_only_valid_vertices, sample_random_shuffle=p.graph_sample_random_shuffle,
                neighbor_count=p.graph_neighbor_count, enforce_neighbor_count=p.graph_enforce_neighbor_count, node_coverage=p.node_coverage)
            self.depth_image_graph = g
            self.graph_source_mesh = G.TriangleMesh(g.vertices, None, g.faces.to(torch.int64))
            self.sampled_node_positions, self.sampled_node_vertex_indices = g.node_positions, g.node_vertex_indices
            self.geodesic_edges, self.graph_clusters = g.edges, g.clusters
            nodes = g.node_positions.cpu().numpy()
            edge_rows = g.edges.cpu().numpy()
        else:
            nodes = np.asarray(self._provided_nodes, np.float32)
        self.active_graph = self.make_warp_field(nodes)
        if p.anchor_computation_mode == AnchorComputationMode.SHORTEST_PATH:
            # the fitter computes anchors in the warp field's virtual node order
            virtual_order = self.node_order[self.active_graph.get_virtual_node_indices()]
            self.anchor_graph_edges = remap_edges_to_node_order(edge_rows, virtual_order)
            self.optimizer.set_anchor_graph(self.anchor_graph_edges)

    def make_warp_field(self, nodes) -> G.HierarchicalGraphWarpField:
        """Hierarchical warp field over `nodes`, re-ordered toward the hierarchy's virtual order first (a few passes) so the
        virtual -> original permutation is the identity where the median-grid subsample allows it (reference quirk A5:
        anchors use virtual order, WarpMesh original order)."""
        p = self.parameters

        def build(n):
            return G.HierarchicalGraphWarpField(n, node_coverage=p.node_coverage, anchor_count=p.anchor_node_count,
                                                minimum_valid_anchor_count=p.fusion_minimum_valid_anchor_count,
                                                layer_count=p.graph_layer_count, device=self.device)
        nodes = np.ascontiguousarray(nodes, np.float32)
        order = np.arange(len(nodes))
        wf = build(nodes)
        for _ in range(3):
            vidx = wf.get_virtual_node_indices()
            if np.array_equal(vidx, np.arange(len(nodes))):
                break
            nodes = nodes[vidx]
            order = order[vidx]
            wf = build(nodes)
        self.node_order = order
        return wf

    def _extend_graph(self) -> int:
        """New nodes over the canonical surface the graph does not support yet, moving with the current warp; the number
        added. The optimizer needs no reset: the fitter rebuilds its per-graph state for a warp field it has not prepared
        (it recognises fields by a unique id), and TSDF integration and warp_mesh read the field they are handed."""
        p = self.parameters
        previous_order = self.node_order
        graph, order, added = extend_warp_field(self.active_graph, self.canonical_mesh, lambda nodes: (self.make_warp_field(nodes), self.node_order),
                                                p.warp_field_extension_support_ratio, p.warp_field_extension_minimum_new_node_count)
        if graph is self.active_graph:
            return 0
        self.active_graph = graph
        self.node_order = np.concatenate([previous_order, np.arange(len(previous_order), len(order))])[order]
        return int(added.shape[0])

    def extract_canonical_mesh(self):
        mesh = self.volume.extract_triangle_mesh(float(self.mesh_extraction_threshold()), -1)
        return mesh

    def render_canonical_model(self, render_attributes=("depth", "normal"), extrinsics=None, weight_threshold=None):
        """Ray-cast the canonical volume over all of its blocks with the sequence's intrinsics and image size
        (VoxelBlockGrid.ray_cast): a dict of device tensors, "range" and one map per attribute. `extrinsics`
        defaults to the loop's current camera, `weight_threshold` to mesh_extraction_threshold(); the truncation
        multiplier, depth scale and far limit are the loop's own. Nothing in the loop calls this."""
        E = self.extrinsics if extrinsics is None else extrinsics
        threshold = self.mesh_extraction_threshold() if weight_threshold is None else weight_threshold
        return self.volume.ray_cast(self.volume.get_block_coordinates(), self.K, E, self.intrinsics.width, self.intrinsics.height,
                                    render_attributes, depth_scale=self.parameters.depth_scale, depth_max=self._depth_max(),
                                    weight_threshold=float(threshold), trunc_voxel_multiplier=self.truncation_voxel_multiplier)

    def _warped_model_in_camera(self, extrinsics=None):
        if self.active_graph is None or self.canonical_mesh is None or self.canonical_mesh.triangle_indices.shape[0] == 0:
            raise RuntimeError("there is no canonical mesh to warp yet: process a frame first")
        E = self.extrinsics if extrinsics is None else extrinsics
        return self.active_graph.warp_mesh(self.canonical_mesh, extrinsics=E)

    def render_warped_model(self, shader=None, extrinsics=None):
        """Draw the canonical mesh warped by the current graph with the sequence's intrinsics and image size:
        (image uint8 [H, W, 3], fragments), raster pixel (u, v) being pixel (u, v) of the depth frames. `extrinsics`
        defaults to the loop's current camera, `shader` to VertexColorShader when the mesh has colours, else
        HeadlightShader. Nothing in the default loop calls this."""
        mesh = self._warped_model_in_camera(extrinsics)
        if shader is None:
            shader = rendering.VertexColorShader() if mesh.vertex_colors is not None else rendering.HeadlightShader()
        return rendering.render_meshes(mesh, self.K, (self.intrinsics.height, self.intrinsics.width), shader,
                                       ndc_convention=rendering.NDC_CONSISTENT)

    def measure_model_agreement(self, depth):
        """(DepthAgreement, difference image) of the warped canonical mesh's rasterized depth against `depth`, a raw depth
        frame, in the loop's current camera and with its depth scale and far limit."""
        p = self.parameters
        fragments, _ = rendering.rasterize_meshes(self._warped_model_in_camera(), self.K, (self.intrinsics.height, self.intrinsics.width),
                                                  ndc_convention=rendering.NDC_CONSISTENT)
        return rendering.compare_depth_to_raster(fragments[0], fragments[1], depth, p.depth_scale, self._depth_max(),
                                                 p.model_agreement_inlier_threshold)

    def render_model_motion(self, source_graph, source_extrinsics, target_graph=None, target_extrinsics=None):
        """(MotionImages, fragments) of the current canonical mesh between two states of the warp field: warped
        by `source_graph` and seen by the camera `source_extrinsics`, against warped by `target_graph` and seen by
        `target_extrinsics`, which default to the loop's current graph and camera. The images are on the source camera's
        pixel grid, raster pixel (u, v) being pixel (u, v) of the depth frames. Both graphs must be over the node set the
        canonical mesh is anchored to."""
        if self.active_graph is None or self.canonical_mesh is None or self.canonical_mesh.triangle_indices.shape[0] == 0:
            raise RuntimeError("there is no canonical mesh to warp yet: process a frame first")
        target_graph = self.active_graph if target_graph is None else target_graph
        target_extrinsics = self.extrinsics if target_extrinsics is None else target_extrinsics
        source = source_graph.warp_mesh(self.canonical_mesh, extrinsics=source_extrinsics)
        target = target_graph.warp_mesh(self.canonical_mesh, extrinsics=target_extrinsics)
        return rendering.render_motion(source, target.vertex_positions, self.K, (self.intrinsics.height, self.intrinsics.width),
                                       ndc_convention=rendering.NDC_CONSISTENT)

    def _score_motion(self, frame, res):
        """FrameResult's flow fields from last_motion and, if there is a provider with truth for this frame, its truth."""
        motion = self.last_motion
        res.motion_pixel_count = int(motion.mask.sum())
        truth = self.flow_truth_provider(self, frame) if self.flow_truth_provider is not None else None
        if not truth:
            return
        # the inlier count is not reported, so the threshold only has to be legal
        if truth.get("scene_flow") is not None:
            a, _ = rendering.compare_flow(motion.scene_flow, motion.mask, truth["scene_flow"], truth.get("scene_flow_mask"), inlier_threshold=0.0)
            res.scene_flow_count, res.scene_flow_epe_mean, res.scene_flow_rmse = a.both, a.mean_epe, a.rmse
        if truth.get("optical_flow") is not None:
            a, _ = rendering.compare_flow(motion.optical_flow, motion.mask, truth["optical_flow"], truth.get("optical_flow_mask"),
                                          inlier_threshold=0.0)
            res.optical_flow_count, res.optical_flow_epe_mean, res.optical_flow_rmse = a.both, a.mean_epe, a.rmse

    def filtered_point_image(self, depth):
        """The point image tracked frames use when a depth filter is on: the median with holes kept, then the bilateral
        smoother on its result, back-projected. `depth`: the frame's uint16 depth on the device, which is
        left as it is: the volume integrates the raw frame."""
        p = self.parameters
        filtered = image_proc.filter_depth(depth, p.depth_median_radius, preserve_zero=True) if p.depth_median_radius > 0 else depth
        if p.depth_bilateral_radius == 0:
            return image_proc.backproject_depth_ushort(filtered, self.fx, self.fy, self.cx, self.cy, p.depth_scale)
        spatial_sigma = p.depth_bilateral_spatial_sigma if p.depth_bilateral_spatial_sigma > 0 else p.depth_bilateral_radius / 2.0
        metres = image_proc.bilateral_filter_depth(filtered, p.depth_bilateral_radius, spatial_sigma, p.depth_bilateral_range_sigma,
                                                   depth_scale=p.depth_scale)
        return image_proc.backproject_depth_float(metres, self.fx, self.fy, self.cx, self.cy)

    # -- the loop -----------------------------------------------------------------------------------------------
    def process_frame(self, frame) -> FrameResult:
        t0 = time.perf_counter()
        p = self.parameters
        depth_np, depth, color = self._load_frame(frame)
        self.processed_frames += 1
        res = FrameResult(frame.frame_index)
        if self.feature_tracker is not None:
            self.feature_tracker.advance(color, self.extrinsics)   # the extrinsics are still the previous frame's here
        depth_max = self._depth_max()
        if self.active_graph is None:
            # canonical frame: rigid integration, then the motion graph (pipeline.py:224-248)
            blocks = self.volume.compute_unique_block_coordinates(depth, self.K, self.extrinsics, p.depth_scale, depth_max,
                                                                  self.truncation_voxel_multiplier)
            self.volume.integrate(blocks, depth, color, self.K, self.K, self.extrinsics, p.depth_scale, depth_max,
                                  self.truncation_voxel_multiplier)
            self._initialize_graph(depth)
            res.new_block_count = int(blocks.shape[0])
        else:
            # track: fit the canonical mesh extracted at the end of the previous frame to this frame's depth (the
            # tracking-method switch, pipeline.py:356-365)
            canonical = self.canonical_mesh
            if p.motion_images:
                # the state the fit starts from and the camera it was seen by: the previous frame's
                graph_before, extrinsics_before = self.active_graph.clone(), np.array(self.extrinsics, np.float64)
            if p.depth_median_radius > 0 or p.depth_bilateral_radius > 0:
                points = self.filtered_point_image(depth)
                res.depth_filtered = True
            else:
                points = image_proc.backproject_depth_ushort(depth, self.fx, self.fy, self.cx, self.cy, p.depth_scale)
            self.tracking_point_image = points
            res.canonical_vertex_count, res.canonical_triangle_count = canonical.vertex_positions.shape[0], canonical.triangle_indices.shape[0]
            if p.rigid_alignment and self.warped_mesh is not None and self.warped_mesh.triangle_indices.shape[0] > 0:
                # the camera's motion since the previous frame, before the non-rigid fit (pipeline.py:338-354): the warped
                # surface as of the previous frame (world coordinates) against the live points
                schedule = dict(initial_transformation=self.extrinsics, iteration_counts=p.rigid_alignment_iteration_counts,
                                distance_threshold=p.rigid_alignment_distance_threshold,
                                normal_agreement_cos=p.rigid_alignment_normal_agreement_cos)
                if p.rigid_alignment_photometric_weight > 0 and self.warped_mesh.vertex_colors is not None:
                    rigid = align_rigid_hybrid(
                        self.warped_mesh.vertex_positions, self.warped_mesh.vertex_normals, self.warped_mesh.vertex_colors, points, color,
                        self.K, photometric_weight=p.rigid_alignment_photometric_weight,
                        photometric_residual_threshold=p.rigid_alignment_photometric_residual_threshold, **schedule)
                else:
                    rigid = align_rigid_point_to_plane(self.warped_mesh.vertex_positions, self.warped_mesh.vertex_normals, points, self.K,
                                                       **schedule)
                if rigid.status == 0:
                    self.extrinsics = rigid.transformation
                res.rigid_correspondence_count, res.rigid_inlier_rmse = rigid.correspondence_count, rigid.inlier_rmse
                res.rigid_photometric_count, res.rigid_photometric_rmse = rigid.photometric_count, rigid.photometric_rmse
            if res.canonical_triangle_count > 0:
                landmarks = self.landmark_provider(self, frame, canonical, points) if self.landmark_provider is not None else None
                if landmarks is not None and len(landmarks[0]) == 0:
                    landmarks = None
                if self.feature_tracker is not None:
                    res.tracked_feature_count = self.feature_tracker.feature_count
                self.optimizer.optimize_graph(self.active_graph, canonical, points, extrinsics=self.extrinsics, landmarks=landmarks)
                res.tracked = True
                if landmarks is not None:
                    distances, active = self.optimizer.fitter.landmark_distances()
                    res.landmark_count, res.landmark_active_count = len(active), int(active.sum())
                    if active.any():
                        res.landmark_rmse = float(np.sqrt((distances[active].astype(np.float64) ** 2).sum(axis=1).mean()))
                summary = self.optimizer.last_step_summary
                if summary is not None:
                    res.iterations_used, res.final_cost = summary["iterations_used"], summary["final_cost"]
                    res.rejected_step_count = summary["rejected_step_count"]
                if p.model_agreement:
                    agreement, _ = self.measure_model_agreement(depth)
                    res.model_overlap_count, res.model_only_count, res.frame_only_count = agreement.both, agreement.model_only, agreement.frame_only
                    res.model_depth_mean_abs, res.model_depth_rmse = agreement.mean_abs, agreement.rmse
                    res.model_inlier_ratio = agreement.inlier_ratio
                if p.motion_images:
                    self.last_motion, _ = self.render_model_motion(graph_before, extrinsics_before)
                    self._score_motion(frame, res)
            # fuse: blocks the warped surface's truncation band touches, then non-rigid integration (:371-417)
            blocks = self.volume.find_blocks_intersecting_truncation_region(depth, self.active_graph, self.K, self.extrinsics,
                                                                            p.depth_scale, depth_max, self.truncation_voxel_multiplier)
            self.volume.activate(blocks)
            normals = G.compute_ordered_point_cloud_normals(points.reshape(-1, 3), (depth_np.shape[0], depth_np.shape[1]))
            self.volume.integrate_non_rigid(blocks, self.active_graph, depth, color, normals, self.K, self.K, self.extrinsics,
                                            p.depth_scale, depth_max, self.truncation_voxel_multiplier)
            res.new_block_count = int(blocks.shape[0])
        # canonical + warped mesh of the volume as fused so far (pipeline.py:419-420; the reference skips the first frame)
        self.canonical_mesh = self.extract_canonical_mesh()
        if p.warp_field_extension and res.tracked and self.canonical_mesh.triangle_indices.shape[0]:
            res.new_node_count = self._extend_graph()
        res.node_count = self.active_graph.node_count
        self.warped_mesh = self.active_graph.warp_mesh(self.canonical_mesh) if self.canonical_mesh.triangle_indices.shape[0] else None
        res.active_block_count = self.volume.get_block_count()
        res.extrinsics = np.array(self.extrinsics, np.float64)
        torch.cuda.synchronize(self.device)
        res.seconds = time.perf_counter() - t0
        self.results.append(res)
        return res

    def run(self) -> List[FrameResult]:
        while self.sequence.has_more_frames():
            self.process_frame(self.sequence.get_next_frame())
        return self.results
