"""nnrt.alignment: DeformableMeshToImageFitter (cpp/alignment/DeformableMeshToImageFitter.h:34-91) and IterationMode
(cpp/alignment/IterationMode.h:24-28) -- absent from the reference's bindings, added here as SURVEY 8(b) specifies."""
from __future__ import annotations

import ctypes
import dataclasses
import enum

import numpy as np
import torch

from .. import _native as N
from ._tensors import to_device, to_host_f64
from .geometry import HierarchicalGraphWarpField, TriangleMesh
from .rigid_alignment import (DEGENERATE, HybridRigidAlignmentResult, RigidAlignmentResult, align_rigid_hybrid,  # noqa: F401
                              align_rigid_point_to_plane)

# nnrt_fitter_iterate_timed stage order (include/nnrt_mi355x.h, NNRT_TIMED_STAGES)
TIMED_STAGES = ("warp", "raster", "pixel_jacobians", "node_reduce", "arap", "solve")
# nnrt_fitter_time_kernels order (include/nnrt_mi355x.h, NNRT_KERNEL_TIMES)
KERNEL_TIMES = ("k_warp_mesh_quad", "k_raster_scatter_mesh", "k_fit_pixels_fused", "solve", "iteration")


class IterationMode(enum.IntEnum):
    ALL = 0
    TRANSLATION_ONLY = 1
    ROTATION_ONLY = 2


class PenaltyForm(enum.IntEnum):
    """The form the Tukey (data term) and Huber (ARAP term) penalties take where the fitter's parameters enable them
    (include/nnrt_mi355x.h NNRT_PENALTY_*): the reference's branches as written, or iteratively
    re-weighted least squares."""
    REFERENCE = 0
    IRLS = 1


class DataCoupling(enum.IntEnum):
    """How the data term couples the nodes (include/nnrt_mi355x.h NNRT_DATA_*): the reference's block-diagonal Hessian
    (SURVEY A17), or the full Gauss-Newton system with an off-diagonal block for every pair of nodes that share a face
    (DESIGN section 23). Real sequences should use COUPLED: the block-diagonal step diverges after its first iteration."""
    BLOCK_DIAGONAL = 0
    COUPLED = 1


class StepDecision(enum.IntEnum):
    """What one iteration under step control decided (include/nnrt_mi355x.h NNRT_STEP_*)."""
    HOLD = 0            # the fit was done already: the frozen state is re-evaluated
    START = 1           # first iteration, or the one after a reject: the state becomes the best state, then a step
    ACCEPT = 2          # the cost fell: new best state, lambda shrinks, step
    CONVERGED = 3       # the cost fell by no more than the relative tolerance: new best state, done
    REJECT = 4          # the cost rose (or is not finite): best state put back, lambda grows
    REJECT_FINAL = 5    # a reject with lambda already at lambda_max: done
    SMALL_UPDATE = 6    # a step whose max |update| is below minimal_update_threshold: best state put back, done


class StepObjective(enum.IntEnum):
    """The cost step control compares (include/nnrt_mi355x.h NNRT_STEP_OBJECTIVE_*). SQUARE (default):
    the sum of squared residuals, which limits step control to SQUARE penalties. ROBUST: the objective PenaltyForm.IRLS
    minimises (Tukey's biweight over the raw pixel residuals, Huber over the edges), so that step control and IRLS run
    together; one more pass over the pixels per iteration. Real sequences should use ROBUST with IRLS."""
    SQUARE = 0
    ROBUST = 1


STEP_DONE_DECISIONS = (StepDecision.CONVERGED, StepDecision.REJECT_FINAL, StepDecision.SMALL_UPDATE)


@dataclasses.dataclass(frozen=True)
class StepControl:
    """Settings of the fitter's on-device step control (nnrt_step_control): keep a Gauss-Newton step
    only if the cost fell, damp harder if not, stop when nothing moves. IterationMode.ALL only; SQUARE penalties only
    under StepObjective.SQUARE (the default), PenaltyForm.IRLS too under StepObjective.ROBUST.
    initial_lambda 0 starts from preconditioning_dampening_factor. poll_interval k > 0: fit_to_image synchronises every k
    iterations and returns once the device reports done; 0: never synchronises."""
    initial_lambda: float = 0.0
    increase: float = 10.0
    decrease: float = 0.5
    lambda_min: float = 1e-6
    lambda_max: float = 1.0
    relative_cost_tolerance: float = 1e-4
    poll_interval: int = 0


@dataclasses.dataclass(frozen=True)
class StepRecord:
    """One iteration of a fit under step control: the cost of the state it started from, the damping its solve used, its
    decision and (stepping iterations) the largest absolute update."""
    iteration: int
    cost: float
    lambda_used: float
    decision: StepDecision
    max_update: float


def summarize_step_history(history) -> dict:
    """iterations_used, final_cost, rejected_step_count and done of a list of StepRecords (zeros for an empty one)."""
    used, done, final_cost, rejected = len(history), False, 0.0, 0
    for i, r in enumerate(history):
        if r.decision in (StepDecision.START, StepDecision.ACCEPT, StepDecision.CONVERGED):
            final_cost = r.cost   # the best state's cost
        if r.decision in (StepDecision.REJECT, StepDecision.REJECT_FINAL):
            rejected += 1
        if not done and (r.decision in STEP_DONE_DECISIONS or r.decision == StepDecision.HOLD):
            used, done = (i + 1 if r.decision != StepDecision.HOLD else i), True
    return dict(iterations_used=used, final_cost=float(final_cost), rejected_step_count=rejected, done=done)


def landmarks_from_pixel_matches(pixel_face_indices, pixel_barycentric_coordinates, triangle_indices, source_uv, target_uv, target_point_image,
                                 weights=None):
    """2-D matches -> the (vertex_indices, targets, weights | None) tuple DeformableMeshToImageFitter.set_landmarks and
    RenderingAlignmentOptimizer.optimize_graph(landmarks=...) take: the bridge from optical flow or keypoint matches.

    pixel_face_indices [H, W] (or [H, W, 1]; < 0: background) and pixel_barycentric_coordinates [H, W, 3] (or
    [H, W, 1, 3]) are a render of the warped model, triangle_indices [F, 3] its faces; source_uv / target_uv [M, 2] integer
    pixel coordinates (u = column, v = row) in that render and in the live frame, target_point_image [H', W', 3] the live
    frame's camera-space points. Each match takes, from its source pixel, the face vertex with the largest barycentric
    weight as the vertex, and the target pixel's point as the target. A match whose source pixel is background (or off the
    render), or whose target point is off the image, non-finite or has z <= 0, is dropped. Torch only; the results stay on
    the inputs' device."""
    faces = torch.as_tensor(pixel_face_indices)
    dev = faces.device
    faces = faces.reshape(faces.shape[0], faces.shape[1], -1)[..., 0].to(torch.int64)
    H, W = faces.shape
    bary = torch.as_tensor(pixel_barycentric_coordinates).to(dev).reshape(H, W, -1)[..., :3]
    tri = torch.as_tensor(triangle_indices).to(dev).to(torch.int64).reshape(-1, 3)
    src = torch.as_tensor(source_uv).to(dev).to(torch.int64).reshape(-1, 2)
    tgt = torch.as_tensor(target_uv).to(dev).to(torch.int64).reshape(-1, 2)
    points = torch.as_tensor(target_point_image).to(dev).to(torch.float32)
    Ht, Wt = points.shape[0], points.shape[1]
    points = points.reshape(Ht, Wt, 3)
    if src.shape[0] != tgt.shape[0]:
        raise ValueError(f"{src.shape[0]} source pixels but {tgt.shape[0]} target pixels")
    w = None
    if weights is not None:
        w = torch.as_tensor(weights).to(dev).to(torch.float32).reshape(-1)
        if w.shape[0] != src.shape[0]:
            raise ValueError(f"{src.shape[0]} matches but {w.shape[0]} weights")
    inside = (src[:, 0] >= 0) & (src[:, 0] < W) & (src[:, 1] >= 0) & (src[:, 1] < H) & (tgt[:, 0] >= 0) & (tgt[:, 0] < Wt) & (tgt[:, 1] >= 0) & \
             (tgt[:, 1] < Ht)
    su, sv = src[:, 0].clamp(0, W - 1), src[:, 1].clamp(0, H - 1)
    tu, tv = tgt[:, 0].clamp(0, Wt - 1), tgt[:, 1].clamp(0, Ht - 1)
    face = faces[sv, su]
    q = points[tv, tu]
    keep = inside & (face >= 0) & (face < tri.shape[0]) & torch.isfinite(q).all(dim=1) & (q[:, 2] > 0)
    corner = bary[sv, su].argmax(dim=1)
    vertex = tri[face.clamp(0, max(tri.shape[0] - 1, 0)), corner]
    return vertex[keep].to(torch.int32), q[keep].contiguous(), (None if w is None else w[keep])


@dataclasses.dataclass(frozen=True)
class FeatureTracking:
    """Parameters of the sparse feature tracker that feeds the landmark term from the colour frames (FeatureTrackLandmarks,
    FusionParameters.landmark_tracking). Selection: at most max_features Shi-Tomasi corners (window
    radius window_radius) with a score of at least quality times the best, no two within nms_radius pixels. Tracking:
    pyramidal Lucas-Kanade over `levels` levels with the same window radius, max_iterations per level (epsilon > 0 stops a
    level once a step is shorter, in pixels), levels and features flatter than min_eigen_threshold dropped, features
    whose mean absolute intensity difference at the result exceeds max_residual dropped (<= 0: kept), and a round trip
    that must close within forward_backward_threshold pixels (None: no backward pass). weight: the weight every landmark
    carries into the fit. The defaults are conventional values for 8-bit images scaled to [0, 1]; none of them has been
    tuned on any real sequence."""
    max_features: int = 512
    quality: float = 0.01
    nms_radius: int = 5
    window_radius: int = 7
    levels: int = 3
    max_iterations: int = 10
    epsilon: float = 0.01
    min_eigen_threshold: float = 1e-6
    max_residual: float = 0.05
    forward_backward_threshold: float | None = 0.5
    weight: float = 1.0


class FeatureTrackLandmarks:
    """The built-in landmark provider (FusionPipeline(landmark_provider=...) signature): landmarks from features tracked
    between the previous colour frame and the current one.

    advance(color, extrinsics) takes every frame's uint8 [H, W, 3] colour image, the first included, with the world -> camera
    matrix the previous frame was tracked with; it keeps the previous frame's intensity pyramid and builds the current
    one. Called for a tracked frame, the provider rasterizes the canonical mesh, warped by the graph's current state (the
    previous frame's fit), at those extrinsics with one face per pixel; selects features in the previous intensity under
    the mask "pixel has a face"; tracks them into the current frame; rounds the tracked positions to the nearest pixel;
    and returns landmarks_from_pixel_matches(...) with `weight` on every landmark. The rounding moves a target by up to
    half a pixel's footprint on the surface (z / fx); a sub-pixel lookup of the target point is not done.
    feature_count: the features selected by the last call."""

    def __init__(self, parameters: FeatureTracking | None = None):
        self.parameters = parameters or FeatureTracking()
        self.previous_pyramid = None
        self.current_pyramid = None
        self.previous_extrinsics = None
        self.feature_count = 0

    def advance(self, color, extrinsics=None):
        from .image_proc import intensity_from_rgb8, intensity_pyramid
        self.previous_pyramid = self.current_pyramid
        self.current_pyramid = intensity_pyramid(intensity_from_rgb8(color), self.parameters.levels)
        self.previous_extrinsics = np.eye(4) if extrinsics is None else np.array(extrinsics, np.float64)

    def __call__(self, pipeline, frame, canonical, point_image):
        from . import rendering
        from .image_proc import FEATURE_TRACKED, corner_scores, select_features, track_features
        p = self.parameters
        self.feature_count = 0
        if self.previous_pyramid is None or self.current_pyramid is None:
            return None
        previous = self.previous_pyramid[0]
        H, W = int(previous.shape[0]), int(previous.shape[1])
        warped = pipeline.active_graph.warp_mesh(canonical, extrinsics=self.previous_extrinsics)
        (faces, _, bary, _), _ = rendering.rasterize_meshes(warped, pipeline.K, (H, W), faces_per_pixel=1, ndc_convention=NDC_CONSISTENT)
        faces = faces.reshape(H, W)
        source = select_features(corner_scores(previous, p.window_radius), p.max_features, p.quality, p.nms_radius, mask=faces >= 0)
        self.feature_count = int(source.shape[0])
        if self.feature_count == 0:
            return None
        target, status, _ = track_features(self.previous_pyramid, self.current_pyramid, source, p.window_radius, p.max_iterations, p.epsilon,
                                           p.min_eigen_threshold, p.max_residual, p.forward_backward_threshold)
        kept = status == FEATURE_TRACKED
        source_uv = source[kept].to(torch.int64)
        target_uv = torch.floor(target[kept] + 0.5).to(torch.int64)
        weights = torch.full((int(source_uv.shape[0]),), float(p.weight), dtype=torch.float32, device=source.device)
        return landmarks_from_pixel_matches(faces, bary, canonical.triangle_indices, source_uv, target_uv, point_image, weights)


NDC_REFERENCE = 0     # the reference's image -> NDC mapping
NDC_CONSISTENT = 1    # raster pixel (u, v) == pixel (u, v) of the intrinsics

# use_hip_graph (include/nnrt_mi355x.h NNRT_GRAPH_*): False/0 eager launches; True/1 a sequence of iterations runs eagerly
# the first time it is requested after prepare() and is graph-captured and replayed from its second request on (the
# default: a one-off frame fit never pays capture + instantiate); 2 captures on first use
GRAPH_NEVER, GRAPH_AUTO, GRAPH_ALWAYS = 0, 1, 2


class DeformableMeshToImageFitter:
    def __init__(self, max_iteration_count: int = 100, iteration_mode_sequence=(IterationMode.ALL,), minimal_update_threshold: float = 1e-6,
                 use_perspective_correction: bool = True, max_depth: float = 10.0, use_tukey_penalty_for_data_term: bool = False,
                 tukey_penalty_cutoff_cm: float = 0.01, preconditioning_dampening_factor: float = 0.0, arap_term_weight: float = 200.0,
                 use_huber_penalty_for_arap_term: bool = False, huber_penalty_constant: float = 1e-4, device: int | None = None,
                 use_hip_graph: int = 1, ndc_convention: int = 0, step_objective: StepObjective = StepObjective.SQUARE,
                 penalty_form: PenaltyForm = PenaltyForm.REFERENCE, guard_zero_rotation: bool = False):
        device = N.current_device() if device is None else int(device)
        p = N.FitterParams()
        N.lib().nnrt_fitter_default_params(ctypes.byref(p))
        modes = list(iteration_mode_sequence)
        p.max_iteration_count = int(max_iteration_count)
        p.iteration_mode_count = len(modes)
        for i, m in enumerate(modes):
            p.iteration_modes[i] = int(m)
        p.minimal_update_threshold = float(minimal_update_threshold)
        p.use_perspective_correction = int(use_perspective_correction)
        p.max_depth = float(max_depth)
        p.use_tukey_penalty_for_data_term = int(use_tukey_penalty_for_data_term)
        p.tukey_penalty_cutoff_cm = float(tukey_penalty_cutoff_cm)
        p.preconditioning_dampening_factor = float(preconditioning_dampening_factor)
        p.arap_term_weight = float(arap_term_weight)
        p.use_huber_penalty_for_arap_term = int(use_huber_penalty_for_arap_term)
        p.huber_penalty_constant = float(huber_penalty_constant)
        p.use_hip_graph = int(use_hip_graph)
        p.ndc_convention = int(ndc_convention)   # NDC_REFERENCE (A11, y-mirrored renders) or NDC_CONSISTENT (real depth frames)
        h = ctypes.c_void_p()
        N.check(N.lib().nnrt_fitter_create(ctypes.byref(p), int(device), ctypes.byref(h)))
        self._h = h
        self.params = p
        self.device = torch.device("cuda", device)
        self.modes = modes
        self._frame = None
        self.set_robust_options(penalty_form, guard_zero_rotation)
        self.set_step_objective(step_objective)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                N.lib().nnrt_fitter_destroy(h)
            except Exception:   # interpreter shutdown
                pass
            self._h = None

    # ---- split API (once-per-frame prepare + GN iterations) ----
    def prepare(self, warp_field: HierarchicalGraphWarpField, canonical_mesh: TriangleMesh, reference_depth_image,
                reference_image_mask, intrinsic_matrix, extrinsic_matrix=None, depth_scale: float = 1.0, stream=None):
        N.require_gpu()
        dev = self.device
        p, n, f = canonical_mesh.on_device(dev)
        d = to_device(reference_depth_image, torch.float32, dev)
        if d.dim() == 3:
            d = d[..., 0].contiguous()
        H, W = d.shape
        m = None if reference_image_mask is None else to_device(reference_image_mask, torch.uint8, dev).reshape(H, W)
        K = to_host_f64(intrinsic_matrix)
        E = None if extrinsic_matrix is None else to_host_f64(extrinsic_matrix)
        self._frame = (p, n, f, d, m, K, E, H, W)   # keep device inputs alive for the duration of the frame
        self._node_count = warp_field.node_count
        N.check(N.lib().nnrt_fitter_prepare(self._h, warp_field.handle, N.ptr(p), N.ptr(n), p.shape[0], N.ptr(f), f.shape[0], N.ptr(d), N.ptr(m),
                                            H, W, N.ptr(K), N.ptr(E), float(depth_scale), N.stream_ptr(stream)))

    def prepare_point_cloud(self, warp_field: HierarchicalGraphWarpField, canonical_mesh: TriangleMesh, reference_point_cloud,
                            reference_point_mask, intrinsic_matrix, extrinsic_matrix, rendering_image_size, stream=None):
        """Once-per-frame setup of the point-cloud overload (DeformableMeshToImageFitter.cpp:85-106): organized reference
        points [H*W,3] (or [H,W,3]) and their mask, rendered at rendering_image_size = (H, W)."""
        N.require_gpu()
        dev = self.device
        p, n, f = canonical_mesh.on_device(dev)
        H, W = int(rendering_image_size[0]), int(rendering_image_size[1])
        q = to_device(reference_point_cloud, torch.float32, dev).reshape(-1, 3).contiguous()
        if q.shape[0] != H * W:
            raise ValueError(f"reference point cloud has {q.shape[0]} points, expected an organized cloud of {H}x{W}")
        m = None if reference_point_mask is None else to_device(reference_point_mask, torch.uint8, dev).reshape(-1).contiguous()
        K = to_host_f64(intrinsic_matrix)
        E = None if extrinsic_matrix is None else to_host_f64(extrinsic_matrix)
        self._frame = (p, n, f, q, m, K, E, H, W)
        self._node_count = warp_field.node_count
        N.check(N.lib().nnrt_fitter_prepare_point_cloud(self._h, warp_field.handle, N.ptr(p), N.ptr(n), p.shape[0], N.ptr(f), f.shape[0],
                                                        N.ptr(q), N.ptr(m), H, W, N.ptr(K), N.ptr(E), N.stream_ptr(stream)))

    def iterate(self, warp_field: HierarchicalGraphWarpField, first_iteration: int = 0, count: int = 1, stream=None):
        N.check(N.lib().nnrt_fitter_iterate(self._h, warp_field.handle, int(first_iteration), int(count), N.stream_ptr(stream)))

    def iterate_from_identity(self, warp_field: HierarchicalGraphWarpField, first_iteration: int = 0, count: int = 1, stream=None):
        """iterate() with the warp field's motion reset to the identity before every iteration (benchmark form: each
        iteration is the first GN iteration of the prepared frame); graph-captured like iterate()."""
        N.check(N.lib().nnrt_fitter_iterate_from_identity(self._h, warp_field.handle, int(first_iteration), int(count),
                                                           N.stream_ptr(stream)))

    def snapshot_motion(self, warp_field: HierarchicalGraphWarpField, stream=None):
        """Store the warp field's node motion (R, t) in the fitter (device copy) for iterate_from_snapshot()."""
        N.check(N.lib().nnrt_fitter_snapshot_motion(self._h, warp_field.handle, N.stream_ptr(stream)))

    def iterate_from_snapshot(self, warp_field: HierarchicalGraphWarpField, first_iteration: int = 0, count: int = 1, stream=None):
        """iterate() with the node motion restored from the snapshot before every iteration (a device copy captured
        with the iteration): each iteration is the same GN iteration k of the frame, through the general kernels."""
        N.check(N.lib().nnrt_fitter_iterate_from_snapshot(self._h, warp_field.handle, int(first_iteration), int(count),
                                                           N.stream_ptr(stream)))

    def fit_from_snapshot(self, warp_field: HierarchicalGraphWarpField, count: int, stream=None):
        """A whole frame fit of `count` iterations from the snapshot (restored once, before the first iteration)."""
        N.check(N.lib().nnrt_fitter_fit_from_snapshot(self._h, warp_field.handle, int(count), N.stream_ptr(stream)))

    def restore_motion(self, warp_field: HierarchicalGraphWarpField, stream=None):
        N.check(N.lib().nnrt_fitter_restore_motion(self._h, warp_field.handle, N.stream_ptr(stream)))

    def iterate_timed(self, warp_field: HierarchicalGraphWarpField, first_iteration: int = 0, count: int = 1, stream=None) -> dict:
        """Eager iterations with HIP events between stages; returns average device ms per iteration per stage."""
        ms = np.zeros(len(TIMED_STAGES), np.float32)
        N.check(N.lib().nnrt_fitter_iterate_timed(self._h, warp_field.handle, int(first_iteration), int(count), N.ptr(ms), N.stream_ptr(stream)))
        return {name: float(v) for name, v in zip(TIMED_STAGES, ms)}

    def refine_info(self, stream=None) -> dict:
        """The last arrowhead solve's refinement gate: the corner factorization's smallest pivot / diag(S) ratio, the
        threshold, whether the refinement step ran, its max |d| / max |x| and whether its safeguard accepted it."""
        out = np.zeros(5, np.float32)
        N.check(N.lib().nnrt_fitter_refine_info(self._h, N.ptr(out), N.stream_ptr(stream)))
        return dict(pivot_ratio=float(out[0]), threshold=float(out[1]), refined=bool(out[2]), correction=float(out[3]),
                    accepted=bool(out[4]))

    def set_refine_ratio(self, ratio: float):
        """Upper end of the arrowhead solve's refinement window: one refinement step runs when the corner
        factorization's min pivot / diag(S) lies in [floor, ratio) (floor 1e-5, _native.refine_floor(); default ratio
        1e-2; 0: never refine; inf: refine whenever the ratio is at least the floor). refine_info() reports
        the threshold the last launched iterations ran with."""
        N.check(N.lib().nnrt_fitter_set_refine_ratio(self._h, float(ratio)))

    def set_robust_options(self, penalty_form, guard_zero_rotation):
        """penalty_form: PenaltyForm.REFERENCE (default) keeps the reference's Tukey / Huber branches; PenaltyForm.IRLS
        re-weights instead. Data term (use_tukey_penalty_for_data_term): a masked-in pixel with residual r contributes
        iff |r| <= c; s = 1 - (r / c)^2, residual s r, Jacobian row s J. ARAP term (use_huber_penalty_for_arap_term):
        the edge's residual 3-vector and Jacobian terms times s = 1 if |r| <= delta else sqrt(delta / |r|). No effect on
        a square term. guard_zero_rotation: a node whose rotation update is exactly zero keeps its rotation instead of
        getting Rodrigues' NaN. Drops the cached graphs, keeps the prepared frame; other values raise."""
        if isinstance(guard_zero_rotation, (bool, np.bool_)):
            guard_zero_rotation = int(guard_zero_rotation)
        N.check(N.lib().nnrt_fitter_set_robust_options(self._h, int(penalty_form), int(guard_zero_rotation)))

    @property
    def robust_options(self):
        """(PenaltyForm, guard_zero_rotation) as the fitter holds them."""
        form, guard = ctypes.c_int32(), ctypes.c_int32()
        N.check(N.lib().nnrt_fitter_get_robust_options(self._h, ctypes.byref(form), ctypes.byref(guard)))
        return PenaltyForm(form.value), bool(guard.value)

    def set_data_coupling(self, data_coupling):
        """DataCoupling.BLOCK_DIAGONAL (default: the reference's arithmetic) or DataCoupling.COUPLED (the data term's
        off-diagonal blocks and one sparse solve of the whole system; IterationMode.ALL only). A change drops the cached
        graphs and invalidates the prepared frame: call prepare() again. Other values, or COUPLED on a fitter whose mode
        list holds another mode, raise."""
        N.check(N.lib().nnrt_fitter_set_data_coupling(self._h, int(data_coupling)))

    @property
    def data_coupling(self) -> DataCoupling:
        v = ctypes.c_int32()
        N.check(N.lib().nnrt_fitter_get_data_coupling(self._h, ctypes.byref(v)))
        return DataCoupling(v.value)

    @property
    def coupled_pair_count(self) -> int:
        """Node pairs of the prepared frame's coupled system (0 in block-diagonal mode)."""
        return int(N.lib().nnrt_fitter_coupled_pair_count(self._h))

    def coupled_system(self, stream=None):
        """The last coupled iteration's float system as the fitter solved it (virtual order): diagonal blocks [N,6,6]
        with LM, pairs [M,2] (i < j, ascending), block (i, j) of each pair [M,6,6], right-hand side [6N]."""
        n, m = self._node_count, self.coupled_pair_count
        d = np.empty((n, 6, 6), np.float32)
        pairs = np.empty((m, 2), np.int32)
        blocks = np.empty((m, 6, 6), np.float32)
        b = np.empty(6 * n, np.float32)
        N.check(N.lib().nnrt_fitter_get_coupled_system(self._h, N.ptr(d), N.ptr(pairs), N.ptr(blocks), N.ptr(b), n, m, N.stream_ptr(stream)))
        return d, pairs, blocks, b

    def set_step_control(self, step_control: StepControl | None):
        """Turn the on-device step control on with these settings, or off with None (the default: every output as
        without it). A change drops the cached graphs and invalidates the prepared frame: call prepare() again.
        Out-of-range settings, PenaltyForm.IRLS under StepObjective.SQUARE, or a mode list holding another mode than ALL
        raise."""
        if step_control is None:
            N.check(N.lib().nnrt_fitter_set_step_control(self._h, None))
            return
        c = step_control
        s = N.StepControlSettings(float(c.initial_lambda), float(c.increase), float(c.decrease), float(c.lambda_min), float(c.lambda_max),
                                  float(c.relative_cost_tolerance), int(c.poll_interval))
        N.check(N.lib().nnrt_fitter_set_step_control(self._h, ctypes.byref(s)))

    @property
    def step_control(self) -> StepControl | None:
        on, s = ctypes.c_int32(), N.StepControlSettings()
        N.check(N.lib().nnrt_fitter_get_step_control(self._h, ctypes.byref(on), ctypes.byref(s)))
        if not on.value:
            return None
        return StepControl(s.initial_lambda, s.increase, s.decrease, s.lambda_min, s.lambda_max, s.relative_cost_tolerance, s.poll_interval)

    def set_step_objective(self, step_objective):
        """StepObjective.SQUARE (default) or StepObjective.ROBUST: the cost step control compares. Under ROBUST,
        PenaltyForm.IRLS and step control are accepted together, in either order. ROBUST with PenaltyForm.REFERENCE and a
        penalty enabled raises, and so does SQUARE while step control is on with PenaltyForm.IRLS. A change drops the
        cached graphs and, with step control on, invalidates the prepared frame: call prepare() again."""
        N.check(N.lib().nnrt_fitter_set_step_objective(self._h, int(step_objective)))

    @property
    def step_objective(self) -> StepObjective:
        v = ctypes.c_int32()
        N.check(N.lib().nnrt_fitter_get_step_objective(self._h, ctypes.byref(v)))
        return StepObjective(v.value)

    def raw_residuals(self, stream=None) -> np.ndarray:
        """[H * W] float32: the raw point-to-plane residual r of every pixel as the last iteration's cost launch resolved
        it (0 outside the residual mask), before the IRLS scaling diagnostics()['residuals'] carries. Step control on
        under StepObjective.ROBUST only. Synchronizes."""
        _, _, _, _, _, _, _, H, W = self._frame
        out = np.empty(H * W, np.float32)
        N.check(N.lib().nnrt_fitter_get_raw_residuals(self._h, N.ptr(out), H * W, N.stream_ptr(stream)))
        return out

    def set_landmarks(self, vertex_indices, target_points, weights=None, term_weight: float = 1.0, cutoff: float = 0.0, stream=None):
        """Sparse 3-D correspondences for the next fit (nnrt_fitter_set_landmarks): landmark l pulls
        canonical vertex vertex_indices[l] towards the camera-space point target_points[l] with residual
        term_weight * weights[l] * (warped vertex - target). weights None: all 1; cutoff > 0 (metres) drops a landmark
        farther from its target than that. An empty set clears the landmarks. IterationMode.ALL only. Takes effect at
        the next prepare() (fit_to_image), which raises for an index outside the mesh or a vertex without a face;
        invalidates the prepared frame. The same count and settings keep the captured graphs. term_weight = 1 is untuned."""
        idx = to_device(vertex_indices, torch.int32, self.device).reshape(-1).contiguous()
        tgt = to_device(target_points, torch.float32, self.device).reshape(-1, 3).contiguous()
        if tgt.shape[0] != idx.shape[0]:
            raise ValueError(f"{idx.shape[0]} vertex indices but {tgt.shape[0]} target points")
        w = None
        if weights is not None:
            w = to_device(weights, torch.float32, self.device).reshape(-1).contiguous()
            if w.shape[0] != idx.shape[0]:
                raise ValueError(f"{idx.shape[0]} vertex indices but {w.shape[0]} weights")
        N.check(N.lib().nnrt_fitter_set_landmarks(self._h, N.ptr(idx), N.ptr(tgt), N.ptr(w), idx.shape[0], float(term_weight), float(cutoff),
                                                  N.stream_ptr(stream)))

    def clear_landmarks(self, stream=None):
        """Back to a fitter without landmarks: every launch and output as if none had ever been set."""
        N.check(N.lib().nnrt_fitter_set_landmarks(self._h, None, None, None, 0, 1.0, 0.0, N.stream_ptr(stream)))

    def landmark_distances(self, stream=None):
        """([L, 3] float32 warped vertex - target, [L] bool active) of every landmark as of the state the last iteration
        started from (zeros before the first). Synchronizes."""
        L = self.landmark_info()["count"]
        out = np.zeros((L, 4), np.float32)
        N.check(N.lib().nnrt_fitter_get_landmark_distances(self._h, N.ptr(out), L, N.stream_ptr(stream)))
        return out[:, :3].copy(), out[:, 3] != 0

    def landmark_info(self) -> dict:
        """Landmarks set and, of the prepared frame, their node associations, node runs and pair associations."""
        out = np.zeros(4, np.int64)
        N.check(N.lib().nnrt_fitter_landmark_info(self._h, N.ptr(out), out.size))
        return {k: int(v) for k, v in zip(("count", "associations", "node_runs", "pair_associations"), out)}

    def step_history(self, stream=None) -> list:
        """The StepRecords of the iterations since the fit started (iterate() from iteration 0), oldest first: at most
        the last 256. Empty with step control off. Synchronizes."""
        buf = (N.StepRecord * N.STEP_HISTORY_CAPACITY)()
        n = ctypes.c_int64()
        N.check(N.lib().nnrt_fitter_get_step_history(self._h, buf, N.STEP_HISTORY_CAPACITY, ctypes.byref(n), N.stream_ptr(stream)))
        return [StepRecord(r.iteration, r.cost, r.lambda_, StepDecision(r.decision), r.max_update) for r in buf[: n.value]]

    def step_summary(self, stream=None) -> dict:
        """From step_history(): iterations_used (up to and including the one that set done; all of them otherwise),
        final_cost (the best state's, which the fit ends on), rejected_step_count and done. Zeros with step control off."""
        return summarize_step_history(self.step_history(stream))

    @property
    def graph_count(self) -> int:
        """Instantiated iteration-sequence graphs the fitter holds."""
        return int(N.lib().nnrt_fitter_graph_count(self._h))

    def set_anchor_graph(self, edges, stream=None):
        """Anchor the canonical mesh along a motion graph's edges (the reference's AnchorComputationMethod.SHORTEST_PATH):
        `edges` [N, D] int32 rows in the warp field's virtual node order (entry < 0 = empty), N the node count of the warp
        field later handed to prepare(); None returns to Euclidean anchors. Takes effect at the next prepare()."""
        if edges is None:
            N.check(N.lib().nnrt_fitter_set_anchor_graph(self._h, None, 0, 0, N.stream_ptr(stream)))
            return
        dtype = edges.dtype if isinstance(edges, torch.Tensor) else np.asarray(edges).dtype
        if dtype not in (torch.int32, np.dtype(np.int32)) or len(edges.shape) != 2:
            raise RuntimeError(f"`edges` needs to be an int32 tensor of shape [node count, graph degree]. Got {dtype} {tuple(edges.shape)}.")
        e = to_device(edges, torch.int32, self.device)
        N.check(N.lib().nnrt_fitter_set_anchor_graph(self._h, N.ptr(e), e.shape[0], e.shape[1], N.stream_ptr(stream)))

    def time_kernels(self,warp_field: HierarchicalGraphWarpField, reps: int = 20, trials: int = 5, stream=None) -> dict:
        """Per-kernel device ms of one iteration from the snapshot state, each kernel in its real context (prefix
        sequences of `reps` graph-captured iterations, median of `trials`; include/nnrt_mi355x.h)."""
        ms = np.zeros(len(KERNEL_TIMES), np.float32)
        N.check(N.lib().nnrt_fitter_time_kernels(self._h, warp_field.handle, int(reps), int(trials), N.ptr(ms), N.stream_ptr(stream)))
        return {name: float(v) for name, v in zip(KERNEL_TIMES, ms)}

    def check(self, stream=None):
        N.check(N.lib().nnrt_fitter_check(self._h, N.stream_ptr(stream)))

    def fit_to_image(self, warp_field: HierarchicalGraphWarpField, canonical_mesh: TriangleMesh, *args):
        """The three FitToImage overloads (DeformableMeshToImageFitter.h:58-90); all mutate the warp field in place:

        * (warp_field, mesh, rgbd_image, reference_image_mask, K, E, depth_scale) -- rgbd_image has .color / .depth
          (DeformableMeshToImageFitter.cpp:316-329);
        * (warp_field, mesh, color, depth, reference_image_mask, K, E, depth_scale) (:278-314);
        * (warp_field, mesh, color, reference_point_cloud, reference_point_mask, K, E, rendering_image_size) (:85-276).

        The colour image is unused, as in the reference. A14: all max_iteration_count iterations run."""
        if len(args) == 5 and hasattr(args[0], "depth"):
            rgbd, mask, K, E, scale = args
            self.prepare(warp_field, canonical_mesh, rgbd.depth, mask, K, E, scale)
        elif len(args) == 6 and isinstance(args[5], (tuple, list, torch.Size)):
            _color, points, mask, K, E, size = args
            self.prepare_point_cloud(warp_field, canonical_mesh, points, mask, K, E, size)
        elif len(args) in (5, 6):
            _color, depth, mask, K = args[:4]
            E = args[4] if len(args) > 4 else None
            scale = args[5] if len(args) > 5 else 1.0
            self.prepare(warp_field, canonical_mesh, depth, mask, K, E, scale)
        else:
            raise TypeError("fit_to_image: no overload matches the arguments (see DeformableMeshToImageFitter.h:58-90)")
        total = self.params.max_iteration_count
        control = self.step_control
        k = control.poll_interval if control is not None else 0
        if k <= 0:
            self.iterate(warp_field, 0, total)
        else:   # step control's host early exit: k iterations at a time until the device reports done
            for first in range(0, total, k):
                self.iterate(warp_field, first, min(k, total - first))
                if self.step_summary()["done"]:
                    break
        self.check()

    def diagnostics(self, stream=None) -> dict:
        """Residuals, residual mask, rasterized face per pixel, motion updates, negative gradient and data-term Hessian
        blocks of the most recent iteration (host numpy)."""
        _, _, _, _, _, _, _, H, W = self._frame
        P = H * W
        s = 6   # upper bound (3-dof modes fill the first N*3 / N*9 entries)
        nodes = self._node_count
        out = dict(residuals=np.empty(P, np.float32), residual_mask=np.empty(P, np.uint8), pixel_faces=np.empty(P, np.int32),
                   updates=np.empty(nodes * s, np.float32), gradient=np.empty(nodes * s, np.float32),
                   hessian=np.empty(nodes * s * s, np.float32))
        N.check(N.lib().nnrt_fitter_get_diagnostics(self._h, N.ptr(out["residuals"]), N.ptr(out["residual_mask"]), N.ptr(out["pixel_faces"]),
                                                    N.ptr(out["updates"]), N.ptr(out["gradient"]), N.ptr(out["hessian"]), N.stream_ptr(stream)))
        out["residual_mask"] = out["residual_mask"].astype(bool)
        return out

    def corner_info(self) -> dict:
        """Schur-corner plan of the prepared frame's arrowhead solve (csrc/corner.hip): corner nodes, tile columns,
        factorization / back-substitution launches, stored vs dense lower 64 x 64 tiles."""
        out = np.zeros(6, np.int64)
        N.check(N.lib().nnrt_fitter_corner_info(self._h, N.ptr(out)))
        keys = ("corner_nodes", "tile_columns", "factor_launches", "back_launches", "stored_tiles", "dense_lower_tiles")
        return {k: int(v) for k, v in zip(keys, out)}

    def launch_plan(self) -> dict:
        """Launch choices of the last prepared frame (csrc/launch_plan.hpp), 0 / 1 each: which pixel-launch order table and
        build, anchor format, warp kernel and raster kernel its iterations use."""
        out = np.zeros(6, np.int32)
        N.check(N.lib().nnrt_fitter_launch_plan(self._h, N.ptr(out), out.size))
        keys = ("tile_order", "quad_order", "pix_low_occupancy", "anchors16", "warp_vertex", "raster_dense")
        return {k: int(v) for k, v in zip(keys, out)}

    def arrowhead_system(self, node_count: int, edge_count: int, stream=None):
        """The last ARAP iteration's float arrowhead system as the fitter solved it (virtual order): diagonal blocks
        [N,6,6] with LM, wing blocks [E,6,6] (block (i, j) of edge (i, j)), right-hand side [6N]."""
        d = np.empty((node_count, 6, 6), np.float32)
        w = np.empty((edge_count, 6, 6), np.float32)
        b = np.empty(6 * node_count, np.float32)
        N.check(N.lib().nnrt_fitter_get_arrowhead_system(self._h, N.ptr(d), N.ptr(w), N.ptr(b), int(node_count), int(edge_count),
                                                          N.stream_ptr(stream)))
        return d, w, b

    def warped_mesh(self, vertex_count: int, stream=None):
        """The last iteration's warped canonical mesh (positions, normals [V,3]) as the fitter rasterized it; vertex_count
        must equal the prepared mesh's (the C-ABI refuses a mismatch instead of writing past the buffers)."""
        p = np.empty((vertex_count, 3), np.float32)
        n = np.empty((vertex_count, 3), np.float32)
        N.check(N.lib().nnrt_fitter_get_warped_mesh(self._h, N.ptr(p), N.ptr(n), int(vertex_count), N.stream_ptr(stream)))
        return p, n

    def corner_work(self) -> dict:
        """The plan's factorization work as executed (csrc/corner.hip): MFMA flops (update-term tile products + rank-32
        products), update terms, eliminated tile columns (real columns summed)."""
        out = np.zeros(3, np.int64)
        N.check(N.lib().nnrt_fitter_corner_work(self._h, N.ptr(out)))
        return {k: int(v) for k, v in zip(("mfma_flops", "update_terms", "eliminated_columns"), out)}

    def anchors(self, vertex_count: int, anchor_count: int, stream=None):
        a = np.empty((vertex_count, anchor_count), np.int32)
        w = np.empty((vertex_count, anchor_count), np.float32)
        N.check(N.lib().nnrt_fitter_get_anchors(self._h, N.ptr(a), N.ptr(w), N.stream_ptr(stream)))
        return a, w
