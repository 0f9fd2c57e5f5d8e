"""nnrt.rendering mirror (cpp/pybind/rendering/rendering.cpp:36-43, functional/functional.cpp:36-62)."""
from __future__ import annotations

import ctypes
import math
import types
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native as N
from . import geometry as _geometry
from . import image_proc
from ._overloads import Overloaded
from ._tensors import to_device, to_host_f64


def _dev():
    return torch.device("cuda", N.current_device())


def rasterize_ndc_triangles(ndc_face_vertices, clipped_faces_mask, image_size, blur_radius_pixels=0.0, faces_per_pixel=8, bin_size=-1,
                            max_faces_per_bin=-1, perspective_correct_barycentric_coordinates=False, clip_barycentric_coordinates=False,
                            cull_back_faces=True):
    """Returns (pixel_face_indices [H,W,K] int64, depths [H,W,K], barycentrics [H,W,K,3], signed distances [H,W,K])."""
    dev = _dev()
    H, W = int(image_size[0]), int(image_size[1])
    f = to_device(ndc_face_vertices, torch.float32, dev).reshape(-1, 3, 3)
    m = None if clipped_faces_mask is None else to_device(clipped_faces_mask, torch.uint8, dev)
    K = int(faces_per_pixel)
    fi = torch.empty((H, W, K), dtype=torch.int64, device=dev)
    dep = torch.empty((H, W, K), dtype=torch.float32, device=dev)
    bary = torch.empty((H, W, K, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((H, W, K), dtype=torch.float32, device=dev)
    N.check(N.lib().nnrt_rasterize_ndc_triangles(N.ptr(f), N.ptr(m), f.shape[0], H, W, float(blur_radius_pixels), K, int(bin_size),
                                                 int(max_faces_per_bin), int(perspective_correct_barycentric_coordinates),
                                                 int(clip_barycentric_coordinates), int(cull_back_faces), N.ptr(fi), N.ptr(dep), N.ptr(bary),
                                                 N.ptr(dist), N.stream_ptr()))
    return fi, dep, bary, dist


def _check_clipping(image_size, near_clipping_distance, far_clipping_distance):
    """CheckClippingRangeAndImageSize (cpp/rendering/functional/ExtractFaceVertices.cpp:41-54)."""
    if near_clipping_distance < 0.0:
        raise RuntimeError(f"near_clipping_distance cannot be less than 0.0. Got {near_clipping_distance}.")
    if near_clipping_distance > far_clipping_distance:
        raise RuntimeError("near_clipping_distance cannot be greater than far_clipping_distance. Got "
                           f"{near_clipping_distance} and {far_clipping_distance}, respectively.")
    if len(image_size) != 2:
        raise RuntimeError(f"image_size should be a SizeVector of size 2. Got size {len(image_size)}.")


def _mesh_arrays(mesh, dev):
    if mesh.triangle_indices is None or mesh.vertex_positions is None:
        raise RuntimeError("Argument mesh needs to have both triangle vertex indices and vertex positions.")
    return to_device(mesh.vertex_positions, torch.float32, dev).reshape(-1, 3), to_device(mesh.triangle_indices, torch.int64, dev).reshape(-1, 3)


get_mesh_ndc_face_vertices_and_clip_mask = Overloaded(
    "get_mesh_ndc_face_vertices_and_clip_mask",
    "GetMeshNdcFaceVerticesAndClipMask, both overloads (cpp/pybind/rendering/functional/functional.cpp:36-54 -> ExtractFaceVertices.cpp:56-126): "
    "face vertices in NDC x, y + camera z [F,3,3] and the clip mask [F] (True = keep); a list of meshes is concatenated in mesh order and "
    "also returns the per-mesh face counts.")


@get_mesh_ndc_face_vertices_and_clip_mask.overload(lambda a: isinstance(a["camera_space_meshes"], (list, tuple)))
def _ndc_meshes(camera_space_meshes, intrinsic_matrix, image_size, near_clipping_distance=0.0, far_clipping_distance=float("inf")):
    _check_clipping(image_size, near_clipping_distance, far_clipping_distance)
    dev = _dev()
    arrays = [_mesh_arrays(m, dev) for m in camera_space_meshes]
    counts = np.array([f.shape[0] for _, f in arrays], np.int64)
    total = int(counts.sum())
    K = to_host_f64(intrinsic_matrix)
    H, W = int(image_size[0]), int(image_size[1])
    out = torch.empty((total, 3, 3), dtype=torch.float32, device=dev)
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    vptr = (ctypes.c_void_p * max(len(arrays), 1))(*[v.data_ptr() for v, _ in arrays])
    fptr = (ctypes.c_void_p * max(len(arrays), 1))(*[f.data_ptr() for _, f in arrays])
    N.check(N.lib().nnrt_get_meshes_ndc_face_vertices_and_clip_mask(vptr, fptr, N.ptr(counts), len(arrays), N.ptr(K), H, W,
                                                                    float(near_clipping_distance), float(far_clipping_distance), N.ptr(out),
                                                                    N.ptr(mask), N.stream_ptr()))
    return out, mask.bool(), torch.from_numpy(counts)


@get_mesh_ndc_face_vertices_and_clip_mask.overload()
def _ndc_mesh(camera_space_mesh, intrinsic_matrix, image_size, near_clipping_distance=0.0, far_clipping_distance=float("inf")):
    _check_clipping(image_size, near_clipping_distance, far_clipping_distance)
    dev = _dev()
    p, f = _mesh_arrays(camera_space_mesh, dev)
    K = to_host_f64(intrinsic_matrix)
    H, W = int(image_size[0]), int(image_size[1])
    out = torch.empty((f.shape[0], 3, 3), dtype=torch.float32, device=dev)
    mask = torch.empty(f.shape[0], dtype=torch.uint8, device=dev)
    N.check(N.lib().nnrt_get_mesh_ndc_face_vertices_and_clip_mask(N.ptr(p), N.ptr(f), f.shape[0], N.ptr(K), H, W, float(near_clipping_distance),
                                                                  float(far_clipping_distance), N.ptr(out), N.ptr(mask), N.stream_ptr()))
    return out, mask.bool()


def interpolate_vertex_attributes(pixel_face_indices, barycentric_coordinates, face_vertex_attributes):
    dev = _dev()
    pf = to_device(pixel_face_indices, torch.int64, dev)
    b = to_device(barycentric_coordinates, torch.float32, dev)
    a = to_device(face_vertex_attributes, torch.float32, dev)
    H, W, K = pf.shape
    C = a.shape[2]
    out = torch.empty((H, W, K, C), dtype=torch.float32, device=dev)
    N.check(N.lib().nnrt_interpolate_face_attributes(N.ptr(pf), N.ptr(b), H * W, K, N.ptr(a), C, N.ptr(out), N.stream_ptr()))
    return out


functional = types.SimpleNamespace(get_mesh_ndc_face_vertices_and_clip_mask=get_mesh_ndc_face_vertices_and_clip_mask,
                                   interpolate_vertex_attributes=interpolate_vertex_attributes)


# ---- shaders (csrc/shading.hip) --------------------------------------------------------------------------
SHADE_VERTEX_COLOR, SHADE_FLAT_EDGE, SHADE_HEADLIGHT = 0, 1, 2
NDC_REFERENCE, NDC_CONSISTENT = 0, 1   # nnrt_fitter_params.ndc_convention


def _one_mesh(meshes):
    """None, a mesh or a list of meshes -> None or one mesh, the list joined in mesh order."""
    if meshes is None:
        return None
    if isinstance(meshes, (list, tuple)):
        if len(meshes) == 0:
            return None
        return meshes[0] if len(meshes) == 1 else _geometry.join_triangle_meshes(meshes)
    return meshes


def _color3(color, name):
    c = np.ascontiguousarray(np.asarray(color, np.float32).reshape(-1))
    if c.shape != (3,):
        raise ValueError(f"{name} must have three components, got {c.shape[0]}")
    return c


def _shade(mode, pixel_face_indices, pixel_barycentric_coordinates, pixel_face_distances, mesh, color, pixel_line_width, ambient):
    dev = _dev()
    pf = to_device(pixel_face_indices, torch.int64, dev)
    if pf.dim() != 3:
        raise ValueError(f"pixel_face_indices must be [H, W, K], got {tuple(pf.shape)}")
    H, W, K = pf.shape
    bary = to_device(pixel_barycentric_coordinates, torch.float32, dev)
    dist = to_device(pixel_face_distances, torch.float32, dev)
    if tuple(bary.shape) != (H, W, K, 3) or tuple(dist.shape) != (H, W, K):
        raise ValueError(f"fragment shapes disagree: faces {tuple(pf.shape)}, barycentrics {tuple(bary.shape)}, distances {tuple(dist.shape)}")
    tri = colors = normals = None
    face_count = vertex_count = 0
    if mesh is not None and mode != SHADE_FLAT_EDGE:
        tri = to_device(mesh.triangle_indices, torch.int64, dev).reshape(-1, 3)
        face_count = tri.shape[0]
        attribute = to_device(mesh.vertex_colors if mode == SHADE_VERTEX_COLOR else mesh.vertex_normals, torch.float32, dev).reshape(-1, 3)
        vertex_count = attribute.shape[0]
        colors, normals = (attribute, None) if mode == SHADE_VERTEX_COLOR else (None, attribute)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    N.check(N.lib().nnrt_shade_pixels(mode, N.ptr(pf), N.ptr(bary), N.ptr(dist), H, W, K, N.ptr(tri), face_count, N.ptr(colors), N.ptr(normals),
                                      vertex_count, N.ptr(color), float(pixel_line_width), float(ambient), N.ptr(out), N.stream_ptr()))
    return out


class VertexColorShader:
    """VertexColorShader (cpp/rendering/VertexColorShader.cpp:29-61): the front fragment's barycentric mix of its face's
    vertex colours, times 255, as uint8 (values outside [0, 255] are clamped: DESIGN §22)."""

    def shade_meshes(self, pixel_face_indices, pixel_depths, pixel_barycentric_coordinates, pixel_face_distances, meshes=None):
        mesh = _one_mesh(meshes)
        if mesh is None:
            raise RuntimeError("VertexColorShader requires meshes argument to be filled with meshes that were used during rasterization "
                               "resulting in its other arguments, in order to retrieve and interpolate the vertex colors.")
        if mesh.vertex_colors is None:
            raise RuntimeError("VertexColorShader requires every mesh to have vertex_colors.")
        return _shade(SHADE_VERTEX_COLOR, pixel_face_indices, pixel_barycentric_coordinates, pixel_face_distances, mesh, None, 0.0, 0.0)


class FlatEdgeShader:
    """FlatEdgeShader (cpp/rendering/FlatEdgeShader.cpp, kernel/FlatEdgeShaderImpl.h:66-98): pixels whose front fragment lies
    within the line width of its face's edge, fading from line_color at the edge to black; needs a rasterization with a
    blur radius of at least the line width to see both sides of an edge. Needs no meshes."""

    def __init__(self, pixel_line_width, line_color):
        self.set_pixel_line_width(pixel_line_width)
        self.set_line_color(line_color)

    def set_pixel_line_width(self, width):
        self.pixel_line_width = float(width)

    def set_line_color(self, color):
        self.line_color = tuple(float(c) for c in _color3(color, "line_color"))

    def get_ndc_line_width(self, image_height, image_width) -> float:
        """ImageSpaceDistanceToNdc (CoordinateSystemConversions.h:98-101), in float32."""
        return float(np.float32(self.pixel_line_width) / (np.float32(min(int(image_height), int(image_width))) / np.float32(2.0)))

    def shade_meshes(self, pixel_face_indices, pixel_depths, pixel_barycentric_coordinates, pixel_face_distances, meshes=None):
        return _shade(SHADE_FLAT_EDGE, pixel_face_indices, pixel_barycentric_coordinates, pixel_face_distances, None,
                      _color3(self.line_color, "line_color"), self.pixel_line_width, 0.0)


class HeadlightShader:
    """Lambertian shading under a light along the optical axis (the reference has no lit shader): color times
    ambient + (1 - ambient) max(0, -n_z / |n|) of the interpolated camera-space vertex normal."""

    def __init__(self, color=(0.8, 0.8, 0.8), ambient=0.1):
        self.color = tuple(float(c) for c in _color3(color, "color"))
        self.ambient = float(ambient)

    def shade_meshes(self, pixel_face_indices, pixel_depths, pixel_barycentric_coordinates, pixel_face_distances, meshes=None):
        mesh = _one_mesh(meshes)
        if mesh is None:
            raise RuntimeError("HeadlightShader requires the meshes that were rasterized, for their vertex normals.")
        if mesh.vertex_normals is None:
            raise RuntimeError("HeadlightShader requires every mesh to have vertex_normals.")
        return _shade(SHADE_HEADLIGHT, pixel_face_indices, pixel_barycentric_coordinates, pixel_face_distances, mesh,
                      _color3(self.color, "color"), 0.0, self.ambient)


def _to_camera_space(mesh, extrinsics, dev):
    """World-space mesh -> camera space on the device: p' = R p + t, n' = R n (float32); the identity changes nothing."""
    E = to_host_f64(extrinsics).reshape(4, 4)
    p = to_device(mesh.vertex_positions, torch.float32, dev).reshape(-1, 3)
    n = None if mesh.vertex_normals is None else to_device(mesh.vertex_normals, torch.float32, dev).reshape(-1, 3)
    if not np.array_equal(E, np.eye(4)):
        R = torch.as_tensor(E[:3, :3], dtype=torch.float32, device=dev)
        t = torch.as_tensor(E[:3, 3], dtype=torch.float32, device=dev)
        p = p @ R.T + t
        n = None if n is None else n @ R.T
    return _geometry.TriangleMesh(p, n, to_device(mesh.triangle_indices, torch.int64, dev).reshape(-1, 3), None,
                                  None if mesh.vertex_colors is None else to_device(mesh.vertex_colors, torch.float32, dev).reshape(-1, 3))


def rasterize_meshes(meshes, intrinsic_matrix, image_size, extrinsics=np.eye(4), blur_radius_pixels=0.0, faces_per_pixel=1,
                     near_clipping_distance=0.0, far_clipping_distance=float("inf"), cull_back_faces=True, ndc_convention=NDC_REFERENCE):
    """render_meshes without the shader: (fragments, the meshes in camera space on the device)."""
    _check_clipping(image_size, near_clipping_distance, far_clipping_distance)
    dev = _dev()
    mesh_list = list(meshes) if isinstance(meshes, (list, tuple)) else [meshes]
    camera = [_to_camera_space(m, extrinsics, dev) for m in mesh_list]
    H, W = int(image_size[0]), int(image_size[1])
    consistent = int(ndc_convention) == NDC_CONSISTENT
    # the consistent mapping does not mirror y, which turns the winding in NDC: extract with two vertices swapped, as the
    # fitter does, and swap the barycentrics back
    faces = [m.triangle_indices[:, [0, 2, 1]].contiguous() if consistent else m.triangle_indices for m in camera]
    counts = np.array([f.shape[0] for f in faces], np.int64)
    total = int(counts.sum())
    K = to_host_f64(intrinsic_matrix)
    ndc = torch.empty((total, 3, 3), dtype=torch.float32, device=dev)
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    vptr = (ctypes.c_void_p * max(len(camera), 1))(*[m.vertex_positions.data_ptr() for m in camera])
    fptr = (ctypes.c_void_p * max(len(camera), 1))(*[f.data_ptr() for f in faces])
    N.check(N.lib().nnrt_get_meshes_ndc_face_vertices_and_clip_mask_in_convention(
        vptr, fptr, N.ptr(counts), len(camera), N.ptr(K), H, W, float(near_clipping_distance), float(far_clipping_distance),
        NDC_CONSISTENT if consistent else NDC_REFERENCE, N.ptr(ndc), N.ptr(mask), N.stream_ptr()))
    fi, depths, bary, dist = rasterize_ndc_triangles(ndc, mask, (H, W), blur_radius_pixels, faces_per_pixel, cull_back_faces=cull_back_faces)
    if consistent:
        bary = bary[..., [0, 2, 1]].contiguous()
    return (fi, depths, bary, dist), camera


def render_meshes(meshes, intrinsic_matrix, image_size, shader, extrinsics=np.eye(4), blur_radius_pixels=0.0, faces_per_pixel=1,
                  near_clipping_distance=0.0, far_clipping_distance=float("inf"), cull_back_faces=True, ndc_convention=NDC_REFERENCE):
    """World-space mesh or meshes -> (image uint8 [H, W, 3], fragments): to camera space by `extrinsics` (world -> camera),
    NDC extraction, rasterization, `shader`.shade_meshes. `fragments` are the rasterizer's four tensors (face indices,
    depths, barycentrics, distances), faces numbered over the meshes in order. ndc_convention: NDC_REFERENCE is
    get_mesh_ndc_face_vertices_and_clip_mask's mapping (reference quirk A11: rows mirrored about cy); NDC_CONSISTENT puts
    pixel (u, v) of the intrinsics on raster pixel (u, v), which a render compared with a depth frame needs. The
    barycentrics refer to the meshes' own triangles in both."""
    fragments, camera = rasterize_meshes(meshes, intrinsic_matrix, image_size, extrinsics, blur_radius_pixels, faces_per_pixel,
                                         near_clipping_distance, far_clipping_distance, cull_back_faces, ndc_convention)
    return shader.shade_meshes(*fragments, camera), fragments


@dataclass
class DepthAgreement:
    """Statistics of rasterized model depth minus frame depth over the pixels valid on both sides (`both`); `model_only` and
    `frame_only` count the pixels valid on one side; `inliers` those of `both` with |d| <= the inlier threshold."""
    both: int = 0
    model_only: int = 0
    frame_only: int = 0
    inliers: int = 0
    sum_abs: float = 0.0
    sum_sq: float = 0.0
    max_abs: float = 0.0

    @property
    def mean_abs(self) -> float:
        return self.sum_abs / self.both if self.both else 0.0

    @property
    def rmse(self) -> float:
        return math.sqrt(self.sum_sq / self.both) if self.both else 0.0

    @property
    def inlier_ratio(self) -> float:
        return self.inliers / self.both if self.both else 0.0


class _DepthAgreementRecord(ctypes.Structure):
    _fields_ = [("both", ctypes.c_int64), ("model_only", ctypes.c_int64), ("frame_only", ctypes.c_int64), ("inliers", ctypes.c_int64),
                ("sum_abs", ctypes.c_double), ("sum_sq", ctypes.c_double), ("max_abs", ctypes.c_float), ("reserved", ctypes.c_int32)]


def compare_depth_to_raster(pixel_face_indices, pixel_depths, depth, depth_scale=1000.0, depth_max=3.0, inlier_threshold=0.01):
    """Rasterized model depth (slot 0; valid where the face is >= 0) against a depth frame [H, W], uint16 in sensor units or
    float32 (valid iff 0 < raw / depth_scale < depth_max): (DepthAgreement, difference image [H, W] float32 on the device,
    model - frame in metres, NaN where either side is invalid). The sums are reproducible (csrc/shading.hip)."""
    dev = _dev()
    pf = to_device(pixel_face_indices, torch.int64, dev)
    pd = to_device(pixel_depths, torch.float32, dev)
    if pf.dim() != 3 or pd.shape != pf.shape:
        raise ValueError(f"pixel_face_indices and pixel_depths must both be [H, W, K], got {tuple(pf.shape)} and {tuple(pd.shape)}")
    H, W, K = pf.shape
    if image_proc._is_depth_u16(depth):
        d, code = image_proc._depth_on_device(depth, torch.int16), image_proc.DTYPE_UINT16
    elif (isinstance(depth, np.ndarray) and depth.dtype == np.float32) or (isinstance(depth, torch.Tensor) and depth.dtype == torch.float32):
        d, code = image_proc._depth_on_device(depth, torch.float32), image_proc.DTYPE_FLOAT32
    else:
        raise ValueError("depth must be a uint16 or float32 image (numpy or torch)")
    if tuple(d.shape) != (H, W):
        raise ValueError(f"depth must be [{H}, {W}] like the fragments, got {tuple(d.shape)}")
    difference = torch.empty((H, W), dtype=torch.float32, device=dev)
    record = _DepthAgreementRecord()
    N.check(N.lib().nnrt_compare_depth_to_raster(N.ptr(pf), N.ptr(pd), H, W, K, N.ptr(d), code, float(depth_scale), float(depth_max),
                                                 float(inlier_threshold), N.ptr(difference), ctypes.byref(record), N.stream_ptr()))
    return DepthAgreement(int(record.both), int(record.model_only), int(record.frame_only), int(record.inliers), float(record.sum_abs),
                          float(record.sum_sq), float(record.max_abs)), difference


# ---- the model's motion field and its score against a flow image (csrc/motion.hip) -------------------------
@dataclass
class MotionImages:
    """The motion of a mesh between two states on the source state's pixel grid, device tensors: `source_points` [H, W, 3]
    (source camera space, metres), `scene_flow` [H, W, 3] (target point in the target camera minus source point in the
    source camera), `optical_flow` [H, W, 2] (pixels: the projection of the target point minus that of the source point)
    and `mask` [H, W] bool. Where the mask is False the three images are zero (DeepDeform's convention)."""
    source_points: torch.Tensor
    scene_flow: torch.Tensor
    optical_flow: torch.Tensor
    mask: torch.Tensor


def motion_from_fragments(pixel_face_indices, pixel_barycentric_coordinates, triangle_indices, source_positions, target_positions,
                          intrinsic_matrix):
    """MotionImages from slot 0 of a rasterization of the source state: per pixel with a face, the barycentric blend of the
    face's vertices in `source_positions` [V, 3] (source camera space) and in `target_positions` [V, 3] (target camera
    space), their difference and the difference of their projections by `intrinsic_matrix`. Valid iff the pixel has a face
    and both blended points have z > 0. The barycentrics refer to the rows of `triangle_indices` as given."""
    dev = _dev()
    pf = to_device(pixel_face_indices, torch.int64, dev)
    if pf.dim() != 3:
        raise ValueError(f"pixel_face_indices must be [H, W, K], got {tuple(pf.shape)}")
    H, W, K = pf.shape
    bary = to_device(pixel_barycentric_coordinates, torch.float32, dev)
    if tuple(bary.shape) != (H, W, K, 3):
        raise ValueError(f"pixel_barycentric_coordinates must be [{H}, {W}, {K}, 3] like the faces, got {tuple(bary.shape)}")
    tri = to_device(triangle_indices, torch.int64, dev).reshape(-1, 3)
    source = to_device(source_positions, torch.float32, dev)
    target = to_device(target_positions, torch.float32, dev)
    if source.dim() != 2 or source.shape[1] != 3 or target.shape != source.shape:
        raise ValueError(f"source_positions and target_positions must both be [V, 3], got {tuple(source.shape)} and {tuple(target.shape)}")
    Km = to_host_f64(intrinsic_matrix)
    points = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    scene = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    optical = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    N.check(N.lib().nnrt_motion_pixels(N.ptr(pf), N.ptr(bary), H, W, K, N.ptr(tri), tri.shape[0], N.ptr(source), N.ptr(target), source.shape[0],
                                       float(Km[0, 0]), float(Km[1, 1]), float(Km[0, 2]), float(Km[1, 2]), N.ptr(points), N.ptr(scene),
                                       N.ptr(optical), N.ptr(mask), N.stream_ptr()))
    return MotionImages(points, scene, optical, mask.bool())


def render_motion(source_mesh, target_vertex_positions, intrinsic_matrix, image_size, source_extrinsics=np.eye(4), target_extrinsics=np.eye(4),
                  ndc_convention=NDC_CONSISTENT):
    """(MotionImages, fragments) of a world-space mesh that moves from `source_mesh`'s vertex positions, seen by the camera
    `source_extrinsics` (world -> camera), to `target_vertex_positions` [V, 3], seen by `target_extrinsics`: both sides to
    their camera spaces, the source rasterized at one face per pixel, motion_from_fragments. The images are on the source
    camera's pixel grid; with NDC_CONSISTENT (the default) raster pixel (u, v) is pixel (u, v) of the intrinsics, which a
    comparison with a flow image of the source frame needs."""
    dev = _dev()
    source = _to_camera_space(source_mesh, source_extrinsics, dev)
    moved = to_device(target_vertex_positions, torch.float32, dev)
    if tuple(moved.shape) != tuple(source.vertex_positions.shape):
        raise ValueError(f"target_vertex_positions must be {tuple(source.vertex_positions.shape)} like the source mesh's vertices, "
                         f"got {tuple(moved.shape)}")
    target = _to_camera_space(_geometry.TriangleMesh(moved, None, source.triangle_indices), target_extrinsics, dev)
    fragments, _ = rasterize_meshes(source, intrinsic_matrix, image_size, faces_per_pixel=1, ndc_convention=ndc_convention)
    images = motion_from_fragments(fragments[0], fragments[2], source.triangle_indices, source.vertex_positions, target.vertex_positions,
                                   intrinsic_matrix)
    return images, fragments


@dataclass
class FlowAgreement:
    """Statistics of the end-point error of a predicted flow image against a truth image over the pixels valid on both sides
    (`both`); `predicted_only` and `truth_only` count the pixels valid on one side; `inliers` those of `both` with an error
    <= the inlier threshold. `sum_epe` and `sum_sq` are the float64 sums of the error and of its square."""
    both: int = 0
    predicted_only: int = 0
    truth_only: int = 0
    inliers: int = 0
    sum_epe: float = 0.0
    sum_sq: float = 0.0
    max_epe: float = 0.0

    @property
    def mean_epe(self) -> float:
        return self.sum_epe / self.both if self.both else 0.0

    @property
    def rmse(self) -> float:
        return math.sqrt(self.sum_sq / self.both) if self.both else 0.0

    @property
    def inlier_ratio(self) -> float:
        return self.inliers / self.both if self.both else 0.0


class _FlowAgreementRecord(ctypes.Structure):   # nnrt_flow_agreement
    _fields_ = [("both", ctypes.c_int64), ("predicted_only", ctypes.c_int64), ("truth_only", ctypes.c_int64), ("inliers", ctypes.c_int64),
                ("sum_epe", ctypes.c_double), ("sum_sq", ctypes.c_double), ("max_epe", ctypes.c_float), ("reserved", ctypes.c_int32)]


def compare_flow(predicted, predicted_mask, truth, truth_mask=None, *, inlier_threshold):
    """A predicted flow image [H, W, C] with its mask [H, W] against a truth image [H, W, C], C = 2 (optical flow, pixels) or
    3 (scene flow, metres): (FlowAgreement, error image [H, W] float32 on the device, NaN where either side is invalid). A
    truth pixel is valid iff `truth_mask`, if given, is non-zero there and all its channels are finite. `inlier_threshold`
    is in the flow's own unit and has no default. The sums are reproducible (csrc/motion.hip)."""
    dev = _dev()
    flow = to_device(predicted, torch.float32, dev)
    if flow.dim() != 3 or flow.shape[2] not in (2, 3):
        raise ValueError(f"predicted must be [H, W, 2] or [H, W, 3], got {tuple(flow.shape)}")
    H, W, C = flow.shape
    true_flow = to_device(truth, torch.float32, dev)
    if tuple(true_flow.shape) != (H, W, C):
        raise ValueError(f"truth must be [{H}, {W}, {C}] like predicted, got {tuple(true_flow.shape)}")

    def mask_on_device(mask, name):
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
        if tuple(m.shape) != (H, W):
            raise ValueError(f"{name} must be [{H}, {W}], got {tuple(m.shape)}")
        return (m != 0).to(device=dev, dtype=torch.uint8).contiguous()

    flow_mask = mask_on_device(predicted_mask, "predicted_mask")
    true_mask = None if truth_mask is None else mask_on_device(truth_mask, "truth_mask")
    error = torch.empty((H, W), dtype=torch.float32, device=dev)
    record = _FlowAgreementRecord()
    N.check(N.lib().nnrt_flow_error(N.ptr(flow), N.ptr(flow_mask), N.ptr(true_flow), N.ptr(true_mask), H, W, C, float(inlier_threshold),
                                    N.ptr(error), ctypes.byref(record), N.stream_ptr()))
    return FlowAgreement(int(record.both), int(record.predicted_only), int(record.truth_only), int(record.inliers), float(record.sum_epe),
                         float(record.sum_sq), float(record.max_epe)), error
