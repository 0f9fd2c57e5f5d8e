// The C-ABI (include/nnrt_mi355x.h) apart from the fitter (fitter.hip): the warp-field handle and the stateless entry points.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <list>
#include <vector>

#include "handles.hpp"

namespace nnrt {

namespace {
thread_local std::string g_error;
std::atomic<uint64_t> g_next_warp_field_id{1};
}
void set_error(const std::string& message) { g_error = message; }
const std::string& get_error() { return g_error; }

NdcSetup make_ndc_setup(const double* K, int height, int width, bool consistent) {
	// CoordinateSystemConversions.h:109-146. consistent = false reproduces the reference (A11: rows mirrored about cy, columns
	// shifted by w - 2cx, clip window centred on the NDC principal point); consistent = true maps pixel (u, v) of the
	// intrinsics K onto the centre of raster pixel (u, v), the clip window being the image.
	const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
	const double h = height, w = width;
	const double s = std::min(w, h);
	const float range_x = ndc_range(width, height);
	const float range_y = ndc_range(height, width);
	const double fx_ndc = 2.0 * fx / s, fy_ndc = (consistent ? 2.0 : -2.0) * fy / s;
	const double cx_ndc = consistent ? (2.0 * cx + 1.0 - w) / s : -(2.0 * cx - w) / s;
	const double cy_ndc = consistent ? (2.0 * cy + 1.0 - h) / s : (2.0 * cy - h) / s;
	const double wx = consistent ? 0.0 : cx_ndc, wy = consistent ? 0.0 : cy_ndc;
	NdcSetup r;
	r.ndc = Camera{static_cast<float>(fx_ndc), static_cast<float>(fy_ndc), static_cast<float>(cx_ndc), static_cast<float>(cy_ndc)};
	r.min_x = static_cast<float>(wx - range_x / 2.f);
	r.max_x = static_cast<float>(wx + range_x / 2.f);
	r.min_y = static_cast<float>(wy - range_y / 2.f);
	r.max_y = static_cast<float>(wy + range_y / 2.f);
	return r;
}

WarpExtrinsics make_extrinsics(const double* E) {
	WarpExtrinsics r{};
	r.identity = 1;
	const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
	for (int i = 0; i < 12; i++) {
		const double v = E ? E[i] : I[i];
		r.m[i] = static_cast<float>(v);
		if (v != I[i]) r.identity = 0;
	}
	return r;
}

Camera pixel_camera(const double* K) {
	return Camera{static_cast<float>(K[0]), static_cast<float>(K[4]), static_cast<float>(K[2]), static_cast<float>(K[5])};
}

} // namespace nnrt

using namespace nnrt;

// =====================================================================================================================
// warp field
// =====================================================================================================================

namespace nnrt {
WarpFieldView warp_field_view(const void* handle) {
	const nnrt_warp_field* wf = static_cast<const nnrt_warp_field*>(handle);
	WarpFieldView v{};
	v.N = wf->N;
	v.anchor_count = wf->anchor_count;
	v.minimum_valid = wf->minimum_valid;
	v.fixed_coverage = wf->coverage_method == NNRT_MINIMAL_K_NEIGHBOR_NODE_DISTANCE ? 0 : 1;
	v.coverage = wf->coverage;
	v.state = wf->state.ptr;
	v.node_weights = wf->node_weights.ptr;
	v.device = wf->device;
	return v;
}
} // namespace nnrt

namespace {
nnrt_status wf_download_state(const nnrt_warp_field* wf, std::vector<float>& host) {
	host.resize(static_cast<size_t>(wf->N) * NODE_STRIDE);
	NNRT_HIP(hipMemcpy(host.data(), wf->state.ptr, sizeof(float) * host.size(), hipMemcpyDeviceToHost));
	return NNRT_OK;
}
nnrt_status wf_upload_state(nnrt_warp_field* wf, const std::vector<float>& host) {
	NNRT_HIP(hipMemcpy(wf->state.ptr, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice));
	return NNRT_OK;
}
} // namespace

extern "C" {

const char* nnrt_last_error(void) { return get_error().c_str(); }

int32_t nnrt_runtime_version(void) {
	int v = 0;
	if (hipRuntimeGetVersion(&v) != hipSuccess) return -1;
	return v;
}

int32_t nnrt_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return -1;
	return n;
}

int64_t nnrt_device_bytes_in_use(void) { return g_device_bytes_in_use.load(std::memory_order_relaxed); }

nnrt_status nnrt_warp_field_create(const float* h_nodes, int32_t node_count, float node_coverage, int32_t threshold_nodes_by_distance,
                                   int32_t anchor_count, int32_t minimum_valid_anchor_count, int32_t coverage_method, int32_t layer_count,
                                   int32_t max_vertex_degree, const float* h_layer_radii, int32_t device, nnrt_warp_field** out) {
	NNRT_CHECK_ARG(out != nullptr && h_nodes != nullptr, "null pointer");
	NNRT_CHECK_ARG(node_count >= 1, "node_count must be positive");
	NNRT_CHECK_ARG(anchor_count >= 1 && anchor_count <= MAX_ANCHORS, "anchor_count must be in [1, 8]");
	if (node_count < anchor_count) {
		set_error("Anchor count for warp field exceeds node count (WarpField.cpp:57-61)");
		return NNRT_ERROR_ARGUMENT;
	}
	NNRT_CHECK_ARG(minimum_valid_anchor_count >= 0 && minimum_valid_anchor_count <= anchor_count, "minimum_valid_anchor_count > anchor_count");
	NNRT_CHECK_ARG(coverage_method == NNRT_FIXED_NODE_COVERAGE || coverage_method == NNRT_MINIMAL_K_NEIGHBOR_NODE_DISTANCE,
	               "unknown coverage method");
	DeviceGuard guard(device);
	auto wf = std::make_unique<nnrt_warp_field>();
	wf->device = device;
	wf->id = g_next_warp_field_id.fetch_add(1);
	wf->N = node_count;
	wf->coverage = node_coverage;
	wf->threshold = threshold_nodes_by_distance;
	wf->anchor_count = anchor_count;
	wf->minimum_valid = minimum_valid_anchor_count;
	wf->coverage_method = coverage_method;
	wf->nodes_original.assign(h_nodes, h_nodes + 3 * static_cast<size_t>(node_count));
	HierarchyOps& ops = device_hierarchy_ops();
	nnrt_status st = build_hierarchy(h_nodes, node_count, node_coverage, layer_count, max_vertex_degree, h_layer_radii, ops, wf->h);
	if (st) return st;
	std::vector<float> weights_original;
	if ((st = ops.coverage_weights(h_nodes, node_count, node_coverage, weights_original))) return st;
	std::vector<float> state(static_cast<size_t>(node_count) * NODE_STRIDE, 0.f), pos(3 * static_cast<size_t>(node_count));
	wf->weights_virtual.resize(node_count);
	for (int v = 0; v < node_count; v++) {
		const int64_t o = wf->h.virtual_indices[v];
		float* s = &state[static_cast<size_t>(v) * NODE_STRIDE];
		for (int c = 0; c < 3; c++) {
			s[c] = h_nodes[3 * o + c];
			pos[3 * v + c] = h_nodes[3 * o + c];
		}
		s[6] = s[10] = s[14] = 1.f;   // identity rotation (WarpField::ResetRotations)
		wf->weights_virtual[v] = weights_original[o];
	}
	if ((st = wf->state.ensure(state.size()))) return st;
	if ((st = wf->node_positions.ensure(pos.size()))) return st;
	if ((st = wf->node_weights.ensure(node_count))) return st;
	const int E = wf->E();
	if ((st = wf->edges.ensure(2 * static_cast<size_t>(E)))) return st;
	if ((st = wf->edge_layers.ensure(E))) return st;
	if ((st = wf->radii.ensure(wf->h.radii.size()))) return st;
	NNRT_HIP(hipMemcpy(wf->state.ptr, state.data(), sizeof(float) * state.size(), hipMemcpyHostToDevice));
	NNRT_HIP(hipMemcpy(wf->node_positions.ptr, pos.data(), sizeof(float) * pos.size(), hipMemcpyHostToDevice));
	NNRT_HIP(hipMemcpy(wf->node_weights.ptr, wf->weights_virtual.data(), sizeof(float) * node_count, hipMemcpyHostToDevice));
	if (E > 0) {
		NNRT_HIP(hipMemcpy(wf->edges.ptr, wf->h.edges.data(), sizeof(int32_t) * 2 * E, hipMemcpyHostToDevice));
		NNRT_HIP(hipMemcpy(wf->edge_layers.ptr, wf->h.edge_layers.data(), sizeof(int8_t) * E, hipMemcpyHostToDevice));
	}
	NNRT_HIP(hipMemcpy(wf->radii.ptr, wf->h.radii.data(), sizeof(float) * wf->h.radii.size(), hipMemcpyHostToDevice));
	*out = wf.release();
	return NNRT_OK;
}

void nnrt_warp_field_destroy(nnrt_warp_field* wf) {
	if (!wf) return;
	DeviceGuard guard(wf->device);
	delete wf;
}

int32_t nnrt_warp_field_node_count(const nnrt_warp_field* wf) { return wf ? wf->N : -1; }
int32_t nnrt_warp_field_edge_count(const nnrt_warp_field* wf) { return wf ? wf->E() : -1; }
int32_t nnrt_warp_field_layer_counts(const nnrt_warp_field* wf, int32_t* h_counts) {
	if (!wf) return -1;
	for (size_t i = 0; i < wf->h.layer_counts.size(); i++)
		if (h_counts) h_counts[i] = wf->h.layer_counts[i];
	return static_cast<int32_t>(wf->h.layer_counts.size());
}

nnrt_status nnrt_warp_field_get_virtual_node_indices(const nnrt_warp_field* wf, int64_t* h_out) {
	NNRT_CHECK_ARG(wf && h_out, "null pointer");
	std::memcpy(h_out, wf->h.virtual_indices.data(), sizeof(int64_t) * wf->N);
	return NNRT_OK;
}

nnrt_status nnrt_warp_field_get_edges(const nnrt_warp_field* wf, int32_t* h_edges, int8_t* h_edge_layers) {
	NNRT_CHECK_ARG(wf, "null pointer");
	if (h_edges) std::memcpy(h_edges, wf->h.edges.data(), sizeof(int32_t) * wf->h.edges.size());
	if (h_edge_layers) std::memcpy(h_edge_layers, wf->h.edge_layers.data(), wf->h.edge_layers.size());
	return NNRT_OK;
}

static nnrt_status wf_get(const nnrt_warp_field* wf, float* h_out, int virtual_order, int offset, int width) {
	NNRT_CHECK_ARG(wf && h_out, "null pointer");
	DeviceGuard guard(wf->device);
	std::vector<float> s;
	nnrt_status st = wf_download_state(wf, s);
	if (st) return st;
	for (int v = 0; v < wf->N; v++) {
		const int64_t dst = virtual_order ? v : wf->h.virtual_indices[v];
		for (int c = 0; c < width; c++) h_out[dst * width + c] = s[static_cast<size_t>(v) * NODE_STRIDE + offset + c];
	}
	return NNRT_OK;
}

static nnrt_status wf_set(nnrt_warp_field* wf, const float* h_in, int virtual_order, int offset, int width) {
	NNRT_CHECK_ARG(wf && h_in, "null pointer");
	DeviceGuard guard(wf->device);
	std::vector<float> s;
	nnrt_status st = wf_download_state(wf, s);
	if (st) return st;
	for (int v = 0; v < wf->N; v++) {
		const int64_t src = virtual_order ? v : wf->h.virtual_indices[v];
		for (int c = 0; c < width; c++) s[static_cast<size_t>(v) * NODE_STRIDE + offset + c] = h_in[src * width + c];
	}
	return wf_upload_state(wf, s);
}

nnrt_status nnrt_warp_field_get_node_positions(const nnrt_warp_field* wf, float* h_out, int32_t virtual_order) {
	return wf_get(wf, h_out, virtual_order, 0, 3);
}
nnrt_status nnrt_warp_field_get_node_translations(const nnrt_warp_field* wf, float* h_out, int32_t virtual_order) {
	return wf_get(wf, h_out, virtual_order, 3, 3);
}
nnrt_status nnrt_warp_field_get_node_rotations(const nnrt_warp_field* wf, float* h_out, int32_t virtual_order) {
	return wf_get(wf, h_out, virtual_order, 6, 9);
}
nnrt_status nnrt_warp_field_set_node_translations(nnrt_warp_field* wf, const float* h_in, int32_t virtual_order) {
	return wf_set(wf, h_in, virtual_order, 3, 3);
}
nnrt_status nnrt_warp_field_set_node_rotations(nnrt_warp_field* wf, const float* h_in, int32_t virtual_order) {
	return wf_set(wf, h_in, virtual_order, 6, 9);
}
__global__ void k_reset_motion(float* state, int N) {
	const int n = blockIdx.x * blockDim.x + threadIdx.x;
	if (n >= N) return;
	float* s = state + static_cast<int64_t>(n) * NODE_STRIDE;
	for (int c = 3; c < 15; c++) s[c] = 0.f;
	s[6] = s[10] = s[14] = 1.f;
}

// node-state copy (snapshot / restore): one float4 per lane; a 1500-node state is 96 KB (a runtime blit kernel costs
// several microseconds more inside a graph)
__global__ void k_copy_state(const float4* __restrict__ src, float4* __restrict__ dst, int count) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < count) dst[i] = src[i];
}

nnrt_status nnrt_warp_field_reset_motion(nnrt_warp_field* wf, void* stream) {
	NNRT_CHECK_ARG(wf, "null pointer");
	DeviceGuard guard(wf->device);
	return launch_reset_motion(wf->state.ptr, wf->N, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_warp_field_get_node_coverage_weights(const nnrt_warp_field* wf, float* h_out) {
	NNRT_CHECK_ARG(wf && h_out, "null pointer");
	std::memcpy(h_out, wf->weights_virtual.data(), sizeof(float) * wf->N);
	return NNRT_OK;
}

} // extern "C"

namespace nnrt {
nnrt_status launch_reset_motion(float* state, int N, hipStream_t s) {
	k_reset_motion<<<static_cast<unsigned>(ceil_div(N, 256)), 256, 0, s>>>(state, N);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}
nnrt_status launch_copy_state(const float* src, float* dst, int N, hipStream_t s) {
	const int count = N * (NODE_STRIDE / 4);
	k_copy_state<<<static_cast<unsigned>(ceil_div(count, 256)), 256, 0, s>>>(reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), count);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}
} // namespace nnrt

// [a, a + na) and [b, b + nb) share a byte
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
	const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
	return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

extern "C" {

// ---------------------------------------------------------------------------------------------------------------------
// stage entry points
// ---------------------------------------------------------------------------------------------------------------------
nnrt_status nnrt_compute_anchors_and_weights_shortest_path(const float* d_points, int64_t V, const float* d_nodes, int32_t N, const int32_t* d_edges,
                                                           int32_t D, int32_t K, float coverage, const float* d_node_weights,
                                                           int32_t* d_anchors, float* d_weights, void* stream) {
	NNRT_CHECK_ARG(V == 0 || (d_points && d_anchors && d_weights), "null pointer");
	NNRT_CHECK_ARG(N == 0 || V == 0 || (d_nodes && d_edges), "null pointer");
	return launch_anchors_shortest_path(d_points, V, d_nodes, N, d_edges, D, K, coverage, d_node_weights, d_anchors, d_weights,
	                                    static_cast<hipStream_t>(stream));
}

// the argument checks the two rigid alignment entry points share; log_columns: 2, or 4 for the hybrid log
static nnrt_status check_rigid_align_arguments(const float* d_points, const float* d_normals, int64_t V, const float* d_target_points,
                                               const float* d_target_normals, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                               const double* h_T_init, int32_t iterations, float distance_threshold, float normal_agreement_cos,
                                               int32_t minimum_correspondence_count, const double* h_T_out, const double* h_log,
                                               int32_t log_row_capacity, const int32_t* h_status) {
	NNRT_CHECK_ARG(V >= 0, "points: negative vertex count");
	NNRT_CHECK_ARG(V == 0 || d_points, "points: null pointer");
	NNRT_CHECK_ARG(V == 0 || d_normals, "normals: null pointer");
	NNRT_CHECK_ARG(H >= 1 && W >= 1, "target_points: height and width must be at least 1");
	NNRT_CHECK_ARG(V == 0 || d_target_points, "target_points: null pointer");
	NNRT_CHECK_ARG(V == 0 || d_target_normals, "target_normals: null pointer");
	NNRT_CHECK_ARG(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy), "intrinsics: fx, fy, cx, cy must be finite");
	NNRT_CHECK_ARG(h_T_init, "T_init: null pointer");
	for (int k = 0; k < 12; k++) NNRT_CHECK_ARG(std::isfinite(h_T_init[k]), "T_init: rows 0..2 must be finite");
	NNRT_CHECK_ARG(iterations >= 1, "iterations must be at least 1");
	NNRT_CHECK_ARG(std::isfinite(distance_threshold) && distance_threshold > 0.f, "distance_threshold must be positive and finite");
	NNRT_CHECK_ARG(!std::isnan(normal_agreement_cos), "normal_agreement_cos is NaN");
	NNRT_CHECK_ARG(minimum_correspondence_count >= 0, "minimum_correspondence_count is negative");
	NNRT_CHECK_ARG(h_T_out, "T_out: null pointer");
	NNRT_CHECK_ARG(h_log, "log: null pointer");
	NNRT_CHECK_ARG(log_row_capacity >= iterations, "log: room for " + std::to_string(log_row_capacity) + " rows, " +
	                                                    std::to_string(iterations) + " iterations need as many");
	NNRT_CHECK_ARG(h_status, "status: null pointer");
	return NNRT_OK;
}

nnrt_status nnrt_rigid_align_point_to_plane(const float* d_points, const float* d_normals, int64_t V, const float* d_target_points,
                                            const float* d_target_normals, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                                            const double* h_T_init, int32_t iterations, float distance_threshold, float normal_agreement_cos,
                                            int32_t cull_back_faces, int32_t minimum_correspondence_count, double* h_T_out, double* h_log,
                                            int32_t log_row_capacity, int32_t* h_status, void* stream) {
	if (nnrt_status st = check_rigid_align_arguments(d_points, d_normals, V, d_target_points, d_target_normals, H, W, fx, fy, cx, cy, h_T_init,
	                                                 iterations, distance_threshold, normal_agreement_cos, minimum_correspondence_count, h_T_out,
	                                                 h_log, log_row_capacity, h_status))
		return st;
	if (V == 0) {   // nothing to align: an ordinary result
		for (int k = 0; k < 16; k++) h_T_out[k] = h_T_init[k];
		for (int k = 0; k < 2 * iterations; k++) h_log[k] = 0.0;
		*h_status = NNRT_RIGID_ALIGN_DEGENERATE;
		return NNRT_OK;
	}
	return launch_rigid_align(d_points, d_normals, V, d_target_points, d_target_normals, H, W, fx, fy, cx, cy, h_T_init, iterations,
	                          distance_threshold, normal_agreement_cos, cull_back_faces, minimum_correspondence_count, h_T_out, h_log, h_status,
	                          static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_rigid_align_hybrid(const float* d_points, const float* d_normals, const float* d_colors, int64_t V, const float* d_target_points,
                                    const float* d_target_normals, const float* d_target_intensity, int32_t H, int32_t W, float fx, float fy,
                                    float cx, float cy, const double* h_T_init, int32_t iterations, float distance_threshold,
                                    float normal_agreement_cos, int32_t cull_back_faces, int32_t minimum_correspondence_count,
                                    float photometric_weight, float photometric_residual_threshold, double* h_T_out, double* h_log,
                                    int32_t log_row_capacity, int32_t* h_status, void* stream) {
	if (nnrt_status st = check_rigid_align_arguments(d_points, d_normals, V, d_target_points, d_target_normals, H, W, fx, fy, cx, cy, h_T_init,
	                                                 iterations, distance_threshold, normal_agreement_cos, minimum_correspondence_count, h_T_out,
	                                                 h_log, log_row_capacity, h_status))
		return st;
	NNRT_CHECK_ARG(V == 0 || d_colors, "colors: null pointer");
	NNRT_CHECK_ARG(V == 0 || d_target_intensity, "target_intensity: null pointer");
	NNRT_CHECK_ARG(std::isfinite(photometric_weight) && photometric_weight > 0.f, "photometric_weight must be positive and finite");
	NNRT_CHECK_ARG(!std::isnan(photometric_residual_threshold), "photometric_residual_threshold is NaN");
	// the host outputs are written after the inputs were read, but a log or status inside T_out (or one another) would be clobbered
	const size_t log_bytes = sizeof(double) * 4 * static_cast<size_t>(iterations);
	NNRT_CHECK_ARG(!ranges_overlap(h_T_out, sizeof(double) * 16, h_log, log_bytes) && !ranges_overlap(h_T_out, sizeof(double) * 16, h_status, 4) &&
	                   !ranges_overlap(h_log, log_bytes, h_status, 4),
	               "T_out, log and status must not overlap");
	NNRT_CHECK_ARG(!ranges_overlap(h_T_init, sizeof(double) * 16, h_log, log_bytes) && !ranges_overlap(h_T_init, sizeof(double) * 16, h_status, 4),
	               "log and status must not overlap T_init");
	if (V == 0) {
		for (int k = 0; k < 16; k++) h_T_out[k] = h_T_init[k];
		for (int k = 0; k < 4 * iterations; k++) h_log[k] = 0.0;
		*h_status = NNRT_RIGID_ALIGN_DEGENERATE;
		return NNRT_OK;
	}
	return launch_rigid_align(d_points, d_normals, V, d_target_points, d_target_normals, H, W, fx, fy, cx, cy, h_T_init, iterations,
	                          distance_threshold, normal_agreement_cos, cull_back_faces, minimum_correspondence_count, h_T_out, h_log, h_status,
	                          static_cast<hipStream_t>(stream), d_colors, d_target_intensity, photometric_weight,
	                          photometric_residual_threshold);
}

nnrt_status nnrt_intensity_from_rgb8(const uint8_t* d_rgb, int32_t height, int32_t width, float* d_out, void* stream) {
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_rgb, "null d_rgb");
	NNRT_CHECK_ARG(d_out, "null d_out");
	NNRT_CHECK_ARG(!ranges_overlap(d_rgb, 3 * pixels, d_out, sizeof(float) * pixels), "d_out must not overlap d_rgb");
	return launch_intensity_rgb8(d_rgb, height, width, d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_intensity_halve(const float* d_in, int32_t height, int32_t width, float* d_out, void* stream) {
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_in, "null d_in");
	NNRT_CHECK_ARG(d_out, "null d_out");
	const size_t out_pixels = static_cast<size_t>((height + 1) / 2) * static_cast<size_t>((width + 1) / 2);
	NNRT_CHECK_ARG(!ranges_overlap(d_in, sizeof(float) * pixels, d_out, sizeof(float) * out_pixels),
	               "d_out must not overlap d_in (the filter reads every pixel's neighbours)");
	return launch_intensity_halve(d_in, height, width, d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_corner_scores(const float* d_intensity, int32_t height, int32_t width, int32_t window_radius, float* d_out_scores, void* stream) {
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(window_radius >= 1 && window_radius <= NNRT_FEATURE_MAX_WINDOW_RADIUS, "window_radius must be in [1, 7]");
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	NNRT_CHECK_ARG(pixels < (size_t(1) << 31), "height * width must be below 2^31");
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_intensity, "null d_intensity");
	NNRT_CHECK_ARG(d_out_scores, "null d_out_scores");
	NNRT_CHECK_ARG(!ranges_overlap(d_intensity, sizeof(float) * pixels, d_out_scores, sizeof(float) * pixels),
	               "d_out_scores must not overlap d_intensity");
	return launch_corner_scores(d_intensity, height, width, window_radius, d_out_scores, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_select_features(const float* d_scores, const uint8_t* d_mask, int32_t height, int32_t width, float quality, int32_t nms_radius,
                                 int32_t max_count, float* d_out_points, int64_t* h_out_count, void* stream) {
	NNRT_CHECK_ARG(h_out_count, "null h_out_count");
	*h_out_count = 0;
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(quality >= 0.f && quality <= 1.f, "quality must be in [0, 1]");   // refuses NaN
	NNRT_CHECK_ARG(nms_radius >= 0 && nms_radius <= NNRT_FEATURE_MAX_NMS_RADIUS, "nms_radius must be in [0, 15]");
	NNRT_CHECK_ARG(max_count >= 1 && max_count <= (1 << 20), "max_count must be in [1, 2^20]");
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	NNRT_CHECK_ARG(pixels < (size_t(1) << 31), "height * width must be below 2^31");
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_scores, "null d_scores");
	NNRT_CHECK_ARG(d_out_points, "null d_out_points");
	const size_t out_bytes = sizeof(float) * 2 * static_cast<size_t>(max_count);
	NNRT_CHECK_ARG(!ranges_overlap(d_scores, sizeof(float) * pixels, d_out_points, out_bytes) &&
	                   !(d_mask && ranges_overlap(d_mask, pixels, d_out_points, out_bytes)),
	               "d_out_points must not overlap d_scores or d_mask");
	return launch_select_features(d_scores, d_mask, height, width, quality, nms_radius, max_count, d_out_points, h_out_count,
	                              static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_track_features(const float* const* h_pyramid_a, const float* const* h_pyramid_b, const int32_t* h_heights,
                                const int32_t* h_widths, int32_t levels, const float* d_points, const float* d_initial_flow,
                                const float* d_reference_points, int64_t count, int32_t window_radius, int32_t max_iterations, float epsilon,
                                float min_eigen_threshold, float max_residual, float forward_backward_threshold, float* d_out_points,
                                uint8_t* d_out_status, float* d_out_residual, void* stream) {
	NNRT_CHECK_ARG(count >= 0 && count < (int64_t(1) << 29), "count must be in [0, 2^29)");
	NNRT_CHECK_ARG(levels >= 1 && levels <= NNRT_FEATURE_MAX_LEVELS, "levels must be in [1, 4]");
	NNRT_CHECK_ARG(window_radius >= 1 && window_radius <= NNRT_FEATURE_MAX_WINDOW_RADIUS, "window_radius must be in [1, 7]");
	NNRT_CHECK_ARG(max_iterations >= 1 && max_iterations <= NNRT_FEATURE_MAX_ITERATIONS, "max_iterations must be in [1, 30]");
	NNRT_CHECK_ARG(std::isfinite(epsilon) && epsilon >= 0.f, "epsilon must be finite and >= 0");
	NNRT_CHECK_ARG(std::isfinite(min_eigen_threshold) && min_eigen_threshold >= 0.f, "min_eigen_threshold must be finite and >= 0");
	NNRT_CHECK_ARG(!std::isnan(max_residual), "max_residual is NaN");
	NNRT_CHECK_ARG(!std::isnan(forward_backward_threshold), "forward_backward_threshold is NaN");
	NNRT_CHECK_ARG(!d_reference_points || (std::isfinite(forward_backward_threshold) && forward_backward_threshold >= 0.f),
	               "forward_backward_threshold must be finite and >= 0 with reference points");
	if (count == 0) return NNRT_OK;
	NNRT_CHECK_ARG(h_pyramid_a && h_pyramid_b && h_heights && h_widths, "null pyramid arrays");
	for (int l = 0; l < levels; l++) {
		NNRT_CHECK_ARG(h_heights[l] >= 1 && h_widths[l] >= 1, "pyramid level " + std::to_string(l) + ": height and width must be positive");
		NNRT_CHECK_ARG(static_cast<int64_t>(h_heights[l]) * h_widths[l] < (int64_t(1) << 31),
		               "pyramid level " + std::to_string(l) + ": height * width must be below 2^31");
		NNRT_CHECK_ARG(l == 0 || (h_heights[l] == (h_heights[l - 1] + 1) / 2 && h_widths[l] == (h_widths[l - 1] + 1) / 2),
		               "pyramid level " + std::to_string(l) + ": its size is not ceil(half) of the level below");
		NNRT_CHECK_ARG(h_pyramid_a[l] && h_pyramid_b[l], "pyramid level " + std::to_string(l) + ": null image");
	}
	NNRT_CHECK_ARG(d_points, "null d_points");
	NNRT_CHECK_ARG(d_out_points && d_out_status && d_out_residual, "null output");
	const size_t n = static_cast<size_t>(count), point_bytes = sizeof(float) * 2 * n;
	const struct {
		const void* p;
		size_t bytes;
	} outs[3] = {{d_out_points, point_bytes}, {d_out_status, n}, {d_out_residual, sizeof(float) * n}};
	for (int i = 0; i < 3; i++) {
		for (int j = i + 1; j < 3; j++)
			NNRT_CHECK_ARG(!ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes), "the outputs must not overlap one another");
		NNRT_CHECK_ARG(!ranges_overlap(outs[i].p, outs[i].bytes, d_points, point_bytes) &&
		                   !(d_initial_flow && ranges_overlap(outs[i].p, outs[i].bytes, d_initial_flow, point_bytes)) &&
		                   !(d_reference_points && ranges_overlap(outs[i].p, outs[i].bytes, d_reference_points, point_bytes)),
		               "an output must not overlap d_points, d_initial_flow or d_reference_points");
		for (int l = 0; l < levels; l++) {
			const size_t level_bytes = sizeof(float) * static_cast<size_t>(h_heights[l]) * static_cast<size_t>(h_widths[l]);
			NNRT_CHECK_ARG(!ranges_overlap(outs[i].p, outs[i].bytes, h_pyramid_a[l], level_bytes) &&
			                   !ranges_overlap(outs[i].p, outs[i].bytes, h_pyramid_b[l], level_bytes),
			               "an output must not overlap a pyramid level");
		}
	}
	return launch_track_features(h_pyramid_a, h_pyramid_b, h_heights, h_widths, levels, d_points, d_initial_flow, d_reference_points,
	                             static_cast<int>(count), window_radius, max_iterations, epsilon, min_eigen_threshold, max_residual,
	                             forward_backward_threshold, d_out_points, d_out_status, d_out_residual, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_compute_anchors_and_weights(const float* d_points, int64_t V, const float* d_nodes, int32_t N, int32_t K, float coverage,
                                             const float* d_node_weights, int32_t minimum_valid, int32_t* d_anchors, float* d_weights,
                                             void* stream) {
	NNRT_CHECK_ARG(minimum_valid <= K, "minimum_valid_anchor_count has to be <= anchor_count (WarpAnchorComputation.cpp:92-95)");
	return launch_compute_anchors(d_points, V, d_nodes, N, K, coverage, d_node_weights, minimum_valid, d_anchors, d_weights,
	                              static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_warp_mesh(const float* d_vertices, const float* d_normals, int64_t V, const float* d_nodes, const float* d_rotations,
                           const float* d_translations, int32_t N, const int32_t* d_anchors, const float* d_weights, int32_t K,
                           const double* h_E, float* d_out_vertices, float* d_out_normals, void* stream) {
	NNRT_CHECK_ARG(d_vertices && d_normals && d_nodes && d_anchors && d_weights && d_out_vertices && d_out_normals, "null pointer");
	hipStream_t s = static_cast<hipStream_t>(stream);
	StreamScratch<float> state;
	StreamScratch<float4> wp, wn;
	nnrt_status st;
	if ((st = state.alloc(static_cast<size_t>(NODE_STRIDE) * std::max(N, 1), s)) || (st = wp.alloc(std::max<int64_t>(V, 1), s)) ||
	    (st = wn.alloc(std::max<int64_t>(V, 1), s)))
		return st;
	st = launch_pack_nodes(d_nodes, d_rotations, d_translations, N, state.ptr, s);
	if (!st) st = launch_warp_mesh(d_vertices, d_normals, V, state.ptr, d_anchors, d_weights, K, make_extrinsics(h_E), wp.ptr, wn.ptr, nullptr,
	                              choose_warp_vertex(read_launch_switches(), V), s);
	if (!st) st = launch_unpack_float4x3(wp.ptr, V, d_out_vertices, s);
	if (!st) st = launch_unpack_float4x3(wn.ptr, V, d_out_normals, s);
	return st;
}

nnrt_status nnrt_warp_points(const float* d_points, const float* d_normals, int64_t V, const float* d_nodes, const float* d_rotations,
                             const float* d_translations, int32_t N, const int32_t* d_anchors, const float* d_weights, int32_t K, float coverage,
                             int32_t threshold, int32_t minimum_valid, const double* h_E, float* d_out_points, float* d_out_normals,
                             void* stream) {
	NNRT_CHECK_ARG((d_points && d_nodes && d_rotations && d_translations && d_out_points) || V == 0, "null pointer");
	NNRT_CHECK_ARG(!d_normals == !d_out_normals, "normals in and out must both be given or both be NULL");
	NNRT_CHECK_ARG(K >= 1 && K <= MAX_ANCHORS, "anchor_count needs to satisfy 0 < anchor_count <= 8 (Warping.cpp:70-75)");
	NNRT_CHECK_ARG(minimum_valid >= 0 && minimum_valid <= K,
	               "minimum_valid_anchor_count is required to satisfy 0 <= minimum_valid_anchor_count <= anchor_count (Warping.cpp:76-79)");
	NNRT_CHECK_ARG(!d_anchors == !d_weights, "anchors and anchor_weights must both be given");
	if (V == 0) return NNRT_OK;
	hipStream_t s = static_cast<hipStream_t>(stream);
	StreamScratch<float> state, weights;
	StreamScratch<int32_t> anchors;
	nnrt_status st = state.alloc(static_cast<size_t>(NODE_STRIDE) * std::max(N, 1), s);
	if (st) return st;
	st = launch_pack_nodes(d_nodes, d_rotations, d_translations, N, state.ptr, s);
	const int32_t* a = d_anchors;
	const float* w = d_weights;
	if (!st && !d_anchors) {   // online anchors: FindAnchorsAndWeightsForPoint_Euclidean[_Threshold]_FixedNodeCoverageWeight
		if ((st = anchors.alloc(static_cast<size_t>(V) * K, s)) || (st = weights.alloc(static_cast<size_t>(V) * K, s))) return st;
		st = launch_compute_anchors(d_points, V, d_nodes, N, K, coverage, nullptr, minimum_valid, anchors.ptr, weights.ptr, s, threshold ? 1 : 0);
		a = anchors.ptr;
		w = weights.ptr;
	}
	if (!st) st = launch_warp_points(d_points, d_normals, V, state.ptr, a, w, K, threshold ? minimum_valid : -1, make_extrinsics(h_E), d_out_points,
	                                 d_out_normals, s);
	return st;
}

nnrt_status nnrt_compute_point_to_plane_distances(const float* d_normals1, const float* d_vertices1, const float* d_vertices2, int64_t count,
                                                  float* d_out, void* stream) {
	NNRT_CHECK_ARG((d_normals1 && d_vertices1 && d_vertices2 && d_out) || count == 0, "null pointer");
	return launch_point_to_plane(d_normals1, d_vertices1, d_vertices2, count, d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_get_meshes_ndc_face_vertices_and_clip_mask(const float* const* h_vertex_sets, const int64_t* const* h_face_sets,
                                                            const int64_t* h_face_counts, int32_t mesh_count, const double* h_K, int32_t H,
                                                            int32_t W, float near_clip, float far_clip, float* d_face_ndc, uint8_t* d_clip_mask,
                                                            void* stream) {
	return nnrt_get_meshes_ndc_face_vertices_and_clip_mask_in_convention(h_vertex_sets, h_face_sets, h_face_counts, mesh_count, h_K, H, W, near_clip,
	                                                                     far_clip, NNRT_NDC_REFERENCE, d_face_ndc, d_clip_mask, stream);
}

nnrt_status nnrt_get_meshes_ndc_face_vertices_and_clip_mask_in_convention(const float* const* h_vertex_sets, const int64_t* const* h_face_sets,
                                                                          const int64_t* h_face_counts, int32_t mesh_count, const double* h_K,
                                                                          int32_t H, int32_t W, float near_clip, float far_clip,
                                                                          int32_t ndc_convention, float* d_face_ndc, uint8_t* d_clip_mask,
                                                                          void* stream) {
	NNRT_CHECK_ARG(h_K && h_vertex_sets && h_face_sets && h_face_counts && mesh_count >= 0, "null pointer");
	NNRT_CHECK_ARG(near_clip >= 0.f, "near_clipping_distance cannot be less than 0 (ExtractFaceVertices.cpp:40-44)");
	NNRT_CHECK_ARG(near_clip <= far_clip, "near_clipping_distance cannot be greater than far_clipping_distance");
	NNRT_CHECK_ARG(ndc_convention == NNRT_NDC_REFERENCE || ndc_convention == NNRT_NDC_CONSISTENT, "unknown ndc_convention");
	const NdcSetup ndc = make_ndc_setup(h_K, H, W, ndc_convention == NNRT_NDC_CONSISTENT);
	int64_t offset = 0;
	for (int m = 0; m < mesh_count; m++) {   // face f of mesh m -> output row offset(m) + f (ExtractClippedFaceVerticesImpl.h:111-116)
		const int64_t F = h_face_counts[m];
		NNRT_CHECK_ARG(F >= 0 && (F == 0 || (h_vertex_sets[m] && h_face_sets[m])), "mesh needs both triangle indices and vertex positions");
		nnrt_status st = launch_extract_face_ndc(h_vertex_sets[m], h_face_sets[m], F, ndc, near_clip, far_clip, d_face_ndc + 9 * offset,
		                                         d_clip_mask + offset, static_cast<hipStream_t>(stream));
		if (st) return st;
		offset += F;
	}
	return NNRT_OK;
}

nnrt_status nnrt_get_mesh_ndc_face_vertices_and_clip_mask(const float* d_vertices, const int64_t* d_faces, int64_t F, const double* h_K, int32_t H,
                                                          int32_t W, float near_clip, float far_clip, float* d_face_ndc, uint8_t* d_clip_mask,
                                                          void* stream) {
	NNRT_CHECK_ARG(h_K && d_vertices && d_faces && d_face_ndc && d_clip_mask, "null pointer");
	NNRT_CHECK_ARG(near_clip >= 0.f, "near_clipping_distance cannot be less than 0 (ExtractFaceVertices.cpp:40-44)");
	NNRT_CHECK_ARG(near_clip <= far_clip, "near_clipping_distance cannot be greater than far_clipping_distance");
	return launch_extract_face_ndc(d_vertices, d_faces, F, make_ndc_setup(h_K, H, W, false), near_clip, far_clip, d_face_ndc, d_clip_mask,
	                               static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_rasterize_ndc_triangles(const float* d_face_ndc, const uint8_t* d_clip_mask, int64_t F, int32_t H, int32_t W,
                                         float blur_radius_pixels, int32_t faces_per_pixel, int32_t bin_size, int32_t max_faces_per_bin,
                                         int32_t perspective, int32_t clip_barycentric, int32_t cull_back_faces, int64_t* d_faces_out,
                                         float* d_depth_out, float* d_bary_out, float* d_dist_out, void* stream) {
	(void) max_faces_per_bin;
	NNRT_CHECK_ARG(H > 0 && W > 0, "image_size must be positive");
	if (faces_per_pixel > MAX_FACES_PER_PIXEL || faces_per_pixel < 1) {
		set_error("Need faces_per_pixel <= 8 (RasterizeNdcTriangles.cpp:45-47)");
		return NNRT_ERROR_ARGUMENT;
	}
	// bin-size validation kept for error parity (RasterizeNdcTriangles.cpp:53-76); bins themselves are not needed here
	const int max_dim = std::max(H, W);
	if (bin_size == -1) bin_size = max_dim <= 64 ? 8 : static_cast<int>(std::pow(2, std::max(static_cast<int>(std::ceil(std::log2(static_cast<double>(max_dim)))) - 4, 4)));
	if (bin_size != 0 && 1 + (max_dim - 1) / bin_size >= 22) {
		set_error("The provided bin_size is too small (RasterizeNdcTriangles.cpp:70-76)");
		return NNRT_ERROR_ARGUMENT;
	}
	hipStream_t s = static_cast<hipStream_t>(stream);
	const RasterOptions o = make_raster_options(H, W, blur_radius_pixels / (static_cast<float>(fminf(H, W)) / 2.0f), perspective, clip_barycentric, cull_back_faces);
	if (faces_per_pixel == 1) {
		const int64_t P = static_cast<int64_t>(H) * W;
		StreamScratch<uint64_t> keys;
		nnrt_status st = keys.alloc(static_cast<size_t>(P), s);
		if (st) return st;
		NNRT_HIP(hipMemsetAsync(keys.ptr, 0xff, sizeof(uint64_t) * P, s));
		st = launch_raster_scatter_ndc(d_face_ndc, d_clip_mask, F, o, keys.ptr, s);
		if (!st) st = launch_raster_resolve(d_face_ndc, F, o, keys.ptr, d_faces_out, d_depth_out, d_bary_out, d_dist_out, s);
		return st;
	}
	return launch_raster_multi(d_face_ndc, d_clip_mask, F, o, faces_per_pixel, d_faces_out, d_depth_out, d_bary_out, d_dist_out, s);
}

nnrt_status nnrt_interpolate_face_attributes(const int64_t* d_pixel_faces, const float* d_bary, int64_t P, int32_t Kf, const float* d_attrs,
                                             int32_t C, float* d_out, void* stream) {
	return launch_interpolate(d_pixel_faces, d_bary, P, Kf, d_attrs, C, d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_unproject_depth(const float* d_depth, int32_t H, int32_t W, const double* h_K, float depth_scale, float depth_max,
                                 float* d_points, uint8_t* d_mask, void* stream) {
	NNRT_CHECK_ARG(h_K, "null intrinsics");
	return launch_unproject(d_depth, NNRT_DTYPE_FLOAT32, H, W, pixel_camera(h_K), make_extrinsics(nullptr), depth_scale, depth_max, d_points,
	                        d_mask, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_unproject_depth_image(const void* d_depth, int32_t depth_dtype, int32_t H, int32_t W, const double* h_K, const double* h_E,
                                       float depth_scale, float depth_max, float* d_points, uint8_t* d_mask, void* stream) {
	NNRT_CHECK_ARG(h_K, "null intrinsics");
	NNRT_CHECK_ARG(depth_dtype == NNRT_DTYPE_UINT16 || depth_dtype == NNRT_DTYPE_FLOAT32, "depth must be uint16 or float32");
	NNRT_CHECK_ARG(H >= 0 && W >= 0, "negative image size");
	NNRT_CHECK_ARG((d_depth && d_points && d_mask) || static_cast<int64_t>(H) * W == 0, "null pointer");
	double pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
	if (h_E) {   // Open3D InverseTransformation: [R^T | -R^T t], computed in double, rounded once into TransformIndexer's floats
		for (int r = 0; r < 3; r++) {
			double tr = 0.0;
			for (int c = 0; c < 3; c++) {
				pose[4 * r + c] = h_E[4 * c + r];
				tr += h_E[4 * c + r] * h_E[4 * c + 3];
			}
			pose[4 * r + 3] = -tr;
		}
	}
	return launch_unproject(d_depth, depth_dtype, H, W, pixel_camera(h_K), make_extrinsics(h_E ? pose : nullptr), depth_scale, depth_max,
	                        d_points, d_mask, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_backproject_depth_ushort(const uint16_t* d_depth, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                                          float normalizer, float* d_points, void* stream) {
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative image size");
	NNRT_CHECK_ARG((d_depth && d_points) || height * static_cast<int64_t>(width) == 0, "null image");
	return launch_backproject_depth_u16(d_depth, height, width, BackprojectCamera{fx, fy, cx, cy, normalizer}, d_points,
	                                    static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_backproject_depth_float(const float* d_depth, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                                         float* d_points, void* stream) {
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative image size");
	NNRT_CHECK_ARG((d_depth && d_points) || height * static_cast<int64_t>(width) == 0, "null image");
	return launch_backproject_depth_f32(d_depth, height, width, BackprojectCamera{fx, fy, cx, cy, 1.0f}, d_points,
	                                    static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_filter_depth(const uint16_t* d_in, int32_t height, int32_t width, int32_t radius, int32_t preserve_zero, uint16_t* d_out,
                              void* stream) {
	NNRT_CHECK_ARG(radius >= 0 && radius <= NNRT_DEPTH_FILTER_MAX_RADIUS, "radius must be in [0, 8]");
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	if (height * static_cast<int64_t>(width) == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_in, "null d_in");
	NNRT_CHECK_ARG(d_out, "null d_out");
	NNRT_CHECK_ARG(d_out != d_in, "d_out must not be d_in (the filter reads every pixel's neighbours)");
	return launch_filter_depth_median(d_in, height, width, radius, preserve_zero != 0, d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_bilateral_filter_depth(const void* d_in, int32_t in_dtype, int32_t height, int32_t width, int32_t radius,
                                        const float* h_spatial_weights, const float* h_range_weights, int32_t range_weight_count,
                                        float range_index_scale, float depth_scale, float* d_out, void* stream) {
	NNRT_CHECK_ARG(in_dtype == NNRT_DTYPE_UINT16 || in_dtype == NNRT_DTYPE_FLOAT32, "in_dtype must be uint16 or float32");
	NNRT_CHECK_ARG(radius >= 0 && radius <= NNRT_DEPTH_FILTER_MAX_RADIUS, "radius must be in [0, 8]");
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(range_weight_count >= 1 && range_weight_count <= NNRT_BILATERAL_MAX_RANGE_WEIGHTS, "range_weight_count must be in [1, 4096]");
	NNRT_CHECK_ARG(std::isfinite(range_index_scale) && range_index_scale > 0.f, "range_index_scale must be finite and positive");
	NNRT_CHECK_ARG(std::isfinite(depth_scale) && depth_scale > 0.f, "depth_scale must be finite and positive");
	NNRT_CHECK_ARG(h_spatial_weights, "null h_spatial_weights");
	NNRT_CHECK_ARG(h_range_weights, "null h_range_weights");
	const int spatial_count = (2 * radius + 1) * (2 * radius + 1);
	for (int i = 0; i < spatial_count; i++) {
		NNRT_CHECK_ARG(std::isfinite(h_spatial_weights[i]) && h_spatial_weights[i] >= 0.f, "h_spatial_weights holds a negative or non-finite entry");
	}
	for (int i = 0; i < range_weight_count; i++) {
		NNRT_CHECK_ARG(std::isfinite(h_range_weights[i]) && h_range_weights[i] >= 0.f, "h_range_weights holds a negative or non-finite entry");
	}
	if (height * static_cast<int64_t>(width) == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_in, "null d_in");
	NNRT_CHECK_ARG(d_out, "null d_out");
	NNRT_CHECK_ARG(static_cast<const void*>(d_out) != d_in, "d_out must not be d_in (the filter reads every pixel's neighbours)");
	hipStream_t s = static_cast<hipStream_t>(stream);
	StreamScratch<float> tables;   // spatial, then range
	if (nnrt_status st = tables.alloc(static_cast<size_t>(spatial_count) + range_weight_count, s)) return st;
	NNRT_HIP(hipMemcpyAsync(tables.ptr, h_spatial_weights, sizeof(float) * spatial_count, hipMemcpyHostToDevice, s));
	NNRT_HIP(hipMemcpyAsync(tables.ptr + spatial_count, h_range_weights, sizeof(float) * range_weight_count, hipMemcpyHostToDevice, s));
	return launch_filter_depth_bilateral(d_in, in_dtype, height, width, radius, tables.ptr, tables.ptr + spatial_count, range_weight_count,
	                                     range_index_scale, depth_scale, d_out, s);
}

nnrt_status nnrt_shade_pixels(int32_t mode, const int64_t* d_pixel_face_indices, const float* d_pixel_barycentric_coordinates,
                              const float* d_pixel_face_distances, int32_t height, int32_t width, int32_t faces_per_pixel,
                              const int64_t* d_triangle_indices, int64_t face_count, const float* d_vertex_colors,
                              const float* d_vertex_normals, int64_t vertex_count, const float* h_color, float pixel_line_width,
                              float ambient, uint8_t* d_out_pixels, void* stream) {
	NNRT_CHECK_ARG(mode == NNRT_SHADE_VERTEX_COLOR || mode == NNRT_SHADE_FLAT_EDGE || mode == NNRT_SHADE_HEADLIGHT,
	               "mode must be NNRT_SHADE_VERTEX_COLOR, NNRT_SHADE_FLAT_EDGE or NNRT_SHADE_HEADLIGHT");
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(faces_per_pixel >= 1, "faces_per_pixel must be at least 1");
	NNRT_CHECK_ARG(face_count >= 0, "negative face_count");
	NNRT_CHECK_ARG(vertex_count >= 0, "negative vertex_count");
	const bool flat = mode == NNRT_SHADE_FLAT_EDGE;
	if (flat) NNRT_CHECK_ARG(pixel_line_width > 0.f, "pixel_line_width must be positive");
	if (mode == NNRT_SHADE_HEADLIGHT) NNRT_CHECK_ARG(ambient >= 0.f && ambient <= 1.f, "ambient must be in [0, 1]");
	if (mode != NNRT_SHADE_VERTEX_COLOR) NNRT_CHECK_ARG(h_color, "null h_color");
	if (mode == NNRT_SHADE_VERTEX_COLOR) NNRT_CHECK_ARG(d_vertex_colors || vertex_count == 0, "null d_vertex_colors (NNRT_SHADE_VERTEX_COLOR reads them)");
	if (mode == NNRT_SHADE_HEADLIGHT) NNRT_CHECK_ARG(d_vertex_normals || vertex_count == 0, "null d_vertex_normals (NNRT_SHADE_HEADLIGHT reads them)");
	if (!flat) NNRT_CHECK_ARG(d_triangle_indices || face_count == 0, "null d_triangle_indices");
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_pixel_face_indices, "null d_pixel_face_indices");
	if (flat) NNRT_CHECK_ARG(d_pixel_face_distances, "null d_pixel_face_distances");
	if (!flat) NNRT_CHECK_ARG(d_pixel_barycentric_coordinates, "null d_pixel_barycentric_coordinates");
	NNRT_CHECK_ARG(d_out_pixels, "null d_out_pixels");
	const size_t fragments = pixels * static_cast<size_t>(faces_per_pixel), out_bytes = 3 * pixels;
	const size_t nf = static_cast<size_t>(face_count), nv = static_cast<size_t>(vertex_count);
	NNRT_CHECK_ARG(!(ranges_overlap(d_out_pixels, out_bytes, d_pixel_face_indices, sizeof(int64_t) * fragments) ||
	                 ranges_overlap(d_out_pixels, out_bytes, d_pixel_barycentric_coordinates, sizeof(float) * 3 * fragments) ||
	                 ranges_overlap(d_out_pixels, out_bytes, d_pixel_face_distances, sizeof(float) * fragments) ||
	                 ranges_overlap(d_out_pixels, out_bytes, d_triangle_indices, sizeof(int64_t) * 3 * nf) ||
	                 ranges_overlap(d_out_pixels, out_bytes, d_vertex_colors, sizeof(float) * 3 * nv) ||
	                 ranges_overlap(d_out_pixels, out_bytes, d_vertex_normals, sizeof(float) * 3 * nv)),
	               "d_out_pixels must not overlap an input");
	const float ndc_line_width = flat ? pixel_line_width / (static_cast<float>(std::min(height, width)) / 2.0f) : 0.f;
	return launch_shade_pixels(mode, d_pixel_face_indices, d_pixel_barycentric_coordinates, d_pixel_face_distances, height, width,
	                           faces_per_pixel, d_triangle_indices, face_count, d_vertex_colors, d_vertex_normals, vertex_count, h_color,
	                           ndc_line_width, ambient, d_out_pixels, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_compare_depth_to_raster(const int64_t* d_pixel_face_indices, const float* d_pixel_depths, int32_t height, int32_t width,
                                         int32_t faces_per_pixel, const void* d_depth, int32_t depth_dtype, float depth_scale,
                                         float depth_max, float inlier_threshold, float* d_out_difference,
                                         nnrt_depth_agreement* h_out_statistics, void* stream) {
	NNRT_CHECK_ARG(h_out_statistics, "null h_out_statistics");
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(faces_per_pixel >= 1, "faces_per_pixel must be at least 1");
	NNRT_CHECK_ARG(depth_dtype == NNRT_DTYPE_UINT16 || depth_dtype == NNRT_DTYPE_FLOAT32, "depth_dtype must be uint16 or float32");
	NNRT_CHECK_ARG(std::isfinite(depth_scale) && depth_scale > 0.f, "depth_scale must be finite and positive");
	NNRT_CHECK_ARG(!std::isnan(depth_max), "depth_max must not be NaN");
	NNRT_CHECK_ARG(inlier_threshold >= 0.f, "inlier_threshold must not be negative or NaN");
	std::memset(h_out_statistics, 0, sizeof(*h_out_statistics));
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_pixel_face_indices, "null d_pixel_face_indices");
	NNRT_CHECK_ARG(d_pixel_depths, "null d_pixel_depths");
	NNRT_CHECK_ARG(d_depth, "null d_depth");
	NNRT_CHECK_ARG(d_out_difference, "null d_out_difference");
	const size_t fragments = pixels * static_cast<size_t>(faces_per_pixel), out_bytes = sizeof(float) * pixels;
	NNRT_CHECK_ARG(!(ranges_overlap(d_out_difference, out_bytes, d_pixel_face_indices, sizeof(int64_t) * fragments) ||
	                 ranges_overlap(d_out_difference, out_bytes, d_pixel_depths, sizeof(float) * fragments) ||
	                 ranges_overlap(d_out_difference, out_bytes, d_depth, (depth_dtype == NNRT_DTYPE_UINT16 ? 2 : 4) * pixels)),
	               "d_out_difference must not overlap an input");
	hipStream_t s = static_cast<hipStream_t>(stream);
	const size_t groups = static_cast<size_t>(depth_agreement_partial_count(height, width));
	StreamScratch<nnrt_depth_agreement> records;   // one per workgroup, then the total
	if (nnrt_status st = records.alloc(groups + 1, s)) return st;
	if (nnrt_status st = launch_depth_agreement(d_pixel_face_indices, d_pixel_depths, height, width, faces_per_pixel, d_depth, depth_dtype,
	                                            depth_scale, depth_max, inlier_threshold, d_out_difference, records.ptr,
	                                            records.ptr + groups, s))
		return st;
	NNRT_HIP(hipMemcpyAsync(h_out_statistics, records.ptr + groups, sizeof(*h_out_statistics), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	return NNRT_OK;
}

nnrt_status nnrt_motion_pixels(const int64_t* d_pixel_face_indices, const float* d_pixel_barycentric_coordinates, int32_t height,
                               int32_t width, int32_t faces_per_pixel, const int64_t* d_triangle_indices, int64_t face_count,
                               const float* d_source_positions, const float* d_target_positions, int64_t vertex_count, float fx, float fy,
                               float cx, float cy, float* d_out_source_points, float* d_out_scene_flow, float* d_out_optical_flow,
                               uint8_t* d_out_mask, void* stream) {
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(faces_per_pixel >= 1, "faces_per_pixel must be at least 1");
	NNRT_CHECK_ARG(face_count >= 0, "negative face_count");
	NNRT_CHECK_ARG(vertex_count >= 0, "negative vertex_count");
	NNRT_CHECK_ARG(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy), "fx, fy, cx and cy must be finite");
	NNRT_CHECK_ARG(d_triangle_indices || face_count == 0, "null d_triangle_indices");
	NNRT_CHECK_ARG(d_source_positions || vertex_count == 0, "null d_source_positions");
	NNRT_CHECK_ARG(d_target_positions || vertex_count == 0, "null d_target_positions");
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_pixel_face_indices, "null d_pixel_face_indices");
	NNRT_CHECK_ARG(d_pixel_barycentric_coordinates, "null d_pixel_barycentric_coordinates");
	NNRT_CHECK_ARG(d_out_source_points, "null d_out_source_points");
	NNRT_CHECK_ARG(d_out_scene_flow, "null d_out_scene_flow");
	NNRT_CHECK_ARG(d_out_optical_flow, "null d_out_optical_flow");
	NNRT_CHECK_ARG(d_out_mask, "null d_out_mask");
	const size_t fragments = pixels * static_cast<size_t>(faces_per_pixel);
	const size_t nf = static_cast<size_t>(face_count), nv = static_cast<size_t>(vertex_count);
	const void* outputs[4] = {d_out_source_points, d_out_scene_flow, d_out_optical_flow, d_out_mask};
	const size_t output_bytes[4] = {sizeof(float) * 3 * pixels, sizeof(float) * 3 * pixels, sizeof(float) * 2 * pixels, pixels};
	for (int i = 0; i < 4; i++) {
		NNRT_CHECK_ARG(!(ranges_overlap(outputs[i], output_bytes[i], d_pixel_face_indices, sizeof(int64_t) * fragments) ||
		                 ranges_overlap(outputs[i], output_bytes[i], d_pixel_barycentric_coordinates, sizeof(float) * 3 * fragments) ||
		                 ranges_overlap(outputs[i], output_bytes[i], d_triangle_indices, sizeof(int64_t) * 3 * nf) ||
		                 ranges_overlap(outputs[i], output_bytes[i], d_source_positions, sizeof(float) * 3 * nv) ||
		                 ranges_overlap(outputs[i], output_bytes[i], d_target_positions, sizeof(float) * 3 * nv)),
		               "an output must not overlap an input");
		for (int j = 0; j < i; j++)
			NNRT_CHECK_ARG(!ranges_overlap(outputs[i], output_bytes[i], outputs[j], output_bytes[j]), "the outputs must not overlap each other");
	}
	return launch_motion_pixels(d_pixel_face_indices, d_pixel_barycentric_coordinates, height, width, faces_per_pixel, d_triangle_indices,
	                            face_count, d_source_positions, d_target_positions, vertex_count, fx, fy, cx, cy, d_out_source_points,
	                            d_out_scene_flow, d_out_optical_flow, d_out_mask, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_flow_error(const float* d_predicted, const uint8_t* d_predicted_mask, const float* d_truth, const uint8_t* d_truth_mask,
                            int32_t height, int32_t width, int32_t channels, float inlier_threshold, float* d_out_error,
                            nnrt_flow_agreement* h_out_statistics, void* stream) {
	NNRT_CHECK_ARG(h_out_statistics, "null h_out_statistics");
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative height or width");
	NNRT_CHECK_ARG(channels == 2 || channels == 3, "channels must be 2 or 3");
	NNRT_CHECK_ARG(inlier_threshold >= 0.f, "inlier_threshold must not be negative or NaN");
	std::memset(h_out_statistics, 0, sizeof(*h_out_statistics));
	const size_t pixels = static_cast<size_t>(height) * static_cast<size_t>(width);
	if (pixels == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_predicted, "null d_predicted");
	NNRT_CHECK_ARG(d_predicted_mask, "null d_predicted_mask");
	NNRT_CHECK_ARG(d_truth, "null d_truth");
	NNRT_CHECK_ARG(d_out_error, "null d_out_error");
	const size_t out_bytes = sizeof(float) * pixels, flow_bytes = sizeof(float) * channels * pixels;
	NNRT_CHECK_ARG(!(ranges_overlap(d_out_error, out_bytes, d_predicted, flow_bytes) || ranges_overlap(d_out_error, out_bytes, d_truth, flow_bytes) ||
	                 ranges_overlap(d_out_error, out_bytes, d_predicted_mask, pixels) ||
	                 (d_truth_mask && ranges_overlap(d_out_error, out_bytes, d_truth_mask, pixels))),
	               "d_out_error must not overlap an input");
	hipStream_t s = static_cast<hipStream_t>(stream);
	const size_t groups = static_cast<size_t>(flow_error_partial_count(height, width));
	StreamScratch<nnrt_flow_agreement> records;   // one per workgroup, then the total
	if (nnrt_status st = records.alloc(groups + 1, s)) return st;
	if (nnrt_status st = launch_flow_error(d_predicted, d_predicted_mask, d_truth, d_truth_mask, height, width, channels, inlier_threshold,
	                                       d_out_error, records.ptr, records.ptr + groups, s))
		return st;
	NNRT_HIP(hipMemcpyAsync(h_out_statistics, records.ptr + groups, sizeof(*h_out_statistics), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	return NNRT_OK;
}

nnrt_status nnrt_matmul3d(const float* d_a,const float* d_b, int64_t batch, int32_t m, int32_t k, int32_t n, float* d_c, void* stream) {
	NNRT_CHECK_ARG(batch >= 0 && m >= 0 && k >= 0 && n >= 0, "negative dimension");
	NNRT_CHECK_ARG((d_a && d_b && d_c) || batch * m * n == 0, "null pointer");
	return launch_matmul3d(d_a, d_b, batch, m, k, n, d_c, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_median_grid_subsample_3d_points(const float* d_points, int64_t n, float cell, int64_t* d_out, int64_t* h_count, void* stream) {
	NNRT_CHECK_ARG(h_count && (n == 0 || (d_points && d_out)), "null pointer");
	NNRT_CHECK_ARG(n >= 0 && n < (int64_t(1) << 31), "point count out of range");
	NNRT_CHECK_ARG(cell > 0.f, "grid_cell_size must be positive");
	return launch_median_grid_subsample(d_points, static_cast<int>(n), cell, d_out, h_count, static_cast<hipStream_t>(stream));
}

// shared argument checks of the grid functions over the cell index (spatial_grid.hip)
static nnrt_status check_grid_arguments(const void* d_points, int64_t n, float cell, float ox, float oy, float oz, const void* d_out,
                                        const int64_t* h_count) {
	NNRT_CHECK_ARG(h_count, "null h_cell_count");
	NNRT_CHECK_ARG(n >= 0 && n < (int64_t(1) << 31) / 3, "point count out of range");
	NNRT_CHECK_ARG(cell > 0.f && std::isfinite(cell), "grid_cell_size must be positive and finite");
	NNRT_CHECK_ARG(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), "the grid offset must be finite");
	NNRT_CHECK_ARG(n == 0 || d_points, "null d_points");
	NNRT_CHECK_ARG(n == 0 || d_out, "null output");
	return NNRT_OK;
}

nnrt_status nnrt_mean_grid_downsample_3d_points(const float* d_points, int64_t n, float cell, float ox, float oy, float oz, float* d_out,
                                                int64_t* h_count, void* stream) {
	if (nnrt_status st = check_grid_arguments(d_points, n, cell, ox, oy, oz, d_out, h_count)) return st;
	const float offset[3] = {ox, oy, oz};
	return launch_mean_grid_downsample(d_points, static_cast<int>(n), cell, offset, d_out, h_count, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_closest_to_mean_grid_subsample_3d_points(const float* d_points, int64_t n, float cell, float ox, float oy, float oz,
                                                          int64_t* d_out, int64_t* h_count, void* stream) {
	if (nnrt_status st = check_grid_arguments(d_points, n, cell, ox, oy, oz, d_out, h_count)) return st;
	const float offset[3] = {ox, oy, oz};
	return launch_closest_to_mean_grid_subsample(d_points, static_cast<int>(n), cell, offset, d_out, h_count, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_median_grid_subsample_3d_points_binned(const float* d_points, int64_t n, float cell, float ox, float oy, float oz, int64_t* d_out,
                                                        int64_t* h_count, void* stream) {
	if (nnrt_status st = check_grid_arguments(d_points, n, cell, ox, oy, oz, d_out, h_count)) return st;
	const float offset[3] = {ox, oy, oz};
	return launch_median_grid_subsample_binned(d_points, static_cast<int>(n), cell, offset, d_out, h_count, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_point_index_create(const float* d_points, int64_t point_count, int32_t dimension_count, void* stream, nnrt_point_index** out) {
	NNRT_CHECK_ARG(out, "null output");
	*out = nullptr;
	NNRT_CHECK_ARG(dimension_count == 3, "points must be [point_count, 3]: only 3-D points are indexed");
	NNRT_CHECK_ARG(point_count >= 1 && point_count < (int64_t(1) << 31) / 3, "point_count must be at least 1 (and below 2^31 / 3)");
	NNRT_CHECK_ARG(d_points, "null d_points");
	PointIndex* index = nullptr;
	if (nnrt_status st = point_index_create(d_points, static_cast<int>(point_count), static_cast<hipStream_t>(stream), &index)) return st;
	*out = reinterpret_cast<nnrt_point_index*>(index);
	return NNRT_OK;
}

void nnrt_point_index_destroy(nnrt_point_index* index) {
	if (!index) return;
	hipDeviceSynchronize();   // queries still in flight read the index
	point_index_destroy(reinterpret_cast<PointIndex*>(index));
}

nnrt_status nnrt_point_index_get_info(const nnrt_point_index* index, int64_t* h_point_count, float* h_cell_size, int64_t* h_cell_count,
                                      int32_t* h_build_count) {
	NNRT_CHECK_ARG(index, "null index");
	point_index_info(reinterpret_cast<const PointIndex*>(index), h_point_count, h_cell_size, h_cell_count, h_build_count);
	return NNRT_OK;
}

nnrt_status nnrt_point_index_find_k_nearest(const nnrt_point_index* index, const float* d_query_points, int64_t query_count,
                                            int32_t dimension_count, int32_t k, int32_t* d_out_indices, float* d_out_distances, void* stream) {
	NNRT_CHECK_ARG(index, "null index");
	NNRT_CHECK_ARG(dimension_count == 3, "query_points must be [query_count, 3]: only 3-D points are indexed");
	NNRT_CHECK_ARG(k >= 1 && k <= NNRT_POINT_INDEX_MAX_K, "k must be in [1, 16]");
	NNRT_CHECK_ARG(query_count >= 0 && query_count < (int64_t(1) << 31) / NNRT_POINT_INDEX_MAX_K, "query count out of range");
	if (query_count == 0) return NNRT_OK;
	NNRT_CHECK_ARG(d_query_points, "null d_query_points");
	NNRT_CHECK_ARG(d_out_indices, "null d_out_indices");
	NNRT_CHECK_ARG(d_out_distances, "null d_out_distances");
	return point_index_find_k_nearest(reinterpret_cast<const PointIndex*>(index), d_query_points, static_cast<int>(query_count), k, d_out_indices,
	                                  d_out_distances, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_axis_angle_to_matrices_rodrigues(const float* d_vectors, int32_t count, float* d_matrices, void* stream) {
	return launch_rodrigues(d_vectors, count, d_matrices, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_solve_block_diagonal_cholesky(const float* d_blocks, const float* d_b, int32_t count, int32_t block_size, float* d_x,
                                               void* stream) {
	hipStream_t s = static_cast<hipStream_t>(stream);
	StreamScratch<int> flag;
	nnrt_status st = flag.alloc(1, s);
	if (st) return st;
	NNRT_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), s));
	st = launch_solve_block_diagonal(d_blocks, d_b, count, block_size, d_x, flag.ptr, s);
	if (st) return st;
	int host_flag = 0;
	NNRT_HIP(hipMemcpyAsync(&host_flag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (host_flag) {
		set_error("potrf failed in SolveBlockDiagonalCholesky (block not positive-definite)");
		return NNRT_ERROR_NOT_POSITIVE_DEFINITE;
	}
	return NNRT_OK;
}

nnrt_status nnrt_invert_positive_semidefinite_blocks(const float* d_blocks, int32_t count, int32_t block_size, float* d_out, void* stream) {
	hipStream_t s = static_cast<hipStream_t>(stream);
	NNRT_CHECK_ARG(count >= 0, "negative block count");
	StreamScratch<int> flag;
	nnrt_status st = flag.alloc(1, s);
	if (st) return st;
	NNRT_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), s));
	st = launch_invert_psd_blocks(d_blocks, count, block_size, d_out, flag.ptr, s);
	if (st) return st;
	int host_flag = 0;
	NNRT_HIP(hipMemcpyAsync(&host_flag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (host_flag) {
		set_error("potrf failed in InvertPositiveSemidefiniteBlocks (block not positive-definite)");
		return NNRT_ERROR_NOT_POSITIVE_DEFINITE;
	}
	return NNRT_OK;
}

extern "C++" {
// runs launch(flag) on the stream with a zeroed device flag; a raised flag becomes `code` with `message`
template <typename F>
nnrt_status with_device_flag(hipStream_t s, nnrt_status code, const char* message, F&& launch) {
	StreamScratch<int> flag;
	nnrt_status st = flag.alloc(1, s);
	if (st) return st;
	NNRT_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), s));
	st = launch(flag.ptr);
	if (st) return st;
	int host_flag = 0;
	NNRT_HIP(hipMemcpyAsync(&host_flag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (host_flag) {
		set_error(message);
		return code;
	}
	return NNRT_OK;
}
} // extern "C++"

nnrt_status nnrt_get_vertex_erosion_mask(int64_t vertex_count, const int64_t* d_face_indices, int64_t face_count, int32_t iteration_count,
                                         int32_t min_neighbors, uint8_t* d_out_mask, void* stream) {
	NNRT_CHECK_ARG(vertex_count >= 0 && vertex_count < (int64_t(1) << 31), "vertex count out of range");
	NNRT_CHECK_ARG(face_count >= 0 && face_count < (int64_t(1) << 31) / 3, "face count out of range");
	NNRT_CHECK_ARG(iteration_count >= 0, "negative iteration_count");
	NNRT_CHECK_ARG(face_count == 0 || d_face_indices, "null face indices");
	NNRT_CHECK_ARG(vertex_count == 0 || d_out_mask, "null output mask");
	NNRT_CHECK_ARG(vertex_count == 0 || face_count == 0 ||
	                   !ranges_overlap(d_out_mask, static_cast<size_t>(vertex_count), d_face_indices, sizeof(int64_t) * 3 * static_cast<size_t>(face_count)),
	               "d_out_mask must not overlap d_face_indices");
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (vertex_count == 0 && face_count == 0) return NNRT_OK;
	if (face_count == 0) {
		NNRT_HIP(hipMemsetAsync(d_out_mask, 0, static_cast<size_t>(vertex_count), s));
		return NNRT_OK;
	}
	return with_device_flag(s, NNRT_ERROR_ARGUMENT, "face index outside [0, vertex_count) in get_vertex_erosion_mask", [&](int* flag) {
		return launch_vertex_erosion_mask(vertex_count, d_face_indices, face_count, iteration_count, min_neighbors, d_out_mask, flag, s);
	});
}

nnrt_status nnrt_sample_nodes(const float* d_points, int64_t point_count, const uint8_t* d_mask, const int64_t* d_order, float node_coverage,
                              int64_t* d_out_indices, int64_t out_capacity, int64_t* h_out_count, int32_t* h_out_rounds, void* stream) {
	NNRT_CHECK_ARG(h_out_count, "null h_out_count");
	NNRT_CHECK_ARG(point_count >= 0 && point_count < (int64_t(1) << 31) / 3, "point count out of range");
	NNRT_CHECK_ARG(point_count == 0 || (d_points && d_out_indices), "null pointer");
	NNRT_CHECK_ARG(node_coverage > 0.f && std::isfinite(node_coverage), "node_coverage must be positive and finite");
	NNRT_CHECK_ARG(std::isnormal(node_coverage * node_coverage), "node_coverage squared must be a finite normal float");
	NNRT_CHECK_ARG(out_capacity >= point_count, "out_capacity must be at least point_count");
	const size_t n = static_cast<size_t>(point_count), out_bytes = sizeof(int64_t) * n;
	NNRT_CHECK_ARG(point_count == 0 || !(ranges_overlap(d_out_indices, out_bytes, d_points, sizeof(float) * 3 * n) ||
	                                     (d_mask && ranges_overlap(d_out_indices, out_bytes, d_mask, n)) ||
	                                     (d_order && ranges_overlap(d_out_indices, out_bytes, d_order, sizeof(int64_t) * n))),
	               "d_out_indices must not overlap an input");
	*h_out_count = 0;
	if (h_out_rounds) *h_out_rounds = 0;
	if (point_count == 0) return NNRT_OK;
	return launch_sample_nodes(d_points, point_count, d_mask, d_order, node_coverage, d_out_indices, h_out_count, h_out_rounds,
	                           static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_compute_vertex_support(const float* d_points, int64_t point_count, const float* d_nodes, int32_t node_count, float node_coverage,
                                        const float* d_node_coverage_weights, float* d_out_support_ratio, int32_t* d_out_nearest_node,
                                        void* stream) {
	NNRT_CHECK_ARG(point_count >= 0 && point_count < (int64_t(1) << 31) / 3, "point count out of range");
	NNRT_CHECK_ARG(node_count >= 0, "negative node count");
	NNRT_CHECK_ARG(point_count == 0 || (d_points && d_out_support_ratio && d_out_nearest_node), "null pointer");
	NNRT_CHECK_ARG(point_count == 0 || node_count == 0 || d_nodes, "null nodes");
	NNRT_CHECK_ARG(d_node_coverage_weights || (node_coverage > 0.f && std::isfinite(node_coverage)), "node_coverage must be positive and finite");
	return launch_vertex_support(d_points, point_count, d_nodes, node_count, node_coverage, d_node_coverage_weights, d_out_support_ratio,
	                             d_out_nearest_node, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_blend_node_transforms(const float* d_points, int64_t point_count, const float* d_nodes, const float* d_node_rotations,
                                       const float* d_node_translations, int32_t node_count, int32_t anchor_count, float node_coverage,
                                       float* d_out_rotations, float* d_out_translations, uint8_t* d_out_fallback, int64_t* h_out_fallback_count,
                                       void* stream) {
	NNRT_CHECK_ARG(anchor_count >= 1 && anchor_count <= MAX_ANCHORS, "anchor_count must be in [1, 8]");
	NNRT_CHECK_ARG(point_count >= 0 && point_count < (int64_t(1) << 31) / 9, "point count out of range");
	NNRT_CHECK_ARG(node_count >= 0, "negative node count");
	NNRT_CHECK_ARG(point_count == 0 || node_count >= 1, "no node to blend from");
	NNRT_CHECK_ARG(point_count == 0 || (d_points && d_nodes && d_node_rotations && d_node_translations && d_out_rotations && d_out_translations &&
	                                    d_out_fallback),
	               "null pointer");
	NNRT_CHECK_ARG(node_coverage > 0.f && std::isfinite(node_coverage) && std::isnormal(node_coverage * node_coverage),
	               "node_coverage must be positive and finite, with a finite normal square");
	return launch_blend_node_transforms(d_points, point_count, d_nodes, d_node_rotations, d_node_translations, node_count, anchor_count,
	                                    node_coverage, d_out_rotations, d_out_translations, d_out_fallback, h_out_fallback_count,
	                                    static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_compute_mesh_from_depth(const float* d_point_image, int32_t height, int32_t width, float max_triangle_edge_distance,
                                         float* d_out_vertices, int32_t* d_out_vertex_pixels, int64_t vertex_capacity, int32_t* d_out_faces,
                                         int64_t face_capacity, int64_t* h_out_vertex_count, int64_t* h_out_face_count, void* stream) {
	NNRT_CHECK_ARG(h_out_vertex_count && h_out_face_count, "null h_out_vertex_count or h_out_face_count");
	NNRT_CHECK_ARG(height >= 0 && width >= 0, "negative image size");
	NNRT_CHECK_ARG(static_cast<int64_t>(height) * width < (int64_t(1) << 29), "image size out of range");
	NNRT_CHECK_ARG(vertex_capacity >= 0 && face_capacity >= 0, "negative vertex_capacity or face_capacity");
	NNRT_CHECK_ARG(height == 0 || width == 0 || d_point_image, "null point image");
	NNRT_CHECK_ARG(vertex_capacity == 0 || (d_out_vertices && d_out_vertex_pixels), "null vertex output");
	NNRT_CHECK_ARG(face_capacity == 0 || d_out_faces, "null face output");
	const size_t in_bytes = sizeof(float) * 3 * static_cast<size_t>(height) * static_cast<size_t>(width), nv = static_cast<size_t>(vertex_capacity),
	             nf = static_cast<size_t>(face_capacity);
	NNRT_CHECK_ARG(!(ranges_overlap(d_out_vertices, sizeof(float) * 3 * nv, d_point_image, in_bytes) ||
	                 ranges_overlap(d_out_vertex_pixels, sizeof(int32_t) * 2 * nv, d_point_image, in_bytes) ||
	                 ranges_overlap(d_out_faces, sizeof(int32_t) * 3 * nf, d_point_image, in_bytes)),
	               "an output must not overlap d_point_image");
	*h_out_vertex_count = 0;
	*h_out_face_count = 0;
	if (height < 2 || width < 2) return NNRT_OK;
	return launch_mesh_from_depth(d_point_image, height, width, max_triangle_edge_distance, d_out_vertices, d_out_vertex_pixels, vertex_capacity,
	                              d_out_faces, face_capacity, h_out_vertex_count, h_out_face_count, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_compute_edges_shortest_path(const float* d_vertices, int64_t vertex_count, const uint8_t* d_vertex_mask, const int32_t* d_faces,
                                             int64_t face_count, const int32_t* d_node_vertex_indices, int32_t node_count,
                                             int32_t max_neighbor_count, float node_coverage, int32_t enforce_total_num_neighbors,
                                             int32_t* d_out_edges, float* d_out_weights, float* d_out_distances, int32_t* h_out_passes,
                                             void* stream) {
	NNRT_CHECK_ARG(vertex_count >= 0 && vertex_count < (int64_t(1) << 31) / 3, "vertex count out of range");
	NNRT_CHECK_ARG(face_count >= 0 && face_count < (int64_t(1) << 31) / 6, "face count out of range");
	NNRT_CHECK_ARG(node_count >= 0, "negative node count");
	NNRT_CHECK_ARG(max_neighbor_count >= 1 && max_neighbor_count <= 1024, "max_neighbor_count must be in [1, 1024]");
	NNRT_CHECK_ARG(static_cast<int64_t>(node_count) * max_neighbor_count < (int64_t(1) << 31), "node_count * max_neighbor_count out of range");
	NNRT_CHECK_ARG(node_coverage > 0.f && std::isfinite(node_coverage), "node_coverage must be positive and finite");
	NNRT_CHECK_ARG(vertex_count == 0 || d_vertices, "null vertices");
	NNRT_CHECK_ARG(face_count == 0 || d_faces, "null faces");
	NNRT_CHECK_ARG(node_count == 0 || (d_node_vertex_indices && d_out_edges && d_out_weights && d_out_distances), "null node indices or output");
	if (h_out_passes) *h_out_passes = 0;
	if (node_count == 0) return NNRT_OK;
	return launch_edges_shortest_path(d_vertices, vertex_count, d_vertex_mask, d_faces, face_count, d_node_vertex_indices, node_count,
	                                  max_neighbor_count, node_coverage, enforce_total_num_neighbors != 0, d_out_edges, d_out_weights,
	                                  d_out_distances, h_out_passes, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_node_and_edge_clean_up(const int32_t* h_graph_edges, int64_t node_count, int32_t max_neighbor_count, uint8_t* h_valid_nodes_mask) {
	NNRT_CHECK_ARG(node_count >= 0 && node_count < (int64_t(1) << 31), "node count out of range");
	NNRT_CHECK_ARG(max_neighbor_count >= 0, "negative max_neighbor_count");
	NNRT_CHECK_ARG(node_count == 0 || h_valid_nodes_mask, "null valid nodes mask");
	NNRT_CHECK_ARG(node_count == 0 || max_neighbor_count == 0 || h_graph_edges, "null graph edges");
	return node_and_edge_clean_up_host(h_graph_edges, node_count, max_neighbor_count, h_valid_nodes_mask);
}

nnrt_status nnrt_compute_clusters(const int32_t* h_graph_edges, int64_t node_count, int32_t max_neighbor_count, int32_t* h_out_clusters,
                                  int32_t* h_out_cluster_sizes, int64_t* h_out_cluster_count) {
	NNRT_CHECK_ARG(h_out_cluster_count, "null h_out_cluster_count");
	NNRT_CHECK_ARG(node_count >= 0 && node_count < (int64_t(1) << 31), "node count out of range");
	NNRT_CHECK_ARG(max_neighbor_count >= 0, "negative max_neighbor_count");
	NNRT_CHECK_ARG(node_count == 0 || (h_out_clusters && h_out_cluster_sizes), "null cluster output");
	NNRT_CHECK_ARG(node_count == 0 || max_neighbor_count == 0 || h_graph_edges, "null graph edges");
	return compute_clusters_host(h_graph_edges, node_count, max_neighbor_count, h_out_clusters, h_out_cluster_sizes, h_out_cluster_count);
}

nnrt_status nnrt_matmul_block_sparse_row_wise(const float* d_a_blocks, int32_t a_block_count, const float* d_b_blocks,
                                              const int32_t* d_b_coordinates, int32_t b_block_count, int32_t block_size, float* d_c_blocks,
                                              uint8_t* d_c_mask, void* stream) {
	NNRT_CHECK_ARG(a_block_count >= 0 && b_block_count >= 0 && block_size > 0, "bad block count or block size");
	NNRT_CHECK_ARG(b_block_count == 0 || (d_b_blocks && d_b_coordinates && d_c_blocks && d_c_mask), "null pointer");
	NNRT_CHECK_ARG(a_block_count == 0 || d_a_blocks, "null pointer");
	hipStream_t s = static_cast<hipStream_t>(stream);
	return with_device_flag(s, NNRT_ERROR_ARGUMENT, "negative block row coordinate in MatmulBlockSparseRowWise", [&](int* flag) {
		return launch_matmul_block_sparse_row_wise(d_a_blocks, a_block_count, d_b_blocks, d_b_coordinates, b_block_count, block_size, d_c_blocks,
		                                           d_c_mask, flag, s);
	});
}

nnrt_status nnrt_matmul_block_sparse(const float* d_a_blocks, int32_t a_block_count, const int16_t* d_a_breadboard, int32_t a_block_rows,
                                     int32_t a_block_columns, int32_t transpose_a, const float* d_b_blocks, int32_t b_block_count,
                                     const int16_t* d_b_breadboard, int32_t b_block_rows, int32_t b_block_columns, int32_t transpose_b,
                                     int32_t block_size, float* d_c_blocks, uint8_t* d_c_mask, void* stream) {
	NNRT_CHECK_ARG(a_block_count >= 0 && b_block_count >= 0 && block_size > 0, "bad block count or block size");
	NNRT_CHECK_ARG(a_block_rows >= 0 && a_block_columns >= 0 && b_block_rows >= 0 && b_block_columns >= 0, "negative breadboard size");
	const int32_t a_inner = transpose_a ? a_block_rows : a_block_columns, b_inner = transpose_b ? b_block_columns : b_block_rows;
	NNRT_CHECK_ARG(a_inner == b_inner, "Matrix inner dimensions must but do not match.");
	const int64_t out_blocks = static_cast<int64_t>(transpose_a ? a_block_columns : a_block_rows) * (transpose_b ? b_block_rows : b_block_columns);
	NNRT_CHECK_ARG(out_blocks == 0 || (d_c_blocks && d_c_mask && d_a_breadboard && d_b_breadboard), "null pointer");
	NNRT_CHECK_ARG((a_block_count == 0 || d_a_blocks) && (b_block_count == 0 || d_b_blocks), "null pointer");
	hipStream_t s = static_cast<hipStream_t>(stream);
	return with_device_flag(s, NNRT_ERROR_ARGUMENT, "breadboard block index out of range in MatmulBlockSparse", [&](int* flag) {
		return launch_matmul_block_sparse(d_a_blocks, a_block_count, d_a_breadboard, a_block_rows, a_block_columns, transpose_a != 0, d_b_blocks,
		                                  b_block_count, d_b_breadboard, b_block_rows, b_block_columns, transpose_b != 0, block_size, d_c_blocks,
		                                  d_c_mask, flag, s);
	});
}

nnrt_status nnrt_block_sparse_and_vector_product(const float* d_blocks, const int32_t* d_coordinates, int32_t block_count, int32_t block_size,
                                                 int32_t block_row_offset, int32_t block_column_offset, int32_t transpose,
                                                 const float* d_vector, int64_t vector_length, int64_t m, float* d_out, void* stream) {
	NNRT_CHECK_ARG(block_count >= 0 && block_size > 0 && vector_length >= 0 && m >= 0, "bad size");
	NNRT_CHECK_ARG(m % block_size == 0, "output length m must be a multiple of the block size");
	NNRT_CHECK_ARG((m == 0 || d_out) && (block_count == 0 || (d_blocks && d_coordinates && d_vector)), "null pointer");
	NNRT_CHECK_ARG(m == 0 || block_count == 0 || !ranges_overlap(d_out, sizeof(float) * m, d_vector, sizeof(float) * vector_length),
	               "d_out must not overlap d_vector (it is zeroed first)");
	hipStream_t s = static_cast<hipStream_t>(stream);
	return with_device_flag(s, NNRT_ERROR_ARGUMENT, "block coordinate outside the matrix in BlockSparseAndVectorProduct", [&](int* flag) {
		return launch_block_sparse_vector(d_blocks, d_coordinates, block_count, block_size, block_row_offset, block_column_offset, transpose != 0,
		                                  d_vector, vector_length, d_out, m, flag, s);
	});
}

nnrt_status nnrt_diagonal_block_sparse_and_vector_product(const float* d_blocks, int32_t block_count, int32_t block_size, const float* d_vector,
                                                          float* d_out, void* stream) {
	NNRT_CHECK_ARG(block_count >= 0 && block_size > 0, "bad block count or block size");
	NNRT_CHECK_ARG(block_count == 0 || (d_blocks && d_vector && d_out), "null pointer");
	return launch_diagonal_block_vector(d_blocks, block_count, block_size, d_vector, d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_sparse_blocks_op(float* d_matrix, int64_t rows, int64_t columns, const float* d_blocks, const int32_t* d_coordinates,
                                  int32_t block_count, int32_t block_size, int64_t block_row_offset, int64_t block_column_offset,
                                  int32_t transpose, int32_t op, void* stream) {
	NNRT_CHECK_ARG(rows >= 0 && columns >= 0 && block_count >= 0 && block_size > 0, "bad size");
	NNRT_CHECK_ARG(op >= 0 && op <= 2, "op must be 0 (fill), 1 (add) or 2 (subtract)");
	NNRT_CHECK_ARG(block_count == 0 || (d_matrix && d_blocks), "null pointer");
	hipStream_t s = static_cast<hipStream_t>(stream);
	return with_device_flag(s, NNRT_ERROR_ARGUMENT, "block placed outside the matrix", [&](int* flag) {
		return launch_sparse_blocks_op(d_matrix, rows, columns, d_blocks, d_coordinates, block_count, block_size, block_row_offset,
		                               block_column_offset, transpose != 0, op, flag, s);
	});
}

nnrt_status nnrt_get_sparse_blocks(const float* d_matrix, int64_t rows, int64_t columns, int32_t block_size, const int32_t* d_coordinates,
                                   int32_t block_count, float* d_blocks, void* stream) {
	NNRT_CHECK_ARG(rows >= 0 && columns >= 0 && block_count >= 0 && block_size > 0, "bad size");
	NNRT_CHECK_ARG(block_count == 0 || (d_matrix && d_blocks), "null pointer");
	hipStream_t s = static_cast<hipStream_t>(stream);
	return with_device_flag(s, NNRT_ERROR_ARGUMENT, "block coordinate outside the matrix", [&](int* flag) {
		return launch_get_sparse_blocks(d_matrix, rows, columns, block_size, d_coordinates, block_count, d_blocks, flag, s);
	});
}

nnrt_status nnrt_transpose_blocks_in_place(float* d_blocks, int32_t block_count, int32_t block_size, void* stream) {
	NNRT_CHECK_ARG(block_count >= 0 && block_size > 0, "bad block count or block size");
	NNRT_CHECK_ARG(block_count == 0 || d_blocks, "null pointer");
	return launch_transpose_blocks(d_blocks, block_count, block_size, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_invert_triangular_blocks(const float* d_blocks, int32_t block_count, int32_t block_size, int32_t upper, float* d_out,
                                          void* stream) {
	NNRT_CHECK_ARG(block_count >= 0 && block_size > 0, "bad block count or block size");
	NNRT_CHECK_ARG(block_count == 0 || (d_blocks && d_out), "null pointer");
	const size_t bytes = sizeof(float) * static_cast<size_t>(block_count) * block_size * block_size;
	NNRT_CHECK_ARG(block_count == 0 || !ranges_overlap(d_out, bytes, d_blocks, bytes),
	               "d_out must not overlap d_blocks (each block's inverse is built column by column while its entries are read)");
	hipStream_t s = static_cast<hipStream_t>(stream);
	return with_device_flag(s, NNRT_ERROR_NOT_POSITIVE_DEFINITE, "trtri failed in InvertTriangularBlocks (zero on a block diagonal)",
	                        [&](int* flag) { return launch_invert_triangular_blocks(d_blocks, block_count, block_size, upper != 0, d_out, flag, s); });
}

} // extern "C"

namespace {
// Everything the arrowhead solve derives from the wing structure alone (ArrowheadStructure, which the fitter holds too)
// and the call's error word, kept per (device, N, n0, coordinates) so a
// repeated structure (a fixed hierarchy, solved every iteration) skips the host planning and the allocations. An entry
// is owned by one call at a time (taken out of the pool, returned after the call has synchronised its stream), so
// concurrent calls never share device scratch; the pool holds the ARROW_POOL_MAX most recently used structures.
struct ArrowheadPlan {
	int device = -1;
	std::vector<int32_t> coords;
	ArrowheadStructure arrow;
	DeviceBuffer<int> flag;
	bool matches(int dev, int32_t n, int32_t base, const std::vector<int32_t>& c) const {
		return device == dev && arrow.N == n && arrow.n0 == base && coords == c;
	}
	nnrt_status build(int dev, int32_t n, int32_t base, std::vector<int32_t> c) {
		device = dev;
		coords = std::move(c);
		const nnrt_status st = arrow.build(coords.data(), static_cast<int>(coords.size() / 2), base, n, nullptr, false);
		return st ? st : flag.ensure(1);
	}
};
constexpr size_t ARROW_POOL_MAX = 4;
std::mutex g_arrow_mu;
// heap-allocated and never destroyed: device memory must not be released by static destructors after the HIP runtime
// has shut down at process exit
std::list<std::unique_ptr<ArrowheadPlan>>& arrow_pool() {
	static auto* pool = new std::list<std::unique_ptr<ArrowheadPlan>>();
	return *pool;
}

} // namespace

extern "C" {

nnrt_status nnrt_solve_block_sparse_arrowhead_cholesky(const float* d_diag, const float* d_wing, const int32_t* d_coords, int32_t E, int32_t N,
                                                       int32_t n0, const float* d_b, float* d_x, void* stream) {
	NNRT_CHECK_ARG(E >= 0 && N >= 0, "negative block count");
	NNRT_CHECK_ARG(n0 >= 0 && n0 <= N, "arrow_base_block_index out of range");
	NNRT_CHECK_ARG((N == 0 || (d_diag && d_b && d_x)) && (E == 0 || (d_wing && d_coords)), "null pointer");
	NNRT_CHECK_ARG((reinterpret_cast<uintptr_t>(d_diag) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_wing) & 15) == 0,
	               "diagonal and wing blocks must be 16-byte aligned (the stem reads 6x6 blocks as float4)");
	NNRT_CHECK_ARG((reinterpret_cast<uintptr_t>(d_x) & 7) == 0, "x must be 8-byte aligned");
	hipStream_t s = static_cast<hipStream_t>(stream);
	std::vector<int32_t> coords(2 * static_cast<size_t>(E));
	if (E > 0) {
		NNRT_HIP(hipMemcpyAsync(coords.data(), d_coords, sizeof(int32_t) * 2 * E, hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));
	}
	for (int e = 0; e < E; e++) {   // before any allocation: the host lists index by these
		const int i = coords[2 * e], j = coords[2 * e + 1];
		NNRT_CHECK_ARG(i >= 0 && i < N && j >= 0 && j < N, "wing block coordinate outside [0, diagonal_block_count)");
		NNRT_CHECK_ARG(i != j, "wing block on the block diagonal");
		NNRT_CHECK_ARG(j >= n0, "wing block column inside the arrow stem (the stem is block-diagonal)");
	}
	if (N == 0) return NNRT_OK;   // the empty system: x is empty too, nothing is launched and no plan is kept
	int device = 0;
	NNRT_HIP(hipGetDevice(&device));
	std::unique_ptr<ArrowheadPlan> plan;
	{
		std::lock_guard<std::mutex> lock(g_arrow_mu);
		auto& pool = arrow_pool();
		for (auto it = pool.begin(); it != pool.end(); ++it)
			if ((*it)->matches(device, N, n0, coords)) {
				plan = std::move(*it);
				pool.erase(it);
				break;
			}
	}
	nnrt_status st = NNRT_OK;
	if (!plan) {
		plan = std::make_unique<ArrowheadPlan>();
		if ((st = plan->build(device, N, n0, std::move(coords)))) return st;
	}
	ArrowheadWorkspace ws;
	plan->arrow.bind(ws);
	ws.diag = const_cast<float*>(d_diag);
	ws.rhs = const_cast<float*>(d_b);
	ws.x = d_x;
	int host_flag = 0;
	if (hipMemsetAsync(plan->flag.ptr, 0, sizeof(int), s) != hipSuccess) {
		set_error("hipMemsetAsync failed");
		return NNRT_ERROR_HIP;
	}
	st = arrowhead_solve_core(ws, d_coords, d_wing, plan->flag.ptr, s);
	if (!st) {
		if (hipMemcpyAsync(&host_flag, plan->flag.ptr, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
		    hipStreamSynchronize(s) != hipSuccess) {
			set_error("arrowhead solve: stream synchronisation failed");
			return NNRT_ERROR_HIP;   // the plan is dropped (its device work state is unknown)
		}
		// the stream is drained: the plan's scratch is free for the next call with this structure; evicted plans are
		// destroyed after the lock is released (freeing device memory synchronises the device and must not block other threads' lookups)
		std::list<std::unique_ptr<ArrowheadPlan>> evicted;
		{
			std::lock_guard<std::mutex> lock(g_arrow_mu);
			auto& pool = arrow_pool();
			pool.push_front(std::move(plan));
			while (pool.size() > ARROW_POOL_MAX) {
				evicted.push_back(std::move(pool.back()));
				pool.pop_back();
			}
		}
	}
	if (st) return st;
	if (host_flag & 8) {
		set_error("arrowhead solve: the corner's dataflow substitution launch gave up waiting on a dependency (k_corner_flow spin bound)");
		return NNRT_ERROR_HIP;
	}
	if (host_flag) {
		set_error("arrowhead solve: a stem block or the Schur complement is not positive-definite");
		return NNRT_ERROR_NOT_POSITIVE_DEFINITE;
	}
	return NNRT_OK;
}

void nnrt_release_arrowhead_plans(void) {
	std::list<std::unique_ptr<ArrowheadPlan>> released;   // freed after the lock is dropped (freeing synchronises the device)
	{
		std::lock_guard<std::mutex> lock(g_arrow_mu);
		released.swap(arrow_pool());
	}
}

// ---- DLPack entry points (include/nnrt_dlpack.h): validate, then forward to the pointer entry points ----------------
} // extern "C"

namespace nnrt {
namespace dl {
nnrt_status dl_check(const DLManagedTensor* mt, const char* name, std::initializer_list<std::pair<int, int>> dtypes, int ndim,
                     std::initializer_list<int64_t> dims, Mem mem, int device, const void** data, int64_t* dims_out) {
	if (!mt) {
		set_error(std::string("invalid argument: ") + name + ": null tensor");
		return NNRT_ERROR_ARGUMENT;
	}
	const DLTensor& t = mt->dl_tensor;
	bool dtype_ok = false;
	for (const auto& d : dtypes) dtype_ok |= t.dtype.code == d.first && t.dtype.bits == d.second && t.dtype.lanes == 1;
	if (!dtype_ok) {
		set_error(std::string("invalid argument: ") + name + ": unsupported dtype (code " + std::to_string(t.dtype.code) + ", bits " +
		          std::to_string(t.dtype.bits) + ")");
		return NNRT_ERROR_ARGUMENT;
	}
	if (t.ndim != ndim) {
		set_error(std::string("invalid argument: ") + name + ": expected " + std::to_string(ndim) + " dimensions, got " + std::to_string(t.ndim));
		return NNRT_ERROR_ARGUMENT;
	}
	int k = 0;
	for (int64_t want : dims) {
		if (want >= 0 && t.shape[k] != want) {
			set_error(std::string("invalid argument: ") + name + ": dimension " + std::to_string(k) + " is " + std::to_string(t.shape[k]) +
			          ", expected " + std::to_string(want));
			return NNRT_ERROR_ARGUMENT;
		}
		dims_out[k] = t.shape[k];
		k++;
	}
	if (t.strides) {   // compact row-major only
		int64_t expect = 1;
		for (int d = ndim - 1; d >= 0; d--) {
			if (t.shape[d] > 1 && t.strides[d] != expect) {
				set_error(std::string("invalid argument: ") + name + ": not a compact row-major tensor");
				return NNRT_ERROR_ARGUMENT;
			}
			expect *= t.shape[d];
		}
	}
	const bool on_device = t.device.device_type == kDLROCM;
	const bool on_host = t.device.device_type == kDLCPU || t.device.device_type == kDLROCMHost;
	if (mem == Mem::device && !(on_device && t.device.device_id == device)) {
		set_error(std::string("invalid argument: ") + name + ": must be a ROCm device tensor on device " + std::to_string(device));
		return NNRT_ERROR_ARGUMENT;
	}
	if (mem == Mem::host && !on_host) {
		set_error(std::string("invalid argument: ") + name + ": must be a host (CPU) tensor");
		return NNRT_ERROR_ARGUMENT;
	}
	*data = static_cast<const char*>(t.data) + t.byte_offset;
	return NNRT_OK;
}
} // namespace dl
} // namespace nnrt

extern "C" {

nnrt_status nnrt_warp_field_create_dlpack(const DLManagedTensor* nodes, float node_coverage, int32_t threshold_nodes_by_distance,
                                          int32_t anchor_count, int32_t minimum_valid_anchor_count, int32_t coverage_method,
                                          int32_t layer_count, int32_t max_vertex_degree, const float* h_layer_radii, int32_t device,
                                          nnrt_warp_field** out) {
	using namespace dl;
	NNRT_CHECK_ARG(nodes != nullptr, "nodes: null tensor");
	const bool on_device = nodes->dl_tensor.device.device_type == kDLROCM;
	const void* data = nullptr;
	int64_t dims[2];
	nnrt_status st = dl_check(nodes, "nodes", {F32}, 2, {-1, 3}, on_device ? Mem::device : Mem::host,
	                          on_device ? nodes->dl_tensor.device.device_id : device, &data, dims);
	if (st) return st;
	NNRT_CHECK_ARG(dims[0] <= INT32_MAX, "nodes: too many nodes");
	std::vector<float> host;
	const float* h_nodes = static_cast<const float*>(data);
	if (on_device) {
		DeviceGuard guard(nodes->dl_tensor.device.device_id);
		host.resize(3 * static_cast<size_t>(dims[0]));
		NNRT_HIP(hipMemcpy(host.data(), data, sizeof(float) * host.size(), hipMemcpyDeviceToHost));
		h_nodes = host.data();
	}
	return nnrt_warp_field_create(h_nodes, static_cast<int32_t>(dims[0]), node_coverage, threshold_nodes_by_distance, anchor_count,
	                              minimum_valid_anchor_count, coverage_method, layer_count, max_vertex_degree, h_layer_radii, device, out);
}


nnrt_status nnrt_rasterize_ndc_triangles_dlpack(const DLManagedTensor* face_ndc, const DLManagedTensor* clip_mask, float blur_radius_pixels,
                                                int32_t perspective_correct_barycentric_coordinates, int32_t clip_barycentric_coordinates,
                                                int32_t cull_back_faces, const DLManagedTensor* pixel_faces, const DLManagedTensor* depths,
                                                const DLManagedTensor* barycentrics, const DLManagedTensor* distances, void* stream) {
	using namespace dl;
	NNRT_CHECK_ARG(face_ndc != nullptr, "face_ndc: null tensor");
	const int dev = face_ndc->dl_tensor.device.device_id;
	const void *pn, *pm = nullptr, *pf, *pd, *pb, *ps;
	int64_t dn[3], dm[1], df[3], dd[3], db[4], ds[3];
	nnrt_status st;
	if ((st = dl_check(face_ndc, "face_ndc", {F32}, 3, {-1, 3, 3}, Mem::device, dev, &pn, dn))) return st;
	if (clip_mask && (st = dl_check(clip_mask, "clip_mask", {B8, U8}, 1, {dn[0]}, Mem::device, dev, &pm, dm))) return st;
	if ((st = dl_check(pixel_faces, "pixel_faces", {I64}, 3, {-1, -1, -1}, Mem::device, dev, &pf, df))) return st;
	if ((st = dl_check(depths, "depths", {F32}, 3, {df[0], df[1], df[2]}, Mem::device, dev, &pd, dd))) return st;
	if ((st = dl_check(barycentrics, "barycentrics", {F32}, 4, {df[0], df[1], df[2], 3}, Mem::device, dev, &pb, db))) return st;
	if ((st = dl_check(distances, "distances", {F32}, 3, {df[0], df[1], df[2]}, Mem::device, dev, &ps, ds))) return st;
	NNRT_CHECK_ARG(df[0] <= INT32_MAX && df[1] <= INT32_MAX && df[2] <= INT32_MAX, "pixel_faces: image too large");
	DeviceGuard guard(dev);
	return nnrt_rasterize_ndc_triangles(static_cast<const float*>(pn), static_cast<const uint8_t*>(pm), dn[0], static_cast<int32_t>(df[0]),
	                                    static_cast<int32_t>(df[1]), blur_radius_pixels, static_cast<int32_t>(df[2]), -1, -1,
	                                    perspective_correct_barycentric_coordinates, clip_barycentric_coordinates, cull_back_faces,
	                                    static_cast<int64_t*>(const_cast<void*>(pf)), static_cast<float*>(const_cast<void*>(pd)),
	                                    static_cast<float*>(const_cast<void*>(pb)), static_cast<float*>(const_cast<void*>(ps)), stream);
}

} // extern "C"
