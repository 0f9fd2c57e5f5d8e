// Private to the native library: the warp-field handle and the few host helpers that capi.hip (the warp-field exports,
// the stateless wrappers) and fitter.hip (the fitter) both use. struct nnrt_fitter stays private to fitter.hip.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

#include "fitter_kernels.hpp"
#include "launch_plan.hpp"
#include "warp_field.hpp"
#include "nnrt_dlpack.h"

struct nnrt_warp_field {
	int device = 0;
	int N = 0;
	float coverage = 0.05f;
	int threshold = 0;
	int anchor_count = 4;
	int minimum_valid = 0;
	int coverage_method = NNRT_MINIMAL_K_NEIGHBOR_NODE_DISTANCE;
	nnrt::Hierarchy h;
	std::vector<float> nodes_original;     // [N,3] original order
	std::vector<float> weights_virtual;    // [N] coverage weights, virtual order
	nnrt::DeviceBuffer<float> state;             // [N,16] virtual order
	nnrt::DeviceBuffer<float> node_positions;    // [N,3] virtual order (anchor computation input)
	nnrt::DeviceBuffer<float> node_weights;      // [N] virtual order
	nnrt::DeviceBuffer<int32_t> edges;           // [E,2]
	nnrt::DeviceBuffer<int8_t> edge_layers;      // [E]
	nnrt::DeviceBuffer<float> radii;             // [layers]
	uint64_t id = 0;                       // unique per created warp field (a fitter's cached graphs capture its buffers)
	int E() const { return static_cast<int>(h.edge_layers.size()); }
};

namespace nnrt {
// positions [count, 3] of the nodes first .. first + count - 1 in virtual order (the corner plans' coordinate bisection)
inline std::vector<float> virtual_node_positions(const nnrt_warp_field* wf, int first, int count) {
	std::vector<float> pos(3 * static_cast<size_t>(count));
	for (int a = 0; a < count; a++) {
		const int64_t o = wf->h.virtual_indices.empty() ? first + a : wf->h.virtual_indices[static_cast<size_t>(first + a)];
		for (int c = 0; c < 3; c++) pos[3 * static_cast<size_t>(a) + c] = wf->nodes_original[3 * static_cast<size_t>(o) + c];
	}
	return pos;
}
Camera pixel_camera(const double* K);
// node motion -> identity (k_reset_motion); node state [N,16] copy (k_copy_state), on s (inside or outside a capture)
nnrt_status launch_reset_motion(float* state, int N, hipStream_t s);
nnrt_status launch_copy_state(const float* src, float* dst, int N, hipStream_t s);

namespace dl {   // DLPack argument check of the *_dlpack entry points
enum class Mem { device, host };
// dtypes: list of (code, bits); dims: -1 = any extent (returned through `dims_out`)
nnrt_status dl_check(const DLManagedTensor* mt, const char* name, std::initializer_list<std::pair<int, int>> dtypes, int ndim,
                     std::initializer_list<int64_t> dims, Mem mem, int device, const void** data, int64_t* dims_out);
constexpr std::pair<int, int> F32{kDLFloat, 32}, F64{kDLFloat, 64}, I64{kDLInt, 64}, U8{kDLUInt, 8}, B8{kDLBool, 8};
} // namespace dl
} // namespace nnrt
