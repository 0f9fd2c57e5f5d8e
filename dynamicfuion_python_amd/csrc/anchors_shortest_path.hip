// Shortest-path anchors over the motion graph on gfx950.
//   cpp/core/kernel/KnnUtilities_PriorityQueue.h:102-160 (FindShortestPathKnn_PriorityQueue),
//   cpp/geometry/functional/kernel/WarpUtilities.h:347-375, WarpAnchorComputationImpl.h:146-237.
// Per point: seed a 40-entry min-queue with the Euclidean-nearest node that is not an anchor yet, pop the smallest
// (distance, node), record it as the next anchor unless it already is one, push its graph neighbours at
// distance + edge length; when the queue runs dry before K anchors are found, seed again. Gaussian weights of the path
// distances, normalized.
//
// One lane per point, one wave per workgroup (as k_compute_anchors). The queue lives in LDS, entry-major and
// lane-minor: entry e of lane l is word e * 64 + l, so a wave's access to one entry touches 64 consecutive words (no
// bank conflict) and the divergent walk indexes it at run time without scratch. A pop is a linear minimum scan over the
// live entries (key, then node index), the popped slot is refilled from the last entry: the pop order depends on the
// (key, node) pairs alone, and an insert into a full queue is dropped by its size alone, as in the reference's heap.
// The seed scan runs wave-wide: 64 nodes per coalesced load, broadcast by readlane, entered whenever some lane needs a
// seed; every lane of the wave takes part in the loads (lanes past the last point and lanes that are finished only
// skip the comparison), and the walk's divergence closes before the next scan.
#include "anchor_dispatch.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {
constexpr int SP_BLOCK = 64;
constexpr int SP_QUEUE = 40;   // KnnUtilities_PriorityQueue.h:112

__device__ inline float sp_lane_read(float v, int src) {
	return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// an edge entry >= N raises the flag (the reference reads the node array out of range there; negative = empty)
__global__ __launch_bounds__(256) void k_check_anchor_edges(const int32_t* __restrict__ edges, int64_t count, int node_count,
                                                            int* __restrict__ error_flag) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
	if (i < count && edges[i] >= node_count) atomicOr(error_flag, 1);
}

template <int K>
__global__ __launch_bounds__(SP_BLOCK) void k_anchors_shortest_path(const float* __restrict__ points, int64_t point_count,
                                                                    const float* __restrict__ nodes, int node_count,
                                                                    const int32_t* __restrict__ edges, int degree, float coverage_squared,
                                                                    const float* __restrict__ node_weights, int32_t* __restrict__ anchors,
                                                                    float* __restrict__ weights) {
#pragma clang fp contract(off)
	__shared__ float q_key[SP_QUEUE * SP_BLOCK];
	__shared__ int32_t q_node[SP_QUEUE * SP_BLOCK];
	const int lane = static_cast<int>(threadIdx.x);
	const int64_t i = static_cast<int64_t>(blockIdx.x) * SP_BLOCK + lane;
	const bool active = i < point_count;
	float px = 0.f, py = 0.f, pz = 0.f;
	if (active) {
		px = points[3 * i];
		py = points[3 * i + 1];
		pz = points[3 * i + 2];
	}
	int32_t idx[K];
	float dist[K];
#pragma unroll
	for (int k = 0; k < K; k++) {
		idx[k] = -1;
		dist[k] = 0.f;
	}
	int found = 0, live = 0;
	bool done = !active;   // K anchors found, or no node left to seed with
	auto push = [&](float key, int32_t node) {
		if (live < SP_QUEUE) {   // DeviceHeapCPU.h:30-31: an insert into a full queue is dropped
			q_key[live * SP_BLOCK + lane] = key;
			q_node[live * SP_BLOCK + lane] = node;
			live++;
		}
	};
	// no lane leaves before the loop ends: the seed scan's loads and broadcasts need the whole wave
	while (__any(!done)) {
		// ---- seed: the nearest node that is no anchor yet, strict < in ascending node order (lowest index wins a tie)
		float best = INFINITY;
		int32_t best_node = -1;
		for (int base = 0; base < node_count; base += 64) {
			float cx = 0.f, cy = 0.f, cz = 0.f;
			if (base + lane < node_count) {
				const int64_t j = base + lane;
				cx = nodes[3 * j];
				cy = nodes[3 * j + 1];
				cz = nodes[3 * j + 2];
			}
			const int batch = node_count - base < 64 ? node_count - base : 64;
#pragma unroll 8
			for (int g = 0; g < 64; g++) {
				const float dx = sp_lane_read(cx, g) - px, dy = sp_lane_read(cy, g) - py, dz = sp_lane_read(cz, g) - pz;
				const float sq = (dx * dx + dy * dy) + dz * dz;
				if (g < batch && !done && sq < best) {
					const int32_t j = base + g;
					bool taken = false;
#pragma unroll
					for (int k = 0; k < K; k++) taken |= idx[k] == j;
					if (!taken) {
						best = sq;
						best_node = j;
					}
				}
			}
		}
		if (!done) {
			if (best_node < 0) {
				done = true;
			} else {
				push(sqrtf(best), best_node);
				// ---- walk
				while (live > 0 && found < K) {
					float key = q_key[lane];
					int32_t node = q_node[lane];
					int at = 0;
					for (int e = 1; e < live; e++) {
						const float ke = q_key[e * SP_BLOCK + lane];
						const int32_t ne = q_node[e * SP_BLOCK + lane];
						if (ke < key || (ke == key && ne < node)) {
							key = ke;
							node = ne;
							at = e;
						}
					}
					live--;
					if (at != live) {
						q_key[at * SP_BLOCK + lane] = q_key[live * SP_BLOCK + lane];
						q_node[at * SP_BLOCK + lane] = q_node[live * SP_BLOCK + lane];
					}
					bool taken = false;
#pragma unroll
					for (int k = 0; k < K; k++) taken |= idx[k] == node;
					if (taken) continue;
#pragma unroll
					for (int k = 0; k < K; k++) {
						if (k == found) {
							idx[k] = node;
							dist[k] = key;
						}
					}
					found++;
					if (found >= K) break;
					const float sx = nodes[3 * static_cast<int64_t>(node)], sy = nodes[3 * static_cast<int64_t>(node) + 1],
					            sz = nodes[3 * static_cast<int64_t>(node) + 2];
					const int32_t* row = edges + static_cast<int64_t>(node) * degree;
					for (int s = 0; s < degree; s++) {
						const int32_t t = row[s];
						if (t < 0 || t >= node_count) continue;   // >= node_count: refused by the launcher, never read
						const float dx = nodes[3 * static_cast<int64_t>(t)] - sx, dy = nodes[3 * static_cast<int64_t>(t) + 1] - sy,
						            dz = nodes[3 * static_cast<int64_t>(t) + 2] - sz;
						push(key + sqrtf((dx * dx + dy * dy) + dz * dz), t);
					}
				}
				if (found >= K) done = true;
			}
		}
	}
	if (!active) return;
	// ---- weights (WarpUtilities.h:51-92, :36-46); a slot never filled: anchor -1, weight 0, nothing added to the sum
	float w[K];
	float sum = 0.f;
#pragma unroll
	for (int k = 0; k < K; k++) {
		w[k] = 0.f;
		if (idx[k] >= 0) {
			const float c2 = node_weights ? node_weights[idx[k]] : coverage_squared;
			const float wt = exp_cr(-(dist[k] * dist[k]) / (2 * c2));
			sum += wt;
			w[k] = wt;
		}
	}
#pragma unroll
	for (int k = 0; k < K; k++) {
		anchors[i * K + k] = idx[k];
		weights[i * K + k] = sum > 0.0f ? w[k] / sum : 1.0f / static_cast<float>(K);
	}
}
} // namespace

nnrt_status launch_anchors_shortest_path(const float* points, int64_t V, const float* nodes, int N, const int32_t* edges, int D, int K,
                                         float coverage, const float* node_weights, int32_t* anchors, float* weights, hipStream_t stream,
                                         bool edges_checked) {
	NNRT_CHECK_ARG(K >= 1 && K <= MAX_ANCHORS, "anchor_count must be in [1, 8]");
	NNRT_CHECK_ARG(N >= 0, "negative node count");
	NNRT_CHECK_ARG(D >= 1, "graph_degree must be at least 1");
	NNRT_CHECK_ARG(V >= 0, "negative point count");
	if (V == 0) return NNRT_OK;
	if (!edges_checked && N > 0) {
		nnrt_status st = check_anchor_edges(edges, N, D, stream);
		if (st) return st;
	}
	const dim3 grid(static_cast<unsigned>(ceil_div(V, SP_BLOCK)));
	const float c2 = coverage * coverage;
	const nnrt_status st = dispatch_anchor_count(K, [&](auto kk) {
		k_anchors_shortest_path<decltype(kk)::value><<<grid, SP_BLOCK, 0, stream>>>(points, V, nodes, N, edges, D, c2, node_weights, anchors, weights);
		return NNRT_OK;
	});
	if (st) return st;
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status check_anchor_edges(const int32_t* edges, int N, int D, hipStream_t stream) {
	const int64_t count = static_cast<int64_t>(N) * D;
	if (count == 0) return NNRT_OK;
	DeviceBuffer<int> flag;
	if (nnrt_status st = flag.ensure(1)) return st;
	int err = 0;
	hipError_t e = hipMemsetAsync(flag.ptr, 0, sizeof(int), stream);
	if (e == hipSuccess) {
		k_check_anchor_edges<<<static_cast<unsigned>(ceil_div(count, 256)), 256, 0, stream>>>(edges, count, N, flag.ptr);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(&err, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, stream);
	if (e == hipSuccess) e = hipStreamSynchronize(stream);
	NNRT_HIP(e);
	if (err) {
		set_error("invalid argument: edge entry outside [-1, node_count) in the anchor graph");
		return NNRT_ERROR_ARGUMENT;
	}
	return NNRT_OK;
}

} // namespace nnrt
