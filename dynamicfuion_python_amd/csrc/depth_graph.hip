// Motion graph from a depth image on the GPU: the reference's legacy CPU routines behind
// build_graph_warp_field_from_depth_image (apps/create_graph_data.py:27-296)
//   * compute_mesh_from_depth (cpp/cpu/image_proc.cpp:341-482): the pixel-connected mesh of a point image. A cell is the
//     2x2 pixel square at (x, y), x < W-1, y < H-1. It emits triangle A (00, 01, 10) if all three have z > 0 and all three
//     edge lengths sqrtf((dx*dx + dy*dy) + dz*dz) (unfused f32) are <= the threshold, then triangle B (11, 10, 01) under
//     the same test. A vertex gets its index the first time a valid triangle touches its pixel, cells scanned row-major
//     and the slots of a cell in the order above. That numbering is a scan, not a serial dependence: a pixel is touched by
//     at most four cells, so "is this (cell, slot) the first to touch its pixel" is decided from the validity bits of the
//     up to three earlier cells around it. Per cell: validity bits -> number of new vertices (0..4) and faces (0..2) ->
//     two exclusive scans -> scatter. The output equals the sequential loop's bit for bit, numbering and order included.
//   * compute_edges_shortest_path (cpp/cpu/graph_proc.cpp:181-338): per source node a Dijkstra over the mesh edges, the
//     nearest other nodes by geodesic distance as its neighbours. Each relaxation is d_u + len(u, v) in f32. Adding a
//     non-negative length in f32 is monotone in d_u and never lowers it, so Dijkstra's values are the least fixed point of
//     D(v) = min_u fl(D(u) + len(u, v)), D(source) = 0, and any schedule of relaxations that runs until nothing drops
//     reaches the same bits. Here: one workgroup per source node, a worklist of the vertices whose distance dropped, rounds
//     under __syncthreads, atomicMin on the distance's bit pattern (non-negative floats order as unsigned ints). No
//     workgroup waits on another. A vertex is entered only at D <= R: prefix lengths along a path never decrease, so a
//     path of length <= R has every prefix <= R and the distances <= R found under the restriction are the unrestricted
//     ones. Equal distances are ordered by node index (the reference orders them by its heap's state).
//   * node_and_edge_clean_up and compute_clusters (graph_proc.cpp:540-636): N x K integers, host code.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "common.hpp"
#include "device_primitives.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {
constexpr int GB = 256;   // threads per workgroup

unsigned gblocks(int64_t n) { return static_cast<unsigned>(ceil_div(n, GB)); }

// the reference's (a - b).norm(): unfused, correctly rounded (the build pins -ffp-contract=off; the pragma keeps it so)
__device__ inline float edge_length(const float* __restrict__ a, const float* __restrict__ b) {
#pragma clang fp contract(off)
	const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
	return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// ------------------------------------------------------------------- mesh ----
constexpr uint8_t TRI_A = 1, TRI_B = 2;

__device__ inline bool triangle_ok(const float* __restrict__ p, const float* __restrict__ q, const float* __restrict__ r, float limit) {
	if (!(p[2] > 0.f && q[2] > 0.f && r[2] > 0.f)) return false;   // NaN z is invalid, as in the reference
	return edge_length(p, q) <= limit && edge_length(p, r) <= limit && edge_length(q, r) <= limit;
}

// bits[c] of cell c = y * (W - 1) + x
__global__ __launch_bounds__(GB) void k_cell_bits(const float* __restrict__ pts, int H, int W, float limit, uint8_t* __restrict__ bits) {
	const int c = blockIdx.x * GB + threadIdx.x;
	const int cw = W - 1;
	if (c >= (H - 1) * cw) return;
	const int y = c / cw, x = c - y * cw;
	const float* p00 = pts + 3 * (static_cast<int64_t>(y) * W + x);
	const float* p10 = p00 + 3;
	const float* p01 = p00 + 3 * static_cast<int64_t>(W);
	const float* p11 = p01 + 3;
	uint8_t b = 0;
	if (triangle_ok(p00, p01, p10, limit)) b |= TRI_A;
	if (triangle_ok(p10, p11, p01, limit)) b |= TRI_B;   // d0 = |10 - 01|, d1 = |10 - 11|, d2 = |01 - 11|
	bits[c] = b;
}

__device__ inline uint8_t cell_at(const uint8_t* __restrict__ bits, int x, int y, int cw, int ch) {
	return (x >= 0 && y >= 0 && x < cw && y < ch) ? bits[y * cw + x] : 0;
}

// Which corners of cell (x, y) get their vertex index from this cell, in numbering order (at most 4 pixels, as dx | dy << 1).
// Corner 00 = pixel (x, y) is also 11 of cell (x-1, y-1) [B], 01 of (x, y-1) [A or B], 10 of (x-1, y) [A or B];
// corner 10 = pixel (x+1, y) is also 11 of (x, y-1) [B] and 01 of (x+1, y-1) [A or B]; corner 01 = pixel (x, y+1) is also
// 11 of (x-1, y) [B]; corner 11 is touched by no earlier cell.
__device__ inline int cell_new_corners(const uint8_t* __restrict__ bits, int x, int y, int cw, int ch, uint8_t b, int (&corner)[4]) {
	if (!b) return 0;
	const bool new00 = !(cell_at(bits, x - 1, y - 1, cw, ch) & TRI_B) && !cell_at(bits, x, y - 1, cw, ch) && !cell_at(bits, x - 1, y, cw, ch);
	const bool new10 = !(cell_at(bits, x, y - 1, cw, ch) & TRI_B) && !cell_at(bits, x + 1, y - 1, cw, ch);
	const bool new01 = !(cell_at(bits, x - 1, y, cw, ch) & TRI_B);
	int n = 0;
	if (b & TRI_A) {
		if (new00) corner[n++] = 0;
		if (new01) corner[n++] = 2;
		if (new10) corner[n++] = 1;
		if (b & TRI_B) corner[n++] = 3;
	} else {
		corner[n++] = 3;
		if (new10) corner[n++] = 1;
		if (new01) corner[n++] = 2;
	}
	return n;
}

// counts of cell c; entry C (one past the last cell) is 0, so the exclusive scans end with the totals
__global__ __launch_bounds__(GB) void k_cell_counts(const uint8_t* __restrict__ bits, int H, int W, int* __restrict__ vcount, int* __restrict__ fcount) {
	const int c = blockIdx.x * GB + threadIdx.x;
	const int cw = W - 1, ch = H - 1;
	if (c > ch * cw) return;
	if (c == ch * cw) {
		vcount[c] = 0;
		fcount[c] = 0;
		return;
	}
	const int y = c / cw, x = c - y * cw;
	const uint8_t b = bits[c];
	int corner[4];
	vcount[c] = cell_new_corners(bits, x, y, cw, ch, b, corner);
	fcount[c] = ((b & TRI_A) ? 1 : 0) + ((b & TRI_B) ? 1 : 0);
}

// vertex_cap bounds every write: the caller launches this only when the total fits
__global__ __launch_bounds__(GB) void k_scatter_vertices(const float* __restrict__ pts, const uint8_t* __restrict__ bits, int H, int W,
                                                         const int* __restrict__ voff, int64_t vertex_cap, float* __restrict__ vertices,
                                                         int32_t* __restrict__ pixels, int* __restrict__ pixel_vertex) {
	const int c = blockIdx.x * GB + threadIdx.x;
	const int cw = W - 1, ch = H - 1;
	if (c >= ch * cw) return;
	const int y = c / cw, x = c - y * cw;
	int corner[4];
	const int n = cell_new_corners(bits, x, y, cw, ch, bits[c], corner);
	for (int i = 0; i < n; i++) {
		const int64_t v = static_cast<int64_t>(voff[c]) + i;
		if (v >= vertex_cap) return;
		const int px = x + (corner[i] & 1), py = y + (corner[i] >> 1);
		const int64_t pixel = static_cast<int64_t>(py) * W + px;
		vertices[3 * v] = pts[3 * pixel];
		vertices[3 * v + 1] = pts[3 * pixel + 1];
		vertices[3 * v + 2] = pts[3 * pixel + 2];
		pixels[2 * v] = px;
		pixels[2 * v + 1] = py;
		pixel_vertex[pixel] = static_cast<int>(v);
	}
}

__global__ __launch_bounds__(GB) void k_scatter_faces(const uint8_t* __restrict__ bits, int H, int W, const int* __restrict__ foff, int64_t face_cap,
                                                      const int* __restrict__ pixel_vertex, int32_t* __restrict__ faces) {
	const int c = blockIdx.x * GB + threadIdx.x;
	const int cw = W - 1, ch = H - 1;
	if (c >= ch * cw) return;
	const uint8_t b = bits[c];
	if (!b) return;
	const int y = c / cw, x = c - y * cw;
	const int64_t i00 = static_cast<int64_t>(y) * W + x, i10 = i00 + 1, i01 = i00 + W, i11 = i01 + 1;
	int64_t f = foff[c];
	if (b & TRI_A) {
		if (f >= face_cap) return;
		faces[3 * f] = pixel_vertex[i00];
		faces[3 * f + 1] = pixel_vertex[i01];
		faces[3 * f + 2] = pixel_vertex[i10];
		f++;
	}
	if (b & TRI_B) {
		if (f >= face_cap) return;
		faces[3 * f] = pixel_vertex[i11];
		faces[3 * f + 1] = pixel_vertex[i10];
		faces[3 * f + 2] = pixel_vertex[i01];
	}
}

// -------------------------------------------------------------- adjacency ----
constexpr uint64_t NO_PAIR = ~0ull;

// the six directed pairs (u << 32 | v) of every face; a face with an index outside [0, V) raises the flag and emits
// nothing, a pair with u == v is dropped
__global__ __launch_bounds__(GB) void k_face_pairs(const int32_t* __restrict__ faces, int64_t F, int64_t V, uint64_t* __restrict__ keys,
                                                   int* __restrict__ error_flag) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (f >= F) return;
	const int32_t a[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
	const bool ok = a[0] >= 0 && a[0] < V && a[1] >= 0 && a[1] < V && a[2] >= 0 && a[2] < V;
	if (!ok) atomicOr(error_flag, 1);
	int o = 0;
#pragma unroll
	for (int i = 0; i < 3; i++) {
#pragma unroll
		for (int j = 0; j < 3; j++) {
			if (i == j) continue;
			keys[6 * f + o++] = (ok && a[i] != a[j]) ? ((static_cast<uint64_t>(static_cast<uint32_t>(a[i])) << 32) | static_cast<uint32_t>(a[j])) : NO_PAIR;
		}
	}
}

__global__ __launch_bounds__(GB) void k_pair_flags(const uint64_t* __restrict__ sorted, int64_t n, uint8_t* __restrict__ flags) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = sorted[i];
	flags[i] = (k != NO_PAIR && (i == 0 || sorted[i - 1] != k)) ? 1 : 0;
}

// row_start[v] for v in [0, V]: first unique pair whose source is >= v
__global__ __launch_bounds__(GB) void k_row_starts(const uint64_t* __restrict__ pairs, int E, int64_t V, int* __restrict__ row_start) {
	const int64_t v = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (v > V) return;
	const uint64_t k = static_cast<uint64_t>(v) << 32;
	int lo = 0, hi = E;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (pairs[mid] < k) lo = mid + 1;
		else hi = mid;
	}
	row_start[v] = lo;
}

// pairs hold indices inside [0, V) only (k_face_pairs)
__global__ __launch_bounds__(GB) void k_pair_columns(const uint64_t* __restrict__ pairs, int E, const float* __restrict__ vertices, int* __restrict__ col,
                                                     float* __restrict__ len) {
	const int e = blockIdx.x * GB + threadIdx.x;
	if (e >= E) return;
	const uint64_t k = pairs[e];
	const int64_t u = static_cast<int64_t>(k >> 32), v = static_cast<int64_t>(k & 0xffffffffu);
	col[e] = static_cast<int>(v);
	len[e] = edge_length(vertices + 3 * u, vertices + 3 * v);
}

// node_vertex entries are negative (skipped) or inside [0, V) and distinct (checked on the host)
__global__ __launch_bounds__(GB) void k_vertex_nodes(const int32_t* __restrict__ node_vertex, int N, int* __restrict__ vertex_node) {
	const int i = blockIdx.x * GB + threadIdx.x;
	if (i >= N) return;
	const int32_t v = node_vertex[i];
	if (v >= 0) vertex_node[v] = i;
}

// --------------------------------------------------------------- geodesic ----
constexpr unsigned UNREACHED = 0xffffffffu;


struct GeodesicArgs {
	const int* batch;              // node index per workgroup
	const int32_t* node_vertex;    // [N]
	int64_t V;
	int N, K;
	const int* row_start;          // CSR over the unique directed vertex pairs
	const int* col;
	const float* len;
	const uint8_t* mask;           // [V] or null
	const int* vertex_node;        // [V] node of a vertex or -1
	float radius, coverage;
	// per workgroup slot, V entries each: distance bits (UNREACHED between launches), the round a vertex was last queued
	// in (0 between launches), the reached vertices and two worklists; N candidate keys per slot
	unsigned* dist;
	int* queued_round;
	int* reached;
	int* list_a;
	int* list_b;
	unsigned long long* candidates;
	int32_t* edges;                // [N, K] outputs
	float* weights;
	float* distances;
	int* found;                    // [N] number of other nodes reached
	int* cut;                      // [N] 1 iff the radius refused a relaxation
};

__global__ __launch_bounds__(GB) void k_geodesic(const GeodesicArgs a) {
	__shared__ int n_list[2], n_reached, n_cand, was_cut;
	__shared__ unsigned long long best;
	const int slot = blockIdx.x, tid = threadIdx.x;
	const int node = a.batch[slot];
	const int source = a.node_vertex[node];   // inside [0, V): the host launches no other node
	const int64_t base = static_cast<int64_t>(slot) * a.V;
	unsigned* dist = a.dist + base;
	int* queued_round = a.queued_round + base;
	int* reached = a.reached + base;
	int* lists[2] = {a.list_a + base, a.list_b + base};
	unsigned long long* cand = a.candidates + static_cast<int64_t>(slot) * a.N;
	if (tid == 0) {
		dist[source] = 0u;   // +0.f; the source is entered whatever the mask says, as in the reference
		reached[0] = source;
		lists[0][0] = source;
		n_list[0] = 1;
		n_list[1] = 0;
		n_reached = 1;
		n_cand = 0;
		was_cut = 0;
	}
	__syncthreads();
	// Rounds: every vertex whose distance dropped in the last round relaxes its edges. A vertex enters the next list at
	// most once per round (queued_round), so a list holds at most V entries; a vertex enters `reached` once, on its first
	// drop from UNREACHED.
	for (int round = 1;; round++) {
		const int* cur = lists[(round - 1) & 1];
		int* next = lists[round & 1];
		const int count = n_list[(round - 1) & 1];
		if (count == 0) break;
		for (int j = tid; j < count; j += GB) {
			const int u = cur[j];
			const float du = __uint_as_float(__hip_atomic_load(dist + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
			const int e1 = a.row_start[u + 1];
			for (int e = a.row_start[u]; e < e1; e++) {
				const int v = a.col[e];
				if (a.mask && !a.mask[v]) continue;
				const float nd = du + a.len[e];
				if (!(nd <= a.radius)) {
					if (nd > a.radius) was_cut = 1;   // every writer stores 1; a NaN length cuts nothing and enters nothing
					continue;
				}
				const unsigned nb = __float_as_uint(nd);   // nd >= +0: the bit pattern orders as the value
				const unsigned old = atomicMin(dist + v, nb);
				if (nb >= old) continue;
				if (old == UNREACHED) reached[atomicAdd(&n_reached, 1)] = v;
				if (atomicExch(queued_round + v, round) != round) next[atomicAdd(&n_list[round & 1], 1)] = v;
			}
		}
		__syncthreads();
		if (tid == 0) n_list[(round - 1) & 1] = 0;
		__syncthreads();
	}
	// the other nodes among the reached vertices, as (distance bits, node index) keys: all distinct
	const int total = n_reached;
	for (int j = tid; j < total; j += GB) {
		const int v = reached[j];
		const int other = a.vertex_node[v];
		if (other >= 0 && other != node)
			cand[atomicAdd(&n_cand, 1)] = (static_cast<unsigned long long>(__hip_atomic_load(dist + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) << 32) |
			                              static_cast<unsigned>(other);
	}
	__syncthreads();
	// the K smallest keys in ascending order, one block-wide minimum per output slot
	const int cands = n_cand;
	const int keep = cands < a.K ? cands : a.K;
	unsigned long long last = 0;
	for (int k = 0; k < keep; k++) {
		if (tid == 0) best = ~0ull;
		__syncthreads();
		unsigned long long mine = ~0ull;
		for (int j = tid; j < cands; j += GB) {
			const unsigned long long c = cand[j];
			if ((k == 0 || c > last) && c < mine) mine = c;
		}
		if (mine != ~0ull) atomicMin(&best, mine);
		__syncthreads();
		last = best;
		__syncthreads();
		if (tid == 0) {
			a.edges[static_cast<int64_t>(node) * a.K + k] = static_cast<int32_t>(last & 0xffffffffu);
			a.distances[static_cast<int64_t>(node) * a.K + k] = __uint_as_float(static_cast<unsigned>(last >> 32));
		}
	}
	if (tid == 0) {
		// graph_proc.cpp:171-173 and :316-331: weights from the distances, normalized by their left-to-right sum
		float* w = a.weights + static_cast<int64_t>(node) * a.K;
		const float* d = a.distances + static_cast<int64_t>(node) * a.K;
		float sum = 0.f;
		for (int k = 0; k < keep; k++) {
			w[k] = exp_cr(-(d[k] * d[k]) / (2.f * a.coverage * a.coverage));
			sum += w[k];
		}
		const float by = sum > 0.f ? sum : static_cast<float>(keep);
		for (int k = 0; k < keep; k++) w[k] = w[k] / by;
		a.found[node] = cands;
		a.cut[node] = was_cut;
	}
	// leave the slot as it was found
	for (int j = tid; j < total; j += GB) {
		const int v = reached[j];
		dist[v] = UNREACHED;
		queued_round[v] = 0;
	}
}
} // namespace

// ------------------------------------------------------------ launchers ----
nnrt_status launch_mesh_from_depth(const float* pts, int H, int W, float limit, float* vertices, int32_t* pixels, int64_t vertex_cap, int32_t* faces,
                                   int64_t face_cap, int64_t* h_vertex_count, int64_t* h_face_count, hipStream_t s) {
	*h_vertex_count = 0;
	*h_face_count = 0;
	if (H < 2 || W < 2) return NNRT_OK;
	const int C = (H - 1) * (W - 1);
	DeviceBuffer<uint8_t> bits, tmp;
	DeviceBuffer<int> vcount, fcount, voff, foff, pixel_vertex;
	nnrt_status st;
	if ((st = bits.ensure(C)) || (st = vcount.ensure(C + 1)) || (st = fcount.ensure(C + 1)) || (st = voff.ensure(C + 1)) || (st = foff.ensure(C + 1))) return st;
	k_cell_bits<<<gblocks(C), GB, 0, s>>>(pts, H, W, limit, bits.ptr);
	NNRT_LAUNCH_CHECK();
	k_cell_counts<<<gblocks(C + 1), GB, 0, s>>>(bits.ptr, H, W, vcount.ptr, fcount.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = exclusive_sum(vcount.ptr, voff.ptr, C + 1, tmp, s)) || (st = exclusive_sum(fcount.ptr, foff.ptr, C + 1, tmp, s))) return st;
	int nv = 0, nf = 0;
	NNRT_HIP(hipMemcpyAsync(&nv, voff.ptr + C, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipMemcpyAsync(&nf, foff.ptr + C, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (nv > vertex_cap || nf > face_cap) {
		set_error("invalid argument: the mesh has " + std::to_string(nv) + " vertices and " + std::to_string(nf) + " faces, the capacity is " +
		          std::to_string(vertex_cap) + " and " + std::to_string(face_cap));
		return NNRT_ERROR_ARGUMENT;
	}
	if (nf == 0) return NNRT_OK;   // then nv == 0 too: nothing to index
	if ((st = pixel_vertex.ensure(static_cast<size_t>(H) * W))) return st;
	k_scatter_vertices<<<gblocks(C), GB, 0, s>>>(pts, bits.ptr, H, W, voff.ptr, vertex_cap, vertices, pixels, pixel_vertex.ptr);
	NNRT_LAUNCH_CHECK();
	k_scatter_faces<<<gblocks(C), GB, 0, s>>>(bits.ptr, H, W, foff.ptr, face_cap, pixel_vertex.ptr, faces);
	NNRT_LAUNCH_CHECK();
	NNRT_HIP(hipStreamSynchronize(s));   // the scratch is freed on return
	*h_vertex_count = nv;
	*h_face_count = nf;
	return NNRT_OK;
}

nnrt_status launch_edges_shortest_path(const float* vertices, int64_t V, const uint8_t* mask, const int32_t* faces, int64_t F, const int32_t* node_vertex,
                                       int N, int K, float coverage, bool enforce, int32_t* edges, float* weights, float* distances,
                                       int32_t* h_passes, hipStream_t s) {
	if (h_passes) *h_passes = 0;
	const size_t NK = static_cast<size_t>(N) * K;
	NNRT_HIP(hipMemsetAsync(edges, 0xff, sizeof(int32_t) * NK, s));
	NNRT_HIP(hipMemsetAsync(weights, 0, sizeof(float) * NK, s));
	NNRT_HIP(hipMemsetAsync(distances, 0, sizeof(float) * NK, s));
	// the nodes on the host: range and duplicate checks, and the list of nodes that have a vertex
	std::vector<int32_t> h_nodes(N);
	NNRT_HIP(hipMemcpyAsync(h_nodes.data(), node_vertex, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	std::vector<int> pending;
	{
		std::vector<int32_t> used;
		for (int i = 0; i < N; i++) {
			if (h_nodes[i] < 0) continue;   // an all-default row, as in the reference
			if (h_nodes[i] >= V) {
				set_error("invalid argument: node " + std::to_string(i) + " has vertex index " + std::to_string(h_nodes[i]) + " outside [0, vertex_count)");
				return NNRT_ERROR_ARGUMENT;
			}
			pending.push_back(i);
			used.push_back(h_nodes[i]);
		}
		std::sort(used.begin(), used.end());
		if (std::adjacent_find(used.begin(), used.end()) != used.end()) {
			set_error("invalid argument: duplicate node vertex index " + std::to_string(*std::adjacent_find(used.begin(), used.end())));
			return NNRT_ERROR_ARGUMENT;
		}
	}
	nnrt_status st;
	// CSR adjacency over the unique directed vertex pairs of the faces
	const int64_t P = 6 * F;
	DeviceBuffer<uint64_t> keys, sorted, pairs;
	DeviceBuffer<uint8_t> flags, tmp;
	DeviceBuffer<int> ctrl, d_count, row_start, col, vertex_node;
	DeviceBuffer<float> len;
	if ((st = keys.ensure(P)) || (st = sorted.ensure(P)) || (st = pairs.ensure(P)) || (st = flags.ensure(P)) || (st = ctrl.ensure(1)) ||
	    (st = d_count.ensure(1)) || (st = row_start.ensure(V + 1)) || (st = vertex_node.ensure(V)))
		return st;
	NNRT_HIP(hipMemsetAsync(ctrl.ptr, 0, sizeof(int), s));
	int E = 0;
	if (F > 0) {
		k_face_pairs<<<gblocks(F), GB, 0, s>>>(faces, F, V, keys.ptr, ctrl.ptr);
		NNRT_LAUNCH_CHECK();
		if ((st = sort_keys(keys.ptr, sorted.ptr, P, 64, tmp, s))) return st;
		k_pair_flags<<<gblocks(P), GB, 0, s>>>(sorted.ptr, P, flags.ptr);
		NNRT_LAUNCH_CHECK();
		if ((st = select_flagged(sorted.ptr, flags.ptr, pairs.ptr, d_count.ptr, P, tmp, s))) return st;
		int err = 0;
		NNRT_HIP(hipMemcpyAsync(&E, d_count.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipMemcpyAsync(&err, ctrl.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));
		if (err) {
			set_error("invalid argument: face index outside [0, vertex_count) in compute_edges_shortest_path");
			return NNRT_ERROR_ARGUMENT;
		}
	}
	if (pending.empty()) return NNRT_OK;
	if ((st = col.ensure(E)) || (st = len.ensure(E))) return st;
	k_row_starts<<<gblocks(V + 1), GB, 0, s>>>(pairs.ptr, E, V, row_start.ptr);
	NNRT_LAUNCH_CHECK();
	if (E > 0) {
		k_pair_columns<<<gblocks(E), GB, 0, s>>>(pairs.ptr, E, vertices, col.ptr, len.ptr);
		NNRT_LAUNCH_CHECK();
	}
	NNRT_HIP(hipMemsetAsync(vertex_node.ptr, 0xff, sizeof(int) * V, s));
	k_vertex_nodes<<<gblocks(N), GB, 0, s>>>(node_vertex, N, vertex_node.ptr);
	NNRT_LAUNCH_CHECK();

	// B workgroup slots of 20 bytes per vertex and 8 per node each, within 1 GiB
	const size_t per_slot = 20 * static_cast<size_t>(V) + 8 * static_cast<size_t>(N);
	const int B = static_cast<int>(std::max<size_t>(1, std::min<size_t>(pending.size(), (size_t(1) << 30) / per_slot)));
	const size_t BV = static_cast<size_t>(B) * V;
	DeviceBuffer<unsigned> dist;
	DeviceBuffer<int> queued_round, reached, list_a, list_b, batch, found, cut;
	DeviceBuffer<unsigned long long> candidates;
	if ((st = dist.ensure(BV)) || (st = queued_round.ensure(BV)) || (st = reached.ensure(BV)) || (st = list_a.ensure(BV)) || (st = list_b.ensure(BV)) ||
	    (st = candidates.ensure(static_cast<size_t>(B) * N)) || (st = batch.ensure(N)) || (st = found.ensure(N)) || (st = cut.ensure(N)))
		return st;
	NNRT_HIP(hipMemsetAsync(dist.ptr, 0xff, sizeof(unsigned) * BV, s));
	NNRT_HIP(hipMemsetAsync(queued_round.ptr, 0, sizeof(int) * BV, s));
	GeodesicArgs a;
	a.node_vertex = node_vertex;
	a.V = V;
	a.N = N;
	a.K = K;
	a.row_start = row_start.ptr;
	a.col = col.ptr;
	a.len = len.ptr;
	a.mask = mask;
	a.vertex_node = vertex_node.ptr;
	a.coverage = coverage;
	a.dist = dist.ptr;
	a.queued_round = queued_round.ptr;
	a.reached = reached.ptr;
	a.list_a = list_a.ptr;
	a.list_b = list_b.ptr;
	a.candidates = candidates.ptr;
	a.edges = edges;
	a.weights = weights;
	a.distances = distances;
	a.found = found.ptr;
	a.cut = cut.ptr;
	// Bounded mode: one pass at R = 2 * coverage (graph_proc.cpp:212, :306). Enforced mode: the reference has no bound. A
	// pass at R reaches exactly the vertices with D <= R, at their final distances (file header), so a node that found K
	// other nodes has its K nearest, and one whose frontier met no refusal has everything it can reach; only the others
	// run again, from scratch, at 2 R. R reaches +inf after at most 2^8 doublings and +inf refuses nothing.
	float radius = 2.f * coverage;
	std::vector<int> h_found(N), h_cut(N);
	int passes = 0;
	while (!pending.empty()) {
		a.radius = radius;
		NNRT_HIP(hipMemcpyAsync(batch.ptr, pending.data(), sizeof(int) * pending.size(), hipMemcpyHostToDevice, s));
		for (size_t first = 0; first < pending.size(); first += B) {
			const int nb = static_cast<int>(std::min<size_t>(B, pending.size() - first));
			a.batch = batch.ptr + first;
			k_geodesic<<<nb, GB, 0, s>>>(a);
			NNRT_LAUNCH_CHECK();
		}
		passes++;
		NNRT_HIP(hipMemcpyAsync(h_found.data(), found.ptr, sizeof(int) * N, hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipMemcpyAsync(h_cut.data(), cut.ptr, sizeof(int) * N, hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));   // also: `pending` may change now
		if (!enforce || std::isinf(radius)) break;
		std::vector<int> again;
		for (int i : pending)
			if (h_found[i] < K && h_cut[i]) again.push_back(i);
		pending.swap(again);
		radius *= 2.f;
	}
	if (h_passes) *h_passes = passes;
	return NNRT_OK;   // the stream is idle: the scratch can go
}

// ------------------------------------------------- host-side graph passes ----
nnrt_status node_and_edge_clean_up_host(const int32_t* edges, int64_t N, int K, uint8_t* valid) {
	for (int64_t i = 0; i < N * K; i++) {
		if (edges[i] < -1 || edges[i] >= N) {
			set_error("invalid argument: graph edge " + std::to_string(edges[i]) + " outside [-1, node_count)");
			return NNRT_ERROR_ARGUMENT;
		}
	}
	// graph_proc.cpp:540-590: a live node with at most one live neighbour before its row's first -1 dies, until a pass
	// removes nothing. The reference tests a neighbour against the nodes removed by this call only (a node the caller
	// passed in as invalid still counts as a neighbour); so does this. Removals only lower counts, so the set removed at
	// the fixed point does not depend on the visiting order.
	std::vector<uint8_t> removed(N, 0);
	bool changed = true;
	while (changed) {
		changed = false;
		for (int64_t i = 0; i < N; i++) {
			if (!valid[i]) continue;
			int live = 0;
			for (int k = 0; k < K; k++) {
				const int32_t n = edges[i * K + k];
				if (n == -1) break;
				if (!removed[n]) live++;
			}
			if (live <= 1) {
				valid[i] = 0;
				removed[i] = 1;
				changed = true;
			}
		}
	}
	return NNRT_OK;
}

nnrt_status compute_clusters_host(const int32_t* edges, int64_t N, int K, int32_t* clusters, int32_t* sizes, int64_t* cluster_count) {
	*cluster_count = 0;
	std::vector<std::vector<int32_t>> neighbors(N);
	for (int64_t i = 0; i < N; i++) {
		for (int k = 0; k < K; k++) {
			const int32_t n = edges[i * K + k];
			if (n == -1) break;
			if (n < -1 || n >= N) {
				set_error("invalid argument: graph edge " + std::to_string(n) + " outside [-1, node_count)");
				return NNRT_ERROR_ARGUMENT;
			}
			neighbors[i].push_back(n);
			neighbors[n].push_back(static_cast<int32_t>(i));
		}
	}
	// graph_proc.cpp:510-636: components of the undirected graph, numbered by ascending lowest member
	std::fill(clusters, clusters + N, -1);
	std::vector<int32_t> stack;
	for (int64_t i = 0; i < N; i++) {
		if (clusters[i] != -1) continue;
		const int32_t id = static_cast<int32_t>(*cluster_count);
		int32_t size = 0;
		stack.assign(1, static_cast<int32_t>(i));
		clusters[i] = id;
		while (!stack.empty()) {
			const int32_t u = stack.back();
			stack.pop_back();
			size++;
			for (int32_t v : neighbors[u]) {
				if (clusters[v] == -1) {
					clusters[v] = id;
					stack.push_back(v);
				}
			}
		}
		sizes[(*cluster_count)++] = size;
	}
	return NNRT_OK;
}

} // namespace nnrt
