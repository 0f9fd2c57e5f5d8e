// Motion-graph node selection from a mesh on the GPU: the reference's two legacy CPU routines
//   * get_vertex_erosion_mask (cpp/cpu/graph_proc.cpp:27-90): faces start alive; iteration_count times, count per vertex the
//     alive faces touching it (integer atomics: order-independent) and kill every alive face with a vertex whose count is
//     below min_neighbors; a vertex is non-eroded iff an alive face touches it. One count and one cull kernel per iteration,
//     no host synchronisation inside the loop. Faces with an index outside [0, vertex_count) raise the device error flag
//     and are dead from the start, so no kernel ever dereferences such an index.
//   * sample_nodes (graph_proc.cpp:92-155): the sequential greedy loop "a vertex becomes a node iff no earlier node lies
//     within node_coverage", with ((dx*dx + dy*dy) + dz*dz) <= coverage*coverage in unfused f32 (-ffp-contract=off).
// The greedy node set is the lexicographically first maximal independent set of the "within coverage" graph over the
// candidates in priority order, which is unique, so it can be found in parallel rounds. Every candidate is UNDECIDED,
// ACCEPTED or REJECTED. In a round an undecided candidate c looks at the candidates of lower priority index within
// coverage: one ACCEPTED -> c is REJECTED; else one UNDECIDED -> c waits; else (all REJECTED, or none) -> c is ACCEPTED.
// States only move UNDECIDED -> ACCEPTED / REJECTED and both decisions are taken from final states only: a decision that
// can be taken at all is the sequential algorithm's (induction over the priority index), whatever the other lanes write
// meanwhile. The in-place update within a round is therefore safe (a stale read shows UNDECIDED and only postpones) and the
// fixed point is unique. The undecided candidate of lowest priority index sees only final states at the start of a round
// and is decided by it, so M candidates need at most M rounds; the host loops on the device-side undecided count and
// gives up with NNRT_ERROR_INTERNAL if a round decides nothing. No kernel waits on another workgroup.
// Neighbours are found through a uniform grid kept in O(candidates) memory: 64-bit cell keys (21 bits per axis, x lowest),
// a stable radix sort (each cell's members stay in ascending priority), binary search over the sorted keys. With x the
// lowest field the cells (cx-1 .. cx+1, cy+dy, cz+dz) are one contiguous run of the sorted order: the 27-cell neighbourhood
// is 9 runs, found once per candidate. Positions are gathered into sorted order once; a round's lanes are consecutive
// sorted positions, so a wave's lanes share their runs and the scan's loads are wave-uniform.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "device_primitives.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {
constexpr int GB = 256;   // threads per workgroup

constexpr uint8_t UNDECIDED = 0, ACCEPTED = 1, REJECTED = 2;

constexpr int ERR_ORDER_RANGE = 1, ERR_GRID_EXTENT = 2;

// Cell edge = coverage * (1 + 2^-20), cell coordinates in double. Two points a >= b (one axis) that pass the f32 test have
// RN(dx_f^2) <= RN(c*c) (adding the non-negative dy^2, dz^2 terms and rounding never lowers the sum), hence
// dx_f <= c (1 + u) and a - b <= c (1 + u)^2 with u = 2^-24 (c*c is required to be a normal float, so the bound survives
// an underflowing dx_f^2). The coordinate t(p) = (double(p) - double(min)) / edge carries a relative error below 2^-52
// (two double roundings), on t < 2^21: t(a) - t(b) < (a - b) / edge + 2^-30. With edge = c (1 + 2^-20):
// (1 + 2^-23 + 2^-48) / (1 + 2^-20) + 2^-30 < 1, so floor(t(a)) - floor(t(b)) <= 1 (t is monotone in p): two points within
// coverage are never more than one cell apart on any axis.
constexpr double CELL_MARGIN = 1.0 + 0x1p-20;
constexpr int CELL_BITS = 21;
constexpr double CELL_MAX = static_cast<double>((1 << CELL_BITS) - 3);   // stored as cell + 1; cell + 2 still fits the field

unsigned gblocks(int64_t n) { return static_cast<unsigned>(ceil_div(n, GB)); }

// ---------------------------------------------------------------- erosion ----
__global__ __launch_bounds__(GB) void k_faces_init(const int64_t* __restrict__ faces, int64_t F, int64_t V, uint8_t* __restrict__ alive,
                                                   int* __restrict__ error_flag) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (f >= F) return;
	const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
	const bool ok = a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
	alive[f] = ok ? 1 : 0;
	if (!ok) atomicOr(error_flag, 1);
}

__global__ __launch_bounds__(GB) void k_faces_count(const int64_t* __restrict__ faces, int64_t F, const uint8_t* __restrict__ alive,
                                                    int* __restrict__ counts) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (f >= F || !alive[f]) return;   // alive faces have in-range indices (k_faces_init)
	atomicAdd(counts + faces[3 * f], 1);
	atomicAdd(counts + faces[3 * f + 1], 1);
	atomicAdd(counts + faces[3 * f + 2], 1);
}

__global__ __launch_bounds__(GB) void k_faces_cull(const int64_t* __restrict__ faces, int64_t F, const int* __restrict__ counts, int min_neighbors,
                                                   uint8_t* __restrict__ alive) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (f >= F || !alive[f]) return;
	if (counts[faces[3 * f]] < min_neighbors || counts[faces[3 * f + 1]] < min_neighbors || counts[faces[3 * f + 2]] < min_neighbors) alive[f] = 0;
}

__global__ __launch_bounds__(GB) void k_faces_mark(const int64_t* __restrict__ faces, int64_t F, const uint8_t* __restrict__ alive,
                                                   uint8_t* __restrict__ mask) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (f >= F || !alive[f]) return;
	mask[faces[3 * f]] = 1;   // every writer stores the same value
	mask[faces[3 * f + 1]] = 1;
	mask[faces[3 * f + 2]] = 1;
}

// --------------------------------------------------------------- sampling ----
// order-preserving float <-> unsigned map (for atomicMin over finite floats)
__device__ inline unsigned ordered_bits(float v) {
	const unsigned b = __float_as_uint(v);
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float from_ordered_bits(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// priority position i -> vertex (order[i] or i) and whether it is a candidate (masked in, finite coordinates)
__global__ __launch_bounds__(GB) void k_candidate_flags(const float* __restrict__ pts, int64_t V, const uint8_t* __restrict__ mask,
                                                        const int64_t* __restrict__ order, int64_t* __restrict__ vertex, uint8_t* __restrict__ flags,
                                                        int* __restrict__ error_flag) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * GB + threadIdx.x;
	if (i >= V) return;
	int64_t v = order ? order[i] : i;
	bool ok = true;
	if (v < 0 || v >= V) {
		atomicOr(error_flag, ERR_ORDER_RANGE);
		v = 0;
		ok = false;
	}
	vertex[i] = v;
	if (ok && mask) ok = mask[v] != 0;
	if (ok) ok = isfinite(pts[3 * v]) && isfinite(pts[3 * v + 1]) && isfinite(pts[3 * v + 2]);
	flags[i] = ok ? 1 : 0;
}

__device__ inline unsigned wave_min(unsigned v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = min(v, static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, 64)));
	return v;
}

// bounding-box minimum of the candidates, as ordered bits (lo[] starts at 0xffffffff)
__global__ __launch_bounds__(GB) void k_bbox_min(const float* __restrict__ pts, const int64_t* __restrict__ cand, int M, unsigned* __restrict__ lo) {
	const int j = blockIdx.x * GB + threadIdx.x;
	unsigned x = 0xffffffffu, y = 0xffffffffu, z = 0xffffffffu;
	if (j < M) {
		const int64_t v = cand[j];
		x = ordered_bits(pts[3 * v]);
		y = ordered_bits(pts[3 * v + 1]);
		z = ordered_bits(pts[3 * v + 2]);
	}
	x = wave_min(x);
	y = wave_min(y);
	z = wave_min(z);
	if ((threadIdx.x & 63) == 0) {
		atomicMin(lo, x);
		atomicMin(lo + 1, y);
		atomicMin(lo + 2, z);
	}
}

__device__ inline uint64_t cell_key(uint32_t fx, uint32_t fy, uint32_t fz) {
	return static_cast<uint64_t>(fx) | (static_cast<uint64_t>(fy) << CELL_BITS) | (static_cast<uint64_t>(fz) << (2 * CELL_BITS));
}

// keys[j] = cell key of candidate j (fields hold cell + 1, so a neighbour's cell - 1 is never negative); prio[j] = j
__global__ __launch_bounds__(GB) void k_cell_keys(const float* __restrict__ pts, const int64_t* __restrict__ cand, int M,
                                                  const unsigned* __restrict__ lo, double edge, uint64_t* __restrict__ keys, int* __restrict__ prio,
                                                  int* __restrict__ error_flag) {
	const int j = blockIdx.x * GB + threadIdx.x;
	if (j >= M) return;
	const int64_t v = cand[j];
	uint32_t f[3];
	bool ok = true;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const double t = floor((static_cast<double>(pts[3 * v + a]) - static_cast<double>(from_ordered_bits(lo[a]))) / edge);
		if (!(t >= 0.0 && t <= CELL_MAX)) ok = false;
		f[a] = ok ? static_cast<uint32_t>(t) + 1u : 1u;
	}
	if (!ok) atomicOr(error_flag, ERR_GRID_EXTENT);
	keys[j] = ok ? cell_key(f[0], f[1], f[2]) : cell_key(1, 1, 1);
	prio[j] = j;
}

// sorted position s -> (x, y, z, priority) of its candidate; state UNDECIDED; the first round's work list 0 .. M-1
__global__ __launch_bounds__(GB) void k_gather_sorted(const float* __restrict__ pts, const int64_t* __restrict__ cand, const int* __restrict__ prio_sorted,
                                                      int M, float4* __restrict__ pos, uint8_t* __restrict__ state, int* __restrict__ list) {
	const int s = blockIdx.x * GB + threadIdx.x;
	if (s >= M) return;
	const int p = prio_sorted[s];
	const int64_t v = cand[p];
	pos[s] = make_float4(pts[3 * v], pts[3 * v + 1], pts[3 * v + 2], __int_as_float(p));
	state[s] = UNDECIDED;
	list[s] = s;
}

__device__ inline int lower_bound_key(const uint64_t* __restrict__ keys, int n, uint64_t k) {   // first index with keys[i] >= k
	int lo = 0, hi = n;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (keys[mid] < k) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// runs[r * M + s] = [begin, end) in sorted order of the cells (cx-1 .. cx+1, cy + r % 3 - 1, cz + r / 3 - 1)
__global__ __launch_bounds__(GB) void k_cell_runs(const uint64_t* __restrict__ keys, int M, int2* __restrict__ runs) {
	const int s = blockIdx.x * GB + threadIdx.x;
	if (s >= M) return;
	const uint64_t k = keys[s];
	const uint32_t m = (1u << CELL_BITS) - 1u;
	const uint32_t fx = static_cast<uint32_t>(k) & m, fy = static_cast<uint32_t>(k >> CELL_BITS) & m, fz = static_cast<uint32_t>(k >> (2 * CELL_BITS)) & m;
#pragma unroll
	for (int r = 0; r < 9; r++) {
		const uint32_t y = fy + (r % 3) - 1, z = fz + (r / 3) - 1;   // fields are in [1, 2^21 - 2]: no wrap
		const int b = lower_bound_key(keys, M, cell_key(fx - 1, y, z));
		const int e = lower_bound_key(keys, M, cell_key(fx + 1, y, z) + 1);
		runs[static_cast<int64_t>(r) * M + s] = make_int2(b, e);
	}
}

// one round over the undecided candidates list[0 .. n): see the file header. still[j] = 1 iff list[j] stays undecided.
__global__ __launch_bounds__(GB) void k_round(const int* __restrict__ list, int n, const float4* __restrict__ pos, uint8_t* state,
                                              const int2* __restrict__ runs, int M, float coverage_sq, uint8_t* __restrict__ still) {
	const int j = blockIdx.x * GB + threadIdx.x;
	if (j >= n) return;
	const int s = list[j];
	const float4 me = pos[s];
	const int my_prio = __float_as_int(me.w);
	bool rejected = false, blocked = false;
	for (int r = 0; r < 9 && !rejected; r++) {
		const int2 run = runs[static_cast<int64_t>(r) * M + s];
		for (int t = run.x; t < run.y; t++) {
			// the state byte first: in the later rounds nearly every member is REJECTED and its position is never loaded
			const uint8_t st = __hip_atomic_load(state + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (st == REJECTED) continue;
			const float4 q = pos[t];
			if (__float_as_int(q.w) >= my_prio) continue;
			const float dx = me.x - q.x, dy = me.y - q.y, dz = me.z - q.z;
			if (!(((dx * dx + dy * dy) + dz * dz) <= coverage_sq)) continue;
			if (st == ACCEPTED) {
				rejected = true;
				break;
			}
			blocked = true;
		}
	}
	const bool undecided = !rejected && blocked;
	if (!undecided) __hip_atomic_store(state + s, rejected ? REJECTED : ACCEPTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	still[j] = undecided ? 1 : 0;
}

// accepted[priority] = 1 iff the candidate was accepted
__global__ __launch_bounds__(GB) void k_accepted_by_priority(const float4* __restrict__ pos, const uint8_t* __restrict__ state, int M,
                                                             uint8_t* __restrict__ accepted) {
	const int s = blockIdx.x * GB + threadIdx.x;
	if (s >= M) return;
	accepted[__float_as_int(pos[s].w)] = state[s] == ACCEPTED ? 1 : 0;
}
} // namespace

nnrt_status launch_vertex_erosion_mask(int64_t V, const int64_t* faces, int64_t F, int iteration_count, int min_neighbors, uint8_t* mask,
                                       int* error_flag, hipStream_t s) {
	DeviceBuffer<uint8_t> alive;
	DeviceBuffer<int> counts;
	nnrt_status st;
	if ((st = alive.ensure(F)) || (st = counts.ensure(V))) return st;
	NNRT_HIP(hipMemsetAsync(mask, 0, V, s));
	k_faces_init<<<gblocks(F), GB, 0, s>>>(faces, F, V, alive.ptr, error_flag);
	NNRT_LAUNCH_CHECK();
	for (int i = 0; i < iteration_count; i++) {
		NNRT_HIP(hipMemsetAsync(counts.ptr, 0, sizeof(int) * V, s));
		k_faces_count<<<gblocks(F), GB, 0, s>>>(faces, F, alive.ptr, counts.ptr);
		NNRT_LAUNCH_CHECK();
		k_faces_cull<<<gblocks(F), GB, 0, s>>>(faces, F, counts.ptr, min_neighbors, alive.ptr);
		NNRT_LAUNCH_CHECK();
	}
	k_faces_mark<<<gblocks(F), GB, 0, s>>>(faces, F, alive.ptr, mask);
	NNRT_LAUNCH_CHECK();
	NNRT_HIP(hipStreamSynchronize(s));   // the scratch is freed on return
	return NNRT_OK;
}

nnrt_status launch_sample_nodes(const float* pts, int64_t V, const uint8_t* mask, const int64_t* order, float coverage, int64_t* out,
                                int64_t* h_count, int32_t* h_rounds, hipStream_t s) {
	*h_count = 0;
	if (h_rounds) *h_rounds = 0;
	DeviceBuffer<int64_t> vertex, cand, d_count;
	DeviceBuffer<uint8_t> flags, tmp;
	DeviceBuffer<int> ctrl;
	nnrt_status st;
	if ((st = vertex.ensure(V)) || (st = cand.ensure(V)) || (st = d_count.ensure(1)) || (st = flags.ensure(V)) || (st = ctrl.ensure(4))) return st;
	NNRT_HIP(hipMemsetAsync(ctrl.ptr, 0, 4 * sizeof(int), s));
	k_candidate_flags<<<gblocks(V), GB, 0, s>>>(pts, V, mask, order, vertex.ptr, flags.ptr, ctrl.ptr);
	NNRT_LAUNCH_CHECK();
	// stable compaction: a candidate's priority is its position in `cand`
	if ((st = select_flagged(vertex.ptr, flags.ptr, cand.ptr, d_count.ptr, V, tmp, s))) return st;
	int64_t M64 = 0;
	int err = 0;
	NNRT_HIP(hipMemcpyAsync(&M64, d_count.ptr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipMemcpyAsync(&err, ctrl.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (err & ERR_ORDER_RANGE) {
		set_error("invalid argument: d_order holds an index outside [0, point_count)");
		return NNRT_ERROR_ARGUMENT;
	}
	const int M = static_cast<int>(M64);
	if (M == 0) return NNRT_OK;

	DeviceBuffer<unsigned> lo;
	DeviceBuffer<uint64_t> keys, keys_sorted;
	DeviceBuffer<int> prio, prio_sorted, list_a, list_b;
	DeviceBuffer<float4> pos;
	DeviceBuffer<uint8_t> state, still;
	DeviceBuffer<int2> runs;
	if ((st = lo.ensure(4)) || (st = keys.ensure(M)) || (st = keys_sorted.ensure(M)) || (st = prio.ensure(M)) || (st = prio_sorted.ensure(M)) ||
	    (st = list_a.ensure(M)) || (st = list_b.ensure(M)) || (st = pos.ensure(M)) || (st = state.ensure(M)) || (st = still.ensure(M)) ||
	    (st = runs.ensure(9 * static_cast<size_t>(M))))
		return st;
	NNRT_HIP(hipMemsetAsync(lo.ptr, 0xff, 4 * sizeof(unsigned), s));
	k_bbox_min<<<gblocks(M), GB, 0, s>>>(pts, cand.ptr, M, lo.ptr);
	NNRT_LAUNCH_CHECK();
	const double edge = static_cast<double>(coverage) * CELL_MARGIN;
	k_cell_keys<<<gblocks(M), GB, 0, s>>>(pts, cand.ptr, M, lo.ptr, edge, keys.ptr, prio.ptr, ctrl.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = sort_pairs(keys.ptr, keys_sorted.ptr, prio.ptr, prio_sorted.ptr, M, 3 * CELL_BITS, tmp, s))) return st;
	k_gather_sorted<<<gblocks(M), GB, 0, s>>>(pts, cand.ptr, prio_sorted.ptr, M, pos.ptr, state.ptr, list_a.ptr);
	NNRT_LAUNCH_CHECK();
	k_cell_runs<<<gblocks(M), GB, 0, s>>>(keys_sorted.ptr, M, runs.ptr);
	NNRT_LAUNCH_CHECK();
	NNRT_HIP(hipMemcpyAsync(&err, ctrl.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (err & ERR_GRID_EXTENT) {
		set_error("invalid argument: the candidates' extent exceeds 2^21 - 3 cells of node_coverage along an axis");
		return NNRT_ERROR_ARGUMENT;
	}

	const float coverage_sq = coverage * coverage;
	int* list = list_a.ptr;
	int* next = list_b.ptr;
	int undecided = M, rounds = 0;
	while (undecided > 0) {
		if (rounds >= M) {
			set_error("internal error: node sampling did not reach its fixed point within one round per candidate");
			return NNRT_ERROR_INTERNAL;
		}
		k_round<<<gblocks(undecided), GB, 0, s>>>(list, undecided, pos.ptr, state.ptr, runs.ptr, M, coverage_sq, still.ptr);
		NNRT_LAUNCH_CHECK();
		rounds++;
		if ((st = select_flagged(list, still.ptr, next, d_count.ptr, undecided, tmp, s))) return st;
		int64_t left = 0;
		NNRT_HIP(hipMemcpyAsync(&left, d_count.ptr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));
		if (left >= undecided) {
			set_error("internal error: a node sampling round decided no candidate");
			return NNRT_ERROR_INTERNAL;
		}
		undecided = static_cast<int>(left);
		std::swap(list, next);
	}
	// `flags` (capacity V >= M) is free again: accepted flag per priority, then the vertices in priority order
	k_accepted_by_priority<<<gblocks(M), GB, 0, s>>>(pos.ptr, state.ptr, M, flags.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = select_flagged(cand.ptr, flags.ptr, out, d_count.ptr, M, tmp, s))) return st;
	NNRT_HIP(hipMemcpyAsync(h_count, d_count.ptr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (h_rounds) *h_rounds = rounds;
	return NNRT_OK;
}

} // namespace nnrt
