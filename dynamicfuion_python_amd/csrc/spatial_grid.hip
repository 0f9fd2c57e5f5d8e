// Uniform-grid point index: the grid down-samplers of nnrt.geometry.functional
// (cpp/geometry/functional/kernel/GeometrySamplingMean.h, GeometrySamplingMedian.h over GeometrySamplingGridBinning.h:27-53)
// and an exact K-NN over the same index for nnrt.core.KDTree (cpp/core/KdTree.h FindKNearestToPoints).
//
// Cell index. The cell of a point is floorf(p / cell + offset) per component (GeometrySamplingGridBinning.h:39-40, float32,
// no contraction). The three coordinates, biased by 2^20, pack into one 64-bit key (x lowest, 21 bits each). A stable
// radix sort of (key, point index) groups the members of a cell in ascending point order; segment heads are scanned into
// the cell table (key, start; the next start is the end) and a scan of "is the first member of its cell" over the original
// point order gives every cell its output rank: cells are numbered by their smallest member index. The sorted points are
// kept as float4 (x, y, z, original index bits), so the per-cell kernels and the K-NN read members contiguously.
//
// Per-cell kernels: one wavefront per cell, lanes striding the members (a cell of more than 64 members takes several
// rounds). K-NN: one lane per query, the K best candidates in registers (see k_knn_rows in hierarchy.hip), walking shells
// of cells of growing Chebyshev radius around the query's cell. Every output element is written by plain vector stores.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "device_primitives.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {
constexpr int GB = 256;                       // threads per workgroup
constexpr int WAVES = GB / 64;                // cells per workgroup of the per-cell kernels
constexpr int CELL_BITS = 21;
constexpr int CELL_BIAS = 1 << (CELL_BITS - 1);   // cell coordinates lie in [-2^20, 2^20 - 1]
constexpr int KNN_MAX = NNRT_POINT_INDEX_MAX_K;
constexpr int ERR_NOT_FINITE = 1, ERR_CELL_RANGE = 2;

unsigned gblocks(int64_t n) { return static_cast<unsigned>(ceil_div(std::max<int64_t>(n, 1), GB)); }

__host__ __device__ inline uint64_t cell_key(uint32_t x, uint32_t y, uint32_t z) {
	return static_cast<uint64_t>(x) | (static_cast<uint64_t>(y) << CELL_BITS) | (static_cast<uint64_t>(z) << (2 * CELL_BITS));
}

// keys[i] = packed cell of point i, order[i] = i. A non-finite coordinate or a cell outside the 21-bit range raises the flag.
__global__ __launch_bounds__(GB) void k_index_keys(const float* __restrict__ pts, int n, float cell, float ox, float oy, float oz,
                                                   uint64_t* __restrict__ keys, int* __restrict__ order, int* __restrict__ error_flag) {
	const int i = blockIdx.x * GB + threadIdx.x;
	if (i >= n) return;
	const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
	const float o[3] = {ox, oy, oz};
	uint32_t f[3];
	int err = 0;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const float t = floorf(p[a] / cell + o[a]);
		if (!isfinite(p[a])) err |= ERR_NOT_FINITE;
		else if (!(t >= -static_cast<float>(CELL_BIAS) && t <= static_cast<float>(CELL_BIAS - 1))) err |= ERR_CELL_RANGE;
		f[a] = err ? 0u : static_cast<uint32_t>(static_cast<int>(t) + CELL_BIAS);
	}
	if (err) atomicOr(error_flag, err);
	keys[i] = err ? 0ull : cell_key(f[0], f[1], f[2]);
	order[i] = i;
}

// head[s] = 1 iff sorted position s starts a cell; first[i] = 1 iff point i is its cell's first (smallest-index) member
__global__ __launch_bounds__(GB) void k_index_heads(const uint64_t* __restrict__ keys_sorted, const int* __restrict__ order_sorted, int n,
                                                    int* __restrict__ head, int* __restrict__ first) {
	const int s = blockIdx.x * GB + threadIdx.x;
	if (s >= n) return;
	const int h = (s == 0 || keys_sorted[s] != keys_sorted[s - 1]) ? 1 : 0;
	head[s] = h;
	first[order_sorted[s]] = h;
}

// the sorted points, and per cell c (in key order): its key, its first sorted position and its output rank.
// ctrl[1] = cell count; cell_start[cell count] = n.
__global__ __launch_bounds__(GB) void k_index_cells(const float* __restrict__ pts, const uint64_t* __restrict__ keys_sorted,
                                                    const int* __restrict__ order_sorted, const int* __restrict__ head,
                                                    const int* __restrict__ head_scan, const int* __restrict__ first_scan, int n,
                                                    float4* __restrict__ pos, uint64_t* __restrict__ cell_keys, int* __restrict__ cell_start,
                                                    int* __restrict__ cell_rank, int* __restrict__ ctrl) {
	const int s = blockIdx.x * GB + threadIdx.x;
	if (s >= n) return;
	const int i = order_sorted[s];
	pos[s] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float(i));
	const int c = head_scan[s];
	if (head[s]) {
		cell_keys[c] = keys_sorted[s];
		cell_start[c] = s;
		cell_rank[c] = first_scan[i];
	}
	if (s == n - 1) {
		const int count = c + head[s];
		ctrl[1] = count;
		cell_start[count] = n;
	}
}

__device__ inline double wave_sum(double v) {   // butterfly: every lane adds the same pairs in the same order
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// the smaller of (d, i) pairs, lexicographic, over the wavefront
__device__ inline void wave_min_pair(float& d, int& i) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const float od = __shfl_xor(d, o, 64);
		const int oi = __shfl_xor(i, o, 64);
		const bool take = od < d || (od == d && oi < i);
		d = take ? od : d;
		i = take ? oi : i;
	}
}

// Mean of every cell: float64 partial sums per lane, combined across lanes in a fixed order, divided in float64 and
// rounded once. CLOSEST = false: means[rank] = the mean. CLOSEST = true: flags[i] = 1 for the member i with the smallest
// (dx*dx + dy*dy) + dz*dz (float32) to the float32 mean, ties to the lower point index.
template <bool CLOSEST>
__global__ __launch_bounds__(GB) void k_cell_mean(const float4* __restrict__ pos, const int* __restrict__ cell_start,
                                                  const int* __restrict__ cell_rank, int cells, float* __restrict__ means,
                                                  uint8_t* __restrict__ flags) {
	const int c = blockIdx.x * WAVES + (threadIdx.x >> 6);
	if (c >= cells) return;   // whole wavefronts leave together
	const int lane = threadIdx.x & 63;
	const int begin = cell_start[c], end = cell_start[c + 1];
	double sx = 0.0, sy = 0.0, sz = 0.0;
	for (int t = begin + lane; t < end; t += 64) {
		const float4 p = pos[t];
		sx += static_cast<double>(p.x);
		sy += static_cast<double>(p.y);
		sz += static_cast<double>(p.z);
	}
	const double m = static_cast<double>(end - begin);
	const float mx = static_cast<float>(wave_sum(sx) / m), my = static_cast<float>(wave_sum(sy) / m), mz = static_cast<float>(wave_sum(sz) / m);
	if constexpr (!CLOSEST) {
		if (lane == 0) {
			const int64_t r = cell_rank[c];
			means[3 * r] = mx;
			means[3 * r + 1] = my;
			means[3 * r + 2] = mz;
		}
	} else {
		float best = INFINITY;
		int best_i = INT_MAX;
		for (int t = begin + lane; t < end; t += 64) {
			const float4 p = pos[t];
			const float dx = p.x - mx, dy = p.y - my, dz = p.z - mz;
			const float d = (dx * dx + dy * dy) + dz * dz;
			const int i = __float_as_int(p.w);
			if (d < best || (d == best && i < best_i)) {
				best = d;
				best_i = i;
			}
		}
		wave_min_pair(best, best_i);
		// no member compares (a NaN distance needs a non-finite mean, which finite members cannot give): the first member
		if (best_i == INT_MAX) best_i = __float_as_int(pos[begin].w);
		if (lane == 0) flags[best_i] = 1;
	}
}

// Medoid of every cell, as k_medoid_sums / k_medoid_flags (hierarchy.hip) define it: sum_a = sum over the members b, in
// ascending point order, of sqrtf((dx*dx + dy*dy) + dz*dz); the first member with the smallest sum below FLT_MAX, else the
// cell's first member. A lane owns one candidate a and adds over b sequentially, so the sum's order is the restatement's.
__global__ __launch_bounds__(GB) void k_cell_medoid(const float4* __restrict__ pos, const int* __restrict__ cell_start, int cells,
                                                    uint8_t* __restrict__ flags) {
	const int c = blockIdx.x * WAVES + (threadIdx.x >> 6);
	if (c >= cells) return;
	const int lane = threadIdx.x & 63;
	const int begin = cell_start[c], end = cell_start[c + 1];
	float best = INFINITY;
	int best_i = INT_MAX;
	for (int base = begin; base < end; base += 64) {
		const int a = base + lane;
		const bool live = a < end;
		const float4 pa = pos[live ? a : begin];
		float sum = 0.f;
		for (int b = begin; b < end; b++) {
			const float4 pb = pos[b];   // one address per wavefront
			const float dx = pb.x - pa.x, dy = pb.y - pa.y, dz = pb.z - pa.z;
			sum += sqrtf((dx * dx + dy * dy) + dz * dz);
		}
		const int i = __float_as_int(pa.w);
		if (live && sum < FLT_MAX && (sum < best || (sum == best && i < best_i))) {
			best = sum;
			best_i = i;
		}
	}
	wave_min_pair(best, best_i);
	if (best_i == INT_MAX) best_i = __float_as_int(pos[begin].w);
	if (lane == 0) flags[best_i] = 1;
}

// ------------------------------------------------------------------ K-NN ----
__device__ inline unsigned ordered_bits(float v) {   // order-preserving float -> unsigned map
	const unsigned b = __float_as_uint(v);
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float from_ordered_bits(unsigned o) {
	const unsigned b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
	float v;
	memcpy(&v, &b, sizeof(v));
	return v;
}
__device__ inline unsigned wave_min_u(unsigned v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = min(v, static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, 64)));
	return v;
}
__device__ inline unsigned wave_max_u(unsigned v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, 64)));
	return v;
}

// box[0..2] = minimum, box[3..5] = maximum of the points, as ordered bits (box starts at 0xffffffff x 3, 0 x 3);
// a non-finite coordinate raises the flag
__global__ __launch_bounds__(GB) void k_bounding_box(const float* __restrict__ pts, int n, unsigned* __restrict__ box, int* __restrict__ error_flag) {
	const int i = blockIdx.x * GB + threadIdx.x;
	unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
	if (i < n) {
		bool finite = true;
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const float v = pts[3 * i + a];
			finite = finite && isfinite(v);
			lo[a] = hi[a] = ordered_bits(v);
		}
		if (!finite) atomicOr(error_flag, ERR_NOT_FINITE);
	}
#pragma unroll
	for (int a = 0; a < 3; a++) {
		lo[a] = wave_min_u(lo[a]);
		hi[a] = wave_max_u(hi[a]);
	}
	if ((threadIdx.x & 63) == 0) {
#pragma unroll
		for (int a = 0; a < 3; a++) {
			atomicMin(box + a, lo[a]);
			atomicMax(box + 3 + a, hi[a]);
		}
	}
}

struct IndexView {
	const float4* pos;
	const uint64_t* cell_keys;
	const int* cell_start;
	int cells;
	float cell;
	int lo[3], hi[3];   // biased cell coordinates of the bounding box's corners: every occupied cell lies between them
};

__device__ inline int lower_bound_key(const uint64_t* __restrict__ keys, int n, uint64_t k) {   // first index with keys[i] >= k
	int lo = 0, hi = n;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (keys[mid] < k) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// the K best candidates by (squared distance, index), ascending, in registers (static indices only)
struct Best {
	float d[KNN_MAX];
	int i[KNN_MAX];
	float worst_d;
	int worst_i;
};

__device__ __forceinline__ void best_insert(Best& b, int k, float d, int idx) {
	if (!(d < b.worst_d || (d == b.worst_d && idx < b.worst_i))) return;
	float cd = d;
	int ci = idx;
	bool shifting = false;
#pragma unroll
	for (int q = 0; q < KNN_MAX; q++) {   // insertion: every slot from the insertion point on moves one down
		const bool take = q < k && (shifting || cd < b.d[q] || (cd == b.d[q] && ci < b.i[q]));
		shifting = take;
		const float td = b.d[q];
		const int ti = b.i[q];
		b.d[q] = take ? cd : td;
		b.i[q] = take ? ci : ti;
		cd = take ? td : cd;
		ci = take ? ti : ci;
	}
#pragma unroll
	for (int q = 0; q < KNN_MAX; q++)   // slot k - 1 by a static-index select chain (no scratch indexing)
		if (q == k - 1) {
			b.worst_d = b.d[q];
			b.worst_i = b.i[q];
		}
}

// the members of the cells (x0 .. x1, y, z): one contiguous run of the sorted points, x being the key's lowest field
__device__ __forceinline__ void scan_row(const IndexView& v, int x0, int x1, int y, int z, float qx, float qy, float qz, int k, Best& b) {
	const int ca = lower_bound_key(v.cell_keys, v.cells, cell_key(x0, y, z));
	const int cb = lower_bound_key(v.cell_keys, v.cells, cell_key(x1, y, z) + 1);
	if (ca >= cb) return;
	const int begin = v.cell_start[ca], end = v.cell_start[cb];
	for (int t = begin; t < end; t++) {
		const float4 p = v.pos[t];
		const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
		best_insert(b, k, (dx * dx + dy * dy) + dz * dz, __float_as_int(p.w));
	}
}

// Exact K nearest points of every query, one lane per query. Shell r holds the cells at Chebyshev distance r from the
// query's cell (clamped into the index's cell range). After shell r, every unvisited point lies in a cell that is at
// least r + 1 cells away along some axis, hence beyond one of the six planes bounding the visited box. A cell K holds
// the points with K <= RN(p / cell) < K + 1, so a plane sits at K * cell up to the quotient's rounding: it is moved
// towards the query by |K * cell| * 2^-22 and a sliver for the subnormal range, the squared gap is shrunk by 2^-18 (far
// above the float32 rounding of the squared distance it is compared with) and by 2^-120 (underflowing squares). The
// search stops only when K candidates are held and that bound exceeds the K-th squared distance, so rounding can only
// make it go on; it also ends when the shells have covered the index's whole cell range.
__global__ __launch_bounds__(GB) void k_knn_query(IndexView v, const float* __restrict__ queries, int Q, int k, int32_t* __restrict__ out_i,
                                                  float* __restrict__ out_d) {
	const int s = blockIdx.x * GB + threadIdx.x;
	if (s >= Q) return;
	const float q[3] = {queries[3 * s], queries[3 * s + 1], queries[3 * s + 2]};
	int qc[3];
	int reach = 0;   // the largest shell radius that still meets the cell range
#pragma unroll
	for (int a = 0; a < 3; a++) {
		float t = floorf(q[a] / v.cell + 0.f);
		t = fminf(fmaxf(t, static_cast<float>(v.lo[a] - CELL_BIAS)), static_cast<float>(v.hi[a] - CELL_BIAS));   // NaN -> lo
		qc[a] = static_cast<int>(t) + CELL_BIAS;
		reach = max(reach, max(qc[a] - v.lo[a], v.hi[a] - qc[a]));
	}
	Best b;
#pragma unroll
	for (int j = 0; j < KNN_MAX; j++) {
		b.d[j] = INFINITY;
		b.i[j] = INT_MAX;
	}
	b.worst_d = INFINITY;
	b.worst_i = INT_MAX;
	const double cell = static_cast<double>(v.cell);
	for (int r = 0; r <= reach; r++) {
		const int z0 = max(qc[2] - r, v.lo[2]), z1 = min(qc[2] + r, v.hi[2]);
		const int y0 = max(qc[1] - r, v.lo[1]), y1 = min(qc[1] + r, v.hi[1]);
		const int x0 = max(qc[0] - r, v.lo[0]), x1 = min(qc[0] + r, v.hi[0]);
		for (int z = z0; z <= z1; z++) {
			for (int y = y0; y <= y1; y++) {
				if (abs(z - qc[2]) == r || abs(y - qc[1]) == r) {
					scan_row(v, x0, x1, y, z, q[0], q[1], q[2], k, b);
				} else {   // an inner row of the shell: its two end cells
					if (qc[0] - r >= v.lo[0]) scan_row(v, qc[0] - r, qc[0] - r, y, z, q[0], q[1], q[2], k, b);
					if (qc[0] + r <= v.hi[0]) scan_row(v, qc[0] + r, qc[0] + r, y, z, q[0], q[1], q[2], k, b);
				}
			}
		}
		if (b.worst_i == INT_MAX) continue;   // fewer than k candidates held
		double gap = INFINITY;
#pragma unroll
		for (int a = 0; a < 3; a++) {
			if (qc[a] + r + 1 <= v.hi[a]) {   // cells qc + r + 1 and up: p >= plane
				const double plane = static_cast<double>(qc[a] + r + 1 - CELL_BIAS) * cell;
				gap = fmin(gap, fmax((plane - (fabs(plane) * 0x1p-22 + cell * 0x1p-140)) - static_cast<double>(q[a]), 0.0));
			}
			if (qc[a] - r - 1 >= v.lo[a]) {   // cells qc - r - 1 and down: p < plane
				const double plane = static_cast<double>(qc[a] - r - CELL_BIAS) * cell;
				gap = fmin(gap, fmax(static_cast<double>(q[a]) - (plane + (fabs(plane) * 0x1p-22 + cell * 0x1p-140)), 0.0));
			}
		}
		if (gap * gap * (1.0 - 0x1p-18) - 0x1p-120 > static_cast<double>(b.worst_d)) break;
	}
#pragma unroll
	for (int j = 0; j < KNN_MAX; j++) {
		if (j < k) {
			const bool held = b.i[j] != INT_MAX;
			out_i[static_cast<int64_t>(s) * k + j] = held ? b.i[j] : -1;
			out_d[static_cast<int64_t>(s) * k + j] = held ? sqrtf(b.d[j]) : INFINITY;
		}
	}
}

// ------------------------------------------------------------- host side ----
struct CellIndex {
	int n = 0, cells = 0;
	float cell = 0.f;
	DeviceBuffer<float4> pos;
	DeviceBuffer<uint64_t> cell_keys;
	DeviceBuffer<int> cell_start, cell_rank;
	DeviceBuffer<int> ctrl;   // [0] error flag, [1] cell count
};

nnrt_status raise_index_error(int err) {
	if (err & ERR_NOT_FINITE) set_error("invalid argument: points hold a non-finite coordinate");
	else set_error("invalid argument: a point's grid cell lies outside [-2^20, 2^20) along an axis (grid_cell_size too small for the coordinates)");
	return NNRT_ERROR_ARGUMENT;
}

// Builds the index of n >= 1 points on stream s and waits for it: the cell count is the one value read back.
nnrt_status build_cell_index(CellIndex& ix, const float* pts, int n, float cell, const float* offset, hipStream_t s) {
	ix.n = n;
	ix.cells = 0;
	ix.cell = cell;
	DeviceBuffer<uint64_t> keys, keys_sorted;
	DeviceBuffer<int> order, order_sorted, head, first, head_scan, first_scan;
	DeviceBuffer<uint8_t> tmp;
	nnrt_status st;
	if ((st = keys.ensure(n)) || (st = keys_sorted.ensure(n)) || (st = order.ensure(n)) || (st = order_sorted.ensure(n)) || (st = head.ensure(n)) ||
	    (st = first.ensure(n)) || (st = head_scan.ensure(n)) || (st = first_scan.ensure(n)) || (st = ix.pos.ensure(n)) ||
	    (st = ix.cell_keys.ensure(n)) || (st = ix.cell_start.ensure(static_cast<size_t>(n) + 1)) || (st = ix.cell_rank.ensure(n)) ||
	    (st = ix.ctrl.ensure(2)))
		return st;
	NNRT_HIP(hipMemsetAsync(ix.ctrl.ptr, 0, 2 * sizeof(int), s));
	k_index_keys<<<gblocks(n), GB, 0, s>>>(pts, n, cell, offset[0], offset[1], offset[2], keys.ptr, order.ptr, ix.ctrl.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = sort_pairs(keys.ptr, keys_sorted.ptr, order.ptr, order_sorted.ptr, n, 3 * CELL_BITS, tmp, s))) return st;
	k_index_heads<<<gblocks(n), GB, 0, s>>>(keys_sorted.ptr, order_sorted.ptr, n, head.ptr, first.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = exclusive_sum(head.ptr, head_scan.ptr, n, tmp, s)) || (st = exclusive_sum(first.ptr, first_scan.ptr, n, tmp, s))) return st;
	k_index_cells<<<gblocks(n), GB, 0, s>>>(pts, keys_sorted.ptr, order_sorted.ptr, head.ptr, head_scan.ptr, first_scan.ptr, n, ix.pos.ptr,
	                                        ix.cell_keys.ptr, ix.cell_start.ptr, ix.cell_rank.ptr, ix.ctrl.ptr);
	NNRT_LAUNCH_CHECK();
	int host_ctrl[2] = {0, 0};
	NNRT_HIP(hipMemcpyAsync(host_ctrl, ix.ctrl.ptr, sizeof(host_ctrl), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (host_ctrl[0]) return raise_index_error(host_ctrl[0]);
	if (host_ctrl[1] < 1 || host_ctrl[1] > n) {
		set_error("internal error: the cell index counted no cell or more cells than points");
		return NNRT_ERROR_INTERNAL;
	}
	ix.cells = host_ctrl[1];
	return NNRT_OK;
}

// indices of the flagged points, ascending, into out; the count must be the cell count
nnrt_status select_flagged_points(const uint8_t* flags, int n, int cells, int64_t* out, int64_t* h_count, hipStream_t s) {
	DeviceBuffer<int64_t> d_count;
	DeviceBuffer<uint8_t> tmp;
	nnrt_status st;
	if ((st = d_count.ensure(1))) return st;
	if ((st = select_flagged_indices(flags, out, d_count.ptr, n, tmp, s))) return st;
	NNRT_HIP(hipMemcpyAsync(h_count, d_count.ptr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (*h_count != cells) {
		set_error("internal error: the grid sample does not hold one point per cell");
		return NNRT_ERROR_INTERNAL;
	}
	return NNRT_OK;
}

unsigned cell_blocks(int cells) { return static_cast<unsigned>(ceil_div(cells, WAVES)); }

enum class CellSample { CLOSEST_TO_MEAN, MEDOID };

nnrt_status grid_subsample(const float* pts, int n, float cell, const float* offset, CellSample what, int64_t* out, int64_t* h_count, hipStream_t s) {
	*h_count = 0;
	if (n == 0) return NNRT_OK;
	CellIndex ix;
	nnrt_status st;
	if ((st = build_cell_index(ix, pts, n, cell, offset, s))) return st;
	DeviceBuffer<uint8_t> flags;
	if ((st = flags.ensure(n))) return st;
	NNRT_HIP(hipMemsetAsync(flags.ptr, 0, n, s));
	if (what == CellSample::MEDOID) k_cell_medoid<<<cell_blocks(ix.cells), GB, 0, s>>>(ix.pos.ptr, ix.cell_start.ptr, ix.cells, flags.ptr);
	else k_cell_mean<true><<<cell_blocks(ix.cells), GB, 0, s>>>(ix.pos.ptr, ix.cell_start.ptr, ix.cell_rank.ptr, ix.cells, nullptr, flags.ptr);
	NNRT_LAUNCH_CHECK();
	return select_flagged_points(flags.ptr, n, ix.cells, out, h_count, s);
}
} // namespace

nnrt_status launch_mean_grid_downsample(const float* pts, int n, float cell, const float* offset, float* out, int64_t* h_count, hipStream_t s) {
	*h_count = 0;
	if (n == 0) return NNRT_OK;
	CellIndex ix;
	nnrt_status st;
	if ((st = build_cell_index(ix, pts, n, cell, offset, s))) return st;
	k_cell_mean<false><<<cell_blocks(ix.cells), GB, 0, s>>>(ix.pos.ptr, ix.cell_start.ptr, ix.cell_rank.ptr, ix.cells, out, nullptr);
	NNRT_LAUNCH_CHECK();
	NNRT_HIP(hipStreamSynchronize(s));   // the index is freed on return
	*h_count = ix.cells;
	return NNRT_OK;
}

nnrt_status launch_closest_to_mean_grid_subsample(const float* pts, int n, float cell, const float* offset, int64_t* out, int64_t* h_count,
                                                  hipStream_t s) {
	return grid_subsample(pts, n, cell, offset, CellSample::CLOSEST_TO_MEAN, out, h_count, s);
}

nnrt_status launch_median_grid_subsample_binned(const float* pts, int n, float cell, const float* offset, int64_t* out, int64_t* h_count,
                                                hipStream_t s) {
	return grid_subsample(pts, n, cell, offset, CellSample::MEDOID, out, h_count, s);
}

// ---------------------------------------------------------- point index ----
struct PointIndex {
	CellIndex ix;
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
	int builds = 0;
};

namespace {
constexpr double TARGET_PER_CELL = 4.0;   // points per cell the size aims at; a build with more than twice that is refined
constexpr int MAX_BUILDS = 4;

// A cell size at which the bounding box holds about n / TARGET_PER_CELL cells: the geometric mean over the axes longer
// than the cell itself (a plane or a line is gridded in its own dimensions), not below `floor`.
float cell_size_for(const double* extent, int n, float floor_size) {
	bool active[3] = {extent[0] > 0.0, extent[1] > 0.0, extent[2] > 0.0};
	double c = 0.0;
	for (int pass = 0; pass < 3; pass++) {
		int d = 0;
		double log_volume = 0.0;
		for (int a = 0; a < 3; a++)
			if (active[a]) {
				d++;
				log_volume += std::log(extent[a]);
			}
		if (d == 0) break;
		c = std::exp((log_volume + std::log(TARGET_PER_CELL / n)) / d);
		bool changed = false;
		for (int a = 0; a < 3; a++)
			if (active[a] && extent[a] < c) {
				active[a] = false;
				changed = true;
			}
		if (!changed) break;
	}
	float cell = static_cast<float>(c);
	if (!(cell >= floor_size)) cell = floor_size;
	if (!(cell > 0.f) || !std::isfinite(cell)) cell = 1.f;
	return cell;
}

double box_cells(const double* extent, float cell) {
	double cells = 1.0;
	for (int a = 0; a < 3; a++) cells *= std::floor(extent[a] / cell) + 1.0;
	return cells;
}
} // namespace

nnrt_status point_index_create(const float* pts, int n, hipStream_t s, PointIndex** out) {
	DeviceBuffer<unsigned> box;
	DeviceBuffer<int> flag;
	nnrt_status st;
	if ((st = box.ensure(6)) || (st = flag.ensure(1))) return st;
	NNRT_HIP(hipMemsetAsync(box.ptr, 0xff, 3 * sizeof(unsigned), s));
	NNRT_HIP(hipMemsetAsync(box.ptr + 3, 0, 3 * sizeof(unsigned), s));
	NNRT_HIP(hipMemsetAsync(flag.ptr, 0, sizeof(int), s));
	k_bounding_box<<<gblocks(n), GB, 0, s>>>(pts, n, box.ptr, flag.ptr);
	NNRT_LAUNCH_CHECK();
	unsigned h_box[6];
	int h_flag = 0;
	NNRT_HIP(hipMemcpyAsync(h_box, box.ptr, sizeof(h_box), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipMemcpyAsync(&h_flag, flag.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	if (h_flag) return raise_index_error(h_flag);
	float lo[3], hi[3];
	double extent[3];
	float largest = 0.f;
	for (int a = 0; a < 3; a++) {
		lo[a] = from_ordered_bits(h_box[a]);
		hi[a] = from_ordered_bits(h_box[3 + a]);
		extent[a] = static_cast<double>(hi[a]) - static_cast<double>(lo[a]);
		largest = std::max(largest, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
	}
	// |p / cell| <= 2^19 keeps every cell inside the key's range, whatever the cloud's distance from the origin
	const float floor_size = std::max(largest * 0x1p-19f, FLT_MIN * 0x1p24f);
	float cell = cell_size_for(extent, n, floor_size);
	const bool extended = extent[0] > 0.0 || extent[1] > 0.0 || extent[2] > 0.0;
	const float zero[3] = {0.f, 0.f, 0.f};
	PointIndex* pi = new PointIndex();
	for (;;) {
		if ((st = build_cell_index(pi->ix, pts, n, cell, zero, s))) {
			delete pi;
			return st;
		}
		pi->builds++;
		// a surface or a clustered cloud leaves most of the box empty and its occupied cells crowded: shrink the cell while
		// the box stays within 8 cells per point (which bounds every query's walk over empty shells)
		const double per_cell = static_cast<double>(n) / pi->ix.cells;
		if (!extended || pi->builds >= MAX_BUILDS || per_cell <= 2.0 * TARGET_PER_CELL) break;
		const float finer = std::max(static_cast<float>(cell * std::cbrt(TARGET_PER_CELL / per_cell)), floor_size);
		if (!(finer < cell) || box_cells(extent, finer) > 8.0 * n) break;
		cell = finer;
	}
	for (int a = 0; a < 3; a++) {   // the key kernel's expression: monotone in p, so every point's cell lies between the corners'
		pi->lo[a] = static_cast<int>(floorf(lo[a] / cell + 0.f)) + CELL_BIAS;
		pi->hi[a] = static_cast<int>(floorf(hi[a] / cell + 0.f)) + CELL_BIAS;
	}
	*out = pi;
	return NNRT_OK;
}

void point_index_destroy(PointIndex* pi) { delete pi; }

void point_index_info(const PointIndex* pi, int64_t* point_count, float* cell_size, int64_t* cell_count, int32_t* build_count) {
	if (point_count) *point_count = pi->ix.n;
	if (cell_size) *cell_size = pi->ix.cell;
	if (cell_count) *cell_count = pi->ix.cells;
	if (build_count) *build_count = pi->builds;
}

nnrt_status point_index_find_k_nearest(const PointIndex* pi, const float* queries, int Q, int k, int32_t* out_i, float* out_d, hipStream_t s) {
	if (Q == 0) return NNRT_OK;
	IndexView v;
	v.pos = pi->ix.pos.ptr;
	v.cell_keys = pi->ix.cell_keys.ptr;
	v.cell_start = pi->ix.cell_start.ptr;
	v.cells = pi->ix.cells;
	v.cell = pi->ix.cell;
	for (int a = 0; a < 3; a++) {
		v.lo[a] = pi->lo[a];
		v.hi[a] = pi->hi[a];
	}
	k_knn_query<<<gblocks(Q), GB, 0, s>>>(v, queries, Q, k, out_i, out_d);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
