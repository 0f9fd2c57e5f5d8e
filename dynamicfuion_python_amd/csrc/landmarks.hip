// The fitter's landmark term (landmarks.hpp): the per-frame grouping of the landmarks' associations
// by node and by node pair, and the per-iteration launch that sums them into the normal equations.
#include <cfloat>

#include "fitter_kernels.hpp"
#include "landmarks.hpp"

namespace nnrt {

namespace {

constexpr int LM_GROUP = 8;                      // lanes per run
constexpr int LM_BLOCK = 64;                     // one wave per workgroup: its groups never wait on another wave
constexpr int LM_GROUPS = LM_BLOCK / LM_GROUP;   // runs per workgroup
// a filed row: a node association's J (3 x 6, row-major) and r (3), or a pair association's J_a and J_b (odd stride: the
// stores spread over the banks)
constexpr int LM_PAIR_ROW = 37;

// ---- once per frame --------------------------------------------------------------------------------------------------
__global__ void k_lm_init(int* __restrict__ info, int64_t* __restrict__ node_count, int64_t* __restrict__ pair_count) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	for (int i = 0; i < LM_INFO_WORDS; i++) info[i] = 0;
	info[LM_INFO_BAD_INDEX] = LM_NONE;
	info[LM_INFO_NO_FACE] = LM_NONE;
	*node_count = 0;
	*pair_count = 0;
}

__global__ __launch_bounds__(256) void k_lm_mark_faces(const int4* __restrict__ faces4, int64_t F, int64_t V, uint8_t* __restrict__ in_face) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (f >= F) return;
	const int4 fi = faces4[f];
	if (fi.x == fi.y && fi.y == fi.z) return;   // the degenerate face that stands for one with an index out of range
	if (fi.x >= 0 && fi.x < V) in_face[fi.x] = 1;
	if (fi.y >= 0 && fi.y < V) in_face[fi.y] = 1;
	if (fi.z >= 0 && fi.z < V) in_face[fi.z] = 1;
}

// thread (landmark l, slot k): the association's key = its node (LM_KEY_NONE: no anchor in the slot), value = l K + k;
// slot 0 also checks the landmark against the frame
__global__ __launch_bounds__(256) void k_lm_expand_nodes(int64_t L, int K, int64_t V, const int32_t* __restrict__ index,
                                                         const int32_t* __restrict__ anchors, const uint8_t* __restrict__ in_face,
                                                         uint64_t* __restrict__ keys, int* __restrict__ vals, int* __restrict__ info) {
	const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= L * K) return;
	const int l = static_cast<int>(t / K), k = static_cast<int>(t % K);
	const int v = index[l];
	const bool bad = v < 0 || v >= V;
	if (k == 0) {
		if (bad) atomicMin(info + LM_INFO_BAD_INDEX, l);
		else if (!in_face[v]) atomicMin(info + LM_INFO_NO_FACE, l);
	}
	const int node = bad ? -1 : anchors[static_cast<int64_t>(v) * K + k];
	keys[t] = node >= 0 ? static_cast<uint64_t>(node) : LM_KEY_NONE;
	vals[t] = static_cast<int>(t);
}

// slot of pair (i, j), i < j, in the frame's pair list: binary search in row i of its CSR (-1: not a pair)
__device__ __forceinline__ int lm_pair_slot(const int* __restrict__ row_off, const int32_t* __restrict__ pairs, int i, int j) {
	int lo = row_off[i], hi = row_off[i + 1];
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		const int v = pairs[2 * mid + 1];
		if (v == j) return mid;
		if (v < j) lo = mid + 1;
		else hi = mid;
	}
	return -1;
}

// thread (landmark l, q): the q-th slot pair (ka < kb) of the landmark's vertex; key = the pair slot of its two nodes,
// value = (l K + slot of the lower node) K + slot of the higher node
__global__ __launch_bounds__(256) void k_lm_expand_pairs(int64_t L, int K, int64_t V, int N, const int32_t* __restrict__ index,
                                                         const int32_t* __restrict__ anchors, const int* __restrict__ row_off,
                                                         const int32_t* __restrict__ pairs, uint64_t* __restrict__ keys, int* __restrict__ vals) {
	const int per = K * (K - 1) / 2;
	const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= L * per) return;
	const int l = static_cast<int>(t / per);
	int rem = static_cast<int>(t % per), ka = 0;
	while (rem >= K - 1 - ka) {   // row ka of the strict upper triangle holds K - 1 - ka pairs
		rem -= K - 1 - ka;
		ka++;
	}
	const int kb = ka + 1 + rem;
	const int v = index[l];
	uint64_t key = LM_KEY_NONE;
	int val = 0;
	if (v >= 0 && v < V) {
		const int na = anchors[static_cast<int64_t>(v) * K + ka], nb = anchors[static_cast<int64_t>(v) * K + kb];
		if (na >= 0 && nb >= 0 && na < N && nb < N && na != nb) {
			const bool swap = nb < na;
			const int m = lm_pair_slot(row_off, pairs, swap ? nb : na, swap ? na : nb);
			if (m >= 0) {
				key = static_cast<uint64_t>(m);
				val = (l * K + (swap ? kb : ka)) * K + (swap ? ka : kb);
			}
		}
	}
	keys[t] = key;
	vals[t] = val;
}

__global__ __launch_bounds__(256) void k_lm_heads(const uint64_t* __restrict__ keys, int64_t n, uint8_t* __restrict__ heads) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	heads[i] = i == 0 || keys[i] != keys[i - 1];
}

// associations and runs of one sorted list of n entries whose run starts were selected: a last run keyed LM_KEY_NONE is no run
__device__ void lm_count_runs(const uint64_t* keys, const int64_t* starts, int64_t runs, int64_t n, int* assoc_out, int* runs_out) {
	int64_t assoc = n;
	if (runs > 0 && keys[starts[runs - 1]] == LM_KEY_NONE) {
		assoc = starts[runs - 1];
		runs--;
	}
	*assoc_out = runs > 0 ? static_cast<int>(assoc) : 0;
	*runs_out = static_cast<int>(runs);
}
__global__ void k_lm_info(int* __restrict__ info, const uint64_t* node_keys, const int64_t* node_starts, const int64_t* node_count, int64_t n_node,
                          const uint64_t* pair_keys, const int64_t* pair_starts, const int64_t* pair_count, int64_t n_pair) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	lm_count_runs(node_keys, node_starts, *node_count, n_node, info + LM_INFO_ASSOC, info + LM_INFO_RUNS);
	if (n_pair > 0) lm_count_runs(pair_keys, pair_starts, *pair_count, n_pair, info + LM_INFO_PAIR_ASSOC, info + LM_INFO_PAIR_RUNS);
}

nnrt_status sort_into_runs(LandmarkRuns& r, int64_t n, Scratch& scratch, hipStream_t s) {
	nnrt_status st;
	if ((st = sort_pairs(r.keys_in.ptr, r.keys.ptr, r.vals_in.ptr, r.vals.ptr, n, 32, scratch, s))) return st;
	k_lm_heads<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, s>>>(r.keys.ptr, n, r.heads.ptr);
	NNRT_LAUNCH_CHECK();
	return select_flagged_indices(r.heads.ptr, r.starts.ptr, r.count.ptr, n, scratch, s);
}

nnrt_status allocate_runs(LandmarkRuns& r, size_t n, bool* moved) {
	nnrt_status st;
	// the launch of every iteration reads keys, vals and starts; the rest is the grouping's own
	if ((st = ensure(r.keys, n, moved)) || (st = ensure(r.vals, n, moved)) || (st = ensure(r.starts, n, moved)) || (st = r.keys_in.ensure(n)) ||
	    (st = r.vals_in.ensure(n)) || (st = r.heads.ensure(n)) || (st = r.count.ensure(1)))
		return st;
	return NNRT_OK;
}

// ---- once per iteration -----------------------------------------------------------------------------------------------
struct LmEval {
	f3 d;          // v' - q
	float c;       // w_L s
	bool active;   // contributes rows
	bool dropped;  // on, but beyond the cutoff
};

__device__ __forceinline__ bool lm_finite(float x) { return fabsf(x) <= FLT_MAX; }

// the landmark's distance and gate at this iteration's warped mesh
__device__ __forceinline__ LmEval lm_eval(const FitLandmarkArgs& a, int l) {
	LmEval e;
	const int v = a.index[l];
	const float s = a.weight[l];
	const f3 q = make3(a.target[3 * l], a.target[3 * l + 1], a.target[3 * l + 2]);
	const float4 wp = a.wpos[v];
	e.d = sub3(make3(wp.x, wp.y, wp.z), q);
	const float dist = sqrtf(dot3(e.d, e.d));
	const bool on = s > 0.f && lm_finite(q.x) && lm_finite(q.y) && lm_finite(q.z);
	const bool within = a.cutoff <= 0.f || dist <= a.cutoff;
	e.c = a.term_weight * s;
	e.active = on && within;
	e.dropped = on && !within;
	return e;
}

// The three Jacobian rows of landmark l for the node in anchor slot k of its vertex, J[6 c + 0..2] the rotation part and
// J[6 c + 3..5] the translation part of row c: the rows pixel_node_row's unfused form (pixel_terms.hpp) gives for
// dr/dV = coef e_c at one vertex and no normal part, from warp_slot_state's row -w R (v - g) (kernels.hpp) with the vertex
// as stored (so the extrinsics enter as they do for the data term).
__device__ __forceinline__ void lm_rows(const FitLandmarkArgs& a, int l, int k, float coef, float* __restrict__ J) {
	const int v = a.index[l];
	const int64_t slot = static_cast<int64_t>(v) * a.K + k;
	const int n = a.anchors[slot];
	const float w = a.weights[slot];
	const float* ns = a.state_in + static_cast<int64_t>(n) * NODE_STRIDE;
	const f3 g = make3(ns[0], ns[1], ns[2]);
	float R[9];
#pragma unroll
	for (int i = 0; i < 9; i++) R[i] = a.state_identity ? ((i % 4 == 0) ? 1.f : 0.f) : ns[6 + i];
	const f3 Rj = matvec3(R, sub3(make3(a.mesh_p[3 * static_cast<int64_t>(v)], a.mesh_p[3 * static_cast<int64_t>(v) + 1], a.mesh_p[3 * static_cast<int64_t>(v) + 2]), g));
	const f3 jv = make3(-w * Rj.x, -w * Rj.y, -w * Rj.z);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const f3 dv = make3(c == 0 ? coef : 0.f, c == 1 ? coef : 0.f, c == 2 ? coef : 0.f);
		const f3 t1 = row_times_skew(dv, jv);
		J[6 * c + 0] = t1.x;
		J[6 * c + 1] = t1.y;
		J[6 * c + 2] = t1.z;
		J[6 * c + 3] = dv.x * w;
		J[6 * c + 4] = dv.y * w;
		J[6 * c + 5] = dv.z * w;
	}
}

__device__ __forceinline__ void lm_wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (r0, c0), r0 <= c0, of upper-triangle entry e < 21 of a 6 x 6 block (row-major over the triangle, as acc holds it)
__device__ __forceinline__ void lm_upper_entry(int e, int& r0, int& c0) {
	r0 = 0;
	while (r0 < 5 && e >= 6 - r0) {
		e -= 6 - r0;
		r0++;
	}
	c0 = r0 + e;
}

// One workgroup = one wave = LM_GROUPS runs, one per 8-lane group. A pass files 8 associations of the run (one per lane)
// in the group's LDS rows; then lane j sums its entries j, j + 8, ... over the filed rows in association order, in fp64.
// A run longer than a pass loops; the loop's trip count is the wave's longest run's (the barriers stay wave-uniform), a
// group past its run's end files nothing and sums nothing. After the last pass the group's lanes add their sums to the
// run's row of acc (pair_acc): the run is the row's only writer in this launch, so no atomics and no dependence on
// scheduling. The last workgroup writes every landmark's distance and gate and the cost, summed in landmark order.
__global__ __launch_bounds__(LM_BLOCK) void k_fit_landmarks(FitLandmarkArgs a) {
	__shared__ float s_rows[LM_GROUPS][LM_GROUP][LM_PAIR_ROW];
	__shared__ double s_rho[LM_BLOCK];
	const int lane = static_cast<int>(threadIdx.x), grp = lane / LM_GROUP, j = lane % LM_GROUP;
	const int b = static_cast<int>(blockIdx.x);
	if (b >= a.node_blocks + a.pair_blocks) {
		double total = 0.0;
		for (int base = 0; base < a.L; base += LM_BLOCK) {
			const int l = base + lane;
			double rho = 0.0;
			if (l < a.L) {
				const LmEval e = lm_eval(a, l);
				a.distances[l] = make_float4(e.d.x, e.d.y, e.d.z, e.active ? 1.f : 0.f);
				if (e.active) {
					const double rx = static_cast<double>(e.c * e.d.x), ry = static_cast<double>(e.c * e.d.y), rz = static_cast<double>(e.c * e.d.z);
					rho = (rx * rx + ry * ry) + rz * rz;
				} else if (e.dropped) {
					const double t = static_cast<double>(e.c) * static_cast<double>(a.cutoff);
					rho = t * t;
				}
			}
			s_rho[lane] = rho;
			lm_wave_sync();
			if (lane == 0) {
				const int cnt = a.L - base < LM_BLOCK ? a.L - base : LM_BLOCK;
				for (int q = 0; q < cnt; q++) total += s_rho[q];
			}
			lm_wave_sync();
		}
		if (lane == 0) *a.cost = total;
		return;
	}
	const bool pair_role = b >= a.node_blocks;
	const int r = (pair_role ? b - a.node_blocks : b) * LM_GROUPS + grp;
	const int runs = a.info[pair_role ? LM_INFO_PAIR_RUNS : LM_INFO_RUNS], assoc = a.info[pair_role ? LM_INFO_PAIR_ASSOC : LM_INFO_ASSOC];
	const uint64_t* keys = pair_role ? a.pair_keys : a.node_keys;
	const int* vals = pair_role ? a.pair_vals : a.node_vals;
	const int64_t* starts = pair_role ? a.pair_starts : a.node_starts;
	const bool valid = r < runs;
	const int beg = valid ? static_cast<int>(starts[r]) : 0;
	const int end = valid ? (r + 1 < runs ? static_cast<int>(starts[r + 1]) : assoc) : 0;
	const int64_t row = valid ? static_cast<int64_t>(keys[beg]) : 0;   // the run's node, or its pair slot
	const int entries = pair_role ? 36 : 27;
	constexpr int OWN = 5;   // entries per lane at most (36 / 8 rounded up)
	double sums[OWN] = {0.0, 0.0, 0.0, 0.0, 0.0};
	float* mine = s_rows[grp][j];
	for (int base = beg; __any(base < end); base += LM_GROUP) {
		const int u = base + j;
#pragma unroll
		for (int i = 0; i < LM_PAIR_ROW; i++) mine[i] = 0.f;   // an association past the run's end, or an inactive landmark's
		if (u < end) {
			const int code = vals[u];
			if (pair_role) {
				const int kb = code % a.K, ka = (code / a.K) % a.K, l = code / (a.K * a.K);
				const LmEval e = lm_eval(a, l);
				if (e.active) {
					lm_rows(a, l, ka, e.c, mine);
					lm_rows(a, l, kb, e.c, mine + 18);
				}
			} else {
				const int k = code % a.K, l = code / a.K;
				const LmEval e = lm_eval(a, l);
				if (e.active) {
					lm_rows(a, l, k, e.c, mine);
					mine[18] = e.c * e.d.x;
					mine[19] = e.c * e.d.y;
					mine[20] = e.c * e.d.z;
				}
			}
		}
		lm_wave_sync();
		const int cnt = base < end ? (end - base < LM_GROUP ? end - base : LM_GROUP) : 0;
#pragma unroll
		for (int i = 0; i < OWN; i++) {
			const int e = j + LM_GROUP * i;
			if (e >= entries) continue;
			int x, y;   // the entry sums row[x + 6 c] * row[y + 6 c] over the three residual rows c
			bool rhs = false;
			if (pair_role) {
				x = e / 6;
				y = 18 + e % 6;
			} else if (e < 21) {
				lm_upper_entry(e, x, y);
			} else {
				x = e - 21;
				y = 0;
				rhs = true;
			}
			double s = sums[i];
			for (int q = 0; q < cnt; q++) {
				const float* f = s_rows[grp][q];
#pragma unroll
				for (int c = 0; c < 3; c++) s += static_cast<double>(f[x + 6 * c]) * static_cast<double>(rhs ? f[18 + c] : f[y + 6 * c]);
			}
			sums[i] = s;
		}
		lm_wave_sync();
	}
	if (!valid) return;
	double* out = pair_role ? a.pair_acc + row * 36 : a.acc + row * ACC_STRIDE;
#pragma unroll
	for (int i = 0; i < OWN; i++) {
		const int e = j + LM_GROUP * i;
		if (e < entries) out[e] += sums[i];
	}
}

} // namespace

nnrt_status allocate_landmark_groups(LandmarkSet& lm, const LandmarkFrame& fr, bool* moved) {
	const size_t n_node = static_cast<size_t>(lm.L) * fr.K, n_pair = fr.coupled ? static_cast<size_t>(lm.L) * fr.K * (fr.K - 1) / 2 : 0;
	NNRT_CHECK_ARG(static_cast<int64_t>(lm.L) * fr.K * fr.K < (int64_t(1) << 31), "too many landmarks for int32 association codes");
	nnrt_status st;
	if ((st = ensure(lm.info, LM_INFO_WORDS, moved)) || (st = lm.vertex_in_face.ensure(static_cast<size_t>(fr.V))) ||
	    (st = allocate_runs(lm.node, n_node, moved)) || (st = allocate_runs(lm.pair, n_pair, moved)))
		return st;
	return NNRT_OK;
}

nnrt_status group_landmarks(LandmarkSet& lm, const LandmarkFrame& fr, hipStream_t s) {
	const int64_t L = lm.L, n_node = L * fr.K, n_pair = fr.coupled && fr.M > 0 ? L * fr.K * (fr.K - 1) / 2 : 0;
	nnrt_status st;
	k_lm_init<<<1, 1, 0, s>>>(lm.info.ptr, lm.node.count.ptr, lm.pair.count.ptr);
	NNRT_LAUNCH_CHECK();
	NNRT_HIP(hipMemsetAsync(lm.vertex_in_face.ptr, 0, static_cast<size_t>(fr.V), s));
	k_lm_mark_faces<<<static_cast<unsigned>(ceil_div(fr.F, 256)), 256, 0, s>>>(fr.faces4, fr.F, fr.V, lm.vertex_in_face.ptr);
	NNRT_LAUNCH_CHECK();
	k_lm_expand_nodes<<<static_cast<unsigned>(ceil_div(n_node, 256)), 256, 0, s>>>(L, fr.K, fr.V, lm.index.ptr, fr.anchors, lm.vertex_in_face.ptr,
	                                                                             lm.node.keys_in.ptr, lm.node.vals_in.ptr, lm.info.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = sort_into_runs(lm.node, n_node, lm.scratch, s))) return st;
	if (n_pair > 0) {
		k_lm_expand_pairs<<<static_cast<unsigned>(ceil_div(n_pair, 256)), 256, 0, s>>>(L, fr.K, fr.V, fr.N, lm.index.ptr, fr.anchors, fr.row_off, fr.pairs,
		                                                                             lm.pair.keys_in.ptr, lm.pair.vals_in.ptr);
		NNRT_LAUNCH_CHECK();
		if ((st = sort_into_runs(lm.pair, n_pair, lm.scratch, s))) return st;
	}
	k_lm_info<<<1, 1, 0, s>>>(lm.info.ptr, lm.node.keys.ptr, lm.node.starts.ptr, lm.node.count.ptr, n_node, lm.pair.keys.ptr, lm.pair.starts.ptr,
	                          lm.pair.count.ptr, n_pair);
	NNRT_LAUNCH_CHECK();
	int h[LM_INFO_WORDS] = {};
	NNRT_HIP(hipMemcpyAsync(h, lm.info.ptr, sizeof(h), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	for (int i = 0; i < 4; i++) lm.h_info[i] = 0;
	if (h[LM_INFO_BAD_INDEX] != LM_NONE) {
		set_error("invalid argument: landmark " + std::to_string(h[LM_INFO_BAD_INDEX]) + ": vertex index outside [0, vertex_count) of the prepared mesh");
		return NNRT_ERROR_ARGUMENT;
	}
	if (h[LM_INFO_NO_FACE] != LM_NONE) {
		set_error("invalid argument: landmark " + std::to_string(h[LM_INFO_NO_FACE]) + ": its vertex belongs to no face of the prepared mesh");
		return NNRT_ERROR_ARGUMENT;
	}
	for (int i = 0; i < 4; i++) lm.h_info[i] = h[i];
	return NNRT_OK;
}

nnrt_status launch_fit_landmarks(FitLandmarkArgs args, hipStream_t stream) {
	if (args.L <= 0) return NNRT_OK;
	k_fit_landmarks<<<static_cast<unsigned>(args.node_blocks + args.pair_blocks + 1), LM_BLOCK, 0, stream>>>(args);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
