// The fitter's coupled data term, outside the pixel launches: the per-frame node-pair structure
// (device keys, sort + unique, host tables) and the assembly of the pair blocks the tile-sparse solver factors.
#include "coupled.hpp"
#include "device_primitives.hpp"

namespace nnrt {

namespace {

// thread (face, q): the q-th pair (a < b) of the face's table row; a key where both entries hold a node, else the invalid key
__global__ __launch_bounds__(256) void k_face_pair_keys(const uint32_t* __restrict__ face_nodes, int64_t F, int NS, int per_face,
                                                        uint64_t* __restrict__ keys) {
	const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= F * per_face) return;
	const int64_t f = t / per_face;
	int rem = static_cast<int>(t % per_face), a = 0;
	while (rem >= NS - 1 - a) {   // row a of the strict upper triangle holds NS - 1 - a pairs
		rem -= NS - 1 - a;
		a++;
	}
	const int b = a + 1 + rem;
	const uint32_t ea = face_nodes[f * NS + a], eb = face_nodes[f * NS + b];
	uint64_t key = PAIR_KEY_NONE;
	if (ea != FACE_NODE_NONE && eb != FACE_NODE_NONE) {
		// rows are ascending in node, so a < b gives i < j
		const uint64_t i = ea >> FACE_NODE_SHIFT, j = eb >> FACE_NODE_SHIFT;
		if (i < j) key = i << 32 | j;
	}
	keys[t] = key;
}

__global__ __launch_bounds__(256) void k_edge_pair_keys(const int32_t* __restrict__ edges, int E, int N, uint64_t* __restrict__ keys) {
	const int e = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
	if (e >= E) return;
	const int i = edges[2 * e], j = edges[2 * e + 1];
	const bool ok = i >= 0 && j >= 0 && i < N && j < N && i != j;
	const uint64_t lo = static_cast<uint64_t>(i < j ? i : j), hi = static_cast<uint64_t>(i < j ? j : i);
	keys[e] = ok ? lo << 32 | hi : PAIR_KEY_NONE;
}

// thread (pair s, entry q = 6 r + c)
__global__ __launch_bounds__(256) void k_coupled_assemble(const double* __restrict__ pair_acc, int M, const int* __restrict__ edge_off,
                                                          const int* __restrict__ edge_list, const float* __restrict__ wing,
                                                          float* __restrict__ pair_blocks) {
	const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (t >= static_cast<int64_t>(M) * 36) return;
	const int s = static_cast<int>(t / 36), q = static_cast<int>(t % 36);
	float v = static_cast<float>(pair_acc[t]);
	for (int u = edge_off[s]; u < edge_off[s + 1]; u++) {
		const int code = edge_list[u];
		const float* B = wing + static_cast<int64_t>(code >> 1) * 36;
		v += (code & 1) ? B[6 * (q % 6) + q / 6] : B[q];
	}
	pair_blocks[t] = v;
}

} // namespace

nnrt_status build_pair_structure(PairStructure& ps, const uint32_t* face_nodes, int64_t F, int K, const int32_t* d_edges,
                                 const int32_t* h_edges, int E, int N, hipStream_t s, bool* moved) {
	const int NS = face_node_slots(K), per_face = NS * (NS - 1) / 2;
	const int64_t total = F * per_face + E;
	NNRT_CHECK_ARG(total < (int64_t(1) << 31), "mesh too large for the coupled data term's pair build");
	nnrt_status st;
	if ((st = ps.keys.ensure(static_cast<size_t>(total))) || (st = ps.keys_sorted.ensure(static_cast<size_t>(total))) || (st = ps.d_count.ensure(1)))
		return st;
	if (F > 0) {
		k_face_pair_keys<<<static_cast<unsigned>(ceil_div(F * per_face, 256)), 256, 0, s>>>(face_nodes, F, NS, per_face, ps.keys.ptr);
		NNRT_LAUNCH_CHECK();
	}
	if (E > 0) {
		k_edge_pair_keys<<<static_cast<unsigned>(ceil_div(E, 256)), 256, 0, s>>>(d_edges, E, N, ps.keys.ptr + F * per_face);
		NNRT_LAUNCH_CHECK();
	}
	int unique = 0;
	if (total > 0) {
		// ps.tmp only grows, and no captured graph holds it (nor keys, keys_sorted, d_count): `moved` does not watch them
		if ((st = sort_keys(ps.keys.ptr, ps.keys_sorted.ptr, total, 64, ps.tmp, s)) ||
		    (st = unique_keys(ps.keys_sorted.ptr, ps.keys.ptr, ps.d_count.ptr, total, ps.tmp, s)))
			return st;
		NNRT_HIP(hipMemcpyAsync(&unique, ps.d_count.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));
	}
	NNRT_CHECK_ARG(unique >= 0 && unique <= total, "pair build: unique count out of range");
	std::vector<uint64_t> h_keys(static_cast<size_t>(unique));
	if (unique > 0) NNRT_HIP(hipMemcpy(h_keys.data(), ps.keys.ptr, sizeof(uint64_t) * h_keys.size(), hipMemcpyDeviceToHost));
	ps.M = pairs_from_keys(h_keys, ps.h_pairs);
	PairTables t;
	std::string err;
	if (!build_pair_tables(ps.h_pairs.data(), ps.M, N, h_edges, E, t, &err)) {
		set_error("coupled data term: " + err);
		return NNRT_ERROR_ARGUMENT;
	}
	if ((st = upload(ps.pairs, ps.h_pairs, moved)) || (st = upload(ps.row_off, t.row_off, moved)) ||
	    (st = upload(ps.edge_off, t.edge_off, moved)) || (st = upload(ps.edge_list, t.edge_list, moved)) ||
	    (st = upload(ps.inc_off, t.inc_off, moved)) || (st = upload(ps.inc_list, t.inc_list, moved)))
		return st;
	return NNRT_OK;
}

nnrt_status launch_coupled_assemble(const double* pair_acc, int M, const int* edge_off, const int* edge_list, const float* wing,
                                    float* pair_blocks, hipStream_t stream) {
	if (M == 0) return NNRT_OK;
	k_coupled_assemble<<<static_cast<unsigned>(ceil_div(static_cast<int64_t>(M) * 36, 256)), 256, 0, stream>>>(pair_acc, M, edge_off, edge_list, wing,
	                                                                                                        pair_blocks);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
