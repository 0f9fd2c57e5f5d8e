// Host bookkeeping of the fitter's coupled data term: the tables prepare() derives from the
// frame's node-pair list. Plain C++ (no HIP), so tests/native/pair_tables_check.cpp exercises it under the host
// sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace nnrt {

// invalid key of the pair build (sorts last); a pair (i, j), i < j, is i << 32 | j
constexpr uint64_t PAIR_KEY_NONE = ~0ull;

struct PairTables {
	std::vector<int> row_off;     // [N + 1] CSR by row: pairs (i, .) are [row_off[i], row_off[i + 1]), ascending j
	std::vector<int> edge_off;    // [M + 1] CSR into edge_list by pair
	std::vector<int> edge_list;   // 2 e + t: ARAP edge e lies on the pair; t = 1: it is stored (j, i), its wing block transposed
	std::vector<int> inc_off;     // [N + 1] CSR of pair incidences by node (the refinement's residual rows)
	std::vector<int> inc_list;    // [2 M] 2 s + (node is pair s's second node), ascending s per node
};

// sorted unique keys (the invalid key last, if present) -> pairs [M, 2]; returns M
inline int pairs_from_keys(const std::vector<uint64_t>& keys, std::vector<int32_t>& pairs) {
	size_t m = keys.size();
	if (m > 0 && keys[m - 1] == PAIR_KEY_NONE) m--;
	pairs.resize(2 * m);
	for (size_t s = 0; s < m; s++) {
		pairs[2 * s] = static_cast<int32_t>(keys[s] >> 32);
		pairs[2 * s + 1] = static_cast<int32_t>(keys[s] & 0xffffffffu);
	}
	return static_cast<int>(m);
}

// slot of pair (i, j), i < j, or -1 (binary search in row i)
inline int find_pair(const std::vector<int>& row_off, const int32_t* pairs, int i, int j) {
	int lo = row_off[static_cast<size_t>(i)], hi = row_off[static_cast<size_t>(i) + 1];
	while (lo < hi) {
		const int mid = lo + (hi - lo) / 2;
		const int v = pairs[2 * static_cast<size_t>(mid) + 1];
		if (v == j) return mid;
		if (v < j) lo = mid + 1;
		else hi = mid;
	}
	return -1;
}

// CSR of the incidences of M index pairs [M, 2] by node: off [N + 1] into list [2 M], which holds 2 s + t for entry t of
// pair s (t = 1: the node is the pair's second index), ascending s per node. Every index must lie in [0, N). The pairs of
// the coupled data term, and the ARAP edges of the arrowhead solve (source 2 e, target 2 e + 1), are both listed this way.
inline void incidence_csr(const int32_t* pairs, int M, int N, std::vector<int>& off, std::vector<int>& list) {
	off.assign(static_cast<size_t>(N) + 1, 0);
	for (size_t q = 0; q < 2 * static_cast<size_t>(M); q++) off[static_cast<size_t>(pairs[q]) + 1]++;
	for (int n = 0; n < N; n++) off[static_cast<size_t>(n) + 1] += off[static_cast<size_t>(n)];
	list.assign(2 * static_cast<size_t>(M), 0);
	std::vector<int> fill(off.begin(), off.end() - 1);
	for (size_t q = 0; q < 2 * static_cast<size_t>(M); q++) list[static_cast<size_t>(fill[static_cast<size_t>(pairs[q])]++)] = static_cast<int>(q);
}

// the inverse of such a list: slot[2 s + t] is where the incidence stands in it
inline std::vector<int> incidence_slots(const std::vector<int>& list) {
	std::vector<int> slot(list.size());
	for (size_t q = 0; q < list.size(); q++) slot[static_cast<size_t>(list[q])] = static_cast<int>(q);
	return slot;
}

// pairs [M, 2] strictly ascending in (i, j) with 0 <= i < j < N; edges [E, 2] (virtual order), each of which must lie on a
// pair. false + *err on malformed input (nothing is indexed out of range).
inline bool build_pair_tables(const int32_t* pairs, int M, int N, const int32_t* edges, int E, PairTables& t, std::string* err) {
	auto fail = [&](const char* m) {
		if (err) *err = m;
		return false;
	};
	if (M < 0 || N < 0 || E < 0) return fail("negative count");
	t.row_off.assign(static_cast<size_t>(N) + 1, 0);
	for (int s = 0; s < M; s++) {
		const int i = pairs[2 * static_cast<size_t>(s)], j = pairs[2 * static_cast<size_t>(s) + 1];
		if (i < 0 || j <= i || j >= N) return fail("pair outside 0 <= i < j < node count");
		if (s > 0) {
			const int pi = pairs[2 * static_cast<size_t>(s) - 2], pj = pairs[2 * static_cast<size_t>(s) - 1];
			if (pi > i || (pi == i && pj >= j)) return fail("pair list not strictly ascending");
		}
		t.row_off[static_cast<size_t>(i) + 1]++;
	}
	for (int n = 0; n < N; n++) t.row_off[static_cast<size_t>(n) + 1] += t.row_off[static_cast<size_t>(n)];
	incidence_csr(pairs, M, N, t.inc_off, t.inc_list);
	// the ARAP edges on each pair, ascending edge index per pair
	std::vector<int> slot(static_cast<size_t>(E), 0);
	t.edge_off.assign(static_cast<size_t>(M) + 1, 0);
	for (int e = 0; e < E; e++) {
		const int i = edges[2 * static_cast<size_t>(e)], j = edges[2 * static_cast<size_t>(e) + 1];
		if (i < 0 || i >= N || j < 0 || j >= N || i == j) return fail("edge outside the node range or on the diagonal");
		const int s = find_pair(t.row_off, pairs, std::min(i, j), std::max(i, j));
		if (s < 0) return fail("edge without a pair");
		slot[static_cast<size_t>(e)] = s;
		t.edge_off[static_cast<size_t>(s) + 1]++;
	}
	for (int s = 0; s < M; s++) t.edge_off[static_cast<size_t>(s) + 1] += t.edge_off[static_cast<size_t>(s)];
	t.edge_list.assign(static_cast<size_t>(E), 0);
	{
		std::vector<int> fill(t.edge_off.begin(), t.edge_off.end() - 1);
		for (int e = 0; e < E; e++)
			t.edge_list[static_cast<size_t>(fill[static_cast<size_t>(slot[static_cast<size_t>(e)])]++)] =
			    2 * e + (edges[2 * static_cast<size_t>(e)] > edges[2 * static_cast<size_t>(e) + 1] ? 1 : 0);
	}
	return true;
}

} // namespace nnrt
