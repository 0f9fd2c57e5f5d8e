// Host-only check of the coupled data term's per-frame bookkeeping (csrc/coupled_host.hpp), test infrastructure: the
// product header compiled alone, with the host sanitizers. Random node-pair structures with edges on some pairs (both
// orientations, and doubled) are turned into keys and back, the tables are built and every entry is checked against a
// brute-force search; malformed input must be refused without indexing anything. incidence_csr, which also lists the ARAP
// edges of the arrowhead solve by node, is called directly on the degenerate sizes and, given a file of edges
// ([E, N] then E x 2 int32: the 8 x 8 node grid's two-layer hierarchy, written by tests/test_pair_tables.py), on those,
// each against an O(N M) restatement, with incidence_slots as its inverse. Exit code 0 = all checks pass.
#include "coupled_host.hpp"

#include <cstdio>
#include <random>
#include <set>

using namespace nnrt;

static int fail(const char* what, int c) {
	printf("case %d: %s\n", c, what);
	return 1;
}

// incidence_csr / incidence_slots of pairs [M, 2] over N nodes against the definition, stated naively
static const char* check_incidences(const std::vector<int32_t>& pairs, int N) {
	const int M = static_cast<int>(pairs.size() / 2);
	std::vector<int> off, list;
	incidence_csr(pairs.data(), M, N, off, list);
	if (static_cast<int>(off.size()) != N + 1 || static_cast<int>(list.size()) != 2 * M || off[0] != 0 || off[N] != 2 * M) return "incidence sizes";
	for (int n = 0; n < N; n++) {   // node n's list is exactly: every (s, t) with pairs[2 s + t] == n, ascending s, then t
		int u = off[n];
		for (int s = 0; s < M; s++)
			for (int t = 0; t < 2; t++)
				if (pairs[2 * s + t] == n) {
					if (u >= off[n + 1] || list[u] != 2 * s + t) return "incidence list differs from the naive one";
					u++;
				}
		if (u != off[n + 1]) return "incidence count differs from the naive one";
	}
	const std::vector<int> slot = incidence_slots(list);
	if (slot.size() != list.size()) return "slot size";
	for (int q = 0; q < 2 * M; q++)
		if (slot[q] < 0 || slot[q] >= 2 * M || list[slot[q]] != q || slot[list[q]] != q) return "inc_slot does not invert inc_list";
	return nullptr;
}

int main(int argc, char** argv) {
	if (argc > 1) {   // an edge list from a file
		FILE* f = fopen(argv[1], "rb");
		int32_t head[2] = {0, 0};
		if (!f || fread(head, sizeof(int32_t), 2, f) != 2 || head[0] < 0 || head[1] < 0) return fail("edge file header", -2);
		std::vector<int32_t> edges(2 * static_cast<size_t>(head[0]));
		const bool ok = fread(edges.data(), sizeof(int32_t), edges.size(), f) == edges.size();
		fclose(f);
		if (!ok) return fail("edge file body", -2);
		for (int32_t v : edges)
			if (v < 0 || v >= head[1]) return fail("edge file index out of range", -2);
		if (const char* what = check_incidences(edges, head[1])) return fail(what, -2);
		printf("%d edges over %d nodes ok\n", head[0], head[1]);
		return 0;
	}
	{   // incidence_csr at the degenerate sizes
		struct {
			int N;
			std::vector<int32_t> pairs;
		} const fixed[] = {
		    {0, {}},                                        // nothing at all
		    {5, {}},                                        // M = 0
		    {1, {}},                                        // N = 1, no pair
		    {1, {0, 0, 0, 0}},                              // N = 1: only self loops can exist (the edge form allows them)
		    {2, {0, 1}},                                    // one pair
		    {6, {0, 1, 1, 4, 0, 4}},                        // nodes 2, 3, 5 in no pair
		    {5, {2, 0, 2, 1, 3, 2, 2, 4}},                  // node 2 in every pair, on either side
		    {4, {3, 0, 3, 0, 0, 3}},                        // a doubled edge and its reverse
		};
		int c = 0;
		for (const auto& fx : fixed) {
			if (const char* what = check_incidences(fx.pairs, fx.N)) return fail(what, -100 - c);
			c++;
		}
	}
	std::mt19937 rng(17);
	int cases = 0;
	for (int c = 0; c < 200; c++, cases++) {
		const int N = 1 + static_cast<int>(rng() % 40);
		std::set<std::pair<int, int>> set;
		const int want = static_cast<int>(rng() % (3 * N + 1));
		for (int q = 0; q < want && N > 1; q++) {
			const int i = static_cast<int>(rng() % N), j = static_cast<int>(rng() % N);
			if (i != j) set.insert({std::min(i, j), std::max(i, j)});
		}
		std::vector<uint64_t> keys;
		for (auto& p : set) keys.push_back(static_cast<uint64_t>(p.first) << 32 | static_cast<uint64_t>(p.second));
		if (c % 2) keys.push_back(PAIR_KEY_NONE);   // the padding key of faces with fewer nodes than slots sorts last
		std::vector<int32_t> pairs;
		const int M = pairs_from_keys(keys, pairs);
		if (M != static_cast<int>(set.size()) || pairs.size() != 2 * set.size()) return fail("pairs_from_keys count", c);
		std::vector<int32_t> edges;
		for (int s = 0; s < M; s++)
			if (rng() % 3 == 0) {
				const bool flip = rng() % 2;
				edges.push_back(pairs[2 * s + (flip ? 1 : 0)]);
				edges.push_back(pairs[2 * s + (flip ? 0 : 1)]);
				if (rng() % 5 == 0) {   // a second edge on the same pair, the other way round
					edges.push_back(pairs[2 * s + (flip ? 0 : 1)]);
					edges.push_back(pairs[2 * s + (flip ? 1 : 0)]);
				}
			}
		const int E = static_cast<int>(edges.size() / 2);
		PairTables t;
		std::string err;
		if (!build_pair_tables(pairs.data(), M, N, edges.data(), E, t, &err)) return fail(err.c_str(), c);
		if (const char* what = check_incidences(pairs, N)) return fail(what, c);
		if (const char* what = check_incidences(edges, N)) return fail(what, c);
		if (static_cast<int>(t.row_off.size()) != N + 1 || t.row_off[N] != M || static_cast<int>(t.inc_off.size()) != N + 1 || t.inc_off[N] != 2 * M ||
		    static_cast<int>(t.edge_off.size()) != M + 1 || t.edge_off[M] != E || static_cast<int>(t.edge_list.size()) != E)
			return fail("table sizes", c);
		for (int i = 0; i < N; i++)
			for (int j = i + 1; j < N; j++) {
				const int s = find_pair(t.row_off, pairs.data(), i, j);
				if (set.count({i, j}) != (s >= 0)) return fail("find_pair presence", c);
				if (s >= 0 && (pairs[2 * s] != i || pairs[2 * s + 1] != j || s < t.row_off[i] || s >= t.row_off[i + 1])) return fail("find_pair slot", c);
			}
		std::vector<int> seen_edge(E, 0);
		for (int s = 0; s < M; s++)
			for (int u = t.edge_off[s]; u < t.edge_off[s + 1]; u++) {
				const int e = t.edge_list[u] >> 1, tr = t.edge_list[u] & 1;
				if (e < 0 || e >= E || seen_edge[e]++) return fail("edge listed twice or out of range", c);
				const int i = edges[2 * e], j = edges[2 * e + 1];
				if (std::min(i, j) != pairs[2 * s] || std::max(i, j) != pairs[2 * s + 1] || tr != (i > j)) return fail("edge on the wrong pair / orientation", c);
				if (u > t.edge_off[s] && (t.edge_list[u - 1] >> 1) >= e) return fail("edges of a pair not ascending", c);
			}
		for (int e = 0; e < E; e++)
			if (!seen_edge[e]) return fail("edge missing from the lists", c);
		std::vector<int> seen_inc(2 * M, 0);
		for (int n = 0; n < N; n++)
			for (int u = t.inc_off[n]; u < t.inc_off[n + 1]; u++) {
				const int code = t.inc_list[u];
				if (code < 0 || code >= 2 * M || seen_inc[code]++) return fail("incidence listed twice or out of range", c);
				if (pairs[2 * (code >> 1) + (code & 1)] != n) return fail("incidence at the wrong node", c);
				if (u > t.inc_off[n] && (t.inc_list[u - 1] >> 1) >= (code >> 1)) return fail("incidences of a node not ascending", c);
			}
	}
	// malformed input is refused
	{
		PairTables t;
		std::string err;
		const int32_t unsorted[] = {1, 2, 0, 3}, reversed[] = {2, 1}, range[] = {0, 5}, ok[] = {0, 1, 1, 2};
		const int32_t stray_edge[] = {0, 2}, loop_edge[] = {1, 1}, far_edge[] = {0, 9};
		if (build_pair_tables(unsorted, 2, 4, nullptr, 0, t, &err)) return fail("unsorted pairs accepted", -1);
		if (build_pair_tables(reversed, 1, 4, nullptr, 0, t, &err)) return fail("reversed pair accepted", -1);
		if (build_pair_tables(range, 1, 4, nullptr, 0, t, &err)) return fail("pair out of range accepted", -1);
		if (build_pair_tables(ok, 2, 3, stray_edge, 1, t, &err)) return fail("edge without a pair accepted", -1);
		if (build_pair_tables(ok, 2, 3, loop_edge, 1, t, &err)) return fail("diagonal edge accepted", -1);
		if (build_pair_tables(ok, 2, 3, far_edge, 1, t, &err)) return fail("edge out of range accepted", -1);
		if (!build_pair_tables(ok, 2, 3, nullptr, 0, t, &err)) return fail("valid pairs refused", -1);
		if (!build_pair_tables(nullptr, 0, 0, nullptr, 0, t, &err)) return fail("empty structure refused", -1);
		std::vector<int32_t> none;
		if (pairs_from_keys({}, none) != 0 || pairs_from_keys({PAIR_KEY_NONE}, none) != 0) return fail("empty key lists", -1);
	}
	printf("%d cases ok\n", cases);
	return 0;
}
