// Host check of two rules stated once in csrc/: the anchor-count dispatch (anchor_dispatch.hpp) and the voxel grid's
// hash-table sizing (hash_table_size.hpp, HashTable::size_for). Plain C++ under the host sanitizers.
//   - dispatch_anchor_count calls f once with each of 1..8 as an integral constant and returns f's status;
//   - it refuses 0, 9 and -1 with NNRT_ERROR_ARGUMENT and an error text, without calling f;
//   - the table size is 16 for 0 and 8 entries, the next power of two at or above 2n for n = 9, 2^20, 2^20 + 1, and
//     always a power of two above 2n - 1 (a table holding n keys is never more than half full).
// Prints "grid_rules_check OK" and returns 0, or the failed expectation and 1.
#include <cstdio>
#include <string>

#include "anchor_dispatch.hpp"
#include "hash_table_size.hpp"

namespace nnrt {
static std::string g_error;
void set_error(const std::string& m) { g_error = m; }
}   // namespace nnrt

using namespace nnrt;

static int failures = 0;
#define EXPECT(cond)                                                      \
	do {                                                                  \
		if (!(cond)) {                                                    \
			fprintf(stderr, "line %d: expected %s\n", __LINE__, #cond);   \
			failures++;                                                   \
		}                                                                 \
	} while (0)

int main() {
	for (int K = 1; K <= 8; K++) {
		int calls = 0, seen = 0;
		const nnrt_status want = K % 2 ? NNRT_OK : NNRT_ERROR_HIP;   // f's own status comes back
		const nnrt_status st = dispatch_anchor_count(K, [&](auto kk) {
			static_assert(decltype(kk)::value >= 1 && decltype(kk)::value <= 8, "instantiated for 1..8 only");
			calls++;
			seen = decltype(kk)::value;
			return want;
		});
		EXPECT(calls == 1 && seen == K && st == want);
	}
	for (int K : {0, 9, -1}) {
		int calls = 0;
		g_error.clear();
		const nnrt_status st = dispatch_anchor_count(K, [&](auto) {
			calls++;
			return NNRT_OK;
		});
		EXPECT(st == NNRT_ERROR_ARGUMENT && calls == 0 && !g_error.empty());
	}

	EXPECT(hash_table_size_for(0) == 16 && hash_table_size_for(8) == 16);
	EXPECT(hash_table_size_for(9) == 32);
	EXPECT(hash_table_size_for(int64_t{1} << 20) == uint64_t{1} << 21);
	EXPECT(hash_table_size_for((int64_t{1} << 20) + 1) == uint64_t{1} << 22);
	for (int64_t n = 0; n <= 5000; n++) {
		const uint64_t s = hash_table_size_for(n);
		EXPECT(s >= 16 && (s & (s - 1)) == 0);                             // a power of two
		EXPECT(static_cast<int64_t>(s) > 2 * n - 1);                        // never more than half full
		EXPECT(s == 16 || s / 2 < static_cast<uint64_t>(2 * n));            // and the smallest such
	}
	if (failures) return 1;
	printf("grid_rules_check OK\n");
	return 0;
}
