// The voxel grid's one hash-table sizing rule (HashTable::size_for, tsdf_grid.hpp). Plain host C++
// (tests/native/grid_rules_check.cpp compiles it alone).
#pragma once
#include <cstdint>

namespace nnrt {

// slots for `entries` keys: a power of two, at least 16 and at least 2 * entries, so that a table holding them is never
// more than half full and linear probing always meets an empty slot
inline uint64_t hash_table_size_for(int64_t entries) {
	uint64_t size = 16;
	while (size < static_cast<uint64_t>(2 * entries)) size <<= 1;
	return size;
}

} // namespace nnrt
