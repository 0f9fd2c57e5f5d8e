// The anchor-count dispatch. Kernels that keep a point's K anchors in registers are templates over K; every launcher
// picks its instantiation here. Plain host C++ (tests/native/grid_rules_check.cpp compiles it alone).
#pragma once
#include <string>
#include <type_traits>

#include "nnrt_mi355x.h"

namespace nnrt {

void set_error(const std::string& message);

// f(std::integral_constant<int, K>{}) for K in 1..8, returning f's status; any other K is refused and f is not called
template <typename F>
nnrt_status dispatch_anchor_count(int K, F&& f) {
	switch (K) {
		case 1: return f(std::integral_constant<int, 1>{});
		case 2: return f(std::integral_constant<int, 2>{});
		case 3: return f(std::integral_constant<int, 3>{});
		case 4: return f(std::integral_constant<int, 4>{});
		case 5: return f(std::integral_constant<int, 5>{});
		case 6: return f(std::integral_constant<int, 6>{});
		case 7: return f(std::integral_constant<int, 7>{});
		case 8: return f(std::integral_constant<int, 8>{});
	}
	set_error("invalid argument: anchor_count must be in [1, 8]");
	return NNRT_ERROR_ARGUMENT;
}

} // namespace nnrt
