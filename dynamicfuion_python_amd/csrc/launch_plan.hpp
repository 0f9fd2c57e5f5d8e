// The fitter's per-frame launch choices: which kernel builds and work tables a frame's iterations use. Plain host C++
// (tests/native/launch_plan_check.cpp compiles it alone). read_launch_switches() is the only place the six development
// switches are read; choose_launches() is a pure function of them and of the frame's sizes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace nnrt {

// each switch: -1 = unset, otherwise the first character of its value (0 for an empty value)
struct LaunchSwitches {
	int tile_order = -1, pix_wpe4 = -1, quad_order = -1, anchors16 = -1, warp_vertex = -1, raster_dense = -1;
};

// a development switch of the library's, read from the environment in that form (the only getenv of the fitter's code)
inline int env_switch(const char* name) {
	const char* v = std::getenv(name);
	return v ? static_cast<int>(static_cast<unsigned char>(*v)) : -1;
}
// an on / off switch: unset = dflt, a value beginning with 0 = off, any other value = on (the corner's switches)
inline bool env_flag(const char* name, bool dflt) {
	const int v = env_switch(name);
	return v < 0 ? dflt : v != '0';
}

inline LaunchSwitches read_launch_switches() {
	LaunchSwitches sw;
	sw.tile_order = env_switch("NNRT_TILE_ORDER");
	sw.pix_wpe4 = env_switch("NNRT_PIX_WPE4");
	sw.quad_order = env_switch("NNRT_QUAD_ORDER");
	sw.anchors16 = env_switch("NNRT_ANCHORS16");
	sw.warp_vertex = env_switch("NNRT_WARP_VERTEX");
	sw.raster_dense = env_switch("NNRT_RASTER_DENSE");
	return sw;
}

// 0 / 1 each, in the order nnrt_fitter_launch_plan reports them
struct LaunchChoices {
	int32_t tile_order, quad_order, pix_low_occupancy, anchors16, warp_vertex, raster_dense;
};
constexpr int LAUNCH_CHOICE_COUNT = sizeof(LaunchChoices) / sizeof(int32_t);

// launch_warp_mesh's lane-per-vertex kernels (the launcher still takes the quad kernel when K > 4 or rows are gathered)
inline bool choose_warp_vertex(const LaunchSwitches& sw, int64_t V) {
	if (sw.warp_vertex >= 0) return sw.warp_vertex == '1';   // development switch: 0 / 1 force a path
	return V >= (int64_t{1} << 16);
}

// launch_raster_scatter_mesh's one-face-per-lane kernel
inline bool choose_raster_dense(const LaunchSwitches& sw, int64_t F, int H, int W) {
	if (sw.raster_dense >= 0) return sw.raster_dense == '1';   // development switch: 0 / 1 force a path
	return F >= static_cast<int64_t>(H) * W;
}

// cus: the device's compute units; tile_order_supported: fit_pixels_tile_order_supported()
inline LaunchChoices choose_launches(const LaunchSwitches& sw, int64_t V, int64_t F, int H, int W, int N, int K, int cus,
                                     bool tile_order_supported) {
	// the pixel launch's per-frame tile order, for launches of more than one residency round (5 waves per SIMD): their
	// last round's workgroups decide the tail, and the order gives those the tiles without reference pixels (C3 fused
	// launch 214 -> 197 us). In one round every wave starts at once and whole tiles are too coarse to change which SIMDs
	// carry the most working waves (C2 40.2 -> 41.8 with the tile table): those launches take the quadrant table below.
	// NNRT_TILE_ORDER=0: never, =2: always.
	const size_t tiles = static_cast<size_t>((W + 15) / 16) * static_cast<size_t>((H + 15) / 16);
	const bool multi_round = 4 * tiles > static_cast<size_t>(5 * 4 * cus);
	const bool tile_order_wanted = tile_order_supported && (sw.tile_order == '0' ? false : sw.tile_order == '2' ? true : multi_round);
	// the same launches take the pixel kernel's 4-waves-per-SIMD build: their pass-2 gathers miss L2 (C3's 72-MB
	// canonical mesh) and fewer, spill-free waves congest the memory pipeline less (C3 fused launch 198.6 -> 188 us; at C2,
	// one round, 40.4 -> 47.2). NNRT_PIX_WPE4=0 / 1 forces.
	const bool pix_low = sw.pix_wpe4 >= 0 ? sw.pix_wpe4 == '1' : multi_round;
	// launches of one residency round take the quadrant-granular table instead: their length follows the SIMDs that
	// hold five working waves while others hold three and idle ones, and the table deals each XCD band's working
	// quadrants out first (launch_quad_order; C2 fused launch 38.5 -> 35.3 us with the 5-wave build, 36.3 with the 4-wave
	// build). NNRT_QUAD_ORDER=0: never, =1: always; a forced tile table (NNRT_TILE_ORDER=2) keeps it off.
	const bool quad_order =
	    tile_order_supported && (sw.quad_order == '0' ? false : sw.quad_order == '1' ? true : !multi_round && sw.tile_order != '2');
	LaunchChoices c{};
	c.tile_order = tile_order_wanted && !quad_order;   // one table per launch
	c.quad_order = quad_order;
	c.pix_low_occupancy = pix_low;
	// the warp's 16-bit anchor copy (every index fits: N < 65535; -1 as 0xFFFF); NNRT_ANCHORS16 is a development
	// switch: 0 = the int32 anchors
	c.anchors16 = K == 4 && N < 65535 && sw.anchors16 != '0';
	c.warp_vertex = choose_warp_vertex(sw, V);
	c.raster_dense = choose_raster_dense(sw, F, H, W);
	return c;
}

} // namespace nnrt
