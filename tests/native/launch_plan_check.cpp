// Host check of the fitter's launch choices (csrc/launch_plan.hpp choose_launches): a table of cases, each with the six
// choices written out by hand from the rules -- every switch unset and forced, the pixel launch's tile count one below,
// at and one above the residency-round boundary (5 * compute units), K in {3, 4}, N in {65534, 65535}, V in
// {65535, 65536}, F in {H W - 1, H W}, and a forced tile table against a forced quadrant table. No device is touched.
#include <cstdio>
#include <cstdlib>

#include "launch_plan.hpp"

using namespace nnrt;

namespace {
constexpr int U = -1;   // switch unset
struct Case {
	const char* name;
	LaunchSwitches sw;   // tile_order, pix_wpe4, quad_order, anchors16, warp_vertex, raster_dense
	int64_t V, F;
	int H, W, N, K, cus;
	bool supported;
	LaunchChoices want;   // tile_order, quad_order, pix_low_occupancy, anchors16, warp_vertex, raster_dense
};

// 256 compute units: one residency round holds 5 * 256 = 1280 tiles. 640 x 480 is 40 x 30 = 1200 tiles (one round),
// 1280 x 960 is 80 x 60 = 4800 (several).
const Case CASES[] = {
    {"one round, nothing set", {U, U, U, U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"several rounds, nothing set", {U, U, U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {1, 0, 1, 1, 0, 0}},
    // the boundary: 1279 = 1279 x 1, 1280 = 40 x 32, 1281 = 21 x 61 tiles
    {"1279 tiles", {U, U, U, U, U, U}, 1000, 2000, 16, 16 * 1279, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"1280 tiles", {U, U, U, U, U, U}, 1000, 2000, 512, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"1281 tiles", {U, U, U, U, U, U}, 1000, 2000, 976, 336, 100, 4, 256, true, {1, 0, 1, 1, 0, 0}},
    {"1281 tiles, ragged image", {U, U, U, U, U, U}, 1000, 2000, 976 - 15, 336 - 15, 100, 4, 256, true, {1, 0, 1, 1, 0, 0}},
    // 4 compute units: 20 tiles a round; 19 = 19 x 1, 20 = 5 x 4, 21 = 7 x 3
    {"4 CUs, 19 tiles", {U, U, U, U, U, U}, 1000, 2000, 16, 304, 100, 4, 4, true, {0, 1, 0, 1, 0, 0}},
    {"4 CUs, 20 tiles", {U, U, U, U, U, U}, 1000, 2000, 64, 80, 100, 4, 4, true, {0, 1, 0, 1, 0, 0}},
    {"4 CUs, 21 tiles", {U, U, U, U, U, U}, 1000, 2000, 48, 112, 100, 4, 4, true, {1, 0, 1, 1, 0, 0}},
    // NNRT_TILE_ORDER: 0 never, 2 always (and keeps the quadrant table off), anything else the default
    {"TILE_ORDER=0, several rounds", {'0', U, U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {0, 0, 1, 1, 0, 0}},
    {"TILE_ORDER=0, one round", {'0', U, U, U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"TILE_ORDER=2, one round", {'2', U, U, U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {1, 0, 0, 1, 0, 0}},
    {"TILE_ORDER=2, several rounds", {'2', U, U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {1, 0, 1, 1, 0, 0}},
    {"TILE_ORDER=1, one round", {'1', U, U, U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"TILE_ORDER empty, several rounds", {0, U, U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {1, 0, 1, 1, 0, 0}},
    // NNRT_QUAD_ORDER: 0 never, 1 always; one table per launch
    {"QUAD_ORDER=0, one round", {U, U, '0', U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 0, 0, 1, 0, 0}},
    {"QUAD_ORDER=0, several rounds", {U, U, '0', U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {1, 0, 1, 1, 0, 0}},
    {"QUAD_ORDER=1, several rounds", {U, U, '1', U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {0, 1, 1, 1, 0, 0}},
    {"QUAD_ORDER=2, one round", {U, U, '2', U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"forced tile table against forced quad table", {'2', U, '1', U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"forced tile table, quad table off", {'2', U, '0', U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {1, 0, 0, 1, 0, 0}},
    {"both tables off", {'0', U, '0', U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {0, 0, 1, 1, 0, 0}},
    // a build whose pixel launch ignores the tables
    {"tables unsupported, several rounds", {U, U, U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, false, {0, 0, 1, 1, 0, 0}},
    {"tables unsupported, both forced", {'2', U, '1', U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, false, {0, 0, 0, 1, 0, 0}},
    // NNRT_PIX_WPE4: set = forced to (value == 1)
    {"PIX_WPE4=1, one round", {U, '1', U, U, U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 1, 1, 0, 0}},
    {"PIX_WPE4=0, several rounds", {U, '0', U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {1, 0, 0, 1, 0, 0}},
    {"PIX_WPE4 empty, several rounds", {U, 0, U, U, U, U}, 1000, 2000, 960, 1280, 100, 4, 256, true, {1, 0, 0, 1, 0, 0}},
    // anchors16 needs K == 4 and N < 65535; NNRT_ANCHORS16=0 turns it off, nothing turns it on
    {"K = 3", {U, U, U, U, U, U}, 1000, 2000, 480, 640, 100, 3, 256, true, {0, 1, 0, 0, 0, 0}},
    {"N = 65534", {U, U, U, U, U, U}, 1000, 2000, 480, 640, 65534, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"N = 65535", {U, U, U, U, U, U}, 1000, 2000, 480, 640, 65535, 4, 256, true, {0, 1, 0, 0, 0, 0}},
    {"ANCHORS16=0", {U, U, U, '0', U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 0, 0, 0}},
    {"ANCHORS16=1", {U, U, U, '1', U, U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"ANCHORS16=1, K = 3", {U, U, U, '1', U, U}, 1000, 2000, 480, 640, 100, 3, 256, true, {0, 1, 0, 0, 0, 0}},
    {"ANCHORS16=1, N = 65535", {U, U, U, '1', U, U}, 1000, 2000, 480, 640, 65535, 4, 256, true, {0, 1, 0, 0, 0, 0}},
    // the warp's vertex path: V >= 2^16; NNRT_WARP_VERTEX set = forced to (value == 1)
    {"V = 65535", {U, U, U, U, U, U}, 65535, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"V = 65536", {U, U, U, U, U, U}, 65536, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 1, 0}},
    {"WARP_VERTEX=1, small mesh", {U, U, U, U, '1', U}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 1, 0}},
    {"WARP_VERTEX=0, large mesh", {U, U, U, U, '0', U}, 65536, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"WARP_VERTEX=1, K = 3 (the launcher decides about K)", {U, U, U, U, '1', U}, 1000, 2000, 480, 640, 100, 3, 256, true, {0, 1, 0, 0, 1, 0}},
    // the dense raster: F >= H W; NNRT_RASTER_DENSE set = forced to (value == 1)
    {"F = H W - 1", {U, U, U, U, U, U}, 1000, 480 * 640 - 1, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    {"F = H W", {U, U, U, U, U, U}, 1000, 480 * 640, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 1}},
    {"RASTER_DENSE=1, sparse mesh", {U, U, U, U, U, '1'}, 1000, 2000, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 1}},
    {"RASTER_DENSE=0, dense mesh", {U, U, U, U, U, '0'}, 1000, 480 * 640, 480, 640, 100, 4, 256, true, {0, 1, 0, 1, 0, 0}},
    // everything forced against every default
    {"all forced", {'2', '0', '0', '0', '0', '0'}, 65536, 4 * 960 * 1280, 960, 1280, 100, 4, 256, true, {1, 0, 0, 0, 0, 0}},
};
} // namespace

int main() {
	int bad = 0, count = 0;
	for (const Case& c : CASES) {
		const LaunchChoices got = choose_launches(c.sw, c.V, c.F, c.H, c.W, c.N, c.K, c.cus, c.supported);
		const int32_t g[6] = {got.tile_order, got.quad_order, got.pix_low_occupancy, got.anchors16, got.warp_vertex, got.raster_dense};
		const int32_t w[6] = {c.want.tile_order, c.want.quad_order, c.want.pix_low_occupancy, c.want.anchors16, c.want.warp_vertex, c.want.raster_dense};
		bool same = true;
		for (int i = 0; i < 6; i++) same = same && g[i] == w[i];
		if (!same) {
			std::printf("MISMATCH %s: got %d %d %d %d %d %d, want %d %d %d %d %d %d\n", c.name, g[0], g[1], g[2], g[3], g[4], g[5], w[0], w[1], w[2], w[3],
			            w[4], w[5]);
			bad++;
		}
		// the stateless warp wrapper and the fitter must agree on the two launcher choices
		if (choose_warp_vertex(c.sw, c.V) != (got.warp_vertex != 0) || choose_raster_dense(c.sw, c.F, c.H, c.W) != (got.raster_dense != 0)) {
			std::printf("MISMATCH %s: launcher choice differs from the plan's\n", c.name);
			bad++;
		}
		count++;
	}
	// the reader: unset = -1, otherwise the value's first character
	setenv("NNRT_TILE_ORDER", "2", 1);
	setenv("NNRT_PIX_WPE4", "", 1);
	unsetenv("NNRT_QUAD_ORDER");
	setenv("NNRT_ANCHORS16", "0", 1);
	setenv("NNRT_WARP_VERTEX", "1", 1);
	setenv("NNRT_RASTER_DENSE", "10", 1);
	const LaunchSwitches sw = read_launch_switches();
	if (sw.tile_order != '2' || sw.pix_wpe4 != 0 || sw.quad_order != -1 || sw.anchors16 != '0' || sw.warp_vertex != '1' || sw.raster_dense != '1') {
		std::printf("MISMATCH read_launch_switches: %d %d %d %d %d %d\n", sw.tile_order, sw.pix_wpe4, sw.quad_order, sw.anchors16, sw.warp_vertex,
		            sw.raster_dense);
		bad++;
	}
	if (bad) return 1;
	std::printf("launch plan: %d cases ok\n", count);
	return 0;
}
