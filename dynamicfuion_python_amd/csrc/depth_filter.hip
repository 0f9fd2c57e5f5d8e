// Depth image filters ahead of tracking: the reference's zero-skipping median
// (cpp/pybind/nnrt_pybind.cpp:97-104 -> cpp/cpu/image_proc.cpp:837-887) and a table-driven bilateral smoother, which the
// reference does not have.
//
// Both are stencils over an [H, W] image. One 256-thread workgroup (four wavefronts) owns a 16 x 16 tile of output
// pixels, thread (tx, ty) = (t % 16, t / 16) the pixel (16 bx + tx, 16 by + ty); a wavefront is four tile rows. The tile
// and its halo of `radius` pixels, (16 + 2 radius)^2 <= 32 x 32 values, are staged once in LDS (positions outside the
// image hold 0 and are never read: each pixel's window is clipped to the image by its loop bounds, which are fixed
// before the loops start). Within a 32-lane half of a wavefront the lanes read two rows of 16 consecutive values:
// 2 x 9 dwords (uint16) or 2 x 16 dwords (float) of distinct banks, or the same dword twice, which broadcasts. Every
// output pixel is written by its own thread with a plain vector store; there are no atomics.
#include "kernels.hpp"

namespace nnrt {

namespace {

constexpr int TILE = 16;
constexpr int MAX_RADIUS = NNRT_DEPTH_FILTER_MAX_RADIUS;
constexpr int MAX_SIDE = TILE + 2 * MAX_RADIUS;
constexpr int MAX_RANGE_WEIGHTS = NNRT_BILATERAL_MAX_RANGE_WEIGHTS;

// The clipped window of pixel (x, y) as offsets into the staged tile: rows [y0, y1], columns [x0, x1] of the LDS image,
// whose origin is the image pixel (16 bx - r, 16 by - r).
struct Window {
	int x0, x1, y0, y1;
};
__device__ inline Window clipped_window(int x, int y, int tx, int ty, int r, int H, int W) {
	Window w;
	w.x0 = tx + r - min(r, x);
	w.x1 = tx + r + min(r, W - 1 - x);
	w.y0 = ty + r - min(r, y);
	w.y1 = ty + r + min(r, H - 1 - y);
	return w;
}

// Median of the values > 0 of the clipped window: element n / 2 of their ascending order (n of them), 0 if n == 0.
// LDS holds value - 1 in 16 bits, so an empty position (0) is 0xffff and never counts as "below" any 16-bit candidate.
// The k-th smallest (k = n / 2 + 1) stored value t is built bit by bit from the top: a candidate c is kept while fewer
// than k stored values are below it, which leaves the largest t with count(< t) < k, i.e. count(<= t) >= k. Sixteen
// counting passes over the window, whatever the data.
__global__ void __launch_bounds__(TILE* TILE) k_median_depth(const uint16_t* __restrict__ in, int H, int W, int r, int preserve_zero,
                                                              uint16_t* __restrict__ out) {
	__shared__ uint16_t s_tile[MAX_SIDE * MAX_SIDE];
	const int side = TILE + 2 * r;
	const int t = static_cast<int>(threadIdx.x);
	const int ox = static_cast<int>(blockIdx.x) * TILE - r, oy = static_cast<int>(blockIdx.y) * TILE - r;
	for (int i = t; i < side * side; i += TILE * TILE) {
		const int gx = ox + i % side, gy = oy + i / side;
		const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
		const uint16_t v = inside ? in[static_cast<int64_t>(gy) * W + gx] : uint16_t(0);
		s_tile[i] = static_cast<uint16_t>(v - 1u);
	}
	__syncthreads();
	const int tx = t % TILE, ty = t / TILE;
	const int x = ox + r + tx, y = oy + r + ty;
	if (x >= W || y >= H) return;
	uint32_t result = 0;
	const bool hole = s_tile[(ty + r) * side + tx + r] == 0xffffu;
	if (!(preserve_zero && hole)) {
		const Window w = clipped_window(x, y, tx, ty, r, H, W);
		uint32_t n = 0;
		for (int yy = w.y0; yy <= w.y1; yy++) {
			for (int xx = w.x0; xx <= w.x1; xx++) n += s_tile[yy * side + xx] != 0xffffu ? 1u : 0u;
		}
		if (n > 0) {
			const uint32_t k = n / 2 + 1;
			uint32_t found = 0;
			for (int bit = 15; bit >= 0; bit--) {
				const uint32_t candidate = found | (1u << bit);
				uint32_t below = 0;
				for (int yy = w.y0; yy <= w.y1; yy++) {
					for (int xx = w.x0; xx <= w.x1; xx++) below += static_cast<uint32_t>(s_tile[yy * side + xx]) < candidate ? 1u : 0u;
				}
				if (below < k) found = candidate;
			}
			result = found + 1u;
		}
	}
	out[static_cast<int64_t>(y) * W + x] = static_cast<uint16_t>(result);
}

__device__ inline bool valid_depth(float v) { return v > 0.f && v <= 3.402823466e+38f; }   // false for NaN and +inf

// Bilateral filter with host-built weight tables (no exp here): float32 arithmetic in the order DESIGN.md section 20
// writes down, dy outer and dx inner, so a float32 restatement equals it bit for bit. The range table is staged in LDS
// next to the tile (at most 16 KB).
template <typename T>
__global__ void __launch_bounds__(TILE* TILE) k_bilateral_depth(const T* __restrict__ in, int H, int W, int r, const float* __restrict__ spatial,
                                                                 const float* __restrict__ range, int range_count, float index_scale,
                                                                 float depth_scale, float* __restrict__ out) {
	__shared__ float s_tile[MAX_SIDE * MAX_SIDE];
	__shared__ float s_spatial[(2 * MAX_RADIUS + 1) * (2 * MAX_RADIUS + 1)];
	__shared__ float s_range[MAX_RANGE_WEIGHTS];
	const int side = TILE + 2 * r, taps = 2 * r + 1;
	const int t = static_cast<int>(threadIdx.x);
	const int ox = static_cast<int>(blockIdx.x) * TILE - r, oy = static_cast<int>(blockIdx.y) * TILE - r;
	for (int i = t; i < side * side; i += TILE * TILE) {
		const int gx = ox + i % side, gy = oy + i / side;
		const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
		s_tile[i] = inside ? static_cast<float>(in[static_cast<int64_t>(gy) * W + gx]) : 0.f;
	}
	for (int i = t; i < taps * taps; i += TILE * TILE) s_spatial[i] = spatial[i];
	for (int i = t; i < range_count; i += TILE * TILE) s_range[i] = range[i];
	__syncthreads();
	const int tx = t % TILE, ty = t / TILE;
	const int x = ox + r + tx, y = oy + r + ty;
	if (x >= W || y >= H) return;
	const float c = s_tile[(ty + r) * side + tx + r];
	float result = 0.f;
	if (valid_depth(c)) {
		const Window w = clipped_window(x, y, tx, ty, r, H, W);
		const float limit = static_cast<float>(range_count);
		float sum_w = 0.f, sum_v = 0.f;
		for (int yy = w.y0; yy <= w.y1; yy++) {
			const int row = (yy - ty) * taps - tx;   // spatial[dy + r][dx + r] with dy + r = yy - ty, dx + r = xx - tx
			for (int xx = w.x0; xx <= w.x1; xx++) {
				const float v = s_tile[yy * side + xx];
				if (!valid_depth(v)) continue;
				const float f = fabsf(v - c) * index_scale;
				if (!(f < limit)) continue;   // int(f) >= range_count; also an overflowed difference
				const float wgt = s_spatial[row + xx] * s_range[static_cast<int>(f)];
				sum_w = sum_w + wgt;
				sum_v = sum_v + wgt * v;
			}
		}
		if (sum_w > 0.f) result = (sum_v / sum_w) / depth_scale;
	}
	out[static_cast<int64_t>(y) * W + x] = result;
}

dim3 tile_grid(int H, int W) { return dim3(static_cast<unsigned>(ceil_div(W, TILE)), static_cast<unsigned>(ceil_div(H, TILE)), 1); }

} // namespace

nnrt_status launch_filter_depth_median(const uint16_t* in, int H, int W, int radius, bool preserve_zero, uint16_t* out, hipStream_t stream) {
	if (static_cast<int64_t>(H) * W == 0) return NNRT_OK;
	k_median_depth<<<tile_grid(H, W), TILE * TILE, 0, stream>>>(in, H, W, radius, preserve_zero ? 1 : 0, out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_filter_depth_bilateral(const void* in, int in_dtype, int H, int W, int radius, const float* spatial, const float* range,
                                          int range_count, float index_scale, float depth_scale, float* out, hipStream_t stream) {
	if (static_cast<int64_t>(H) * W == 0) return NNRT_OK;
	if (in_dtype == NNRT_DTYPE_UINT16) {
		k_bilateral_depth<uint16_t><<<tile_grid(H, W), TILE * TILE, 0, stream>>>(static_cast<const uint16_t*>(in), H, W, radius, spatial, range,
		                                                                        range_count, index_scale, depth_scale, out);
	} else {
		k_bilateral_depth<float><<<tile_grid(H, W), TILE * TILE, 0, stream>>>(static_cast<const float*>(in), H, W, radius, spatial, range,
		                                                                     range_count, index_scale, depth_scale, out);
	}
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
