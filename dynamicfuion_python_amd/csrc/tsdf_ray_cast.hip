// =====================================================================================================================
// Ray cast of the voxel block grid (tsdf_grid.hpp): the range map and the march.
// RayCast (VoxelBlockGrid.cpp:353-427 -> Open3D voxel_grid::EstimateRange + RayCast; restated in DESIGN.md section 19
// with two deviations from Open3D: ceiling-sized range map, empty blocks left through their box instead of by one side).
// All arithmetic is float32 in the order DESIGN states; tests/_ray_cast_util.py restates it in numpy bit for bit.
// Every loop below has an integer trip bound.
// =====================================================================================================================
#include <climits>
#include <cmath>

#include "tsdf_grid.hpp"

namespace nnrt {
namespace {

constexpr int RC_TILE = 8;      // one wavefront renders 8 x 8 pixels
constexpr int RC_BLOCK = 256;   // 4 wavefronts
constexpr int RC_MAX_STEPS = 1 << 20;

struct RayCastArgs {
	int W, H;
	int tiles_x, tiles_y;   // 8 x 8 pixel tiles of the image (one wavefront each)
	int f, TW, TH;          // range_map_down_factor and the range map's size
	int attr;               // NNRT_RAY_CAST_* bits
	int max_steps;
	float depth_scale, weight_threshold, sdf_trunc;
	Xform pose;   // camera -> world: float rows of the inverted extrinsic, and the intrinsics
	const float* range;
	float *depth, *vertex, *normal, *color;
};

// every entry starts at (depth_max, depth_min): a tile no block reaches has an empty range
__global__ void k_range_init(float* __restrict__ range, int64_t n, float depth_max, float depth_min) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i < n) range[i] = (i & 1) ? depth_min : depth_max;
}

// (a) range map: one wavefront per block coordinate; lanes stride over the tiles its projection covers. Non-negative
// floats order as their bit patterns, so min / max are unsigned integer atomics: the result is order-independent.
__global__ __launch_bounds__(RC_BLOCK) void k_range_blocks(GridView g, const int32_t* __restrict__ coords, int64_t count, Xform world_to_cam, int f,
                                                           int TW, int TH, float depth_min, float depth_max, unsigned* __restrict__ range) {
	const int64_t wave = (static_cast<int64_t>(blockIdx.x) * RC_BLOCK + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (wave >= count) return;
	const int bx = coords[3 * wave], by = coords[3 * wave + 1], bz = coords[3 * wave + 2];
	if (find_block(g.hash, bx, by, bz) < 0) return;   // inactive (or out of key range): contributes nothing
	const float side = static_cast<float>(g.res) * g.voxel_size;
	float zmin = INFINITY, zmax = -INFINITY, umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
	bool any_behind = false;
#pragma unroll
	for (int c = 0; c < 8; c++) {
		const float x = static_cast<float>(bx + (c & 1)) * side, y = static_cast<float>(by + ((c >> 1) & 1)) * side,
		            z = static_cast<float>(bz + (c >> 2)) * side;
		float xc, yc, zc;
		world_to_cam.rigid(x, y, z, xc, yc, zc);
		zmin = fminf(zmin, zc);
		zmax = fmaxf(zmax, zc);
		if (zc <= 0.f) {
			any_behind = true;
		} else {
			float u, v;
			world_to_cam.project(xc, yc, zc, u, v);
			umin = fminf(umin, u);
			umax = fmaxf(umax, u);
			vmin = fminf(vmin, v);
			vmax = fmaxf(vmax, v);
		}
	}
	if (!(zmax > 0.f)) return;   // all eight corners behind the camera
	int x0 = 0, x1 = TW - 1, y0 = 0, y1 = TH - 1;
	float z_lo = depth_min;
	if (!any_behind) {
		const float ff = static_cast<float>(f);
		const float fx0 = fmaxf(floorf(umin / ff), 0.f), fx1 = fminf(floorf(umax / ff), static_cast<float>(TW - 1));
		const float fy0 = fmaxf(floorf(vmin / ff), 0.f), fy1 = fminf(floorf(vmax / ff), static_cast<float>(TH - 1));
		if (!(fx0 <= fx1 && fy0 <= fy1)) return;   // off the map
		x0 = static_cast<int>(fx0);   // all four lie in [0, TW - 1] x [0, TH - 1] here
		x1 = static_cast<int>(fx1);
		y0 = static_cast<int>(fy0);
		y1 = static_cast<int>(fy1);
		z_lo = fmaxf(zmin, depth_min);
	}
	const float z_hi = fminf(zmax, depth_max);
	if (!(z_lo < z_hi)) return;
	const unsigned lo = __float_as_uint(z_lo), hi = __float_as_uint(z_hi);
	const int rw = x1 - x0 + 1;
	const int64_t n = static_cast<int64_t>(rw) * (y1 - y0 + 1);
	for (int64_t i = lane; i < n; i += 64) {
		const int64_t tile = (y0 + i / rw) * TW + (x0 + i % rw);
		atomicMin(range + 2 * tile, lo);
		atomicMax(range + 2 * tile + 1, hi);
	}
}

// floor division of a voxel coordinate into (block, voxel inside the block)
__device__ inline void split_voxel(int q, int res, int& block, int& local) {
	block = q / res;
	local = q - block * res;
	if (local < 0) {
		block -= 1;
		local += res;
	}
}

// each lane's last (block key -> buffer index) pair: neighbouring steps of a ray mostly stay in one block
struct BlockCache {
	int x, y, z, buf;
};
__device__ inline int cached_block(const HashView& h, BlockCache& c, int x, int y, int z) {
	if (x != c.x || y != c.y || z != c.z) {
		c.buf = find_block(h, x, y, z);
		c.x = x;
		c.y = y;
		c.z = z;
	}
	return c.buf;
}

// (b) march + (c) outputs: one wavefront per 8 x 8 pixel tile, one ray per lane; lanes leave the loop on their own
__global__ __launch_bounds__(RC_BLOCK) void k_ray_cast(GridView g, RayCastArgs a) {
	const int64_t wave = (static_cast<int64_t>(blockIdx.x) * RC_BLOCK + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (wave >= static_cast<int64_t>(a.tiles_x) * a.tiles_y) return;
	const int x = static_cast<int>(wave % a.tiles_x) * RC_TILE + (lane & 7), y = static_cast<int>(wave / a.tiles_x) * RC_TILE + (lane >> 3);
	if (x >= a.W || y >= a.H) return;
	const int64_t pix = static_cast<int64_t>(y) * a.W + x;

	const float* m = a.pose.m;
	const float ca = (static_cast<float>(x) - a.pose.cx) / a.pose.fx, cb = (static_cast<float>(y) - a.pose.cy) / a.pose.fy;
	const float dw[3] = {(ca * m[0] + cb * m[1]) + m[2], (ca * m[4] + cb * m[5]) + m[6], (ca * m[8] + cb * m[9]) + m[10]};
	const float o[3] = {m[3], m[7], m[11]};
	const float vs = g.voxel_size, half_voxel = 0.5f * vs, side = static_cast<float>(g.res) * vs;

	const int64_t tile = static_cast<int64_t>(y / a.f) * a.TW + x / a.f;
	float t = a.range[2 * tile];
	const float t_max = a.range[2 * tile + 1];
	BlockCache cache{INT_MIN, INT_MIN, INT_MIN, -1};
	bool have_prev = false, hit = false;
	float t_prev = 0.f, tsdf_prev = 0.f, t_hit = 0.f;
	for (int step = 0; step < a.max_steps; step++) {
		if (!(t < t_max)) break;
		int b[3], l[3];
#pragma unroll
		for (int k = 0; k < 3; k++) split_voxel(static_cast<int>(floorf((o[k] + t * dw[k]) / vs)), g.res, b[k], l[k]);
		const int buf = cached_block(g.hash, cache, b[0], b[1], b[2]);
		if (buf < 0) {
			// leave the absent block's box, plus half a voxel
			have_prev = false;
			float t_exit = INFINITY;
#pragma unroll
			for (int k = 0; k < 3; k++)
				if (dw[k] != 0.f) t_exit = fminf(t_exit, (static_cast<float>(b[k] + (dw[k] > 0.f ? 1 : 0)) * side - o[k]) / dw[k]);
			t = fmaxf(t_exit, t) + half_voxel;
			continue;
		}
		const int64_t lin = static_cast<int64_t>(buf) * g.res3 + (l[0] + g.res * (l[1] + g.res * l[2]));
		if (read_store(g.weight, g.weight_type, lin) < a.weight_threshold) {
			have_prev = false;
			t += vs;
			continue;
		}
		const float tsdf = g.tsdf[lin];
		if (have_prev && tsdf_prev > 0.f && tsdf <= 0.f) {
			t_hit = (t * tsdf_prev - t_prev * tsdf) / (tsdf_prev - tsdf);
			hit = true;
			break;
		}
		tsdf_prev = tsdf;
		t_prev = t;
		have_prev = true;
		const float d = tsdf * a.sdf_trunc;
		t += d < vs ? vs : d;
	}

	float vtx[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
	float depth = 0.f;
	if (hit) {
		depth = t_hit * a.depth_scale;
#pragma unroll
		for (int k = 0; k < 3; k++) vtx[k] = o[k] + t_hit * dw[k];
		if (a.attr & (NNRT_RAY_CAST_NORMAL | NNRT_RAY_CAST_COLOR)) {
			// the interpolation cell: 8 voxels base + (i, j, k), corner c = i + 2 j + 4 k, weights (wx_i wy_j) wz_k
			int base[3];
			float r[3], u[3];
#pragma unroll
			for (int k = 0; k < 3; k++) {
				const float gk = vtx[k] / vs, fl = floorf(gk);
				base[k] = static_cast<int>(fl);
				r[k] = gk - fl;
				u[k] = 1.0f - r[k];
			}
			const bool want_color = (a.attr & NNRT_RAY_CAST_COLOR) != 0;
			float T[8];
			float wsum = 0.f, csum[3] = {0.f, 0.f, 0.f};
			bool all_valid = true;
#pragma unroll
			for (int c = 0; c < 8; c++) {
				const int i = c & 1, j = (c >> 1) & 1, k = c >> 2;
				int bb[3], ll[3];
				split_voxel(base[0] + i, g.res, bb[0], ll[0]);
				split_voxel(base[1] + j, g.res, bb[1], ll[1]);
				split_voxel(base[2] + k, g.res, bb[2], ll[2]);
				const int cbuf = cached_block(g.hash, cache, bb[0], bb[1], bb[2]);
				bool valid = false;
				T[c] = 0.f;
				if (cbuf >= 0) {
					const int64_t lin = static_cast<int64_t>(cbuf) * g.res3 + (ll[0] + g.res * (ll[1] + g.res * ll[2]));
					if (read_store(g.weight, g.weight_type, lin) >= a.weight_threshold) {
						valid = true;
						T[c] = g.tsdf[lin];
						if (want_color) {
							const float w = ((i ? r[0] : u[0]) * (j ? r[1] : u[1])) * (k ? r[2] : u[2]);
							wsum += w;
#pragma unroll
							for (int ch = 0; ch < 3; ch++) csum[ch] += w * read_store(g.color, g.color_type, 3 * lin + ch);
						}
					}
				}
				all_valid = all_valid && valid;
			}
			if (want_color && wsum > 0.f) {
#pragma unroll
				for (int ch = 0; ch < 3; ch++) col[ch] = (csum[ch] / wsum) / 255.0f;
			}
			if ((a.attr & NNRT_RAY_CAST_NORMAL) && all_valid) {
				// gradient of the trilinear interpolant at r (DESIGN section 19 writes these three lines out)
				const float gx = (((T[1] - T[0]) * u[1]) * u[2] + ((T[3] - T[2]) * r[1]) * u[2]) + (((T[5] - T[4]) * u[1]) * r[2] + ((T[7] - T[6]) * r[1]) * r[2]);
				const float gy = (((T[2] - T[0]) * u[0]) * u[2] + ((T[3] - T[1]) * r[0]) * u[2]) + (((T[6] - T[4]) * u[0]) * r[2] + ((T[7] - T[5]) * r[0]) * r[2]);
				const float gz = (((T[4] - T[0]) * u[0]) * u[1] + ((T[5] - T[1]) * r[0]) * u[1]) + (((T[6] - T[2]) * u[0]) * r[1] + ((T[7] - T[3]) * r[0]) * r[1]);
				const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
				if (len > 0.f) {
					nrm[0] = gx / len;
					nrm[1] = gy / len;
					nrm[2] = gz / len;
				}
			}
		}
	}
	if (a.attr & NNRT_RAY_CAST_DEPTH) a.depth[pix] = depth;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		if (a.attr & NNRT_RAY_CAST_VERTEX) a.vertex[3 * pix + k] = vtx[k];
		if (a.attr & NNRT_RAY_CAST_NORMAL) a.normal[3 * pix + k] = nrm[k];
		if (a.attr & NNRT_RAY_CAST_COLOR) a.color[3 * pix + k] = col[k];
	}
}

} // namespace
} // namespace nnrt

using namespace nnrt;

extern "C" {

nnrt_status nnrt_voxel_grid_ray_cast(nnrt_voxel_grid* vg, const int32_t* d_block_coords, int64_t count, const double* h_K, const double* h_E,
                                     int32_t width, int32_t height, int32_t attribute_mask, float depth_scale, float depth_min, float depth_max,
                                     float weight_threshold, float trunc_voxel_multiplier, int32_t range_map_down_factor, float* d_range,
                                     float* d_depth, float* d_vertex, float* d_normal, float* d_color, void* stream) {
	// the scalar and pointer checks come before the grid is read
	NNRT_CHECK_ARG(vg, "null grid");
	NNRT_CHECK_ARG(h_K, "null intrinsic matrix");
	NNRT_CHECK_ARG(d_range, "null range map");
	NNRT_CHECK_ARG(count >= 0 && (count == 0 || d_block_coords), "null block coordinates");
	NNRT_CHECK_ARG(width >= 1 && height >= 1, "width and height must be at least 1");
	NNRT_CHECK_ARG(range_map_down_factor >= 1, "range_map_down_factor must be at least 1");
	NNRT_CHECK_ARG(depth_min >= 0.f && depth_min < depth_max, "depth limits must satisfy 0 <= depth_min < depth_max");
	NNRT_CHECK_ARG(depth_scale > 0.f, "depth_scale must be positive");
	NNRT_CHECK_ARG((attribute_mask & ~(NNRT_RAY_CAST_DEPTH | NNRT_RAY_CAST_VERTEX | NNRT_RAY_CAST_NORMAL | NNRT_RAY_CAST_COLOR)) == 0,
	               "unknown bits in attribute_mask");
	NNRT_CHECK_ARG(!(attribute_mask & NNRT_RAY_CAST_DEPTH) || d_depth, "depth requested with a null depth map");
	NNRT_CHECK_ARG(!(attribute_mask & NNRT_RAY_CAST_VERTEX) || d_vertex, "vertex requested with a null vertex map");
	NNRT_CHECK_ARG(!(attribute_mask & NNRT_RAY_CAST_NORMAL) || d_normal, "normal requested with a null normal map");
	NNRT_CHECK_ARG(!(attribute_mask & NNRT_RAY_CAST_COLOR) || d_color, "color requested with a null color map");
	NNRT_CHECK_ARG(!(attribute_mask & NNRT_RAY_CAST_COLOR) || vg->color_type != ST_NONE, "color requested on a grid without color storage");
	double Einv[16];
	NNRT_CHECK_ARG(inverse_extrinsics(h_E, Einv), "extrinsic matrix is singular");
	// every step advances t by at least half a voxel, so no ray needs more steps than this
	const double steps = std::ceil(2.0 * (static_cast<double>(depth_max) - static_cast<double>(depth_min)) / static_cast<double>(vg->voxel_size)) + 2.0;
	NNRT_CHECK_ARG(steps <= static_cast<double>(RC_MAX_STEPS), "the ray step bound 2 (depth_max - depth_min) / voxel_size + 2 exceeds 2^20");

	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	const GridView g = vg->view();
	RayCastArgs a{};
	a.W = width;
	a.H = height;
	a.tiles_x = (width - 1) / RC_TILE + 1;
	a.tiles_y = (height - 1) / RC_TILE + 1;
	a.f = range_map_down_factor;
	a.TW = (width - 1) / range_map_down_factor + 1;
	a.TH = (height - 1) / range_map_down_factor + 1;
	a.attr = attribute_mask;
	a.max_steps = static_cast<int>(steps);
	a.depth_scale = depth_scale;
	a.weight_threshold = weight_threshold;
	a.sdf_trunc = vg->voxel_size * trunc_voxel_multiplier;
	a.pose = make_xform(h_K, Einv);
	a.range = d_range;
	a.depth = d_depth;
	a.vertex = d_vertex;
	a.normal = d_normal;
	a.color = d_color;
	const int64_t range_tiles = static_cast<int64_t>(a.TW) * a.TH;
	k_range_init<<<grid_of(2 * range_tiles), 256, 0, s>>>(d_range, 2 * range_tiles, depth_max, depth_min);
	if (count > 0 && vg->active > 0)
		k_range_blocks<<<grid_of(count * 64, RC_BLOCK), RC_BLOCK, 0, s>>>(g, d_block_coords, count, make_xform(h_K, h_E), a.f, a.TW, a.TH, depth_min,
		                                                                  depth_max, reinterpret_cast<unsigned*>(d_range));
	const int64_t waves = static_cast<int64_t>(a.tiles_x) * a.tiles_y;
	k_ray_cast<<<grid_of(waves * 64, RC_BLOCK), RC_BLOCK, 0, s>>>(g, a);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // extern "C"
