// Integration into the voxel block grid (tsdf_grid.hpp, DESIGN.md sections 12 and 29): the rigid pass, the non-rigid pass
// with its anchor search and blend, and the block queries around it -- warped block boxes, depth segments and the surface
// mask, the inactive neighbour blocks inside the truncation region.
#include <cfloat>
#include <cmath>
#include <vector>

#include "anchor_dispatch.hpp"
#include "tsdf_grid.hpp"

namespace nnrt {
namespace {

// Open3D ArrayIndexer::InBoundary for float pixel coordinates of an H x W image
__device__ inline bool in_image(float u, float v, int H, int W) {
	return u >= 0.f && v >= 0.f && u <= static_cast<float>(W) - 1.0f && v <= static_cast<float>(H) - 1.0f;
}
__device__ inline float read_color(const ImageView& im, int u, int v, int c) {
	const int64_t i = (static_cast<int64_t>(v) * im.Wc + u) * 3 + c;
	return im.depth_type == ST_U16 ? static_cast<float>(static_cast<const uint8_t*>(im.color)[i]) : static_cast<const float*>(im.color)[i];
}
// buffer index of each coordinate (-1: inactive)
__global__ void k_find_blocks(HashView h, const int32_t* __restrict__ coords, int64_t n, int* __restrict__ out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	out[i] = find_block(h, coords[3 * i], coords[3 * i + 1], coords[3 * i + 2]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Open3D Integrate (VoxelBlockGrid.cpp:317-350 -> voxel_grid::Integrate): one lane per voxel of the listed blocks.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_integrate_rigid(GridView g, const int* __restrict__ blocks, int64_t nb, ImageView im, Xform depth_x, Xform color_x,
                                  float sdf_trunc, float color_multiplier) {
	const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (w >= nb * g.res3) return;
	const int b = blocks[w / g.res3];
	if (b < 0) return;
	const int vi = static_cast<int>(w % g.res3);
	int xv, yv, zv;
	voxel_local(vi, g.res, xv, yv, zv);
	const float x = static_cast<float>(g.keys[3 * b] * g.res + xv) * g.voxel_size;
	const float y = static_cast<float>(g.keys[3 * b + 1] * g.res + yv) * g.voxel_size;
	const float z = static_cast<float>(g.keys[3 * b + 2] * g.res + zv) * g.voxel_size;
	float xc, yc, zc, u, v;
	depth_x.rigid(x, y, z, xc, yc, zc);
	depth_x.project(xc, yc, zc, u, v);
	if (!in_image(u, v, im.H, im.W)) return;
	int ui = static_cast<int>(roundf(u)), vi2 = static_cast<int>(roundf(v));
	const float depth = read_depth(im, ui, vi2) / im.depth_scale;
	float sdf = depth - zc;
	if (depth <= 0.0f || depth > im.depth_max || zc <= 0.0f || sdf < -sdf_trunc) return;
	sdf = sdf < sdf_trunc ? sdf : sdf_trunc;
	sdf /= sdf_trunc;
	const int64_t lin = static_cast<int64_t>(b) * g.res3 + vi;
	const float weight = read_store(g.weight, g.weight_type, lin);
	const float inv_wsum = 1.0f / (weight + 1);
	g.tsdf[lin] = (weight * g.tsdf[lin] + sdf) * inv_wsum;
	if (g.color && im.color) {
		float xu, yu, zu, uc, vc;
		depth_x.unproject(static_cast<float>(ui), static_cast<float>(vi2), 1.0f, xu, yu, zu);
		color_x.project(xu, yu, zu, uc, vc);
		if (in_image(uc, vc, im.Hc, im.Wc)) {
			ui = static_cast<int>(roundf(uc));
			vi2 = static_cast<int>(roundf(vc));
			for (int c = 0; c < 3; c++) {
				const float old = read_store(g.color, g.color_type, 3 * lin + c);
				write_store(g.color, g.color_type, 3 * lin + c, (weight * old + read_color(im, ui, vi2, c) * color_multiplier) * inv_wsum);
			}
		}
	}
	write_store(g.weight, g.weight_type, lin, weight + 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// Anchors of a point with the node-distance threshold (WarpUtilities.h:131-153, :319-341; KnnUtilities.h:146-220): the
// K nearest nodes by Euclidean norm with replace-the-current-maximum insertion, squared norms above 4 c^2 dropped (-1),
// Gaussian weights exp(-d^2 / 2c^2) normalized over the valid ones. Only nodes within 2 c (the largest coverage for
// variable coverage) can be valid, so the search runs over those candidates in ascending node order; the valid set
// equals the reference KD-tree's (its slot order, and thus the blend's float summation order, may differ).
// Nodes farther than that range never enter the search (per voxel), so the slot order is a function of the in-range
// nodes alone. Returns the valid count; weights are normalized only when valid >= minimum (the reference returns false otherwise
// and, where the return value is ignored, blends the unnormalized weights).
// ---------------------------------------------------------------------------------------------------------------------
template <int KT>
struct Anchors {
	int idx[KT];
	float w[KT];
	int valid;
	bool ok;
	__device__ void reset() {
#pragma unroll
		for (int k = 0; k < KT; k++) {
			idx[k] = -1;
			w[k] = INFINITY;
		}
	}
};

// replace-the-maximum insertion with static register indices (the slot to overwrite is selected, not indexed)
template <int KT>
__device__ inline void knn_insert(Anchors<KT>& a, float d, int node, float& maxd, int& max_at) {
	if (maxd > d) {
#pragma unroll
		for (int k = 0; k < KT; k++)
			if (k == max_at) {
				a.w[k] = d;   // distances held in the weight slots (WarpUtilities.h:325)
				a.idx[k] = node;
			}
		max_at = 0;
		maxd = a.w[0];
#pragma unroll
		for (int k = 1; k < KT; k++)
			if (a.w[k] > maxd) {
				max_at = k;
				maxd = a.w[k];
			}
	}
}
template <int KT>
__device__ inline void anchors_finish(Anchors<KT>& a, const WarpFieldView& wf) {
	const float c2_fixed = wf.coverage * wf.coverage;
	float sum = 0.f;
	a.valid = 0;
#pragma unroll
	for (int k = 0; k < KT; k++) {
		if (a.idx[k] < 0) continue;
		float sq = a.w[k];
		sq = sq * sq;
		const float c2 = wf.fixed_coverage ? c2_fixed : wf.node_weights[a.idx[k]];
		if (sq > 4 * c2) {
			a.idx[k] = -1;
			continue;
		}
		const float wt = exp_cr(-sq / (2 * c2));
		sum += wt;
		a.w[k] = wt;
		a.valid++;
	}
	a.ok = a.valid >= wf.minimum_valid;
	if (a.ok) {   // NormalizeAnchorWeights (WarpUtilities.h:36-46)
		if (sum > 0.0f) {
#pragma unroll
			for (int k = 0; k < KT; k++) a.w[k] /= sum;
		} else if (a.valid > 0) {
#pragma unroll
			for (int k = 0; k < KT; k++) a.w[k] = 1.0f / static_cast<float>(a.valid);
		}
	}
}
// BlendWarp (WarpUtilities.h:429-445): sum_k w_k (g_k + R_k (p - g_k) + t_k) over valid anchors
template <int KT>
__device__ inline void blend_warp(const Anchors<KT>& a, const WarpFieldView& wf, float px, float py, float pz, float& ox, float& oy, float& oz) {
	ox = oy = oz = 0.f;
#pragma unroll
	for (int k = 0; k < KT; k++) {
		const int n = a.idx[k];
		if (n < 0) continue;
		const float* s = wf.state + static_cast<int64_t>(n) * NODE_STRIDE;
		const float gx = s[0], gy = s[1], gz = s[2];
		const float dx = px - gx, dy = py - gy, dz = pz - gz;
		const float rx = (s[6] * dx + s[7] * dy) + s[8] * dz;
		const float ry = (s[9] * dx + s[10] * dy) + s[11] * dz;
		const float rz = (s[12] * dx + s[13] * dy) + s[14] * dz;
		const float w = a.w[k];
		ox += w * ((gx + rx) + s[3]);
		oy += w * ((gy + ry) + s[4]);
		oz += w * ((gz + rz) + s[5]);
	}
}
__device__ inline float node_dist(const float* s, float px, float py, float pz) {
	const float dx = s[0] - px, dy = s[1] - py, dz = s[2] - pz;
	return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// ---------------------------------------------------------------------------------------------------------------------
// IntegrateNonRigid (NonRigidSurfaceVoxelBlockGridImpl.h:52-229): one workgroup per active block. The block's nodes
// within anchor range (2 c of its camera-space bounding box) are compacted into LDS in ascending node order; each
// voxel searches only those. Reproduced as written: the weight is read but never incremented, oblique views
// (cos(view, normal) > 0.5) and psdf <= -trunc are skipped, the cosine map is written before those tests.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int NR_BLOCK = 256;
constexpr int NR_CAND = 2048;
template <int KT>
__global__ __launch_bounds__(NR_BLOCK) void k_integrate_non_rigid(GridView g, int64_t nb, WarpFieldView wf, ImageView im, const float* __restrict__ normals,
                                                                  Xform depth_x, Xform color_x, float sdf_trunc, float color_multiplier,
                                                                  float range, uint64_t* __restrict__ cos_key, int grow_surface) {
	__shared__ int s_cand[NR_CAND];
	__shared__ int s_count;
	__shared__ int s_wave_counts[NR_BLOCK / 64];
	const int b = blockIdx.x;
	if (b >= nb) return;
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	// camera-space bounding box of the block (its 8 corners, as voxel centres span [0, res - 1])
	float bmin[3] = {INFINITY, INFINITY, INFINITY}, bmax[3] = {-INFINITY, -INFINITY, -INFINITY};
	for (int c = 0; c < 8; c++) {
		const float x = static_cast<float>(g.keys[3 * b] * g.res + ((c & 1) ? g.res - 1 : 0)) * g.voxel_size;
		const float y = static_cast<float>(g.keys[3 * b + 1] * g.res + ((c & 2) ? g.res - 1 : 0)) * g.voxel_size;
		const float z = static_cast<float>(g.keys[3 * b + 2] * g.res + ((c & 4) ? g.res - 1 : 0)) * g.voxel_size;
		float o[3];
		depth_x.rigid(x, y, z, o[0], o[1], o[2]);
		for (int k = 0; k < 3; k++) {
			bmin[k] = fminf(bmin[k], o[k]);
			bmax[k] = fmaxf(bmax[k], o[k]);
		}
	}
	if (t == 0) s_count = 0;
	__syncthreads();
	bool overflow = false;
	for (int base = 0; base < wf.N; base += NR_BLOCK) {   // ordered compaction of the candidates
		const int n = base + t;
		bool near = false;
		if (n < wf.N) {
			const float* s = wf.state + static_cast<int64_t>(n) * NODE_STRIDE;
			float d2 = 0.f;
			for (int k = 0; k < 3; k++) {
				const float e = fmaxf(fmaxf(bmin[k] - s[k], s[k] - bmax[k]), 0.f);
				d2 += e * e;
			}
			near = d2 <= range * range * 1.0001f + 1e-12f;
		}
		const uint64_t m = __ballot(near);
		if (lane == 0) s_wave_counts[wave] = __popcll(m);
		__syncthreads();
		int before = s_count;
		for (int w = 0; w < wave; w++) before += s_wave_counts[w];
		const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
		if (near && pos < NR_CAND) s_cand[pos] = n;
		__syncthreads();
		if (t == 0) {
			int tot = s_count;
			for (int w = 0; w < NR_BLOCK / 64; w++) tot += s_wave_counts[w];
			s_count = tot;
		}
		__syncthreads();
	}
	const int ncand = s_count;
	overflow = ncand > NR_CAND;
	for (int vi = t; vi < g.res3; vi += NR_BLOCK) {
		int xv, yv, zv;
		voxel_local(vi, g.res, xv, yv, zv);
		const float x = static_cast<float>(g.keys[3 * b] * g.res + xv) * g.voxel_size;
		const float y = static_cast<float>(g.keys[3 * b + 1] * g.res + yv) * g.voxel_size;
		const float z = static_cast<float>(g.keys[3 * b + 2] * g.res + zv) * g.voxel_size;
		float xc, yc, zc;
		depth_x.rigid(x, y, z, xc, yc, zc);
		Anchors<KT> a;
		a.reset();
		float maxd = INFINITY;
		int max_at = 0;
		if (!overflow) {
			for (int q = 0; q < ncand; q++) {
				const int n = s_cand[q];
				const float d = node_dist(wf.state + static_cast<int64_t>(n) * NODE_STRIDE, xc, yc, zc);
				if (d <= range) knn_insert<KT>(a, d, n, maxd, max_at);
			}
		} else {
			for (int n = 0; n < wf.N; n++) {
				const float d = node_dist(wf.state + static_cast<int64_t>(n) * NODE_STRIDE, xc, yc, zc);
				if (d <= range) knn_insert<KT>(a, d, n, maxd, max_at);
			}
		}
		anchors_finish<KT>(a, wf);
		if (!a.ok) continue;
		float wx, wy, wz;
		blend_warp<KT>(a, wf, xc, yc, zc, wx, wy, wz);
		if (wz < 0) continue;
		float u, v;
		depth_x.project(wx, wy, wz, u, v);
		if (!in_image(u, v, im.H, im.W)) continue;
		int ui = static_cast<int>(roundf(u)), vr = static_cast<int>(roundf(v));
		const float depth = read_depth(im, ui, vr) / im.depth_scale;
		if (depth <= 0.0f || depth > im.depth_max) continue;
		const float psdf = depth - wz;
		float vx = -wx, vy = -wy, vz = -wz;   // view direction, Eigen normalize()
		const float vn2 = (vx * vx + vy * vy) + vz * vz;
		if (vn2 > 0.f) {
			const float vn = sqrtf(vn2);
			vx /= vn;
			vy /= vn;
			vz /= vn;
		}
		const int64_t pix = static_cast<int64_t>(vr) * im.W + ui;
		const float cosine = (vx * normals[3 * pix] + vy * normals[3 * pix + 1]) + vz * normals[3 * pix + 2];
		const int64_t lin = static_cast<int64_t>(b) * g.res3 + vi;
		// the reference's plain store races between voxels that project to one pixel; here the voxel with the highest
		// linear index wins (the serial loop's last writer)
		atomicMax(reinterpret_cast<unsigned long long*>(cos_key + pix),
		          (static_cast<unsigned long long>(lin + 1) << 32) | __builtin_bit_cast(uint32_t, cosine));
		// the reference skips cosine > 0.5, which with camera-facing normals is every surface seen head-on (T1);
		// grow_surface keeps those and skips the grazing ones (and pixels without a normal: cosine 0) instead
		if (psdf <= -sdf_trunc || (grow_surface ? !(cosine >= 0.5f) : cosine > 0.5f)) continue;
		const float tsdf_n = (psdf < sdf_trunc ? psdf : sdf_trunc) / sdf_trunc;
		const float weight = read_store(g.weight, g.weight_type, lin);
		const float inv_wsum = 1.0f / (weight + 1);
		g.tsdf[lin] = (weight * g.tsdf[lin] + tsdf_n) * inv_wsum;
		if (g.color && im.color) {
			float xu, yu, zu, uc, vc;
			depth_x.unproject(static_cast<float>(ui), static_cast<float>(vr), 1.0f, xu, yu, zu);
			color_x.project(xu, yu, zu, uc, vc);
			if (in_image(uc, vc, im.Hc, im.Wc)) {
				ui = static_cast<int>(roundf(uc));
				vr = static_cast<int>(roundf(vc));
				for (int c = 0; c < 3; c++) {
					const float old = read_store(g.color, g.color_type, 3 * lin + c);
					write_store(g.color, g.color_type, 3 * lin + c, (weight * old + read_color(im, ui, vr, c) * color_multiplier) * inv_wsum);
				}
			}
		}
		// the reference never counts the observation (T2), so a voxel first seen here keeps weight 0 and never reaches
		// the extracted mesh; grow_surface counts it as k_integrate_rigid does
		if (grow_surface) write_store(g.weight, g.weight_type, lin, weight + 1);
	}
}

__global__ void k_cos_resolve(const uint64_t* __restrict__ key, int64_t n, float* __restrict__ cos_out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = key[i];
	cos_out[i] = k ? __builtin_bit_cast(float, static_cast<uint32_t>(k & 0xffffffffu)) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// GetBoundingBoxesOfWarpedBlocks (NonRigidSurfaceVoxelBlockGridImpl.h:289-356), reproduced as written: the block corner
// is the integer block key itself plus the block side length (metric only when the side is 1), the anchors' return
// value is ignored, and the min / max updates are an if / else-if pair.
// ---------------------------------------------------------------------------------------------------------------------
// One lane per (block, corner): 8 consecutive lanes hold one block's corners (the corner order of the reference's
// block_corners array); node positions are staged in LDS and only nodes within 2 c of the corner enter the K-NN
// (nodes farther away are never valid anchors; the oracle applies the same rule). Lane 0 of each octet then folds the
// 8 warped corners in order with the reference's if / else-if min-max.
constexpr int BOX_BLOCK = 256;
constexpr int BOX_LDS_NODES = 4096;
template <int KT>
__global__ __launch_bounds__(BOX_BLOCK) void k_warped_block_boxes(const int32_t* __restrict__ keys, int64_t n, float side, WarpFieldView wf,
                                                                  Xform ex, float range, float* __restrict__ boxes) {
	__shared__ float s_nodes[BOX_LDS_NODES * 3];
	const bool staged = wf.N <= BOX_LDS_NODES;
	if (staged)
		for (int i = threadIdx.x; i < wf.N; i += BOX_BLOCK)
			for (int k = 0; k < 3; k++) s_nodes[3 * i + k] = wf.state[static_cast<int64_t>(i) * NODE_STRIDE + k];
	__syncthreads();
	const int64_t gid = static_cast<int64_t>(blockIdx.x) * BOX_BLOCK + threadIdx.x;
	const int64_t i = gid >> 3;
	const int c = static_cast<int>(gid & 7);
	float w[3] = {0.f, 0.f, 0.f};
	if (i < n) {
		const float x0 = static_cast<float>(keys[3 * i]), y0 = static_cast<float>(keys[3 * i + 1]), z0 = static_cast<float>(keys[3 * i + 2]);
		const float x1 = x0 + side, y1 = y0 + side, z1 = z0 + side;
		// block_corners order (:322-331): 000, 001, 010, 100, 011, 101, 110, 111 (bit pattern x y z)
		const int pat[8] = {0, 1, 2, 4, 3, 5, 6, 7};
		const int m = pat[c];
		float p[3];
		ex.rigid((m & 4) ? x1 : x0, (m & 2) ? y1 : y0, (m & 1) ? z1 : z0, p[0], p[1], p[2]);
		Anchors<KT> a;
		a.reset();
		float maxd = INFINITY;
		int max_at = 0;
		for (int nn = 0; nn < wf.N; nn++) {
			const float* q = staged ? s_nodes + 3 * nn : wf.state + static_cast<int64_t>(nn) * NODE_STRIDE;
			const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
			const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
			if (d <= range) knn_insert<KT>(a, d, nn, maxd, max_at);
		}
		WarpFieldView fixed = wf;
		fixed.fixed_coverage = 1;   // ComputeAnchorsForPoint<.., true, true>: fixed node coverage
		anchors_finish<KT>(a, fixed);
		blend_warp<KT>(a, wf, p[0], p[1], p[2], w[0], w[1], w[2]);
	}
	float all[8][3];
#pragma unroll
	for (int q = 0; q < 8; q++)
#pragma unroll
		for (int k = 0; k < 3; k++) all[q][k] = __shfl(w[k], (threadIdx.x & ~7) + q);
	if (i < n && c == 0) {
		float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
		for (int q = 0; q < 8; q++)
			for (int k = 0; k < 3; k++) {
				if (mn[k] > all[q][k]) mn[k] = all[q][k];
				else if (mx[k] < all[q][k]) mx[k] = all[q][k];
			}
		for (int k = 0; k < 3; k++) {
			boxes[6 * i + k] = mn[k];
			boxes[6 * i + 3 + k] = mx[k];
		}
	}
}

// GetAxisAlignedBoxesInterceptingSurfaceMask (:359-437): a segment [d - trunc, d + trunc] along the ray of every
// stride-th pixel, slab test (Segment.h IntersectsAxisAlignedBox) against every box. Segments at fixed positions
// (invalid pixels: none), one lane per box walking them.
struct Seg {
	float o[3], inv[3];
	int sign[3];
	int valid;
};
__global__ void k_make_segments(ImageView im, int stride, Xform K, float trunc, Seg* __restrict__ segs) {
	const int rows = im.H / stride, cols = im.W / stride;
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= static_cast<int64_t>(rows) * cols) return;
	const int v = static_cast<int>(i / cols) * stride, u = static_cast<int>(i % cols) * stride;
	const float d = read_depth(im, u, v) / im.depth_scale;
	Seg s{};
	s.valid = d > 0 && d < im.depth_max;
	if (s.valid) {
		float a[3], e[3];
		K.unproject(static_cast<float>(u), static_cast<float>(v), d - trunc, a[0], a[1], a[2]);
		K.unproject(static_cast<float>(u), static_cast<float>(v), d + trunc, e[0], e[1], e[2]);
		for (int k = 0; k < 3; k++) {
			s.o[k] = a[k];
			s.inv[k] = 1.f / (e[k] - a[k]);
			s.sign[k] = s.inv[k] < 0;
		}
	}
	segs[i] = s;
}
__device__ inline bool seg_hits_box(const Seg& s, const float* bmin, const float* bmax) {
	const float* bounds[2] = {bmin, bmax};
	float t_min = (bounds[s.sign[0]][0] - s.o[0]) * s.inv[0];
	float t_max = (bounds[1 - s.sign[0]][0] - s.o[0]) * s.inv[0];
	const float ty_min = (bounds[s.sign[1]][1] - s.o[1]) * s.inv[1];
	const float ty_max = (bounds[1 - s.sign[1]][1] - s.o[1]) * s.inv[1];
	if ((t_min > ty_max) || (ty_min > t_max)) return false;
	if (ty_min > t_min) t_min = ty_min;
	if (ty_max < t_max) t_max = ty_max;
	const float tz_min = (bounds[s.sign[2]][2] - s.o[2]) * s.inv[2];
	const float tz_max = (bounds[1 - s.sign[2]][2] - s.o[2]) * s.inv[2];
	if ((t_min > tz_max) || (tz_min > t_max)) return false;
	if (tz_min > t_min) t_min = tz_min;
	if (tz_max < t_max) t_max = tz_max;
	return !(t_max < 0.0f || t_min > 1.0f);
}
__global__ void k_boxes_mask(const float* __restrict__ boxes, int64_t nbox, const Seg* __restrict__ segs, int64_t nseg, uint8_t* __restrict__ mask) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= nbox) return;
	const float* bmin = boxes + 6 * i;
	const float* bmax = bmin + 3;
	uint8_t hit = 0;
	for (int64_t s = 0; s < nseg && !hit; s++)
		if (segs[s].valid && seg_hits_box(segs[s], bmin, bmax)) hit = 1;
	mask[i] = hit;
}
__global__ void k_and_mask(int* __restrict__ keep, const uint8_t* __restrict__ m, int64_t n) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i < n) keep[i] = m[i] ? 1 : 0;
}

float color_multiplier(int depth_dtype) { return depth_dtype == NNRT_DTYPE_FLOAT32 ? 255.0f : 1.0f; }

} // namespace
} // namespace nnrt

using namespace nnrt;

extern "C" {

nnrt_status nnrt_voxel_grid_integrate(nnrt_voxel_grid* vg, const int32_t* d_block_coords, int64_t count, const void* d_depth, int32_t depth_dtype,
                                      int32_t height, int32_t width, const void* d_color, int32_t color_height, int32_t color_width,
                                      const double* h_depth_K, const double* h_color_K, const double* h_E, float depth_scale, float depth_max,
                                      float trunc_voxel_multiplier, void* stream) {
	NNRT_CHECK_ARG(vg && d_depth && h_depth_K && height > 0 && width > 0 && count >= 0 && (count == 0 || d_block_coords), "invalid arguments");
	NNRT_CHECK_ARG(depth_dtype == NNRT_DTYPE_UINT16 || depth_dtype == NNRT_DTYPE_FLOAT32, "depth must be uint16 or float32");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	nnrt_status st;
	if ((st = activate_coords(vg, d_block_coords, count, s))) return st;
	if (count == 0) return NNRT_OK;
	if ((st = vg->integ.blocks.ensure(count))) return st;
	const GridView g = vg->view();
	k_find_blocks<<<grid_of(count), 256, 0, s>>>(g.hash, d_block_coords, count, vg->integ.blocks.ptr);
	const ImageView im = make_image(d_depth, depth_dtype, height, width, d_color, color_height, color_width, depth_scale, depth_max);
	k_integrate_rigid<<<grid_of(count * vg->res3), 256, 0, s>>>(g, vg->integ.blocks.ptr, count, im, make_xform(h_depth_K, h_E),
	                                                           make_xform(h_color_K ? h_color_K : h_depth_K, nullptr),
	                                                           vg->voxel_size * trunc_voxel_multiplier, color_multiplier(depth_dtype));
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_set_non_rigid_surface_growth(nnrt_voxel_grid* vg, int32_t enabled) {
	NNRT_CHECK_ARG(vg, "null voxel grid");
	vg->grow_surface = enabled != 0;
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_integrate_non_rigid(nnrt_voxel_grid* vg, const int32_t* d_block_coords, int64_t count, const nnrt_warp_field* wf,
                                                const void* d_depth, int32_t depth_dtype, int32_t height, int32_t width, const void* d_color,
                                                int32_t color_height, int32_t color_width, const float* d_depth_normals, const double* h_depth_K,
                                                const double* h_color_K, const double* h_E, float depth_scale, float depth_max,
                                                float trunc_voxel_multiplier, float* d_cos_out, void* stream) {
	NNRT_CHECK_ARG(vg && wf && d_depth && d_depth_normals && h_depth_K && d_cos_out && height > 0 && width > 0 && count >= 0 &&
	                   (count == 0 || d_block_coords),
	               "invalid arguments");
	NNRT_CHECK_ARG(depth_dtype == NNRT_DTYPE_UINT16 || depth_dtype == NNRT_DTYPE_FLOAT32, "depth must be uint16 or float32");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	nnrt_status st;
	if ((st = activate_coords(vg, d_block_coords, count, s))) return st;
	const WarpFieldView wv = warp_field_view(wf);
	NNRT_CHECK_ARG(wv.anchor_count >= 1 && wv.anchor_count <= MAX_ANCHORS, "anchor_count must be in [1, 8]");
	const int64_t P = static_cast<int64_t>(height) * width;
	NNRT_HIP(hipMemsetAsync(d_cos_out, 0, sizeof(float) * P, s));   // Tensor::Zeros (:72)
	if (vg->active == 0) return NNRT_OK;
	if ((st = vg->integ.cos_key.ensure(P))) return st;
	uint64_t* const cos_key = vg->integ.cos_key.ptr;
	NNRT_HIP(hipMemsetAsync(cos_key, 0, sizeof(uint64_t) * P, s));
	float range = 2.f * wv.coverage;   // nodes farther than 2 c are never valid anchors
	if (!wv.fixed_coverage) {
		std::vector<float> w(static_cast<size_t>(wv.N));
		NNRT_HIP(hipMemcpy(w.data(), wv.node_weights, sizeof(float) * w.size(), hipMemcpyDeviceToHost));
		float mx = 0.f;
		for (float v : w) mx = std::max(mx, v);
		range = 2.f * std::sqrt(mx);
	}
	const ImageView im = make_image(d_depth, depth_dtype, height, width, d_color, color_height, color_width, depth_scale, depth_max);
	const GridView gv = vg->view();
	const Xform xd = make_xform(h_depth_K, h_E), xc = make_xform(h_color_K ? h_color_K : h_depth_K, nullptr);
	const float trunc = vg->voxel_size * trunc_voxel_multiplier, cm = color_multiplier(depth_dtype);
	if ((st = dispatch_anchor_count(wv.anchor_count, [&](auto kk) {
		     k_integrate_non_rigid<decltype(kk)::value><<<static_cast<unsigned>(vg->active), NR_BLOCK, 0, s>>>(
		         gv, vg->active, wv, im, d_depth_normals, xd, xc, trunc, cm, range, cos_key, vg->grow_surface ? 1 : 0);
		     return NNRT_OK;
	     })))
		return st;
	k_cos_resolve<<<grid_of(P), 256, 0, s>>>(cos_key, P, d_cos_out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_warped_block_boxes(const nnrt_voxel_grid* vg, const int32_t* d_block_keys, int64_t count, const nnrt_warp_field* wf,
                                               const double* h_E, float* d_boxes, void* stream) {
	NNRT_CHECK_ARG(vg && wf && (count == 0 || (d_block_keys && d_boxes)) && count >= 0, "invalid arguments");
	DeviceGuard guard(vg->device);
	const WarpFieldView wv = warp_field_view(wf);
	NNRT_CHECK_ARG(wv.anchor_count >= 1 && wv.anchor_count <= MAX_ANCHORS, "anchor_count must be in [1, 8]");
	if (count == 0) return NNRT_OK;
	const float side = static_cast<float>(vg->res) * vg->voxel_size;
	const Xform ex = make_xform(nullptr, h_E);
	hipStream_t s = static_cast<hipStream_t>(stream);
	const nnrt_status st = dispatch_anchor_count(wv.anchor_count, [&](auto kk) {
		k_warped_block_boxes<decltype(kk)::value><<<grid_of(8 * count, BOX_BLOCK), BOX_BLOCK, 0, s>>>(d_block_keys, count, side, wv, ex, 2.f * wv.coverage, d_boxes);
		return NNRT_OK;
	});
	if (st) return st;
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status nnrt_boxes_intersecting_surface_mask(const float* d_boxes, int64_t count, const void* d_depth, int32_t depth_dtype, int32_t height,
                                                 int32_t width, const double* h_K, float depth_scale, float depth_max, int32_t stride,
                                                 float truncation_distance, uint8_t* d_mask, void* stream) {
	NNRT_CHECK_ARG((count == 0 || (d_boxes && d_mask)) && d_depth && h_K && height > 0 && width > 0 && stride >= 1 && count >= 0,
	               "invalid arguments");
	NNRT_CHECK_ARG(depth_dtype == NNRT_DTYPE_UINT16 || depth_dtype == NNRT_DTYPE_FLOAT32, "depth must be uint16 or float32");
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (count == 0) return NNRT_OK;
	const int64_t nseg = static_cast<int64_t>(height / stride) * (width / stride);
	StreamScratch<Seg> segs;   // no grid here to keep it on: stream-ordered
	nnrt_status st = segs.alloc(static_cast<size_t>(std::max<int64_t>(nseg, 1)), s);
	if (st) return st;
	const ImageView im = make_image(d_depth, depth_dtype, height, width, nullptr, 0, 0, depth_scale, depth_max);
	if (nseg > 0) k_make_segments<<<grid_of(nseg), 256, 0, s>>>(im, stride, make_xform(h_K, nullptr), truncation_distance, segs.ptr);
	k_boxes_mask<<<grid_of(count), 256, 0, s>>>(d_boxes, count, segs.ptr, nseg, d_mask);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_find_blocks_intersecting_truncation_region(nnrt_voxel_grid* vg, const void* d_depth, int32_t depth_dtype, int32_t height,
                                                                       int32_t width, const nnrt_warp_field* wf, const double* h_K, const double* h_E,
                                                                       float depth_scale, float depth_max, float trunc_voxel_multiplier,
                                                                       int64_t* h_count, void* stream) {
	NNRT_CHECK_ARG(vg && wf && d_depth && h_K && h_count, "invalid arguments");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	auto& q = vg->query;
	nnrt_status st;
	if ((st = inactive_neighbor_coords(vg, s))) return st;
	const int64_t m = vg->coords.count;
	*h_count = 0;
	if (m == 0) return NNRT_OK;
	if ((st = q.boxes.ensure(6 * static_cast<size_t>(m))) || (st = q.mask.ensure(m))) return st;
	// the candidates go back to query.coords [m, 3] (it held all 27 active neighbours, so it has the room)
	NNRT_HIP(hipMemcpyAsync(q.coords.ptr, vg->coords.rows.ptr, sizeof(int32_t) * 3 * m, hipMemcpyDeviceToDevice, s));
	if ((st = nnrt_voxel_grid_warped_block_boxes(vg, q.coords.ptr, m, wf, h_E, q.boxes.ptr, stream))) return st;
	// NonRigidSurfaceVoxelBlockGrid.cpp:163-166: stride 4, truncation = voxel_size * trunc_voxel_multiplier (default 8)
	if ((st = nnrt_boxes_intersecting_surface_mask(q.boxes.ptr, m, d_depth, depth_dtype, height, width, h_K, depth_scale, depth_max, 4,
	                                               vg->voxel_size * trunc_voxel_multiplier, q.mask.ptr, stream)))
		return st;
	k_and_mask<<<grid_of(m), 256, 0, s>>>(q.keep.ptr, q.mask.ptr, m);
	NNRT_LAUNCH_CHECK();
	if ((st = compact_kept_coords(vg, m, s))) return st;
	*h_count = vg->coords.count;
	return NNRT_OK;
}

} // extern "C"
