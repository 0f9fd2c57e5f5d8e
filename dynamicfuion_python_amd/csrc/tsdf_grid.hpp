// TSDF voxel block grid on gfx950: the canonical-mesh source and sink either side of the fitter in a DynamicFusion loop
// (SURVEY.md 8(f) row 2). Reference: nnrt.geometry.NonRigidSurfaceVoxelBlockGrid (cpp/geometry/NonRigidSurfaceVoxelBlockGrid.cpp,
// cpp/geometry/kernel/NonRigidSurfaceVoxelBlockGridImpl.h) over NNRT's VoxelBlockGrid (cpp/geometry/VoxelBlockGrid.cpp), whose
// hash map, depth touch, rigid integration and mesh extraction are Open3D 0.17 kernels (third-party, not in the
// reference tree; restated from Open3D's published t::geometry::kernel::voxel_grid algorithms).
//
// This header is what the grid's four sources share: keys and the hash table, the views kernels
// take, the handle and its owners. tsdf_grid.hip holds the table, growth and activation; tsdf_integrate.hip the rigid
// and non-rigid integration and the block queries around it; tsdf_extract.hip voxel values and marching cubes;
// tsdf_ray_cast.hip the ray cast. The library is not built as relocatable device code, so device helpers here are inline.
//
// Layout in HBM (one grid):
//   block keys   int32 [capacity, 3]; buffer index = activation order (dense: blocks are never erased)
//   hash table   open addressing, linear probing: uint64 packed key [T] + int32 buffer index [T], T = pow2 >= 2 capacity
//   voxels       tsdf f32 [capacity, res^3], weight (f32 | u16) [capacity, res^3], color (f32 | u16 | u8) [capacity, res^3, 3];
//                voxel (x, y, z) of a block at x + res (y + res z) (Open3D ArrayIndexer order)
// Activation is deterministic: every key takes the lowest input index that carries it (atomicMin), new keys get buffer
// indices by a prefix sum in input order -- so block order, and everything derived from it, is reproducible.
#pragma once
#include <algorithm>

#include "device_primitives.hpp"
#include "hash_table_size.hpp"
#include "kernels.hpp"

namespace nnrt {

constexpr uint64_t HASH_EMPTY = ~0ull;
constexpr int KEY_BIAS = 1 << 20;   // block coordinates in [-2^20, 2^20)

enum StoreType : int { ST_NONE = 0, ST_F32 = 1, ST_U16 = 2, ST_U8 = 3 };

__host__ __device__ inline bool key_in_range(int x, int y, int z) {
	return x >= -KEY_BIAS && x < KEY_BIAS && y >= -KEY_BIAS && y < KEY_BIAS && z >= -KEY_BIAS && z < KEY_BIAS;
}
__host__ __device__ inline uint64_t pack_key(int x, int y, int z) {
	return static_cast<uint64_t>(static_cast<uint32_t>(x + KEY_BIAS)) | (static_cast<uint64_t>(static_cast<uint32_t>(y + KEY_BIAS)) << 21) |
	       (static_cast<uint64_t>(static_cast<uint32_t>(z + KEY_BIAS)) << 42);
}
__device__ inline uint64_t hash_mix(uint64_t k) {
	k ^= k >> 33;
	k *= 0xff51afd7ed558ccdull;
	k ^= k >> 33;
	k *= 0xc4ceb9fe1a85ec53ull;
	k ^= k >> 33;
	return k;
}

struct HashView {
	uint64_t* keys;
	int* block;     // buffer index per slot (-1: none yet)
	int* first;     // scratch: lowest input index per slot during one activation / dedupe
	uint64_t mask;
};

// the slot holding `key`, inserting it if absent (never fails: the table is kept at most half full)
__device__ inline uint64_t hash_insert(const HashView& h, uint64_t key) {
	uint64_t s = hash_mix(key) & h.mask;
	while (true) {
		const uint64_t prev = atomicCAS(reinterpret_cast<unsigned long long*>(h.keys + s), HASH_EMPTY, key);
		if (prev == HASH_EMPTY || prev == key) return s;
		s = (s + 1) & h.mask;
	}
}
__device__ inline int hash_find(const HashView& h, uint64_t key) {
	uint64_t s = hash_mix(key) & h.mask;
	while (true) {
		const uint64_t k = h.keys[s];
		if (k == key) return h.block[s];
		if (k == HASH_EMPTY) return -1;
		s = (s + 1) & h.mask;
	}
}
__device__ inline int find_block(const HashView& h, int x, int y, int z) {
	return key_in_range(x, y, z) ? hash_find(h, pack_key(x, y, z)) : -1;
}

// Open3D TransformIndexer (float rows of the 3x4 extrinsic, float intrinsics)
struct Xform {
	float m[12];
	float fx, fy, cx, cy;
	__device__ __host__ void rigid(float x, float y, float z, float& ox, float& oy, float& oz) const {
		ox = ((x * m[0] + y * m[1]) + z * m[2]) + m[3];
		oy = ((x * m[4] + y * m[5]) + z * m[6]) + m[7];
		oz = ((x * m[8] + y * m[9]) + z * m[10]) + m[11];
	}
	__device__ __host__ void project(float x, float y, float z, float& u, float& v) const {
		const float inv_z = 1.0f / z;
		u = (fx * x) * inv_z + cx;
		v = (fy * y) * inv_z + cy;
	}
	__device__ __host__ void unproject(float u, float v, float d, float& x, float& y, float& z) const {
		x = ((u - cx) * d) / fx;
		y = ((v - cy) * d) / fy;
		z = d;
	}
};
inline Xform make_xform(const double* K, const double* E) {
	Xform t{};
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 4; c++) t.m[4 * r + c] = E ? static_cast<float>(E[4 * r + c]) : (r == c ? 1.f : 0.f);
	if (K) {
		t.fx = static_cast<float>(K[0]);
		t.fy = static_cast<float>(K[4]);
		t.cx = static_cast<float>(K[2]);
		t.cy = static_cast<float>(K[5]);
	} else {
		t.fx = t.fy = 1.f;
		t.cx = t.cy = 0.f;
	}
	return t;
}
// out = inverse of the 4x4 extrinsic h_E (identity when null), in double on the host as Open3D inverts it; false: singular
bool inverse_extrinsics(const double* h_E, double* out);

// storage element read / write by runtime store type
__device__ inline float read_store(const void* base, int type, int64_t i) {
	switch (type) {
		case ST_F32: return static_cast<const float*>(base)[i];
		case ST_U16: return static_cast<float>(static_cast<const uint16_t*>(base)[i]);
		case ST_U8: return static_cast<float>(static_cast<const uint8_t*>(base)[i]);
		default: return 0.f;
	}
}
// C++ float -> integer conversion truncates toward zero (as the reference's typed stores)
__device__ inline void write_store(void* base, int type, int64_t i, float v) {
	switch (type) {
		case ST_F32: static_cast<float*>(base)[i] = v; break;
		case ST_U16: static_cast<uint16_t*>(base)[i] = static_cast<uint16_t>(static_cast<uint32_t>(v)); break;
		case ST_U8: static_cast<uint8_t*>(base)[i] = static_cast<uint8_t>(static_cast<uint32_t>(v)); break;
		default: break;
	}
}
inline size_t store_bytes(int type) { return type == ST_F32 ? 4 : type == ST_U16 ? 2 : type == ST_U8 ? 1 : 0; }

struct GridView {
	float voxel_size;
	int res, res3;
	const int32_t* keys;   // [cap,3]
	float* tsdf;
	void* weight;
	int weight_type;
	void* color;
	int color_type;
	HashView hash;
};

struct ImageView {
	const void* depth;
	int depth_type;   // ST_F32 | ST_U16
	int H, W;
	const void* color;   // [Hc, Wc, 3]: f32 when depth is f32, else u8 (Open3D input_color_t)
	int Hc, Wc;
	float depth_scale, depth_max;
};
inline ImageView make_image(const void* depth, int depth_dtype, int H, int W, const void* color, int Hc, int Wc, float scale, float dmax) {
	ImageView im{};
	im.depth = depth;
	im.depth_type = depth_dtype == NNRT_DTYPE_UINT16 ? ST_U16 : ST_F32;
	im.H = H;
	im.W = W;
	im.color = color;
	im.Hc = Hc;
	im.Wc = Wc;
	im.depth_scale = scale;
	im.depth_max = dmax;
	return im;
}

__device__ inline float read_depth(const ImageView& im, int u, int v) {
	const int64_t i = static_cast<int64_t>(v) * im.W + u;
	return im.depth_type == ST_U16 ? static_cast<float>(static_cast<const uint16_t*>(im.depth)[i]) : static_cast<const float*>(im.depth)[i];
}

__device__ inline void voxel_local(int idx, int res, int& x, int& y, int& z) {
	x = idx % res;
	y = (idx / res) % res;
	z = idx / (res * res);
}

inline unsigned grid_of(int64_t n, int block = 256) { return static_cast<unsigned>((n + block - 1) / block); }

// dst row rank[i] = src row i, for the rows with flags[i] != 0 (rank: the exclusive scan of the flags)
template <typename T>
__global__ void k_compact_rows(const T* __restrict__ src, const int* __restrict__ flags, const int* __restrict__ rank, int64_t n, int width,
                               T* __restrict__ dst) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n || !flags[i]) return;
	for (int c = 0; c < width; c++) dst[rank[i] * width + c] = src[i * width + c];
}

// ---------------------------------------------------------------------------------------------------------------------
// The owners on the handle.
// ---------------------------------------------------------------------------------------------------------------------
// A hash table's three arrays and its size: the grid's own (key -> block) and the scratch one that dedupes a frame's
// touched keys. Tables only grow, and a reset one is empty: no key, no block, `first` at its ceiling.
struct HashTable {
	DeviceBuffer<uint64_t> keys;
	DeviceBuffer<int> block, first;
	uint64_t size = 0;

	static uint64_t size_for(int64_t entries) { return hash_table_size_for(entries); }
	nnrt_status reset(uint64_t new_size, hipStream_t s);   // room for new_size slots, all three arrays refilled
	nnrt_status clear_first(hipStream_t s);                // before each activation over a table that keeps its keys
	HashView view() const { return HashView{keys.ptr, block.ptr, first.ptr, size - 1}; }
};

// rows [count, width] awaiting a copy-out
template <typename T>
struct ResultRows {
	DeviceBuffer<T> rows;
	int64_t count = 0;
	int width = 0;
	nnrt_status copy_out(T* d_out, hipStream_t s) const {
		if (count) NNRT_HIP(hipMemcpyAsync(d_out, rows.ptr, sizeof(T) * count * width, hipMemcpyDeviceToDevice, s));
		return NNRT_OK;
	}
};
using CoordResult = ResultRows<int32_t>;   // block coordinates, width 3
using RowResult = ResultRows<float>;       // voxel rows, width 5 or 8

struct MeshResult {
	DeviceBuffer<float> vpos, vnrm, vcol;
	DeviceBuffer<int64_t> tris;
	int64_t nv = 0, nt = 0;
	// null outputs are skipped
	nnrt_status copy_out(float* d_vertices, float* d_normals, float* d_colors, int64_t* d_triangles, hipStream_t s) const {
		const size_t v = sizeof(float) * 3 * static_cast<size_t>(nv), t = sizeof(int64_t) * 3 * static_cast<size_t>(nt);
		if (v && d_vertices) NNRT_HIP(hipMemcpyAsync(d_vertices, vpos.ptr, v, hipMemcpyDeviceToDevice, s));
		if (v && d_normals) NNRT_HIP(hipMemcpyAsync(d_normals, vnrm.ptr, v, hipMemcpyDeviceToDevice, s));
		if (v && d_colors) NNRT_HIP(hipMemcpyAsync(d_colors, vcol.ptr, v, hipMemcpyDeviceToDevice, s));
		if (t && d_triangles) NNRT_HIP(hipMemcpyAsync(d_triangles, tris.ptr, t, hipMemcpyDeviceToDevice, s));
		return NNRT_OK;
	}
};

} // namespace nnrt

// Every buffer below grows on demand and is kept: nothing under the grid allocates per call except growth.
struct nnrt_voxel_grid {
	int device = 0;
	float voxel_size = 0.f;
	int res = 8, res3 = 512;
	int64_t capacity = 0, active = 0;
	int weight_type = nnrt::ST_F32, color_type = nnrt::ST_NONE;
	bool grow_surface = false;   // nnrt_voxel_grid_set_non_rigid_surface_growth
	// block storage
	nnrt::DeviceBuffer<float> tsdf;
	nnrt::DeviceBuffer<uint8_t> weight, color;
	nnrt::DeviceBuffer<int32_t> keys;
	nnrt::HashTable table;    // block key -> buffer index
	nnrt::HashTable dedupe;   // unique_packed's: the keys one depth frame touches
	struct {   // compact(): the flags' ranks and the scan's temporary (marching cubes scans with the latter too)
		nnrt::DeviceBuffer<int> rank;
		nnrt::Scratch scan;
	} compaction;
	struct {   // activation and the dedupe of touched keys (tsdf_grid.hip)
		nnrt::DeviceBuffer<uint64_t> touched, slot;   // a frame's packed keys; the table slot of every input
		nnrt::DeviceBuffer<int> flag;                 // input i creates a block / is a key's first carrier
		nnrt::DeviceBuffer<int> error;                // one word: an input's coordinate is out of range
	} act;
	struct {   // integration (tsdf_integrate.hip)
		nnrt::DeviceBuffer<int> blocks;          // buffer index of every listed block
		nnrt::DeviceBuffer<uint64_t> cos_key;    // per pixel: (writer voxel + 1, cosine bits)
	} integ;
	struct {   // block and voxel queries: inactive neighbours, blocks in the truncation region, values at coordinates
		nnrt::DeviceBuffer<int32_t> coords;
		nnrt::DeviceBuffer<int> keep;
		nnrt::DeviceBuffer<float> boxes, rows;
		nnrt::DeviceBuffer<uint8_t> mask;
	} query;
	struct {   // marching cubes (tsdf_extract.hip)
		nnrt::DeviceBuffer<int> nbr, ntri, toff, vidx, eflag;
		nnrt::DeviceBuffer<uint8_t> cube;
	} mesh_scratch;
	// results awaiting a copy-out
	nnrt::CoordResult coords;
	nnrt::RowResult rows;
	nnrt::MeshResult mesh;

	nnrt::GridView view() const {
		nnrt::GridView g{};
		g.voxel_size = voxel_size;
		g.res = res;
		g.res3 = res3;
		g.keys = keys.ptr;
		g.tsdf = tsdf.ptr;
		g.weight = weight.ptr;
		g.weight_type = weight_type;
		g.color = color_type != nnrt::ST_NONE ? color.ptr : nullptr;
		g.color_type = color_type;
		g.hash = table.view();
		return g;
	}
	int channels() const { return color_type != nnrt::ST_NONE ? 8 : 5; }

	// The grid's one compaction step. rank = exclusive scan of flags[0, n); room in dst for max(total, 1) rows of `width`;
	// then scatter(total), which launches the kernel that writes the kept rows (a non-zero status from it ends the step:
	// activation reads its error word there, before any block is assigned); launch check; synchronise. *total = rows kept.
	template <typename T, typename Scatter>
	nnrt_status compact(const int* flags, int64_t n, nnrt::DeviceBuffer<T>& dst, size_t width, hipStream_t s, int64_t* total, Scatter&& scatter) {
		*total = 0;
		nnrt_status st;
		if ((st = compaction.rank.ensure(std::max<int64_t>(n, 1)))) return st;
		if ((st = nnrt::exclusive_sum_total(flags, compaction.rank.ptr, n, compaction.scan, s, total))) return st;
		if ((st = dst.ensure(width * static_cast<size_t>(std::max<int64_t>(*total, 1))))) return st;
		if ((st = scatter(*total))) return st;
		NNRT_LAUNCH_CHECK();
		NNRT_HIP(hipStreamSynchronize(s));
		return NNRT_OK;
	}
};

namespace nnrt {
// tsdf_grid.hip, for the other stages:
// activate the blocks at coordinates [n, 3]; a call with an out-of-range coordinate is refused and leaves the grid as it was
nnrt_status activate_coords(nnrt_voxel_grid* vg, const int32_t* d_coords, int64_t n, hipStream_t s);
// vg->coords = the inactive neighbours of every active block (neighbour-major, duplicates kept)
nnrt_status inactive_neighbor_coords(nnrt_voxel_grid* vg, hipStream_t s);
// vg->coords = the rows of query.coords [n, 3] with query.keep set
nnrt_status compact_kept_coords(nnrt_voxel_grid* vg, int64_t n, hipStream_t s);
} // namespace nnrt
