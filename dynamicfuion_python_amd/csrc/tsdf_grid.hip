// The voxel block grid itself (tsdf_grid.hpp): create / destroy / info, the hash table, capacity
// growth, activation, the dedupe of the blocks a depth frame touches, block coordinates and sleeve blocks.
#include <cmath>
#include <memory>
#include <type_traits>

#include "tsdf_grid.hpp"

namespace nnrt {
namespace {

// inverse of a 4x4 (double, Gauss-Jordan with partial pivoting; Open3D inverts the extrinsic in double on the host)
bool invert4(const double* a, double* out) {
	double m[4][8];
	for (int r = 0; r < 4; r++)
		for (int c = 0; c < 8; c++) m[r][c] = c < 4 ? a[4 * r + c] : (c - 4 == r ? 1.0 : 0.0);
	for (int c = 0; c < 4; c++) {
		int p = c;
		for (int r = c + 1; r < 4; r++)
			if (std::fabs(m[r][c]) > std::fabs(m[p][c])) p = r;
		if (m[p][c] == 0.0) return false;
		if (p != c)
			for (int k = 0; k < 8; k++) std::swap(m[p][k], m[c][k]);
		const double d = m[c][c];
		for (int k = 0; k < 8; k++) m[c][k] /= d;
		for (int r = 0; r < 4; r++)
			if (r != c) {
				const double f = m[r][c];
				for (int k = 0; k < 8; k++) m[r][k] -= f * m[c][k];
			}
	}
	for (int r = 0; r < 4; r++)
		for (int c = 0; c < 4; c++) out[4 * r + c] = m[r][c + 4];
	return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// hash activation / dedupe
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_insert_min(HashView h, const int32_t* __restrict__ coords, const uint64_t* __restrict__ packed, int64_t n,
                             uint64_t* __restrict__ in_slot, int* error_flag) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	uint64_t key;
	if (coords) {
		const int x = coords[3 * i], y = coords[3 * i + 1], z = coords[3 * i + 2];
		if (!key_in_range(x, y, z)) {
			atomicOr(error_flag, 1);
			in_slot[i] = HASH_EMPTY;
			return;
		}
		key = pack_key(x, y, z);
	} else {
		key = packed[i];
		if (key == HASH_EMPTY) {
			in_slot[i] = HASH_EMPTY;
			return;
		}
	}
	const uint64_t s = hash_insert(h, key);
	atomicMin(h.first + s, static_cast<int>(i));
	in_slot[i] = s;
}

// new[i] = input i is the first carrier of a key not yet holding a block
__global__ void k_mark_new(HashView h, const uint64_t* __restrict__ in_slot, int64_t n, int* __restrict__ is_new) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t s = in_slot[i];
	is_new[i] = (s != HASH_EMPTY && h.first[s] == static_cast<int>(i) && h.block[s] < 0) ? 1 : 0;
}

__global__ void k_assign_blocks(HashView h, const uint64_t* __restrict__ in_slot, const int* __restrict__ is_new, const int* __restrict__ rank,
                                int64_t n, int64_t base, int32_t* __restrict__ keys_out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n || !is_new[i]) return;
	const uint64_t s = in_slot[i];
	const int64_t b = base + rank[i];
	h.block[s] = static_cast<int>(b);
	const uint64_t k = h.keys[s];
	keys_out[3 * b] = static_cast<int32_t>(k & 0x1fffff) - KEY_BIAS;
	keys_out[3 * b + 1] = static_cast<int32_t>((k >> 21) & 0x1fffff) - KEY_BIAS;
	keys_out[3 * b + 2] = static_cast<int32_t>((k >> 42) & 0x1fffff) - KEY_BIAS;
}

__global__ void k_fill_i32(int* p, int64_t n, int v) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i < n) p[i] = v;
}
__global__ void k_fill_u64(uint64_t* p, int64_t n, uint64_t v) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i < n) p[i] = v;
}
// rehash: every existing block key back into a fresh table
__global__ void k_rehash(HashView h, const int32_t* __restrict__ keys, int64_t n) {
	const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (b >= n) return;
	const uint64_t s = hash_insert(h, pack_key(keys[3 * b], keys[3 * b + 1], keys[3 * b + 2]));
	h.block[s] = static_cast<int>(b);
}

// ---------------------------------------------------------------------------------------------------------------------
// Open3D DepthTouch (GetUniqueBlockCoordinates, VoxelBlockGrid.cpp:237-270, down factor 4): every 4th pixel (both axes)
// with 0 < d < depth_max samples 4 points t_min + i (t_max - t_min) / 3 along its camera ray (t in [max(d - trunc, 0),
// min(d + trunc, depth_max)]) and touches the blocks that contain them. Keys are written at fixed positions
// (pixel-major, then sample) and deduplicated in that order.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TOUCH_STEPS = 3;
__global__ void k_touch_depth(ImageView im, int stride, Xform cam_to_world, float sdf_trunc, float block_size, uint64_t* __restrict__ out) {
	const int rows = im.H / stride, cols = im.W / stride;
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= static_cast<int64_t>(rows) * cols) return;
	const int y = static_cast<int>(i / cols) * stride, x = static_cast<int>(i % cols) * stride;
	const float d = read_depth(im, x, y) / im.depth_scale;
	uint64_t* o = out + (TOUCH_STEPS + 1) * i;
	if (!(d > 0.f && d < im.depth_max)) {
		for (int s = 0; s <= TOUCH_STEPS; s++) o[s] = HASH_EMPTY;
		return;
	}
	float xc, yc, zc, xg, yg, zg;
	cam_to_world.unproject(static_cast<float>(x), static_cast<float>(y), 1.0f, xc, yc, zc);
	cam_to_world.rigid(xc, yc, zc, xg, yg, zg);
	const float xo = cam_to_world.m[3], yo = cam_to_world.m[7], zo = cam_to_world.m[11];
	const float xd = xg - xo, yd = yg - yo, zd = zg - zo;
	const float t_min = fmaxf(d - sdf_trunc, 0.0f);
	const float t_max = fminf(d + sdf_trunc, im.depth_max);
	const float t_step = (t_max - t_min) / static_cast<float>(TOUCH_STEPS);
	float t = t_min;
	for (int s = 0; s <= TOUCH_STEPS; s++) {
		const int xb = static_cast<int>(floorf((xo + t * xd) / block_size));
		const int yb = static_cast<int>(floorf((yo + t * yd) / block_size));
		const int zb = static_cast<int>(floorf((zo + t * zd) / block_size));
		o[s] = key_in_range(xb, yb, zb) ? pack_key(xb, yb, zb) : HASH_EMPTY;
		t += t_step;
	}
}

__global__ void k_unique_compact(HashView h, const uint64_t* __restrict__ packed, const uint64_t* __restrict__ in_slot, const int* __restrict__ first,
                                 const int* __restrict__ rank, int64_t n, int32_t* __restrict__ out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n || !first[i]) return;
	const uint64_t k = packed[i];
	const int64_t r = rank[i];
	out[3 * r] = static_cast<int32_t>(k & 0x1fffff) - KEY_BIAS;
	out[3 * r + 1] = static_cast<int32_t>((k >> 21) & 0x1fffff) - KEY_BIAS;
	out[3 * r + 2] = static_cast<int32_t>((k >> 42) & 0x1fffff) - KEY_BIAS;
	(void) h;
	(void) in_slot;
}
__global__ void k_mark_first(HashView h, const uint64_t* __restrict__ in_slot, int64_t n, int* __restrict__ first) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t s = in_slot[i];
	first[i] = (s != HASH_EMPTY && h.first[s] == static_cast<int>(i)) ? 1 : 0;
}

// BufferCoordinatesOfInactiveNeighborBlocks (NonRigidSurfaceVoxelBlockGrid.cpp:68-96): the 27 neighbours of every
// active block, neighbour-major ([27][count]), kept when inactive (duplicates kept, as the reference)
__global__ void k_inactive_neighbors(GridView g, int64_t nb, int32_t* __restrict__ coords, int* __restrict__ inactive) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= 27 * nb) return;
	const int nbr = static_cast<int>(i / nb);
	const int64_t b = i % nb;
	const int dz = nbr / 9, dy = (nbr % 9) / 3, dx = nbr % 3;
	const int x = g.keys[3 * b] + dx - 1, y = g.keys[3 * b + 1] + dy - 1, z = g.keys[3 * b + 2] + dz - 1;
	coords[3 * i] = x;
	coords[3 * i + 1] = y;
	coords[3 * i + 2] = z;
	inactive[i] = key_in_range(x, y, z) && find_block(g.hash, x, y, z) < 0 ? 1 : 0;
}

int store_type_of(int dtype) {
	switch (dtype) {
		case NNRT_DTYPE_FLOAT32: return ST_F32;
		case NNRT_DTYPE_UINT16: return ST_U16;
		case NNRT_DTYPE_UINT8: return ST_U8;
		default: return ST_NONE;
	}
}

} // namespace

bool inverse_extrinsics(const double* h_E, double* out) {
	static const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
	return invert4(h_E ? h_E : I4, out);
}

nnrt_status HashTable::reset(uint64_t new_size, hipStream_t s) {
	nnrt_status st;
	if ((st = keys.ensure(new_size)) || (st = block.ensure(new_size)) || (st = first.ensure(new_size))) return st;
	size = new_size;
	const int64_t n = static_cast<int64_t>(size);
	k_fill_u64<<<grid_of(n), 256, 0, s>>>(keys.ptr, n, HASH_EMPTY);
	k_fill_i32<<<grid_of(n), 256, 0, s>>>(block.ptr, n, -1);
	return clear_first(s);
}
nnrt_status HashTable::clear_first(hipStream_t s) {
	const int64_t n = static_cast<int64_t>(size);
	k_fill_i32<<<grid_of(n), 256, 0, s>>>(first.ptr, n, 0x7fffffff);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

namespace {
// an empty table of `size` slots, then every block key back into it
nnrt_status rebuild_table(nnrt_voxel_grid* vg, uint64_t size, hipStream_t s) {
	const nnrt_status st = vg->table.reset(size, s);
	if (st) return st;
	if (vg->active > 0) k_rehash<<<grid_of(vg->active), 256, 0, s>>>(vg->table.view(), vg->keys.ptr, vg->active);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

// grow block storage to hold `need` blocks (x2 steps), keeping contents; the table is rebuilt at >= 2x capacity
nnrt_status ensure_capacity(nnrt_voxel_grid* vg, int64_t need, hipStream_t s) {
	if (need <= vg->capacity) return NNRT_OK;
	int64_t cap = std::max<int64_t>(vg->capacity, 1);
	while (cap < need) cap *= 2;
	const size_t vox_old = static_cast<size_t>(vg->capacity) * vg->res3, vox_new = static_cast<size_t>(cap) * vg->res3;
	auto grow = [&](auto& buf, size_t elem_old, size_t elem_new) -> nnrt_status {
		using T = std::remove_pointer_t<decltype(buf.ptr)>;
		DeviceBuffer<T> fresh;
		nnrt_status gs = fresh.ensure(elem_new);
		if (gs) return gs;
		NNRT_HIP(hipMemsetAsync(fresh.ptr, 0, sizeof(T) * elem_new, s));
		if (buf.ptr && elem_old) NNRT_HIP(hipMemcpyAsync(fresh.ptr, buf.ptr, sizeof(T) * elem_old, hipMemcpyDeviceToDevice, s));
		NNRT_HIP(hipStreamSynchronize(s));
		buf = std::move(fresh);
		return NNRT_OK;
	};
	nnrt_status st;
	if ((st = grow(vg->tsdf, vox_old, vox_new)) || (st = grow(vg->weight, vox_old * store_bytes(vg->weight_type), vox_new * store_bytes(vg->weight_type))) ||
	    (st = grow(vg->color, vox_old * 3 * store_bytes(vg->color_type), vox_new * 3 * store_bytes(vg->color_type))) ||
	    (st = grow(vg->keys, static_cast<size_t>(vg->capacity) * 3, static_cast<size_t>(cap) * 3)))
		return st;
	vg->capacity = cap;
	const uint64_t tsize = HashTable::size_for(cap);
	if (tsize != vg->table.size) return rebuild_table(vg, tsize, s);
	return NNRT_OK;
}

// unique coordinates of packed keys (HASH_EMPTY skipped), in first-occurrence order, into vg->coords, via the dedupe
// table (the grid's own table is not touched)
nnrt_status unique_packed(nnrt_voxel_grid* vg, const uint64_t* packed, int64_t n, hipStream_t s) {
	vg->coords.count = 0;
	if (n == 0) return NNRT_OK;
	auto& a = vg->act;
	nnrt_status st;
	if ((st = vg->dedupe.reset(HashTable::size_for(n), s)) || (st = a.slot.ensure(n)) || (st = a.flag.ensure(n))) return st;
	const HashView h = vg->dedupe.view();
	k_insert_min<<<grid_of(n), 256, 0, s>>>(h, nullptr, packed, n, a.slot.ptr, nullptr);
	k_mark_first<<<grid_of(n), 256, 0, s>>>(h, a.slot.ptr, n, a.flag.ptr);
	NNRT_LAUNCH_CHECK();
	int64_t total = 0;
	if ((st = vg->compact(a.flag.ptr, n, vg->coords.rows, 3, s, &total, [&](int64_t) {
		     k_unique_compact<<<grid_of(n), 256, 0, s>>>(h, packed, a.slot.ptr, a.flag.ptr, vg->compaction.rank.ptr, n, vg->coords.rows.ptr);
		     return NNRT_OK;
	     })))
		return st;
	vg->coords.count = total;
	return NNRT_OK;
}
} // namespace

// Activate (Open3D HashMap::Activate): every key takes the lowest input index that carries it; the first carriers of
// keys without a block create blocks, in input order
nnrt_status activate_coords(nnrt_voxel_grid* vg, const int32_t* d_coords, int64_t n, hipStream_t s) {
	if (n == 0) return NNRT_OK;
	auto& a = vg->act;
	nnrt_status st;
	// worst case: every input new -> keep the table at most half full before inserting
	if ((st = ensure_capacity(vg, vg->active + n, s))) return st;
	if ((st = a.slot.ensure(n)) || (st = a.flag.ensure(n)) || (st = a.error.ensure(1))) return st;
	NNRT_HIP(hipMemsetAsync(a.error.ptr, 0, sizeof(int), s));
	if ((st = vg->table.clear_first(s))) return st;
	const HashView h = vg->table.view();
	k_insert_min<<<grid_of(n), 256, 0, s>>>(h, d_coords, nullptr, n, a.slot.ptr, a.error.ptr);
	k_mark_new<<<grid_of(n), 256, 0, s>>>(h, a.slot.ptr, n, a.flag.ptr);
	NNRT_LAUNCH_CHECK();
	int64_t total = 0;
	// the destination is the key storage itself, which ensure_capacity has sized: new keys land at rows active + rank
	st = vg->compact(a.flag.ptr, n, vg->keys, 3, s, &total, [&](int64_t created) -> nnrt_status {
		// a call with an out-of-range coordinate is refused as a whole, before any block is assigned: its in-range keys
		// already sit in the table (without a block), so the table is rebuilt from the block keys and the grid is as it
		// was before the call
		int refused = 0;
		NNRT_HIP(hipMemcpyAsync(&refused, a.error.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));
		if (refused) {
			const nnrt_status rs = rebuild_table(vg, vg->table.size, s);
			if (rs) return rs;
			set_error("block coordinate out of range (|coordinate| must stay below 2^20)");
			return NNRT_ERROR_ARGUMENT;
		}
		if (created > 0) k_assign_blocks<<<grid_of(n), 256, 0, s>>>(h, a.slot.ptr, a.flag.ptr, vg->compaction.rank.ptr, n, vg->active, vg->keys.ptr);
		return NNRT_OK;
	});
	if (st) return st;
	if (total > 0) {   // new blocks start at zero (tsdf, weight, color)
		const size_t v0 = static_cast<size_t>(vg->active) * vg->res3, nv = static_cast<size_t>(total) * vg->res3;
		NNRT_HIP(hipMemsetAsync(vg->tsdf.ptr + v0, 0, sizeof(float) * nv, s));
		NNRT_HIP(hipMemsetAsync(vg->weight.ptr + v0 * store_bytes(vg->weight_type), 0, nv * store_bytes(vg->weight_type), s));
		if (vg->color_type != ST_NONE) NNRT_HIP(hipMemsetAsync(vg->color.ptr + v0 * 3 * store_bytes(vg->color_type), 0, nv * 3 * store_bytes(vg->color_type), s));
	}
	vg->active += total;
	return NNRT_OK;
}

nnrt_status compact_kept_coords(nnrt_voxel_grid* vg, int64_t n, hipStream_t s) {
	auto& q = vg->query;
	vg->coords.count = 0;
	int64_t total = 0;
	const nnrt_status st = vg->compact(q.keep.ptr, n, vg->coords.rows, 3, s, &total, [&](int64_t) {
		if (n > 0) k_compact_rows<int32_t><<<grid_of(n), 256, 0, s>>>(q.coords.ptr, q.keep.ptr, vg->compaction.rank.ptr, n, 3, vg->coords.rows.ptr);
		return NNRT_OK;
	});
	if (st) return st;
	vg->coords.count = total;
	return NNRT_OK;
}

nnrt_status inactive_neighbor_coords(nnrt_voxel_grid* vg, hipStream_t s) {
	auto& q = vg->query;
	const int64_t n = 27 * vg->active;
	nnrt_status st;
	if ((st = q.coords.ensure(3 * static_cast<size_t>(std::max<int64_t>(n, 1)))) || (st = q.keep.ensure(std::max<int64_t>(n, 1)))) return st;
	if (n > 0) k_inactive_neighbors<<<grid_of(n), 256, 0, s>>>(vg->view(), vg->active, q.coords.ptr, q.keep.ptr);
	NNRT_LAUNCH_CHECK();
	return compact_kept_coords(vg, n, s);
}

} // namespace nnrt

using namespace nnrt;

extern "C" {

nnrt_status nnrt_voxel_grid_create(float voxel_size, int32_t block_resolution, int64_t block_count, int32_t weight_dtype, int32_t color_dtype,
                                   int32_t device, nnrt_voxel_grid** out) {
	NNRT_CHECK_ARG(out, "null output");
	*out = nullptr;
	NNRT_CHECK_ARG(voxel_size > 0.f && block_resolution >= 2 && block_resolution <= 32 && block_count >= 1, "invalid grid geometry");
	NNRT_CHECK_ARG(weight_dtype == NNRT_DTYPE_FLOAT32 || weight_dtype == NNRT_DTYPE_UINT16, "weight dtype must be float32 or uint16");
	NNRT_CHECK_ARG(color_dtype == NNRT_DTYPE_NONE || color_dtype == NNRT_DTYPE_FLOAT32 || color_dtype == NNRT_DTYPE_UINT16 ||
	                   color_dtype == NNRT_DTYPE_UINT8,
	               "color dtype must be none, float32, uint16 or uint8");
	DeviceGuard guard(device);
	std::unique_ptr<nnrt_voxel_grid> vg(new nnrt_voxel_grid());
	vg->device = device;
	vg->voxel_size = voxel_size;
	vg->res = block_resolution;
	vg->res3 = block_resolution * block_resolution * block_resolution;
	vg->weight_type = store_type_of(weight_dtype);
	vg->color_type = store_type_of(color_dtype);
	vg->coords.width = 3;
	const nnrt_status st = ensure_capacity(vg.get(), block_count, nullptr);   // block_count >= 1: builds the table too
	if (st) return st;
	NNRT_HIP(hipDeviceSynchronize());
	*out = vg.release();
	return NNRT_OK;
}

void nnrt_voxel_grid_destroy(nnrt_voxel_grid* vg) {
	if (!vg) return;
	DeviceGuard guard(vg->device);
	hipDeviceSynchronize();
	delete vg;
}

nnrt_status nnrt_voxel_grid_get_info(const nnrt_voxel_grid* vg, int64_t* h_active_blocks, int64_t* h_capacity, float* h_voxel_size,
                                     int32_t* h_block_resolution) {
	NNRT_CHECK_ARG(vg, "null grid");
	if (h_active_blocks) *h_active_blocks = vg->active;
	if (h_capacity) *h_capacity = vg->capacity;
	if (h_voxel_size) *h_voxel_size = vg->voxel_size;
	if (h_block_resolution) *h_block_resolution = vg->res;
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_activate(nnrt_voxel_grid* vg, const int32_t* d_block_coords, int64_t count, void* stream) {
	NNRT_CHECK_ARG(vg && (count == 0 || d_block_coords) && count >= 0, "invalid arguments");
	DeviceGuard guard(vg->device);
	return activate_coords(vg, d_block_coords, count, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_voxel_grid_get_block_coordinates(const nnrt_voxel_grid* vg, int32_t* d_out, void* stream) {
	NNRT_CHECK_ARG(vg && d_out, "invalid arguments");
	DeviceGuard guard(vg->device);
	if (vg->active) NNRT_HIP(hipMemcpyAsync(d_out, vg->keys.ptr, sizeof(int32_t) * 3 * vg->active, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_unique_block_coordinates(nnrt_voxel_grid* vg, const void* d_depth, int32_t depth_dtype, int32_t height, int32_t width,
                                                     const double* h_K, const double* h_E, float depth_scale, float depth_max,
                                                     float trunc_voxel_multiplier, int64_t* h_count, void* stream) {
	NNRT_CHECK_ARG(vg && d_depth && h_K && h_count && height > 0 && width > 0, "invalid arguments");
	NNRT_CHECK_ARG(depth_dtype == NNRT_DTYPE_UINT16 || depth_dtype == NNRT_DTYPE_FLOAT32, "depth must be uint16 or float32");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	double Einv[16];
	if (!inverse_extrinsics(h_E, Einv)) {
		set_error("extrinsic matrix is singular");   // as first written: without the "invalid argument: " that the ray cast's carries
		return NNRT_ERROR_ARGUMENT;
	}
	constexpr int STRIDE = 4;   // VoxelBlockGrid.cpp:250 down_factor
	const int64_t n = static_cast<int64_t>(height / STRIDE) * (width / STRIDE) * (TOUCH_STEPS + 1);
	nnrt_status st;
	if ((st = vg->act.touched.ensure(std::max<int64_t>(n, 1)))) return st;
	const ImageView im = make_image(d_depth, depth_dtype, height, width, nullptr, 0, 0, depth_scale, depth_max);
	if (n > 0) k_touch_depth<<<grid_of(n / (TOUCH_STEPS + 1)), 256, 0, s>>>(im, STRIDE, make_xform(h_K, Einv), vg->voxel_size * trunc_voxel_multiplier,
	                                                                      vg->voxel_size * static_cast<float>(vg->res), vg->act.touched.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = unique_packed(vg, vg->act.touched.ptr, n, s))) return st;
	*h_count = vg->coords.count;
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_copy_result_coordinates(const nnrt_voxel_grid* vg, int32_t* d_out, void* stream) {
	NNRT_CHECK_ARG(vg && (d_out || vg->coords.count == 0), "invalid arguments");
	DeviceGuard guard(vg->device);
	return vg->coords.copy_out(d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_voxel_grid_activate_sleeve_blocks(nnrt_voxel_grid* vg, int64_t* h_count, void* stream) {
	NNRT_CHECK_ARG(vg && h_count, "invalid arguments");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	nnrt_status st;
	if ((st = inactive_neighbor_coords(vg, s))) return st;
	const int64_t m = vg->coords.count;
	*h_count = m;   // the reference returns the count with duplicates (:109)
	if (m == 0) return NNRT_OK;
	if ((st = vg->query.coords.ensure(3 * static_cast<size_t>(m)))) return st;
	NNRT_HIP(hipMemcpyAsync(vg->query.coords.ptr, vg->coords.rows.ptr, sizeof(int32_t) * 3 * m, hipMemcpyDeviceToDevice, s));
	return activate_coords(vg, vg->query.coords.ptr, m, s);
}

} // extern "C"
