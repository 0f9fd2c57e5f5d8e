// Reading the voxel block grid out (tsdf_grid.hpp, DESIGN.md sections 12 and 29): voxel values of every active block and
// at given coordinates, and the triangle mesh by marching cubes.
#include <cstring>

#include "mc_table.hpp"
#include "tsdf_grid.hpp"

namespace nnrt {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// ExtractVoxelValuesAndCoordinates / ExtractVoxelValuesAt (NonRigidSurfaceVoxelBlockGridImpl.h:446-652)
// rows: x, y, z (metres), tsdf, weight, (r, g, b)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_values_all(GridView g, int64_t nb, int C, float* __restrict__ out) {
	const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (w >= nb * g.res3) return;
	const int b = static_cast<int>(w / g.res3), vi = static_cast<int>(w % g.res3);
	int xv, yv, zv;
	voxel_local(vi, g.res, xv, yv, zv);
	float* o = out + w * C;
	o[0] = static_cast<float>(g.keys[3 * b] * g.res + xv) * g.voxel_size;
	o[1] = static_cast<float>(g.keys[3 * b + 1] * g.res + yv) * g.voxel_size;
	o[2] = static_cast<float>(g.keys[3 * b + 2] * g.res + zv) * g.voxel_size;
	const int64_t lin = static_cast<int64_t>(b) * g.res3 + vi;
	o[3] = g.tsdf[lin];
	o[4] = read_store(g.weight, g.weight_type, lin);
	if (C > 5)
		for (int c = 0; c < 3; c++) o[5 + c] = read_store(g.color, g.color_type, 3 * lin + c);
}

// The reference indexes the voxel inside its block with the GLOBAL coordinate (CoordToWorkload of x, y, z, :619-620),
// which is the local index only for block (0, 0, 0); reproduced, rows whose index leaves the voxel storage keep -2.
// Query blocks are x / res with C++ integer division (toward zero), as the tensor division at :239.
__global__ void k_values_at(GridView g, int64_t active, const int32_t* __restrict__ q, int64_t n, int C, float* __restrict__ out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float* o = out + i * C;
	for (int c = 0; c < C; c++) o[c] = -2.f;
	const int x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
	const int b = find_block(g.hash, x / g.res, y / g.res, z / g.res);
	if (b < 0) return;
	const int64_t vib = static_cast<int64_t>(x) + static_cast<int64_t>(g.res) * (y + static_cast<int64_t>(g.res) * z);
	const int64_t lin = static_cast<int64_t>(b) * g.res3 + vib;
	if (lin < 0 || lin >= active * g.res3) return;
	o[0] = static_cast<float>(x) * g.voxel_size;
	o[1] = static_cast<float>(y) * g.voxel_size;
	o[2] = static_cast<float>(z) * g.voxel_size;
	o[3] = g.tsdf[lin];
	o[4] = read_store(g.weight, g.weight_type, lin);
	if (C > 5)
		for (int c = 0; c < 3; c++) o[5 + c] = read_store(g.color, g.color_type, 3 * lin + c);
}
// rows of found queries only (the reference drops queries whose block is inactive, :241-243)
__global__ void k_found_mask(GridView g, const int32_t* __restrict__ q, int64_t n, int* __restrict__ found) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= n) return;
	found[i] = find_block(g.hash, q[3 * i] / g.res, q[3 * i + 1] / g.res, q[3 * i + 2] / g.res) >= 0 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Marching cubes (the Open3D ExtractTriangleMesh algorithm, VoxelBlockGrid.cpp:461-497 -> voxel_grid::ExtractTriangleMesh,
// restated): corner i of the cube at voxel v is v + (i & 1, (i >> 1) & 1, i >> 2) in Bourke numbering (v0 (0,0,0),
// v1 (1,0,0), v2 (1,1,0), v3 (0,1,0), v4..v7 the same at z + 1); bit i of the cube index is tsdf < 0. A cube counts
// only if all 8 corners exist with weight > threshold. Every cube edge is owned by its lower voxel and axis (the
// reference's edge_shifts): a vertex lives on each owned edge of some valid surface cube, at the zero crossing of the
// linear interpolation, with the normal interpolated from central-difference tsdf gradients and the color likewise.
// The triangle table is the published one Open3D indexes (csrc/mc_table.hpp: Lorensen-Cline / Bourke), each triangle
// emitted in Open3D's vertex order (normals towards positive tsdf).
// Vertex and triangle order: blocks in buffer order, voxels in block order, owned edges x, y, z -- deterministic.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MC_MAX_TRI = 10;
struct McTables {
	uint16_t edge_mask[256];
	int8_t tri[256][3 * MC_MAX_TRI + 1];   // edge triples, -1 terminated
	int8_t ntri[256];
};
__constant__ McTables c_mc;
__constant__ int8_t c_edge_owner[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
                                           {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};

McTables build_mc_tables() {
	static const int edge_v[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
	McTables t{};
	for (int cfg = 0; cfg < 256; cfg++) {
		uint16_t mask = 0;
		for (int e = 0; e < 12; e++)
			if (((cfg >> edge_v[e][0]) & 1) != ((cfg >> edge_v[e][1]) & 1)) mask |= static_cast<uint16_t>(1u << e);
		t.edge_mask[cfg] = mask;
		int nt = 0;
		// (a, b, c) -> (c, b, a): Open3D's ExtractTriangleMesh stores table vertex v at triangle slot 2 - v (third-party,
		// absent here: restated from its published source; same winding as (a, c, b), parity unpinned)
		for (int i = 0; i < 16 && MC_TRI_TABLE[cfg][i] >= 0; i += 3, nt++) {
			t.tri[cfg][3 * nt] = MC_TRI_TABLE[cfg][i + 2];
			t.tri[cfg][3 * nt + 1] = MC_TRI_TABLE[cfg][i + 1];
			t.tri[cfg][3 * nt + 2] = MC_TRI_TABLE[cfg][i];
		}
		t.tri[cfg][3 * nt] = -1;
		t.ntri[cfg] = static_cast<int8_t>(nt);
	}
	return t;
}

struct MeshGridView {
	GridView g;
	const int* nbr;   // [nb, 27] buffer index of neighbour (dx, dy, dz) in {-1,0,1}^3 at (dx+1) + 3 (dy+1) + 9 (dz+1); -1: none
	float weight_threshold;
};
// the voxel at local (x, y, z) of block b, which may lie in a neighbouring block (-1: none)
__device__ inline int64_t voxel_at(const MeshGridView& m, int b, int x, int y, int z) {
	const int R = m.g.res;
	const int dx = x < 0 ? -1 : (x >= R ? 1 : 0), dy = y < 0 ? -1 : (y >= R ? 1 : 0), dz = z < 0 ? -1 : (z >= R ? 1 : 0);
	const int nb = m.nbr[27 * static_cast<int64_t>(b) + (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)];
	if (nb < 0) return -1;
	const int lx = x - dx * R, ly = y - dy * R, lz = z - dz * R;
	return static_cast<int64_t>(nb) * m.g.res3 + lx + R * (ly + R * lz);
}

__global__ void k_block_neighbors(GridView g, int64_t nb, int* __restrict__ nbr) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= 27 * nb) return;
	const int64_t b = i / 27;
	const int k = static_cast<int>(i % 27);
	nbr[i] = find_block(g.hash, g.keys[3 * b] + k % 3 - 1, g.keys[3 * b + 1] + (k / 3) % 3 - 1, g.keys[3 * b + 2] + k / 9 - 1);
}

// pass 1: cube index per voxel (0 = no surface) and its triangle count
__global__ void k_mc_cubes(MeshGridView m, int64_t nb, uint8_t* __restrict__ cube, int* __restrict__ ntri, int* __restrict__ edge_flag) {
	const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (w >= nb * m.g.res3) return;
	const int b = static_cast<int>(w / m.g.res3), vi = static_cast<int>(w % m.g.res3);
	int x, y, z;
	voxel_local(vi, m.g.res, x, y, z);
	int idx = 0;
	bool valid = true;
	// Bourke corner offsets
	const int off[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
	for (int c = 0; c < 8; c++) {
		const int64_t v = voxel_at(m, b, x + off[c][0], y + off[c][1], z + off[c][2]);
		if (v < 0 || !(read_store(m.g.weight, m.g.weight_type, v) > m.weight_threshold)) {
			valid = false;
			break;
		}
		if (m.g.tsdf[v] < 0) idx |= 1 << c;
	}
	if (!valid || idx == 0 || idx == 255) {
		cube[w] = 0;
		ntri[w] = 0;
		return;
	}
	cube[w] = static_cast<uint8_t>(idx);
	ntri[w] = c_mc.ntri[idx];
	const uint16_t mask = c_mc.edge_mask[idx];
	for (int e = 0; e < 12; e++) {
		if (!(mask & (1u << e))) continue;
		const int64_t ov = voxel_at(m, b, x + c_edge_owner[e][0], y + c_edge_owner[e][1], z + c_edge_owner[e][2]);
		edge_flag[3 * ov + c_edge_owner[e][3]] = 1;   // benign race: every writer stores 1
	}
}

__device__ inline float tsdf_or(const MeshGridView& m, int b, int x, int y, int z, float fallback) {
	const int64_t v = voxel_at(m, b, x, y, z);
	return v < 0 ? fallback : m.g.tsdf[v];
}
// central-difference tsdf gradient (a missing neighbour contributes the centre value)
__device__ inline void grad_at(const MeshGridView& m, int b, int x, int y, int z, float c, float* n) {
	n[0] = tsdf_or(m, b, x + 1, y, z, c) - tsdf_or(m, b, x - 1, y, z, c);
	n[1] = tsdf_or(m, b, x, y + 1, z, c) - tsdf_or(m, b, x, y - 1, z, c);
	n[2] = tsdf_or(m, b, x, y, z + 1, c) - tsdf_or(m, b, x, y, z - 1, c);
}

// pass 2: vertices on the flagged owned edges (index = exclusive scan of the flags)
__global__ void k_mc_vertices(MeshGridView m, int64_t nb, const int* __restrict__ edge_flag, const int* __restrict__ vidx, float* __restrict__ vpos,
                              float* __restrict__ vnrm, float* __restrict__ vcol) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= 3 * nb * m.g.res3 || !edge_flag[i]) return;
	const int64_t w = i / 3;
	const int d = static_cast<int>(i % 3);
	const int b = static_cast<int>(w / m.g.res3), vi = static_cast<int>(w % m.g.res3);
	int x, y, z;
	voxel_local(vi, m.g.res, x, y, z);
	const int ex = d == 0, ey = d == 1, ez = d == 2;
	const int64_t vo = w, ve = voxel_at(m, b, x + ex, y + ey, z + ez);
	const float to = m.g.tsdf[vo], te = m.g.tsdf[ve];
	const float ratio = (0.0f - to) / (te - to);
	const int64_t o = vidx[i];
	const int R = m.g.res;
	vpos[3 * o] = (static_cast<float>(m.g.keys[3 * b] * R + x) + ratio * ex) * m.g.voxel_size;
	vpos[3 * o + 1] = (static_cast<float>(m.g.keys[3 * b + 1] * R + y) + ratio * ey) * m.g.voxel_size;
	vpos[3 * o + 2] = (static_cast<float>(m.g.keys[3 * b + 2] * R + z) + ratio * ez) * m.g.voxel_size;
	float no[3], ne[3], n[3];
	grad_at(m, b, x, y, z, to, no);
	grad_at(m, b, x + ex, y + ey, z + ez, te, ne);
	for (int k = 0; k < 3; k++) n[k] = (1 - ratio) * no[k] + ratio * ne[k];
	const float nn = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
	for (int k = 0; k < 3; k++) vnrm[3 * o + k] = nn > 0.f ? n[k] / nn : 0.f;
	if (vcol) {
		for (int k = 0; k < 3; k++) {
			const float co = read_store(m.g.color, m.g.color_type, 3 * vo + k), ce = read_store(m.g.color, m.g.color_type, 3 * ve + k);
			vcol[3 * o + k] = ((1 - ratio) * co + ratio * ce) / 255.0f;
		}
	}
}

// pass 3: triangles (offset = exclusive scan of the per-cube counts)
__global__ void k_mc_triangles(MeshGridView m, int64_t nb, const uint8_t* __restrict__ cube, const int* __restrict__ toff, const int* __restrict__ vidx,
                               int64_t* __restrict__ tris) {
	const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (w >= nb * m.g.res3 || cube[w] == 0) return;
	const int idx = cube[w];
	const int b = static_cast<int>(w / m.g.res3), vi = static_cast<int>(w % m.g.res3);
	int x, y, z;
	voxel_local(vi, m.g.res, x, y, z);
	int64_t o = toff[w];
	for (int t = 0; t < c_mc.ntri[idx]; t++, o++) {
		for (int k = 0; k < 3; k++) {
			const int e = c_mc.tri[idx][3 * t + k];
			const int64_t ov = voxel_at(m, b, x + c_edge_owner[e][0], y + c_edge_owner[e][1], z + c_edge_owner[e][2]);
			tris[3 * o + k] = vidx[3 * ov + c_edge_owner[e][3]];
		}
	}
}

nnrt_status upload_mc_tables() {
	static bool done_for[64] = {false};
	int dev = 0;
	hipGetDevice(&dev);
	if (dev >= 0 && dev < 64 && done_for[dev]) return NNRT_OK;
	const McTables t = build_mc_tables();
	NNRT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_mc), &t, sizeof(t)));
	if (dev >= 0 && dev < 64) done_for[dev] = true;
	return NNRT_OK;
}

} // namespace
} // namespace nnrt

using namespace nnrt;

extern "C" {

nnrt_status nnrt_voxel_grid_extract_voxel_values_and_coordinates(const nnrt_voxel_grid* vg, float* d_out, int32_t* h_channels, void* stream) {
	NNRT_CHECK_ARG(vg && (d_out || vg->active == 0), "invalid arguments");
	DeviceGuard guard(vg->device);
	if (h_channels) *h_channels = vg->channels();
	const int64_t n = vg->active * vg->res3;
	if (n > 0) k_values_all<<<grid_of(n), 256, 0, static_cast<hipStream_t>(stream)>>>(vg->view(), vg->active, vg->channels(), d_out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_extract_voxel_values_at(nnrt_voxel_grid* vg, const int32_t* d_query, int64_t count, int64_t* h_rows, int32_t* h_channels,
                                                    void* stream) {
	NNRT_CHECK_ARG(vg && h_rows && (count == 0 || d_query) && count >= 0, "invalid arguments");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	auto& q = vg->query;
	const int C = vg->channels();
	if (h_channels) *h_channels = C;
	vg->rows.width = C;
	vg->rows.count = 0;
	*h_rows = 0;
	if (count == 0) return NNRT_OK;
	nnrt_status st;
	if ((st = q.rows.ensure(static_cast<size_t>(count) * C)) || (st = q.keep.ensure(count))) return st;
	const GridView g = vg->view();
	// the storage of the active blocks bounds the quirk index: rows do not depend on how far the capacity has grown
	k_values_at<<<grid_of(count), 256, 0, s>>>(g, vg->active, d_query, count, C, q.rows.ptr);
	k_found_mask<<<grid_of(count), 256, 0, s>>>(g, d_query, count, q.keep.ptr);
	NNRT_LAUNCH_CHECK();
	int64_t total = 0;
	if ((st = vg->compact(q.keep.ptr, count, vg->rows.rows, C, s, &total, [&](int64_t) {
		     k_compact_rows<float><<<grid_of(count), 256, 0, s>>>(q.rows.ptr, q.keep.ptr, vg->compaction.rank.ptr, count, C, vg->rows.rows.ptr);
		     return NNRT_OK;
	     })))
		return st;
	vg->rows.count = total;
	*h_rows = total;
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_copy_result_rows(const nnrt_voxel_grid* vg, float* d_out, void* stream) {
	NNRT_CHECK_ARG(vg && (d_out || vg->rows.count == 0), "invalid arguments");
	DeviceGuard guard(vg->device);
	return vg->rows.copy_out(d_out, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_voxel_grid_extract_triangle_mesh(nnrt_voxel_grid* vg, float weight_threshold, int64_t* h_vertex_count, int64_t* h_triangle_count,
                                                  void* stream) {
	NNRT_CHECK_ARG(vg && h_vertex_count && h_triangle_count, "invalid arguments");
	DeviceGuard guard(vg->device);
	hipStream_t s = static_cast<hipStream_t>(stream);
	auto& w = vg->mesh_scratch;
	auto& r = vg->mesh;
	nnrt_status st;
	if ((st = upload_mc_tables())) return st;
	r.nv = r.nt = 0;
	*h_vertex_count = *h_triangle_count = 0;
	const int64_t nb = vg->active, nvox = nb * vg->res3;
	if (nb == 0) return NNRT_OK;
	if ((st = w.nbr.ensure(27 * static_cast<size_t>(nb))) || (st = w.cube.ensure(nvox)) || (st = w.ntri.ensure(nvox)) || (st = w.toff.ensure(nvox)) ||
	    (st = w.eflag.ensure(3 * static_cast<size_t>(nvox))) || (st = w.vidx.ensure(3 * static_cast<size_t>(nvox))))
		return st;
	MeshGridView m{vg->view(), w.nbr.ptr, weight_threshold};
	k_block_neighbors<<<grid_of(27 * nb), 256, 0, s>>>(m.g, nb, w.nbr.ptr);
	NNRT_HIP(hipMemsetAsync(w.eflag.ptr, 0, sizeof(int) * 3 * nvox, s));
	k_mc_cubes<<<grid_of(nvox), 256, 0, s>>>(m, nb, w.cube.ptr, w.ntri.ptr, w.eflag.ptr);
	NNRT_LAUNCH_CHECK();
	int64_t nv = 0, nt = 0;
	if ((st = exclusive_sum_total(w.eflag.ptr, w.vidx.ptr, 3 * nvox, vg->compaction.scan, s, &nv))) return st;
	if ((st = exclusive_sum_total(w.ntri.ptr, w.toff.ptr, nvox, vg->compaction.scan, s, &nt))) return st;
	const size_t v3 = 3 * static_cast<size_t>(std::max<int64_t>(nv, 1)), t3 = 3 * static_cast<size_t>(std::max<int64_t>(nt, 1));
	if ((st = r.vpos.ensure(v3)) || (st = r.vnrm.ensure(v3)) || (st = r.vcol.ensure(v3)) || (st = r.tris.ensure(t3))) return st;
	k_mc_vertices<<<grid_of(3 * nvox), 256, 0, s>>>(m, nb, w.eflag.ptr, w.vidx.ptr, r.vpos.ptr, r.vnrm.ptr, vg->color_type != ST_NONE ? r.vcol.ptr : nullptr);
	k_mc_triangles<<<grid_of(nvox), 256, 0, s>>>(m, nb, w.cube.ptr, w.toff.ptr, w.vidx.ptr, r.tris.ptr);
	NNRT_LAUNCH_CHECK();
	NNRT_HIP(hipStreamSynchronize(s));
	r.nv = nv;
	r.nt = nt;
	*h_vertex_count = nv;
	*h_triangle_count = nt;
	return NNRT_OK;
}

nnrt_status nnrt_voxel_grid_copy_mesh(const nnrt_voxel_grid* vg, float* d_vertices, float* d_normals, float* d_colors, int64_t* d_triangles, void* stream) {
	NNRT_CHECK_ARG(vg, "null grid");
	DeviceGuard guard(vg->device);
	return vg->mesh.copy_out(d_vertices, d_normals, vg->color_type != ST_NONE ? d_colors : nullptr, d_triangles, static_cast<hipStream_t>(stream));
}

// the marching-cubes triangle table in emission order (host copy, for tests): tri [256][31] int8 (edge triples, -1 terminated)
nnrt_status nnrt_marching_cubes_table(int8_t* h_tri, uint16_t* h_edge_mask) {
	NNRT_CHECK_ARG(h_tri || h_edge_mask, "null output");
	const McTables t = build_mc_tables();
	if (h_tri) std::memcpy(h_tri, t.tri, sizeof(t.tri));
	if (h_edge_mask) std::memcpy(h_edge_mask, t.edge_mask, sizeof(t.edge_mask));
	return NNRT_OK;
}

} // extern "C"
