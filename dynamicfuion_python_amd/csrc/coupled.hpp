// The fitter's coupled data term (NNRT_DATA_COUPLED): the frame's node-pair structure, the launch
// that sums the off-diagonal data blocks, and the assembly of the full Gauss-Newton system for the tile-sparse solver.
#pragma once

#include "coupled_host.hpp"
#include "fitter_kernels.hpp"

namespace nnrt {

// Once per frame: the unique unordered node pairs (i, j), i < j, that share a face (k_face_node_table's rows), united
// with the hierarchy's edges; ascending (i, j); with the tables of coupled_host.hpp on the device.
struct PairStructure {
	int M = 0;
	std::vector<int32_t> h_pairs;          // [M, 2]
	DeviceBuffer<int32_t> pairs;           // [M, 2]
	DeviceBuffer<int> row_off, edge_off, edge_list, inc_off, inc_list;
	DeviceBuffer<uint64_t> keys, keys_sorted;
	DeviceBuffer<int> d_count;
	DeviceBuffer<uint8_t> tmp;
	// The coupled solve is the arrowhead solve over the pairs with an empty stem (arrow base 0: every node is in the
	// corner, which `corner` plans over h_pairs), a different shape from ArrowheadStructure's: no stem blocks, no Schur
	// lists. The structure-derived fields of its workspace; no_dinv [>= 1] and no_edges [1] = {0} stand for the stem's
	// buffers, which no launch reads past.
	void bind(ArrowheadWorkspace& ws, const CornerSolver& corner, int N, float* no_dinv, int* no_edges) const {
		ws.N = N;
		ws.n0 = 0;
		ws.E = M;
		ws.m = 6 * N;
		ws.corner = &corner;
		ws.dinv = ws.dinv_b = no_dinv;
		ws.edge_offsets = ws.edge_list = no_edges;
		ws.inc_off = inc_off.ptr;
		ws.inc_list = inc_list.ptr;
	}
};
// builds ps on stream s (device: keys, sort, unique; one host round trip for the count and the coordinates, which the
// solver's plan needs; then the host tables). h_edges / d_edges: the hierarchy's edges [E, 2] (virtual order).
// *moved: a device buffer a captured graph may hold was reallocated.
nnrt_status build_pair_structure(PairStructure& ps, const uint32_t* face_nodes, int64_t F, int K, const int32_t* d_edges,
                                 const int32_t* h_edges, int E, int N, hipStream_t s, bool* moved);

// per iteration, after the fused pixel launch: block (a, b) of every pair of a contributing pixel's face nodes gains
// J_a^T J_b, the exact products summed in double (pair_acc [M, 36], zeroed on the stream before the launch).
// `args`: the fused launch's arguments (its keys buffer is refilled from pixel_face and consumed again).
struct FitPairArgs {
	const int* row_off;
	const int32_t* pairs;
	double* pair_acc;
	int wave_base;   // first of the workgroup's waves this launch runs (k_fit_pairs)
};
nnrt_status launch_fit_pairs(const FitPixelArgs& args, FitPairArgs pa, int M, hipStream_t stream);

// pair blocks of the system: float(pair_acc) + the ARAP wing blocks of the edges on the pair (transposed where the edge
// is stored (j, i))
nnrt_status launch_coupled_assemble(const double* pair_acc, int M, const int* edge_off, const int* edge_list, const float* wing,
                                    float* pair_blocks, hipStream_t stream);

// arap.hip: data accumulator + ARAP edge terms -> diagonal blocks (+ LM) and right-hand side (k_arrow_prepare alone);
// lm_device (nullable): the damping is read from this device word instead of `lm` (step control)
nnrt_status launch_arrow_prepare(int N, float lm, double* acc, const int* inc_off, const float* edge_terms, float* diag, float* rhs,
                                 float* gradient_out, float* hessian_out, hipStream_t stream, const float* lm_device = nullptr);

} // namespace nnrt
