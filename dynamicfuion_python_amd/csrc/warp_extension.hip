// Extending the warp field over newly fused surface (DynamicFusion, Newcombe et al. 2015, section 3.4): the two per-frame
// kernels around the node sampler (graph_sampling.hip).
//   * k_vertex_support: for every canonical vertex the nearest node and the support ratio d_min / c. Vertices whose ratio
//     exceeds a threshold are the candidates new nodes are sampled from.
//   * k_blend_node_transforms: the current warp evaluated at the new nodes' own positions -- translation and the rotation
//     nearest to the weighted rotation average -- so that a new node starts where the field already moves its surroundings.
// Squared distances are ((dx*dx + dy*dy) + dz*dz) with d = node - point in unfused f32, the expression of
// k_compute_anchors (geometry.hip): the nearest node agrees with that kernel's slot 0. Both kernels are deterministic: no
// atomics, one lane owns every output it writes.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {
constexpr int SUPPORT_BLOCK = 256;   // lanes per workgroup = nodes per LDS tile
constexpr int BLEND_BLOCK = 64;

// One lane per vertex. The nodes pass through LDS in tiles of SUPPORT_BLOCK (x, y, z, 1 / coverage weight): every lane
// of a wave reads the same tile entry (a broadcast read, no bank conflict). Strict '<' in ascending node order: the
// lowest index wins ties. VARIABLE: the key is sq * RN(1 / w_j) with w_j the node's squared coverage weight, and the
// ratio its square root; else the key is sq and the ratio sqrtf(sq) / coverage. sqrtf and the divisions are correctly
// rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so a float32 host restatement is bit-identical.
template <bool VARIABLE>
__global__ __launch_bounds__(SUPPORT_BLOCK) void k_vertex_support(const float* __restrict__ points, int64_t point_count,
                                                                   const float* __restrict__ nodes, int node_count, float coverage,
                                                                   const float* __restrict__ node_weights, float* __restrict__ ratio,
                                                                   int32_t* __restrict__ nearest) {
	__shared__ float4 tile[SUPPORT_BLOCK];
	const int64_t i = static_cast<int64_t>(blockIdx.x) * SUPPORT_BLOCK + threadIdx.x;
	const bool active = i < point_count;
	float px = 0.f, py = 0.f, pz = 0.f;
	if (active) {
		px = points[3 * i];
		py = points[3 * i + 1];
		pz = points[3 * i + 2];
	}
	float best = INFINITY;
	int best_at = -1;
	for (int base = 0; base < node_count; base += SUPPORT_BLOCK) {
		const int64_t j = static_cast<int64_t>(base) + threadIdx.x;
		if (j < node_count) tile[threadIdx.x] = make_float4(nodes[3 * j], nodes[3 * j + 1], nodes[3 * j + 2], VARIABLE ? 1.0f / node_weights[j] : 1.0f);
		__syncthreads();
		const int count = min(SUPPORT_BLOCK, node_count - base);
#pragma unroll 8
		for (int q = 0; q < count; q++) {
			const float4 g = tile[q];
			const float dx = g.x - px, dy = g.y - py, dz = g.z - pz;
			float key = (dx * dx + dy * dy) + dz * dz;
			if (VARIABLE) key = key * g.w;
			if (key < best) {
				best = key;
				best_at = base + q;
			}
		}
		__syncthreads();   // the tile is overwritten by the next pass
	}
	if (!active) return;
	// a vertex with a non-finite coordinate is never a candidate (the sampler skips it): ratio 0, no node
	const bool finite = isfinite(px) && isfinite(py) && isfinite(pz);
	ratio[i] = finite ? (VARIABLE ? sqrtf(best) : sqrtf(best) / coverage) : 0.f;
	nearest[i] = finite ? best_at : -1;
}

constexpr int EMPTY_SLOT = 0x7fffffff;
constexpr int POLAR_ITERATIONS = 20;
constexpr float POLAR_MIN_DETERMINANT = 1e-3f;
constexpr float POLAR_ORTHOGONALITY_TOLERANCE = 1e-5f;

// cofactor matrix C of X (X^-T = C / det X) and det X
__device__ inline float cofactors3(const float* X, float* C) {
	C[0] = X[4] * X[8] - X[5] * X[7];
	C[1] = X[5] * X[6] - X[3] * X[8];
	C[2] = X[3] * X[7] - X[4] * X[6];
	C[3] = X[2] * X[7] - X[1] * X[8];
	C[4] = X[0] * X[8] - X[2] * X[6];
	C[5] = X[1] * X[6] - X[0] * X[7];
	C[6] = X[1] * X[5] - X[2] * X[4];
	C[7] = X[2] * X[3] - X[0] * X[5];
	C[8] = X[0] * X[4] - X[1] * X[3];
	return (X[0] * C[0] + X[1] * C[1]) + X[2] * C[2];
}

// One lane per query point. The MAX_ANCHORS nearest nodes are kept sorted by (squared distance, index) while the nodes
// are scanned in ascending index (node addresses are wave-uniform); the first min(K, N) slots are blended, in slot order, f32:
//   w_k = exp(-(d_k^2 - d_0^2) / (2 c^2)) / sum   -- exp(-d_k^2 / (2 c^2)) normalised, with the common factor exp(-d_0^2 / (2 c^2))
//                                                  taken out so that the nearest node's weight never underflows
//   t   = sum_k w_k ((R_k d_k - d_k) + t_k), d_k = p - g_k   -- equal to sum_k w_k (g_k + R_k d_k + t_k) - p for weights that
//                                                  sum to one, without the cancellation against p: identity motion gives exactly 0
//   R   = the orthogonal polar factor of B = sum_k w_k R_k by POLAR_ITERATIONS Newton steps X <- (X + X^-T) / 2 (Higham),
//         which keep the sign of det X: det R > 0. det B <= POLAR_MIN_DETERMINANT (the singular values of B are at most 1,
//         so each is above that bound otherwise and the fixed count converges) or max |R^T R - I| >
//         POLAR_ORTHOGONALITY_TOLERANCE: the nearest node's rotation, and fallback[i] = 1.
__global__ __launch_bounds__(BLEND_BLOCK) void k_blend_node_transforms(const float* __restrict__ points, int64_t point_count,
                                                                        const float* __restrict__ nodes, const float* __restrict__ rotations,
                                                                        const float* __restrict__ translations, int node_count, int K,
                                                                        float coverage_squared, float* __restrict__ out_rotations,
                                                                        float* __restrict__ out_translations, uint8_t* __restrict__ fallback) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * BLEND_BLOCK + threadIdx.x;
	const bool active = i < point_count;
	float px = 0.f, py = 0.f, pz = 0.f;
	if (active) {
		px = points[3 * i];
		py = points[3 * i + 1];
		pz = points[3 * i + 2];
	}
	float d2[MAX_ANCHORS];
	int idx[MAX_ANCHORS];
#pragma unroll
	for (int k = 0; k < MAX_ANCHORS; k++) {
		d2[k] = INFINITY;
		idx[k] = EMPTY_SLOT;
	}
	for (int j = 0; j < node_count; j++) {
		const float dx = nodes[3 * static_cast<int64_t>(j)] - px, dy = nodes[3 * static_cast<int64_t>(j) + 1] - py,
		            dz = nodes[3 * static_cast<int64_t>(j) + 2] - pz;
		float cd = (dx * dx + dy * dy) + dz * dz;
		int cj = j;
		if (!(cd < d2[MAX_ANCHORS - 1])) continue;   // also a NaN distance
		// insertion by carrying the displaced entry upwards (static register indices)
#pragma unroll
		for (int k = 0; k < MAX_ANCHORS; k++) {
			if (cd < d2[k] || (cd == d2[k] && cj < idx[k])) {
				const float sd = d2[k];
				const int sj = idx[k];
				d2[k] = cd;
				idx[k] = cj;
				cd = sd;
				cj = sj;
			}
		}
	}
	if (!active) return;
	float B[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, R0[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
	float w[MAX_ANCHORS];
	float sum = 0.f;
#pragma unroll
	for (int k = 0; k < MAX_ANCHORS; k++) {
		w[k] = 0.f;
		if (k < K && idx[k] != EMPTY_SLOT) {
			w[k] = exp_cr(-(d2[k] - d2[0]) / (2 * coverage_squared));
			sum += w[k];
		}
	}
	float tx = 0.f, ty = 0.f, tz = 0.f;
#pragma unroll
	for (int k = 0; k < MAX_ANCHORS; k++) {
		if (k < K && idx[k] != EMPTY_SLOT) {
			const int64_t n = idx[k];
			const float wk = w[k] / sum;   // slot 0 has weight exp(0) = 1: sum >= 1
			float R[9];
#pragma unroll
			for (int e = 0; e < 9; e++) {
				R[e] = rotations[9 * n + e];
				B[e] += wk * R[e];
				if (k == 0) R0[e] = R[e];
			}
			const f3 d = make3(px - nodes[3 * n], py - nodes[3 * n + 1], pz - nodes[3 * n + 2]);
			const f3 Rd = matvec3(R, d);
			tx += wk * ((Rd.x - d.x) + translations[3 * n]);
			ty += wk * ((Rd.y - d.y) + translations[3 * n + 1]);
			tz += wk * ((Rd.z - d.z) + translations[3 * n + 2]);
		}
	}
	float X[9], C[9];
#pragma unroll
	for (int e = 0; e < 9; e++) X[e] = B[e];
	bool ok = cofactors3(X, C) > POLAR_MIN_DETERMINANT;   // false for NaN
	if (ok) {
#pragma unroll 1
		for (int it = 0; it < POLAR_ITERATIONS; it++) {
			const float det = cofactors3(X, C);
#pragma unroll
			for (int e = 0; e < 9; e++) X[e] = 0.5f * (X[e] + C[e] / det);
		}
		float worst = 0.f;
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int b = 0; b < 3; b++) {
				const float g = (X[a] * X[b] + X[3 + a] * X[3 + b]) + X[6 + a] * X[6 + b];
				worst = fmaxf(worst, fabsf(g - (a == b ? 1.f : 0.f)));
				if (!isfinite(g)) ok = false;
			}
		if (!(worst <= POLAR_ORTHOGONALITY_TOLERANCE)) ok = false;
	}
#pragma unroll
	for (int e = 0; e < 9; e++) out_rotations[9 * i + e] = ok ? X[e] : R0[e];
	out_translations[3 * i] = tx;
	out_translations[3 * i + 1] = ty;
	out_translations[3 * i + 2] = tz;
	fallback[i] = ok ? 0 : 1;
}
} // namespace

nnrt_status launch_vertex_support(const float* points, int64_t V, const float* nodes, int N, float coverage, const float* node_weights,
                                  float* ratio, int32_t* nearest, hipStream_t s) {
	if (V == 0) return NNRT_OK;
	const dim3 grid(static_cast<unsigned>(ceil_div(V, SUPPORT_BLOCK)));
	if (node_weights) k_vertex_support<true><<<grid, SUPPORT_BLOCK, 0, s>>>(points, V, nodes, N, coverage, node_weights, ratio, nearest);
	else k_vertex_support<false><<<grid, SUPPORT_BLOCK, 0, s>>>(points, V, nodes, N, coverage, nullptr, ratio, nearest);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_blend_node_transforms(const float* points, int64_t M, const float* nodes, const float* rotations, const float* translations,
                                         int N, int K, float coverage, float* out_rotations, float* out_translations, uint8_t* fallback,
                                         int64_t* h_fallback_count, hipStream_t s) {
	if (h_fallback_count) *h_fallback_count = 0;
	if (M == 0) return NNRT_OK;
	k_blend_node_transforms<<<static_cast<unsigned>(ceil_div(M, BLEND_BLOCK)), BLEND_BLOCK, 0, s>>>(
	    points, M, nodes, rotations, translations, N, K, coverage * coverage, out_rotations, out_translations, fallback);
	NNRT_LAUNCH_CHECK();
	if (h_fallback_count) {
		std::vector<uint8_t> flags(static_cast<size_t>(M));
		NNRT_HIP(hipMemcpyAsync(flags.data(), fallback, flags.size(), hipMemcpyDeviceToHost, s));
		NNRT_HIP(hipStreamSynchronize(s));
		int64_t count = 0;
		for (const uint8_t f : flags) count += f;
		*h_fallback_count = count;
	}
	return NNRT_OK;
}

} // namespace nnrt
