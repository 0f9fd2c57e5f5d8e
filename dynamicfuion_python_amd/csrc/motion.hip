// The motion field of a mesh between two states, as images on the source state's pixel grid, and a flow image scored
// against another.
//
// k_motion_pixels: one lane per pixel, pixels of a row on consecutive lanes; only the front fragment (slot 0 of the K slots
// of a pixel) is read. With face f >= 0, vertices (i0, i1, i2) and barycentrics b, p_s = (b0 S[i0] + b1 S[i1]) + b2 S[i2]
// over the source positions S, p_t the same blend of the target positions T, scene flow p_t - p_s and optical flow
// pi(p_t) - pi(p_s) with pi(p) = ((fx x) / z + cx, (fy y) / z + cy). A pixel is valid iff f >= 0, p_s.z > 0 and p_t.z > 0
// (false for NaN); every other pixel gets zeros and mask 0, so no output needs a zero fill. A face index >= face_count or
// a vertex index outside [0, vertex_count) is treated as background instead of being read through.
//
// k_flow_error + k_flow_error_finish: the end-point error of a predicted flow image against a truth image over the pixels
// valid on both sides, one lane per pixel, and its statistics. The sums are reproducible: agreement_sums.hpp reduces a
// workgroup to one record, and the finish launch, one wavefront, has lane l add records l, l + 64, ... in ascending order
// before the same shuffle tree. No atomics, no workgroup waits on another.
//
// Float arithmetic is unfused and in the order written (the build's -ffp-contract=off; the pragmas keep it so), float32
// divides are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so a float32 restatement of the blends
// equals the kernel bit for bit.
#include "agreement_sums.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {

constexpr int SB = 256;   // threads per workgroup, as in shading.hip

struct MotionArguments {
	const int64_t* pixel_faces;   // [P, K]
	const float* barycentrics;    // [P, K, 3]
	const int64_t* triangles;     // [F, 3]
	const float* source;          // [V, 3], source camera space
	const float* target;          // [V, 3], target camera space
	int64_t pixel_count;
	int64_t face_count;
	int64_t vertex_count;
	int K;
	float fx, fy, cx, cy;
};

__global__ void __launch_bounds__(SB) k_motion_pixels(MotionArguments a, float* __restrict__ source_points, float* __restrict__ scene_flow,
                                                      float* __restrict__ optical_flow, uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
	const int64_t p = static_cast<int64_t>(blockIdx.x) * SB + threadIdx.x;
	if (p >= a.pixel_count) return;
	const int64_t fragment = p * a.K;
	const int64_t face = a.pixel_faces[fragment];
	float ps[3] = {0.f, 0.f, 0.f}, flow[3] = {0.f, 0.f, 0.f};
	float du = 0.f, dv = 0.f;
	uint8_t valid = 0;
	if (face >= 0 && face < a.face_count) {
		const int64_t i0 = a.triangles[3 * face], i1 = a.triangles[3 * face + 1], i2 = a.triangles[3 * face + 2];
		const bool inside = i0 >= 0 && i0 < a.vertex_count && i1 >= 0 && i1 < a.vertex_count && i2 >= 0 && i2 < a.vertex_count;
		if (inside) {
			const float b0 = a.barycentrics[3 * fragment], b1 = a.barycentrics[3 * fragment + 1], b2 = a.barycentrics[3 * fragment + 2];
			float s[3], t[3];
#pragma unroll
			for (int c = 0; c < 3; c++) {
				s[c] = (b0 * a.source[3 * i0 + c] + b1 * a.source[3 * i1 + c]) + b2 * a.source[3 * i2 + c];
				t[c] = (b0 * a.target[3 * i0 + c] + b1 * a.target[3 * i1 + c]) + b2 * a.target[3 * i2 + c];
			}
			if (s[2] > 0.f && t[2] > 0.f) {   // false for NaN
				valid = 1;
#pragma unroll
				for (int c = 0; c < 3; c++) {
					ps[c] = s[c];
					flow[c] = t[c] - s[c];
				}
				const float us = (a.fx * s[0]) / s[2] + a.cx, vs = (a.fy * s[1]) / s[2] + a.cy;
				const float ut = (a.fx * t[0]) / t[2] + a.cx, vt = (a.fy * t[1]) / t[2] + a.cy;
				du = ut - us;
				dv = vt - vs;
			}
		}
	}
#pragma unroll
	for (int c = 0; c < 3; c++) {
		source_points[3 * p + c] = ps[c];
		scene_flow[3 * p + c] = flow[c];
	}
	optical_flow[2 * p] = du;
	optical_flow[2 * p + 1] = dv;
	mask[p] = valid;
}

// ------------------------------------------------------------------------------------------------------ flow error ----
__device__ inline void store_record(nnrt_flow_agreement* record, const AgreementSums& s) {
	record->both = s.both;
	record->predicted_only = s.first_only;
	record->truth_only = s.second_only;
	record->inliers = s.inliers;
	record->sum_epe = s.sum;
	record->sum_sq = s.sum_sq;
	record->max_epe = s.max;
	record->reserved = 0;
}

// truth_mask may be null: every pixel with finite channels is then valid truth
template <int C>
__global__ void __launch_bounds__(SB) k_flow_error(const float* __restrict__ predicted, const uint8_t* __restrict__ predicted_mask,
                                                   const float* __restrict__ truth, const uint8_t* __restrict__ truth_mask, int64_t pixel_count,
                                                   float inlier_threshold, float* __restrict__ error, nnrt_flow_agreement* __restrict__ partials) {
#pragma clang fp contract(off)
	__shared__ AgreementSums s_waves[SB / 64];
	AgreementSums sums{0, 0, 0, 0, 0.0, 0.0, 0.f};
	const int64_t p = static_cast<int64_t>(blockIdx.x) * SB + threadIdx.x;
	if (p < pixel_count) {   // no early return: every thread reaches the workgroup's reduction
		float g[C];
		bool known = truth_mask == nullptr || truth_mask[p] != 0;
#pragma unroll
		for (int c = 0; c < C; c++) {
			g[c] = truth[C * p + c];
			known = known && fabsf(g[c]) <= 3.402823466e+38f;   // finite: false for NaN and the infinities
		}
		const bool drawn = predicted_mask[p] != 0;
		float e32 = __builtin_nanf("");
		if (drawn && known) {
			double squares = 0.0;
#pragma unroll
			for (int c = 0; c < C; c++) {
				const double d = static_cast<double>(predicted[C * p + c] - g[c]);   // the float32 difference, widened
				squares = squares + d * d;
			}
			const double e = sqrt(squares);
			e32 = static_cast<float>(e);
			sums.both = 1;
			sums.inliers = e <= static_cast<double>(inlier_threshold) ? 1 : 0;
			sums.sum = e;
			sums.sum_sq = e * e;
			sums.max = e32;
		} else if (drawn) {
			sums.first_only = 1;
		} else if (known) {
			sums.second_only = 1;
		}
		error[p] = e32;
	}
	if (reduce_workgroup<SB / 64>(sums, s_waves)) store_record(partials + blockIdx.x, sums);
}

// one wavefront: lane l adds records l, l + 64, ... in ascending order, then the shuffle tree
__global__ void __launch_bounds__(64) k_flow_error_finish(const nnrt_flow_agreement* __restrict__ partials, int count,
                                                          nnrt_flow_agreement* __restrict__ result) {
#pragma clang fp contract(off)
	if (blockIdx.x != 0) return;
	AgreementSums sums{0, 0, 0, 0, 0.0, 0.0, 0.f};
	for (int i = static_cast<int>(threadIdx.x); i < count; i += 64) {
		const nnrt_flow_agreement r = partials[i];
		sums.add(AgreementSums{r.both, r.predicted_only, r.truth_only, r.inliers, r.sum_epe, r.sum_sq, r.max_epe});
	}
	reduce_wavefront(sums);
	if (threadIdx.x == 0) store_record(result, sums);
}

} // namespace

nnrt_status launch_motion_pixels(const int64_t* pixel_faces, const float* barycentrics, int H, int W, int K, const int64_t* triangles,
                                 int64_t face_count, const float* source, const float* target, int64_t vertex_count, float fx, float fy, float cx,
                                 float cy, float* source_points, float* scene_flow, float* optical_flow, uint8_t* mask, hipStream_t stream) {
	const int64_t P = static_cast<int64_t>(H) * W;
	if (P == 0) return NNRT_OK;
	MotionArguments a{pixel_faces, barycentrics, triangles, source, target, P, face_count, vertex_count, K, fx, fy, cx, cy};
	k_motion_pixels<<<static_cast<unsigned>(ceil_div(P, SB)), SB, 0, stream>>>(a, source_points, scene_flow, optical_flow, mask);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

int64_t flow_error_partial_count(int H, int W) { return ceil_div(static_cast<int64_t>(H) * W, SB); }

nnrt_status launch_flow_error(const float* predicted, const uint8_t* predicted_mask, const float* truth, const uint8_t* truth_mask, int H, int W,
                              int C, float inlier_threshold, float* error, nnrt_flow_agreement* partials, nnrt_flow_agreement* result,
                              hipStream_t stream) {
	const int64_t P = static_cast<int64_t>(H) * W;
	const int64_t groups = flow_error_partial_count(H, W);
	const unsigned grid = static_cast<unsigned>(groups);
	if (C == 2)
		k_flow_error<2><<<grid, SB, 0, stream>>>(predicted, predicted_mask, truth, truth_mask, P, inlier_threshold, error, partials);
	else
		k_flow_error<3><<<grid, SB, 0, stream>>>(predicted, predicted_mask, truth, truth_mask, P, inlier_threshold, error, partials);
	NNRT_LAUNCH_CHECK();
	k_flow_error_finish<<<1, 64, 0, stream>>>(partials, static_cast<int>(groups), result);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
