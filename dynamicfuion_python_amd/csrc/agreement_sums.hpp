// Reproducible agreement statistics of two images (DESIGN.md sections 22 and 32): the sums a lane keeps over its pixels
// and the workgroup's reduction of them, shared by k_depth_agreement (shading.hip) and k_flow_error (motion.hip). A
// wavefront reduces by a fixed shuffle tree (offsets 32, 16, ..., 1), thread 0 of the workgroup adds the wavefronts in
// wavefront order. No atomics, so the same input gives the same bits run to run.
#pragma once
#include <hip/hip_runtime.h>

namespace nnrt {

struct AgreementSums {
	long long both, first_only, second_only, inliers;   // pixels valid on both sides, on one side only; of `both`, within the threshold
	double sum, sum_sq;                                  // of the per-pixel magnitude, over `both`
	float max;

	__device__ void add(const AgreementSums& o) {
		both += o.both;
		first_only += o.first_only;
		second_only += o.second_only;
		inliers += o.inliers;
		sum = sum + o.sum;
		sum_sq = sum_sq + o.sum_sq;
		max = fmaxf(max, o.max);
	}
};

__device__ inline AgreementSums shuffled_down(const AgreementSums& s, int offset) {
	AgreementSums o;
	o.both = __shfl_down(s.both, offset, 64);
	o.first_only = __shfl_down(s.first_only, offset, 64);
	o.second_only = __shfl_down(s.second_only, offset, 64);
	o.inliers = __shfl_down(s.inliers, offset, 64);
	o.sum = __shfl_down(s.sum, offset, 64);
	o.sum_sq = __shfl_down(s.sum_sq, offset, 64);
	o.max = __shfl_down(s.max, offset, 64);
	return o;
}

// lane 0 of a wavefront ends with the wavefront's sums
__device__ inline void reduce_wavefront(AgreementSums& sums) {
	for (int offset = 32; offset >= 1; offset >>= 1) sums.add(shuffled_down(sums, offset));
}

// Every thread of a workgroup of WAVES wavefronts calls this with its own sums; true for thread 0, whose `sums` are then
// the workgroup's. s_waves: WAVES entries of LDS. (k_depth_agreement keeps the same steps written out in its body: through
// this function the compiler allocates its registers differently, and its code is to stay what it was.)
template <int WAVES>
__device__ inline bool reduce_workgroup(AgreementSums& sums, AgreementSums* s_waves) {
	const int t = static_cast<int>(threadIdx.x);
	reduce_wavefront(sums);
	if ((t & 63) == 0) s_waves[t >> 6] = sums;
	__syncthreads();
	if (t != 0) return false;
	for (int w = 1; w < WAVES; w++) sums.add(s_waves[w]);
	return true;
}

} // namespace nnrt
