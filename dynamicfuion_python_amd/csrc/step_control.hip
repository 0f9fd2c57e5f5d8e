// On-device step control of the fitter (step_control.hpp).
#include <cmath>

#include "step_control.hpp"

namespace nnrt {

__global__ void k_step_reset(StepState* st, float lambda) {
	st->c_best = 0.0;
	st->lambda = lambda;
	st->retry = 0;
	st->done = 0;
	st->iteration = 0;
	st->hold = 0;
	st->decision = NNRT_STEP_HOLD;
	st->saved_error = 0;
	st->ticket = 0u;
	st->cost = 0.0;
}

// Phase 1, every workgroup: the fp64 sum of its chunk of squared float residuals (masked pixels, then the ARAP edge
// residual entries), each thread its items in ascending order, the wave by a fixed shuffle tree, the workgroup's waves in
// wave order: partials[block]. Thread 0 then takes a ticket (agent-scope acquire-release: the partial it stored before is
// released with it). Phase 2, the workgroup that arrives last (its thread 0 has acquired every other partial): thread 0
// sums the partials in index order -- the same value whichever workgroup is last -- and takes the decision; the workgroup
// then copies the current motion into the best motion where the decision says so, one lane per float.
// Everything after a thread's own sum is step_cost_finish, which k_step_cost and k_step_cost_robust share.
__device__ __forceinline__ void step_cost_finish(const StepCostArgs& a, double sum) {
	__shared__ double s_wave[STEP_COST_THREADS / 64];
	__shared__ int s_last, s_copy;
	const int t = static_cast<int>(threadIdx.x);
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
	if ((t & 63) == 0) s_wave[t >> 6] = sum;
	__syncthreads();
	if (t == 0) {
		double block_sum = s_wave[0];
#pragma unroll
		for (int w = 1; w < STEP_COST_THREADS / 64; w++) block_sum += s_wave[w];
		a.partials[blockIdx.x] = block_sum;
		const unsigned arrived = __hip_atomic_fetch_add(&a.st->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
		s_last = arrived == static_cast<unsigned>(a.blocks) - 1u;
		s_copy = 0;
		if (s_last) {
			StepState* st = a.st;
			double c = 0.0;
			for (int b = 0; b < a.blocks; b++) c += a.partials[b];
			if (a.landmark_cost) c += *a.landmark_cost;   // the same in both objectives
			float lambda = st->lambda;
			double c_best = st->c_best;
			int done = st->done, retry = st->retry, hold, decision, copy = 0;
			if (done) {
				hold = 1;
				decision = NNRT_STEP_HOLD;
			} else if (st->iteration == 0 || retry) {
				c_best = c;
				copy = 1;
				retry = 0;
				hold = 0;
				decision = NNRT_STEP_START;
			} else if (c <= c_best) {
				copy = 1;
				if ((c_best - c) <= static_cast<double>(a.relative_cost_tolerance) * c_best) {
					done = 1;
					hold = 1;
					decision = NNRT_STEP_CONVERGED;
				} else {
					lambda = fmaxf(lambda * a.decrease, a.lambda_min);
					hold = 0;
					decision = NNRT_STEP_ACCEPT;
				}
				c_best = c;
			} else {   // a higher cost, or a cost that is not a number
				decision = NNRT_STEP_REJECT;
				if (lambda >= a.lambda_max) {
					done = 1;
					decision = NNRT_STEP_REJECT_FINAL;
				}
				lambda = fminf(lambda * a.increase, a.lambda_max);
				retry = 1;
				hold = 1;
			}
			st->c_best = c_best;
			st->cost = c;
			st->lambda = lambda;
			st->retry = retry;
			st->done = done;
			st->hold = hold;
			st->decision = decision;
			st->saved_error = *a.error_flag;
			__hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			s_copy = copy;
		}
	}
	__syncthreads();
	if (!s_last || !s_copy) return;
	const int64_t count = static_cast<int64_t>(a.N) * STEP_BEST_STRIDE;
	for (int64_t i = t; i < count; i += STEP_COST_THREADS) {
		const int64_t n = i / STEP_BEST_STRIDE;
		a.best[i] = a.state_in[n * NODE_STRIDE + 3 + (i - n * STEP_BEST_STRIDE)];
	}
}

__global__ __launch_bounds__(STEP_COST_THREADS) void k_step_cost(StepCostArgs a) {
	const int t = static_cast<int>(threadIdx.x);
	const int64_t base = static_cast<int64_t>(blockIdx.x) * a.chunk, items = a.P + a.E3;
	double sum = 0.0;
	for (int64_t k = 0; k < a.chunk; k += STEP_COST_THREADS) {
		const int64_t i = base + k + t;
		if (i < a.P) {
			if (a.residual_mask[i]) {
				const double r = static_cast<double>(a.residuals[i]);
				sum += r * r;
			}
		} else if (i < items) {
			const double r = static_cast<double>(a.edge_residuals[i - a.P]);
			sum += r * r;
		}
	}
	step_cost_finish(a, sum);
}

// The cost under NNRT_STEP_OBJECTIVE_ROBUST. Same structure as k_step_cost, one lane per item, the
// items being the P pixels and then the E edges. The fused pixel launch leaves the scaled residual s r behind, from which
// r cannot be recovered, so a masked pixel is resolved again from what the iteration has left on the device: the pixel's
// face (pixel_face), the warped mesh and the reference point, by pass 1's own resolve (resolve_face and resolve_distance
// in pixel_terms.hpp; -ffp-contract=off: the same IEEE operations give the same bits). r goes to raw[p] (0 outside the
// mask). Per pixel, in fp64: r^2, or with the IRLS Tukey penalty (c^2 / 3)(1 - (1 - q^2)^3),
// q = r / c, formed as (c^2 / 3) q^2 (3 + q^2 (q^2 - 3)) (no cancellation for small q), c^2 / 3 beyond the cutoff; NaN
// where r is not finite. Per edge: m^2 = the fp64 sum of squares of its three stored entries, or with the IRLS Huber
// penalty m^2 if m^2 <= delta^2 else 2 m^2 - delta^2 (the stored entries are sqrt(delta / n) e, so m^2 = delta n).
__global__ __launch_bounds__(STEP_COST_THREADS) void k_step_cost_robust(StepCostRobustArgs ra) {
	const StepCostArgs& a = ra.base;
	const int t = static_cast<int>(threadIdx.x);
	const int64_t base = static_cast<int64_t>(blockIdx.x) * a.chunk, items = a.P + ra.E;
	const double c = static_cast<double>(ra.tukey_c), c23 = c * c / 3.0;
	const double d2 = static_cast<double>(ra.huber_delta) * static_cast<double>(ra.huber_delta);
	double sum = 0.0;
	if (blockIdx.x == 0) {
		// A node motion that is not finite (Rodrigues' 0 / 0 without the zero-rotation guard) unrenders the faces it moves,
		// so their pixels leave the mask and no residual shows it: the cost of such a state is NaN, which rejects it
		const int64_t count = static_cast<int64_t>(a.N) * STEP_BEST_STRIDE;
		for (int64_t i = t; i < count; i += STEP_COST_THREADS) {
			const int64_t n = i / STEP_BEST_STRIDE;
			if (!(fabsf(a.state_in[n * NODE_STRIDE + 3 + (i - n * STEP_BEST_STRIDE)]) <= 3.402823466e+38f)) sum = NAN;
		}
	}
	for (int64_t k = 0; k < a.chunk; k += STEP_COST_THREADS) {
		const int64_t i = base + k + t;
		if (i < a.P) {
			float dist = 0.0f;
			const bool mask = a.residual_mask[i] != 0;
			const int32_t face = mask ? ra.pixel_face[i] : -1;
			if (face >= 0 && face < ra.F) {
				const int u = static_cast<int>(i % ra.W), v = static_cast<int>(i / ra.W);
				PixelResolve r = resolve_pixel(ra.view, u, v);
				if (resolve_face(ra.view, face, r)) {
					resolve_distance(ra.view, u, v, i, true, true, r);   // (the mask says that pass 1 found the depth valid)
					dist = r.dist;
				}
			}
			ra.raw[i] = dist;
			if (mask) {
				const double r = static_cast<double>(dist);
				double term = r * r;
				if (ra.use_tukey) {
					const double q = r / c, q2 = q * q;
					term = fabsf(dist) <= ra.tukey_c ? c23 * (q2 * (3.0 + q2 * (q2 - 3.0))) : c23;
				}
				if (!(fabsf(dist) <= 3.402823466e+38f)) term = NAN;   // not a saturated finite cost: the decision rejects it
				sum += term;
			}
		} else if (i < items) {
			const float* e = a.edge_residuals + 3 * (i - a.P);
			const double r0 = static_cast<double>(e[0]), r1 = static_cast<double>(e[1]), r2 = static_cast<double>(e[2]);
			const double m2 = (r0 * r0 + r1 * r1) + r2 * r2;
			sum += (!ra.use_huber || m2 <= d2) ? m2 : 2.0 * m2 - d2;
		}
	}
	step_cost_finish(a, sum);
}

// One workgroup, after the update. A held iteration: motion <- best motion, and the error word goes back to what it was
// at the decision. A stepping iteration: max |update| (an update that is not finite counts as +inf); below the threshold
// the best motion is put back and the fit is done. Then the iteration's history record.
__global__ __launch_bounds__(STEP_SELECT_THREADS) void k_step_select(StepSelectArgs a) {
	__shared__ float s_max[STEP_SELECT_THREADS / 64];
	__shared__ int s_restore;
	const int t = static_cast<int>(threadIdx.x);
	StepState* st = a.st;
	const int hold = st->hold;
	float m = 0.f;
	if (!hold) {
		for (int i = t; i < 6 * a.N; i += STEP_SELECT_THREADS) {
			float u = fabsf(a.updates[i]);
			if (!(u <= 3.402823466e+38f)) u = INFINITY;
			m = fmaxf(m, u);
		}
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
		if ((t & 63) == 0) s_max[t >> 6] = m;
	}
	__syncthreads();
	if (t == 0) {
		int decision = st->decision;
		int restore = hold;
		if (hold) {
			*a.error_flag = st->saved_error;
		} else {
			m = s_max[0];
			for (int w = 1; w < STEP_SELECT_THREADS / 64; w++) m = fmaxf(m, s_max[w]);
			if (m < a.minimal_update_threshold) {
				st->done = 1;
				decision = NNRT_STEP_SMALL_UPDATE;
				restore = 1;
			}
		}
		const int it = st->iteration;
		nnrt_step_record rec;
		rec.cost = st->cost;
		rec.lambda = st->lambda;
		rec.max_update = m;
		rec.decision = decision;
		rec.iteration = it;
		a.history[it % NNRT_STEP_HISTORY_CAPACITY] = rec;
		st->iteration = it + 1;
		s_restore = restore;
	}
	__syncthreads();
	if (!s_restore) return;
	const int64_t count = static_cast<int64_t>(a.N) * STEP_BEST_STRIDE;
	for (int64_t i = t; i < count; i += STEP_SELECT_THREADS) {
		const int64_t n = i / STEP_BEST_STRIDE;
		a.node_state[n * NODE_STRIDE + 3 + (i - n * STEP_BEST_STRIDE)] = a.best[i];
	}
}

nnrt_status launch_step_reset(StepState* st, float lambda, hipStream_t stream) {
	k_step_reset<<<1, 1, 0, stream>>>(st, lambda);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_step_cost(const StepCostArgs& args, hipStream_t stream) {
	k_step_cost<<<static_cast<unsigned>(args.blocks), STEP_COST_THREADS, 0, stream>>>(args);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_step_cost_robust(const StepCostRobustArgs& args, hipStream_t stream) {
	k_step_cost_robust<<<static_cast<unsigned>(args.base.blocks), STEP_COST_THREADS, 0, stream>>>(args);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_step_select(const StepSelectArgs& args, hipStream_t stream) {
	k_step_select<<<1, STEP_SELECT_THREADS, 0, stream>>>(args);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
