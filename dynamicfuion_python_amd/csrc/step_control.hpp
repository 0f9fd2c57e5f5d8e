// The fitter's on-device step control (nnrt_fitter_set_step_control): the state machine's device
// state and the two launches an iteration gains -- k_step_cost between the fused pixel launch and the solve (total cost,
// accept / reject, the damping the solve reads) and k_step_select after the update (keep the step or put the best motion
// back, the history record). Under NNRT_STEP_OBJECTIVE_ROBUST k_step_cost_robust takes k_step_cost's
// place: the same tail, the robust cost of the raw residuals it resolves again.
#pragma once

#include "pixel_terms.hpp"

namespace nnrt {

constexpr int STEP_COST_THREADS = 256;        // workgroup of k_step_cost
constexpr int STEP_COST_ITEMS = 16;           // residuals per thread before another workgroup is added
constexpr int STEP_COST_MAX_BLOCKS = 256;     // workgroups (= partial sums) at most: larger images give each thread more
constexpr int STEP_SELECT_THREADS = 1024;     // the one workgroup of k_step_select
constexpr int STEP_BEST_STRIDE = 12;          // best motion per node: t (3), R (9)

struct StepState {   // one per fitter, on the device
	double c_best;
	float lambda;        // the damping the solve launches read
	int retry;           // the last decision rejected: the next iteration restarts from the restored best state
	int done;
	int iteration;       // since the restart
	int hold;            // this iteration's decision: 1 = the update is discarded
	int decision;        // NNRT_STEP_* of this iteration
	int saved_error;     // the fitter's error word at the decision (a held iteration puts it back)
	unsigned ticket;     // k_step_cost's arrivals (back to 0 when the launch ends)
	double cost;         // this iteration's cost
};

struct StepCostArgs {
	int64_t P;                     // pixels
	int64_t E3;                    // ARAP edge residual entries (3 E; 0 without a hierarchy)
	int N;
	int blocks;                    // the launch's workgroups
	int64_t chunk;                 // items per workgroup (a multiple of STEP_COST_THREADS)
	const float* residuals;        // [P]
	const uint8_t* residual_mask;  // [P]
	const float* edge_residuals;   // [E3]
	const float* state_in;         // [N,16] the motion the iteration started from
	float* best;                   // [N,12]
	double* partials;              // [blocks]
	StepState* st;
	const int* error_flag;
	float increase, decrease, lambda_min, lambda_max, relative_cost_tolerance;
	const double* landmark_cost;   // the landmark term's cost of the same state (k_fit_landmarks; null: no landmarks set)
};

// k_step_cost_robust (NNRT_STEP_OBJECTIVE_ROBUST): base.blocks / base.chunk are those of P + E items
// (one per pixel, one per edge); base.residuals is not read
struct StepCostRobustArgs {
	StepCostArgs base;
	PixelResolveView view;         // what the resolve reads, as the fused pixel launch received it
	int64_t F;                     // faces (pixel_face is checked against it)
	int E;                         // ARAP edges
	int W;
	int use_tukey, use_huber;      // 1: the IRLS form of the penalty is on
	float tukey_c, huber_delta;
	const int32_t* pixel_face;     // [P] the face pass 1 resolved (-1: none)
	float* raw;                    // [P] out: the raw point-to-plane distance (0 outside the mask)
};

struct StepSelectArgs {
	int N;
	const float* updates;          // [6N]
	float* node_state;             // [N,16] the motion the update wrote
	const float* best;             // [N,12]
	StepState* st;
	nnrt_step_record* history;     // [NNRT_STEP_HISTORY_CAPACITY]
	int* error_flag;
	float minimal_update_threshold;
};

// workgroups of k_step_cost for `items` = P + E3 values, and the items each takes
inline int step_cost_blocks(int64_t items) {
	const int64_t b = ceil_div(items, static_cast<int64_t>(STEP_COST_THREADS) * STEP_COST_ITEMS);
	return static_cast<int>(b < 1 ? 1 : b > STEP_COST_MAX_BLOCKS ? STEP_COST_MAX_BLOCKS : b);
}
inline int64_t step_cost_chunk(int64_t items, int blocks) { return ceil_div(ceil_div(items, blocks), STEP_COST_THREADS) * STEP_COST_THREADS; }

nnrt_status launch_step_reset(StepState* st, float lambda, hipStream_t stream);
nnrt_status launch_step_cost(const StepCostArgs& args, hipStream_t stream);
nnrt_status launch_step_cost_robust(const StepCostRobustArgs& args, hipStream_t stream);
nnrt_status launch_step_select(const StepSelectArgs& args, hipStream_t stream);

} // namespace nnrt
