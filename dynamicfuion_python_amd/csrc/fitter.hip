// The fitter: host orchestration of FitToImage and its C-ABI (include/nnrt_mi355x.h, nnrt_fitter_*).
//
// FitToImage (cpp/alignment/DeformableMeshToImageFitter.cpp:85-276) as a static-shape loop: every buffer is sized at
// prepare() time, nothing in the iteration synchronizes with the host or allocates, so one GN iteration per iteration
// mode is captured into a hipGraph and replayed (the reference's per-stage host syncs: SURVEY.md section 3 CS-1).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "coupled.hpp"
#include "handles.hpp"
#include "landmarks.hpp"
#include "step_control.hpp"

using namespace nnrt;

// =====================================================================================================================
// fitter
// =====================================================================================================================
// Everything a captured graph bakes into its kernel arguments that is not a buffer address: the frame's sizes, the warp
// field (recognised by its unique id, not its address alone), the per-frame constants and the launch choices.
// prepare_frame builds one per frame and compares it bytewise with the last: no padding (checked below), and built
// in zeroed storage.
struct FrameKey {
	int64_t V, F;
	const nnrt_warp_field* wf;
	uint64_t wf_id;               // id of the warp field whose buffers the cached graphs captured
	uint64_t corner_generation;   // CornerSolver::generation: the corner's plan and buffers
	uint64_t pair_generation;     // the coupled data term's solver plan (0: block-diagonal data term)
	int H, W, N, K;
	int E, n0;                    // the warp field's edges and first-layer nodes (the ARAP terms' launch arguments)
	int quad_slots;              // the pixel launch's wave slots at four waves per SIMD (launch_quad_order's overflow bound)
	int coupled, M;              // nnrt_fitter_set_data_coupling at prepare(), and the frame's node pairs (coupled only)
	NdcSetup ndc;
	Camera pix;
	WarpExtrinsics extr;
	LaunchChoices launch;
};
static_assert(std::is_trivially_copyable<FrameKey>::value &&
                  sizeof(FrameKey) == 2 * sizeof(int64_t) + sizeof(void*) + 3 * sizeof(uint64_t) + 9 * sizeof(int) + sizeof(NdcSetup) +
                                          sizeof(Camera) + sizeof(WarpExtrinsics) + sizeof(LaunchChoices),
              "FrameKey is compared with memcmp: no padding");

struct nnrt_fitter {
	nnrt_fitter_params p{};
	int device = 0;
	hipStream_t work = nullptr;
	hipEvent_t ev_in = nullptr, ev_out = nullptr;
	bool prepared = false;
	FrameKey key{};   // of the last prepared frame
	// buffers
	DeviceBuffer<float> mesh_p, mesh_n;
	DeviceBuffer<int4> faces4;
	DeviceBuffer<int32_t> anchors;
	DeviceBuffer<uint2> anchors16;   // [V] the anchors as 4 x 16 bits (K = 4, N < 65535): the vertex warp's loads
	DeviceBuffer<float> weights;
	DeviceBuffer<uint32_t> face_nodes;   // [F, face_node_slots(K)] distinct anchor nodes per face (once per frame)
	DeviceBuffer<float4> wpos, wnrm;
	DeviceBuffer<float2> jrows;        // [V,K,3] warped-Jacobian rows (store_jacobian_row; NNRT_GATHER_ROWS builds only)
	DeviceBuffer<float4> mesh_p4, mesh_n4;   // [V] canonical positions / normals as float4 (pass 2 forms the Jacobian rows)
	DeviceBuffer<float4> ref_points;   // [P] reference point (x, y, z, valid)
	DeviceBuffer<int> tile_flags, tile_order;   // the pixel launch's per-frame workgroup -> tile table (launch_tile_order)
	DeviceBuffer<int> quad_scratch, quad_order;   // the same per 8 x 8 quadrant, one entry per wave (launch_quad_order)
	DeviceBuffer<float4> records;      // [P, 4] pixel Jacobian records
	DeviceBuffer<uint64_t> keys;
	DeviceBuffer<float> residuals;
	DeviceBuffer<uint8_t> residual_mask;
	DeviceBuffer<int32_t> pixel_face;
	DeviceBuffer<double> acc;       // [N, ACC_STRIDE] data term (fp64)
	DeviceBuffer<float> edge_jr;   // [E,8] ARAP edge Jacobian + residual
	DeviceBuffer<float> updates, gradient, hessian;
	DeviceBuffer<int> error_flag;
	// ARAP / arrowhead
	DeviceBuffer<float> wing, edge_residuals;
	ArrowheadStructure arap;   // what the solve derives from the hierarchy's edges, the Schur corner's plan and storage included
	DeviceBuffer<float> a_diag, a_rhs, a_x, a_res, a_dx;   // the solve's vectors (the coupled mode's too)
	float refine_ratio = NNRT_REFINE_PIVOT_RATIO;   // refinement gate threshold (nnrt_fitter_set_refine_ratio)
	float refine_ratio_used = NNRT_REFINE_PIVOT_RATIO;   // the threshold the last launched iterations ran with (refine_info)
	// nnrt_fitter_set_robust_options: the form the Tukey / Huber penalties take where the parameters enable them, and
	// whether a node update of rotation angle exactly 0 keeps the rotation (launch arguments of every iteration)
	int32_t penalty_form = NNRT_PENALTY_REFERENCE;
	int32_t guard_zero_rotation = 0;
	// nnrt_fitter_set_data_coupling: NNRT_DATA_COUPLED adds the data term's off-diagonal blocks. The
	// pair structure, the solver plan over it (arrow base 0: every node in the corner) and the workspace are per frame.
	int32_t data_coupling = NNRT_DATA_BLOCK_DIAGONAL;
	PairStructure ps;
	CornerSolver pair_corner;
	DeviceBuffer<double> pair_acc;      // [M, 36] fp64 sums of J_a^T J_b (zeroed on the stream before every pair launch)
	DeviceBuffer<float> pair_blocks;    // [M, 36] the system's pair blocks (data + ARAP wing blocks on the pair)
	DeviceBuffer<int> zero_inc;         // [N + 1] zeros: the prepare launch's incidence offsets without a hierarchy
	DeviceBuffer<int> c_edge_off;       // [1] the empty stem's edge CSR
	DeviceBuffer<float> c_dinv;         // [1] (no stem blocks)
	// nnrt_fitter_set_step_control: the settings, and the state machine's device state (allocated by
	// prepare() while the mode is on)
	bool step_on = false;
	nnrt_step_control step{};
	DeviceBuffer<StepState> step_state;
	DeviceBuffer<nnrt_step_record> step_history;   // [NNRT_STEP_HISTORY_CAPACITY]
	DeviceBuffer<float> step_best;                 // [N, STEP_BEST_STRIDE] best motion (t, R)
	DeviceBuffer<double> step_partials;            // [step_cost_blocks] k_step_cost's partial sums
	// nnrt_fitter_set_step_objective: the cost step control compares. ROBUST: k_step_cost_robust takes
	// k_step_cost's place and leaves the raw residuals it resolved in step_raw (allocated by prepare() in that mode)
	int32_t step_objective = NNRT_STEP_OBJECTIVE_SQUARE;
	DeviceBuffer<float> step_raw;                  // [P]
	// nnrt_fitter_set_landmarks: the landmarks of the next fit and, once a frame is prepared, their
	// associations grouped by node and by pair (lm.L == 0: none set, and every launch is as without them)
	LandmarkSet lm;
	int last_mode = 0;
	DeviceBuffer<float> snapshot;   // [N,16] node state stored by nnrt_fitter_snapshot_motion (restore-before-iteration runs)
	// nnrt_fitter_set_anchor_graph: edge rows [graph_nodes, graph_degree] in the warp field's virtual node order (checked
	// when set); graph_degree == 0: Euclidean anchors
	DeviceBuffer<int32_t> graph_edges;
	int graph_nodes = 0, graph_degree = 0;
	bool snapshot_valid = false;    // cleared by prepare() (the warp field or the node count may have changed)
	// graphs: one per iteration sequence (the modes of the `count` iterations of an iterate() call, and what each
	// iteration restarts from: RESET_NONE / RESET_IDENTITY / RESET_SNAPSHOT), captured once and replayed as ONE launch; the
	// most recent few are kept. exec == nullptr records a sequence that ran eagerly once (use_hip_graph = 1 captures a
	// sequence on its second request only, so a sequence launched once per frame never pays capture + instantiate).
	struct SeqGraph {
		std::vector<int> modes;
		int reset = 0;
		hipGraphExec_t exec = nullptr;
	};
	std::vector<SeqGraph> graphs;

	void drop_graphs() {
		for (auto& g : graphs)
			if (g.exec) hipGraphExecDestroy(g.exec);
		graphs.clear();
	}
	// a new sequence enters the cache, the oldest leaving it when it is full
	SeqGraph* remember(const std::vector<int>& modes, int reset, hipGraphExec_t exec) {
		constexpr size_t MAX_CACHED_GRAPHS = 8;
		if (graphs.size() >= MAX_CACHED_GRAPHS) {
			if (graphs.front().exec) hipGraphExecDestroy(graphs.front().exec);
			graphs.erase(graphs.begin());
		}
		graphs.push_back({modes, reset, exec});
		return &graphs.back();
	}
};

namespace {

// Orders the fitter's work stream after the caller's stream now, and the caller's stream after the work stream when the
// scope ends, on every path out of it: an error return still leaves the caller's stream ordered after whatever the work
// stream was given (it costs one event; without it the caller could reuse its inputs while the work stream reads them).
// The success path calls leave() so that a failure of the join itself is reported; the destructor cannot report one.
class WorkScope {
public:
	WorkScope(nnrt_fitter* ft, hipStream_t us) : ft_(ft), us_(us) {}
	WorkScope(const WorkScope&) = delete;
	WorkScope& operator=(const WorkScope&) = delete;
	nnrt_status enter() {
		NNRT_HIP(hipEventRecord(ft_->ev_in, us_));
		NNRT_HIP(hipStreamWaitEvent(ft_->work, ft_->ev_in, 0));
		entered_ = true;
		return NNRT_OK;
	}
	nnrt_status leave() {
		if (!entered_) return NNRT_OK;
		entered_ = false;
		NNRT_HIP(hipEventRecord(ft_->ev_out, ft_->work));
		NNRT_HIP(hipStreamWaitEvent(us_, ft_->ev_out, 0));
		return NNRT_OK;
	}
	~WorkScope() {   // an error return: the error string stays the first failure's
		if (entered_ && hipEventRecord(ft_->ev_out, ft_->work) == hipSuccess) hipStreamWaitEvent(us_, ft_->ev_out, 0);
	}

private:
	nnrt_fitter* ft_;
	hipStream_t us_;
	bool entered_ = false;
};

// the damping step control starts a fit with: initial_lambda, or preconditioning_dampening_factor when that is 0, clamped
// into [lambda_min, lambda_max]
float step_initial_lambda(const nnrt_fitter* ft) {
	const float l = ft->step.initial_lambda > 0.f ? ft->step.initial_lambda : ft->p.preconditioning_dampening_factor;
	return fminf(fmaxf(l, ft->step.lambda_min), ft->step.lambda_max);
}

// a Tukey or Huber penalty is enabled in the fitter's parameters (its form is nnrt_fitter_set_robust_options')
bool penalties_enabled(const nnrt_fitter* ft) { return ft->p.use_tukey_penalty_for_data_term || ft->p.use_huber_penalty_for_arap_term; }

// timing events, destroyed on every return
struct Events {
	std::vector<hipEvent_t> ev;
	explicit Events(size_t n) : ev(n, nullptr) {}
	Events(const Events&) = delete;
	Events& operator=(const Events&) = delete;
	nnrt_status create() {
		for (auto& e : ev) NNRT_HIP(hipEventCreate(&e));
		return NNRT_OK;
	}
	~Events() {
		for (hipEvent_t e : ev)
			if (e) hipEventDestroy(e);
	}
};

// Captures what `enqueue` launches on `s` into an executable graph: a partially returned graph is destroyed on every
// early exit, and the graph itself once it is instantiated.
template <class Enqueue>
nnrt_status capture(hipStream_t s, Enqueue&& enqueue, hipGraphExec_t* exec) {
	hipGraph_t g = nullptr;
	NNRT_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
	const nnrt_status st = enqueue();
	const hipError_t ce = hipStreamEndCapture(s, &g);
	if (st || ce != hipSuccess) {
		if (g) hipGraphDestroy(g);
		if (st == NNRT_ERROR_HIP) set_error("kernel launch failed during graph capture");
		if (st) return st;
		NNRT_HIP(ce);
	}
	const hipError_t ie = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
	hipGraphDestroy(g);
	NNRT_HIP(ie);
	return NNRT_OK;
}

// depth overload (DeformableMeshToImageFitter.cpp:278-314): UnprojectDepthImageWithoutFiltering with the pixel intrinsics
// (PerspectiveProjectionImpl.h:60-146): d = depth / scale, valid iff 0 < d < max_depth (AND the optional image mask)
__global__ void k_prepare_reference_depth(const float* __restrict__ depth, const uint8_t* __restrict__ mask, int H, int W, float scale,
                                          float max_depth, Camera pix, float4* __restrict__ out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= static_cast<int64_t>(H) * W) return;
	const int u = static_cast<int>(i % W), v = static_cast<int>(i / W);
	const float d = depth[i] / scale;
	const bool valid = d > 0 && d < max_depth && (mask == nullptr || mask[i] != 0);
	out[i] = valid ? make_float4((static_cast<float>(u) - pix.cx) * d / pix.fx, (static_cast<float>(v) - pix.cy) * d / pix.fy, d, 1.f)
	               : make_float4(0.f, 0.f, 0.f, 0.f);
}

// point-cloud overload (:85-95): organized reference points [P,3] and their mask
__global__ void k_prepare_reference_points(const float* __restrict__ points, const uint8_t* __restrict__ mask, int64_t P,
                                           float4* __restrict__ out) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= P) return;
	const bool valid = mask == nullptr || mask[i] != 0;
	out[i] = valid ? make_float4(points[3 * i], points[3 * i + 1], points[3 * i + 2], 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// canonical vertices / normals [V,3] -> float4 [V] (w = 0): pass 2 forms the warped-surface Jacobian rows from them
__global__ void k_to_float4(const float* __restrict__ p, const float* __restrict__ n, int64_t V, float4* __restrict__ p4, float4* __restrict__ n4) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (i >= V) return;
	p4[i] = make_float4(p[3 * i], p[3 * i + 1], p[3 * i + 2], 0.f);
	n4[i] = make_float4(n[3 * i], n[3 * i + 1], n[3 * i + 2], 0.f);
}

// faces -> int4; an index outside [0, V) becomes the degenerate face (0, 0, 0) (never rasterized, never gathered out of
// bounds) and sets error bit 4, which nnrt_fitter_check reports
// flip_winding: the consistent NDC convention keeps rows in image order, which negates every face's NDC area relative to
// the reference's mirrored image; swapping two corners restores the orientation the back-face test expects.
__global__ void k_faces_to_int4(const int64_t* __restrict__ faces, int64_t F, int64_t V, int flip_winding, int4* __restrict__ out,
                                int* error_flag) {
	const int64_t f = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	if (f >= F) return;
	const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
	if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
		atomicOr(error_flag, 4);
		out[f] = make_int4(0, 0, 0, 0);
		return;
	}
	out[f] = flip_winding ? make_int4(static_cast<int>(i0), static_cast<int>(i2), static_cast<int>(i1), 0)
	                      : make_int4(static_cast<int>(i0), static_cast<int>(i1), static_cast<int>(i2), 0);
}

// from_identity: the warp and the update treat every node's motion as R = I, t = 0 without reading it (only on the
// block-diagonal path with <= 4 anchors, see fold_reset); the result equals a reset followed by the iteration.
// state_in (default: the warp field's state): where the warp and the update read the node motion the iteration starts
// from; the update always writes the warp field's state (a restore-from-snapshot folded into the iteration reads the
// snapshot directly instead of copying it first).
// stages of one iteration (nnrt_fitter_time_kernels launches subsets of them)
enum : unsigned { STAGE_WARP = 1u, STAGE_RASTER = 2u, STAGE_PIXEL = 4u, STAGE_SOLVE = 8u, STAGE_ALL = 15u };

// the fused pixel launch's arguments (the pair launch and the robust step cost take theirs from them)
FitPixelArgs fit_pixel_args(const nnrt_fitter* ft, const nnrt_warp_field* wf, const RasterOptions& ro, const float* state_in, bool from_identity) {
	FitPixelArgs fa{};
	fa.H = ft->key.H;
	fa.W = ft->key.W;
	fa.tiles_x = static_cast<int>(ceil_div(ft->key.W, 16));
	fa.tiles_y = static_cast<int>(ceil_div(ft->key.H, 16));
	fa.tile_row0 = 0;
	fa.pix = ft->key.pix;
	fa.ndc = ft->key.ndc;
	fa.blur = ro.blur;
	fa.ax = ro.ax;
	fa.ay = ro.ay;
	fa.perspective = ft->p.use_perspective_correction;
	fa.max_depth = ft->p.max_depth;
	const int penalty = ft->penalty_form == NNRT_PENALTY_IRLS ? PENALTY_IRLS : PENALTY_REFERENCE;
	fa.use_tukey = ft->p.use_tukey_penalty_for_data_term ? penalty : PENALTY_NONE;
	fa.tukey_c = ft->p.tukey_penalty_cutoff_cm;
	fa.anchor_count = ft->key.K;
	fa.keys = ft->keys.ptr;
	fa.faces4 = ft->faces4.ptr;
	fa.wpos = ft->wpos.ptr;
	fa.wnrm = ft->wnrm.ptr;
	fa.anchors = ft->anchors.ptr;
	fa.face_nodes = ft->face_nodes.ptr;
	fa.jrows = ft->jrows.ptr;
	fa.state_in = reinterpret_cast<const float4*>(state_in);
	fa.state_identity = from_identity;
	fa.cmesh_p = ft->mesh_p4.ptr;
	fa.cmesh_n = ft->mesh_n4.ptr;
	fa.weights = ft->weights.ptr;
	fa.ref_points = ft->ref_points.ptr;
	if (ft->key.launch.quad_order) {
		fa.quad_order = ft->quad_order.ptr;
		fa.order_blocks = quad_order_blocks(4 * fa.tiles_x * fa.tiles_y);
	} else if (ft->key.launch.tile_order) {
		fa.tile_order = ft->tile_order.ptr;
		fa.order_blocks = tile_order_blocks(fa.tiles_x * fa.tiles_y);
	}
	fa.records = ft->records.ptr;
	fa.low_occupancy = ft->key.launch.pix_low_occupancy;
	fa.residuals = ft->residuals.ptr;
	fa.residual_mask = ft->residual_mask.ptr;
	fa.pixel_face = ft->pixel_face.ptr;
	fa.acc = ft->acc.ptr;
	if (ft->key.E > 0) {   // the ARAP edge terms ride in the pixel launch's extra workgroups
		ArapArgs& aa = fa.arap;
		aa.E = ft->key.E;
		aa.N = ft->key.N;
		aa.n0 = ft->key.n0;
		aa.lambda = ft->p.arap_term_weight;
		aa.use_huber = ft->p.use_huber_penalty_for_arap_term ? penalty : PENALTY_NONE;
		aa.huber_delta = ft->p.huber_penalty_constant;
		aa.coverage_variable = wf->coverage_method == NNRT_MINIMAL_K_NEIGHBOR_NODE_DISTANCE;
		aa.edges = wf->edges.ptr;
		aa.edge_layers = wf->edge_layers.ptr;
		aa.radii = wf->radii.ptr;
		aa.node_weights = wf->node_weights.ptr;
		aa.node_state = state_in;
		aa.edge_jr = ft->edge_jr.ptr;
		aa.inc_slot = ft->arap.inc_slot.ptr;
		aa.wing = ft->wing.ptr;
		aa.edge_residuals = ft->edge_residuals.ptr;
		aa.error_flag = ft->error_flag.ptr;
		fa.arap_blocks = fit_pixels_arap_blocks(ft->key.E);
	}
	return fa;
}

// k_step_cost's arguments: one item per pixel and per ARAP edge residual entry
StepCostArgs step_cost_args(const nnrt_fitter* ft, const float* state_in) {
	StepCostArgs ca{};
	ca.P = static_cast<int64_t>(ft->key.H) * ft->key.W;
	ca.E3 = 3 * static_cast<int64_t>(ft->key.E);
	ca.N = ft->key.N;
	ca.blocks = step_cost_blocks(ca.P + ca.E3);
	ca.chunk = step_cost_chunk(ca.P + ca.E3, ca.blocks);
	ca.residuals = ft->residuals.ptr;
	ca.residual_mask = ft->residual_mask.ptr;
	ca.edge_residuals = ft->edge_residuals.ptr;
	ca.state_in = state_in;
	ca.best = ft->step_best.ptr;
	ca.partials = ft->step_partials.ptr;
	ca.st = ft->step_state.ptr;
	ca.error_flag = ft->error_flag.ptr;
	ca.increase = ft->step.increase;
	ca.decrease = ft->step.decrease;
	ca.lambda_min = ft->step.lambda_min;
	ca.lambda_max = ft->step.lambda_max;
	ca.relative_cost_tolerance = ft->step.relative_cost_tolerance;
	ca.landmark_cost = ft->lm.L > 0 ? ft->lm.cost.ptr : nullptr;
	return ca;
}

// k_step_cost_robust's, the robust cost of the raw residuals: the kernel resolves each masked pixel again from the buffers
// the warp, the scatter and the fused launch left (nothing between that launch and this one writes them: the pair launch
// only reads), one item per pixel and per edge
StepCostRobustArgs step_cost_robust_args(const nnrt_fitter* ft, const FitPixelArgs& fa, StepCostArgs ca) {
	StepCostRobustArgs ra{};
	ca.blocks = step_cost_blocks(ca.P + ft->key.E);
	ca.chunk = step_cost_chunk(ca.P + ft->key.E, ca.blocks);
	ra.base = ca;
	ra.view = pixel_resolve_view(fa);
	ra.F = ft->key.F;
	ra.E = ft->key.E;
	ra.W = ft->key.W;
	ra.use_tukey = fa.use_tukey == PENALTY_IRLS;
	ra.use_huber = ft->key.E > 0 && fa.arap.use_huber == PENALTY_IRLS;
	ra.tukey_c = fa.tukey_c;
	ra.huber_delta = ft->p.huber_penalty_constant;
	ra.pixel_face = fa.pixel_face;
	ra.raw = ft->step_raw.ptr;
	return ra;
}

// k_fit_landmarks' arguments (landmarks set and grouped by prepare())
FitLandmarkArgs fit_landmark_args(const nnrt_fitter* ft, const float* state_in, bool from_identity) {
	const LandmarkSet& lm = ft->lm;
	FitLandmarkArgs la{};
	la.L = static_cast<int>(lm.L);
	la.K = ft->key.K;
	la.term_weight = lm.term_weight;
	la.cutoff = lm.cutoff;
	la.state_identity = from_identity;
	la.index = lm.index.ptr;
	la.target = lm.target.ptr;
	la.weight = lm.weight.ptr;
	la.anchors = ft->anchors.ptr;
	la.weights = ft->weights.ptr;
	la.mesh_p = ft->mesh_p.ptr;
	la.wpos = ft->wpos.ptr;
	la.state_in = state_in;
	la.node_keys = lm.node.keys.ptr;
	la.node_vals = lm.node.vals.ptr;
	la.node_starts = lm.node.starts.ptr;
	la.pair_keys = lm.pair.keys.ptr;
	la.pair_vals = lm.pair.vals.ptr;
	la.pair_starts = lm.pair.starts.ptr;
	la.info = lm.info.ptr;
	la.acc = ft->acc.ptr;
	la.distances = lm.distances.ptr;
	la.cost = lm.cost.ptr;
	constexpr int RUNS_PER_BLOCK = 8;
	la.node_blocks = static_cast<int>(ceil_div(landmark_node_run_bound(lm.L, la.K, ft->key.N), RUNS_PER_BLOCK));
	if (ft->key.coupled && ft->ps.M > 0) {
		la.pair_acc = ft->pair_acc.ptr;
		la.pair_blocks = static_cast<int>(ceil_div(landmark_pair_run_bound(lm.L, la.K, ft->ps.M), RUNS_PER_BLOCK));
	}
	return la;
}

// the block-diagonal solve + update's, with the damping as a launch argument or a device word
template <class Lm>
SolveArgsT<Lm> solve_args(const nnrt_fitter* ft, const nnrt_warp_field* wf, const float* state_in, Lm lm) {
	SolveArgsT<Lm> sa{};
	sa.N = ft->key.N;
	sa.lm = lm;
	sa.acc = ft->acc.ptr;
	sa.state_in = state_in;
	sa.node_state = wf->state.ptr;
	sa.updates_out = ft->updates.ptr;
	sa.gradient_out = ft->gradient.ptr;
	sa.hessian_out = ft->hessian.ptr;
	sa.error_flag = ft->error_flag.ptr;
	sa.guard_zero_rotation = ft->guard_zero_rotation;
	return sa;
}

// the two tile-sparse solves' workspaces, built where they are launched: the structure-derived fields from the structure's
// bind(), the vectors and the two launch settings from the fitter (their only home)
ArrowheadWorkspace with_solve_vectors(const nnrt_fitter* ft, ArrowheadWorkspace ws) {
	ws.diag = ft->a_diag.ptr;
	ws.rhs = ft->a_rhs.ptr;
	ws.x = ft->a_x.ptr;
	ws.res = ft->a_res.ptr;
	ws.dx = ft->a_dx.ptr;
	ws.refine = NNRT_ARAP_REFINE != 0;
	ws.refine_ratio = ft->refine_ratio;
	ws.guard_zero_rotation = ft->guard_zero_rotation;
	return ws;
}
ArrowheadWorkspace arrowhead_workspace(const nnrt_fitter* ft) {
	ArrowheadWorkspace ws;
	ft->arap.bind(ws);
	return with_solve_vectors(ft, ws);
}
ArrowheadWorkspace coupled_workspace(const nnrt_fitter* ft) {
	ArrowheadWorkspace ws;
	ft->ps.bind(ws, ft->pair_corner, ft->key.N, ft->c_dinv.ptr, ft->c_edge_off.ptr);
	return with_solve_vectors(ft, ws);
}

nnrt_status enqueue_iteration(nnrt_fitter* ft, const nnrt_warp_field* wf, int mode, hipStream_t s, hipEvent_t* marks = nullptr,
                              bool from_identity = false, const float* state_in = nullptr, unsigned stages = STAGE_ALL) {
	if (!state_in) state_in = wf->state.ptr;
	nnrt_status st;
	auto mark = [&](int i) -> nnrt_status {
		if (marks) NNRT_HIP(hipEventRecord(marks[i], s));
		return NNRT_OK;
	};
	if ((st = mark(0))) return st;
	const bool with_jacobians = NNRT_GATHER_ROWS != 0;
	if ((stages & STAGE_WARP) &&
	    (st = launch_warp_mesh(ft->mesh_p.ptr, ft->mesh_n.ptr, ft->key.V, state_in, ft->anchors.ptr, ft->weights.ptr, ft->key.K, ft->key.extr,
	                           ft->wpos.ptr, ft->wnrm.ptr, with_jacobians ? ft->jrows.ptr : nullptr, ft->key.launch.warp_vertex != 0, s, from_identity,
	                           ft->key.launch.anchors16 ? ft->anchors16.ptr : nullptr)))
		return st;
	if ((st = mark(1))) return st;
	const RasterOptions ro = make_raster_options(ft->key.H, ft->key.W, 0.5f / (static_cast<float>(fminf(ft->key.H, ft->key.W)) / 2.0f), ft->p.use_perspective_correction, 0, 1);
	if ((stages & STAGE_RASTER) && (st = launch_raster_scatter_mesh(ft->wpos.ptr, ft->faces4.ptr, ft->key.F, ft->key.ndc, 0.0f, 10.0f, ro, ft->keys.ptr,
	                                                                ft->key.launch.raster_dense != 0, s)))
		return st;
	if ((st = mark(2))) return st;
	const FitPixelArgs fa = fit_pixel_args(ft, wf, ro, state_in, from_identity);
	if ((stages & STAGE_PIXEL) && (st = launch_fit_pixels(mode, fa, s, marks ? marks[3] : nullptr))) return st;
	const bool coupled = ft->key.coupled != 0;
	if (coupled && (stages & STAGE_PIXEL) && ft->ps.M > 0) {   // the off-diagonal data blocks: a second launch on the same stream
		NNRT_HIP(hipMemsetAsync(ft->pair_acc.ptr, 0, sizeof(double) * 36 * static_cast<size_t>(ft->ps.M), s));
		if ((st = launch_fit_pairs(fa, FitPairArgs{ft->ps.row_off.ptr, ft->ps.pairs.ptr, ft->pair_acc.ptr, 0}, ft->ps.M, s))) return st;
	}
	// the landmark term: its sums join the data term's in acc (and pair_acc) before anything reads them
	if (ft->lm.L > 0 && (stages & STAGE_PIXEL) && (st = launch_fit_landmarks(fit_landmark_args(ft, state_in, from_identity), s))) return st;
	if ((st = mark(4))) return st;
	if (!(stages & STAGE_SOLVE)) return mark(6);
	if ((st = mark(5))) return st;
	// step control: the cost of the state this iteration started from and the decision, before the solve; the solve
	// launches then read the damping the decision left on the device
	const bool step = ft->step_on;
	const float* lm_device = step ? &ft->step_state.ptr->lambda : nullptr;
	if (step) {
		const StepCostArgs ca = step_cost_args(ft, state_in);
		if (ft->step_objective == NNRT_STEP_OBJECTIVE_ROBUST) {
			if ((st = launch_step_cost_robust(step_cost_robust_args(ft, fa, ca), s))) return st;
		} else if ((st = launch_step_cost(ca, s))) {
			return st;
		}
	}
	if (coupled) {
		// diagonal blocks (data + ARAP + LM) and right-hand side as on the arrowhead path, the pair blocks, then the
		// tile-sparse solve with arrow base 0 and the node updates
		if ((st = launch_arrow_prepare(ft->key.N, ft->p.preconditioning_dampening_factor, ft->acc.ptr,
		                               ft->key.E > 0 ? ft->arap.inc_off.ptr : ft->zero_inc.ptr, ft->edge_jr.ptr, ft->a_diag.ptr, ft->a_rhs.ptr,
		                               ft->gradient.ptr, ft->hessian.ptr, s, lm_device)) ||
		    (st = launch_coupled_assemble(ft->pair_acc.ptr, ft->ps.M, ft->ps.edge_off.ptr, ft->ps.edge_list.ptr, ft->wing.ptr, ft->pair_blocks.ptr, s)))
			return st;
		if ((st = arrowhead_solve_core(coupled_workspace(ft), ft->ps.pairs.ptr, ft->pair_blocks.ptr, ft->error_flag.ptr, s, false, wf->state.ptr, ft->updates.ptr, state_in)))
			return st;
	} else if (ft->key.E > 0) {
		const float lm = ft->p.preconditioning_dampening_factor;
		if ((st = launch_arrowhead_iteration(arrowhead_workspace(ft), ft->acc.ptr, lm, wf->edges.ptr, ft->wing.ptr, wf->state.ptr, ft->edge_jr.ptr,
		                                     ft->updates.ptr, ft->gradient.ptr, ft->hessian.ptr, ft->error_flag.ptr, s, state_in, lm_device)))
			return st;
	} else if (step) {
		if ((st = launch_solve_update_device_lm(solve_args(ft, wf, state_in, lm_device), s))) return st;
	} else {
		if ((st = launch_solve_update(mode, solve_args(ft, wf, state_in, ft->p.preconditioning_dampening_factor), s, from_identity))) return st;
	}
	if (step) {   // keep the step, or put the best motion back; the history record
		StepSelectArgs sa{};
		sa.N = ft->key.N;
		sa.updates = ft->updates.ptr;
		sa.node_state = wf->state.ptr;
		sa.best = ft->step_best.ptr;
		sa.st = ft->step_state.ptr;
		sa.history = ft->step_history.ptr;
		sa.error_flag = ft->error_flag.ptr;
		sa.minimal_update_threshold = ft->p.minimal_update_threshold;
		if ((st = launch_step_select(sa, s))) return st;
	}
	return mark(6);
}

} // namespace

extern "C" {

void nnrt_fitter_default_params(nnrt_fitter_params* p) {
	if (!p) return;
	std::memset(p, 0, sizeof(*p));
	p->max_iteration_count = 100;
	p->iteration_mode_count = 1;
	p->iteration_modes[0] = NNRT_ITERATION_ALL;
	p->minimal_update_threshold = 1e-6f;
	p->use_perspective_correction = 1;
	p->max_depth = 10.f;
	p->use_tukey_penalty_for_data_term = 0;
	p->tukey_penalty_cutoff_cm = 0.01f;
	p->preconditioning_dampening_factor = 0.f;
	p->arap_term_weight = 200.f;
	p->use_huber_penalty_for_arap_term = 0;
	p->huber_penalty_constant = 1e-4f;
	p->use_hip_graph = 1;
	p->ndc_convention = NNRT_NDC_REFERENCE;
}

nnrt_status nnrt_fitter_create(const nnrt_fitter_params* params, int32_t device, nnrt_fitter** out) {
	NNRT_CHECK_ARG(params && out, "null pointer");
	if (params->preconditioning_dampening_factor < 0.f || params->preconditioning_dampening_factor > 1.f) {
		set_error("`preconditioning_dampening_factor` should be a small non-negative value between 0 and 1 (DeformableMeshToImageFitter.cpp:79-82)");
		return NNRT_ERROR_ARGUMENT;
	}
	NNRT_CHECK_ARG(params->iteration_mode_count >= 1 && params->iteration_mode_count <= 16, "iteration_mode_count must be in [1, 16]");
	for (int i = 0; i < params->iteration_mode_count; i++)
		NNRT_CHECK_ARG(params->iteration_modes[i] >= 0 && params->iteration_modes[i] <= 2, "unknown iteration mode");
	NNRT_CHECK_ARG(params->ndc_convention == NNRT_NDC_REFERENCE || params->ndc_convention == NNRT_NDC_CONSISTENT, "unknown ndc_convention");
	DeviceGuard guard(device);
	auto ft = std::make_unique<nnrt_fitter>();
	ft->p = *params;
	ft->device = device;
	NNRT_HIP(hipStreamCreateWithFlags(&ft->work, hipStreamNonBlocking));
	NNRT_HIP(hipEventCreateWithFlags(&ft->ev_in, hipEventDisableTiming));
	NNRT_HIP(hipEventCreateWithFlags(&ft->ev_out, hipEventDisableTiming));

	nnrt_status st = ft->error_flag.ensure(1);
	if (st) return st;
	NNRT_HIP(hipMemset(ft->error_flag.ptr, 0, sizeof(int)));
	*out = ft.release();
	return NNRT_OK;
}

void nnrt_fitter_destroy(nnrt_fitter* ft) {
	if (!ft) return;
	DeviceGuard guard(ft->device);
	hipStreamSynchronize(ft->work);
	ft->drop_graphs();
	if (ft->ev_in) hipEventDestroy(ft->ev_in);
	if (ft->ev_out) hipEventDestroy(ft->ev_out);
	if (ft->work) hipStreamDestroy(ft->work);
	delete ft;   // the members free their device memory: after the work stream has drained and the graph execs are gone
}

namespace {
// reference input of one frame: either a depth image (+ scale) or an organized point cloud, with an optional mask
struct FrameReference {
	const float* depth = nullptr;
	const float* points = nullptr;
	const uint8_t* mask = nullptr;
	float depth_scale = 1.f;
};

// what prepare() is given besides the fitter, the warp field and the stream
struct FrameInputs {
	const float *vertices, *normals;
	int64_t V;
	const int64_t* faces;
	int64_t F;
	FrameReference ref;
	int32_t H, W;
	const double *K, *E;
};

// prepare()'s steps, in calling order (prepare_frame below); static: this unnamed namespace stands inside extern "C", where
// a function's unmangled name would be exported. The refusals that leave the fitter as it was:
static nnrt_status check_frame_arguments(const nnrt_fitter* ft, const nnrt_warp_field* wf, const FrameInputs& in) {
	NNRT_CHECK_ARG(ft && wf && in.vertices && in.normals && in.faces && (in.ref.depth || in.ref.points) && in.K, "null pointer");
	NNRT_CHECK_ARG(in.V > 0 && in.F > 0 && in.H > 0 && in.W > 0, "empty mesh or image");
	NNRT_CHECK_ARG(in.V < (int64_t(1) << 31) && in.F < (int64_t(1) << 31), "mesh too large for int32 indexing");
	NNRT_CHECK_ARG(in.ref.depth_scale > 0.f, "depth_scale must be positive");
	NNRT_CHECK_ARG(wf->device == ft->device, "the warp field and the fitter live on different devices");
	return NNRT_OK;
}

// and those of a warp field this fitter cannot take (by then the fitter counts as unprepared)
static nnrt_status check_frame_warp_field(const nnrt_fitter* ft, const nnrt_warp_field* wf) {
	NNRT_CHECK_ARG(wf->N >= wf->anchor_count, "the warp field has fewer nodes than anchors per vertex");
	NNRT_CHECK_ARG(wf->N < FACE_NODE_MAX_NODES, "node count exceeds the face-node table's 20-bit node field");
	NNRT_CHECK_ARG(ft->graph_degree == 0 || ft->graph_nodes == wf->N, "the anchor graph's node_count differs from the warp field's");
	if (wf->E() > 0) {
		for (int i = 0; i < ft->p.iteration_mode_count; i++)
			if (ft->p.iteration_modes[i] != NNRT_ITERATION_ALL) {
				set_error("the regularized (ARAP) solve supports IterationMode ALL only (reference A15: the ARAP Hessian is 6x6-only)");
				return NNRT_ERROR_UNSUPPORTED;
			}
	}
	return NNRT_OK;
}

// This frame's key, as far as it is known before any device work: the two solver plans' generations and the coupled
// mode's pair count are entered by the steps that build them, before the key is compared.
static FrameKey make_frame_key(const nnrt_fitter* ft, const nnrt_warp_field* wf, const FrameInputs& in) {
	int cus = 0;
	if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ft->device) != hipSuccess || cus <= 0) cus = 256;
	FrameKey key;
	std::memset(&key, 0, sizeof(key));
	key.V = in.V;
	key.F = in.F;
	key.wf = wf;
	key.wf_id = wf->id;
	key.H = in.H;
	key.W = in.W;
	key.N = wf->N;
	key.K = wf->anchor_count;
	key.E = wf->E();
	key.n0 = wf->h.layer_counts.empty() ? wf->N : wf->h.layer_counts[0];
	key.quad_slots = 4 * 4 * cus;
	key.ndc = make_ndc_setup(in.K, in.H, in.W, ft->p.ndc_convention == NNRT_NDC_CONSISTENT);
	key.pix = pixel_camera(in.K);
	key.extr = make_extrinsics(in.E);
	key.coupled = ft->data_coupling == NNRT_DATA_COUPLED;
	key.launch = choose_launches(read_launch_switches(), in.V, in.F, in.H, in.W, key.N, key.K, cus, fit_pixels_tile_order_supported());
	return key;
}

// Graph invalidation's one owner in prepare(). Captured graphs bake every buffer's address and the frame's key into
// their kernel arguments, so a step that moves or loses a buffer or re-plans a solver sets `stale`, as does a key that
// differs from the last frame's; the graphs are dropped once, on every path out, the error returns included.
struct GraphInvalidation {
	nnrt_fitter* ft;
	bool stale = false;
	explicit GraphInvalidation(nnrt_fitter* f) : ft(f) {}
	GraphInvalidation(const GraphInvalidation&) = delete;
	GraphInvalidation& operator=(const GraphInvalidation&) = delete;
	~GraphInvalidation() {
		if (stale) ft->drop_graphs();
	}
};

// (re)allocates the frame's buffers, grouped by what needs them; every allocation of the frame reports a moved pointer
static nnrt_status allocate_frame(nnrt_fitter* ft, const FrameKey& key, bool* moved) {
	const size_t V = static_cast<size_t>(key.V), F = static_cast<size_t>(key.F), N = static_cast<size_t>(key.N), K = static_cast<size_t>(key.K);
	const size_t E = static_cast<size_t>(key.E), P = static_cast<size_t>(key.H) * static_cast<size_t>(key.W);
	nnrt_status st;
	// every frame
	if ((st = ensure(ft->mesh_p, 3 * V, moved)) || (st = ensure(ft->mesh_n, 3 * V, moved)) || (st = ensure(ft->faces4, F, moved)) ||
	    (st = ensure(ft->anchors, V * K, moved)) || (st = ensure(ft->weights, V * K, moved)) ||
	    (st = ensure(ft->face_nodes, F * face_node_slots(key.K), moved)) || (st = ensure(ft->wpos, V, moved)) || (st = ensure(ft->wnrm, V, moved)) ||
	    (st = ensure(ft->jrows, NNRT_GATHER_ROWS ? 3 * V * K : 1, moved)) || (st = ensure(ft->mesh_p4, V, moved)) ||
	    (st = ensure(ft->mesh_n4, V, moved)) || (st = ensure(ft->anchors16, key.K == 4 && key.N < 65535 ? V : 1, moved)) ||
	    (st = ensure(ft->ref_points, P, moved)) || (st = ensure(ft->records, 4 * P, moved)) || (st = ensure(ft->keys, P, moved)) ||
	    (st = ensure(ft->residuals, P, moved)) || (st = ensure(ft->residual_mask, P, moved)) || (st = ensure(ft->pixel_face, P, moved)) ||
	    (st = ensure(ft->acc, N * ACC_STRIDE, moved)) || (st = ensure(ft->updates, N * 6, moved)) || (st = ensure(ft->gradient, N * 6, moved)) ||
	    (st = ensure(ft->hessian, N * 36, moved)))
		return st;
	// the pixel launch's order table (one per launch: choose_launches)
	const int tiles = static_cast<int>(ceil_div(key.W, 16) * ceil_div(key.H, 16));
	if (key.launch.quad_order && ((st = ensure(ft->quad_scratch, quad_order_scratch(4 * tiles), moved)) ||
	                              (st = ensure(ft->quad_order, 4 * static_cast<size_t>(quad_order_blocks(4 * tiles)), moved))))
		return st;
	if (key.launch.tile_order &&
	    ((st = ensure(ft->tile_flags, tiles, moved)) || (st = ensure(ft->tile_order, static_cast<size_t>(tile_order_blocks(tiles)), moved))))
		return st;
	// ARAP: the edge terms; and the tile-sparse solves' vectors, the coupled mode's too (without a hierarchy its prepare
	// launch still takes an edge-term pointer)
	if (E > 0 && ((st = ensure(ft->wing, E * 36, moved)) || (st = ensure(ft->edge_residuals, 3 * E, moved)))) return st;
	if ((E > 0 || key.coupled) &&
	    ((st = ensure(ft->a_diag, N * 36, moved)) || (st = ensure(ft->edge_jr, 2 * E * EDGE_TERMS, moved)) || (st = ensure(ft->a_rhs, 6 * N, moved)) ||
	     (st = ensure(ft->a_x, 6 * N, moved)) || (st = ensure(ft->a_res, 6 * N, moved)) || (st = ensure(ft->a_dx, 6 * N, moved))))
		return st;
	// coupled: what stands for the empty stem, and the prepare launch's incidence offsets without a hierarchy
	if (key.coupled) {
		if ((st = ensure(ft->zero_inc, N + 1, moved)) || (st = ensure(ft->c_edge_off, 1, moved)) || (st = ensure(ft->c_dinv, 36, moved))) return st;
		NNRT_HIP(hipMemset(ft->zero_inc.ptr, 0, sizeof(int) * (N + 1)));
		NNRT_HIP(hipMemset(ft->c_edge_off.ptr, 0, sizeof(int)));
	}
	// step control's device state
	if (ft->step_on) {
		if ((st = ensure(ft->step_state, 1, moved)) || (st = ensure(ft->step_history, NNRT_STEP_HISTORY_CAPACITY, moved)) ||
		    (st = ensure(ft->step_best, N * STEP_BEST_STRIDE, moved)) ||
		    (st = ensure(ft->step_partials, static_cast<size_t>(step_cost_blocks(static_cast<int64_t>(P + 3 * E))), moved)))
			return st;
		if (ft->step_objective == NNRT_STEP_OBJECTIVE_ROBUST && (st = ensure(ft->step_raw, P, moved))) return st;
	}
	return NNRT_OK;
}

// the arrowhead solve's structure over the hierarchy's edges (host planning and uploads; an unchanged hierarchy keeps it)
static nnrt_status build_arap_structure(nnrt_fitter* ft, const nnrt_warp_field* wf, FrameKey& key, bool* moved) {
	nnrt_status st = NNRT_OK;
	if (key.E > 0) {
		st = ft->arap.build(wf->h.edges.data(), key.E, key.n0, key.N, virtual_node_positions(wf, key.n0, key.N - key.n0).data(), true);
		if (ft->arap.moved) *moved = true;
	}
	key.corner_generation = ft->arap.corner.generation;
	return st;
}

// the mesh side of the frame on the work stream: copies, conversions, anchors and the face-node table
static nnrt_status enqueue_mesh_setup(nnrt_fitter* ft, const nnrt_warp_field* wf, const FrameKey& key, const FrameInputs& in, hipStream_t s) {
	const int64_t V = key.V, F = key.F;
	nnrt_status st;
	NNRT_HIP(hipMemcpyAsync(ft->mesh_p.ptr, in.vertices, sizeof(float) * 3 * V, hipMemcpyDeviceToDevice, s));
	NNRT_HIP(hipMemcpyAsync(ft->mesh_n.ptr, in.normals, sizeof(float) * 3 * V, hipMemcpyDeviceToDevice, s));
	k_faces_to_int4<<<static_cast<unsigned>(ceil_div(F, 256)), 256, 0, s>>>(in.faces, F, V, ft->p.ndc_convention == NNRT_NDC_CONSISTENT,
	                                                                        ft->faces4.ptr, ft->error_flag.ptr);
	NNRT_LAUNCH_CHECK();
	k_to_float4<<<static_cast<unsigned>(ceil_div(V, 256)), 256, 0, s>>>(in.vertices, in.normals, V, ft->mesh_p4.ptr, ft->mesh_n4.ptr);
	NNRT_LAUNCH_CHECK();
	// once per frame (:96-106): anchors & weights on the canonical mesh in virtual node order
	const float* anchor_node_weights = wf->coverage_method == NNRT_MINIMAL_K_NEIGHBOR_NODE_DISTANCE ? wf->node_weights.ptr : nullptr;
	if (ft->graph_degree > 0) {
		// along the anchor graph's edges (PlanarGraphWarpField::PrecomputeAnchorsAndWeights, SHORTEST_PATH): no distance
		// threshold in this mode
		if ((st = launch_anchors_shortest_path(ft->mesh_p.ptr, V, wf->node_positions.ptr, key.N, ft->graph_edges.ptr, ft->graph_degree, key.K,
		                                       wf->coverage, anchor_node_weights, ft->anchors.ptr, ft->weights.ptr, s, true)))
			return st;
	} else if ((st = launch_compute_anchors(ft->mesh_p.ptr, V, wf->node_positions.ptr, key.N, key.K, wf->coverage, anchor_node_weights,
	                                        wf->threshold ? wf->minimum_valid : 0, ft->anchors.ptr, ft->weights.ptr, s)))
		return st;
	// the faces' distinct anchor nodes (AssociateFacesWithAnchors, :105), consumed by the node pass of every iteration
	if ((st = launch_face_node_table(ft->faces4.ptr, F, ft->anchors.ptr, key.K, ft->face_nodes.ptr, s))) return st;
	if (key.launch.anchors16 && (st = launch_pack_anchors16(ft->anchors.ptr, V, ft->anchors16.ptr, s))) return st;
	return NNRT_OK;
}

// Coupled mode: the frame's node pairs from the face-node table (+ the hierarchy's edges) on the work stream, then the
// solver plan over them: the one host round trip of the mode (the plan needs the coordinates); iterate() plans nothing.
// The plan's generation and the pair count enter the key here.
static nnrt_status build_coupled_structure(nnrt_fitter* ft, const nnrt_warp_field* wf, FrameKey& key, hipStream_t s, bool* moved) {
	if (!key.coupled) return NNRT_OK;
	nnrt_status st = build_pair_structure(ft->ps, ft->face_nodes.ptr, key.F, key.K, wf->edges.ptr, wf->h.edges.data(), key.E, key.N, s, moved);
	if (!st) st = ft->pair_corner.prepare(ft->ps.h_pairs.data(), ft->ps.M, 0, key.N, virtual_node_positions(wf, 0, key.N).data());
	if (st) {   // what the pair buffers and the plan hold now is unknown
		*moved = true;
		return st;
	}
	key.pair_generation = ft->pair_corner.generation;
	key.M = ft->ps.M;
	const size_t M = static_cast<size_t>(ft->ps.M);
	if ((st = ensure(ft->pair_acc, 36 * M, moved)) || (st = ensure(ft->pair_blocks, 36 * M, moved))) return st;
	return NNRT_OK;
}

// The landmarks of this fit against this frame's mesh and anchors: their associations grouped by node and, in coupled
// mode, by pair (group_landmarks waits for the work stream: the refusals are the host's to report).
static nnrt_status build_landmark_structure(nnrt_fitter* ft, const FrameKey& key, hipStream_t s, bool* moved) {
	if (ft->lm.L == 0) return NNRT_OK;
	LandmarkFrame fr{};
	fr.V = key.V;
	fr.F = key.F;
	fr.N = key.N;
	fr.K = key.K;
	fr.faces4 = ft->faces4.ptr;
	fr.anchors = ft->anchors.ptr;
	fr.coupled = key.coupled;
	fr.M = key.coupled ? ft->ps.M : 0;
	fr.row_off = ft->ps.row_off.ptr;
	fr.pairs = ft->ps.pairs.ptr;
	nnrt_status st = allocate_landmark_groups(ft->lm, fr, moved);
	if (!st) st = group_landmarks(ft->lm, fr, s);
	return st;
}

// the image side of the frame on the work stream: reference points, the pixel launch's order table, the raster keys and
// the accumulators, step control's restart
static nnrt_status enqueue_reference_setup(nnrt_fitter* ft, const FrameKey& key, const FrameReference& ref, hipStream_t s) {
	const int H = key.H, W = key.W, tiles_x = static_cast<int>(ceil_div(W, 16)), tiles_y = static_cast<int>(ceil_div(H, 16));
	const int64_t P = static_cast<int64_t>(H) * W;
	nnrt_status st;
	// reference point cloud (:289-306): depth / scale with 0 < d < max_depth, AND the user mask; stored as depth (0 = masked)
	if (ref.depth)
		k_prepare_reference_depth<<<static_cast<unsigned>(ceil_div(P, 256)), 256, 0, s>>>(ref.depth, ref.mask, H, W, ref.depth_scale,
		                                                                                  ft->p.max_depth, key.pix, ft->ref_points.ptr);
	else
		k_prepare_reference_points<<<static_cast<unsigned>(ceil_div(P, 256)), 256, 0, s>>>(ref.points, ref.mask, P, ft->ref_points.ptr);
	NNRT_LAUNCH_CHECK();
	// the pixel launch's tile order for this frame's reference points
	if (key.launch.tile_order && (st = launch_tile_order(ft->ref_points.ptr, H, W, tiles_x, tiles_y, ft->tile_flags.ptr, ft->tile_order.ptr, s))) return st;
	if (key.launch.quad_order &&
	    (st = launch_quad_order(ft->ref_points.ptr, H, W, tiles_x, tiles_y, key.quad_slots, ft->quad_scratch.ptr, ft->quad_order.ptr, s)))
		return st;
	NNRT_HIP(hipMemsetAsync(ft->keys.ptr, 0xff, sizeof(uint64_t) * P, s));
	NNRT_HIP(hipMemsetAsync(ft->acc.ptr, 0, sizeof(double) * key.N * ACC_STRIDE, s));
	if (ft->step_on) {
		if ((st = launch_step_reset(ft->step_state.ptr, step_initial_lambda(ft), s))) return st;
		// an edge the ARAP launch refuses (A3, error bit 2) writes no residual: the cost then sums zeros there, not stale values
		if (key.E > 0) NNRT_HIP(hipMemsetAsync(ft->edge_residuals.ptr, 0, sizeof(float) * 3 * static_cast<size_t>(key.E), s));
		// nnrt_fitter_get_raw_residuals before the first iteration reads zeros
		if (ft->step_objective == NNRT_STEP_OBJECTIVE_ROBUST) NNRT_HIP(hipMemsetAsync(ft->step_raw.ptr, 0, sizeof(float) * static_cast<size_t>(P), s));
	}
	return NNRT_OK;
}

nnrt_status prepare_frame(nnrt_fitter* ft, nnrt_warp_field* wf, const FrameInputs& in, void* stream) {
	nnrt_status st;
	if ((st = check_frame_arguments(ft, wf, in))) return st;
	DeviceGuard guard(ft->device);
	// until this frame is fully prepared the fitter is not: a failure below (allocation, corner plan) leaves iterate()
	// refusing rather than replaying graphs over buffers that may have been released
	ft->prepared = false;
	if ((st = check_frame_warp_field(ft, wf))) return st;
	FrameKey key = make_frame_key(ft, wf, in);
	GraphInvalidation graphs(ft);
	if ((st = allocate_frame(ft, key, &graphs.stale)) || (st = build_arap_structure(ft, wf, key, &graphs.stale))) return st;
	hipStream_t us = static_cast<hipStream_t>(stream), s = ft->work;
	WorkScope scope(ft, us);   // the work stream runs after the caller's stream, and the caller's after it again on every return
	if ((st = scope.enter()) || (st = enqueue_mesh_setup(ft, wf, key, in, s)) || (st = build_coupled_structure(ft, wf, key, s, &graphs.stale)) ||
	    (st = build_landmark_structure(ft, key, s, &graphs.stale)))
		return st;
	// the key is complete: any other change of what the graphs bake in drops them too
	if (std::memcmp(&key, &ft->key, sizeof(key)) != 0) graphs.stale = true;
	ft->key = key;
	ft->snapshot_valid = false;
	if ((st = enqueue_reference_setup(ft, key, in.ref, s)) || (st = scope.leave())) return st;
	ft->prepared = true;
	return NNRT_OK;
}
} // namespace

nnrt_status nnrt_fitter_prepare(nnrt_fitter* ft, nnrt_warp_field* wf, const float* d_vertices, const float* d_normals, int64_t V,
                                const int64_t* d_faces, int64_t F, const float* d_depth, const uint8_t* d_mask, int32_t H, int32_t W,
                                const double* h_K, const double* h_E, float depth_scale, void* stream) {
	FrameReference ref;
	ref.depth = d_depth;
	ref.mask = d_mask;
	ref.depth_scale = depth_scale;
	NNRT_CHECK_ARG(d_depth, "null depth image");
	return prepare_frame(ft, wf, FrameInputs{d_vertices, d_normals, V, d_faces, F, ref, H, W, h_K, h_E}, stream);
}

int32_t nnrt_fit_quad_order_blocks(int32_t quadrants) { return quadrants > 0 ? quad_order_blocks(quadrants) : 0; }

nnrt_status nnrt_fit_quad_order_table(const uint8_t* h_valid, int32_t H, int32_t W, int32_t slots, int32_t* h_counts, int32_t* h_table) {
	NNRT_CHECK_ARG(h_valid && h_counts && h_table, "null pointer");
	NNRT_CHECK_ARG(H > 0 && W > 0 && slots >= 0, "empty image or negative slot count");
	const int tiles_x = static_cast<int>(ceil_div(W, 16)), tiles_y = static_cast<int>(ceil_div(H, 16)), quadrants = 4 * tiles_x * tiles_y;
	const size_t P = static_cast<size_t>(H) * W, entries = 4 * static_cast<size_t>(quad_order_blocks(quadrants));
	std::vector<float4> ref(P);
	for (size_t p = 0; p < P; p++) ref[p] = make_float4(0.f, 0.f, 1.f, h_valid[p] ? 1.f : 0.f);
	DeviceBuffer<float4> d_ref;
	DeviceBuffer<int> d_scratch, d_order;
	nnrt_status st = NNRT_OK;
	if (!(st = upload(d_ref, ref)) && !(st = d_scratch.ensure(quad_order_scratch(quadrants))) && !(st = d_order.ensure(entries)) &&
	    !(st = launch_quad_order(d_ref.ptr, H, W, tiles_x, tiles_y, slots, d_scratch.ptr, d_order.ptr, nullptr))) {
		if (hipMemcpy(h_counts, d_scratch.ptr, sizeof(int) * quadrants, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(h_table, d_order.ptr, sizeof(int) * entries, hipMemcpyDeviceToHost) != hipSuccess) {
			set_error("hipMemcpy failed");
			st = NNRT_ERROR_HIP;
		}
	}
	return st;
}

nnrt_status nnrt_fitter_prepare_point_cloud(nnrt_fitter* ft, nnrt_warp_field* wf, const float* d_vertices, const float* d_normals,
                                            int64_t V, const int64_t* d_faces, int64_t F, const float* d_points, const uint8_t* d_point_mask,
                                            int32_t H, int32_t W, const double* h_K, const double* h_E, void* stream) {
	FrameReference ref;
	ref.points = d_points;
	ref.mask = d_point_mask;
	NNRT_CHECK_ARG(d_points, "null reference point cloud");
	return prepare_frame(ft, wf, FrameInputs{d_vertices, d_normals, V, d_faces, F, ref, H, W, h_K, h_E}, stream);
}

namespace {
constexpr int MAX_GRAPH_ITERATIONS = 64;   // iterations per captured sequence graph (longer runs replay several)
// what the iterations of a sequence restart from: nothing; the identity warp (every iteration); the stored snapshot (every
// iteration); the stored snapshot before the first iteration of the call only (a whole frame fit from a stored state)
enum { RESET_NONE = 0, RESET_IDENTITY = 1, RESET_SNAPSHOT = 2, RESET_SNAPSHOT_FIRST = 3 };

// A restart folded into the iteration's kernels where they support it: from the identity (block-diagonal path, <= 4
// anchors: the identity-specialised warp / update), or from the snapshot (every path: the warp, the ARAP edge terms and
// the update read the snapshot as the starting state). Otherwise a separate kernel restarts.
bool fold_reset(const nnrt_fitter* ft) { return ft->key.E == 0 && ft->key.K <= 4 && !ft->key.coupled; }
bool fold_snapshot(const nnrt_fitter*) { return true; }

nnrt_status check_frame(const nnrt_fitter* ft, const nnrt_warp_field* wf, const char* who) {
	if (!ft->prepared || ft->key.wf != wf || ft->key.wf_id != wf->id) {
		set_error(std::string("nnrt_fitter_prepare must be called with this warp field before ") + who);
		return NNRT_ERROR_ARGUMENT;
	}
	if (wf->device != ft->device) {
		set_error("the warp field and the fitter live on different devices");
		return NNRT_ERROR_ARGUMENT;
	}
	return NNRT_OK;
}

// how iteration i of a sequence starts
struct Restart {   // internal (static helpers below), not part of the C-ABI
	int kernel = RESET_NONE;         // restart launched before the iteration (RESET_NONE: none)
	bool from_identity = false;      // folded identity start
	const float* state_in = nullptr; // folded snapshot start
};

static Restart restart_plan(const nnrt_fitter* ft, int r) {
	Restart p;
	if (r == RESET_IDENTITY) {
		if (fold_reset(ft)) p.from_identity = true;
		else p.kernel = RESET_IDENTITY;
	} else if (r == RESET_SNAPSHOT) {
		if (fold_snapshot(ft)) p.state_in = ft->snapshot.ptr;
		else p.kernel = RESET_SNAPSHOT;
	}
	return p;
}

// a restart launched on s (inside or outside a capture)
nnrt_status enqueue_restart(nnrt_fitter* ft, nnrt_warp_field* wf, int kernel, hipStream_t s) {
	if (kernel == RESET_IDENTITY) return launch_reset_motion(wf->state.ptr, wf->N, s);
	if (kernel == RESET_SNAPSHOT) return launch_copy_state(ft->snapshot.ptr, wf->state.ptr, wf->N, s);
	return NNRT_OK;
}

nnrt_status enqueue_step(nnrt_fitter* ft, nnrt_warp_field* wf, int mode, int restart, hipStream_t s) {
	const Restart p = restart_plan(ft, restart);
	nnrt_status st = enqueue_restart(ft, wf, p.kernel, s);
	if (st) return st;
	return enqueue_iteration(ft, wf, mode, s, nullptr, p.from_identity, p.state_in);
}

int restart_of(int reset, bool first_of_call) {
	return reset == RESET_SNAPSHOT_FIRST ? (first_of_call ? RESET_SNAPSHOT : RESET_NONE) : reset;
}

nnrt_status iterate_impl(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t first_iteration, int32_t count, int reset, hipStream_t us) {
	ft->refine_ratio_used = ft->refine_ratio;
	nnrt_status st;
	if (ft->step_on) {
		if (reset == RESET_IDENTITY || reset == RESET_SNAPSHOT) {
			set_error("invalid argument: step control is on: iterations that restart every time (nnrt_fitter_iterate_from_identity / _from_snapshot) are refused");
			return NNRT_ERROR_ARGUMENT;
		}
		// a fit starts: the state machine restarts (outside the captured sequences, which stay the same launches)
		if (first_iteration == 0 && count > 0 && (st = launch_step_reset(ft->step_state.ptr, step_initial_lambda(ft), us))) return st;
	}
	for (int it0 = first_iteration; it0 < first_iteration + count; it0 += MAX_GRAPH_ITERATIONS) {
		const int n = std::min(MAX_GRAPH_ITERATIONS, first_iteration + count - it0);
		std::vector<int> modes(static_cast<size_t>(n));
		for (int i = 0; i < n; i++) modes[static_cast<size_t>(i)] = ft->p.iteration_modes[(it0 + i) % ft->p.iteration_mode_count];
		ft->last_mode = modes.back();
		// a sequence graph is keyed by its modes and by what each of its iterations restarts from
		const int key_reset = reset == RESET_SNAPSHOT_FIRST && it0 != first_iteration ? RESET_NONE : reset;
		nnrt_fitter::SeqGraph* seen = nullptr;
		for (auto& g : ft->graphs)
			if (g.reset == key_reset && g.modes == modes) seen = &g;
		const bool graphed = ft->p.use_hip_graph == NNRT_GRAPH_ALWAYS || (ft->p.use_hip_graph == NNRT_GRAPH_AUTO && seen != nullptr);
		auto enqueue_on = [&](hipStream_t s) {
			nnrt_status r = NNRT_OK;
			for (int i = 0; i < n && !r; i++) r = enqueue_step(ft, wf, modes[static_cast<size_t>(i)], restart_of(reset, it0 + i == first_iteration), s);
			return r;
		};
		if (!graphed) {
			// eager launches on the caller's stream
			if ((st = enqueue_on(us))) return st;
			if (ft->p.use_hip_graph == NNRT_GRAPH_AUTO && !seen) ft->remember(modes, key_reset, nullptr);
			continue;
		}
		// Graphs are captured on the fitter's private stream (capture needs a non-legacy stream) and replayed on the
		// caller's: a whole run of iterations is one launch.
		if (!seen || !seen->exec) {
			hipGraphExec_t exec = nullptr;
			if ((st = capture(ft->work, [&] { return enqueue_on(ft->work); }, &exec))) return st;
			if (seen) seen->exec = exec;
			else seen = ft->remember(modes, key_reset, exec);
		}
		NNRT_HIP(hipGraphLaunch(seen->exec, us));
	}
	return NNRT_OK;
}
} // namespace

nnrt_status nnrt_fitter_iterate(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t first_iteration, int32_t count, void* stream) {
	NNRT_CHECK_ARG(ft && wf && count >= 0, "invalid arguments");
	nnrt_status st = check_frame(ft, wf, "nnrt_fitter_iterate");
	if (st) return st;
	DeviceGuard guard(ft->device);
	return iterate_impl(ft, wf, first_iteration, count, RESET_NONE, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_fitter_iterate_from_identity(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t first_iteration, int32_t count, void* stream) {
	NNRT_CHECK_ARG(ft && wf && count >= 0, "invalid arguments");
	nnrt_status st = check_frame(ft, wf, "nnrt_fitter_iterate_from_identity");
	if (st) return st;
	DeviceGuard guard(ft->device);
	return iterate_impl(ft, wf, first_iteration, count, RESET_IDENTITY, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_fitter_corner_info(const nnrt_fitter* ft, int64_t* h_out) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	const CornerSolver& c = ft->arap.corner;
	const bool on = ft->key.E > 0;
	h_out[0] = on ? ft->key.N - ft->key.n0 : 0;
	h_out[1] = on ? c.tile_columns() : 0;
	h_out[2] = on ? c.levels() : 0;
	h_out[3] = on ? c.back_launches() : 0;
	h_out[4] = on ? c.stored_tiles() : 0;
	h_out[5] = on ? c.dense_lower_tiles() : 0;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_launch_plan(const nnrt_fitter* ft, int32_t* h_out, int64_t count) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	NNRT_CHECK_ARG(count >= LAUNCH_CHOICE_COUNT, "count must be at least 6");
	NNRT_CHECK_ARG(ft->prepared, "no prepared frame");
	std::memcpy(h_out, &ft->key.launch, sizeof(ft->key.launch));
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_warped_mesh(nnrt_fitter* ft, float* h_positions, float* h_normals, int64_t vertex_count, void* stream) {
	NNRT_CHECK_ARG(ft && h_positions && h_normals, "null pointer");
	NNRT_CHECK_ARG(ft->key.V > 0 && ft->wpos.ptr, "no prepared frame");
	// the host buffers hold vertex_count rows: a mismatch with the prepared mesh is refused, not written past
	NNRT_CHECK_ARG(vertex_count == ft->key.V, "vertex_count differs from the prepared mesh's vertex count");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	std::vector<float4> p(static_cast<size_t>(ft->key.V)), n(static_cast<size_t>(ft->key.V));
	NNRT_HIP(hipMemcpy(p.data(), ft->wpos.ptr, sizeof(float4) * p.size(), hipMemcpyDeviceToHost));
	NNRT_HIP(hipMemcpy(n.data(), ft->wnrm.ptr, sizeof(float4) * n.size(), hipMemcpyDeviceToHost));
	for (size_t v = 0; v < p.size(); v++) {
		h_positions[3 * v] = p[v].x;
		h_positions[3 * v + 1] = p[v].y;
		h_positions[3 * v + 2] = p[v].z;
		h_normals[3 * v] = n[v].x;
		h_normals[3 * v + 1] = n[v].y;
		h_normals[3 * v + 2] = n[v].z;
	}
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_arrowhead_system(nnrt_fitter* ft, float* h_diag, float* h_wing, float* h_rhs, int64_t node_count, int64_t edge_count,
                                             void* stream) {
	NNRT_CHECK_ARG(ft && h_diag && h_wing && h_rhs, "null pointer");
	NNRT_CHECK_ARG(ft->key.E > 0 && ft->a_diag.ptr && ft->wing.ptr && ft->a_rhs.ptr, "no prepared ARAP frame (the arrowhead system needs layer_count > 1)");
	NNRT_CHECK_ARG(node_count == ft->key.N && edge_count == ft->key.E, "node_count / edge_count differ from the prepared frame's");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	NNRT_HIP(hipMemcpy(h_diag, ft->a_diag.ptr, sizeof(float) * 36 * static_cast<size_t>(ft->key.N), hipMemcpyDeviceToHost));
	NNRT_HIP(hipMemcpy(h_wing, ft->wing.ptr, sizeof(float) * 36 * static_cast<size_t>(ft->key.E), hipMemcpyDeviceToHost));
	NNRT_HIP(hipMemcpy(h_rhs, ft->a_rhs.ptr, sizeof(float) * 6 * static_cast<size_t>(ft->key.N), hipMemcpyDeviceToHost));
	return NNRT_OK;
}

nnrt_status nnrt_fitter_corner_work(const nnrt_fitter* ft, int64_t* h_out) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	const CornerSolver& c = ft->arap.corner;
	const bool on = ft->key.E > 0;
	h_out[0] = on ? c.mfma_flops() : 0;
	h_out[1] = on ? c.update_terms() : 0;
	h_out[2] = on ? c.eliminated_columns() : 0;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_refine_info(nnrt_fitter* ft, float* h_out, void* stream) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	DeviceGuard guard(ft->device);
	// the gate as the last launched solve applied it: its device pivot word and the threshold it ran with (a later
	// nnrt_fitter_set_refine_ratio changes the next solve, not the report of this one: ADVICE r4)
	h_out[0] = 1.f;
	h_out[1] = ft->refine_ratio_used;
	h_out[2] = 0.f;
	h_out[3] = 0.f;
	h_out[4] = 0.f;
	if (ft->key.E > 0 && ft->arap.corner.pivot_ratio()) {
		NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
		NNRT_HIP(hipStreamSynchronize(ft->work));
		unsigned w[REFINE_WORDS] = {};
		NNRT_HIP(hipMemcpy(w, ft->arap.corner.pivot_ratio(), sizeof(w), hipMemcpyDeviceToHost));
		float r, dm, xm;
		std::memcpy(&r, &w[0], sizeof(r));
		std::memcpy(&dm, &w[REFINE_GUARD_D], sizeof(dm));
		std::memcpy(&xm, &w[REFINE_GUARD_X], sizeof(xm));
		const bool ran = NNRT_ARAP_REFINE != 0 && refine_window(r, ft->refine_ratio_used);
		h_out[0] = r;
		h_out[2] = ran ? 1.f : 0.f;
		h_out[3] = ran ? (xm > 0.f ? dm / xm : dm) : 0.f;
		h_out[4] = ran && refine_accept(dm, xm) ? 1.f : 0.f;
	}
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_refine_ratio(nnrt_fitter* ft, float ratio) {
	NNRT_CHECK_ARG(ft, "null pointer");
	NNRT_CHECK_ARG(ratio >= 0.f, "refine ratio must be >= 0 (0: never refine)");
	if (ratio == ft->refine_ratio) return NNRT_OK;
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->refine_ratio = ratio;
	ft->drop_graphs();   // the threshold is a launch argument of the captured sequences
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_robust_options(nnrt_fitter* ft, int32_t penalty_form, int32_t guard_zero_rotation) {
	NNRT_CHECK_ARG(ft, "null pointer");
	NNRT_CHECK_ARG(penalty_form == NNRT_PENALTY_REFERENCE || penalty_form == NNRT_PENALTY_IRLS,
	               "penalty_form must be NNRT_PENALTY_REFERENCE (0) or NNRT_PENALTY_IRLS (1)");
	NNRT_CHECK_ARG(guard_zero_rotation == 0 || guard_zero_rotation == 1, "guard_zero_rotation must be 0 or 1");
	NNRT_CHECK_ARG(!(ft->step_on && penalty_form == NNRT_PENALTY_IRLS && ft->step_objective == NNRT_STEP_OBJECTIVE_SQUARE),
	               "penalty_form: NNRT_PENALTY_IRLS is refused while step control is on (its cost is the square objective)");
	NNRT_CHECK_ARG(!(ft->step_objective == NNRT_STEP_OBJECTIVE_ROBUST && penalty_form == NNRT_PENALTY_REFERENCE && penalties_enabled(ft)),
	               "penalty_form: NNRT_PENALTY_REFERENCE with a penalty enabled is refused under NNRT_STEP_OBJECTIVE_ROBUST (the "
	               "reference's branches have no objective)");
	if (penalty_form == ft->penalty_form && guard_zero_rotation == ft->guard_zero_rotation) return NNRT_OK;
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->penalty_form = penalty_form;
	ft->guard_zero_rotation = guard_zero_rotation;
	ft->drop_graphs();   // both are launch arguments of the captured sequences; the prepared frame stays
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_data_coupling(nnrt_fitter* ft, int32_t data_coupling) {
	NNRT_CHECK_ARG(ft, "null pointer");
	NNRT_CHECK_ARG(data_coupling == NNRT_DATA_BLOCK_DIAGONAL || data_coupling == NNRT_DATA_COUPLED,
	               "data_coupling must be NNRT_DATA_BLOCK_DIAGONAL (0) or NNRT_DATA_COUPLED (1)");
	if (data_coupling == NNRT_DATA_COUPLED)
		for (int i = 0; i < ft->p.iteration_mode_count; i++)
			NNRT_CHECK_ARG(ft->p.iteration_modes[i] == NNRT_ITERATION_ALL,
			               "data_coupling: NNRT_DATA_COUPLED supports IterationMode ALL only (6x6 blocks), and the fitter's mode list holds another");
	if (data_coupling == ft->data_coupling) return NNRT_OK;
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->data_coupling = data_coupling;
	ft->drop_graphs();      // the captured sequences hold the launches of the other mode
	ft->prepared = false;   // the pair structure and the solver plan over it are built in prepare()
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_data_coupling(const nnrt_fitter* ft, int32_t* data_coupling) {
	NNRT_CHECK_ARG(ft && data_coupling, "null pointer");
	*data_coupling = ft->data_coupling;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_step_control(nnrt_fitter* ft, const nnrt_step_control* settings) {
	nnrt_step_control v{};
	if (settings) {   // the ranges first: they need no fitter
		v = *settings;
		// (every comparison is false for a NaN, which is refused with the rest)
		NNRT_CHECK_ARG(v.initial_lambda >= 0.f && std::isfinite(v.initial_lambda), "step control: initial_lambda must be finite and >= 0 (0: preconditioning_dampening_factor)");
		NNRT_CHECK_ARG(v.increase > 1.f && std::isfinite(v.increase), "step control: increase must be finite and > 1");
		NNRT_CHECK_ARG(v.decrease > 0.f && v.decrease <= 1.f, "step control: decrease must lie in (0, 1]");
		NNRT_CHECK_ARG(v.lambda_min >= 0.f && v.lambda_max >= v.lambda_min && v.lambda_max > 0.f && std::isfinite(v.lambda_max),
		               "step control: lambda_min / lambda_max must satisfy 0 <= lambda_min <= lambda_max, 0 < lambda_max < inf");
		NNRT_CHECK_ARG(v.relative_cost_tolerance >= 0.f && std::isfinite(v.relative_cost_tolerance),
		               "step control: relative_cost_tolerance must be finite and >= 0");
		NNRT_CHECK_ARG(v.poll_interval >= 0, "step control: poll_interval must be >= 0");
	}
	NNRT_CHECK_ARG(ft, "null pointer");
	if (settings) {
		NNRT_CHECK_ARG(ft->penalty_form != NNRT_PENALTY_IRLS || ft->step_objective == NNRT_STEP_OBJECTIVE_ROBUST,
		               "step control is refused while NNRT_PENALTY_IRLS is set (SQUARE penalties only: the residual buffer holds the scaled residual)");
		for (int i = 0; i < ft->p.iteration_mode_count; i++)
			NNRT_CHECK_ARG(ft->p.iteration_modes[i] == NNRT_ITERATION_ALL,
			               "step control supports IterationMode ALL only, and the fitter's mode list holds another");
	}
	const bool on = settings != nullptr;
	if (on == ft->step_on && std::memcmp(&v, &ft->step, sizeof(v)) == 0) return NNRT_OK;
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->step_on = on;
	ft->step = v;
	ft->drop_graphs();      // the captured sequences hold the launches of the other mode
	ft->prepared = false;   // the state machine's buffers are prepare()'s
	if (!on) {              // nothing of the mode stays allocated
		ft->step_state.release();
		ft->step_history.release();
		ft->step_best.release();
		ft->step_partials.release();
		ft->step_raw.release();
	}
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_step_objective(nnrt_fitter* ft, int32_t objective) {
	NNRT_CHECK_ARG(objective == NNRT_STEP_OBJECTIVE_SQUARE || objective == NNRT_STEP_OBJECTIVE_ROBUST,
	               "objective must be NNRT_STEP_OBJECTIVE_SQUARE (0) or NNRT_STEP_OBJECTIVE_ROBUST (1)");
	NNRT_CHECK_ARG(ft, "null pointer");
	NNRT_CHECK_ARG(!(objective == NNRT_STEP_OBJECTIVE_ROBUST && ft->penalty_form == NNRT_PENALTY_REFERENCE && penalties_enabled(ft)),
	               "objective: NNRT_STEP_OBJECTIVE_ROBUST is refused with NNRT_PENALTY_REFERENCE and a penalty enabled (the reference's "
	               "branches have no objective)");
	NNRT_CHECK_ARG(!(objective == NNRT_STEP_OBJECTIVE_SQUARE && ft->step_on && ft->penalty_form == NNRT_PENALTY_IRLS),
	               "objective: NNRT_STEP_OBJECTIVE_SQUARE is refused while step control is on and NNRT_PENALTY_IRLS is set (SQUARE "
	               "penalties only under that objective)");
	if (objective == ft->step_objective) return NNRT_OK;
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->step_objective = objective;
	ft->drop_graphs();   // the captured sequences hold the other cost launch
	if (objective == NNRT_STEP_OBJECTIVE_SQUARE) ft->step_raw.release();
	// with step control on, the raw residual buffer is prepare()'s, and the state machine restarts there
	if (ft->step_on) ft->prepared = false;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_step_objective(const nnrt_fitter* ft, int32_t* objective) {
	NNRT_CHECK_ARG(ft && objective, "null pointer");
	*objective = ft->step_objective;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_raw_residuals(nnrt_fitter* ft, float* h_out, int64_t count, void* stream) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	NNRT_CHECK_ARG(ft->prepared && ft->step_on && ft->step_objective == NNRT_STEP_OBJECTIVE_ROBUST && ft->step_raw.ptr,
	               "no prepared frame with step control on under NNRT_STEP_OBJECTIVE_ROBUST");
	// the host buffer holds `count` floats: a mismatch with the prepared image is refused, not written past
	NNRT_CHECK_ARG(count == static_cast<int64_t>(ft->key.H) * ft->key.W, "count differs from the prepared image's pixel count");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	NNRT_HIP(hipMemcpy(h_out, ft->step_raw.ptr, sizeof(float) * static_cast<size_t>(count), hipMemcpyDeviceToHost));
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_landmarks(nnrt_fitter* ft, const int32_t* d_vertex_indices, const float* d_targets, const float* d_weights, int64_t count,
                                      float term_weight, float cutoff, void* stream) {
	// the ranges first: they need no fitter
	NNRT_CHECK_ARG(count >= 0 && count < (int64_t(1) << 24), "landmarks: count must lie in [0, 2^24)");
	NNRT_CHECK_ARG(std::isfinite(term_weight) && term_weight > 0.f, "landmarks: term_weight must be finite and > 0");
	NNRT_CHECK_ARG(std::isfinite(cutoff), "landmarks: cutoff must be finite (<= 0: no cutoff)");
	NNRT_CHECK_ARG(count == 0 || (d_vertex_indices && d_targets), "landmarks: null d_vertex_indices or d_targets");
	NNRT_CHECK_ARG(ft, "null pointer");
	if (count > 0)
		for (int i = 0; i < ft->p.iteration_mode_count; i++)
			NNRT_CHECK_ARG(ft->p.iteration_modes[i] == NNRT_ITERATION_ALL,
			               "landmarks support IterationMode ALL only (6x6 blocks), and the fitter's mode list holds another");
	LandmarkSet& lm = ft->lm;
	if (count == 0 && lm.L == 0) return NNRT_OK;
	DeviceGuard guard(ft->device);
	hipStream_t us = static_cast<hipStream_t>(stream);
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->prepared = false;   // the grouping by node and by pair is prepare()'s
	if (count == 0) {
		NNRT_HIP(hipStreamSynchronize(us));   // (an iteration enqueued there may still read the buffers)
		ft->drop_graphs();
		lm.release_all();
		return NNRT_OK;
	}
	// the captured sequences bake the count (their grids), the two settings and the buffers' addresses
	bool moved = lm.L != count || lm.term_weight != term_weight || lm.cutoff != cutoff;
	const size_t L = static_cast<size_t>(count);
	nnrt_status st;
	if ((st = ensure(lm.index, L, &moved)) || (st = ensure(lm.target, 3 * L, &moved)) || (st = ensure(lm.weight, L, &moved)) ||
	    (st = ensure(lm.distances, L, &moved)) || (st = ensure(lm.cost, 1, &moved))) {
		ft->drop_graphs();
		lm.L = 0;
		return st;
	}
	if (moved) ft->drop_graphs();
	lm.L = count;
	lm.term_weight = term_weight;
	lm.cutoff = cutoff;
	for (auto& v : lm.h_info) v = 0;
	NNRT_HIP(hipMemcpyAsync(lm.index.ptr, d_vertex_indices, sizeof(int32_t) * L, hipMemcpyDeviceToDevice, us));
	NNRT_HIP(hipMemcpyAsync(lm.target.ptr, d_targets, sizeof(float) * 3 * L, hipMemcpyDeviceToDevice, us));
	if (d_weights) NNRT_HIP(hipMemcpyAsync(lm.weight.ptr, d_weights, sizeof(float) * L, hipMemcpyDeviceToDevice, us));
	else NNRT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lm.weight.ptr), 0x3f800000, L, us));   // 1.0f
	// what nnrt_fitter_get_landmark_distances reads before the first iteration: zeros
	NNRT_HIP(hipMemsetAsync(lm.distances.ptr, 0, sizeof(float4) * L, us));
	NNRT_HIP(hipMemsetAsync(lm.cost.ptr, 0, sizeof(double), us));
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_landmark_distances(nnrt_fitter* ft, float* h_out, int64_t count, void* stream) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	NNRT_CHECK_ARG(ft->lm.L > 0 && ft->lm.distances.ptr, "no landmarks set");
	// the host buffer holds 4 * count floats: a mismatch with the landmark count is refused, not written past
	NNRT_CHECK_ARG(count == ft->lm.L, "count differs from the number of landmarks set");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	NNRT_HIP(hipMemcpy(h_out, ft->lm.distances.ptr, sizeof(float4) * static_cast<size_t>(count), hipMemcpyDeviceToHost));
	return NNRT_OK;
}

nnrt_status nnrt_fitter_landmark_info(const nnrt_fitter* ft, int64_t* h_out, int64_t out_count) {
	NNRT_CHECK_ARG(ft && h_out, "null pointer");
	NNRT_CHECK_ARG(out_count >= 4, "out_count must be at least 4");
	const bool grouped = ft->prepared && ft->lm.L > 0;
	h_out[0] = ft->lm.L;
	h_out[1] = grouped ? ft->lm.h_info[LM_INFO_ASSOC] : 0;
	h_out[2] = grouped ? ft->lm.h_info[LM_INFO_RUNS] : 0;
	h_out[3] = grouped ? ft->lm.h_info[LM_INFO_PAIR_ASSOC] : 0;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_step_control(const nnrt_fitter* ft, int32_t* enabled, nnrt_step_control* settings) {
	NNRT_CHECK_ARG(ft && enabled, "null pointer");
	*enabled = ft->step_on ? 1 : 0;
	if (settings) *settings = ft->step;
	return NNRT_OK;
}

namespace {
// the device's state word, after everything enqueued on the caller's stream (and the work stream) has run
nnrt_status read_step_state(nnrt_fitter* ft, hipStream_t us, StepState* out) {
	NNRT_HIP(hipStreamSynchronize(us));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	NNRT_HIP(hipMemcpy(out, ft->step_state.ptr, sizeof(StepState), hipMemcpyDeviceToHost));
	return NNRT_OK;
}
} // namespace

nnrt_status nnrt_fitter_get_step_history(nnrt_fitter* ft, nnrt_step_record* records, int64_t capacity, int64_t* out_count, void* stream) {
	NNRT_CHECK_ARG(ft && out_count, "null pointer");
	*out_count = 0;
	if (!ft->step_on || !ft->prepared || !ft->step_state.ptr) return NNRT_OK;
	DeviceGuard guard(ft->device);
	StepState ss;
	nnrt_status st = read_step_state(ft, static_cast<hipStream_t>(stream), &ss);
	if (st) return st;
	const int64_t total = ss.iteration, n = std::min<int64_t>(total, NNRT_STEP_HISTORY_CAPACITY);
	*out_count = n;
	// the host buffer holds `capacity` records: fewer than there are is refused, not written past
	NNRT_CHECK_ARG(capacity >= n && (records || n == 0), "capacity is smaller than the number of step records");
	if (n == 0) return NNRT_OK;
	std::vector<nnrt_step_record> ring(NNRT_STEP_HISTORY_CAPACITY);
	NNRT_HIP(hipMemcpy(ring.data(), ft->step_history.ptr, sizeof(nnrt_step_record) * ring.size(), hipMemcpyDeviceToHost));
	for (int64_t k = 0; k < n; k++) records[k] = ring[static_cast<size_t>((total - n + k) % NNRT_STEP_HISTORY_CAPACITY)];
	return NNRT_OK;
}

int64_t nnrt_fitter_coupled_pair_count(const nnrt_fitter* ft) {
	if (!ft) return -1;
	return ft->prepared && ft->key.coupled ? ft->ps.M : 0;
}

nnrt_status nnrt_fitter_get_coupled_system(nnrt_fitter* ft, float* h_diag, int32_t* h_pairs, float* h_blocks, float* h_rhs, int64_t node_count,
                                           int64_t pair_count, void* stream) {
	NNRT_CHECK_ARG(ft && h_diag && h_pairs && h_blocks && h_rhs, "null pointer");
	NNRT_CHECK_ARG(ft->prepared && ft->key.coupled && ft->a_diag.ptr && ft->a_rhs.ptr, "no prepared frame in NNRT_DATA_COUPLED mode");
	NNRT_CHECK_ARG(node_count == ft->key.N && pair_count == ft->ps.M, "node_count / pair_count differ from the prepared frame's");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	const size_t M = static_cast<size_t>(ft->ps.M);
	NNRT_HIP(hipMemcpy(h_diag, ft->a_diag.ptr, sizeof(float) * 36 * static_cast<size_t>(ft->key.N), hipMemcpyDeviceToHost));
	NNRT_HIP(hipMemcpy(h_rhs, ft->a_rhs.ptr, sizeof(float) * 6 * static_cast<size_t>(ft->key.N), hipMemcpyDeviceToHost));
	if (M > 0) {
		std::memcpy(h_pairs, ft->ps.h_pairs.data(), sizeof(int32_t) * 2 * M);
		NNRT_HIP(hipMemcpy(h_blocks, ft->pair_blocks.ptr, sizeof(float) * 36 * M, hipMemcpyDeviceToHost));
	}
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_robust_options(const nnrt_fitter* ft, int32_t* penalty_form, int32_t* guard_zero_rotation) {
	NNRT_CHECK_ARG(ft && penalty_form && guard_zero_rotation, "null pointer");
	*penalty_form = ft->penalty_form;
	*guard_zero_rotation = ft->guard_zero_rotation;
	return NNRT_OK;
}

nnrt_status nnrt_fitter_set_anchor_graph(nnrt_fitter* ft, const int32_t* d_edges, int32_t node_count, int32_t graph_degree, void* stream) {
	NNRT_CHECK_ARG(ft, "null pointer");
	DeviceGuard guard(ft->device);
	hipStream_t us = static_cast<hipStream_t>(stream);
	if (!d_edges && ft->graph_degree == 0) return NNRT_OK;
	if (d_edges) {
		NNRT_CHECK_ARG(node_count >= 1 && graph_degree >= 1, "the anchor graph needs node_count >= 1 and graph_degree >= 1");
		nnrt_status st = check_anchor_edges(d_edges, node_count, graph_degree, us);   // synchronizes the caller's stream
		if (st) return st;
	}
	NNRT_HIP(hipStreamSynchronize(ft->work));
	ft->drop_graphs();   // the anchors are inputs of the captured sequences
	ft->prepared = false;   // the prepared frame's anchors are the previous mode's
	ft->graph_nodes = ft->graph_degree = 0;
	if (!d_edges) return NNRT_OK;
	const size_t count = static_cast<size_t>(node_count) * graph_degree;
	nnrt_status st = ft->graph_edges.ensure(count);
	if (st) return st;
	NNRT_HIP(hipMemcpyAsync(ft->graph_edges.ptr, d_edges, sizeof(int32_t) * count, hipMemcpyDeviceToDevice, us));
	NNRT_HIP(hipStreamSynchronize(us));
	ft->graph_nodes = node_count;
	ft->graph_degree = graph_degree;
	return NNRT_OK;
}

int32_t nnrt_fitter_graph_count(const nnrt_fitter* ft) {
	if (!ft) return -1;
	int32_t n = 0;
	for (const auto& g : ft->graphs) n += g.exec != nullptr;
	return n;
}

nnrt_status nnrt_fitter_snapshot_motion(nnrt_fitter* ft, nnrt_warp_field* wf, void* stream) {
	NNRT_CHECK_ARG(ft && wf, "null pointer");
	nnrt_status st = check_frame(ft, wf, "nnrt_fitter_snapshot_motion");
	if (st) return st;
	DeviceGuard guard(ft->device);
	const auto before = ft->snapshot.ptr;
	if ((st = ft->snapshot.ensure(static_cast<size_t>(wf->N) * NODE_STRIDE))) return st;
	if (ft->snapshot.ptr != before) ft->drop_graphs();
	if ((st = launch_copy_state(wf->state.ptr, ft->snapshot.ptr, wf->N, static_cast<hipStream_t>(stream)))) return st;
	ft->snapshot_valid = true;
	return NNRT_OK;
}

static nnrt_status from_snapshot(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t first_iteration, int32_t count, int reset, void* stream,
                                 const char* who) {
	NNRT_CHECK_ARG(ft && wf && count >= 0, "invalid arguments");
	nnrt_status st = check_frame(ft, wf, who);
	if (st) return st;
	if (!ft->snapshot_valid) {
		set_error(std::string("nnrt_fitter_snapshot_motion must be called after prepare() before ") + who);
		return NNRT_ERROR_ARGUMENT;
	}
	DeviceGuard guard(ft->device);
	return iterate_impl(ft, wf, first_iteration, count, reset, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_fitter_iterate_from_snapshot(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t first_iteration, int32_t count, void* stream) {
	return from_snapshot(ft, wf, first_iteration, count, RESET_SNAPSHOT, stream, "nnrt_fitter_iterate_from_snapshot");
}

nnrt_status nnrt_fitter_fit_from_snapshot(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t count, void* stream) {
	return from_snapshot(ft, wf, 0, count, RESET_SNAPSHOT_FIRST, stream, "nnrt_fitter_fit_from_snapshot");
}

nnrt_status nnrt_fitter_restore_motion(nnrt_fitter* ft, nnrt_warp_field* wf, void* stream) {
	NNRT_CHECK_ARG(ft && wf, "null pointer");
	nnrt_status st = check_frame(ft, wf, "nnrt_fitter_restore_motion");
	if (st) return st;
	if (!ft->snapshot_valid) {
		set_error("nnrt_fitter_snapshot_motion must be called after prepare() before nnrt_fitter_restore_motion");
		return NNRT_ERROR_ARGUMENT;
	}
	DeviceGuard guard(ft->device);
	return enqueue_restart(ft, wf, RESET_SNAPSHOT, static_cast<hipStream_t>(stream));
}

nnrt_status nnrt_fitter_iterate_timed(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t first_iteration, int32_t count, float* h_stage_ms,
                                      void* stream) {
	NNRT_CHECK_ARG(ft && wf && h_stage_ms && count > 0, "invalid arguments");
	if (nnrt_status cst = check_frame(ft, wf, "nnrt_fitter_iterate_timed")) return cst;
	DeviceGuard guard(ft->device);
	ft->refine_ratio_used = ft->refine_ratio;
	hipStream_t us = static_cast<hipStream_t>(stream);
	WorkScope scope(ft, us);
	nnrt_status st = scope.enter();
	if (st) return st;
	constexpr int NS = NNRT_TIMED_STAGES;
	Events events(static_cast<size_t>(count) * (NS + 1));
	if ((st = events.create())) return st;
	std::vector<hipEvent_t>& ev = events.ev;
	for (int i = 0; i < count; i++) {
		const int it = first_iteration + i;
		const int mode = ft->p.iteration_modes[it % ft->p.iteration_mode_count];
		ft->last_mode = mode;
		if ((st = enqueue_iteration(ft, wf, mode, ft->work, &ev[static_cast<size_t>(i) * (NS + 1)]))) return st;
	}
	NNRT_HIP(hipStreamSynchronize(ft->work));
	for (int k = 0; k < NS; k++) h_stage_ms[k] = 0.f;
	for (int i = 0; i < count; i++)
		for (int k = 0; k < NS; k++) {
			float ms = 0.f;
			NNRT_HIP(hipEventElapsedTime(&ms, ev[static_cast<size_t>(i) * (NS + 1) + k], ev[static_cast<size_t>(i) * (NS + 1) + k + 1]));
			h_stage_ms[k] += ms / count;
		}
	return scope.leave();
}

nnrt_status nnrt_fitter_time_kernels(nnrt_fitter* ft, nnrt_warp_field* wf, int32_t reps, int32_t trials, float* h_kernel_ms, void* stream) {
	NNRT_CHECK_ARG(ft && wf && h_kernel_ms && reps > 0 && trials > 0, "invalid arguments");
	if (nnrt_status cst = check_frame(ft, wf, "nnrt_fitter_time_kernels")) return cst;
	if (!ft->snapshot_valid) {
		set_error("nnrt_fitter_snapshot_motion must be called after prepare() before nnrt_fitter_time_kernels");
		return NNRT_ERROR_ARGUMENT;
	}
	DeviceGuard guard(ft->device);
	hipStream_t us = static_cast<hipStream_t>(stream);
	hipStream_t s = ft->work;
	WorkScope scope(ft, us);
	nnrt_status st = scope.enter();
	if (st) return st;
	ft->refine_ratio_used = ft->refine_ratio;
	// an error the caller's own earlier iterations raised and has not checked yet survives the timing replays (their
	// flags are discarded below): saved here, restored at the end
	int pending_flag = 0;
	NNRT_HIP(hipStreamSynchronize(s));
	NNRT_HIP(hipMemcpy(&pending_flag, ft->error_flag.ptr, sizeof(int), hipMemcpyDeviceToHost));
	// prefix sequences, each `reps` iterations from the snapshot state in one graph: every kernel runs after the launch
	// it follows in a real iteration (the raster alone excepted, which repeats its own idempotent scatter)
	const unsigned seq[4] = {STAGE_ALL, STAGE_RASTER | STAGE_PIXEL | STAGE_SOLVE, STAGE_RASTER | STAGE_PIXEL, STAGE_RASTER};
	const int mode = ft->p.iteration_modes[0];
	hipGraphExec_t exec[4] = {};
	Events events(2);
	std::vector<hipEvent_t>& ev = events.ev;
	std::vector<float> per_rep[4];
	const size_t P = static_cast<size_t>(ft->key.H) * ft->key.W;
	auto run = [&]() -> nnrt_status {
		if (nnrt_status es = events.create()) return es;
		for (int q = 0; q < 4; q++) {
			auto enqueue = [&] {
				nnrt_status cs = NNRT_OK;
				for (int i = 0; i < reps && !cs; i++) cs = enqueue_iteration(ft, wf, mode, s, nullptr, false, ft->snapshot.ptr, seq[q]);
				return cs;
			};
			if (nnrt_status cs = capture(s, enqueue, &exec[q])) return cs;
		}
		// trials interleave the four sequences (clock drift cancels); consumers' state (raster keys, accumulators) is
		// reset outside the timed region before every replay
		for (int t = -1; t < trials; t++)
			for (int q = 0; q < 4; q++) {
				NNRT_HIP(hipMemsetAsync(ft->keys.ptr, 0xff, sizeof(uint64_t) * P, s));
				NNRT_HIP(hipMemsetAsync(ft->acc.ptr, 0, sizeof(double) * static_cast<size_t>(ft->key.N) * ACC_STRIDE, s));
				NNRT_HIP(hipEventRecord(ev[0], s));
				NNRT_HIP(hipGraphLaunch(exec[q], s));
				NNRT_HIP(hipEventRecord(ev[1], s));
				NNRT_HIP(hipEventSynchronize(ev[1]));
				float ms = 0.f;
				NNRT_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
				if (t >= 0) per_rep[q].push_back(ms / reps);   // trial -1 warms the graph
			}
		return NNRT_OK;
	};
	st = run();
	for (auto& e : exec)
		if (e) hipGraphExecDestroy(e);
	if (!st) {
		float med[4];
		for (int q = 0; q < 4; q++) {
			std::vector<float> v = per_rep[q];
			std::sort(v.begin(), v.end());
			med[q] = v[v.size() / 2];
		}
		h_kernel_ms[0] = med[0] - med[1];   // warp
		h_kernel_ms[1] = med[3];            // raster
		h_kernel_ms[2] = med[2] - med[3];   // fused pixel launch
		h_kernel_ms[3] = med[1] - med[2];   // solve + update (ARAP: the whole arrowhead chain)
		h_kernel_ms[4] = med[0];            // whole iteration
		// leave the fitter as an iteration would: raster keys empty, accumulators zero, motion = the snapshot's result;
		// the device error flag goes back to what the caller's own iterations left (the replays' flags are dropped:
		// nnrt_fitter_check reports the caller's iterations only)
		NNRT_HIP(hipMemsetAsync(ft->keys.ptr, 0xff, sizeof(uint64_t) * P, s));
		NNRT_HIP(hipMemsetAsync(ft->acc.ptr, 0, sizeof(double) * static_cast<size_t>(ft->key.N) * ACC_STRIDE, s));
		NNRT_HIP(hipStreamSynchronize(s));
		NNRT_HIP(hipMemcpy(ft->error_flag.ptr, &pending_flag, sizeof(int), hipMemcpyHostToDevice));
		// the replays drove step control's state machine: it restarts (a fit in progress does not survive the timing)
		if (ft->step_on) {
			if (nnrt_status rs = launch_step_reset(ft->step_state.ptr, step_initial_lambda(ft), s)) return rs;
		}
	}
	return st ? st : scope.leave();
}

nnrt_status nnrt_fitter_check(nnrt_fitter* ft, void* stream) {
	NNRT_CHECK_ARG(ft, "null pointer");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	int flag = 0;
	NNRT_HIP(hipMemcpy(&flag, ft->error_flag.ptr, sizeof(int), hipMemcpyDeviceToHost));
	NNRT_HIP(hipMemset(ft->error_flag.ptr, 0, sizeof(int)));
	if (flag & 8) {
		set_error("the corner's dataflow substitution launch gave up waiting on a dependency (k_corner_flow spin bound)");
		return NNRT_ERROR_HIP;
	}
	if (flag & 1) {
		set_error("potrf failed: a Hessian block (or the Schur complement) is not positive-definite (reference NNRT_LAPACK_CHECK, "
		          "SolveBlockDiagonalCholeskyCPU.cpp:48-51)");
		return NNRT_ERROR_NOT_POSITIVE_DEFINITE;
	}
	if (flag & 2) {
		set_error("fixed-coverage ARAP residual indexes edge_layer_indices[node_j] out of bounds (reference quirk A3)");
		return NNRT_ERROR_UNSUPPORTED;
	}
	if (flag & 4) {
		set_error("mesh triangle index out of range (faces must index [0, vertex_count))");
		return NNRT_ERROR_ARGUMENT;
	}
	return NNRT_OK;
}

// a whole frame's iterations: all of them in one call; with step control's poll_interval = k > 0, k at a time, the host
// reading the device's `done` between the calls and stopping there
static nnrt_status fit_iterations(nnrt_fitter* ft, nnrt_warp_field* wf, void* stream) {
	const int total = ft->p.max_iteration_count, k = ft->step_on ? ft->step.poll_interval : 0;
	if (k <= 0) return nnrt_fitter_iterate(ft, wf, 0, total, stream);
	for (int it0 = 0; it0 < total; it0 += k) {
		nnrt_status st = nnrt_fitter_iterate(ft, wf, it0, std::min(k, total - it0), stream);
		if (st) return st;
		DeviceGuard guard(ft->device);
		StepState ss;
		if ((st = read_step_state(ft, static_cast<hipStream_t>(stream), &ss))) return st;
		if (ss.done) break;
	}
	return NNRT_OK;
}

nnrt_status nnrt_fitter_fit_to_image(nnrt_fitter* ft, nnrt_warp_field* wf, const float* d_vertices, const float* d_normals, int64_t V,
                                     const int64_t* d_faces, int64_t F, const float* d_depth, const uint8_t* d_mask, int32_t H, int32_t W,
                                     const double* h_K, const double* h_E, float depth_scale, void* stream) {
	nnrt_status st = nnrt_fitter_prepare(ft, wf, d_vertices, d_normals, V, d_faces, F, d_depth, d_mask, H, W, h_K, h_E, depth_scale, stream);
	if (st) return st;
	// A14: the reference never updates `maximum_update`, so the loop always runs max_iteration_count iterations
	if ((st = fit_iterations(ft, wf, stream))) return st;
	return nnrt_fitter_check(ft, stream);
}

nnrt_status nnrt_fitter_fit_to_point_cloud(nnrt_fitter* ft, nnrt_warp_field* wf, const float* d_vertices, const float* d_normals, int64_t V,
                                           const int64_t* d_faces, int64_t F, const float* d_points, const uint8_t* d_point_mask, int32_t H,
                                           int32_t W, const double* h_K, const double* h_E, void* stream) {
	nnrt_status st = nnrt_fitter_prepare_point_cloud(ft, wf, d_vertices, d_normals, V, d_faces, F, d_points, d_point_mask, H, W, h_K, h_E, stream);
	if (st) return st;
	if ((st = fit_iterations(ft, wf, stream))) return st;
	return nnrt_fitter_check(ft, stream);
}

nnrt_status nnrt_fitter_get_diagnostics(nnrt_fitter* ft, float* h_residuals, uint8_t* h_mask, int32_t* h_faces, float* h_updates,
                                        float* h_gradient, float* h_hessian, void* stream) {
	NNRT_CHECK_ARG(ft && ft->prepared, "fitter not prepared");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	const int64_t P = static_cast<int64_t>(ft->key.H) * ft->key.W;
	const int s = ft->last_mode == NNRT_ITERATION_ALL ? 6 : 3;
	if (h_residuals) NNRT_HIP(hipMemcpy(h_residuals, ft->residuals.ptr, sizeof(float) * P, hipMemcpyDeviceToHost));
	if (h_mask) NNRT_HIP(hipMemcpy(h_mask, ft->residual_mask.ptr, P, hipMemcpyDeviceToHost));
	if (h_faces) NNRT_HIP(hipMemcpy(h_faces, ft->pixel_face.ptr, sizeof(int32_t) * P, hipMemcpyDeviceToHost));
	if (h_updates) NNRT_HIP(hipMemcpy(h_updates, ft->updates.ptr, sizeof(float) * ft->key.N * s, hipMemcpyDeviceToHost));
	if (h_gradient) NNRT_HIP(hipMemcpy(h_gradient, ft->gradient.ptr, sizeof(float) * ft->key.N * s, hipMemcpyDeviceToHost));
	if (h_hessian) NNRT_HIP(hipMemcpy(h_hessian, ft->hessian.ptr, sizeof(float) * ft->key.N * s * s, hipMemcpyDeviceToHost));
	return NNRT_OK;
}

nnrt_status nnrt_fitter_get_anchors(nnrt_fitter* ft, int32_t* h_anchors, float* h_weights, void* stream) {
	NNRT_CHECK_ARG(ft && ft->prepared, "fitter not prepared");
	DeviceGuard guard(ft->device);
	NNRT_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
	NNRT_HIP(hipStreamSynchronize(ft->work));
	if (h_anchors) NNRT_HIP(hipMemcpy(h_anchors, ft->anchors.ptr, sizeof(int32_t) * ft->key.V * ft->key.K, hipMemcpyDeviceToHost));
	if (h_weights) NNRT_HIP(hipMemcpy(h_weights, ft->weights.ptr, sizeof(float) * ft->key.V * ft->key.K, hipMemcpyDeviceToHost));
	return NNRT_OK;
}

// ---- DLPack entry point (include/nnrt_dlpack.h): validate, then forward to the pointer entry point -----------------
nnrt_status nnrt_fitter_fit_to_image_dlpack(nnrt_fitter* ft, nnrt_warp_field* wf, const DLManagedTensor* vertices, const DLManagedTensor* normals,
                                            const DLManagedTensor* faces, const DLManagedTensor* depth, const DLManagedTensor* mask,
                                            const DLManagedTensor* K, const DLManagedTensor* E, float depth_scale, void* stream) {
	using namespace dl;
	NNRT_CHECK_ARG(ft && wf, "null handle");
	NNRT_CHECK_ARG(wf->device == ft->device, "the warp field and the fitter live on different devices");
	const int dev = ft->device;
	const void *pv, *pn, *pf, *pd, *pm = nullptr, *pk, *pe;
	int64_t dv[2], dn[2], df[2], dd[2], dm[2], dk[2], de[2];
	nnrt_status st;
	if ((st = dl_check(vertices, "vertices", {F32}, 2, {-1, 3}, Mem::device, dev, &pv, dv))) return st;
	if ((st = dl_check(normals, "normals", {F32}, 2, {dv[0], 3}, Mem::device, dev, &pn, dn))) return st;
	if ((st = dl_check(faces, "faces", {I64}, 2, {-1, 3}, Mem::device, dev, &pf, df))) return st;
	if ((st = dl_check(depth, "depth", {F32}, 2, {-1, -1}, Mem::device, dev, &pd, dd))) return st;
	if (mask && (st = dl_check(mask, "mask", {B8, U8}, 2, {dd[0], dd[1]}, Mem::device, dev, &pm, dm))) return st;
	if ((st = dl_check(K, "K", {F64}, 2, {3, 3}, Mem::host, dev, &pk, dk))) return st;
	if ((st = dl_check(E, "E", {F64}, 2, {4, 4}, Mem::host, dev, &pe, de))) return st;
	NNRT_CHECK_ARG(dd[0] <= INT32_MAX && dd[1] <= INT32_MAX, "depth: image too large");
	return nnrt_fitter_fit_to_image(ft, wf, static_cast<const float*>(pv), static_cast<const float*>(pn), dv[0], static_cast<const int64_t*>(pf),
	                                df[0], static_cast<const float*>(pd), static_cast<const uint8_t*>(pm), static_cast<int32_t>(dd[0]),
	                                static_cast<int32_t>(dd[1]), static_cast<const double*>(pk), static_cast<const double*>(pe), depth_scale, stream);
}

} // extern "C"
