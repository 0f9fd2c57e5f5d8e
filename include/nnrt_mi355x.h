/*
 * nnrt_mi355x.h -- C-ABI of the MI355X-native DeformableMeshToImageFitter hot path.
 *
 * Drop-in boundary for henry123-boy/Dynamicfuion_python's dense non-rigid tracker. Every entry point replaces a
 * reference interface, cited per function (paths relative to the reference repository root). Plain pointers and
 * sizes only: arrays marked d_ are DEVICE pointers (hipMalloc'd or torch.cuda tensors on the same device), h_ arrays
 * are HOST pointers. All functions return 0 on success and a non-zero nnrt_status otherwise, with a message retrievable
 * through nnrt_last_error() (thread-local). No exceptions cross the ABI. A `stream` argument is a hipStream_t (NULL =
 * the legacy default stream). Handles are not thread-safe: use one handle per host thread.
 *
 * Layout conventions follow the reference tensors: float32 row-major, vertex/face/node-major; rotations [N,3,3]
 * row-major; triangle indices int64 [F,3]; intrinsics/extrinsics float64 [3,3]/[4,4] on the host.
 */
#ifndef NNRT_MI355X_H
#define NNRT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t nnrt_status;
enum {
	NNRT_OK = 0,
	NNRT_ERROR_ARGUMENT = 1,
	NNRT_ERROR_HIP = 2,
	NNRT_ERROR_NOT_POSITIVE_DEFINITE = 3,   /* reference: NNRT_LAPACK_CHECK potrf failure -> RuntimeError */
	NNRT_ERROR_UNSUPPORTED = 4,
	NNRT_ERROR_CAPACITY = 5,
	NNRT_ERROR_INTERNAL = 6                 /* an algorithm's own invariant failed (never expected; reported, not spun on) */
};

/* iteration modes: cpp/alignment/IterationMode.h:24-28 */
enum { NNRT_ITERATION_ALL = 0, NNRT_ITERATION_TRANSLATION_ONLY = 1, NNRT_ITERATION_ROTATION_ONLY = 2 };
/* warp-node coverage: cpp/geometry/WarpNodeCoverageComputationMethod.h */
enum { NNRT_FIXED_NODE_COVERAGE = 0, NNRT_MINIMAL_K_NEIGHBOR_NODE_DISTANCE = 1 };

typedef struct nnrt_warp_field nnrt_warp_field;
typedef struct nnrt_fitter nnrt_fitter;

const char* nnrt_last_error(void);
/* HIP runtime version the library was built against and the number of visible devices (-1 on error). */
int32_t nnrt_runtime_version(void);
int32_t nnrt_device_count(void);
/* Bytes of device memory the library's handles and temporaries hold at this moment, process-wide (diagnostic: a handle
 * that is destroyed returns what it took, so a leak shows as a count that does not come back; stream-ordered temporaries
 * leave the count when their entry point returns). */
int64_t nnrt_device_bytes_in_use(void);
/* Pixel-node Jacobian arithmetic of this build: 0 = the reference CPU path's unfused expressions (the product), 1 = FMA
 * form (a development build, -DNNRT_JAC_FMA=1). Both are the reference's expression (PixelVertexAnchorJacobiansImpl.h
 * :179-363, WarpedSurfaceJacobiansImpl.h:117-156); the test checker selects its matching mode from this. */
int32_t nnrt_build_jacobian_fma(void);
/* The arrowhead solve's refinement floor of this build (NNRT_REFINE_PIVOT_FLOOR): no refinement step below this corner
 * pivot / diag(S) ratio. */
float nnrt_build_refine_floor(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Warp field -- replaces nnrt::geometry::HierarchicalGraphWarpField (cpp/geometry/HierarchicalGraphWarpField.h:37-97,
 * cpp/geometry/HierarchicalGraphWarpField.cpp:37-313) and the exported GraphWarpField accessors
 * (cpp/pybind/geometry/geometry.cpp:278-320). Node state lives on the device in virtual (hierarchy) order.
 * h_layer_radii may be NULL (default radius (i+1) * node_coverage, HierarchicalGraphWarpField.h:46-47).
 * ------------------------------------------------------------------------------------------------------------- */
nnrt_status nnrt_warp_field_create(const float* h_nodes, int32_t node_count, float node_coverage, int32_t threshold_nodes_by_distance,
                                   int32_t anchor_count, int32_t minimum_valid_anchor_count, int32_t coverage_method,
                                   int32_t layer_count, int32_t max_vertex_degree, const float* h_layer_radii, int32_t device,
                                   nnrt_warp_field** out);
void nnrt_warp_field_destroy(nnrt_warp_field* warp_field);
int32_t nnrt_warp_field_node_count(const nnrt_warp_field* warp_field);
int32_t nnrt_warp_field_edge_count(const nnrt_warp_field* warp_field);
/* layer sizes (fine -> coarse) into h_counts[layer_count]; returns layer_count */
int32_t nnrt_warp_field_layer_counts(const nnrt_warp_field* warp_field, int32_t* h_counts);
/* HierarchicalGraphWarpField::GetVirtualNodeIndices (:206-208): h_out[N] int64 (virtual -> original) */
nnrt_status nnrt_warp_field_get_virtual_node_indices(const nnrt_warp_field* warp_field, int64_t* h_out);
/* GetEdges / GetEdgeLayerIndices (:201-228): h_edges[E,2] int32 virtual indices, h_edge_layers[E] int8 (either may be NULL) */
nnrt_status nnrt_warp_field_get_edges(const nnrt_warp_field* warp_field, int32_t* h_edges, int8_t* h_edge_layers);
/* GetNodePositions/Rotations/Translations(use_virtual_ordering) (:210-224) and Set/Translate/Rotate counterparts. */
nnrt_status nnrt_warp_field_get_node_positions(const nnrt_warp_field* warp_field, float* h_out, int32_t virtual_order);
nnrt_status nnrt_warp_field_get_node_rotations(const nnrt_warp_field* warp_field, float* h_out, int32_t virtual_order);
nnrt_status nnrt_warp_field_get_node_translations(const nnrt_warp_field* warp_field, float* h_out, int32_t virtual_order);
nnrt_status nnrt_warp_field_set_node_rotations(nnrt_warp_field* warp_field, const float* h_in, int32_t virtual_order);
nnrt_status nnrt_warp_field_set_node_translations(nnrt_warp_field* warp_field, const float* h_in, int32_t virtual_order);
/* Resets every node to the identity motion on `stream`: R = I (as WarpField::ResetRotations, WarpField.cpp:151-156) and t = 0. */
nnrt_status nnrt_warp_field_reset_motion(nnrt_warp_field* warp_field, void* stream);
/* node coverage weights (MINIMAL_K_NEIGHBOR_NODE_DISTANCE, WarpField.cpp:249-263), virtual order */
nnrt_status nnrt_warp_field_get_node_coverage_weights(const nnrt_warp_field* warp_field, float* h_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Fitter -- replaces nnrt::alignment::DeformableMeshToImageFitter (cpp/alignment/DeformableMeshToImageFitter.h:34-91,
 * .cpp:56-448). Parameters mirror the constructor (.h:34-46).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct nnrt_fitter_params {
	int32_t max_iteration_count;            /* 100 */
	int32_t iteration_mode_count;           /* 1 */
	int32_t iteration_modes[16];            /* {NNRT_ITERATION_ALL} */
	float minimal_update_threshold;         /* 1e-6 (never effective in the reference: A14; step control gives it effect) */
	int32_t use_perspective_correction;     /* 1 */
	float max_depth;                        /* 10 */
	int32_t use_tukey_penalty_for_data_term;/* 0 */
	float tukey_penalty_cutoff_cm;          /* 0.01 */
	float preconditioning_dampening_factor; /* 0 ; must be in [0, 1] */
	float arap_term_weight;                 /* 200 */
	int32_t use_huber_penalty_for_arap_term;/* 0 */
	float huber_penalty_constant;           /* 1e-4 */
	int32_t use_hip_graph;                  /* NNRT_GRAPH_AUTO (1, default): an iteration sequence runs eagerly the first
	                                           time it is requested after (re)preparation and is captured into a hipGraph
	                                           and replayed from its second request on; NNRT_GRAPH_ALWAYS (2): captured on
	                                           first use; NNRT_GRAPH_NEVER (0): always eager launches */
	int32_t ndc_convention;                 /* NNRT_NDC_REFERENCE (0): the reference's image-space -> NDC mapping, whose
	                                           rendered points are y-mirrored about cy (CoordinateSystemConversions.h:
	                                           130-136); NNRT_NDC_CONSISTENT (1): raster pixel (u, v) is pixel (u, v) of K, for
	                                           fitting real depth frames (a deliberate divergence) */
} nnrt_fitter_params;
#define NNRT_NDC_REFERENCE 0
#define NNRT_NDC_CONSISTENT 1
#define NNRT_GRAPH_NEVER 0
#define NNRT_GRAPH_AUTO 1
#define NNRT_GRAPH_ALWAYS 2

void nnrt_fitter_default_params(nnrt_fitter_params* params);
nnrt_status nnrt_fitter_create(const nnrt_fitter_params* params, int32_t device, nnrt_fitter** out);
void nnrt_fitter_destroy(nnrt_fitter* fitter);

/* FitToImage(warp_field, canonical_mesh, color, depth, mask, K, E, depth_scale) (DeformableMeshToImageFitter.cpp:278-314).
 * d_depth: float32 [H,W] metric depth * depth_scale; d_mask: uint8 [H,W] or NULL; h_K: float64[9]; h_E: float64[16] or
 * NULL (identity). Mutates the warp field's rotations/translations in place. */
nnrt_status nnrt_fitter_fit_to_image(nnrt_fitter* fitter, nnrt_warp_field* warp_field, const float* d_vertices, const float* d_normals,
                                     int64_t vertex_count, const int64_t* d_faces, int64_t face_count, const float* d_depth,
                                     const uint8_t* d_mask, int32_t height, int32_t width, const double* h_K, const double* h_E,
                                     float depth_scale, void* stream);
/* The same call split in two for benchmarking / streaming use: prepare() runs the once-per-frame setup of
 * FitToImage (:96-106: anchors, NDC intrinsics, face<->anchor association, reference point cloud); iterate() runs
 * `count` GN iterations (loop body :111-275) starting at iteration index `first_iteration` (selects the mode). */
nnrt_status nnrt_fitter_prepare(nnrt_fitter* fitter, nnrt_warp_field* warp_field, const float* d_vertices, const float* d_normals,
                                int64_t vertex_count, const int64_t* d_faces, int64_t face_count, const float* d_depth,
                                const uint8_t* d_mask, int32_t height, int32_t width, const double* h_K, const double* h_E,
                                float depth_scale, void* stream);
/* The per-frame wave -> 8 x 8 quadrant table of the fitter's pixel launch, as prepare() builds it for launches of one
 * residency round (development / tests). Quadrants are numbered tile-major: 16 x 16 tiles in raster order, then the
 * four quadrants of a tile (x fastest); quadrants = 4 * ceil(W / 16) * ceil(H / 16). The table has
 * 4 * nnrt_fit_quad_order_blocks(quadrants) entries in 8 equal bands (one per XCD): a band's share of the quadrants
 * with a valid pixel first, then its share of the others, then the value `quadrants` as padding. A band holding more
 * quadrants with valid pixels than slots / 8 moves the excess, those with the fewest valid pixels, to the end of that
 * run. h_valid: [H*W] uint8 (host); h_counts: [quadrants] valid pixels per quadrant; h_table: the table (host). */
int32_t nnrt_fit_quad_order_blocks(int32_t quadrants);
nnrt_status nnrt_fit_quad_order_table(const uint8_t* h_valid, int32_t height, int32_t width, int32_t slots, int32_t* h_counts,
                                      int32_t* h_table);
/* FitToImage(warp_field, canonical_mesh, color, reference_point_cloud, reference_point_mask, K, E, rendering_image_size)
 * (DeformableMeshToImageFitter.cpp:85-276, the overload the depth variant forwards to): d_points float32 [H*W,3]
 * organized reference points, d_point_mask uint8 [H*W] or NULL (all valid), (height, width) = rendering image size. */
nnrt_status nnrt_fitter_prepare_point_cloud(nnrt_fitter* fitter, nnrt_warp_field* warp_field, const float* d_vertices,
                                            const float* d_normals, int64_t vertex_count, const int64_t* d_faces, int64_t face_count,
                                            const float* d_points, const uint8_t* d_point_mask, int32_t height, int32_t width,
                                            const double* h_K, const double* h_E, void* stream);
nnrt_status nnrt_fitter_fit_to_point_cloud(nnrt_fitter* fitter, nnrt_warp_field* warp_field, const float* d_vertices,
                                           const float* d_normals, int64_t vertex_count, const int64_t* d_faces, int64_t face_count,
                                           const float* d_points, const uint8_t* d_point_mask, int32_t height, int32_t width,
                                           const double* h_K, const double* h_E, void* stream);
/* Iterations are enqueued on `stream` itself. With use_hip_graph the `count` iterations (up to 64 per launch) are
 * captured once as one graph per mode sequence and replayed on `stream` as a single launch. */
nnrt_status nnrt_fitter_iterate(nnrt_fitter* fitter, nnrt_warp_field* warp_field, int32_t first_iteration, int32_t count, void* stream);
/* Benchmark / diagnostic form of iterate(): every iteration first resets the warp field's motion to the identity
 * (R = I, t = 0, as nnrt_warp_field_reset_motion), so each is the first GN iteration of the prepared frame. Same
 * graph behaviour as iterate() (the resets are captured with the iterations). */
nnrt_status nnrt_fitter_iterate_from_identity(nnrt_fitter* fitter, nnrt_warp_field* warp_field, int32_t first_iteration, int32_t count,
                                              void* stream);
/* Number of instantiated iteration-sequence graphs the fitter holds (diagnostic for the use_hip_graph policy). */
int32_t nnrt_fitter_graph_count(const nnrt_fitter* fitter);
/* Schur-corner plan of the prepared frame's arrowhead solve (diagnostic; zeros without ARAP): h_out[6] = corner nodes,
 * 64-unknown tile columns, factorization launches (elimination-tree levels), back-substitution launches, stored
 * (structurally non-zero) tiles, lower tiles of the dense corner. */
nnrt_status nnrt_fitter_corner_info(const nnrt_fitter* fitter, int64_t* h_out);
/* h_out[0..count): tile_order, quad_order, pix_low_occupancy, anchors16, warp_vertex, raster_dense (0/1) of the
   last prepared frame; count must be >= 6 (NNRT_ERROR_ARGUMENT otherwise, and before prepare). */
nnrt_status nnrt_fitter_launch_plan(const nnrt_fitter* fitter, int32_t* h_out, int64_t count);
/* Work of that plan's factorization as executed (diagnostic; zeros without ARAP): h_out[3] = MFMA flops per
 * factorization (every update term's 64 x 64 x 64 tile product + the rank-32 products of the split eliminations),
 * update terms, tile-column eliminations (real columns summed). The reference's dense count is (6 n1)^3 / 3 + ... */
nnrt_status nnrt_fitter_corner_work(const nnrt_fitter* fitter, int64_t* h_out);
/* The last iteration's warped canonical mesh (diagnostic; synchronizes `stream`): h_positions / h_normals [V,3] as the
 * fitter rasterized them (Warping.cpp:222-264 of the motion the iteration started from). */
nnrt_status nnrt_fitter_get_warped_mesh(nnrt_fitter* fitter, float* h_positions, float* h_normals, int64_t vertex_count, void* stream);
/* The last ARAP iteration's float arrowhead system exactly as the fitter factored and refined it (diagnostic; synchronizes
 * `stream`; virtual node order): h_diag [N,36] diagonal blocks (data + ARAP + LM), h_wing [E,36] wing blocks (block (i, j)
 * of edge e = (i, j), its transpose at (j, i)), h_rhs [6N] right-hand side (negative gradient). The reference holds the
 * same system between ComputeArapHessian and SolveBlockSparseArrowheadCholesky (DeformableMeshToImageFitter.cpp:223-247). */
nnrt_status nnrt_fitter_get_arrowhead_system(nnrt_fitter* fitter, float* h_diag, float* h_wing, float* h_rhs, int64_t node_count,
                                             int64_t edge_count, void* stream);
/* The last arrowhead solve's refinement gate (diagnostic; synchronizes `stream`): h_out[5] = the corner factorization's
 * smallest pivot / diag(S) ratio (1 without ARAP), the threshold below which one step of iterative refinement runs (it
 * does not below the build's floor, 1e-5, where one step is not relied on), 1 if it ran, the step's max |d| / max |x|
 * and 1 if its safeguard accepted it (max |d| <= 1e-2 max |x|; else the plain solve stands). */
nnrt_status nnrt_fitter_refine_info(nnrt_fitter* fitter, float* h_out, void* stream);
/* Threshold of the refinement gate (default 1e-2): the arrowhead solve refines when the corner's smallest pivot /
 * diag(S) ratio falls below it (and is at least 1e-5); 0 never refines. Drops the fitter's cached graphs (a launch
 * argument). */
nnrt_status nnrt_fitter_set_refine_ratio(nnrt_fitter* fitter, float ratio);
/* Robust options (both off by default: the reference's arithmetic, NaN for NaN). They are launch arguments, so the
 * setter drops the fitter's cached graphs; the prepared frame stays. Any other value of either argument is
 * NNRT_ERROR_ARGUMENT, nnrt_last_error() naming the argument.
 *  penalty_form: the form of the penalties that use_tukey_penalty_for_data_term / use_huber_penalty_for_arap_term
 *   enable (no effect on a square term). NNRT_PENALTY_REFERENCE: the reference's branches as written.
 *   NNRT_PENALTY_IRLS: iteratively re-weighted least squares.
 *    Data term, Tukey's biweight: r = n_l . (w_l - o_l), c = tukey_penalty_cutoff_cm; a pixel contributes iff it is
 *    masked in and |r| <= c; q = r / c, s = 1 - q q (the square root of the weight (1 - q^2)^2); residual s r (0 where
 *    the pixel does not contribute), Jacobian row s J: H = sum s^2 J^T J, g = sum (s J)^T (s r).
 *    ARAP term, Huber's weight on the edge's residual 3-vector r: n = |r|, delta = huber_penalty_constant,
 *    s = 1 if n <= delta else sqrt(delta / n); the edge's residual and Jacobian terms are multiplied by s.
 *  guard_zero_rotation: 1 = a node whose rotation update has angle exactly 0 (every node without pixels under the
 *   block-diagonal solve) keeps its rotation; its translation update is applied as usual. 0: Rodrigues' 0 / 0 makes that
 *   node's rotation NaN, as in the reference. nnrt_axis_angle_to_matrices_rodrigues is not affected. */
#define NNRT_PENALTY_REFERENCE 0
#define NNRT_PENALTY_IRLS 1
nnrt_status nnrt_fitter_set_robust_options(nnrt_fitter* fitter, int32_t penalty_form, int32_t guard_zero_rotation);
nnrt_status nnrt_fitter_get_robust_options(const nnrt_fitter* fitter, int32_t* penalty_form, int32_t* guard_zero_rotation);
/* Coupling of the data term across nodes. NNRT_DATA_BLOCK_DIAGONAL (default): the reference's
 * data Hessian, one 6x6 block per node, bit for bit. NNRT_DATA_COUPLED: the full Gauss-Newton step -- every
 * pair (a, b), a < b, of nodes that anchor vertices of one face gets the off-diagonal block sum over the face's
 * contributing pixels of J_a^T J_b (with the IRLS scale where it is on), united with the ARAP wing blocks, and the whole
 * system is factored by the tile-sparse solver (arrow base 0). Real sequences should use it: the block-diagonal step
 * overshoots from its second iteration on. IterationMode ALL only: a fitter whose mode list holds
 * another mode refuses NNRT_DATA_COUPLED with NNRT_ERROR_ARGUMENT; any other value is NNRT_ERROR_ARGUMENT too,
 * nnrt_last_error() naming the argument. A change drops the fitter's cached graphs AND invalidates the prepared frame
 * (the pair structure and the solver plan over it are built in prepare(), with one host round trip): prepare() must be
 * called again before the next iterate(). A singular system (lambda = 0 and a node without pixels or edges) is reported by
 * nnrt_fitter_check as NNRT_ERROR_NOT_POSITIVE_DEFINITE. */
#define NNRT_DATA_BLOCK_DIAGONAL 0
#define NNRT_DATA_COUPLED 1
nnrt_status nnrt_fitter_set_data_coupling(nnrt_fitter* fitter, int32_t data_coupling);
nnrt_status nnrt_fitter_get_data_coupling(const nnrt_fitter* fitter, int32_t* data_coupling);
/* Node pairs of the prepared frame's coupled system (0 in block-diagonal mode or without a prepared frame; -1: null). */
int64_t nnrt_fitter_coupled_pair_count(const nnrt_fitter* fitter);
/* The last coupled iteration's float system exactly as the fitter factored it (diagnostic; synchronizes `stream`; virtual
 * node order), the counterpart of nnrt_fitter_get_arrowhead_system: h_diag [N,36] diagonal blocks (data + ARAP + LM),
 * h_pairs [M,2] the pairs (i, j), i < j, ascending, h_blocks [M,36] block (i, j) of each pair (its transpose at (j, i)),
 * h_rhs [6N] right-hand side (negative gradient). node_count / pair_count must equal the prepared frame's. */
nnrt_status nnrt_fitter_get_coupled_system(nnrt_fitter* fitter, float* h_diag, int32_t* h_pairs, float* h_blocks, float* h_rhs,
                                           int64_t node_count, int64_t pair_count, void* stream);
/* Step control, off by default: with it off every launch, the launch plan, the graph count and
 * every output are what they were. With it on, every iteration forms the total cost c of the state it starts from (the
 * fp64 sum over the residual mask of the squared float residuals, plus the squared ARAP edge residuals with a hierarchy;
 * per-workgroup partial sums in a fixed order, then one lane sums the partials in index order: no atomics on the sum, a
 * graph replay equals the eager run) and decides ON THE DEVICE, so an iteration stays one fixed sequence of launches:
 *   done already                         NNRT_STEP_HOLD
 *   first iteration, or after a reject   NNRT_STEP_START   c_best = c, best motion = current, lambda unchanged, step
 *   c <= c_best                          best motion = current, then: (c_best - c) <= relative_cost_tolerance * c_best:
 *                                        NNRT_STEP_CONVERGED (done, hold); else NNRT_STEP_ACCEPT, lambda =
 *                                        max(lambda * decrease, lambda_min), step; c_best = c in both
 *   anything else (a non-finite c too)   NNRT_STEP_REJECT  lambda = min(lambda * increase, lambda_max), hold; the next
 *                                        iteration re-linearises the restored best state under the larger lambda (a
 *                                        rejection costs two iterations). lambda already at lambda_max:
 *                                        NNRT_STEP_REJECT_FINAL, done
 * The solve launches read lambda from the device. At the end of the iteration a held iteration puts the best motion back
 * (the solve's update is discarded, and so are the error bits it raised: the error word is saved at the decision and
 * restored); a stepping iteration whose max |update| is below minimal_update_threshold puts the best motion back and is
 * done (NNRT_STEP_SMALL_UPDATE): the one mode in which that parameter has an effect (A14). Every iteration appends one
 * nnrt_step_record to a ring of NNRT_STEP_HISTORY_CAPACITY records. nnrt_fitter_iterate with first_iteration == 0
 * restarts the state machine (lambda = initial_lambda, empty history).
 * Limits: IterationMode ALL only, and SQUARE penalties only under NNRT_STEP_OBJECTIVE_SQUARE (the default step objective;
 * nnrt_fitter_set_step_objective below lifts this) -- under NNRT_PENALTY_IRLS the residual buffer holds the scaled
 * residual s r, from which the robust objective cannot be evaluated. Under NNRT_STEP_OBJECTIVE_SQUARE, enabling step
 * control while NNRT_PENALTY_IRLS is set, or
 * setting NNRT_PENALTY_IRLS while step control is on, returns NNRT_ERROR_ARGUMENT; so does
 * a mode list holding another mode than ALL, and nnrt_fitter_iterate_from_identity / _from_snapshot (every iteration a
 * restart) while it is on. An ARAP edge the fixed-coverage weight lookup refuses (quirk A3, error bit 2 of
 * nnrt_fitter_check) contributes 0 to the cost; that fit is reported as failed anyway.
 *  initial_lambda: 0 = preconditioning_dampening_factor; either is clamped into [lambda_min, lambda_max] (a lambda of 0
 *   never grows: give lambda_min > 0). increase > 1; 0 < decrease <= 1; 0 <= lambda_min <= lambda_max, lambda_max > 0;
 *   relative_cost_tolerance >= 0; poll_interval >= 0: k > 0 makes nnrt_fitter_fit_to_image / _to_point_cloud synchronise
 *   after every k iterations and return once the device reports done; 0 (default) never synchronises, the held
 *   iterations then re-evaluate the frozen state. Values outside these ranges (NaN included) are NNRT_ERROR_ARGUMENT,
 *   nnrt_last_error() naming the field. settings == NULL turns the mode off. A change drops the fitter's cached graphs (as
 *   nnrt_fitter_set_data_coupling does) and invalidates the prepared frame: prepare() again before iterating. */
typedef struct nnrt_step_control {
	float initial_lambda;
	float increase;
	float decrease;
	float lambda_min;
	float lambda_max;
	float relative_cost_tolerance;
	int32_t poll_interval;
} nnrt_step_control;
typedef struct nnrt_step_record {
	double cost;        /* c of the state the iteration started from */
	float lambda;       /* the damping the iteration's solve used (after the decision) */
	float max_update;   /* max |update| of a stepping iteration (+inf if an update is not finite); 0 on a held one */
	int32_t decision;   /* NNRT_STEP_* */
	int32_t iteration;  /* index since the restart */
} nnrt_step_record;
#define NNRT_STEP_HOLD 0
#define NNRT_STEP_START 1
#define NNRT_STEP_ACCEPT 2
#define NNRT_STEP_CONVERGED 3
#define NNRT_STEP_REJECT 4
#define NNRT_STEP_REJECT_FINAL 5
#define NNRT_STEP_SMALL_UPDATE 6
#define NNRT_STEP_HISTORY_CAPACITY 256
nnrt_status nnrt_fitter_set_step_control(nnrt_fitter* fitter, const nnrt_step_control* settings);
/* *enabled = 0 / 1; *settings (nullable) receives the settings as held (zeros when off). */
nnrt_status nnrt_fitter_get_step_control(const nnrt_fitter* fitter, int32_t* enabled, nnrt_step_control* settings);
/* The records of the iterations since the restart, oldest first (synchronizes `stream`): *out_count of them, at most
 * NNRT_STEP_HISTORY_CAPACITY (the most recent ones of a longer run). A `capacity` below that count is refused with
 * NNRT_ERROR_ARGUMENT, nothing written, as nnrt_fitter_get_warped_mesh refuses a wrong vertex count; *out_count is still
 * set, so records == NULL with capacity 0 asks for the count. 0 records with step control off. */
nnrt_status nnrt_fitter_get_step_history(nnrt_fitter* fitter, nnrt_step_record* records, int64_t capacity, int64_t* out_count, void* stream);
/* The cost step control compares. NNRT_STEP_OBJECTIVE_SQUARE (default): the sum of squares above,
 * with every refusal above. NNRT_STEP_OBJECTIVE_ROBUST: the objective the IRLS penalties minimise, in fp64, so that step
 * control and NNRT_PENALTY_IRLS are accepted together, set in either order:
 *   data term   every pixel of the residual mask, r = n_l . (w_l - o_l) its raw float residual before any scaling: r^2
 *               without the Tukey penalty; with it (c = tukey_penalty_cutoff_cm, q = r / c)
 *               (c^2 / 3) (1 - (1 - q^2)^3) if fabsf(r) <= c, else c^2 / 3 -- twice the biweight's rho, whose IRLS weight
 *               is the (1 - q^2)^2 of nnrt_fitter_set_robust_options; it tends to r^2 as c grows. A masked-in pixel whose
 *               r is not finite adds NaN (a reject), not the saturated c^2 / 3.
 *   state       a node translation or rotation entry of the evaluated state that is not finite makes the cost NaN: the
 *               faces such a node moves are not rendered, so their pixels leave the mask and no residual would show it.
 *   ARAP term   every edge, m^2 = the fp64 sum of squares of its three stored residual entries: m^2 without the Huber
 *               penalty; with it (delta = huber_penalty_constant) m^2 if m^2 <= delta^2, else 2 m^2 - delta^2 (the stored
 *               entries carry the factor sqrt(delta / n), so this is 2 delta n - delta^2, twice Huber's rho). A refused
 *               edge (A3) adds 0.
 * The fused pixel launch keeps only s r, so one more launch per iteration (in k_step_cost's place, same partial sums,
 * ticket and decision) resolves every masked pixel again, bit for bit as that launch did, and leaves r in a [P] buffer:
 * nnrt_fitter_get_raw_residuals. With both penalties off and no hierarchy the costs equal NNRT_STEP_OBJECTIVE_SQUARE's
 * bit for bit. Refused with NNRT_ERROR_ARGUMENT: any other value; ROBUST while the penalty form is NNRT_PENALTY_REFERENCE
 * and a penalty is enabled (the reference's branches A8 / A9 have no objective; nnrt_fitter_set_robust_options refuses the
 * reverse order); SQUARE while step control is on and NNRT_PENALTY_IRLS is set. A change drops the fitter's cached graphs
 * and, with step control on, invalidates the prepared frame (prepare() again: the state machine restarts). With the
 * objective at SQUARE, or step control off, the launch plan, the graph count and every output are what they were. */
#define NNRT_STEP_OBJECTIVE_SQUARE 0
#define NNRT_STEP_OBJECTIVE_ROBUST 1
nnrt_status nnrt_fitter_set_step_objective(nnrt_fitter* fitter, int32_t objective);
nnrt_status nnrt_fitter_get_step_objective(const nnrt_fitter* fitter, int32_t* objective);
/* The raw residuals r of the last iteration under step control with NNRT_STEP_OBJECTIVE_ROBUST (0 outside the residual
 * mask; zeros before the first iteration), h_out [count] floats on the host. count must equal the prepared image's H * W;
 * without such a prepared frame NNRT_ERROR_ARGUMENT. Synchronizes `stream`. */
nnrt_status nnrt_fitter_get_raw_residuals(nnrt_fitter* fitter, float* h_out, int64_t count, void* stream);
/* Landmark term: `count` sparse 3-D correspondences for the next fit. Landmark l ties canonical vertex
 * d_vertex_indices[l] (int32, device) to the camera-space point d_targets[3 l .. 3 l + 2] (float, device) with weight
 * d_weights[l] >= 0 (device; NULL: all 1). With v' the warped vertex, d = v' - q, the residual is
 * r = term_weight * weight * d in R^3; the landmark is active iff weight > 0, q is finite and (cutoff <= 0 or |d| <= cutoff,
 * metres); its cost is |r|^2 when active, (term_weight weight cutoff)^2 when the cutoff dropped it, 0 otherwise (a
 * truncated quadratic, whose IRLS weight the gate is). Active landmarks add J^T J and J^T r to the blocks of the vertex's
 * anchor nodes (and, under NNRT_DATA_COUPLED, J_a^T J_b to the blocks of their pairs) in every iteration, on all three
 * solve paths, and their cost to what step control compares (both objectives). The arrays are copied on `stream`.
 * count == 0 clears the landmarks (the pointers are then ignored). The ranges are checked before anything else:
 * term_weight must be finite and > 0, cutoff finite. IterationMode ALL only (another mode in the fitter's list:
 * NNRT_ERROR_ARGUMENT). The landmarks take effect at the next prepare(), which refuses (NNRT_ERROR_ARGUMENT, naming the
 * landmark) a vertex index outside the mesh or a vertex no face references; the call invalidates the prepared frame.
 * The same count, term_weight and cutoff as before keep the captured graphs; a change of any, or a clear, drops them.
 * A fitter without landmarks launches what it launched before this term existed. term_weight's default of 1 is untuned.
 * count < 2^24 is the addressing limit, not a tuned range: one wave writes the distances and sums the cost, 64 landmarks per
 * pass, which suits the hundreds to few thousands of matches a frame yields; nothing larger has been measured. */
nnrt_status nnrt_fitter_set_landmarks(nnrt_fitter* fitter, const int32_t* d_vertex_indices, const float* d_targets, const float* d_weights,
                                      int64_t count, float term_weight, float cutoff, void* stream);
/* h_out [4 * count] floats on the host: per landmark (d.x, d.y, d.z, active as 0 / 1) as of the state the last iteration
 * started from (zeros before the first). count must equal the number of landmarks set (a mismatch is refused, not written
 * past). Synchronizes `stream`. */
nnrt_status nnrt_fitter_get_landmark_distances(nnrt_fitter* fitter, float* h_out, int64_t count, void* stream);
/* h_out[0..3] = landmarks set, and of the prepared frame: their (node, landmark, slot) associations, the runs of equal
 * nodes among them, and their (pair, landmark, slot, slot) associations (0 outside NNRT_DATA_COUPLED); zeros for a frame
 * that is not prepared. out_count: the room in h_out, at least 4. */
nnrt_status nnrt_fitter_landmark_info(const nnrt_fitter* fitter, int64_t* h_out, int64_t out_count);
/* Anchor the canonical mesh along a motion graph's edges instead of by Euclidean distance (the reference's
 * AnchorComputationMethod::SHORTEST_PATH, PlanarGraphWarpField::PrecomputeAnchorsAndWeights; apps/fusion/pipeline.py:577-582):
 * d_edges [node_count, graph_degree] int32 rows in the warp field's virtual node order (entry < 0 = empty) are copied
 * into the fitter, and every later prepare() / prepare_point_cloud() computes its anchors with
 * nnrt_compute_anchors_and_weights_shortest_path (the warp field's node weights when its coverage is variable). An
 * entry >= node_count is refused here; prepare() refuses a node_count that differs from the warp field's.
 * d_edges == NULL returns to Euclidean anchors. Drops the fitter's cached graphs and the prepared frame (prepare()
 * again before iterating). Synchronizes `stream`. */
nnrt_status nnrt_fitter_set_anchor_graph(nnrt_fitter* fitter, const int32_t* d_edges, int32_t node_count, int32_t graph_degree,
                                         void* stream);
/* Store the warp field's current node motion (R, t) in the fitter (a device copy on `stream`). */
nnrt_status nnrt_fitter_snapshot_motion(nnrt_fitter* fitter, nnrt_warp_field* warp_field, void* stream);
/* Benchmark form of iterate() that runs the general (non-identity) kernels: before every iteration the warp field's
 * node motion is restored from the snapshot by a device copy (captured into the graph with the iteration), so each
 * iteration is the same GN iteration k of the frame (the state it was taken at). Requires nnrt_fitter_snapshot_motion
 * after the last prepare(). */
nnrt_status nnrt_fitter_iterate_from_snapshot(nnrt_fitter* fitter, nnrt_warp_field* warp_field, int32_t first_iteration, int32_t count,
                                              void* stream);
/* A whole frame fit (the FitToImage loop, :111-275) from the stored snapshot: the node motion is restored once, then
 * iterations 0 .. count-1 run (graph-captured as one sequence under the use_hip_graph policy). */
nnrt_status nnrt_fitter_fit_from_snapshot(nnrt_fitter* fitter, nnrt_warp_field* warp_field, int32_t count, void* stream);
/* Restore the warp field's node motion from the snapshot (a device copy on `stream`). */
nnrt_status nnrt_fitter_restore_motion(nnrt_fitter* fitter, nnrt_warp_field* warp_field, void* stream);
/* iterate() without graphs, with HIP events between the stages of every iteration; h_stage_ms[NNRT_TIMED_STAGES]
 * receives the average per-iteration device time of: 0 warp (+warped Jacobians), 1 raster scatter, 2 pixel pass
 * (0: fused into 3), 3 pixel + node pass (residuals, rasterized Jacobians, node Jacobians, JtJ / Jt r: one launch,
 * k_fit_pixels_fused), 4 ARAP edges, 5 linear solve + update ("ms/solve"). Synchronizes `stream`. */
#define NNRT_TIMED_STAGES 6
nnrt_status nnrt_fitter_iterate_timed(nnrt_fitter* fitter, nnrt_warp_field* warp_field, int32_t first_iteration, int32_t count,
                                      float* h_stage_ms, void* stream);
/* Per-kernel device time of one GN iteration in its real context (measurement; loop body
 * DeformableMeshToImageFitter.cpp:111-275). Four prefix sequences of `reps` iterations from the snapshot state are each
 * captured as one graph -- [warp, raster, pixel, solve], [raster, pixel, solve], [raster, pixel], [raster] -- and
 * replayed `trials` times, interleaved, between HIP events on the fitter's stream; the median per-iteration times give
 * h_kernel_ms[NNRT_KERNEL_TIMES] = 0 warp (k_warp_mesh_quad), 1 raster (k_raster_scatter_mesh), 2 fused pixel launch
 * (k_fit_pixels_fused), 3 solve + update (k_solve_update; ARAP: the whole arrowhead chain), 4 whole iteration, by
 * differences. Leaves raster keys empty, the accumulators zero and the node motion at the snapshot's one-iteration
 * result. Requires nnrt_fitter_snapshot_motion after the last prepare(). Synchronizes `stream`. With step control on the
 * solve time includes its two launches; every replayed iteration restarts from the snapshot, so from the third on they
 * are held iterations (the node motion ends at the snapshot), and the state machine is restarted afterwards (empty
 * history, initial lambda): a fit in progress does not survive the timing. */
#define NNRT_KERNEL_TIMES 5
nnrt_status nnrt_fitter_time_kernels(nnrt_fitter* fitter, nnrt_warp_field* warp_field, int32_t reps, int32_t trials, float* h_kernel_ms,
                                     void* stream);
/* Reports (and clears) a failure recorded on the device by earlier iterate() calls (e.g. a non-positive-definite block,
 * which the reference raises from potrf). Synchronizes `stream`. */
nnrt_status nnrt_fitter_check(nnrt_fitter* fitter, void* stream);
/* Diagnostics of the most recent iteration, copied to the host (any pointer may be NULL): residuals [H*W] float32,
 * residual mask [H*W] uint8, rasterized face per pixel [H*W] int32 (-1 = none), motion updates [N*s] (s = 6 for ALL,
 * 3 otherwise), negative gradient [N*s], data-term Hessian blocks [N*s*s]. Synchronizes `stream`. */
nnrt_status nnrt_fitter_get_diagnostics(nnrt_fitter* fitter, float* h_residuals, uint8_t* h_residual_mask, int32_t* h_pixel_faces,
                                        float* h_updates, float* h_negative_gradient, float* h_hessian_blocks, void* stream);
/* Once-per-frame outputs of prepare(): anchors [V,K] int32 and weights [V,K] float32 (device -> host). */
nnrt_status nnrt_fitter_get_anchors(nnrt_fitter* fitter, int32_t* h_anchors, float* h_weights, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Stage entry points (parity surface; all device pointers, all asynchronous on `stream`)
 * ------------------------------------------------------------------------------------------------------------- */
/* nnrt.geometry.functional.compute_anchors_and_weights_euclidean_{fixed,variable}_node_weight
 * (cpp/pybind/geometry/functional/functional.cpp:52-90 -> WarpAnchorComputationImpl.h:42-140).
 * d_node_coverage_weights == NULL -> fixed coverage. */
nnrt_status nnrt_compute_anchors_and_weights(const float* d_points, int64_t point_count, const float* d_nodes, int32_t node_count,
                                             int32_t anchor_count, float node_coverage, const float* d_node_coverage_weights,
                                             int32_t minimum_valid_anchor_count, int32_t* d_anchors, float* d_weights, void* stream);
/* nnrt.geometry.functional.compute_anchors_and_weights_shortest_path_{fixed,variable}_node_weight
 * (cpp/pybind/geometry/functional/functional.cpp:63-73 -> WarpAnchorComputationImpl.h:146-237,
 * KnnUtilities_PriorityQueue.h:102-160, WarpUtilities.h:347-375): per point, K anchors in the order a 40-entry
 * min-queue over (path length, node) pops them, seeded with the Euclidean-nearest node that is no anchor yet and fed
 * along d_edges [node_count, graph_degree] int32 (entry < 0 = empty); seeded again whenever the queue runs dry.
 * Weights exp(-d^2 / (2 c^2)) of the path lengths, normalized; no distance threshold, no minimum valid count.
 * d_node_coverage_weights == NULL -> fixed coverage. Equal keys of two different nodes pop the lower index first. A
 * slot never filled (fewer than K reachable nodes) is anchor -1 with weight 0; a row without any anchor has weights
 * 1 / K. anchor_count in [1, 8], graph_degree >= 1, node_count >= 0. An edge entry >= node_count is refused
 * (NNRT_ERROR_ARGUMENT) before anything is written; that check synchronizes `stream`. */
nnrt_status nnrt_compute_anchors_and_weights_shortest_path(const float* d_points, int64_t point_count, const float* d_nodes,
                                                           int32_t node_count, const int32_t* d_edges, int32_t graph_degree,
                                                           int32_t anchor_count, float node_coverage,
                                                           const float* d_node_coverage_weights, int32_t* d_anchors, float* d_weights,
                                                           void* stream);
/* WarpTriangleMeshUsingSuppliedAnchors (cpp/geometry/functional/Warping.cpp:222-264). h_E may be NULL. */
nnrt_status nnrt_warp_mesh(const float* d_vertices, const float* d_normals, int64_t vertex_count, const float* d_nodes,
                           const float* d_rotations, const float* d_translations, int32_t node_count, const int32_t* d_anchors,
                           const float* d_weights, int32_t anchor_count, const double* h_E, float* d_out_vertices,
                           float* d_out_normals, void* stream);
/* nnrt.geometry.functional.warp_triangle_mesh (both overloads, threshold_nodes_by_distance / minimum_valid_anchor_count /
 * extrinsics) and warp_point_cloud (both overloads) (cpp/pybind/geometry/functional/functional.cpp:77-111 ->
 * cpp/geometry/functional/Warping.cpp:61-264 -> Warp3dPointsAndNormalsImpl.h:33-438, WarpUtilities.h:34-580).
 * d_normals / d_out_normals may be NULL (points only). d_anchors == NULL: anchors computed over d_nodes with the fixed
 * node_coverage (the online-anchor overloads); otherwise d_anchors int32 / d_weights float32 [count, anchor_count].
 * threshold_nodes_by_distance = 0: BlendWarp over the valid slots; 1: online anchors farther than 2 * node_coverage are
 * dropped and a point with fewer than minimum_valid_anchor_count valid anchors stays (0, 0, 0) (warp_point_cloud always
 * thresholds). h_E: float64[16] or NULL (identity). Outputs [count,3]. */
nnrt_status nnrt_warp_points(const float* d_points, const float* d_normals, int64_t count, const float* d_nodes, const float* d_rotations,
                             const float* d_translations, int32_t node_count, const int32_t* d_anchors, const float* d_weights,
                             int32_t anchor_count, float node_coverage, int32_t threshold_nodes_by_distance,
                             int32_t minimum_valid_anchor_count, const double* h_E, float* d_out_points, float* d_out_normals, void* stream);
/* nnrt.geometry.functional.compute_point_to_plane_distances(mesh1, mesh2 | point_cloud) (functional.cpp:118-125 ->
 * PointToPlaneDistances.cpp:25-90, kernel PointToPlaneDistancesImpl.h:26-50): d_out [count] = n1 . (v1 - v2). */
nnrt_status nnrt_compute_point_to_plane_distances(const float* d_normals1, const float* d_vertices1, const float* d_vertices2, int64_t count,
                                                  float* d_out, void* stream);
/* nnrt.geometry.functional.unproject_raster_depth_without_filtering(depth, intrinsics, extrinsics, depth_scale, depth_max,
 * preserve_pixel_layout) (functional.cpp:128-140 -> PerspectiveProjection.cpp:26-39, PerspectiveProjectionImpl.h:60-146):
 * depth uint16 (NNRT_DTYPE_UINT16) or float32 (NNRT_DTYPE_FLOAT32) [H,W]; points [H*W,3] in the frame of
 * extrinsics^-1 (h_E float64[16] or NULL = identity), zero where rejected; d_mask uint8 [H*W]. The pixel layout of the
 * outputs is the same either way (preserve_pixel_layout is a shape, [H,W,3] vs [H*W,3]). */
nnrt_status nnrt_unproject_depth_image(const void* d_depth, int32_t depth_dtype, int32_t height, int32_t width, const double* h_K,
                                       const double* h_E, float depth_scale, float depth_max, float* d_points, uint8_t* d_mask, void* stream);
/* nnrt.rendering.functional.get_mesh_ndc_face_vertices_and_clip_mask([meshes], ...) (cpp/pybind/rendering/functional/
 * functional.cpp:36-44 -> ExtractFaceVertices.cpp:87-126): the meshes' faces concatenated in mesh order; h_vertex_sets /
 * h_face_sets are HOST arrays of mesh_count DEVICE pointers, h_face_counts the per-mesh face counts (the reference's
 * face_counts output). d_face_ndc [sum F,3,3], d_clip_mask [sum F]. */
nnrt_status nnrt_get_meshes_ndc_face_vertices_and_clip_mask(const float* const* h_vertex_sets, const int64_t* const* h_face_sets,
                                                            const int64_t* h_face_counts, int32_t mesh_count, const double* h_K,
                                                            int32_t height, int32_t width, float near_clip, float far_clip,
                                                            float* d_face_ndc, uint8_t* d_clip_mask, void* stream);
/* The same with the image -> NDC mapping chosen: NNRT_NDC_REFERENCE is the function above; NNRT_NDC_CONSISTENT puts pixel
 * (u, v) of K on the centre of raster pixel (u, v) with the image as the clip window (nnrt_fitter_params.ndc_convention),
 * which a render that is compared with a depth frame needs. That mapping does not mirror y, so it turns every face's
 * winding in NDC: a caller that culls back faces swaps two vertices of each face first, as the fitter does. Any other
 * ndc_convention is NNRT_ERROR_ARGUMENT. */
nnrt_status nnrt_get_meshes_ndc_face_vertices_and_clip_mask_in_convention(const float* const* h_vertex_sets, const int64_t* const* h_face_sets,
                                                                          const int64_t* h_face_counts, int32_t mesh_count, const double* h_K,
                                                                          int32_t height, int32_t width, float near_clip, float far_clip,
                                                                          int32_t ndc_convention, float* d_face_ndc, uint8_t* d_clip_mask,
                                                                          void* stream);
/* nnrt.rendering.functional.get_mesh_ndc_face_vertices_and_clip_mask (cpp/rendering/functional/ExtractFaceVertices.cpp:56-85).
 * d_face_ndc [F,3,3], d_clip_mask [F] uint8 (1 = keep). */
nnrt_status nnrt_get_mesh_ndc_face_vertices_and_clip_mask(const float* d_vertices, const int64_t* d_faces, int64_t face_count,
                                                          const double* h_K, int32_t height, int32_t width, float near_clip,
                                                          float far_clip, float* d_face_ndc, uint8_t* d_clip_mask, void* stream);
/* nnrt.rendering.rasterize_ndc_triangles (cpp/pybind/rendering/rendering.cpp:36-43 -> RasterizeNdcTriangles.cpp:33-129).
 * Outputs fragments: face [H,W,Kf] int64 (-1), depth [H,W,Kf], barycentrics [H,W,Kf,3], signed distance [H,W,Kf]
 * (-1 fill). d_clip_mask may be NULL. bin_size / max_faces_per_bin are accepted for signature parity; the MI355X
 * rasterizer does not need coarse bins (faces_per_pixel == 1: per-face scatter with a (depth, face) 64-bit atomic
 * minimum; faces_per_pixel > 1: per-pixel lists of the faces covering the pixel centre, replayed in ascending face
 * order through the reference's bounded queue). */
nnrt_status nnrt_rasterize_ndc_triangles(const float* d_face_ndc, const uint8_t* d_clip_mask, int64_t face_count, int32_t height,
                                         int32_t width, float blur_radius_pixels, int32_t faces_per_pixel, int32_t bin_size,
                                         int32_t max_faces_per_bin, int32_t perspective_correct_barycentric_coordinates,
                                         int32_t clip_barycentric_coordinates, int32_t cull_back_faces, int64_t* d_pixel_faces,
                                         float* d_pixel_depths, float* d_pixel_barycentrics, float* d_pixel_face_distances,
                                         void* stream);
/* nnrt.rendering.functional.interpolate_vertex_attributes (InterpolateFaceAttributesImpl.h:30-75): [H,W,Kf,C] */
nnrt_status nnrt_interpolate_face_attributes(const int64_t* d_pixel_faces, const float* d_barycentrics, int64_t pixel_count,
                                             int32_t faces_per_pixel, const float* d_face_attributes, int32_t channels,
                                             float* d_out, void* stream);
/* nnrt.geometry.functional.unproject_raster_depth_without_filtering (PerspectiveProjectionImpl.h:60-146), float32 depth */
nnrt_status nnrt_unproject_depth(const float* d_depth, int32_t height, int32_t width, const double* h_K, float depth_scale,
                                 float depth_max, float* d_points, uint8_t* d_mask, void* stream);
/* nnrt.backproject_depth_ushort(image_in, point_image_out, fx, fy, cx, cy, normalizer) (cpp/pybind/nnrt_pybind.cpp:52-57,
 * cpp/cpu/image_proc.cpp:275-302): uint16 depth [H,W] -> ordered point image d_points [H,W,3]; depth = d / normalizer,
 * (depth*(x-cx)/fx, depth*(y-cy)/fy, depth), zeros where depth <= 0 (the reference leaves those entries as allocated). */
nnrt_status nnrt_backproject_depth_ushort(const uint16_t* d_depth, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                                          float normalizer, float* d_points, void* stream);
/* nnrt.backproject_depth_float(image_in, point_image_out, fx, fy, cx, cy) (nnrt_pybind.cpp:66-67, image_proc.cpp:312-339): float
 * depth in metres [H,W] -> [H,W,3], as above with normalizer 1. */
nnrt_status nnrt_backproject_depth_float(const float* d_depth, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                                         float* d_points, void* stream);
/* nnrt.filter_depth(depth_image_in, depth_image_out, radius) / (depth_image_in, radius) (nnrt_pybind.cpp:97-104 ->
 * image_proc.cpp:837-887): zero-skipping median of a uint16 depth image [H,W]. For every pixel the values > 0 of the
 * (2 radius + 1)^2 window, clipped to the image, are put in ascending order; with n of them the output is the one of
 * index n / 2 (integer division: the upper median of an even count). The result is exact. Two deviations from the
 * reference: n == 0 gives 0 (the reference indexes an empty vector); with preserve_zero != 0 a pixel whose own value is
 * 0 stays 0, while preserve_zero == 0 keeps the reference's behaviour, in which a hole takes the median of its valid
 * neighbours and silhouettes grow by `radius`. 0 <= radius <= NNRT_DEPTH_FILTER_MAX_RADIUS; radius 0 copies the input.
 * NNRT_ERROR_ARGUMENT for a radius outside that range, a negative height or width, null images of a non-empty size, and
 * d_out == d_in (the stencil reads its neighbours). An empty image is no error. */
#define NNRT_DEPTH_FILTER_MAX_RADIUS 8
nnrt_status nnrt_filter_depth(const uint16_t* d_in, int32_t height, int32_t width, int32_t radius, int32_t preserve_zero, uint16_t* d_out,
                              void* stream);
/* Bilateral filter of a depth image, an edge-preserving smoother the reference does not have (its only depth filter is
 * filter_depth, nnrt_pybind.cpp:97-104 -> image_proc.cpp:837-887, above). d_in [H,W] uint16 (NNRT_DTYPE_UINT16) or
 * float32 (NNRT_DTYPE_FLOAT32), d_out [H,W] float32. The weights are two host tables, copied to the device on `stream`
 * ahead of the launch: h_spatial_weights (2 radius + 1)^2 floats, row-major over (dy, dx); h_range_weights
 * range_weight_count floats. float32 arithmetic in this order: c = float(in[y][x]); a value is invalid unless it is
 * > 0 and finite, and an invalid pixel gives 0. Otherwise, over dy = -radius..radius (outer) and dx = -radius..radius
 * (inner), skipping positions outside the image: v = float(in[y+dy][x+dx]), skipped if invalid;
 * i = int(fabsf(v - c) * range_index_scale), truncated, skipped if i >= range_weight_count;
 * w = spatial[dy+radius][dx+radius] * range[i]; S_w = S_w + w; S_v = S_v + w * v. out = (S_v / S_w) / depth_scale if
 * S_w > 0, else 0. 0 <= radius <= NNRT_DEPTH_FILTER_MAX_RADIUS, 1 <= range_weight_count <=
 * NNRT_BILATERAL_MAX_RANGE_WEIGHTS. NNRT_ERROR_ARGUMENT, before anything is launched, for values outside those ranges,
 * a depth_scale or range_index_scale that is not finite and positive, null tables, a table entry that is negative or
 * not finite, an unknown dtype, a negative height or width, and null images of a non-empty size. */
#define NNRT_BILATERAL_MAX_RANGE_WEIGHTS 4096
nnrt_status nnrt_bilateral_filter_depth(const void* d_in, int32_t in_dtype, int32_t height, int32_t width, int32_t radius,
                                        const float* h_spatial_weights, const float* h_range_weights, int32_t range_weight_count,
                                        float range_index_scale, float depth_scale, float* d_out, void* stream);
/* Shaders: the front fragment (slot 0 of the faces_per_pixel slots) of every pixel of a rasterization -> d_out_pixels
 * [H,W,3] uint8 RGB. Every pixel is written; a pixel whose slot-0 face is negative is (0,0,0). Fragments as
 * nnrt_rasterize_ndc_triangles writes them: d_pixel_face_indices [H,W,K] int64, d_pixel_barycentric_coordinates
 * [H,W,K,3], d_pixel_face_distances [H,W,K]. Mesh data: d_triangle_indices [face_count,3] int64 over the joined meshes
 * (faces numbered as nnrt_get_meshes_ndc_face_vertices_and_clip_mask numbers them), d_vertex_colors and
 * d_vertex_normals [vertex_count,3] float32; the reference's gathered [F,3,3] face attributes are never formed. A face
 * index >= face_count or a vertex index outside [0, vertex_count) is drawn as background. byte(x) truncates the float32
 * product toward zero, with x <= 0 and NaN -> 0 and x >= 255 -> 255 (the reference's cast is undefined there). float32
 * arithmetic, unfused, in this order:
 *   NNRT_SHADE_VERTEX_COLOR  VertexColorShader::ShadeMeshes (cpp/rendering/VertexColorShader.cpp:29-61 over
 *     InterpolateFaceAttributesImpl.h:60-66): per channel a = 0; a += b0 c0; a += b1 c1; a += b2 c2; byte(a * 255).
 *   NNRT_SHADE_FLAT_EDGE     FlatEdgeShader (cpp/rendering/kernel/FlatEdgeShaderImpl.h:66-98, FlatEdgeShader.cpp:56-58,
 *     CoordinateSystemConversions.h:98-101): w = pixel_line_width / (min(H, W) / 2), w2 = w w, d = |distance|; if
 *     d < w2 every channel is byte(255 * color_c * ((w2 - d) / w2)), else 0. h_color [3] is the line colour.
 *   NNRT_SHADE_HEADLIGHT     (not in the reference) n = (b0 n0 + b1 n1) + b2 n2 of camera-space vertex normals,
 *     s = max(0, -n_z / |n|), 0 if |n| is 0 or not finite; byte(255 * color_c * (ambient + (1 - ambient) s)).
 * Refused on the host with NNRT_ERROR_ARGUMENT before any device work, naming the argument: an unknown mode, a negative
 * height, width, face_count or vertex_count, faces_per_pixel < 1, pixel_line_width <= 0 (FLAT_EDGE; the reference raises
 * there), ambient outside [0, 1] (HEADLIGHT), a null h_color (FLAT_EDGE, HEADLIGHT), null d_vertex_colors (VERTEX_COLOR)
 * or d_vertex_normals (HEADLIGHT) with vertex_count > 0, null d_triangle_indices with face_count > 0 (VERTEX_COLOR,
 * HEADLIGHT), and, for a non-empty image, a null fragment array the mode reads, a null d_out_pixels, or d_out_pixels
 * overlapping an input. height == 0 or width == 0 is no error and launches nothing. */
#define NNRT_SHADE_VERTEX_COLOR 0
#define NNRT_SHADE_FLAT_EDGE 1
#define NNRT_SHADE_HEADLIGHT 2
nnrt_status nnrt_shade_pixels(int32_t mode, const int64_t* d_pixel_face_indices, const float* d_pixel_barycentric_coordinates,
                              const float* d_pixel_face_distances, int32_t height, int32_t width, int32_t faces_per_pixel,
                              const int64_t* d_triangle_indices, int64_t face_count, const float* d_vertex_colors,
                              const float* d_vertex_normals, int64_t vertex_count, const float* h_color, float pixel_line_width,
                              float ambient, uint8_t* d_out_pixels, void* stream);
/* The rasterized model depth (slot 0 of d_pixel_depths [H,W,K], valid where d_pixel_face_indices [H,W,K] >= 0) against a
 * depth frame d_depth [H,W], uint16 (NNRT_DTYPE_UINT16) or float32 (NNRT_DTYPE_FLOAT32). A frame pixel is valid iff
 * z = raw / depth_scale (float32) satisfies 0 < z < depth_max, which NaN fails: the rule of nnrt_unproject_depth_image
 * (PerspectiveProjectionImpl.h:60-146). d_out_difference [H,W] float32 receives model - frame in metres, NaN where
 * either side is invalid. *h_out_statistics receives the counts of pixels valid on both sides, on the model's only and
 * on the frame's only, and over the pixels valid on both sides, with d the float32 difference: the count of
 * |d| <= inlier_threshold, the float64 sums of |d| and of |d|^2 and the largest |d|. The sums are reproducible (fixed
 * order, no atomics: DESIGN.md section 22). Synchronizes `stream`. Refused on the host with NNRT_ERROR_ARGUMENT before
 * any device work, naming the argument: a null h_out_statistics, a negative height or width, faces_per_pixel < 1, an
 * unknown depth_dtype, a depth_scale that is not finite and positive, a NaN depth_max, a negative or NaN
 * inlier_threshold, and, for a non-empty image, a null array or d_out_difference overlapping an input. height == 0 or
 * width == 0 is no error and launches nothing; the statistics are then all zero. */
typedef struct nnrt_depth_agreement {
	int64_t both, model_only, frame_only, inliers;
	double sum_abs, sum_sq;
	float max_abs;
	int32_t reserved;   /* 0 */
} nnrt_depth_agreement;
nnrt_status nnrt_compare_depth_to_raster(const int64_t* d_pixel_face_indices, const float* d_pixel_depths, int32_t height, int32_t width,
                                         int32_t faces_per_pixel, const void* d_depth, int32_t depth_dtype, float depth_scale,
                                         float depth_max, float inlier_threshold, float* d_out_difference,
                                         nnrt_depth_agreement* h_out_statistics, void* stream);
/* The motion field of a mesh between two states, as images on the source state's pixel grid. Slot 0
 * of the source state's fragments (d_pixel_face_indices [H,W,K] int64, d_pixel_barycentric_coordinates [H,W,K,3], the
 * barycentrics over the rows of d_triangle_indices [face_count,3] as given) selects, per pixel with face f >= 0, the
 * vertices (i0, i1, i2) and weights b. With S = d_source_positions [vertex_count,3] in the source camera's space and
 * T = d_target_positions [vertex_count,3] in the target camera's space, in float32, every product and sum rounded on its
 * own and in this order:
 *   p_s = (b0 S[i0] + b1 S[i1]) + b2 S[i2], p_t the same blend of T, pi(p) = ((fx x) / z + cx, (fy y) / z + cy)
 *   d_out_source_points [H,W,3] = p_s, d_out_scene_flow [H,W,3] = p_t - p_s, d_out_optical_flow [H,W,2] = pi(p_t) - pi(p_s)
 * A pixel is valid iff f >= 0, p_s.z > 0 and p_t.z > 0 (NaN fails); d_out_mask [H,W] is 1 there. Every other pixel gets
 * zeros in the three images and mask 0; so does a pixel whose face is >= face_count or has a vertex outside
 * [0, vertex_count). Every pixel is written. Asynchronous on `stream`. Refused on the host with NNRT_ERROR_ARGUMENT before
 * any device work, naming the argument: a negative height or width, faces_per_pixel < 1, a negative face_count or
 * vertex_count, an intrinsic that is not finite, null d_triangle_indices with face_count > 0, null d_source_positions or
 * d_target_positions with vertex_count > 0, and, for a non-empty image, a null fragment array or output, or an output
 * overlapping an input or another output. height == 0 or width == 0 is no error and launches nothing. */
nnrt_status nnrt_motion_pixels(const int64_t* d_pixel_face_indices, const float* d_pixel_barycentric_coordinates, int32_t height,
                               int32_t width, int32_t faces_per_pixel, const int64_t* d_triangle_indices, int64_t face_count,
                               const float* d_source_positions, const float* d_target_positions, int64_t vertex_count, float fx, float fy,
                               float cx, float cy, float* d_out_source_points, float* d_out_scene_flow, float* d_out_optical_flow,
                               uint8_t* d_out_mask, void* stream);
/* A predicted flow image d_predicted [H,W,C] with its mask d_predicted_mask [H,W] (valid where non-zero) against a truth
 * image d_truth [H,W,C], C = channels = 2 (optical flow, pixels) or 3 (scene flow, metres). A truth pixel is valid iff
 * d_truth_mask [H,W], which may be null, is non-zero there and all C channels are finite. Per pixel valid on both sides the
 * end-point error is e = sqrt(sum_c d_c^2) in float64 over the float32 differences d_c = predicted_c - truth_c, summed in
 * channel order. d_out_error [H,W] float32 receives e, NaN where either side is invalid. *h_out_statistics receives the
 * counts of pixels valid on both sides, on the prediction's only and on the truth's only, and over the pixels valid on
 * both sides: the count of e <= inlier_threshold, the float64 sums of e and of e e and the largest e as float32. The sums
 * are reproducible (fixed order, no atomics: DESIGN.md section 32). Synchronizes `stream`. Refused on the host with
 * NNRT_ERROR_ARGUMENT before any device work, naming the argument: a null h_out_statistics, a negative height or width,
 * channels other than 2 or 3, a negative or NaN inlier_threshold, and, for a non-empty image, a null array other than
 * d_truth_mask or d_out_error overlapping an input. height == 0 or width == 0 is no error and launches nothing; the
 * statistics are then all zero. */
typedef struct nnrt_flow_agreement {
	int64_t both, predicted_only, truth_only, inliers;
	double sum_epe, sum_sq;
	float max_epe;
	int32_t reserved;   /* 0 */
} nnrt_flow_agreement;
nnrt_status nnrt_flow_error(const float* d_predicted, const uint8_t* d_predicted_mask, const float* d_truth, const uint8_t* d_truth_mask,
                            int32_t height, int32_t width, int32_t channels, float inlier_threshold, float* d_out_error,
                            nnrt_flow_agreement* h_out_statistics, void* stream);
/* nnrt.geometry.functional.compute_triangle_normals(mesh, normalized=True) (cpp/geometry/functional/NormalsOperations.cpp:36-46,
 * kernel NormalsOperationsImpl.h:39-68): d_out [F,3] = (v1 - v0) x (v2 - v0), optionally normalized (zero stays zero,
 * NaN -> (0,0,1)) */
nnrt_status nnrt_compute_triangle_normals(const float* d_vertices, int64_t vertex_count, const int64_t* d_faces, int64_t face_count,
                                          int32_t normalized, float* d_out, void* stream);
/* nnrt.geometry.functional.compute_vertex_normals(mesh, normalized=True) (NormalsOperations.cpp:52-66, kernel :95-166): sum of the
 * unnormalized incident triangle normals, in ascending face order (the reference's serial order; its CUDA path uses
 * unordered atomics), optionally normalized. Synchronizes `stream`. */
nnrt_status nnrt_compute_vertex_normals(const float* d_vertices, int64_t vertex_count, const int64_t* d_faces, int64_t face_count,
                                        int32_t normalized, float* d_out, void* stream);
/* nnrt.geometry.functional.compute_ordered_point_cloud_normals(point_cloud, source_image_size) (NormalsOperations.cpp:74-95,
 * kernel NormalsOperationsImpl.h:170-214): organized [H*W,3] points -> [H*W,3] normals facing the camera, 0 on the border */
nnrt_status nnrt_compute_ordered_point_cloud_normals(const float* d_points, int64_t point_count, int32_t height, int32_t width, float* d_out,
                                                     void* stream);
/* Rigid frame-to-model alignment (the rigid step of the reference loop, apps/fusion/pipeline.py:338-354, an Open3D call
 * there): dense projective point-to-plane Gauss-Newton of model vertices d_points / d_normals [vertex_count,3] against an
 * organized live point image d_target_points [height,width,3] with normals d_target_normals [height,width,3] (camera
 * frame; a pixel with a non-finite entry, z <= 0 or a zero normal is no target). h_T_init float64[16] row-major maps
 * model to live-camera coordinates (rows 0..2 are read; they must be finite). Per iteration and vertex, in float:
 * q = R p + t, m = R n; dropped unless q is finite with q.z > 0 and pixel (floor(fx q.x / q.z + cx + 0.5),
 * floor(fy q.y / q.z + cy + 0.5)) lies in the image and holds a target (d, g); dropped if |q - d|^2 >
 * distance_threshold^2, unless |m . g| >= normal_agreement_cos (a value <= 0 disables this test), if cull_back_faces
 * and m . q >= 0, or if a term overflowed float. Residual r = g . (q - d), Jacobian row [q x g, g] (left perturbation
 * about the camera origin). The 6 x 6 normal equations are summed in float64 in an order fixed by vertex_count alone
 * (bit-reproducible), solved by float64 Cholesky on the device, and T <- exp(xi^) T. The `iterations` (>= 1) steps are
 * enqueued back to back on `stream`; pose, log and status are read once at the end (one stream synchronization).
 * h_log [iterations,2] float64 receives (correspondence count, sum r^2) as found at the start of each iteration;
 * log_row_capacity is the number of rows h_log has room for and must be >= iterations. *h_status: 0, or
 * NNRT_RIGID_ALIGN_DEGENERATE when some iteration found fewer than minimum_correspondence_count correspondences, a
 * Cholesky pivot <= 1e-12 * the largest diagonal entry, or a non-finite update: that iteration left T as it was (never a
 * NaN, never an error). vertex_count == 0 is legal: DEGENERATE, h_T_out = h_T_init, a zero log. h_T_out float64[16]. */
#define NNRT_RIGID_ALIGN_DEGENERATE 1
nnrt_status nnrt_rigid_align_point_to_plane(const float* d_points, const float* d_normals, int64_t vertex_count,
                                            const float* d_target_points, const float* d_target_normals, int32_t height, int32_t width,
                                            float fx, float fy, float cx, float cy, const double* h_T_init, int32_t iterations,
                                            float distance_threshold, float normal_agreement_cos, int32_t cull_back_faces,
                                            int32_t minimum_correspondence_count, double* h_T_out, double* h_log,
                                            int32_t log_row_capacity, int32_t* h_status, void* stream);
/* Luminance of an RGB image for the hybrid alignment below: d_rgb uint8 [height,width,3] -> d_out float32 [height,width],
 * in float I = ((0.299 R + 0.587 G) + 0.114 B) / 255, one value per pixel in [0, 1]. NNRT_ERROR_ARGUMENT for a negative
 * height or width, null images of a non-empty size, and images that overlap. An empty image is no error. */
nnrt_status nnrt_intensity_from_rgb8(const uint8_t* d_rgb, int32_t height, int32_t width, float* d_out, void* stream);
/* One level of the intensity pyramid: d_in float32 [height,width] -> d_out [ceil(height/2), ceil(width/2)]. Output pixel
 * (i, j) is the 3 x 3 binomial mean, weights (1, 2, 1) / 4 per axis, centred on input pixel (2 i, 2 j) with indices
 * clamped to the image, so level pixel (i, j) stays image pixel (2 i, 2 j): the convention of decimating the point image
 * by [::2, ::2]. In float, each of the three rows first, h = ((left + 2 centre) + right) / 4, then ((h0 + 2 h1) + h2) / 4.
 * Argument checks as for nnrt_intensity_from_rgb8. */
nnrt_status nnrt_intensity_halve(const float* d_in, int32_t height, int32_t width, float* d_out, void* stream);
/* nnrt_rigid_align_point_to_plane with a photometric term (the role of Method.Hybrid in Open3D's RGB-D odometry, which
 * the reference loop's rigid step calls, apps/fusion/pipeline.py:338-354): every argument of that function with the same
 * meaning and checks, plus the model's colours d_colors [vertex_count,3] float32 in [0, 1] and the live intensity image
 * d_target_intensity [height,width] float32 of the same level as d_target_points. The geometric row of a vertex is
 * decided and formed as there. A vertex whose geometric row was kept then, in float:
 * c = (0.299 cr + 0.587 cg) + 0.114 cb, dropped unless finite; u0 = floor(u), v0 = floor(v) of its unrounded pixel (u, v),
 * dropped unless u0 >= 0, u0 + 1 <= width - 1, v0 >= 0, v0 + 1 <= height - 1; dropped unless all four taps (v0, u0),
 * (v0, u0 + 1), (v0 + 1, u0), (v0 + 1, u0 + 1) hold a target point with finite z > 0 and a finite intensity; with
 * a = u - u0, b = v - v0: top = I00 + a (I01 - I00), bot = I10 + a (I11 - I10), I = top + b (bot - top),
 * Iu = (I01 - I00) + b ((I11 - I10) - (I01 - I00)), Iv = bot - top; rI = I - c, dropped if
 * photometric_residual_threshold > 0 and not |rI| <= it; gI = ((Iu fx) / q.z, (Iv fy) / q.z,
 * -(((Iu fx) q.x + (Iv fy) q.y) / (q.z q.z))), row [q x gI, gI]; row and rI times photometric_weight (finite, > 0; metres
 * per unit of intensity), dropped if any entry is not finite. The scaled row joins the same float64 normal equations
 * after the vertex's geometric products. h_log [iterations,4] receives (correspondence count, sum r^2, photometric
 * count, sum rI^2 unscaled). photometric_residual_threshold <= 0 disables its test; NaN is refused. No atomics, the
 * same fixed summation order: bit-reproducible. vertex_count == 0: DEGENERATE, h_T_out = h_T_init, a zero log. */
nnrt_status nnrt_rigid_align_hybrid(const float* d_points, const float* d_normals, const float* d_colors, int64_t vertex_count,
                                    const float* d_target_points, const float* d_target_normals, const float* d_target_intensity,
                                    int32_t height, int32_t width, float fx, float fy, float cx, float cy, const double* h_T_init,
                                    int32_t iterations, float distance_threshold, float normal_agreement_cos, int32_t cull_back_faces,
                                    int32_t minimum_correspondence_count, float photometric_weight, float photometric_residual_threshold,
                                    double* h_T_out, double* h_log, int32_t log_row_capacity, int32_t* h_status, void* stream);
/* Sparse feature tracker over intensity images (no counterpart in the reference, whose matches come
 * from PWC-Net / DeformNet): Shi-Tomasi scores, the selection of separated corners, pyramidal Lucas-Kanade. Images are
 * float32 [height,width]; pyramid level l is l applications of nnrt_intensity_halve, so level pixel (i, j) is image pixel
 * (2^l i, 2^l j) and a level-0 coordinate p is p / 2^l at level l. Points are (u, v) = (column, row). No float atomics,
 * every sum in a fixed order: bit-reproducible.
 *
 * nnrt_corner_scores: d_out_scores [height,width] = the smaller eigenvalue of the gradient matrix over the
 * (2 window_radius + 1)^2 window of each pixel, 1 <= window_radius <= NNRT_FEATURE_MAX_WINDOW_RADIUS. In float,
 * Ix = 0.5 (I[y, x + 1] - I[y, x - 1]), Iy = 0.5 (I[y + 1, x] - I[y - 1, x]). In float64, over the window in row-major
 * order, a = sum Ix Ix, b = sum Ix Iy, c = sum Iy Iy (each product of the two floats formed in float64, exact);
 * lambda = 0.5 ((a + c) - sqrt((a - c)(a - c) + 4 b b)) / (2 r + 1)^2, rounded once to float. A pixel (x, y) whose window
 * with its gradients' taps leaves the image (x - r - 1 < 0, x + r + 1 > width - 1, likewise y) scores 0, and so does a
 * result that is not finite. NNRT_ERROR_ARGUMENT for a negative height or width, height * width >= 2^31, a radius out
 * of range, nulls of a non-empty image and images that overlap. An empty image is no error. Asynchronous on `stream`.
 *
 * nnrt_select_features: at most max_count (1 .. 2^20) pixels of d_scores as d_out_points float32 [max_count,2], strongest
 * first. The maximum M is taken over the finite scores > 0 (0 if there is none). A pixel is a candidate iff its score s is
 * finite and > 0, s >= quality * M (a float product; 0 <= quality <= 1), d_mask (uint8 [height,width], nullable) is
 * non-zero there, and no pixel of its (2 nms_radius + 1)^2 neighbourhood clipped to the image (0 <= nms_radius <=
 * NNRT_FEATURE_MAX_NMS_RADIUS) has a larger score or an equal score and a lower pixel index y * width + x. Candidates
 * are ordered by descending score, ties by ascending pixel index; the first min(count, max_count) are written and
 * *h_out_count receives their number. Rows past it are not written. Synchronizes `stream` once (the candidate count).
 *
 * nnrt_track_features: Bouguet's pyramidal Lucas-Kanade from pyramid A to pyramid B, one feature per wavefront.
 * h_pyramid_a / h_pyramid_b: host arrays of `levels` (1 .. NNRT_FEATURE_MAX_LEVELS) device pointers, level l of size
 * h_heights[l] x h_widths[l] with h_heights[l] = ceil(h_heights[l - 1] / 2), likewise the widths. d_points [count,2];
 * d_initial_flow [count,2] nullable (level-0 pixels); d_reference_points [count,2] nullable. Per feature p, with r =
 * window_radius (1 .. NNRT_FEATURE_MAX_WINDOW_RADIUS), window offsets (i, j), |i|, |j| <= r, and S(I, x, y) the bilinear
 * sample in float: x0 = floor(x) (at most width - 2), a = x - x0, likewise y0, b; top = I00 + a (I01 - I00),
 * bot = I10 + a (I11 - I10), S = top + b (bot - top). "The window of margin m at (x, y) is inside" means, in float,
 * x - m >= 0, x + m <= width - 1, y - m >= 0, y + m <= height - 1 of the level.
 * g = initial flow / 2^(levels - 1), or 0. p, or g, not finite: NON_FINITE. For l = levels - 1 .. 0, in float unless said:
 *   pl = p * 2^-l. If the window of margin r + 1 at pl is not inside A_l: l > 0 skips the level, g <- 2 g; l = 0 is
 *   OUT_OF_IMAGE. T(i, j) = S(A_l, pl.x + i, pl.y + j), Tx = 0.5 (S(.., x + 1, y) - S(.., x - 1, y)), Ty likewise in y.
 *   In float64, Gxx = sum Tx Tx, Gxy = sum Tx Ty, Gyy = sum Ty Ty (products of the floats formed in float64; per lane
 *   over window pixels lane, lane + 64, .. in row-major numbering, then an xor butterfly over the 64 lanes);
 *   e_min = 0.5 ((Gxx + Gyy) - sqrt((Gxx - Gyy)(Gxx - Gyy) + 4 Gxy Gxy)) / (2 r + 1)^2; not finite: NON_FINITE;
 *   e_min < min_eigen_threshold: l > 0 skips the level (g <- 2 g), l = 0 is FLAT. v = 0; for k < max_iterations
 *   (1 .. NNRT_FEATURE_MAX_ITERATIONS): q = (pl + g) + v; q not finite: NON_FINITE; the window of margin r at q not
 *   inside B_l: OUT_OF_IMAGE; e = T - S(B_l, q.x + i, q.y + j); in float64 bx = sum e Tx, by = sum e Ty (summed as G),
 *   D = Gxx Gyy - Gxy Gxy, dx = (Gyy bx - Gxy by) / D, dy = (Gxx by - Gxy bx) / D; not finite: NON_FINITE;
 *   v <- v + (float) d; stop if epsilon > 0 and dx dx + dy dy < epsilon^2 (epsilon = 0: exactly max_iterations).
 *   l > 0: g <- 2 (g + v). l = 0: result = (p + g) + v; not finite: NON_FINITE; the window of margin r at the result not
 *   inside B_0: OUT_OF_IMAGE; residual = (float)(sum |e| in float64 at the result / (2 r + 1)^2); not finite:
 *   NON_FINITE; max_residual > 0 and residual > max_residual: RESIDUAL; with d_reference_points, unless
 *   |result - reference|^2 <= forward_backward_threshold^2 (float, dx dx + dy dy): FB_FAILED. Otherwise TRACKED.
 * d_out_points [count,2] (a lost feature keeps its input point: never a NaN the input did not hold), d_out_status uint8
 * [count] (NNRT_FEATURE_*), d_out_residual [count] (the level-0 residual for TRACKED, RESIDUAL and FB_FAILED, else 0).
 * A round-trip check is two calls: A -> B, then B -> A from the results with the original points as reference.
 * NNRT_ERROR_ARGUMENT for a negative count, nulls of non-empty inputs, outputs that overlap an input or one another,
 * level sizes that are not a pyramid, ranges as above, a NaN parameter, a negative or infinite epsilon or
 * min_eigen_threshold, and a reference without a finite forward_backward_threshold >= 0. count == 0 launches nothing.
 * Asynchronous on `stream`. */
#define NNRT_FEATURE_MAX_WINDOW_RADIUS 7
#define NNRT_FEATURE_MAX_NMS_RADIUS 15
#define NNRT_FEATURE_MAX_LEVELS 4
#define NNRT_FEATURE_MAX_ITERATIONS 30
#define NNRT_FEATURE_TRACKED 0
#define NNRT_FEATURE_OUT_OF_IMAGE 1
#define NNRT_FEATURE_FLAT 2
#define NNRT_FEATURE_RESIDUAL 3
#define NNRT_FEATURE_NON_FINITE 4
#define NNRT_FEATURE_FB_FAILED 5
nnrt_status nnrt_corner_scores(const float* d_intensity, int32_t height, int32_t width, int32_t window_radius, float* d_out_scores, void* stream);
nnrt_status nnrt_select_features(const float* d_scores, const uint8_t* d_mask, int32_t height, int32_t width, float quality, int32_t nms_radius,
                                 int32_t max_count, float* d_out_points, int64_t* h_out_count, void* stream);
nnrt_status nnrt_track_features(const float* const* h_pyramid_a, const float* const* h_pyramid_b, const int32_t* h_heights,
                                const int32_t* h_widths, int32_t levels, const float* d_points, const float* d_initial_flow,
                                const float* d_reference_points, int64_t count, int32_t window_radius, int32_t max_iterations, float epsilon,
                                float min_eigen_threshold, float max_residual, float forward_backward_threshold, float* d_out_points,
                                uint8_t* d_out_status, float* d_out_residual, void* stream);
/* nnrt.core.matmul3d(array_of_matrices_a, array_of_matrices_b) (cpp/pybind/core/core.cpp:32 -> cpp/core/linalg/Matmul3D.cpp:25-83):
 * d_c [batch, m, n] = d_a [batch, m, k] x d_b [batch, k, n] per batch entry, float32 row-major (n = 1: array of vectors). */
nnrt_status nnrt_matmul3d(const float* d_a, const float* d_b, int64_t batch, int32_t m, int32_t k, int32_t n, float* d_c, void* stream);
/* nnrt.geometry.functional.median_grid_subsample_3d_points(points, grid_cell_size) (functional.cpp:152-153 ->
 * GeometrySampling.cpp:62-68, GeometrySamplingMedian.h:264-296): indices of one medoid per occupied grid cell, in ascending
 * index order (the reference's order is its hash map's bin order). d_out_indices needs room for point_count int64;
 * *h_sample_count receives the number written. Synchronizes `stream`. */
nnrt_status nnrt_median_grid_subsample_3d_points(const float* d_points, int64_t point_count, float grid_cell_size, int64_t* d_out_indices,
                                                 int64_t* h_sample_count, void* stream);
/* Grid down-samplers over a sorted cell index. The cell of a point is floorf(p / grid_cell_size +
 * offset) per component in float32 (GridBinPoints, cpp/geometry/functional/kernel/GeometrySamplingGridBinning.h:39-40);
 * cells are numbered by their smallest member index (the reference's order is its hash map's bin order). All three take
 * d_points [point_count,3] float32, need room for point_count output rows, write the number of occupied cells to
 * *h_cell_count and synchronize `stream`. NNRT_ERROR_ARGUMENT, before anything is launched, for a grid_cell_size that is
 * not finite and positive, a non-finite offset, a negative point_count and null pointers; after the first kernel, for a
 * non-finite coordinate and for a cell coordinate outside [-2^20, 2^20). point_count == 0 gives 0 cells.
 *
 * nnrt.geometry.functional.mean_grid_downsample_3d_points(points, grid_cell_size) (functional.cpp:143-145 ->
 * GeometrySamplingImpl.h:48-54, GeometrySamplingMean.h): d_out_points [cells,3] float32, row r the mean of the members of
 * cell r, summed in float64 and rounded once. */
nnrt_status nnrt_mean_grid_downsample_3d_points(const float* d_points, int64_t point_count, float grid_cell_size, float offset_x, float offset_y,
                                                float offset_z, float* d_out_points, int64_t* h_cell_count, void* stream);
/* nnrt.geometry.functional.closest_to_mean_grid_subsample_3d_points(points, grid_cell_size) (functional.cpp:146-148 ->
 * GeometrySamplingImpl.h:56-62): per cell the member with the smallest (dx*dx + dy*dy) + dz*dz (float32) to the cell's
 * float32 mean, ties to the lower index; d_out_indices int64, ascending. */
nnrt_status nnrt_closest_to_mean_grid_subsample_3d_points(const float* d_points, int64_t point_count, float grid_cell_size, float offset_x,
                                                          float offset_y, float offset_z, int64_t* d_out_indices, int64_t* h_cell_count,
                                                          void* stream);
/* MedianGridSamplePoints with a grid offset (GeometrySamplingMedian.h:264-296, the stages of FastMedianRadiusSubsample3dPoints,
 * GeometrySamplingImpl.h:104-118): the medoids of nnrt_median_grid_subsample_3d_points, bit for bit at offset 0, found per
 * cell of the index instead of by all-pairs scans; d_out_indices int64, ascending. */
nnrt_status nnrt_median_grid_subsample_3d_points_binned(const float* d_points, int64_t point_count, float grid_cell_size, float offset_x,
                                                        float offset_y, float offset_z, int64_t* d_out_indices, int64_t* h_cell_count,
                                                        void* stream);
/* nnrt.core.KDTree(points) and KDTree.find_k_nearest_to_points(query_points, k, sort_output=false) (cpp/pybind/core/core.cpp ->
 * cpp/core/KdTree.h): an exact K-nearest-neighbour index over d_points [point_count, 3] float32, held as a uniform grid of
 * cells (not the reference's tree), with its own copy of the points. point_count >= 1; dimension_count must be 3; a
 * non-finite coordinate is refused. Creation synchronizes `stream`; the handle owns its device memory.
 * nnrt_point_index_find_k_nearest: d_out_indices [query_count, k] int32 and d_out_distances [query_count, k] float32,
 * each row ordered by ((dx*dx + dy*dy) + dz*dz in float32 with d = point - query, point index) ascending; the distance
 * written is sqrtf of that sum (Euclidean, as the reference returns). Slots past point_count hold -1 and +inf.
 * 1 <= k <= NNRT_POINT_INDEX_MAX_K; anything else is NNRT_ERROR_ARGUMENT and nothing is launched. query_count == 0
 * launches nothing. Does not synchronize. */
#define NNRT_POINT_INDEX_MAX_K 16
typedef struct nnrt_point_index nnrt_point_index;
nnrt_status nnrt_point_index_create(const float* d_points, int64_t point_count, int32_t dimension_count, void* stream, nnrt_point_index** out);
void nnrt_point_index_destroy(nnrt_point_index* index);
/* any of the outputs may be null: the point count, the cell size chosen, the occupied cells and how often the index was built */
nnrt_status nnrt_point_index_get_info(const nnrt_point_index* index, int64_t* h_point_count, float* h_cell_size, int64_t* h_cell_count,
                                      int32_t* h_build_count);
nnrt_status nnrt_point_index_find_k_nearest(const nnrt_point_index* index, const float* d_query_points, int64_t query_count,
                                            int32_t dimension_count, int32_t k, int32_t* d_out_indices, float* d_out_distances, void* stream);
/* nnrt.get_vertex_erosion_mask(vertex_positions, face_indices, iteration_count, min_neighbors) (nnrt_pybind.cpp:121-123 ->
 * cpp/cpu/graph_proc.cpp:27-90): faces start alive; iteration_count times, every alive face with a vertex touched by fewer
 * than min_neighbors alive faces dies. d_out_mask [vertex_count] uint8 = 1 where an alive face touches the vertex.
 * d_face_indices [face_count, 3] int64. A face index outside [0, vertex_count) gives NNRT_ERROR_ARGUMENT (the reference
 * reads out of range); such a face is never dereferenced. vertex_count == 0 or face_count == 0 with nothing to write
 * launches nothing; face_count == 0 zeroes the mask. Synchronizes `stream`. */
nnrt_status nnrt_get_vertex_erosion_mask(int64_t vertex_count, const int64_t* d_face_indices, int64_t face_count, int32_t iteration_count,
                                         int32_t min_neighbors, uint8_t* d_out_mask, void* stream);
/* nnrt.sample_nodes(vertex_positions_in, vertex_erosion_mask_in, node_coverage, use_only_non_eroded_indices,
 * random_shuffle) (nnrt_pybind.cpp:124-126 -> cpp/cpu/graph_proc.cpp:92-155): the greedy node set -- in priority order, a
 * vertex becomes a node iff no earlier node q has ((dx*dx + dy*dy) + dz*dz) <= node_coverage * node_coverage (unfused
 * f32) -- computed in parallel rounds, bit for bit the sequential result. d_points [point_count, 3] float32; d_mask
 * [point_count] uint8 or NULL (use_only_non_eroded_indices = false); d_order [point_count] int64 permutation giving the
 * priority order (the reference's shuffle) or NULL for ascending index; an entry outside [0, point_count) gives
 * NNRT_ERROR_ARGUMENT. d_out_indices (capacity out_capacity >= point_count int64) receives the node vertex indices in
 * acceptance order, *h_out_count their number, *h_out_rounds (nullable) the number of rounds taken. node_coverage must be
 * positive and finite with a finite, normal square. Vertices with a non-finite coordinate are never candidates (in the
 * reference such a vertex always becomes a node). NNRT_ERROR_ARGUMENT if the candidates span more than 2^21 - 3 cells of
 * node_coverage along an axis; NNRT_ERROR_INTERNAL if a round decides nothing (never expected). Memory is
 * O(point_count). Synchronizes `stream`. */
nnrt_status nnrt_sample_nodes(const float* d_points, int64_t point_count, const uint8_t* d_mask, const int64_t* d_order, float node_coverage,
                              int64_t* d_out_indices, int64_t out_capacity, int64_t* h_out_count, int32_t* h_out_rounds, void* stream);
/* Extending the warp field over newly fused surface (DynamicFusion section 3.4; no counterpart in the reference).
 * nnrt_compute_vertex_support: for each of point_count points the nearest of node_count nodes (d_out_nearest_node int32,
 * the lowest index on ties) and the support ratio d_min / c (d_out_support_ratio float32), with the squared distance
 * ((dx*dx + dy*dy) + dz*dz), d = node - point, in unfused f32 as nnrt_compute_anchors_and_weights forms it.
 * d_node_coverage_weights NULL: c = node_coverage, the ratio is sqrtf(min sq) / node_coverage. Otherwise [node_count]
 * squared per-node coverages w_j > 0 (nnrt_warp_field_get_node_coverage_weights; node_coverage is ignored): the minimum
 * is taken over sq * RN(1 / w_j) and the ratio is its sqrtf. A point with a non-finite coordinate gets ratio 0 and
 * index -1; node_count == 0 gives ratio +inf and index -1. Asynchronous on `stream`.
 * nnrt_blend_node_transforms: the motion of the field (d_nodes [node_count, 3], d_node_rotations [node_count, 3, 3],
 * d_node_translations [node_count, 3]) at each of point_count query points p: over the min(anchor_count, node_count)
 * nearest nodes in ascending (distance, index) order, without a distance threshold, with weights
 * exp(-d^2 / (2 node_coverage^2)) normalised and f32 sums in that order: d_out_translations = sum_k w_k ((R_k (p - g_k) -
 * (p - g_k)) + t_k), i.e. the warped point minus p; d_out_rotations = the rotation nearest to sum_k w_k R_k (its
 * orthogonal polar factor, det = +1, by a fixed number of Newton steps). Where that sum's determinant is at most 1e-3
 * (rotations about 180 degrees apart) or the result misses orthogonality by more than 1e-5, the rotation is the nearest
 * node's and d_out_fallback [point_count] uint8 is 1, else 0. h_out_fallback_count (nullable) receives the number of
 * such points; when it is given the call synchronizes `stream`. anchor_count must be in [1, 8], node_count >= 1 unless
 * point_count == 0. */
nnrt_status nnrt_compute_vertex_support(const float* d_points, int64_t point_count, const float* d_nodes, int32_t node_count, float node_coverage,
                                        const float* d_node_coverage_weights, float* d_out_support_ratio, int32_t* d_out_nearest_node,
                                        void* stream);
nnrt_status nnrt_blend_node_transforms(const float* d_points, int64_t point_count, const float* d_nodes, const float* d_node_rotations,
                                       const float* d_node_translations, int32_t node_count, int32_t anchor_count, float node_coverage,
                                       float* d_out_rotations, float* d_out_translations, uint8_t* d_out_fallback, int64_t* h_out_fallback_count,
                                       void* stream);
/* nnrt.compute_mesh_from_depth(point_image, max_triangle_edge_distance) (nnrt_pybind.cpp:79-80 -> cpp/cpu/image_proc.cpp:341-482):
 * the pixel-connected mesh of d_point_image [height, width, 3] float32. The 2x2 pixel cell at (x, y) emits triangle
 * (00, 01, 10) if all three points have z > 0 (NaN is invalid) and all three edges have
 * sqrtf((dx*dx + dy*dy) + dz*dz) <= max_triangle_edge_distance (unfused f32), then triangle (11, 10, 01) under the same
 * test; a vertex is numbered the first time a valid triangle touches its pixel, cells in row-major order -- computed with
 * two scans, bit for bit the sequential result, numbering and face order included. d_out_vertices [vertex_capacity, 3]
 * float32, d_out_vertex_pixels [vertex_capacity, 2] int32 as (x, y), d_out_faces [face_capacity, 3] int32;
 * *h_out_vertex_count and *h_out_face_count receive the numbers written. height * width vertices and
 * 2 (height - 1)(width - 1) faces always suffice; a capacity the mesh exceeds gives NNRT_ERROR_ARGUMENT and nothing is
 * written. height < 2, width < 2 or no valid triangle gives two zero counts and launches nothing that indexes the outputs
 * (the reference leaves its output arrays unsized then). Synchronizes `stream`. */
nnrt_status nnrt_compute_mesh_from_depth(const float* d_point_image, int32_t height, int32_t width, float max_triangle_edge_distance,
                                         float* d_out_vertices, int32_t* d_out_vertex_pixels, int64_t vertex_capacity, int32_t* d_out_faces,
                                         int64_t face_capacity, int64_t* h_out_vertex_count, int64_t* h_out_face_count, void* stream);
/* nnrt.compute_edges_shortest_path(vertex_positions_in, [vertex_mask_in,] face_indices_in, node_indices_in, max_neighbor_count,
 * node_coverage, enforce_total_num_neighbors) (nnrt_pybind.cpp:143-153 -> cpp/cpu/graph_proc.cpp:181-338): per node i with
 * vertex d_node_vertex_indices[i], D_i(v) is the float32 shortest-path length over the mesh edges, every relaxation
 * d_u + sqrtf((dx*dx + dy*dy) + dz*dz) in unfused f32 -- the values of the reference's Dijkstra, found by parallel relaxation
 * to the same fixed point. A vertex with d_vertex_mask[v] == 0 is never entered (NULL mask: every vertex; the node's own
 * vertex is the start whatever its mask). enforce_total_num_neighbors == 0: a vertex is entered only at
 * D <= 2 * node_coverage; otherwise the radius doubles for the nodes that have fewer than max_neighbor_count neighbours
 * and were stopped by it, until none is left. Row i of d_out_edges [node_count, max_neighbor_count] int32 holds the other
 * nodes whose vertex was reached, by ascending D (equal D: by ascending node index; the reference orders ties by its
 * heap's state), unused slots -1; d_out_distances their D, unused 0; d_out_weights exp(-(D*D) / (2 c c)) divided by the
 * row's left-to-right sum (by the count if the sum is 0), unused 0. A negative node vertex index gives an all-default
 * row. The reference's dense node_count x vertex_count distance matrix is not produced. d_faces [face_count, 3] int32; a
 * face index outside [0, vertex_count), a node vertex index >= vertex_count or two nodes on one vertex give
 * NNRT_ERROR_ARGUMENT (the reference reads out of range / keeps the later node). max_neighbor_count in [1, 1024].
 * *h_out_passes (nullable) receives the number of radius passes. Scratch: 20 bytes per vertex per concurrently processed
 * node, at most 1 GiB. Synchronizes `stream`. */
nnrt_status nnrt_compute_edges_shortest_path(const float* d_vertices, int64_t vertex_count, const uint8_t* d_vertex_mask, const int32_t* d_faces,
                                             int64_t face_count, const int32_t* d_node_vertex_indices, int32_t node_count,
                                             int32_t max_neighbor_count, float node_coverage, int32_t enforce_total_num_neighbors,
                                             int32_t* d_out_edges, float* d_out_weights, float* d_out_distances, int32_t* h_out_passes,
                                             void* stream);
/* nnrt.node_and_edge_clean_up(graph_edges, valid_nodes_mask) (nnrt_pybind.cpp:219-220 -> graph_proc.cpp:540-590), host code on
 * host arrays: h_valid_nodes_mask [node_count] uint8 is cleared for every valid node of which at most one entry before its
 * row's first -1 names a node not removed by this call, repeated to the fixed point (which does not depend on the visiting
 * order). h_graph_edges [node_count, max_neighbor_count] int32; an entry outside [-1, node_count) gives
 * NNRT_ERROR_ARGUMENT. */
nnrt_status nnrt_node_and_edge_clean_up(const int32_t* h_graph_edges, int64_t node_count, int32_t max_neighbor_count, uint8_t* h_valid_nodes_mask);
/* nnrt.compute_clusters(graph_edges_in) (nnrt_pybind.cpp:222-225 -> graph_proc.cpp:510-636), host code on host arrays: the
 * connected components of the undirected graph over each row's entries up to its first -1, numbered by ascending lowest
 * member. h_out_clusters [node_count] int32, h_out_cluster_sizes (room for node_count int32), *h_out_cluster_count. An entry
 * outside [-1, node_count) before a row's first -1 gives NNRT_ERROR_ARGUMENT. */
nnrt_status nnrt_compute_clusters(const int32_t* h_graph_edges, int64_t node_count, int32_t max_neighbor_count, int32_t* h_out_clusters,
                                  int32_t* h_out_cluster_sizes, int64_t* h_out_cluster_count);
/* nnrt.core.linalg AxisAngleVectorsToMatricesRodrigues (cpp/core/linalg/RodriguesImpl.h:66-88) */
nnrt_status nnrt_axis_angle_to_matrices_rodrigues(const float* d_vectors, int32_t count, float* d_matrices, void* stream);
/* SolveBlockDiagonalCholesky (cpp/core/linalg/SolveBlockDiagonalCholesky.cpp): x_i = A_i^-1 b_i, block size 3 or 6 */
nnrt_status nnrt_solve_block_diagonal_cholesky(const float* d_blocks, const float* d_b, int32_t block_count, int32_t block_size,
                                               float* d_x, void* stream);
/* InvertPositiveSemidefiniteBlocks (cpp/core/linalg/InvertBlocks.cpp:82-126: potrf + potrs against the identity per
 * block), block size 3 or 6, row-major [count, s, s] -> [count, s, s]; the arrowhead stem's D^-1 runs the same device
 * functions. NNRT_ERROR_NOT_POSITIVE_DEFINITE if a block's potrf fails (its output is NaN). */
nnrt_status nnrt_invert_positive_semidefinite_blocks(const float* d_blocks, int32_t block_count, int32_t block_size, float* d_out,
                                                     void* stream);
/* ---- block-sparse stages of the arrowhead solve (SolveBlockSparseArrowheadCholesky.cpp:30-95, SchurComplement.cpp:43-78),
 * standalone; row-major [count, s, s] float blocks, int32 [count, 2] block coordinates (row, column). Coordinates outside
 * the matrix / vector give NNRT_ERROR_ARGUMENT (the reference does not check them). ---- */
/* MatmulBlockSparseRowWisePadded (cpp/core/linalg/MatmulBlockSparse.h; MatmulBlockSparseImpl.h:39-157): c_i = a[row_i] b_i;
 * blocks whose row has no A block (row >= a_block_count) are zero with mask 0. MatmulBlockSparseRowWise = the mask-1 blocks
 * and their coordinates. */
nnrt_status nnrt_matmul_block_sparse_row_wise(const float* d_a_blocks, int32_t a_block_count, const float* d_b_blocks,
                                              const int32_t* d_b_coordinates, int32_t b_block_count, int32_t block_size, float* d_c_blocks,
                                              uint8_t* d_c_mask, void* stream);
/* MatmulBlockSparse (MatmulBlockSparseImpl.h:160-439): op(A) op(B) with int16 breadboards [block rows, block columns]
 * holding block indices (-1 = empty); op = transpose when transpose_x != 0. Output: d_c_blocks [out_rows * out_cols, s, s]
 * in row-major block order and d_c_mask (1 = some block pair contributes); the reference returns the mask-1 blocks and
 * their (row, column) coordinates. */
nnrt_status nnrt_matmul_block_sparse(const float* d_a_blocks, int32_t a_block_count, const int16_t* d_a_breadboard, int32_t a_block_rows,
                                     int32_t a_block_columns, int32_t transpose_a, const float* d_b_blocks, int32_t b_block_count,
                                     const int16_t* d_b_breadboard, int32_t b_block_rows, int32_t b_block_columns, int32_t transpose_b,
                                     int32_t block_size, float* d_c_blocks, uint8_t* d_c_mask, void* stream);
/* BlockSparseAndVectorProduct (MatmulBlockSparseImpl.h:441-602): out [m] = op(A) v, A given by blocks at coordinates + the
 * (row, column) block offset; transpose places block (i, j) at (j, i) transposed. d_out must not overlap d_vector
 * (NNRT_ERROR_ARGUMENT). */
nnrt_status nnrt_block_sparse_and_vector_product(const float* d_blocks, const int32_t* d_coordinates, int32_t block_count, int32_t block_size,
                                                 int32_t block_row_offset, int32_t block_column_offset, int32_t transpose,
                                                 const float* d_vector, int64_t vector_length, int64_t m, float* d_out, void* stream);
/* DiagonalBlockSparseAndVectorProduct (MatmulBlockSparseImpl.h:604-690): out_i = D_i v_i, [count * s] */
nnrt_status nnrt_diagonal_block_sparse_and_vector_product(const float* d_blocks, int32_t block_count, int32_t block_size, const float* d_vector,
                                                          float* d_out, void* stream);
/* FillInSparseBlocks / AddSparseBlocks / SubtractSparseBlocks (SparseBlocksImpl.h:30-190), op 0 / 1 / 2, into a row-major
 * [rows, columns] matrix; d_coordinates == NULL: block i at (i, i) (FillInDiagonalBlocks, DiagonalBlocksImpl.h). Add and
 * subtract are atomic; a fill with repeated coordinates keeps one of the blocks, unspecified which (the reference's
 * ParallelFor races the same way). */
nnrt_status nnrt_sparse_blocks_op(float* d_matrix, int64_t rows, int64_t columns, const float* d_blocks, const int32_t* d_coordinates,
                                  int32_t block_count, int32_t block_size, int64_t block_row_offset, int64_t block_column_offset,
                                  int32_t transpose, int32_t op, void* stream);
/* GetSparseBlocks (SparseBlocksImpl.h:192-230); d_coordinates == NULL: GetDiagonalBlocks */
nnrt_status nnrt_get_sparse_blocks(const float* d_matrix, int64_t rows, int64_t columns, int32_t block_size, const int32_t* d_coordinates,
                                   int32_t block_count, float* d_blocks, void* stream);
/* TransposeBlocksInPlace (TransposeBlocks.h) */
nnrt_status nnrt_transpose_blocks_in_place(float* d_blocks, int32_t block_count, int32_t block_size, void* stream);
/* InvertTriangularBlocks (InvertBlocks.cpp, trtri per block), upper != 0: UpLoTriangular::UPPER; a zero diagonal entry
 * gives NNRT_ERROR_NOT_POSITIVE_DEFINITE (trtri info > 0). d_out must not overlap d_blocks (NNRT_ERROR_ARGUMENT). */
nnrt_status nnrt_invert_triangular_blocks(const float* d_blocks, int32_t block_count, int32_t block_size, int32_t upper, float* d_out,
                                          void* stream);
/* SolveBlockSparseArrowheadCholesky (cpp/core/linalg/SolveBlockSparseArrowheadCholesky.cpp:30-95), 6x6 blocks:
 * d_diagonal_blocks [N,6,6], d_wing_blocks [E,6,6] at block coordinates d_wing_coordinates [E,2] (row < arrow_base
 * <= column for stem-to-corner blocks; row >= arrow_base for corner off-diagonal blocks), b [6N]. Coordinates outside
 * [0, N), a diagonal coordinate (row == column) or a column inside the stem (column < arrow_base) give
 * NNRT_ERROR_ARGUMENT, checked before any allocation; so do a negative block count and a NULL pointer to a non-empty
 * array. Every split is solved: arrow_base == N (no corner: a block-diagonal solve), arrow_base == 0 (corner only),
 * wing_block_count == 0 (the array pointers may then be NULL), corner off-diagonal blocks without any stem-to-corner
 * block. diagonal_block_count == 0 is the empty system: NNRT_OK, nothing is read, written or launched (all pointers may
 * be NULL). A stem block or a Schur complement that is not positive definite (a NaN pivot included) gives
 * NNRT_ERROR_NOT_POSITIVE_DEFINITE; x is then unspecified, and the structure's plan stays valid. The Schur corner is factored tile-sparse (nested-dissection order
 * of the corner blocks); its size is bounded by device memory only. The structure-derived plan (stem lists, corner plan,
 * scratch) of the 4 most recently solved wing structures is kept per process and reused by a later call with the same
 * device, block count, arrow base and coordinates (one call owns a plan at a time; calls synchronise their stream
 * before returning it); nnrt_release_arrowhead_plans frees them. */
nnrt_status nnrt_solve_block_sparse_arrowhead_cholesky(const float* d_diagonal_blocks, const float* d_wing_blocks,
                                                       const int32_t* d_wing_coordinates, int32_t wing_block_count,
                                                       int32_t diagonal_block_count, int32_t arrow_base_block_index,
                                                       const float* d_b, float* d_x, void* stream);
/* Frees the arrowhead plans kept by nnrt_solve_block_sparse_arrowhead_cholesky (device memory; none is in use by a
 * concurrent call: plans being solved with are not in the pool). */
void nnrt_release_arrowhead_plans(void);

/* ---- TSDF voxel block grid (NonRigidSurfaceVoxelBlockGrid, cpp/geometry/NonRigidSurfaceVoxelBlockGrid.h:30-65 over
 * VoxelBlockGrid, cpp/geometry/VoxelBlockGrid.h; Python: nnrt.geometry.NonRigidSurfaceVoxelBlockGrid, pybind
 * cpp/pybind/geometry/geometry.cpp:61-275). Attributes tsdf (float32), weight (float32 | uint16), color (none |
 * float32 | uint16 | uint8, 3 channels). Block coordinates are int32 [n,3]; images are device arrays: depth [H,W]
 * uint16 or float32, color [Hc,Wc,3] uint8 (uint16 depth) or float32 (float32 depth, [0,1]); intrinsics double[9],
 * extrinsics double[16] (NULL: identity). Functions producing a variable-size result return its size and keep it in
 * the grid until the matching copy_* call (the grid owns the workspace). ---- */
typedef struct nnrt_voxel_grid nnrt_voxel_grid;
#define NNRT_DTYPE_NONE -1
#define NNRT_DTYPE_FLOAT32 0
#define NNRT_DTYPE_UINT16 1
#define NNRT_DTYPE_UINT8 2
/* VoxelBlockGrid(attr_names, attr_dtypes, attr_channels, voxel_size, block_resolution, block_count, device)
 * (VoxelBlockGrid.h:52-58); storage grows (x2) past block_count as Open3D's hash map does. */
nnrt_status nnrt_voxel_grid_create(float voxel_size, int32_t block_resolution, int64_t block_count, int32_t weight_dtype,
                                   int32_t color_dtype, int32_t device, nnrt_voxel_grid** out);
void nnrt_voxel_grid_destroy(nnrt_voxel_grid* grid);
nnrt_status nnrt_voxel_grid_get_info(const nnrt_voxel_grid* grid, int64_t* h_active_blocks, int64_t* h_capacity, float* h_voxel_size,
                                     int32_t* h_block_resolution);
/* hashmap().activate(block_coords) (Open3D HashMap::Activate); new blocks start at zero */
nnrt_status nnrt_voxel_grid_activate(nnrt_voxel_grid* grid, const int32_t* d_block_coords, int64_t count, void* stream);
/* active block coordinates [active,3] in buffer order (ExtractVoxelBlockCoordinates before its metric scaling,
 * NonRigidSurfaceVoxelBlockGrid.cpp:186-191) */
nnrt_status nnrt_voxel_grid_get_block_coordinates(const nnrt_voxel_grid* grid, int32_t* d_out, void* stream);
/* GetUniqueBlockCoordinates(depth, intrinsic, extrinsic, depth_scale, depth_max, trunc_voxel_multiplier)
 * (VoxelBlockGrid.cpp:237-270, Open3D DepthTouch); result -> nnrt_voxel_grid_copy_result_coordinates */
nnrt_status nnrt_voxel_grid_unique_block_coordinates(nnrt_voxel_grid* grid, const void* d_depth, int32_t depth_dtype, int32_t height,
                                                     int32_t width, const double* h_K, const double* h_E, float depth_scale,
                                                     float depth_max, float trunc_voxel_multiplier, int64_t* h_count, void* stream);
nnrt_status nnrt_voxel_grid_copy_result_coordinates(const nnrt_voxel_grid* grid, int32_t* d_out, void* stream);
/* Integrate(block_coords, depth, color, depth_intrinsic, color_intrinsic, extrinsic, depth_scale, depth_max,
 * trunc_voxel_multiplier) (VoxelBlockGrid.cpp:317-350, Open3D voxel_grid::Integrate); d_color may be NULL */
nnrt_status nnrt_voxel_grid_integrate(nnrt_voxel_grid* grid, const int32_t* d_block_coords, int64_t count, const void* d_depth,
                                      int32_t depth_dtype, int32_t height, int32_t width, const void* d_color, int32_t color_height,
                                      int32_t color_width, const double* h_depth_K, const double* h_color_K, const double* h_E,
                                      float depth_scale, float depth_max, float trunc_voxel_multiplier, void* stream);
/* IntegrateNonRigid(block_coords, warp_field, depth, color, depth_normals, depth_intrinsics, color_intrinsics,
 * extrinsics, depth_scale, depth_max, truncation_voxel_multiplier) -> cos_voxel_ray_to_normal [H,W]
 * (NonRigidSurfaceVoxelBlockGrid.cpp:33-66, NonRigidSurfaceVoxelBlockGridImpl.h:52-229); d_depth_normals [H,W,3] */
nnrt_status nnrt_voxel_grid_integrate_non_rigid(nnrt_voxel_grid* grid, const int32_t* d_block_coords, int64_t count,
                                                const nnrt_warp_field* warp_field, const void* d_depth, int32_t depth_dtype,
                                                int32_t height, int32_t width, const void* d_color, int32_t color_height,
                                                int32_t color_width, const float* d_depth_normals, const double* h_depth_K,
                                                const double* h_color_K, const double* h_E, float depth_scale, float depth_max,
                                                float trunc_voxel_multiplier, float* d_cos_out, void* stream);
/* No counterpart in the reference. Off (the default), nnrt_voxel_grid_integrate_non_rigid is the reference's: it skips
 * a voxel whose view ray and (camera-facing) pixel normal have cosine > 0.5 and never increments the voxel weight, so
 * surface first seen in a non-rigid step never reaches the extracted mesh. enabled != 0: later calls on this grid skip
 * cosine < 0.5 instead (grazing views, and pixels without a normal) and add 1 to the weight of every voxel they
 * update, as nnrt_voxel_grid_integrate does. Host state only. */
nnrt_status nnrt_voxel_grid_set_non_rigid_surface_growth(nnrt_voxel_grid* grid, int32_t enabled);
/* ExtractVoxelValuesAndCoordinates (NonRigidSurfaceVoxelBlockGrid.cpp:168-184): d_out [active * res^3, C], rows
 * (x, y, z, tsdf, weight[, r, g, b]), C = 5 or 8 (h_channels) */
nnrt_status nnrt_voxel_grid_extract_voxel_values_and_coordinates(const nnrt_voxel_grid* grid, float* d_out, int32_t* h_channels,
                                                                 void* stream);
/* ExtractVoxelValuesAt(query_voxel_coordinates) (NonRigidSurfaceVoxelBlockGrid.cpp:193-224): rows of the queries whose
 * block is active -> nnrt_voxel_grid_copy_result_rows */
nnrt_status nnrt_voxel_grid_extract_voxel_values_at(nnrt_voxel_grid* grid, const int32_t* d_query, int64_t count, int64_t* h_rows,
                                                    int32_t* h_channels, void* stream);
nnrt_status nnrt_voxel_grid_copy_result_rows(const nnrt_voxel_grid* grid, float* d_out, void* stream);
/* GetBoundingBoxesOfWarpedBlocks(block_keys, warp_field, extrinsics) (NonRigidSurfaceVoxelBlockGrid.cpp:113-124):
 * d_boxes [n,6] (min xyz, max xyz) */
nnrt_status nnrt_voxel_grid_warped_block_boxes(const nnrt_voxel_grid* grid, const int32_t* d_block_keys, int64_t count,
                                               const nnrt_warp_field* warp_field, const double* h_E, float* d_boxes, void* stream);
/* GetAxisAlignedBoxesInterceptingSurfaceMask (NonRigidSurfaceVoxelBlockGridImpl.h:359-437): d_mask [n] uint8 */
nnrt_status nnrt_boxes_intersecting_surface_mask(const float* d_boxes, int64_t count, const void* d_depth, int32_t depth_dtype,
                                                 int32_t height, int32_t width, const double* h_K, float depth_scale, float depth_max,
                                                 int32_t stride, float truncation_distance, uint8_t* d_mask, void* stream);
/* FindBlocksIntersectingTruncationRegion(depth, warp_field, intrinsics, extrinsics, depth_scale, depth_max,
 * truncation_voxel_multiplier) (NonRigidSurfaceVoxelBlockGrid.cpp:141-166) -> nnrt_voxel_grid_copy_result_coordinates */
nnrt_status nnrt_voxel_grid_find_blocks_intersecting_truncation_region(nnrt_voxel_grid* grid, const void* d_depth, int32_t depth_dtype,
                                                                       int32_t height, int32_t width, const nnrt_warp_field* warp_field,
                                                                       const double* h_K, const double* h_E, float depth_scale,
                                                                       float depth_max, float trunc_voxel_multiplier, int64_t* h_count,
                                                                       void* stream);
/* ActivateSleeveBlocks() (NonRigidSurfaceVoxelBlockGrid.cpp:98-109): returns the inactive-neighbour count */
nnrt_status nnrt_voxel_grid_activate_sleeve_blocks(nnrt_voxel_grid* grid, int64_t* h_count, void* stream);
/* ExtractTriangleMesh(weight_threshold, estimated_vertex_number) (VoxelBlockGrid.cpp:461-497, Open3D marching cubes)
 * -> counts; then nnrt_voxel_grid_copy_mesh: vertices [V,3], normals [V,3], colors [V,3] in [0,1] (may be NULL),
 * triangles int64 [T,3] */
nnrt_status nnrt_voxel_grid_extract_triangle_mesh(nnrt_voxel_grid* grid, float weight_threshold, int64_t* h_vertex_count,
                                                  int64_t* h_triangle_count, void* stream);
nnrt_status nnrt_voxel_grid_copy_mesh(const nnrt_voxel_grid* grid, float* d_vertices, float* d_normals, float* d_colors,
                                      int64_t* d_triangles, void* stream);
/* RayCast(block_coords, intrinsic, extrinsic, width, height, render_attributes, depth_scale, depth_min, depth_max,
 * weight_threshold, trunc_voxel_multiplier, range_map_down_factor) (VoxelBlockGrid.cpp:353-427, Open3D
 * voxel_grid::EstimateRange + RayCast as restated in DESIGN.md section 19, with its two deviations): a depth range per
 * image tile from the active blocks among d_block_coords [count,3], then one ray per pixel marched through the hashed
 * blocks to the first crossing from positive to negative tsdf. attribute_mask selects the maps (NNRT_RAY_CAST_* bits);
 * map pointers the mask leaves out may be NULL. Outputs (float32, every pixel written on every call, 0 at a miss):
 * d_range [ceil(H/f), ceil(W/f), 2] (always), d_depth [H,W,1] = camera-space depth * depth_scale, d_vertex [H,W,3] and
 * d_normal [H,W,3] in world coordinates (the normal points into free space), d_color [H,W,3] in [0,1]. h_E (world ->
 * camera) may be NULL: identity. count == 0 or an empty grid is no error: every ray misses. NNRT_ERROR_ARGUMENT: a null
 * grid, h_K or d_range; width, height or range_map_down_factor < 1; depth_min < 0, depth_min >= depth_max or
 * depth_scale <= 0; a requested map that is NULL; color on a grid without color storage; a singular extrinsic;
 * a step bound ceil(2 (depth_max - depth_min) / voxel_size) + 2 above 2^20. */
#define NNRT_RAY_CAST_DEPTH 1
#define NNRT_RAY_CAST_VERTEX 2
#define NNRT_RAY_CAST_NORMAL 4
#define NNRT_RAY_CAST_COLOR 8
nnrt_status nnrt_voxel_grid_ray_cast(nnrt_voxel_grid* grid, const int32_t* d_block_coords, int64_t count, const double* h_K,
                                     const double* h_E, int32_t width, int32_t height, int32_t attribute_mask, float depth_scale,
                                     float depth_min, float depth_max, float weight_threshold, float trunc_voxel_multiplier,
                                     int32_t range_map_down_factor, float* d_range, float* d_depth, float* d_vertex, float* d_normal,
                                     float* d_color, void* stream);
/* the marching-cubes tables (host): tri [256][31] int8 edge triples in emission order (-1 terminated; the published
 * Lorensen-Cline / Bourke table Open3D indexes, each triangle (a, b, c) emitted as (c, b, a), Open3D's slot 2 - v), edge mask [256] */
nnrt_status nnrt_marching_cubes_table(int8_t* h_tri, uint16_t* h_edge_mask);

#ifdef __cplusplus
}
#endif

#endif /* NNRT_MI355X_H */
