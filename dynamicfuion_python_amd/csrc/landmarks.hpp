// The fitter's landmark term (nnrt_fitter_set_landmarks): sparse 3-D point correspondences
// (canonical vertex, camera-space target, weight) that enter the same normal equations as the data and ARAP terms.
//
//   once per prepared frame   the landmarks' (node, landmark, slot) associations, sorted stably by node, and the runs of
//                             equal nodes; in coupled mode the same by pair slot (group_landmarks)
//   once per iteration        k_fit_landmarks: every run summed in association order in fp64 by one 8-lane group and added
//                             to acc / pair_acc by that single writer; the landmarks' distances and gates; their cost
#pragma once

#include "device_primitives.hpp"
#include "kernels.hpp"

namespace nnrt {

constexpr int LM_INFO_WORDS = 8;
// info words the grouping leaves on the device (the iteration's launch reads the two run counts from them)
enum { LM_INFO_ASSOC = 0, LM_INFO_RUNS = 1, LM_INFO_PAIR_ASSOC = 2, LM_INFO_PAIR_RUNS = 3, LM_INFO_BAD_INDEX = 4, LM_INFO_NO_FACE = 5 };
constexpr int LM_NONE = 0x7fffffff;   // LM_INFO_BAD_INDEX / LM_INFO_NO_FACE: no such landmark

// One sorted association list: entry u is association vals[u] of the run keyed keys[u]; run r is [starts[r], starts[r + 1])
// (the last one ends at the list's association count). Entries whose key is LM_KEY_NONE sort last and belong to no run.
constexpr uint64_t LM_KEY_NONE = 0xffffffffull;
struct LandmarkRuns {
	DeviceBuffer<uint64_t> keys_in, keys;
	DeviceBuffer<int> vals_in, vals;
	DeviceBuffer<uint8_t> heads;
	DeviceBuffer<int64_t> starts, count;
};

struct LandmarkSet {
	int64_t L = 0;
	float term_weight = 1.f, cutoff = 0.f;
	DeviceBuffer<int32_t> index;       // [L] canonical vertex
	DeviceBuffer<float> target;        // [L, 3] camera space
	DeviceBuffer<float> weight;        // [L]
	DeviceBuffer<float4> distances;    // [L] (d, active) as of the state the last iteration started from
	DeviceBuffer<double> cost;         // [1] sum of rho_l, the same
	DeviceBuffer<int> info;            // [LM_INFO_WORDS]
	DeviceBuffer<uint8_t> vertex_in_face;   // [V]
	LandmarkRuns node, pair;
	Scratch scratch;
	int64_t h_info[4] = {0, 0, 0, 0};  // associations, node runs, pair associations, pair runs of the prepared frame
	void release_all() { *this = LandmarkSet(); }
};

// what the grouping reads of a prepared frame
struct LandmarkFrame {
	int64_t V, F;
	int N, K;
	const int4* faces4;
	const int32_t* anchors;       // [V, K]
	int coupled, M;
	const int* row_off;           // the pair table (coupled)
	const int32_t* pairs;
};
// (re)allocates the grouping's buffers for L landmarks of K anchors; *moved as ensure() sets it
nnrt_status allocate_landmark_groups(LandmarkSet& lm, const LandmarkFrame& fr, bool* moved);
// enqueues the grouping on s, waits for it and checks the landmarks against the frame (NNRT_ERROR_ARGUMENT names the first
// landmark whose vertex is out of range or belongs to no face)
nnrt_status group_landmarks(LandmarkSet& lm, const LandmarkFrame& fr, hipStream_t s);

struct FitLandmarkArgs {
	int L, K;
	float term_weight, cutoff;
	int state_identity;
	const int32_t* index;
	const float* target;
	const float* weight;
	const int32_t* anchors;
	const float* weights;
	const float* mesh_p;          // [V, 3] canonical positions as stored
	const float4* wpos;           // [V] this iteration's warped positions
	const float* state_in;        // [N, 16]
	const uint64_t *node_keys, *pair_keys;
	const int *node_vals, *pair_vals;
	const int64_t *node_starts, *pair_starts;
	const int* info;
	double* acc;                  // [N, ACC_STRIDE]
	double* pair_acc;             // [M, 36] (null: block-diagonal data term)
	float4* distances;
	double* cost;
	int node_blocks, pair_blocks; // workgroups of the node runs and the pair runs; one more takes the distances and the cost
};
// run capacity of the launch for L landmarks (what its grid is sized by: a captured graph keeps it while L, K, N and M stay)
inline int64_t landmark_node_run_bound(int64_t L, int K, int N) { return std::min<int64_t>(L * K, N); }
inline int64_t landmark_pair_run_bound(int64_t L, int K, int M) { return std::min<int64_t>(L * K * (K - 1) / 2, M); }
nnrt_status launch_fit_landmarks(FitLandmarkArgs args, hipStream_t stream);

} // namespace nnrt
