// Rasterizer fragments -> an image, and the rasterized model depth against a depth frame.
//
// k_shade_pixels: the reference's FlatEdgeShader (cpp/rendering/kernel/FlatEdgeShaderImpl.h:66-98) and VertexColorShader
// (cpp/rendering/VertexColorShader.cpp:29-61 over InterpolateFaceAttributesImpl.h:60-66), and a head-lit shader the
// reference does not have. One lane per pixel, pixels of a row on consecutive lanes; only the front fragment (slot 0 of
// the K slots of a pixel) is read. The reference gathers an [F,3,3] face-attribute tensor first; here a lane reads its
// face's three vertex indices and then the three vertex rows. Every pixel is written, the background as (0,0,0), so the
// output needs no zero fill. A face index >= face_count or a vertex index outside [0, vertex_count) is drawn as
// background instead of being read through.
//
// k_depth_agreement + k_depth_agreement_finish: model depth (slot 0) minus frame depth per pixel and the statistics of
// the pixels where both are valid. The sums are reproducible: a lane adds its pixels in ascending order in float64, a
// wavefront reduces by a fixed shuffle tree (offsets 32, 16, ..., 1), lane 0 of the workgroup adds the four wavefronts in
// wavefront order and stores one record per workgroup, and the one-workgroup finish launch adds the records in index
// order. No atomics, no workgroup waits on another.
//
// Float arithmetic is unfused and in the order written (the build's -ffp-contract=off; the pragmas keep it so), divides
// are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so a float32 restatement equals both bit for bit.
#include "agreement_sums.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {

constexpr int SB = 256;                 // threads per workgroup
constexpr int AGREEMENT_PIXELS = 8;     // pixels per lane of k_depth_agreement: pixel = (8 block + j) 256 + thread

// truncation toward zero of a float product; values <= 0 and NaN give 0, values >= 255 give 255 (the reference's cast
// is undefined outside [0, 255])
__device__ inline uint8_t to_byte(float x) {
	if (!(x > 0.f)) return 0;
	if (x >= 255.f) return 255;
	return static_cast<uint8_t>(static_cast<int>(x));
}

struct ShadeArguments {
	const int64_t* pixel_faces;   // [P, K]
	const float* barycentrics;    // [P, K, 3]
	const float* distances;       // [P, K]
	const int64_t* triangles;     // [F, 3]
	const float* colors;          // [V, 3]
	const float* normals;         // [V, 3]
	int64_t pixel_count;
	int64_t face_count;
	int64_t vertex_count;
	int K;
	float r, g, b;
	float ndc_line_width;
	float ambient;
};

template <int MODE>
__global__ void __launch_bounds__(SB) k_shade_pixels(ShadeArguments a, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
	const int64_t p = static_cast<int64_t>(blockIdx.x) * SB + threadIdx.x;
	if (p >= a.pixel_count) return;
	const int64_t fragment = p * a.K;
	const int64_t face = a.pixel_faces[fragment];
	uint8_t red = 0, green = 0, blue = 0;
	if (MODE == NNRT_SHADE_FLAT_EDGE) {
		if (face >= 0) {
			const float w2 = a.ndc_line_width * a.ndc_line_width;
			const float d = fabsf(a.distances[fragment]);
			if (d < w2) {
				const float factor = (w2 - d) / w2;
				red = to_byte(255.f * a.r * factor);
				green = to_byte(255.f * a.g * factor);
				blue = to_byte(255.f * a.b * factor);
			}
		}
	} else if (face >= 0 && face < a.face_count) {
		const int64_t i0 = a.triangles[3 * face], i1 = a.triangles[3 * face + 1], i2 = a.triangles[3 * face + 2];
		const bool inside = i0 >= 0 && i0 < a.vertex_count && i1 >= 0 && i1 < a.vertex_count && i2 >= 0 && i2 < a.vertex_count;
		if (inside) {
			const float b0 = a.barycentrics[3 * fragment], b1 = a.barycentrics[3 * fragment + 1], b2 = a.barycentrics[3 * fragment + 2];
			if (MODE == NNRT_SHADE_VERTEX_COLOR) {
				uint8_t rgb[3];
#pragma unroll
				for (int c = 0; c < 3; c++) {
					float v = 0.f;
					v = v + b0 * a.colors[3 * i0 + c];
					v = v + b1 * a.colors[3 * i1 + c];
					v = v + b2 * a.colors[3 * i2 + c];
					rgb[c] = to_byte(v * 255.f);
				}
				red = rgb[0], green = rgb[1], blue = rgb[2];
			} else {
				const float nx = (b0 * a.normals[3 * i0] + b1 * a.normals[3 * i1]) + b2 * a.normals[3 * i2];
				const float ny = (b0 * a.normals[3 * i0 + 1] + b1 * a.normals[3 * i1 + 1]) + b2 * a.normals[3 * i2 + 1];
				const float nz = (b0 * a.normals[3 * i0 + 2] + b1 * a.normals[3 * i1 + 2]) + b2 * a.normals[3 * i2 + 2];
				const float length = sqrtf((nx * nx + ny * ny) + nz * nz);
				float s = 0.f;
				if (length > 0.f && length <= 3.402823466e+38f) s = fmaxf(0.f, -nz / length);   // a light along the optical axis
				const float shade = a.ambient + (1.f - a.ambient) * s;
				red = to_byte(255.f * a.r * shade);
				green = to_byte(255.f * a.g * shade);
				blue = to_byte(255.f * a.b * shade);
			}
		}
	}
	out[3 * p] = red;
	out[3 * p + 1] = green;
	out[3 * p + 2] = blue;
}

// ------------------------------------------------------------------------------------------------- depth agreement ----
__device__ inline void store_record(nnrt_depth_agreement* record, const AgreementSums& s) {
	record->both = s.both;
	record->model_only = s.first_only;
	record->frame_only = s.second_only;
	record->inliers = s.inliers;
	record->sum_abs = s.sum;
	record->sum_sq = s.sum_sq;
	record->max_abs = s.max;
	record->reserved = 0;
}

template <typename T>
__global__ void __launch_bounds__(SB) k_depth_agreement(const int64_t* __restrict__ pixel_faces, const float* __restrict__ pixel_depths, int K,
                                                        const T* __restrict__ frame, int64_t pixel_count, float depth_scale, float depth_max,
                                                        float inlier_threshold, float* __restrict__ difference,
                                                        nnrt_depth_agreement* __restrict__ partials) {
#pragma clang fp contract(off)
	__shared__ AgreementSums s_waves[SB / 64];
	const int t = static_cast<int>(threadIdx.x);
	AgreementSums sums{0, 0, 0, 0, 0.0, 0.0, 0.f};
	const int64_t first = static_cast<int64_t>(blockIdx.x) * (SB * AGREEMENT_PIXELS) + t;
#pragma unroll
	for (int j = 0; j < AGREEMENT_PIXELS; j++) {
		const int64_t p = first + static_cast<int64_t>(j) * SB;
		if (p >= pixel_count) break;
		const bool model = pixel_faces[p * K] >= 0;
		const float z = static_cast<float>(frame[p]) / depth_scale;
		const bool seen = z > 0.f && z < depth_max;   // the unprojection's rule; false for NaN
		float d = __builtin_nanf("");
		if (model && seen) {
			d = pixel_depths[p * K] - z;
			const float magnitude = fabsf(d);
			const double wide = static_cast<double>(magnitude);
			sums.both += 1;
			sums.inliers += magnitude <= inlier_threshold ? 1 : 0;
			sums.sum = sums.sum + wide;
			sums.sum_sq = sums.sum_sq + wide * wide;
			sums.max = fmaxf(sums.max, magnitude);
		} else if (model) {
			sums.first_only += 1;
		} else if (seen) {
			sums.second_only += 1;
		}
		difference[p] = d;
	}
	for (int offset = 32; offset >= 1; offset >>= 1) sums.add(shuffled_down(sums, offset));
	if ((t & 63) == 0) s_waves[t >> 6] = sums;
	__syncthreads();
	if (t == 0) {
		for (int w = 1; w < SB / 64; w++) sums.add(s_waves[w]);
		store_record(partials + blockIdx.x, sums);
	}
}

// one workgroup; thread 0 adds the workgroups' records in index order
__global__ void __launch_bounds__(64) k_depth_agreement_finish(const nnrt_depth_agreement* __restrict__ partials, int count,
                                                               nnrt_depth_agreement* __restrict__ result) {
#pragma clang fp contract(off)
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	AgreementSums sums{0, 0, 0, 0, 0.0, 0.0, 0.f};
	for (int i = 0; i < count; i++) {
		const nnrt_depth_agreement r = partials[i];
		sums.add(AgreementSums{r.both, r.model_only, r.frame_only, r.inliers, r.sum_abs, r.sum_sq, r.max_abs});
	}
	store_record(result, sums);
}

} // namespace

nnrt_status launch_shade_pixels(int mode, const int64_t* pixel_faces, const float* barycentrics, const float* distances, int H, int W, int K,
                                const int64_t* triangles, int64_t face_count, const float* colors, const float* normals, int64_t vertex_count,
                                const float* color, float ndc_line_width, float ambient, uint8_t* out, hipStream_t stream) {
	const int64_t P = static_cast<int64_t>(H) * W;
	if (P == 0) return NNRT_OK;
	ShadeArguments a{pixel_faces, barycentrics, distances, triangles, colors, normals, P, face_count, vertex_count, K,
	                 color ? color[0] : 0.f, color ? color[1] : 0.f, color ? color[2] : 0.f, ndc_line_width, ambient};
	const unsigned grid = static_cast<unsigned>(ceil_div(P, SB));
	if (mode == NNRT_SHADE_VERTEX_COLOR)
		k_shade_pixels<NNRT_SHADE_VERTEX_COLOR><<<grid, SB, 0, stream>>>(a, out);
	else if (mode == NNRT_SHADE_FLAT_EDGE)
		k_shade_pixels<NNRT_SHADE_FLAT_EDGE><<<grid, SB, 0, stream>>>(a, out);
	else
		k_shade_pixels<NNRT_SHADE_HEADLIGHT><<<grid, SB, 0, stream>>>(a, out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

int64_t depth_agreement_partial_count(int H, int W) { return ceil_div(static_cast<int64_t>(H) * W, SB * AGREEMENT_PIXELS); }

nnrt_status launch_depth_agreement(const int64_t* pixel_faces, const float* pixel_depths, int H, int W, int K, const void* frame, int frame_dtype,
                                   float depth_scale, float depth_max, float inlier_threshold, float* difference,
                                   nnrt_depth_agreement* partials, nnrt_depth_agreement* result, hipStream_t stream) {
	const int64_t P = static_cast<int64_t>(H) * W;
	const int64_t groups = depth_agreement_partial_count(H, W);
	const unsigned grid = static_cast<unsigned>(groups);
	if (frame_dtype == NNRT_DTYPE_UINT16)
		k_depth_agreement<uint16_t><<<grid, SB, 0, stream>>>(pixel_faces, pixel_depths, K, static_cast<const uint16_t*>(frame), P, depth_scale,
		                                                    depth_max, inlier_threshold, difference, partials);
	else
		k_depth_agreement<float><<<grid, SB, 0, stream>>>(pixel_faces, pixel_depths, K, static_cast<const float*>(frame), P, depth_scale,
		                                                 depth_max, inlier_threshold, difference, partials);
	NNRT_LAUNCH_CHECK();
	k_depth_agreement_finish<<<1, 64, 0, stream>>>(partials, static_cast<int>(groups), result);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
