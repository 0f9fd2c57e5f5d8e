// Intensity images for the hybrid rigid alignment: RGB -> luminance, and the halving step of its
// pyramid. One lane per output pixel, float in the operation order written out below (tests/_rigid_hybrid_util.py repeats it).
#include "kernels.hpp"

namespace nnrt {

namespace {
// I = ((0.299 R + 0.587 G) + 0.114 B) / 255 of a uint8 [H, W, 3] image
__global__ __launch_bounds__(256) void k_intensity_rgb8(const uint8_t* __restrict__ rgb, int64_t count, float* __restrict__ out) {
#pragma clang fp contract(off)
	const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
	if (i >= count) return;
	const float r = static_cast<float>(rgb[3 * i]), g = static_cast<float>(rgb[3 * i + 1]), b = static_cast<float>(rgb[3 * i + 2]);
	out[i] = ((0.299f * r + 0.587f * g) + 0.114f * b) / 255.0f;
}

// out (i, j) = the 3 x 3 binomial mean centred on in (2 i, 2 j), indices clamped to the image: level pixel (i, j) stays
// image pixel (2 i, 2 j), the convention of the point image's [::2, ::2] decimation. Each of the three rows first,
// h = ((left + 2 centre) + right) / 4, then the column the same way over h in row order.
__global__ __launch_bounds__(256) void k_intensity_halve(const float* __restrict__ in, int H, int W, int Ho, int Wo, float* __restrict__ out) {
#pragma clang fp contract(off)
	const int64_t o = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
	if (o >= static_cast<int64_t>(Ho) * Wo) return;
	const int i = static_cast<int>(o / Wo), j = static_cast<int>(o % Wo);
	const int y1 = 2 * i, x1 = 2 * j;   // inside the image: Ho = ceil(H / 2), Wo = ceil(W / 2)
	const int y0 = max(y1 - 1, 0), y2 = min(y1 + 1, H - 1), x0 = max(x1 - 1, 0), x2 = min(x1 + 1, W - 1);
	const int ys[3] = {y0, y1, y2};
	float h[3];
#pragma unroll
	for (int r = 0; r < 3; r++) {
		const float* row = in + static_cast<int64_t>(ys[r]) * W;
		h[r] = ((row[x0] + 2.0f * row[x1]) + row[x2]) * 0.25f;
	}
	out[o] = ((h[0] + 2.0f * h[1]) + h[2]) * 0.25f;
}
} // namespace

nnrt_status launch_intensity_rgb8(const uint8_t* rgb, int H, int W, float* out, hipStream_t stream) {
	const int64_t count = static_cast<int64_t>(H) * W;
	k_intensity_rgb8<<<static_cast<unsigned>(ceil_div(count, 256)), 256, 0, stream>>>(rgb, count, out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_intensity_halve(const float* in, int H, int W, float* out, hipStream_t stream) {
	const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
	const int64_t count = static_cast<int64_t>(Ho) * Wo;
	k_intensity_halve<<<static_cast<unsigned>(ceil_div(count, 256)), 256, 0, stream>>>(in, H, W, Ho, Wo, out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
