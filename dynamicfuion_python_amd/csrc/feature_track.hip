// Sparse feature tracker over intensity images: Shi-Tomasi corner scores, the selection of the
// strongest separated corners, and pyramidal Lucas-Kanade tracking (Bouguet's scheme) with one wavefront per feature.
// The arithmetic is the one include/nnrt_mi355x.h states for nnrt_corner_scores, nnrt_select_features and
// nnrt_track_features (tests/_feature_track_util.py repeats it). Float operations in the order written; the sums of
// products in float64 in a fixed order, no float atomics: two runs are bit-identical.
#include <algorithm>

#include "device_primitives.hpp"
#include "kernels.hpp"

namespace nnrt {

namespace {

// -------- corner scores --------
// A workgroup scores CS_BX x CS_BY pixels from an intensity tile with a ring of r + 1 pixels, held in LDS together with
// the two gradient tiles (ring r) formed from it. Tile pixels outside the image repeat the edge: they reach only pixels
// whose window leaves the image, which score 0.
constexpr int CS_BX = 32, CS_BY = 8, CS_RMAX = NNRT_FEATURE_MAX_WINDOW_RADIUS;
constexpr int CS_TW = CS_BX + 2 * CS_RMAX + 2, CS_TH = CS_BY + 2 * CS_RMAX + 2;
constexpr int CS_GW = CS_BX + 2 * CS_RMAX, CS_GH = CS_BY + 2 * CS_RMAX;

__global__ __launch_bounds__(256) void k_corner_score(const float* __restrict__ img, int H, int W, int r, float* __restrict__ out) {
#pragma clang fp contract(off)
	__shared__ float tile[CS_TH * CS_TW];
	__shared__ float gx[CS_GH * CS_GW], gy[CS_GH * CS_GW];
	const int bx0 = blockIdx.x * CS_BX, by0 = blockIdx.y * CS_BY;
	const int tw = CS_BX + 2 * r + 2, th = CS_BY + 2 * r + 2;
	for (int t = threadIdx.x; t < tw * th; t += 256) {
		const int ty = t / tw, tx = t % tw;
		const int y = min(max(by0 + ty - r - 1, 0), H - 1), x = min(max(bx0 + tx - r - 1, 0), W - 1);
		tile[ty * CS_TW + tx] = img[static_cast<int64_t>(y) * W + x];
	}
	__syncthreads();
	const int gw = CS_BX + 2 * r, gh = CS_BY + 2 * r;
	for (int t = threadIdx.x; t < gw * gh; t += 256) {
		const int ty = t / gw, tx = t % gw;   // gradient (ty, tx) is tile pixel (ty + 1, tx + 1)
		gx[ty * CS_GW + tx] = 0.5f * (tile[(ty + 1) * CS_TW + tx + 2] - tile[(ty + 1) * CS_TW + tx]);
		gy[ty * CS_GW + tx] = 0.5f * (tile[(ty + 2) * CS_TW + tx + 1] - tile[ty * CS_TW + tx + 1]);
	}
	__syncthreads();
	const int lx = threadIdx.x % CS_BX, ly = threadIdx.x / CS_BX;
	const int x = bx0 + lx, y = by0 + ly;
	if (x >= W || y >= H) return;
	float score = 0.f;
	if (x - r - 1 >= 0 && x + r + 1 <= W - 1 && y - r - 1 >= 0 && y + r + 1 <= H - 1) {
		double a = 0.0, b = 0.0, c = 0.0;
		for (int j = 0; j <= 2 * r; j++) {
			for (int i = 0; i <= 2 * r; i++) {
				const double ix = gx[(ly + j) * CS_GW + lx + i], iy = gy[(ly + j) * CS_GW + lx + i];
				a += ix * ix;
				b += ix * iy;
				c += iy * iy;
			}
		}
		const double side = 2 * r + 1;
		const double lambda = 0.5 * ((a + c) - sqrt((a - c) * (a - c) + 4.0 * b * b)) / (side * side);
		const float s = static_cast<float>(lambda);
		if (isfinite(s)) score = s;
	}
	out[static_cast<int64_t>(y) * W + x] = score;
}

// -------- selection --------
// the largest finite positive score, as the bit pattern of the float (order-preserving for non-negative floats)
__global__ __launch_bounds__(256) void k_corner_max(const float* __restrict__ scores, int64_t count, unsigned* __restrict__ d_max) {
	const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
	unsigned v = 0;
	if (i < count) {
		const float s = scores[i];
		if (isfinite(s) && s > 0.f) v = __float_as_uint(s);
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = max(v, static_cast<unsigned>(__shfl_xor(static_cast<int>(v), off)));
	if ((threadIdx.x & 63) == 0 && v != 0) atomicMax(d_max, v);
}

// flag and key of every pixel: key = inverted score bits (high), pixel index (low), so ascending keys are descending
// scores with ties by ascending pixel index
__global__ __launch_bounds__(256) void k_corner_flags(const float* __restrict__ scores, const uint8_t* __restrict__ mask, int H, int W, int m,
                                                      float quality, const unsigned* __restrict__ d_max, uint64_t* __restrict__ keys,
                                                      uint8_t* __restrict__ flags) {
#pragma clang fp contract(off)
	const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
	if (idx >= static_cast<int64_t>(H) * W) return;
	const int y = static_cast<int>(idx / W), x = static_cast<int>(idx % W);
	const float s = scores[idx];
	const float bar = quality * __uint_as_float(*d_max);
	bool keep = isfinite(s) && s > 0.f && s >= bar && (mask == nullptr || mask[idx] != 0);
	if (keep) {
		const int y0 = max(y - m, 0), y1 = min(y + m, H - 1), x0 = max(x - m, 0), x1 = min(x + m, W - 1);
		for (int yy = y0; yy <= y1 && keep; yy++) {
			for (int xx = x0; xx <= x1; xx++) {
				const int64_t j = static_cast<int64_t>(yy) * W + xx;
				const float o = scores[j];
				if (o > s || (o == s && j < idx)) {
					keep = false;
					break;
				}
			}
		}
	}
	keys[idx] = (static_cast<uint64_t>(~__float_as_uint(s)) << 32) | static_cast<uint32_t>(idx);
	flags[idx] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_feature_points(const uint64_t* __restrict__ sorted, int count, int W, float* __restrict__ out) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= count) return;
	const uint32_t idx = static_cast<uint32_t>(sorted[k] & 0xffffffffull);
	out[2 * k] = static_cast<float>(idx % static_cast<uint32_t>(W));
	out[2 * k + 1] = static_cast<float>(idx / static_cast<uint32_t>(W));
}

// -------- pyramidal Lucas-Kanade --------
struct TrackPyramids {
	const float* a[NNRT_FEATURE_MAX_LEVELS];
	const float* b[NNRT_FEATURE_MAX_LEVELS];
	int h[NNRT_FEATURE_MAX_LEVELS], w[NNRT_FEATURE_MAX_LEVELS];
};
struct TrackOptions {
	int levels, r, max_iterations;
	float epsilon, min_eigen_threshold, max_residual, forward_backward_threshold;
};

constexpr int TRACK_WAVES = 4;                                        // features per workgroup, one wave each
constexpr int TRACK_SLOTS = ((2 * CS_RMAX + 1) * (2 * CS_RMAX + 1) + 63) / 64;   // window pixels per lane

// every lane ends with the sum over the wave: xor butterfly, the same order in every run
__device__ inline double wave_sum(double v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
	return v;
}

// the whole window of margin `m` about (x, y) lies on pixel centres of a W x H image
__device__ inline bool window_inside(float x, float y, int m, int W, int H) {
	const float mf = static_cast<float>(m);
	return x - mf >= 0.f && x + mf <= static_cast<float>(W - 1) && y - mf >= 0.f && y + mf <= static_cast<float>(H - 1);
}

// bilinear sample in the form of nnrt_rigid_align_hybrid (top, bot, then blend). The caller has checked the position;
// the clamps keep x = W - 1 (a = 1) and anything unforeseen inside the image.
__device__ inline float bilinear(const float* __restrict__ img, int W, int H, float x, float y) {
#pragma clang fp contract(off)
	const int x0 = min(max(static_cast<int>(floorf(x)), 0), W - 2), y0 = min(max(static_cast<int>(floorf(y)), 0), H - 2);
	const float a = x - static_cast<float>(x0), b = y - static_cast<float>(y0);
	const float* row = img + static_cast<int64_t>(y0) * W + x0;
	const float i00 = row[0], i01 = row[1], i10 = row[W], i11 = row[W + 1];
	const float top = i00 + a * (i01 - i00), bot = i10 + a * (i11 - i10);
	return top + b * (bot - top);
}

__global__ __launch_bounds__(64 * TRACK_WAVES) void k_track_lk(TrackPyramids pyr, TrackOptions o, const float* __restrict__ points,
                                                                const float* __restrict__ initial_flow, const float* __restrict__ reference,
                                                                int n, float* __restrict__ out_points, uint8_t* __restrict__ out_status,
                                                                float* __restrict__ out_residual) {
#pragma clang fp contract(off)
	const int f = blockIdx.x * TRACK_WAVES + (threadIdx.x >> 6);   // one feature per wave: everything below is wave-uniform
	const int lane = threadIdx.x & 63;
	if (f >= n) return;
	const float px = points[2 * f], py = points[2 * f + 1];
	auto finish = [&](int status, float x, float y, float residual) {
		if (lane == 0) {
			out_points[2 * f] = x;
			out_points[2 * f + 1] = y;
			out_status[f] = static_cast<uint8_t>(status);
			out_residual[f] = residual;
		}
	};
	float gx = 0.f, gy = 0.f;
	if (initial_flow) {
		const float top = 1.0f / static_cast<float>(1 << (o.levels - 1));
		gx = initial_flow[2 * f] * top;
		gy = initial_flow[2 * f + 1] * top;
	}
	if (!(isfinite(px) && isfinite(py) && isfinite(gx) && isfinite(gy))) return finish(NNRT_FEATURE_NON_FINITE, px, py, 0.f);

	const int r = o.r, side = 2 * r + 1, pixels = side * side;
	bool valid[TRACK_SLOTS];
	float wi[TRACK_SLOTS], wj[TRACK_SLOTS];   // this lane's window offsets (i along x, j along y); (0, 0) where it has none
#pragma unroll
	for (int k = 0; k < TRACK_SLOTS; k++) {
		const int idx = lane + 64 * k;
		valid[k] = idx < pixels;
		wi[k] = valid[k] ? static_cast<float>(idx % side - r) : 0.f;
		wj[k] = valid[k] ? static_cast<float>(idx / side - r) : 0.f;
	}
	const double eps2 = static_cast<double>(o.epsilon) * static_cast<double>(o.epsilon);

	for (int l = o.levels - 1; l >= 0; l--) {
		const float scale = 1.0f / static_cast<float>(1 << l);
		const float plx = px * scale, ply = py * scale;
		const int W = pyr.w[l], H = pyr.h[l];
		const float* __restrict__ A = pyr.a[l];
		const float* __restrict__ B = pyr.b[l];
		bool skip = false;
		double gxx = 0.0, gxy = 0.0, gyy = 0.0;
		float T[TRACK_SLOTS], Tx[TRACK_SLOTS], Ty[TRACK_SLOTS];
		if (!window_inside(plx, ply, r + 1, W, H)) {
			if (l == 0) return finish(NNRT_FEATURE_OUT_OF_IMAGE, px, py, 0.f);
			skip = true;
		} else {
#pragma unroll
			for (int k = 0; k < TRACK_SLOTS; k++) {
				const float x = plx + wi[k], y = ply + wj[k];
				T[k] = bilinear(A, W, H, x, y);
				Tx[k] = 0.5f * (bilinear(A, W, H, x + 1.0f, y) - bilinear(A, W, H, x - 1.0f, y));
				Ty[k] = 0.5f * (bilinear(A, W, H, x, y + 1.0f) - bilinear(A, W, H, x, y - 1.0f));
				if (valid[k]) {
					const double tx = Tx[k], ty = Ty[k];
					gxx += tx * tx;
					gxy += tx * ty;
					gyy += ty * ty;
				}
			}
			gxx = wave_sum(gxx);
			gxy = wave_sum(gxy);
			gyy = wave_sum(gyy);
			const double min_eigen = 0.5 * ((gxx + gyy) - sqrt((gxx - gyy) * (gxx - gyy) + 4.0 * gxy * gxy)) / static_cast<double>(pixels);
			if (!isfinite(min_eigen)) return finish(NNRT_FEATURE_NON_FINITE, px, py, 0.f);
			if (min_eigen < static_cast<double>(o.min_eigen_threshold)) {
				if (l == 0) return finish(NNRT_FEATURE_FLAT, px, py, 0.f);
				skip = true;
			}
		}
		if (skip) {
			gx = 2.0f * gx;
			gy = 2.0f * gy;
			continue;
		}
		const double det = gxx * gyy - gxy * gxy;
		float vx = 0.f, vy = 0.f;
		for (int it = 0; it < o.max_iterations; it++) {
			const float qx = (plx + gx) + vx, qy = (ply + gy) + vy;
			if (!(isfinite(qx) && isfinite(qy))) return finish(NNRT_FEATURE_NON_FINITE, px, py, 0.f);
			if (!window_inside(qx, qy, r, W, H)) return finish(NNRT_FEATURE_OUT_OF_IMAGE, px, py, 0.f);
			double bx = 0.0, by = 0.0;
#pragma unroll
			for (int k = 0; k < TRACK_SLOTS; k++) {
				const float e = T[k] - bilinear(B, W, H, qx + wi[k], qy + wj[k]);
				if (valid[k]) {
					bx += static_cast<double>(e) * static_cast<double>(Tx[k]);
					by += static_cast<double>(e) * static_cast<double>(Ty[k]);
				}
			}
			bx = wave_sum(bx);
			by = wave_sum(by);
			const double dx = (gyy * bx - gxy * by) / det, dy = (gxx * by - gxy * bx) / det;
			if (!(isfinite(dx) && isfinite(dy))) return finish(NNRT_FEATURE_NON_FINITE, px, py, 0.f);
			vx += static_cast<float>(dx);
			vy += static_cast<float>(dy);
			if (o.epsilon > 0.f && dx * dx + dy * dy < eps2) break;
		}
		if (l > 0) {
			gx = 2.0f * (gx + vx);
			gy = 2.0f * (gy + vy);
			continue;
		}
		// level 0: the result, its residual and the checks on them
		const float rx = (px + gx) + vx, ry = (py + gy) + vy;
		if (!(isfinite(rx) && isfinite(ry))) return finish(NNRT_FEATURE_NON_FINITE, px, py, 0.f);
		if (!window_inside(rx, ry, r, W, H)) return finish(NNRT_FEATURE_OUT_OF_IMAGE, px, py, 0.f);
		double sum = 0.0;
#pragma unroll
		for (int k = 0; k < TRACK_SLOTS; k++) {
			const float e = T[k] - bilinear(B, W, H, rx + wi[k], ry + wj[k]);
			if (valid[k]) sum += static_cast<double>(fabsf(e));
		}
		const float residual = static_cast<float>(wave_sum(sum) / static_cast<double>(pixels));
		if (!isfinite(residual)) return finish(NNRT_FEATURE_NON_FINITE, px, py, 0.f);
		if (o.max_residual > 0.f && residual > o.max_residual) return finish(NNRT_FEATURE_RESIDUAL, px, py, residual);
		if (reference) {
			const float ex = rx - reference[2 * f], ey = ry - reference[2 * f + 1];
			const float bar = o.forward_backward_threshold * o.forward_backward_threshold;
			if (!(ex * ex + ey * ey <= bar)) return finish(NNRT_FEATURE_FB_FAILED, px, py, residual);
		}
		return finish(NNRT_FEATURE_TRACKED, rx, ry, residual);
	}
}

} // namespace

nnrt_status launch_corner_scores(const float* intensity, int H, int W, int r, float* out, hipStream_t stream) {
	const dim3 grid(static_cast<unsigned>(ceil_div(W, CS_BX)), static_cast<unsigned>(ceil_div(H, CS_BY)));
	k_corner_score<<<grid, 256, 0, stream>>>(intensity, H, W, r, out);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_select_features(const float* scores, const uint8_t* mask, int H, int W, float quality, int nms_radius, int max_count,
                                   float* out_points, int64_t* h_count, hipStream_t s) {
	const int64_t count = static_cast<int64_t>(H) * W;
	const unsigned blocks = static_cast<unsigned>(ceil_div(count, 256));
	nnrt_status st;
	DeviceBuffer<uint64_t> keys, candidates, sorted;
	DeviceBuffer<uint8_t> flags;
	DeviceBuffer<unsigned> d_max;
	DeviceBuffer<int> d_count;
	Scratch tmp;
	if ((st = keys.ensure(count)) || (st = candidates.ensure(count)) || (st = flags.ensure(count)) || (st = d_max.ensure(1)) ||
	    (st = d_count.ensure(1)))
		return st;
	NNRT_HIP(hipMemsetAsync(d_max.ptr, 0, sizeof(unsigned), s));
	NNRT_HIP(hipMemsetAsync(d_count.ptr, 0, sizeof(int), s));
	k_corner_max<<<blocks, 256, 0, s>>>(scores, count, d_max.ptr);
	NNRT_LAUNCH_CHECK();
	k_corner_flags<<<blocks, 256, 0, s>>>(scores, mask, H, W, nms_radius, quality, d_max.ptr, keys.ptr, flags.ptr);
	NNRT_LAUNCH_CHECK();
	if ((st = select_flagged(keys.ptr, flags.ptr, candidates.ptr, d_count.ptr, count, tmp, s))) return st;
	int found = 0;
	NNRT_HIP(hipMemcpyAsync(&found, d_count.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));   // the one read-back: the sort below takes its size from the host
	const int kept = std::min(found, max_count);
	*h_count = kept;
	if (kept == 0) return NNRT_OK;
	if ((st = sorted.ensure(found))) return st;
	if ((st = sort_keys(candidates.ptr, sorted.ptr, found, 64, tmp, s))) return st;
	k_feature_points<<<static_cast<unsigned>(ceil_div(kept, 256)), 256, 0, s>>>(sorted.ptr, kept, W, out_points);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

nnrt_status launch_track_features(const float* const* pyramid_a, const float* const* pyramid_b, const int* heights, const int* widths, int levels,
                                  const float* points, const float* initial_flow, const float* reference, int n, int r, int max_iterations,
                                  float epsilon, float min_eigen_threshold, float max_residual, float forward_backward_threshold,
                                  float* out_points, uint8_t* out_status, float* out_residual, hipStream_t stream) {
	TrackPyramids pyr{};
	for (int l = 0; l < levels; l++) {
		pyr.a[l] = pyramid_a[l];
		pyr.b[l] = pyramid_b[l];
		pyr.h[l] = heights[l];
		pyr.w[l] = widths[l];
	}
	const TrackOptions o{levels, r, max_iterations, epsilon, min_eigen_threshold, max_residual, forward_backward_threshold};
	k_track_lk<<<static_cast<unsigned>(ceil_div(n, TRACK_WAVES)), 64 * TRACK_WAVES, 0, stream>>>(pyr, o, points, initial_flow, reference, n,
	                                                                                              out_points, out_status, out_residual);
	NNRT_LAUNCH_CHECK();
	return NNRT_OK;
}

} // namespace nnrt
