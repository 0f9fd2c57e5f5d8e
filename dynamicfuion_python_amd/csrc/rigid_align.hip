// Rigid frame-to-model alignment on gfx950: dense, projective, point-to-plane Gauss-Newton of
// model vertices and normals against an organized live point image, the rigid step DynamicFusion runs before the
// non-rigid fit (reference apps/fusion/pipeline.py:338-354, which delegates it to Open3D).
//
// k_rigid_accumulate: one lane per model vertex, grid-stride over a workgroup count that depends on V alone. The
// per-vertex terms are float, in the operation order written out below (tests/_rigid_align_util.py repeats it); the
// residual r and the Jacobian row J = [q x g, g] are then widened to double, where the product of two floats is exact,
// and summed into 29 per-lane doubles (21 upper products J_i J_j, 6 products J_i r, r^2, 1). Lanes reduce by
// __shfl_xor with strides 32 -> 1, waves through LDS in wave order, one [29] row per workgroup: the order of every sum
// is fixed by V, so the result is bit-reproducible. No atomics.
// k_rigid_accumulate<true> is the hybrid build: a vertex whose geometric row was kept also samples
// the live intensity image bilinearly at its unrounded pixel and adds the row of rI = I(u, v) - c, scaled by the
// photometric weight, to the same 27 sums; sum rI^2 and the photometric count follow as sums 29 and 30 (31 per lane).
// The <false> build is the geometric kernel as it was: the same statements in the same order.
// k_rigid_solve_update: one wave adds the rows in index order, logs (count, sum r^2), solves the 6 x 6 system by double
// Cholesky and left-multiplies the pose by exp(xi^). A degenerate system leaves the pose as it is and raises a status bit.
#include <cmath>
#include <vector>

#include "kernels.hpp"

namespace nnrt {

namespace {
constexpr int RA_BLOCK = 256;
constexpr int RA_WAVES = RA_BLOCK / 64;
constexpr int RA_MAX_BLOCKS = 256;
constexpr int RA_SUMS = 29;          // 21 + 6 + 1 + 1
constexpr int RA_SUMS_HYBRID = 31;   // + sum rI^2 + photometric count

struct RigidCamera {
	float fx, fy, cx, cy;
	int H, W;
};

// the hybrid build's further inputs: model colours [V, 3], the level's intensity image [H, W], weight and |rI| threshold (<= 0: off)
struct RigidPhotometric {
	const float* colors;
	const float* intensity;
	float weight, threshold;
};

template <bool PHOTO>
__global__ __launch_bounds__(RA_BLOCK) void k_rigid_accumulate(const float* __restrict__ points, const float* __restrict__ normals, int64_t V,
                                                               const float* __restrict__ target_points,
                                                               const float* __restrict__ target_normals, RigidCamera cam,
                                                               const double* __restrict__ pose, float tau2, float min_cos, int cull,
                                                               RigidPhotometric photo, double* __restrict__ rows) {
#pragma clang fp contract(off)
	constexpr int NS = PHOTO ? RA_SUMS_HYBRID : RA_SUMS;   // sums per lane
	__shared__ double wave_sums[RA_WAVES][NS];
	float T[12];
#pragma unroll
	for (int k = 0; k < 12; k++) T[k] = static_cast<float>(pose[k]);
	double acc[NS];
#pragma unroll
	for (int k = 0; k < NS; k++) acc[k] = 0.0;
	const int64_t stride = static_cast<int64_t>(gridDim.x) * RA_BLOCK;
	for (int64_t i = static_cast<int64_t>(blockIdx.x) * RA_BLOCK + threadIdx.x; i < V; i += stride) {
		const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
		const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
		// 1, 2: q = R p + t, m = R n
		const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
		const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
		const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
		const float mx = (T[0] * nx + T[1] * ny) + T[2] * nz;
		const float my = (T[4] * nx + T[5] * ny) + T[6] * nz;
		const float mz = (T[8] * nx + T[9] * ny) + T[10] * nz;
		// 3
		if (!(isfinite(qx) && isfinite(qy) && isfinite(qz) && qz > 0.f)) continue;
		// 4: the pixel, compared as floats before the conversion (a huge or infinite u never reaches the cast)
		const float u = cam.fx * (qx / qz) + cam.cx, v = cam.fy * (qy / qz) + cam.cy;
		const float uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
		if (!(uf >= 0.f && uf < static_cast<float>(cam.W) && vf >= 0.f && vf < static_cast<float>(cam.H))) continue;
		const int ui = static_cast<int>(uf), vi = static_cast<int>(vf);
		// 5
		const int64_t pix = static_cast<int64_t>(vi) * cam.W + ui;
		const float dx = target_points[3 * pix], dy = target_points[3 * pix + 1], dz = target_points[3 * pix + 2];
		const float gx = target_normals[3 * pix], gy = target_normals[3 * pix + 1], gz = target_normals[3 * pix + 2];
		if (!(isfinite(dx) && isfinite(dy) && isfinite(dz) && isfinite(gx) && isfinite(gy) && isfinite(gz) && dz > 0.f)) continue;
		if (gx == 0.f && gy == 0.f && gz == 0.f) continue;
		// 6
		const float ex = qx - dx, ey = qy - dy, ez = qz - dz;
		if ((ex * ex + ey * ey) + ez * ez > tau2) continue;
		// 7: kept only where |m . g| >= c, so a NaN normal is dropped while the test is on
		if (min_cos > 0.f && !(fabsf((mx * gx + my * gy) + mz * gz) >= min_cos)) continue;
		// 8
		if (cull && (mx * qx + my * qy) + mz * qz >= 0.f) continue;
		// 9
		const float r = (gx * ex + gy * ey) + gz * ez;
		const float J[6] = {qy * gz - qz * gy, qz * gx - qx * gz, qx * gy - qy * gx, gx, gy, gz};
		if (!(isfinite(r) && isfinite(J[0]) && isfinite(J[1]) && isfinite(J[2]))) continue;   // a row that overflowed float
		double Jd[6];
#pragma unroll
		for (int a = 0; a < 6; a++) Jd[a] = static_cast<double>(J[a]);
		const double rd = static_cast<double>(r);
		int k = 0;
#pragma unroll
		for (int a = 0; a < 6; a++) {
#pragma unroll
			for (int b = a; b < 6; b++) acc[k++] += Jd[a] * Jd[b];
		}
#pragma unroll
		for (int a = 0; a < 6; a++) acc[21 + a] += Jd[a] * rd;
		acc[27] += rd * rd;
		acc[28] += 1.0;
		if constexpr (PHOTO) {
			// P1: the model's intensity
			const float cr = photo.colors[3 * i], cg = photo.colors[3 * i + 1], cb = photo.colors[3 * i + 2];
			const float c = (0.299f * cr + 0.587f * cg) + 0.114f * cb;
			if (!isfinite(c)) continue;
			// P2: the four taps around the unrounded pixel of step 4, compared as floats before the conversion
			const float u0f = floorf(u), v0f = floorf(v);
			if (!(u0f >= 0.f && u0f + 1.f <= static_cast<float>(cam.W - 1) && v0f >= 0.f && v0f + 1.f <= static_cast<float>(cam.H - 1))) continue;
			const float a = u - u0f, b = v - v0f;
			// P3: every tap holds a target and a finite intensity
			const int64_t t00 = static_cast<int64_t>(static_cast<int>(v0f)) * cam.W + static_cast<int>(u0f);
			const int64_t t01 = t00 + 1, t10 = t00 + cam.W, t11 = t10 + 1;
			const float z00 = target_points[3 * t00 + 2], z01 = target_points[3 * t01 + 2];
			const float z10 = target_points[3 * t10 + 2], z11 = target_points[3 * t11 + 2];
			if (!(isfinite(z00) && z00 > 0.f && isfinite(z01) && z01 > 0.f && isfinite(z10) && z10 > 0.f && isfinite(z11) && z11 > 0.f)) continue;
			const float I00 = photo.intensity[t00], I01 = photo.intensity[t01], I10 = photo.intensity[t10], I11 = photo.intensity[t11];
			if (!(isfinite(I00) && isfinite(I01) && isfinite(I10) && isfinite(I11))) continue;
			// P4: the sample and the exact gradient of the sampled function
			const float top = I00 + a * (I01 - I00);
			const float bot = I10 + a * (I11 - I10);
			const float Iuv = top + b * (bot - top);
			const float Iu = (I01 - I00) + b * ((I11 - I10) - (I01 - I00));
			const float Iv = bot - top;
			// P5
			const float rI = Iuv - c;
			if (photo.threshold > 0.f && !(fabsf(rI) <= photo.threshold)) continue;
			// P6: gI = dI/dq through the projection, row [q x gI, gI], both scaled by the weight
			const float gIx = (Iu * cam.fx) / qz;
			const float gIy = (Iv * cam.fy) / qz;
			const float gIz = -(((Iu * cam.fx) * qx + (Iv * cam.fy) * qy) / (qz * qz));
			const float JI[6] = {photo.weight * (qy * gIz - qz * gIy), photo.weight * (qz * gIx - qx * gIz), photo.weight * (qx * gIy - qy * gIx),
			                     photo.weight * gIx, photo.weight * gIy, photo.weight * gIz};
			const float rIw = photo.weight * rI;
			if (!(isfinite(rIw) && isfinite(JI[0]) && isfinite(JI[1]) && isfinite(JI[2]) && isfinite(JI[3]) && isfinite(JI[4]) && isfinite(JI[5])))
				continue;
			double JId[6];
#pragma unroll
			for (int e = 0; e < 6; e++) JId[e] = static_cast<double>(JI[e]);
			const double rId = static_cast<double>(rIw), rIu = static_cast<double>(rI);
			int kp = 0;
#pragma unroll
			for (int e = 0; e < 6; e++) {
#pragma unroll
				for (int f = e; f < 6; f++) acc[kp++] += JId[e] * JId[f];
			}
#pragma unroll
			for (int e = 0; e < 6; e++) acc[21 + e] += JId[e] * rId;
			acc[29] += rIu * rIu;
			acc[30] += 1.0;
		}
	}
	// lanes of a wave, strides 32 -> 1; every lane of the workgroup arrives here
#pragma unroll
	for (int k = 0; k < NS; k++) {
		double s = acc[k];
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
		acc[k] = s;
	}
	const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < NS; k++) wave_sums[wave][k] = acc[k];
	}
	__syncthreads();
	if (threadIdx.x < NS) {
		double s = wave_sums[0][threadIdx.x];
#pragma unroll
		for (int w = 1; w < RA_WAVES; w++) s += wave_sums[w][threadIdx.x];
		rows[static_cast<int64_t>(blockIdx.x) * NS + threadIdx.x] = s;
	}
}

// exp of the twist (w, v): R = I + a K + b K^2, V = I + b K + c K^2 with K = hat(w), a = sin(th) / th,
// b = (1 - cos(th)) / th^2 (as 2 sin^2(th / 2) / th^2: no cancellation), c = (th - sin(th)) / th^3; below 1e-8 their series
__device__ inline void se3_exp(const double* xi, double (&R)[3][3], double (&t)[3]) {
	const double wx = xi[0], wy = xi[1], wz = xi[2];
	const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
	double a, b, c;
	if (th < 1e-8) {
		a = 1.0 - th2 / 6.0;
		b = 0.5 - th2 / 24.0;
		c = 1.0 / 6.0 - th2 / 120.0;
	} else {
		const double s = sin(th), h = sin(0.5 * th);
		a = s / th;
		b = 2.0 * h * h / th2;
		c = (th - s) / (th2 * th);
	}
	const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
	double K2[3][3];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) K2[i][j] = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
	for (int i = 0; i < 3; i++) {
		double ti = 0.0;
		for (int j = 0; j < 3; j++) {
			const double id = i == j ? 1.0 : 0.0;
			R[i][j] = (id + a * K[i][j]) + b * K2[i][j];
			ti += ((id + b * K[i][j]) + c * K2[i][j]) * xi[3 + j];
		}
		t[i] = ti;
	}
}

// row_stride: the sums per row, RA_SUMS or RA_SUMS_HYBRID; the hybrid log row is (count, sum r^2, photometric count, sum rI^2)
__global__ __launch_bounds__(64) void k_rigid_solve_update(const double* __restrict__ rows, int row_count, int row_stride, int iteration,
                                                           double min_count, double* __restrict__ pose, double* __restrict__ log,
                                                           int32_t* __restrict__ status) {
#pragma clang fp contract(off)
	__shared__ double sums[RA_SUMS_HYBRID];
	if (static_cast<int>(threadIdx.x) < row_stride) {
		double s = 0.0;
#pragma unroll 8   // the loads of a batch go out together; the additions keep their index order
		for (int g = 0; g < row_count; g++) s += rows[static_cast<int64_t>(g) * row_stride + threadIdx.x];
		sums[threadIdx.x] = s;
	}
	__syncthreads();
	if (threadIdx.x != 0) return;
	if (row_stride == RA_SUMS_HYBRID) {
		log[4 * iteration] = sums[28];
		log[4 * iteration + 1] = sums[27];
		log[4 * iteration + 2] = sums[30];
		log[4 * iteration + 3] = sums[29];
	} else {
		log[2 * iteration] = sums[28];
		log[2 * iteration + 1] = sums[27];
	}
	double A[6][6], x[6];
	int k = 0;
	double max_diag = 0.0;
	for (int a = 0; a < 6; a++) {
		for (int b = a; b < 6; b++) {
			A[a][b] = sums[k];
			A[b][a] = sums[k];
			k++;
		}
		x[a] = -sums[21 + a];
		max_diag = fmax(max_diag, A[a][a]);
	}
	bool ok = sums[28] >= min_count;
	const double floor_pivot = 1e-12 * max_diag;
	// lower Cholesky in place, a pivot at or below the floor (or NaN) ends it
	for (int j = 0; j < 6 && ok; j++) {
		double s = A[j][j];
		for (int c = 0; c < j; c++) s -= A[j][c] * A[j][c];
		if (!(s > floor_pivot) || !(s > 0.0)) {
			ok = false;
			break;
		}
		const double l = sqrt(s);
		A[j][j] = l;
		for (int i = j + 1; i < 6; i++) {
			double t = A[i][j];
			for (int c = 0; c < j; c++) t -= A[i][c] * A[j][c];
			A[i][j] = t / l;
		}
	}
	double out[12];
	if (ok) {
		for (int i = 0; i < 6; i++) {
			double s = x[i];
			for (int c = 0; c < i; c++) s -= A[i][c] * x[c];
			x[i] = s / A[i][i];
		}
		for (int i = 5; i >= 0; i--) {
			double s = x[i];
			for (int c = i + 1; c < 6; c++) s -= A[c][i] * x[c];
			x[i] = s / A[i][i];
		}
		double R[3][3], t[3];
		se3_exp(x, R, t);
		for (int i = 0; i < 3; i++) {
			for (int j = 0; j < 4; j++) out[4 * i + j] = (R[i][0] * pose[j] + R[i][1] * pose[4 + j]) + R[i][2] * pose[8 + j];
			out[4 * i + 3] += t[i];
		}
		for (int i = 0; i < 12; i++) ok = ok && isfinite(out[i]);
	}
	if (ok) {
		for (int i = 0; i < 12; i++) pose[i] = out[i];
	} else {
		*status = *status | NNRT_RIGID_ALIGN_DEGENERATE;
	}
}
} // namespace

nnrt_status launch_rigid_align(const float* points, const float* normals, int64_t V, const float* target_points, const float* target_normals, int H,
                               int W, float fx, float fy, float cx, float cy, const double* h_T_init, int iterations, float distance_threshold,
                               float normal_agreement_cos, int cull_back_faces, int minimum_correspondence_count, double* h_T_out, double* h_log,
                               int32_t* h_status, hipStream_t stream, const float* colors, const float* target_intensity,
                               float photometric_weight, float photometric_residual_threshold) {
	const bool hybrid = colors != nullptr;
	const int sums = hybrid ? RA_SUMS_HYBRID : RA_SUMS, log_columns = hybrid ? 4 : 2;
	const int G = static_cast<int>(std::min<int64_t>(ceil_div(V, RA_BLOCK), RA_MAX_BLOCKS));   // from V alone: reproducible sums
	const size_t row_bytes = sizeof(double) * sums * G, log_bytes = sizeof(double) * log_columns * iterations;
	// one allocation: rows [G, 29 or 31], pose [12], log [iterations, 2 or 4] (doubles), then the status word
	StreamScratch<char> work;
	if (nnrt_status st = work.alloc(row_bytes + sizeof(double) * 12 + log_bytes + sizeof(int32_t), stream)) return st;
	double* rows = reinterpret_cast<double*>(work.ptr);
	double* pose = rows + static_cast<size_t>(sums) * G;
	double* log = pose + 12;
	int32_t* status = reinterpret_cast<int32_t*>(log + log_columns * static_cast<size_t>(iterations));
	double host_pose[12];
	for (int k = 0; k < 12; k++) host_pose[k] = h_T_init[k];
	std::vector<double> host_log(log_columns * static_cast<size_t>(iterations), 0.0);
	int32_t host_status = 0;
	const RigidCamera cam{fx, fy, cx, cy, H, W};
	const RigidPhotometric photo{colors, target_intensity, photometric_weight, photometric_residual_threshold};
	const float tau2 = distance_threshold * distance_threshold;
	hipError_t e = hipMemcpyAsync(pose, host_pose, sizeof(host_pose), hipMemcpyHostToDevice, stream);
	if (e == hipSuccess) e = hipMemsetAsync(log, 0, log_bytes + sizeof(int32_t), stream);
	for (int it = 0; it < iterations && e == hipSuccess; it++) {
		if (hybrid)
			k_rigid_accumulate<true><<<G, RA_BLOCK, 0, stream>>>(points, normals, V, target_points, target_normals, cam, pose, tau2,
			                                                     normal_agreement_cos, cull_back_faces, photo, rows);
		else
			k_rigid_accumulate<false><<<G, RA_BLOCK, 0, stream>>>(points, normals, V, target_points, target_normals, cam, pose, tau2,
			                                                      normal_agreement_cos, cull_back_faces, photo, rows);
		k_rigid_solve_update<<<1, 64, 0, stream>>>(rows, G, sums, it, static_cast<double>(minimum_correspondence_count), pose, log, status);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(host_pose, pose, sizeof(host_pose), hipMemcpyDeviceToHost, stream);
	if (e == hipSuccess) e = hipMemcpyAsync(host_log.data(), log, log_bytes, hipMemcpyDeviceToHost, stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&host_status, status, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
	const hipError_t se = hipStreamSynchronize(stream);   // also on an error: the host buffers above outlive every copy
	NNRT_HIP(e);
	NNRT_HIP(se);
	for (int k = 0; k < 12; k++) h_T_out[k] = host_pose[k];
	h_T_out[12] = h_T_out[13] = h_T_out[14] = 0.0;
	h_T_out[15] = 1.0;
	for (size_t k = 0; k < host_log.size(); k++) h_log[k] = host_log[k];
	*h_status = host_status;
	return NNRT_OK;
}

} // namespace nnrt
