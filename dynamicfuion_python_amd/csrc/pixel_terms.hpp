// The fitter's per-pixel and per-association arithmetic, stated once (DESIGN.md sections 5, 23, 25): the pixel resolve,
// the penalty step, the rasterized-surface record and the pixel-node Jacobian row. The fused pixel launch
// (k_fit_pixels_fused: pass 1 and pass 2's (2b)), the pair launch (k_fit_pairs) and the robust step cost
// (k_step_cost_robust) all call these functions, so the three agree bit for bit by construction (-ffp-contract=off: the
// same IEEE operations in the same order).
#pragma once

#include "fitter_kernels.hpp"

namespace nnrt {

// what the resolve reads of a frame
struct PixelResolveView {
	NdcSetup ndc;
	Camera pix;               // pixel-space intrinsics (float)
	float blur;               // NDC units
	PixelAxis ax, ay;         // pixel-centre NDC constants (make_pixel_axis)
	int perspective;
	const int4* faces4;       // [F]
	const float4* wpos;       // [V] warped positions
	const float4* wnrm;       // [V] warped normals
	const float4* ref_points; // [P] reference point (x, y, z, valid)
};
__host__ __device__ inline PixelResolveView pixel_resolve_view(const FitPixelArgs& a) {
	return PixelResolveView{a.ndc, a.pix, a.blur, a.ax, a.ay, a.perspective, a.faces4, a.wpos, a.wnrm, a.ref_points};
}

struct PixelResolve {
	int vid[3];          // the face's vertices
	int nodes;           // the face's distinct anchor nodes (k_face_node_table)
	f3 V3[3], N3[3];     // their warped positions / normals
	FaceNdc fn;
	float px, py;        // the pixel centre in NDC
	RasterHit h;
	f3 nl, d;            // the interpolated normal n_l and the point map vector w_l - o_l
	float dist;          // dot(n_l, w_l - o_l)
	bool ref_valid;
};

// pixel (u, v) before any face: its centre in NDC, no hit
__device__ __forceinline__ PixelResolve resolve_pixel(const PixelResolveView& w, int u, int v) {
	PixelResolve r;
	r.vid[0] = r.vid[1] = r.vid[2] = 0;
	r.px = pixel_ndc(u, w.ax);
	r.py = pixel_ndc(v, w.ay);
	r.h = RasterHit{0.f, 0.f, 0.f, 0.f, 0.f};
	return r;
}

// `face` at the pixel r was begun for: its vertices to NDC and the ray-face test; false: the face does not cover the
// pixel centre
__device__ __forceinline__ bool resolve_face(const PixelResolveView& w, int32_t face, PixelResolve& r) {
	const int4 fi = w.faces4[face];
	r.nodes = fi.w;
	r.vid[0] = fi.x;
	r.vid[1] = fi.y;
	r.vid[2] = fi.z;
#pragma unroll
	for (int i = 0; i < 3; i++) {
		const float4 wp = w.wpos[r.vid[i]];
		const float4 wn = w.wnrm[r.vid[i]];
		r.V3[i] = make3(wp.x, wp.y, wp.z);
		r.N3[i] = make3(wn.x, wn.y, wn.z);
		w.ndc.ndc.project(r.V3[i].x, r.V3[i].y, r.V3[i].z, &r.fn.x[i], &r.fn.y[i]);
		r.fn.z[i] = r.V3[i].z;
	}
	// the scatter accepted this face for this pixel after the full test; re-resolving needs no distance test
	return face_test<false>(r.fn, r.px, r.py, w.blur, w.perspective, false, true, r.h);
}

// ComputeDepthResiduals (:331-390) up to the raw point-to-plane distance of pixel p = (u, v): n_l where a face was hit,
// the rasterized point where its depth is valid (the caller's test), their distance to the reference point
__device__ __forceinline__ void resolve_distance(const PixelResolveView& w, int u, int v, int64_t p, bool hit, bool rendered_valid, PixelResolve& r) {
	const RasterHit& h = r.h;
	f3 nl = make3(0.f, 0.f, 0.f), prast = make3(0.f, 0.f, 0.f);
	if (hit) {
		float acc;
		acc = 0.0f;
		acc += h.b0 * r.N3[0].x;
		acc += h.b1 * r.N3[1].x;
		acc += h.b2 * r.N3[2].x;
		nl.x = acc;
		acc = 0.0f;
		acc += h.b0 * r.N3[0].y;
		acc += h.b1 * r.N3[1].y;
		acc += h.b2 * r.N3[2].y;
		nl.y = acc;
		acc = 0.0f;
		acc += h.b0 * r.N3[0].z;
		acc += h.b1 * r.N3[1].z;
		acc += h.b2 * r.N3[2].z;
		nl.z = acc;
	}
	if (rendered_valid) {
		const float depth = h.depth;
		prast = make3((static_cast<float>(u) - w.pix.cx) * depth / w.pix.fx, (static_cast<float>(v) - w.pix.cy) * depth / w.pix.fy, depth);
	}
	const float4 qr = w.ref_points[p];
	r.ref_valid = qr.w != 0.f;
	const f3 q = make3(qr.x, qr.y, qr.z);
	r.nl = nl;
	r.d = sub3(prast, q);   // point map vector w_l - o_l
	r.dist = dot3(nl, r.d);
}

// The penalty step on a pixel's distance (0 outside the mask): the residual pass 1 stores, whether the pixel contributes
// to the data term, and dr/dw_l, dr/dn_l as the record folds them in.
struct PixelPenalty {
	float residual;
	bool contributes;
	f3 dr_dwl, dr_dnl;
};
__device__ __forceinline__ PixelPenalty pixel_penalty(int use_tukey, float tukey_c, bool mask, const f3& nl, const f3& d, float dist) {
	PixelPenalty o;
	o.residual = dist;
	o.contributes = mask;
	o.dr_dwl = nl;
	o.dr_dnl = d;
	if (use_tukey == PENALTY_IRLS) {
		// iteratively re-weighted least squares with Tukey's biweight (1 - q^2)^2, q = r / c: residual and Jacobian
		// row are both scaled by its square root s, so pass 2 sums s^2 J^T J and (s J)^T (s r); a pixel beyond the
		// cutoff (or with a NaN residual) carries no weight
		const float c = tukey_c;
		o.contributes = mask && fabsf(dist) <= c;
		const float qq = dist / c;
		const float s = 1.f - qq * qq;
		o.residual = o.contributes ? s * dist : 0.f;
		o.dr_dwl = make3(s * nl.x, s * nl.y, s * nl.z);
		o.dr_dnl = make3(s * d.x, s * d.y, s * d.z);
	} else if (use_tukey) {
		const float c = tukey_c;
		const float c6 = (c * c / 6.f);
		const float qq = dist / c;
		const float left = 1.f - (qq * qq);
		o.residual = c6 * (1.f - left * left * left);
		if (dist <= c) o.residual = c6;   // (:384-385 as written: A8)
	}
	if (o.contributes && use_tukey == PENALTY_REFERENCE) {
		const float r = dot3(nl, d);
		if (fabsf(r) > tukey_c) o.contributes = false;
		const float qq = r / tukey_c;
		float psi = 1 - qq * qq;
		psi = r * psi * psi;
		o.dr_dnl = make3(psi * d.x, psi * d.y, psi * d.z);
		o.dr_dwl = make3(psi * nl.x, psi * nl.y, psi * nl.z);
	}
	return o;
}

// The compact Jacobian record [dr/dV (9), dr/dn_l (3), rho (3), r] of a contributing pixel: the rasterized-surface chain
// (RasterizedSurfaceJacobiansImpl.h:114-284) folded with dr/dw_l, dr/dn_l.
// dn: this lane's 27 parked floats at dn[i * dn_stride] (lane-private LDS column)
// RK: the record goes to the lane's registers (rk); otherwise to memory (rec_f, 16 floats)
template <bool RK>
__device__ __forceinline__ void pixel_record(const PixelResolveView& a, const PixelResolve& res, const PixelPenalty& pen, float* dn, int dn_stride,
                                             float* rec_f, float (&rk)[16]) {
	const RasterHit& h = res.h;
	const FaceNdc& fn = res.fn;
	const f3(&V3)[3] = res.V3;
	const f3(&N3)[3] = res.N3;
	const float px = res.px, py = res.py;
	const f3 dr_dwl = pen.dr_dwl, dr_dnl = pen.dr_dnl;
	const float residual = pen.residual;
	float rn[3], rho[3];
	// ---- rasterized surface Jacobians (RasterizedSurfaceJacobiansImpl.h:114-200) ----
	rho[0] = h.b0;
	rho[1] = h.b1;
	rho[2] = h.b2;
	float A, sa[3], drho[3] = {0.f, 0.f, 0.f};
	A = spa_cw(fn.x[0], fn.y[0], fn.x[1], fn.y[1], fn.x[2], fn.y[2]) + K_EPSILON;
	if (a.perspective) {
		sa[0] = spa_cw(px, py, fn.x[1], fn.y[1], fn.x[2], fn.y[2]);
		sa[1] = spa_cw(px, py, fn.x[2], fn.y[2], fn.x[0], fn.y[0]);
		sa[2] = spa_cw(px, py, fn.x[0], fn.y[0], fn.x[1], fn.y[1]);
		const float inv_A = rcp_rn_normal(A);   // consumed by div_rn only, which ignores it outside (1e-30, 1e30)
#pragma unroll
		for (int i = 0; i < 3; i++) drho[i] = div_rn(sa[i], A, inv_A);
	} else {
#pragma unroll
		for (int i = 0; i < 3; i++) sa[i] = rho[i] * A;
	}
	// d rho / d ndc (BarycentricCoordinateJacobians.h:85-181)
	const float den = A * A + K_EPSILON;
	const float dA[3][2] = {{fn.y[1] - fn.y[2], fn.x[2] - fn.x[1]}, {fn.y[2] - fn.y[0], fn.x[0] - fn.x[2]}, {fn.y[0] - fn.y[1], fn.x[1] - fn.x[0]}};
	// sub-area derivatives: (p, va, vb) -> d/dva = (vb.y - p.y, p.x - vb.x), d/dvb = (p.y - va.y, va.x - p.x)
	const float s0a[2] = {fn.y[2] - py, px - fn.x[2]}, s0b[2] = {py - fn.y[1], fn.x[1] - px};   // (p, v1, v2)
	const float s1a[2] = {fn.y[0] - py, px - fn.x[0]}, s1b[2] = {py - fn.y[2], fn.x[2] - px};   // (p, v2, v0)
	const float s2a[2] = {fn.y[1] - py, px - fn.x[1]}, s2b[2] = {py - fn.y[0], fn.x[0] - px};   // (p, v0, v1)
	const float inv_den = rcp_rn_normal(den);   // (div_rn only)
	// d rho_r / d ndc of face vertex i, component c, and (below) the perspective z-terms of vertex i: parked in LDS
	// (lane-private slots) until vertex i's columns are formed, which keeps the kernel at <= 96 VGPRs (5 waves/SIMD:
	// one residency round at 640x480)
#define DN(i, r, c) dn[(((i) * 3 + (r)) * 2 + (c)) * dn_stride]
#define PZ(r, i) dn[(18 + (r) * 3 + (i)) * dn_stride]
#pragma unroll
	for (int c = 0; c < 2; c++) {
		DN(0, 0, c) = div_rn(-sa[0] * dA[0][c], den, inv_den);
		DN(1, 0, c) = div_rn(A * s0a[c] - sa[0] * dA[1][c], den, inv_den);
		DN(2, 0, c) = div_rn(A * s0b[c] - sa[0] * dA[2][c], den, inv_den);
		DN(0, 1, c) = div_rn(A * s1b[c] - sa[1] * dA[0][c], den, inv_den);
		DN(1, 1, c) = div_rn(-sa[1] * dA[1][c], den, inv_den);
		DN(2, 1, c) = div_rn(A * s1a[c] - sa[1] * dA[2][c], den, inv_den);
		DN(0, 2, c) = div_rn(A * s2a[c] - sa[2] * dA[0][c], den, inv_den);
		DN(1, 2, c) = div_rn(A * s2b[c] - sa[2] * dA[1][c], den, inv_den);
		DN(2, 2, c) = div_rn(-sa[2] * dA[2][c], den, inv_den);
	}
	// perspective-correction factors first (RasterizedSurfaceJacobiansImpl.h:217-284), so the 3x9 Jacobian can be
	// streamed one face vertex (3 columns) at a time: same expressions, far fewer live registers
	float Pd[3][3];
	if (a.perspective) {
		const float z0 = V3[0].z, z1 = V3[1].z, z2 = V3[2].z;
		const float v12 = z1 * z2, v02 = z0 * z2, v01 = z0 * z1;
		const float n0 = drho[0] * v12, n1 = drho[1] * v02, n2 = drho[2] * v01;
		const float dd = fmaxf(n0 + n1 + n2, K_EPSILON);
		const float dd2 = dd * dd;
		const float pd[3][3] = {{(dd - n0) * v12, -n0 * v02, -n0 * v01}, {-n1 * v12, (dd - n1) * v02, -n1 * v01},
		                        {-n2 * v12, -n2 * v02, (dd - n2) * v01}};
		const float pz0 = drho[1] * z2 + z1 * drho[2];
		const float pz1 = drho[0] * z2 + z0 * drho[2];
		const float pz2 = drho[0] * z1 + z0 * drho[1];
		const float pz[3][3] = {{-n0 * pz0, dd * drho[0] * z2 - n0 * pz1, dd * drho[0] * z1 - n0 * pz2},
		                        {dd * drho[1] * z2 - n1 * pz0, -n1 * pz1, dd * drho[1] * z0 - n1 * pz2},
		                        {dd * drho[2] * z1 - n2 * pz0, dd * drho[2] * z0 - n2 * pz1, -n2 * pz2}};
		const float inv_dd2 = rcp_rn_normal(dd2);   // (div_rn only)
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 3; c++) {
				Pd[r][c] = div_rn(pd[r][c], dd2, inv_dd2);
				PZ(r, c) = div_rn(pz[r][c], dd2, inv_dd2);
			}
	}
	// record [dr/dV (9), dr/dn_l (3), rho (3), r]; everything but dr/dV first, so it is not held across the columns
	if constexpr (RK) {
		rk[9] = dr_dnl.x;
		rk[10] = dr_dnl.y;
		rk[11] = dr_dnl.z;
		rk[12] = rho[0];
		rk[13] = rho[1];
		rk[14] = rho[2];
		rk[15] = residual;
	} else {
		rec_f[9] = dr_dnl.x;
		rec_f[10] = dr_dnl.y;
		rec_f[11] = dr_dnl.z;
		reinterpret_cast<float4*>(rec_f)[3] = make_float4(rho[0], rho[1], rho[2], residual);
	}
	// dr/dV = dr/dwl * dwl/dV + dr/dnl * dnl/dV ; dr/dN = dr/dnl (rho (x) I)
	const float rw[3] = {dr_dwl.x, dr_dwl.y, dr_dwl.z};
	rn[0] = dr_dnl.x;
	rn[1] = dr_dnl.y;
	rn[2] = dr_dnl.z;
#pragma unroll
	for (int i = 0; i < 3; i++) {
		__builtin_amdgcn_sched_barrier(0);   // one face vertex's columns at a time: bounds the live registers
		const float z = V3[i].z;
		const float z2 = z * z;
		const float P0[3] = {a.ndc.ndc.fx / z, 0.f, -a.ndc.ndc.fx * V3[i].x / z2};
		const float P1[3] = {0.f, a.ndc.ndc.fy / z, -a.ndc.ndc.fy * V3[i].y / z2};
		float Jc[3][3];   // rows of the 3x9 Jacobian, columns 3i .. 3i+2
#pragma unroll
		for (int r = 0; r < 3; r++)
#pragma unroll
			for (int c = 0; c < 3; c++) Jc[r][c] = DN(i, r, 0) * P0[c] + DN(i, r, 1) * P1[c];
		if (a.perspective) {
			float J2[3][3];
#pragma unroll
			for (int r = 0; r < 3; r++)
#pragma unroll
				for (int c = 0; c < 3; c++) J2[r][c] = (Pd[r][0] * Jc[0][c] + Pd[r][1] * Jc[1][c]) + Pd[r][2] * Jc[2][c];
#pragma unroll
			for (int r = 0; r < 3; r++) J2[r][2] += PZ(r, i);
#pragma unroll
			for (int r = 0; r < 3; r++)
#pragma unroll
				for (int c = 0; c < 3; c++) Jc[r][c] = J2[r][c];
		}
#pragma unroll
		for (int c = 0; c < 3; c++) {
			float w_rc[3], n_rc[3];
#pragma unroll
			for (int r = 0; r < 3; r++) {
				const f3 Vk[3] = {V3[0], V3[1], V3[2]};
				const f3 Nk[3] = {N3[0], N3[1], N3[2]};
				const float vr0 = r == 0 ? Vk[0].x : (r == 1 ? Vk[0].y : Vk[0].z);
				const float vr1 = r == 0 ? Vk[1].x : (r == 1 ? Vk[1].y : Vk[1].z);
				const float vr2 = r == 0 ? Vk[2].x : (r == 1 ? Vk[2].y : Vk[2].z);
				const float nr0 = r == 0 ? Nk[0].x : (r == 1 ? Nk[0].y : Nk[0].z);
				const float nr1 = r == 0 ? Nk[1].x : (r == 1 ? Nk[1].y : Nk[1].z);
				const float nr2 = r == 0 ? Nk[2].x : (r == 1 ? Nk[2].y : Nk[2].z);
				w_rc[r] = (vr0 * Jc[0][c] + vr1 * Jc[1][c]) + vr2 * Jc[2][c];
				if (c == r) w_rc[r] += rho[i];
				n_rc[r] = (nr0 * Jc[0][c] + nr1 * Jc[1][c]) + nr2 * Jc[2][c];
			}
			const float x = (rw[0] * w_rc[0] + rw[1] * w_rc[1]) + rw[2] * w_rc[2];
			const float y = (rn[0] * n_rc[0] + rn[1] * n_rc[1]) + rn[2] * n_rc[2];
			if constexpr (RK) rk[3 * i + c] = x + y;
			else rec_f[3 * i + c] = x + y;   // stored as formed: no 9-float tail of live outputs
		}
	}
#undef DN
#undef PZ
}

// The pixel-node Jacobian row of one association (PixelVertexAnchorJacobiansImpl.h:179-363): jr (rotation) and jt
// (translation) of the node for a pixel whose record is q, from what the caller loaded -- per face vertex the
// Jacobian-row slot rows[fv] (-1: the vertex is not anchored to the node) and its weight in jv[fv].w, then
//   NNRT_GATHER_ROWS builds: the warp's rows (-w R (v - g), -w R n) in jv / jn;
//   otherwise: the node's state ns4 (g, t, R; only ns4[0] is read when state_identity) and the vertices' canonical
//   positions / normals cp4 / cn4 (the default build forms the warp's rows from them in jv / jn).
template <int MODE>
__device__ __forceinline__ void pixel_node_row(const int (&rows)[3], float4 (&jv)[3], float4 (&jn)[3], const float4 (&ns4)[4], const float4 (&cp4)[3],
                                               const float4 (&cn4)[3], const float (&q)[16], bool state_identity, float (&jr)[3], float (&jt)[3]) {
	const float dr_dV[9] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
	const float rn[3] = {q[9], q[10], q[11]};
	const float rho[3] = {q[12], q[13], q[14]};
#pragma unroll
	for (int c = 0; c < 3; c++) jr[c] = jt[c] = 0.f;
#if NNRT_JAC_FMA && !NNRT_GATHER_ROWS
	// Fused form (round 5): per face vertex, with ws = w if the vertex is anchored to the node, else 0,
	//   jt += ws dv,   jr += -ws (dv x R (v - g) + dn x R n)
	// i.e. the reference's dv [-w R (v - g)]_x + dn [-w R n]_x (PixelVertexAnchorJacobiansImpl.h:179-363,
	// WarpedSurfaceJacobiansImpl.h:117-156) with -w factored out of the cross products and every product-sum an
	// FMA (the build is -ffp-contract=off), as nvcc's default contraction of the reference's CUDA path also
	// does: 43 VALU per face vertex instead of 78, the terms within a few float ulps of the unfused rows (the
	// unfused, oracle-bit-identical form: -DNNRT_JAC_FMA=0). A vertex not anchored to the node adds ws = 0
	// products, i.e. +-0, which leave the +0-started sums unchanged bit for bit (finite inputs: the vertex's own
	// canonical position / normal, the pixel's record and the node's state, never the padding row's data).
	{
		float R[9];
		f3 g = make3(0.f, 0.f, 0.f);
		if (MODE != NNRT_ITERATION_TRANSLATION_ONLY) {
			g = make3(ns4[0].x, ns4[0].y, ns4[0].z);
			if (state_identity) {
#pragma unroll
				for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
			} else {
				const float Rl[9] = {ns4[1].z, ns4[1].w, ns4[2].x, ns4[2].y, ns4[2].z, ns4[2].w, ns4[3].x, ns4[3].y, ns4[3].z};
#pragma unroll
				for (int i = 0; i < 9; i++) R[i] = Rl[i];
			}
		}
#pragma unroll
		for (int fv = 0; fv < 3; fv++) {
			const float ws = rows[fv] >= 0 ? jv[fv].w : 0.f;
			const f3 dv = make3(dr_dV[3 * fv], dr_dV[3 * fv + 1], dr_dV[3 * fv + 2]);
			if (MODE != NNRT_ITERATION_ROTATION_ONLY) {
				jt[0] = fmaf(dv.x, ws, jt[0]);
				jt[1] = fmaf(dv.y, ws, jt[1]);
				jt[2] = fmaf(dv.z, ws, jt[2]);
			}
			if (MODE != NNRT_ITERATION_TRANSLATION_ONLY) {
				const f3 d3 = sub3(make3(cp4[fv].x, cp4[fv].y, cp4[fv].z), g);
				const f3 n3 = make3(cn4[fv].x, cn4[fv].y, cn4[fv].z);
				const f3 p = make3(fmaf(R[0], d3.x, fmaf(R[1], d3.y, R[2] * d3.z)), fmaf(R[3], d3.x, fmaf(R[4], d3.y, R[5] * d3.z)),
				                   fmaf(R[6], d3.x, fmaf(R[7], d3.y, R[8] * d3.z)));
				const f3 q = make3(fmaf(R[0], n3.x, fmaf(R[1], n3.y, R[2] * n3.z)), fmaf(R[3], n3.x, fmaf(R[4], n3.y, R[5] * n3.z)),
				                   fmaf(R[6], n3.x, fmaf(R[7], n3.y, R[8] * n3.z)));
				const f3 dn = make3(rn[0] * rho[fv], rn[1] * rho[fv], rn[2] * rho[fv]);
				// dv x p + dn x q
				const float cx = fmaf(dv.y, p.z, fmaf(-dv.z, p.y, fmaf(dn.y, q.z, -dn.z * q.y)));
				const float cy = fmaf(dv.z, p.x, fmaf(-dv.x, p.z, fmaf(dn.z, q.x, -dn.x * q.z)));
				const float cz = fmaf(dv.x, p.y, fmaf(-dv.y, p.x, fmaf(dn.x, q.y, -dn.y * q.x)));
				jr[0] = fmaf(-ws, cx, jr[0]);
				jr[1] = fmaf(-ws, cy, jr[1]);
				jr[2] = fmaf(-ws, cz, jr[2]);
			}
		}
	}
#else
#if !NNRT_GATHER_ROWS
	if (MODE != NNRT_ITERATION_TRANSLATION_ONLY) {
		// (-w R (v - g), -w R n) per face vertex: warp_slot's expressions (kernels.hpp), bit-identical to its rows
		const f3 g = make3(ns4[0].x, ns4[0].y, ns4[0].z);
		float R[9];
		if (state_identity) {
#pragma unroll
			for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
		} else {
			const float Rl[9] = {ns4[1].z, ns4[1].w, ns4[2].x, ns4[2].y, ns4[2].z, ns4[2].w, ns4[3].x, ns4[3].y, ns4[3].z};
#pragma unroll
			for (int i = 0; i < 9; i++) R[i] = Rl[i];
		}
#pragma unroll
		for (int fv = 0; fv < 3; fv++) {
			const float w = jv[fv].w;
			const f3 Rj = matvec3(R, sub3(make3(cp4[fv].x, cp4[fv].y, cp4[fv].z), g));
			const f3 Rnj = matvec3(R, make3(cn4[fv].x, cn4[fv].y, cn4[fv].z));
			jv[fv] = make_float4(-w * Rj.x, -w * Rj.y, -w * Rj.z, w);
			jn[fv] = make_float4(-w * Rnj.x, -w * Rnj.y, -w * Rnj.z, 0.f);
		}
	}
#endif
	// branch-free over the face vertices: a vertex not anchored to the node adds an exact +0 (selected, so the
	// row it loaded in its place -- row 0 -- never reaches the sums, NaN or not)
#pragma unroll
	for (int fv = 0; fv < 3; fv++) {
		const bool on = rows[fv] >= 0;
		const f3 dv = make3(dr_dV[3 * fv], dr_dV[3 * fv + 1], dr_dV[3 * fv + 2]);
		if (MODE != NNRT_ITERATION_ROTATION_ONLY) {
			jt[0] += on ? dv.x * jv[fv].w : 0.f;
			jt[1] += on ? dv.y * jv[fv].w : 0.f;
			jt[2] += on ? dv.z * jv[fv].w : 0.f;
		}
		if (MODE != NNRT_ITERATION_TRANSLATION_ONLY) {
			const f3 dn = make3(rn[0] * rho[fv], rn[1] * rho[fv], rn[2] * rho[fv]);
			const f3 t1 = row_times_skew(dv, make3(jv[fv].x, jv[fv].y, jv[fv].z));
			const f3 t2 = row_times_skew(dn, make3(jn[fv].x, jn[fv].y, jn[fv].z));
			jr[0] += on ? t1.x + t2.x : 0.f;
			jr[1] += on ? t1.y + t2.y : 0.f;
			jr[2] += on ? t1.z + t2.z : 0.f;
		}
	}
#endif
}

} // namespace nnrt
