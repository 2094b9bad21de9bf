// mpm_collision.hpp — level-set collision object of the MGSP grid update.
//
// Device side of Projects/MGSP/boundary_condition.cuh:25-250 (SignedDistanceGrid::detect_and_resolve_collision and
// helpers).  The signed distance and its gradient live in one float4 {sdis, gx, gy, gz} per grid node of the whole
// domain (N^3 nodes, node (i,j,k) at (i N + j) N + k): one 16-byte load per corner of the trilinear stencil instead of
// four scalar loads from four SoA channels of a 4x4x4-blocked field.  The arithmetic keeps the reference's quirks
// (the "cross product" with plus signs, MatrixUtils.h:53-58; the early return of SEPARATE with a zero normal).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#ifndef MPM_DEV// (mpm_device_math.hpp's; this header needs nothing else of it, so that tools/hostcheck can build it alone on x86)
#define MPM_DEV __device__ __forceinline__
#endif

namespace mpm {

struct CollisionObject {// mpm_collision_object + the field
	int type;
	float friction, scale, dsdt;
	float trans[3], trans_vel[3], omega[3];
	float rot[9];// element (i, j) at [3 i + j] (the reference's vec3x3), handed to the column-major helpers as raw arrays
	float time;// the object's clock: the time of the next grid update (mpm_set_collision_clock)
	const float4* field;
};

// No contraction in the per-node code (the pragma at the top of each function): left to the compiler, the stand-alone kernel and the fused
// carry-over came out with different fused multiply-adds and differed in the last bit of a velocity (1.2e-7 relative in position after 60
// substeps of a deterministic scene).  Plain IEEE operations are the same in every kernel that inlines this - and the oracle's arithmetic.
MPM_DEV void col_cross(float (&out)[3], const float (&a)[3], const float (&b)[3]) {// (sic) plus signs
#pragma clang fp contract(off)
	out[0] = a[1] * b[2] + a[2] * b[1];
	out[1] = a[2] * b[0] + a[0] * b[2];
	out[2] = a[0] * b[1] + a[1] * b[0];
}

// The object's pose at one time: everything detect_and_resolve_collision (:164-187) derives from `current_time` alone.  The same for
// every node of a grid update, so the host computes it once per launch (collision_pose) and hands it to the kernel by value: no
// sinf / cosf and no 3x3 products per node.  At t = 0 it is {rot = the start orientation, inv = 1, shift = trans} exactly.
struct CollisionPose {
	float rot[9];  // start orientation x the three axis rotations by omega t
	float inv;	   // 1 / (1 + dsdt t)
	float shift[3];// trans + trans_vel t
	float growth;  // dsdt / scale (time-independent; one IEEE division here instead of one per node)
};
// Host side (plain C++: no contraction, libm's cosf / sinf), statement order of rot_angle_to_matrix (:68-91) and of
// matrix_matrix_multiplication_3d (MatrixUtils.h:147-157) on the raw arrays, as col_rot_angle_to_matrix / matmul3 have it.
inline CollisionPose collision_pose(const CollisionObject& o, float t) {
#pragma clang fp contract(off)
	CollisionPose p;
	for(int d = 0; d < 3; ++d) p.shift[d] = o.trans[d] + o.trans_vel[d] * t;
	for(int i = 0; i < 9; ++i) p.rot[i] = o.rot[i];
	p.inv	 = 1.f / (1.f + o.dsdt * t);
	p.growth = o.dsdt / o.scale;
	if(t != 0.f) {// at t = 0 the three factors are identities (the only case the reference exercises)
		for(int dim = 0; dim < 3; ++dim) {
			float tmp[9], prev[9];
			for(int i = 0; i < 9; ++i) tmp[i] = 0.f;
			const float c = cosf(o.omega[dim] * t), s = sinf(o.omega[dim] * t);
			if(dim == 0) {
				tmp[0] = 1.f;
				tmp[4] = tmp[8] = c;
				tmp[7]			= s;
				tmp[5]			= -s;
			} else if(dim == 1) {
				tmp[4] = 1.f;
				tmp[0] = tmp[8] = c;
				tmp[2]			= s;
				tmp[6]			= -s;
			} else {
				tmp[8] = 1.f;
				tmp[0] = tmp[4] = c;
				tmp[3]			= s;
				tmp[1]			= -s;
			}
			for(int i = 0; i < 9; ++i) prev[i] = p.rot[i];
			for(int j = 0; j < 3; ++j)
				for(int i = 0; i < 3; ++i) p.rot[3 * j + i] = prev[i] * tmp[3 * j] + prev[3 + i] * tmp[3 * j + 1] + prev[6 + i] * tmp[3 * j + 2];
		}
	}
	return p;
}

// The material-point part of detect_and_resolve_collision (:164-187): a domain point X (a node: (float) node * dx) -> xmt = X - shift and its
// position x in the coordinates the level set's samples (or an analytic shape, mpm_collision_shapes.hpp) are given in.
MPM_DEV void collision_material_point(const CollisionObject& o, const CollisionPose& p, const float (&X)[3], float (&xmt)[3], float (&x)[3]) {
#pragma clang fp contract(off)
	float x0[3];
#pragma unroll
	for(int d = 0; d < 3; ++d) xmt[d] = X[d] - p.shift[d];
	const float (&rot)[9] = p.rot;
#pragma unroll
	for(int d = 0; d < 3; ++d) x0[d] = xmt[d] * p.inv;
	x[0] = rot[0] * x0[0] + rot[1] * x0[1] + rot[2] * x0[2];// mat_t_mul_vec_3d
	x[1] = rot[3] * x0[0] + rot[4] * x0[1] + rot[5] * x0[2];
	x[2] = rot[6] * x0[0] + rot[7] * x0[1] + rot[8] * x0[2];
#pragma unroll
	for(int d = 0; d < 3; ++d) x[d] = x[d] * o.scale + o.trans[d];
}

MPM_DEV void collision_respond(const CollisionObject& o, const CollisionPose& p, const float (&xmt)[3], const float (&x)[3], const float (&n)[3], float (&vel)[3]);

// detect_and_resolve_collision (:164-248) behind the pose; node = integer node coordinates; bc_lo / bc_hi = query_sdf's domain box (:141-146)
MPM_DEV void collision_resolve(const CollisionObject& o, const CollisionPose& p, const int (&node)[3], float dx, int N, float bc_lo, float bc_hi, float (&vel)[3]) {
#pragma clang fp contract(off)
	float X[3], xmt[3], x[3];
#pragma unroll
	for(int d = 0; d < 3; ++d) X[d] = (float) node[d] * dx;
	collision_material_point(o, p, X, xmt, x);
	// query_sdf
	if(x[0] < bc_lo || x[0] >= bc_hi || x[1] < bc_lo || x[1] >= bc_hi || x[2] < bc_lo || x[2] >= bc_hi) return;
	int cid[3];
	float w1[3][2];
#pragma unroll
	for(int d = 0; d < 3; ++d) {
		cid[d]			   = (int) (x[d] / dx);
		const float dis_lb = x[d] - ((float) cid[d] * dx);
		w1[d][0]		   = 1.f - dis_lb / dx;
		w1[d][1]		   = dis_lb / dx;
	}
	float sdis = 0.f, n[3] = {0.f, 0.f, 0.f};
#pragma unroll
	for(int i = 0; i < 2; ++i)
#pragma unroll
		for(int j = 0; j < 2; ++j)
#pragma unroll
			for(int k = 0; k < 2; ++k) {
				const float w  = w1[0][i] * w1[1][j] * w1[2][k];
				const float4 v = o.field[((size_t) (cid[0] + i) * N + (size_t) (cid[1] + j)) * N + (size_t) (cid[2] + k)];
				sdis += w * v.x;
				n[0] += w * v.y;
				n[1] += w * v.z;
				n[2] += w * v.w;
			}
	const float nn = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
	for(int d = 0; d < 3; ++d) n[d] /= nn;
	if(!(sdis <= 0.f)) return;
	collision_respond(o, p, xmt, x, n, vel);
}

// The response part (:197-248) for a touched node (sdis <= 0) with unit normal n in material coordinates: the level set's and every
// analytic shape's.
MPM_DEV void collision_respond(const CollisionObject& o, const CollisionPose& p, const float (&xmt)[3], const float (&x)[3], const float (&n)[3], float (&vel)[3]) {
#pragma clang fp contract(off)
	const float (&rot)[9] = p.rot;
	// object velocity in deformation space (:197-204)
	float v_obj[3], radius[3], mat_vel[3];
	col_cross(v_obj, o.omega, xmt);
#pragma unroll
	for(int d = 0; d < 3; ++d) {
		v_obj[d] += xmt[d] * p.growth;
		radius[d] = x[d] - o.trans[d];
	}
	col_cross(mat_vel, o.omega, radius);
#pragma unroll
	for(int d = 0; d < 3; ++d) mat_vel[d] += o.trans_vel[d];
	const float rv0 = rot[0] * mat_vel[0] + rot[3] * mat_vel[1] + rot[6] * mat_vel[2];
	const float rv1 = rot[1] * mat_vel[0] + rot[4] * mat_vel[1] + rot[7] * mat_vel[2];
	const float rv2 = rot[2] * mat_vel[0] + rot[5] * mat_vel[1] + rot[8] * mat_vel[2];
	v_obj[0] += rv0 * o.scale + o.trans_vel[0];
	v_obj[1] += rv1 * o.scale + o.trans_vel[1];
	v_obj[2] += rv2 * o.scale + o.trans_vel[2];
#pragma unroll
	for(int d = 0; d < 3; ++d) vel[d] -= v_obj[d];
	if(o.type == 0) {// STICKY
		vel[0] = vel[1] = vel[2] = 0.f;
	} else {
		if(o.type == 2 && n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) {
			vel[0] = vel[1] = vel[2] = 0.f;
			return;// (:227-230) without adding the object velocity back
		}
		float nr[3];
		nr[0] = rot[0] * n[0] + rot[3] * n[1] + rot[6] * n[2];
		nr[1] = rot[1] * n[0] + rot[4] * n[1] + rot[7] * n[2];
		nr[2] = rot[2] * n[0] + rot[5] * n[1] + rot[8] * n[2];
		const float v_dot_n = nr[0] * vel[0] + nr[1] * vel[1] + nr[2] * vel[2];
		const bool project	= o.type == 1 || v_dot_n < 0.f;// SLIP always removes the normal part, SEPARATE only when approaching
		if(project) {
#pragma unroll
			for(int d = 0; d < 3; ++d) vel[d] -= nr[d] * v_dot_n;
			const bool fric = o.type == 1 ? (o.friction > 0.0f && v_dot_n < 0.f) : (o.friction != 0.f);
			if(fric) {
				const float vel_norm = sqrtf(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]);
				if(-v_dot_n * o.friction < vel_norm) {
#pragma unroll
					for(int d = 0; d < 3; ++d) vel[d] += vel[d] / vel_norm * (v_dot_n * o.friction);
				} else {
					vel[0] = vel[1] = vel[2] = 0.f;
				}
			}
		}
	}
#pragma unroll
	for(int d = 0; d < 3; ++d) vel[d] += v_obj[d];
}

}// namespace mpm
