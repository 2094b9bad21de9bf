// mpm_collision_shapes.hpp — collision objects given in closed form: half-space, sphere, box, capsule.
//
// An extension (the reference knows level sets only).  A shape lives in the coordinates a level set's samples would be given in: a node is
// taken to its material point by collision_material_point (mpm_collision.hpp), the shape answers with a signed distance and a unit normal,
// and from `sdis <= 0` on the node runs through collision_respond, the level set's own response.  No memory, no loads: a shape is nine
// words of kernel arguments.  query_sdf's domain box does not apply - a shape exists everywhere.
// Builds on x86 like mpm_collision.hpp (tools/hostcheck/check_shapes.cpp): MPM_DEV only, contraction off, plain IEEE `/` and sqrtf.
// tests/collision_shape_model.py restates every function below statement for statement with numpy float32.
#pragma once
#include "mpm_collision.hpp"

namespace mpm {

enum { kShapeHalfspace = 1, kShapeSphere = 2, kShapeBox = 3, kShapeCapsule = 4 };// MPM_SHAPE_*
constexpr int kMaxShapes = 4;													  // MPM_MAX_COLLISION_SHAPES

struct CollisionShape {// mpm_collision_shape as installed (a half-space's normal has unit length here)
	int kind;
	int inside_out;
	float a[3], b[3];
	float radius;
};

// Half-space through a with unit outward normal b.  Statement order:
//   d_i = x_i - a_i;  sdis = (d_0 b_0 + d_1 b_1) + d_2 b_2;  n = b.
MPM_DEV void shape_halfspace(const CollisionShape& s, const float (&x)[3], float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	const float d0 = x[0] - s.a[0], d1 = x[1] - s.a[1], d2 = x[2] - s.a[2];
	sdis = d0 * s.b[0] + d1 * s.b[1] + d2 * s.b[2];
	n[0] = s.b[0];
	n[1] = s.b[1];
	n[2] = s.b[2];
}

// The common tail of sphere and capsule: d = x - (nearest point of the core).  Statement order:
//   len = sqrtf((d_0 d_0 + d_1 d_1) + d_2 d_2);  sdis = len - r;  n_i = len > 0 ? d_i / len : +0   (NaN len: n = 0, sdis NaN touches nothing).
MPM_DEV void shape_round(const float (&d)[3], float r, float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
	sdis = len - r;
	const bool pos = len > 0.f;
#pragma unroll
	for(int i = 0; i < 3; ++i) n[i] = pos ? d[i] / len : 0.f;
}

// Sphere of radius r about a.  Statement order: d_i = x_i - a_i; shape_round(d, r).
MPM_DEV void shape_sphere(const CollisionShape& s, const float (&x)[3], float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	const float d[3] = {x[0] - s.a[0], x[1] - s.a[1], x[2] - s.a[2]};
	shape_round(d, s.radius, sdis, n);
}

// Box about a with half extents b.  Statement order:
//   p_i = x_i - a_i;  q_i = |p_i| - b_i;  sg_i = p_i < 0 ? -1 : +1   (sign(+-0) = +)
//   inside (q_0 <= 0 and q_1 <= 0 and q_2 <= 0; a NaN is outside):
//     axis = 0; if(q_1 > q_axis) axis = 1; if(q_2 > q_axis) axis = 2   (ties: the lowest axis);  sdis = q_axis;  n = sg_axis e_axis
//   outside: o_i = q_i < 0 ? +0 : q_i  (a NaN stays);  len = sqrtf((o_0 o_0 + o_1 o_1) + o_2 o_2);  sdis = len;
//     n_i = len > 0 ? sg_i (o_i / len) : +0   (squares that underflow give len = 0: touched, with n = 0).
MPM_DEV void shape_box(const CollisionShape& s, const float (&x)[3], float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	float q[3], sg[3];
#pragma unroll
	for(int i = 0; i < 3; ++i) {
		const float p = x[i] - s.a[i];
		q[i]		  = fabsf(p) - s.b[i];
		sg[i]		  = p < 0.f ? -1.f : 1.f;
	}
	if(q[0] <= 0.f && q[1] <= 0.f && q[2] <= 0.f) {
		const bool one = q[1] > q[0];
		const float m1 = one ? q[1] : q[0];
		const bool two = q[2] > m1;
		sdis		   = two ? q[2] : m1;
		n[0]		   = (!one && !two) ? sg[0] : 0.f;
		n[1]		   = (one && !two) ? sg[1] : 0.f;
		n[2]		   = two ? sg[2] : 0.f;
	} else {
		float o[3];
#pragma unroll
		for(int i = 0; i < 3; ++i) o[i] = q[i] < 0.f ? 0.f : q[i];
		const float len = sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
		sdis			= len;
		const bool pos	= len > 0.f;
#pragma unroll
		for(int i = 0; i < 3; ++i) n[i] = pos ? sg[i] * (o[i] / len) : 0.f;
	}
}

// Capsule of radius r about the segment a b (a != b).  Statement order:
//   e_i = b_i - a_i;  p_i = x_i - a_i;  t = ((p_0 e_0 + p_1 e_1) + p_2 e_2) / ((e_0 e_0 + e_1 e_1) + e_2 e_2)
//   if(t < 0) t = 0;  if(t > 1) t = 1   (a NaN stays);  d_i = p_i - t e_i;  shape_round(d, r).
MPM_DEV void shape_capsule(const CollisionShape& s, const float (&x)[3], float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	float e[3], p[3], d[3];
#pragma unroll
	for(int i = 0; i < 3; ++i) {
		e[i] = s.b[i] - s.a[i];
		p[i] = x[i] - s.a[i];
	}
	float t = (p[0] * e[0] + p[1] * e[1] + p[2] * e[2]) / (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
	if(t < 0.f) t = 0.f;
	if(t > 1.f) t = 1.f;
#pragma unroll
	for(int i = 0; i < 3; ++i) d[i] = p[i] - t * e[i];
	shape_round(d, s.radius, sdis, n);
}

// Signed distance and unit normal of a shape at the material point x.  The kind is the same for every node of a launch (wave-uniform: a
// scalar branch).  inside_out: the solid is the complement - sdis = -sdis, n_i = -n_i.  An unknown kind touches nothing (sdis = +1, n = 0).
MPM_DEV void shape_query(const CollisionShape& s, const float (&x)[3], float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	if(s.kind == kShapeHalfspace)
		shape_halfspace(s, x, sdis, n);
	else if(s.kind == kShapeSphere)
		shape_sphere(s, x, sdis, n);
	else if(s.kind == kShapeBox)
		shape_box(s, x, sdis, n);
	else if(s.kind == kShapeCapsule)
		shape_capsule(s, x, sdis, n);
	else {
		sdis = 1.f;
		n[0] = n[1] = n[2] = 0.f;
	}
	if(s.inside_out) {
		sdis = -sdis;
#pragma unroll
		for(int i = 0; i < 3; ++i) n[i] = -n[i];
	}
}

// One collider acting on one domain point X (a node: (float) node * dx): material point, query, and - where sdis <= 0; a NaN touches
// nothing - the level set's response.
MPM_DEV void shape_resolve(const CollisionObject& o, const CollisionPose& p, const CollisionShape& s, const float (&X)[3], float (&vel)[3]) {
#pragma clang fp contract(off)
	float xmt[3], x[3], n[3], sdis;
	collision_material_point(o, p, X, xmt, x);
	shape_query(s, x, sdis, n);
	if(!(sdis <= 0.f)) return;
	collision_respond(o, p, xmt, x, n, vel);
}

}// namespace mpm
