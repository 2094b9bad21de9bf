// mpm_rigid_body.hpp — rigid bodies: slot colliders that the material pushes back (an extension).
//
// A body is a slot collider - sphere, box, capsule or volume - whose pose and velocity are STATE ON THE DEVICE instead of functions of the
// collision clock.  Per applied grid update the material's nodes take the collider's response as if it were prescribed at (x, q, v, omega), and
// the body afterwards takes the equal and opposite impulse: J and L of its load row (mpm_collider_loads.hpp: float64 sums of the exact per-node
// products (double) m * (double) dv, in a fixed order).  What grid and body exchange is therefore conserved to the last bit per update.  The
// scheme is explicit: stable while the mass of the touched nodes stays below the body's (max_mass_ratio keeps the largest ratio seen).  Bodies do
// not collide with each other, with prescribed colliders or with the domain walls.
// Three parts:
//   1. the definition - BodyState / BodyConst / BodyPose, body_step, body_pose - plain C++ on doubles, `__host__ __device__`, contraction off,
//      only + - x / and sqrt (no trigonometry): it builds on x86 too (tools/hostcheck/check_body.cpp) and tests/rigid_body_model.py restates it in
//      NumPy with the same bits;
//   2. the host side (plain C++): the start state from a collider's pose, the checks of an install, the mass properties of the analytic shapes
//      (closed forms) and of a closed triangle mesh (float64 polyhedral integrals);
//   3. the kernels (HIP only): BodyArgs with its slot_resolve and row_pivot - what a body adds to the one cell walk and the one load frame of
//      mpm_collider_loads.hpp -, grid_update_body_kernel (ONE pass over the grid, loads_frame with the stores: the update and its loads together)
//      and body_step_kernel (load_totals, the readout's reduction, then one lane per body runs body_step).
//
// THE STEP, h = (double) dt, J and L the slot's row sums (impulse and angular impulse ON THE COLLIDER, L about x):
//   1. v <- v + (J + h force) (1 / mass), and + (double) gravity * h on y if the gravity flag is set; locked components become 0; x <- x + h v
//   2. l <- l + L + h torque;  omega = R(q) Ib^-1 R(q)^T l;  locked components of omega become 0, and if any is locked l <- R Ib R^T omega
//   3. q <- (q + h/2 (0, omega) (x) q) / |...|
// Step 3 turns q about omega's exact axis and leaves |q| = 1 to rounding; the ANGLE it turns by is atan(h |omega| / 2) * 2, short of h |omega| by
// (h |omega|)^3 / 12 per step.  With no torque and no lock l is never rounded - it is conserved on bits - and the gyroscopic motion comes from
// omega = Iw(q)^-1 l.  A body ignores the collision clock: it advances with every applied grid update.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MPM_BODY_HD __host__ __device__ inline
#else
#define MPM_BODY_HD inline
#endif
// No contraction anywhere in the definition, spelled for the compiler at hand as mpm_collision_volume.hpp does.
#if defined(__clang__)
#define MPM_BODY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MPM_BODY_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

namespace mpm {

enum { kBodyLockX = 1, kBodyLockY = 2, kBodyLockZ = 4, kBodyLockRX = 8, kBodyLockRY = 16, kBodyLockRZ = 32 };

struct BodyState {// mpm_rigid_body_state, word for word
	double x[3];   // centre of mass (world)
	double q[4];   // unit quaternion body -> world, {w, x, y, z}
	double v[3];
	double omega[3];// derived: R Ib^-1 R^T l
	double l[3];	// angular momentum about x (world)
	double J[3], L[3];// the last update's impulse and angular impulse on the body
	double touched_mass, max_mass_ratio;
	long long touched_nodes, updates;
};
struct BodyConst {
	double mass, inv_mass;
	double Ib[9], Ib_inv[9];// body frame, about the centre of mass, row-major (symmetric)
	double com[3];			// material coordinates
	double force[3], torque[3];// constant, world
	int gravity, lock;
};
struct BodyPose {// what the grid update reads, float32, written by body_step_kernel (and the host at an install)
	float rot[9];// R^T in CollisionPose::rot's layout: material x_i = rot[3 i + j] (X - shift)_j, world normal nr_i = rot[3 j + i] n_j
	float shift[3], vel[3], omega[3];
};
constexpr int kMaxBodies = 4;// one per slot
struct BodyBlock {// the context's one small device buffer
	BodyState st[kMaxBodies];
	BodyConst c[kMaxBodies];
	BodyPose pose[kMaxBodies];
};

// R(q), row-major: R[3 i + j].  Statement order: the nine products xx .. wz of two components each, then per entry one or two additions and
// one doubling: R00 = 1 - 2 (yy + zz), R01 = 2 (xy - wz), R02 = 2 (xz + wy), R10 = 2 (xy + wz), R11 = 1 - 2 (xx + zz), R12 = 2 (yz - wx),
// R20 = 2 (xz - wy), R21 = 2 (yz + wx), R22 = 1 - 2 (xx + yy).
MPM_BODY_HD void body_rotation(const double (&q)[4], double (&R)[9]) {
	MPM_BODY_NO_CONTRACT
	const double w = q[0], x = q[1], y = q[2], z = q[3];
	const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
	R[0] = 1.0 - 2.0 * (yy + zz);
	R[1] = 2.0 * (xy - wz);
	R[2] = 2.0 * (xz + wy);
	R[3] = 2.0 * (xy + wz);
	R[4] = 1.0 - 2.0 * (xx + zz);
	R[5] = 2.0 * (yz - wx);
	R[6] = 2.0 * (xz - wy);
	R[7] = 2.0 * (yz + wx);
	R[8] = 1.0 - 2.0 * (xx + yy);
}
// out = R M R^T a for a body-frame matrix M: t = R^T a, u = M t, out = R u, every dot product (p0 + p1) + p2.
MPM_BODY_HD void body_world_apply(const double (&R)[9], const double (&M)[9], const double (&a)[3], double (&out)[3]) {
	MPM_BODY_NO_CONTRACT
	double t[3], u[3];
	for(int i = 0; i < 3; ++i) t[i] = (R[i] * a[0] + R[3 + i] * a[1]) + R[6 + i] * a[2];
	for(int i = 0; i < 3; ++i) u[i] = (M[3 * i] * t[0] + M[3 * i + 1] * t[1]) + M[3 * i + 2] * t[2];
	for(int i = 0; i < 3; ++i) out[i] = (R[3 * i] * u[0] + R[3 * i + 1] * u[1]) + R[3 * i + 2] * u[2];
}
MPM_BODY_HD bool body_finite(double a) {
	MPM_BODY_NO_CONTRACT
	return (a - a) == 0.0;
}
// omega (and, with a rotation lock, l) from l and q: step 2 behind the addition.
MPM_BODY_HD void body_omega(BodyState& s, const BodyConst& c) {
	MPM_BODY_NO_CONTRACT
	double R[9];
	body_rotation(s.q, R);
	body_world_apply(R, c.Ib_inv, s.l, s.omega);
	if(c.lock & (kBodyLockRX | kBodyLockRY | kBodyLockRZ)) {
		for(int d = 0; d < 3; ++d)
			if(c.lock & (kBodyLockRX << d)) s.omega[d] = 0.0;
		const double w[3] = {s.omega[0], s.omega[1], s.omega[2]};
		body_world_apply(R, c.Ib, w, s.l);
	}
}
// One update (the header's three steps).  n_touched, m_touched: the row's touched nodes and their mass.  Returns false where J, L or the new
// state is not finite (the state is written all the same).
MPM_BODY_HD bool body_step(BodyState& s, const BodyConst& c, const double (&J)[3], const double (&L)[3], double n_touched, double m_touched, double h, double gravity) {
	MPM_BODY_NO_CONTRACT
	for(int d = 0; d < 3; ++d) {
		s.v[d] = s.v[d] + (J[d] + h * c.force[d]) * c.inv_mass;
		if(d == 1 && c.gravity) s.v[d] = s.v[d] + gravity * h;
		if(c.lock & (kBodyLockX << d)) s.v[d] = 0.0;
		s.x[d] = s.x[d] + h * s.v[d];
	}
	for(int d = 0; d < 3; ++d) s.l[d] = (s.l[d] + L[d]) + h * c.torque[d];
	body_omega(s, c);
	const double w = s.q[0], x = s.q[1], y = s.q[2], z = s.q[3], ox = s.omega[0], oy = s.omega[1], oz = s.omega[2], hh = 0.5 * h;
	const double dw = 0.0 - ((ox * x + oy * y) + oz * z);// (0, omega) (x) q
	const double dx = (ox * w + oy * z) - oz * y;
	const double dy = (oy * w + oz * x) - ox * z;
	const double dz = (oz * w + ox * y) - oy * x;
	const double nw = w + hh * dw, nx = x + hh * dx, ny = y + hh * dy, nz = z + hh * dz;
	const double len = sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz);
	s.q[0] = nw / len, s.q[1] = nx / len, s.q[2] = ny / len, s.q[3] = nz / len;
	for(int d = 0; d < 3; ++d) s.J[d] = J[d], s.L[d] = L[d];
	s.touched_mass	= m_touched;
	s.touched_nodes = (long long) n_touched;
	s.updates		= s.updates + 1;
	const double ratio = m_touched * c.inv_mass;
	if(ratio > s.max_mass_ratio) s.max_mass_ratio = ratio;
	bool ok = true;
	for(int d = 0; d < 3; ++d) ok = ok && body_finite(J[d]) && body_finite(L[d]) && body_finite(s.x[d]) && body_finite(s.v[d]) && body_finite(s.l[d]) && body_finite(s.omega[d]);
	for(int d = 0; d < 4; ++d) ok = ok && body_finite(s.q[d]);
	return ok;
}
// The float32 pose of a state: rot = (float) R^T, i.e. rot[3 i + j] = (float) R[3 j + i].
MPM_BODY_HD void body_pose(const BodyState& s, BodyPose& p) {
	MPM_BODY_NO_CONTRACT
	double R[9];
	body_rotation(s.q, R);
	for(int i = 0; i < 3; ++i)
		for(int j = 0; j < 3; ++j) p.rot[3 * i + j] = (float) R[3 * j + i];
	for(int d = 0; d < 3; ++d) p.shift[d] = (float) s.x[d], p.vel[d] = (float) s.v[d], p.omega[d] = (float) s.omega[d];
}

// ---- 2. the host side ---------------------------------------------------------------------------------------------------------------------
// The unit quaternion of a rotation matrix R (row-major, R[3 i + j]): the branch with the largest of {trace, R00, R11, R22} (Shepperd), then
// normalised.  The identity gives {1, 0, 0, 0} exactly.
inline void body_quaternion(const double (&R)[9], double (&q)[4]) {
	const double tr = R[0] + R[4] + R[8];
	if(tr >= R[0] && tr >= R[4] && tr >= R[8]) {
		q[0] = 1.0 + tr, q[1] = R[7] - R[5], q[2] = R[2] - R[6], q[3] = R[3] - R[1];
	} else if(R[0] >= R[4] && R[0] >= R[8]) {
		q[0] = R[7] - R[5], q[1] = 1.0 + R[0] - R[4] - R[8], q[2] = R[1] + R[3], q[3] = R[2] + R[6];
	} else if(R[4] >= R[8]) {
		q[0] = R[2] - R[6], q[1] = R[1] + R[3], q[2] = 1.0 - R[0] + R[4] - R[8], q[3] = R[5] + R[7];
	} else {
		q[0] = R[3] - R[1], q[1] = R[2] + R[6], q[2] = R[5] + R[7], q[3] = 1.0 - R[0] - R[4] + R[8];
	}
	const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
	for(double& c: q) c /= len;
}
// M^-1 of a symmetric 3 x 3 matrix by cofactors; false unless M is positive definite (leading minors > 0) and finite.
inline bool body_invert_spd(const double (&M)[9], double (&inv)[9]) {
	const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
	const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
	if(!(M[0] > 0.0) || !(M[0] * M[4] - M[1] * M[3] > 0.0) || !(det > 0.0) || !body_finite(det)) return false;
	inv[0] = c00 / det, inv[1] = (M[2] * M[7] - M[1] * M[8]) / det, inv[2] = (M[1] * M[5] - M[2] * M[4]) / det;
	inv[3] = c01 / det, inv[4] = (M[0] * M[8] - M[2] * M[6]) / det, inv[5] = (M[2] * M[3] - M[0] * M[5]) / det;
	inv[6] = c02 / det, inv[7] = (M[1] * M[6] - M[0] * M[7]) / det, inv[8] = (M[0] * M[4] - M[1] * M[3]) / det;
	return true;
}
// The fields of mpm_rigid_body (mass, inertia {xx yy zz xy xz yz}, com, gravity, lock, force, torque) into the constants; nullptr, or the
// message that names what an install refuses.
inline const char* body_constants(float mass, const float (&inertia)[6], const float (&com)[3], int gravity, int lock, const float (&force)[3], const float (&torque)[3], BodyConst& out) {
	for(int i = 0; i < 6; ++i)
		if(inertia[i] != inertia[i]) return "rigid body: NaN in inertia";
	for(int d = 0; d < 3; ++d)
		if(com[d] != com[d] || force[d] != force[d] || torque[d] != torque[d]) return "rigid body: NaN in com, force or torque";
	if(!(mass > 0.f) || !body_finite((double) mass)) return "rigid body: mass must be finite and > 0";
	if(lock < 0 || lock > 63) return "rigid body: lock outside bits 0..5";
	for(int d = 0; d < 3; ++d)
		if(!body_finite((double) com[d]) || !body_finite((double) force[d]) || !body_finite((double) torque[d])) return "rigid body: com, force and torque must be finite";
	BodyConst c {};
	c.mass = (double) mass, c.inv_mass = 1.0 / (double) mass;
	const double xx = inertia[0], yy = inertia[1], zz = inertia[2], xy = inertia[3], xz = inertia[4], yz = inertia[5];
	const double I[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
	for(int i = 0; i < 9; ++i) c.Ib[i] = I[i];
	if(!body_invert_spd(c.Ib, c.Ib_inv)) return "rigid body: the inertia is not symmetric positive definite";
	for(int d = 0; d < 3; ++d) c.com[d] = (double) com[d], c.force[d] = (double) force[d], c.torque[d] = (double) torque[d];
	c.gravity = gravity ? 1 : 0, c.lock = lock;
	out = c;
	return nullptr;
}
// The pose fields of a collider that may become a body; nullptr, or the message.  rot: mpm_collision_object.rot_mat (element (i, j) at [3 i + j]).
inline const char* body_object_ok(float scale, float dsdt, const float (&rot)[9], const float (&trans)[3], const float (&trans_vel)[3], const float (&omega)[3]) {
	for(int i = 0; i < 9; ++i)
		if(rot[i] != rot[i]) return "rigid body: NaN in the collider's rot_mat";
	for(int d = 0; d < 3; ++d)
		if(!body_finite((double) trans[d]) || !body_finite((double) trans_vel[d]) || !body_finite((double) omega[d])) return "rigid body: the collider's trans, trans_vel and omega must be finite";
	if(scale != 1.f || dsdt != 0.f) return "rigid body: the collider must have scale == 1 and dsdt == 0";
	double det = 0.0;
	for(int i = 0; i < 3; ++i)
		for(int j = 0; j < 3; ++j) {
			double s = 0.0;
			for(int k = 0; k < 3; ++k) s += (double) rot[3 * k + i] * (double) rot[3 * k + j];
			if(!(fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-5)) return "rigid body: the collider's rot_mat is not a rotation";
		}
	det = (double) rot[0] * ((double) rot[4] * rot[8] - (double) rot[5] * rot[7]) - (double) rot[1] * ((double) rot[3] * rot[8] - (double) rot[5] * rot[6]) +
		  (double) rot[2] * ((double) rot[3] * rot[7] - (double) rot[4] * rot[6]);
	if(det < 0.0) return "rigid body: the collider's rot_mat is a reflection (det < 0)";
	return nullptr;
}
// The start state: the body stands where the collider stands.  The kernels take a node X to the material point rot (X - shift) + trans - rot and
// shift the collider's pose at the moment of the call (rot_mat and trans while its clock is at 0) - so the rotation body -> world is R0 = rot^T;
// the slot is re-pivoted to the centre of mass (trans := com) and x0 = shift + R0 (com - trans), which leaves every node's material point where
// it was.  v0 = trans_vel; omega0 = omega, a TRUE angular velocity (world); l0 = R Ib R^T omega0.
inline void body_start(const float (&rot)[9], const float (&shift)[3], const float (&trans)[3], const float (&trans_vel)[3], const float (&omega)[3], const BodyConst& c, BodyState& s) {
	s = BodyState {};
	double R[9];
	for(int i = 0; i < 3; ++i)
		for(int j = 0; j < 3; ++j) R[3 * i + j] = (double) rot[3 * j + i];
	body_quaternion(R, s.q);
	for(int i = 0; i < 3; ++i) {
		const double d0 = c.com[0] - (double) trans[0], d1 = c.com[1] - (double) trans[1], d2 = c.com[2] - (double) trans[2];
		s.x[i] = (double) shift[i] + ((R[3 * i] * d0 + R[3 * i + 1] * d1) + R[3 * i + 2] * d2);
		s.v[i] = (double) trans_vel[i];
	}
	double Rq[9];
	body_rotation(s.q, Rq);
	const double w[3] = {(double) omega[0], (double) omega[1], (double) omega[2]};
	body_world_apply(Rq, c.Ib, w, s.l);
	body_omega(s, c);
}
// New constants for a body in motion (mpm_set_collider_body on a slot that holds one): q, v, omega and the counters are the old state's float64
// words; x moves with the centre of mass, x + R(q) (com_new - com_old), so that every node's material point stays; l = R Ib_new R^T omega.
inline void body_reconstant(const BodyState& old, const BodyConst& c_old, const BodyConst& c, BodyState& s) {
	s = old;
	double R[9];
	body_rotation(s.q, R);
	const double d[3] = {c.com[0] - c_old.com[0], c.com[1] - c_old.com[1], c.com[2] - c_old.com[2]};
	for(int i = 0; i < 3; ++i) s.x[i] = old.x[i] + ((R[3 * i] * d[0] + R[3 * i + 1] * d[1]) + R[3 * i + 2] * d[2]);
	const double w[3] = {old.omega[0], old.omega[1], old.omega[2]};
	body_world_apply(R, c.Ib, w, s.l);
	body_omega(s, c);
}
// A restart (mpm_set_collider_body_state): any of the four given replaces its part; q is normalised; l follows from omega.
inline const char* body_restart(BodyState& s, const BodyConst& c, const double* x, const double* q, const double* v, const double* omega) {
	for(int d = 0; d < 3; ++d)
		if((x && !body_finite(x[d])) || (v && !body_finite(v[d])) || (omega && !body_finite(omega[d]))) return "rigid body state: position, velocity and omega must be finite";
	if(q) {
		const double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
		if(!(len > 0.0) || !body_finite(len)) return "rigid body state: the orientation must be a finite, non-zero quaternion";
		for(int d = 0; d < 4; ++d) s.q[d] = q[d] / len;
	}
	for(int d = 0; d < 3; ++d) {
		if(x) s.x[d] = x[d];
		if(v) s.v[d] = v[d];
	}
	if(omega || q) {
		double R[9];
		body_rotation(s.q, R);
		const double w[3] = {omega ? omega[0] : s.omega[0], omega ? omega[1] : s.omega[1], omega ? omega[2] : s.omega[2]};
		body_world_apply(R, c.Ib, w, s.l);
		body_omega(s, c);
	}
	return nullptr;
}

// Mass properties.  out6 = {xx yy zz xy xz yz} about the centre of mass, in the frame the shape's parameters are given in.
// sphere: m = rho 4/3 pi r^3, I = 2/5 m r^2.  box (half extents b): m = 8 rho bx by bz, Ixx = m (by^2 + bz^2) / 3.  capsule (radius r, segment
// length l, unit axis u): cylinder mc = rho pi r^2 l and the two half spheres' ms = rho 4/3 pi r^3; about the axis Ia = mc r^2 / 2 + 2/5 ms r^2,
// across it It = mc (l^2 / 12 + r^2 / 4) + ms (2/5 r^2 + l^2 / 4 + 3/8 r l); I = It (1 - u u^T) + Ia u u^T.
inline const char* body_shape_mass(int kind, int inside_out, const float (&a)[3], const float (&b)[3], float radius, double rho, double& mass, double (&I6)[6], double (&com)[3]) {
	const double pi = 3.14159265358979323846;
	if(!(rho > 0.0) || !body_finite(rho)) return "mass properties: density must be finite and > 0";
	if(inside_out) return "mass properties: an inside-out shape is unbounded";
	for(int d = 0; d < 3; ++d)
		if(!body_finite((double) a[d])) return "mass properties: the shape's a must be finite";
	for(double& v: I6) v = 0.0;
	if(kind == 2) {// MPM_SHAPE_SPHERE
		const double r = radius;
		if(!(r > 0.0) || !body_finite(r)) return "mass properties: radius must be finite and > 0";
		mass  = rho * (4.0 / 3.0) * pi * r * r * r;
		I6[0] = I6[1] = I6[2] = 0.4 * mass * r * r;
		for(int d = 0; d < 3; ++d) com[d] = a[d];
	} else if(kind == 3) {// MPM_SHAPE_BOX
		for(int d = 0; d < 3; ++d)
			if(!((double) b[d] > 0.0) || !body_finite((double) b[d])) return "mass properties: half extents b must be finite and > 0";
		const double bx = b[0], by = b[1], bz = b[2];
		mass  = rho * 8.0 * bx * by * bz;
		I6[0] = mass * (by * by + bz * bz) / 3.0, I6[1] = mass * (bx * bx + bz * bz) / 3.0, I6[2] = mass * (bx * bx + by * by) / 3.0;
		for(int d = 0; d < 3; ++d) com[d] = a[d];
	} else if(kind == 4) {// MPM_SHAPE_CAPSULE
		const double r = radius;
		if(!(r > 0.0) || !body_finite(r)) return "mass properties: radius must be finite and > 0";
		double e[3];
		for(int d = 0; d < 3; ++d) {
			if(!body_finite((double) b[d])) return "mass properties: the shape's b must be finite";
			e[d] = (double) b[d] - (double) a[d];
		}
		const double l = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
		if(!(l > 0.0)) return "mass properties: capsule end points a and b coincide";
		const double u[3] = {e[0] / l, e[1] / l, e[2] / l};
		const double mc = rho * pi * r * r * l, ms = rho * (4.0 / 3.0) * pi * r * r * r;
		const double Ia = 0.5 * mc * r * r + 0.4 * ms * r * r;
		const double It = mc * (l * l / 12.0 + r * r / 4.0) + ms * (0.4 * r * r + l * l / 4.0 + 0.375 * r * l);
		mass  = mc + ms;
		I6[0] = It + (Ia - It) * u[0] * u[0], I6[1] = It + (Ia - It) * u[1] * u[1], I6[2] = It + (Ia - It) * u[2] * u[2];
		I6[3] = (Ia - It) * u[0] * u[1], I6[4] = (Ia - It) * u[0] * u[2], I6[5] = (Ia - It) * u[1] * u[2];
		for(int d = 0; d < 3; ++d) com[d] = 0.5 * ((double) a[d] + (double) b[d]);
	} else
		return "mass properties: only a sphere, a box or a capsule has them (a half-space is unbounded)";
	return nullptr;
}
// A closed, outward-oriented triangle mesh: signed tetrahedra against the first vertex (which keeps the terms small), float64.  Volume, centroid
// and the second moments about the centroid.  The caller has validated the mesh (closed, indices in range, finite).
inline const char* body_mesh_mass(const float* verts, size_t nv, const int32_t* tris, size_t nt, double rho, double& mass, double (&I6)[6], double (&com)[3]) {
	if(!(rho > 0.0) || !body_finite(rho)) return "mass properties: density must be finite and > 0";
	(void) nv;
	const double o[3] = {verts[0], verts[1], verts[2]};
	double vol = 0.0, c[3] = {0, 0, 0}, P[6] = {0, 0, 0, 0, 0, 0};// P: integrals of xx yy zz xy xz yz about o
	for(size_t t = 0; t < nt; ++t) {
		double p[3][3];
		for(int k = 0; k < 3; ++k)
			for(int d = 0; d < 3; ++d) p[k][d] = (double) verts[3 * (size_t) tris[3 * t + k] + d] - o[d];
		const double det = p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) - p[0][1] * (p[1][0] * p[2][2] - p[1][2] * p[2][0]) + p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0]);
		vol += det / 6.0;
		for(int d = 0; d < 3; ++d) c[d] += det / 24.0 * (p[0][d] + p[1][d] + p[2][d]);
		const int ab[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
		for(int e = 0; e < 6; ++e) {
			const int i = ab[e][0], j = ab[e][1];
			const double si = p[0][i] + p[1][i] + p[2][i], sj = p[0][j] + p[1][j] + p[2][j];
			P[e] += det / 120.0 * (si * sj + p[0][i] * p[0][j] + p[1][i] * p[1][j] + p[2][i] * p[2][j]);
		}
	}
	if(!(vol > 0.0) || !body_finite(vol)) return "mass properties: the mesh encloses no positive volume (is it oriented outwards?)";
	for(int d = 0; d < 3; ++d) c[d] /= vol;
	const double xx = P[0] - vol * c[0] * c[0], yy = P[1] - vol * c[1] * c[1], zz = P[2] - vol * c[2] * c[2];
	mass  = rho * vol;
	I6[0] = rho * (yy + zz), I6[1] = rho * (xx + zz), I6[2] = rho * (xx + yy);
	I6[3] = -rho * (P[3] - vol * c[0] * c[1]), I6[4] = -rho * (P[4] - vol * c[0] * c[2]), I6[5] = -rho * (P[5] - vol * c[1] * c[2]);
	for(int d = 0; d < 3; ++d) com[d] = o[d] + c[d];
	return nullptr;
}

}// namespace mpm
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#if defined(__HIPCC__)
// ---- 3. the kernels -------------------------------------------------------------------------------------------------------------------------
#include "mpm_collider_loads.hpp"

namespace mpm {

// What travels to the kernels with a body installed: the colliders as ever - a body slot's object with trans = com and trans_vel = omega = 0, so
// that collision_respond's own object velocity is exactly 0 - and where the poses and the states live.  mask: bit s = slot s is a body.
// state_pivots: bit s = row 1 + s takes its torque about the state's x (read from the device) instead of the pivot that travels by value.
struct BodyArgs {
	VolumeColliderArgs va;
	const BodyPose* pose;
	const BodyState* state;
	int mask, state_pivots;
};
template<class Collider>
constexpr bool kCarriesBodies = std::is_same_v<Collider, BodyArgs>;// (what the host's launches ask instead of naming the type)
MPM_DEV const ShapeArgs& shape_args(const BodyArgs& a) { return a.va.ter.col; }

// slot_resolve with bodies among the slots: BodyArgs' part in load_cell, whose every other statement is the prescribed colliders'.  A body slot at
// the node X, in this order and without contraction:
//   r = X - shift;  vb = vel + omega x r (a true cross product);  rel = velocity - vb;  r2 = rel;  slot_resolve(..., pose, X, r2)
//   if any component of r2 differs from rel IN ITS BITS (a NaN differs): velocity = r2 + vb;  else the node is not touched and its velocity keeps
//   its bits.  (On bits, so that a response which turns -0 into +0 - `v - v_obj + v_obj` with v_obj = 0 - does so for a body at rest as well.)
// with pose = {rot, shift} of the BodyPose, inv = 1, growth = 0.
MPM_DEV void slot_resolve(const BodyArgs& a, int s, const float (&X)[3], float (&vel)[3]) {
#pragma clang fp contract(off)
	if(!((a.mask >> s) & 1)) return slot_resolve(a.va, s, X, vel);
	const BodyPose& bp = a.pose[s];// (wave-uniform: s is)
	CollisionPose pose;
#pragma unroll
	for(int i = 0; i < 9; ++i) pose.rot[i] = bp.rot[i];
	pose.inv = 1.f, pose.growth = 0.f;
	float r[3], vb[3], rel[3], r2[3];
#pragma unroll
	for(int d = 0; d < 3; ++d) pose.shift[d] = bp.shift[d], r[d] = X[d] - bp.shift[d];
	vb[0] = bp.vel[0] + (bp.omega[1] * r[2] - bp.omega[2] * r[1]);
	vb[1] = bp.vel[1] + (bp.omega[2] * r[0] - bp.omega[0] * r[2]);
	vb[2] = bp.vel[2] + (bp.omega[0] * r[1] - bp.omega[1] * r[0]);
#pragma unroll
	for(int d = 0; d < 3; ++d) rel[d] = vel[d] - vb[d], r2[d] = rel[d];
	slot_resolve(a.va, s, pose, X, r2);
	auto differs = [](float x, float y) { return __float_as_uint(x) != __float_as_uint(y) || x != x; };
	if(differs(r2[0], rel[0]) || differs(r2[1], rel[1]) || differs(r2[2], rel[2])) {
#pragma unroll
		for(int d = 0; d < 3; ++d) vel[d] = r2[d] + vb[d];
	}
}
// A body row's pivot is the state's x, read here, where state_pivots says so (mpm_collider_loads' default for a body, and every applied update's).
MPM_DEV void row_pivot(const BodyArgs& a, const LoadPivots& piv, int row, double (&p)[3]) {
	p[0] = piv.p[row][0], p[1] = piv.p[row][1], p[2] = piv.p[row][2];
	if(row >= 1 && row <= kMaxBodies && ((a.state_pivots >> (row - 1)) & 1)) {
		const BodyState& st = a.state[row - 1];
		p[0] = st.x[0], p[1] = st.x[1], p[2] = st.x[2];
	}
}

// The grid update with bodies, ONE pass: loads_frame with the stores - the readout's walk over the blocks, its wave reduction into per-wave LDS
// rows, hence the same order of every addition, and totals that equal mpm_collider_loads' bit for bit, because they are the same statements.
// (The readout with a body installed is collider_loads_kernel<BodyArgs>.)
template<class Collider>
__global__ __launch_bounds__(256) void grid_update_body_kernel(GridCfg cfg, const int* __restrict__ nbc_ptr, float* grid, const int* __restrict__ keys, float dt, Collider col, LoadPivots piv, double* __restrict__ partials, unsigned* __restrict__ max_vel_bits) {
	loads_frame<true>(cfg, nbc_ptr, grid, keys, dt, col, piv, partials, max_vel_bits);
}

// One workgroup of kLoadReduceThreads: load_totals - the readout's reduction -, then lane s < kMaxBodies of wave 0 steps body s of `mask` with its
// row's totals and writes BodyState and BodyPose.  A non-finite J, L or state raises the status block's non-finite flag.
__global__ __launch_bounds__(kLoadReduceThreads) void body_step_kernel(const double* __restrict__ partials, int groups, BodyBlock* __restrict__ blk, int mask, float dt, float gravity, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
	__shared__ double s_tot[kLoadRows * kLoadSums];
	const double total = load_totals(partials, groups);
	if(threadIdx.x < kLoadRows * kLoadSums) s_tot[threadIdx.x] = total;
	__syncthreads();
	if(threadIdx.x < kMaxBodies && ((mask >> threadIdx.x) & 1)) {
		const int s		= threadIdx.x;
		const double* t = &s_tot[(1 + s) * kLoadSums];
		const double J[3] = {t[1], t[2], t[3]}, L[3] = {t[4], t[5], t[6]};
		BodyState st = blk->st[s];
		const bool ok = body_step(st, blk->c[s], J, L, t[0], t[7], (double) dt, (double) gravity);
		blk->st[s]	  = st;
		BodyPose p;
		body_pose(st, p);
		blk->pose[s] = p;
		if(!ok) *nonfinite = 1;
	}
}

}// namespace mpm
#endif// __HIPCC__
