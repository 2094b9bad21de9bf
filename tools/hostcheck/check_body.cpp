// x86 build of the rigid bodies' definition and host side (mpm_rigid_body.hpp, parts 1 and 2) behind a small C interface: the step, the float32
// pose, the start state of a collider, the checks of an install.  tests/test_rigid_body_cpu.py compares it with tests/rigid_body_model.py on bits.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Itools/hostcheck -Iclaymore_amd/csrc -o libhostbody.so tools/hostcheck/check_body.cpp
struct float4 {
	float x, y, z, w;
};
#include "../../include/claymore_amd.h"
#include "mpm_collision.hpp"
#include "mpm_rigid_body.hpp"

#include <cstring>
using namespace mpm;
static_assert(sizeof(BodyState) == sizeof(mpm_rigid_body_state), "the ABI's state is the header's");

// nullptr, or why mpm_set_collider_body refuses these constants
extern "C" const char* host_body_constants(const mpm_rigid_body* b) {
	BodyConst c;
	return body_constants(b->mass, b->inertia, b->com, b->gravity, b->lock, b->force, b->torque, c);
}
// nullptr, or why a collider with these pose fields cannot become a body (the clock at 0: rot = rot_mat)
extern "C" const char* host_body_object(const mpm_collision_object* o) {
	return body_object_ok(o->scale, o->dsdt, o->rot_mat, o->trans, o->trans_vel, o->omega);
}
// n steps of body_step from *state with the same J, L, touched nodes and mass each; returns the number of steps that reported a non-finite value
extern "C" int host_body_step(mpm_rigid_body_state* state, const mpm_rigid_body* b, const double* J, const double* L, double n_touched, double m_touched, float dt, float gravity, int steps) {
	BodyConst c;
	if(body_constants(b->mass, b->inertia, b->com, b->gravity, b->lock, b->force, b->torque, c)) return -1;
	BodyState s;
	memcpy(&s, state, sizeof(s));
	const double j[3] = {J[0], J[1], J[2]}, l[3] = {L[0], L[1], L[2]};
	int bad = 0;
	for(int i = 0; i < steps; ++i) bad += body_step(s, c, j, l, n_touched, m_touched, (double) dt, (double) gravity) ? 0 : 1;
	memcpy(state, &s, sizeof(s));
	return bad;
}
// the start state of a body made of this collider at the clock's `time`, and its float32 pose {rot[9], shift[3], vel[3], omega[3]}
extern "C" int host_body_start(const mpm_collision_object* obj, float time, const mpm_rigid_body* b, mpm_rigid_body_state* state, float* pose18) {
	BodyConst c;
	if(body_constants(b->mass, b->inertia, b->com, b->gravity, b->lock, b->force, b->torque, c)) return -1;
	CollisionObject o {};
	o.scale = obj->scale, o.dsdt = obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	const CollisionPose p = collision_pose(o, time);
	BodyState s;
	body_start(p.rot, p.shift, o.trans, o.trans_vel, o.omega, c, s);
	memcpy(state, &s, sizeof(s));
	BodyPose bp;
	body_pose(s, bp);
	memcpy(pose18, &bp, sizeof(bp));
	return 0;
}
extern "C" void host_body_pose(const mpm_rigid_body_state* state, float* pose18) {
	BodyState s;
	memcpy(&s, state, sizeof(s));
	BodyPose bp;
	body_pose(s, bp);
	memcpy(pose18, &bp, sizeof(bp));
}
// a restart: any pointer may be NULL; nullptr or the refusal
extern "C" const char* host_body_restart(mpm_rigid_body_state* state, const mpm_rigid_body* b, const double* x, const double* q, const double* v, const double* omega) {
	BodyConst c;
	if(const char* msg = body_constants(b->mass, b->inertia, b->com, b->gravity, b->lock, b->force, b->torque, c)) return msg;
	BodyState s;
	memcpy(&s, state, sizeof(s));
	const char* msg = body_restart(s, c, x, q, v, omega);
	if(!msg) memcpy(state, &s, sizeof(s));
	return msg;
}
