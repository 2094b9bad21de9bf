// x86 build of the analytic collision shapes (mpm_collision_shapes.hpp) behind a small C interface: the query (material point, signed
// distance, normal) and query + response, one domain point at a time.  The normal of a half-space is normalised as the library does on install.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Itools/hostcheck -Iclaymore_amd/csrc -o libhostshapes.so tools/hostcheck/check_shapes.cpp
struct float4 {
	float x, y, z, w;
};
#include "../../include/claymore_amd.h"
#include "mpm_collision_shapes.hpp"
using namespace mpm;
static void convert(const mpm_collision_object* obj, const mpm_collision_shape* sh, float time, CollisionObject& o, CollisionShape& s, CollisionPose& p) {
	o		   = CollisionObject {};
	o.type	   = obj->type;
	o.friction = obj->friction;
	o.scale	   = obj->scale;
	o.dsdt	   = obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	o.time		 = time;
	o.field		 = nullptr;
	s.kind		 = sh->kind;
	s.inside_out = sh->inside_out ? 1 : 0;
	for(int d = 0; d < 3; ++d) s.a[d] = sh->a[d], s.b[d] = sh->b[d];
	s.radius = sh->radius;
	if(sh->kind == MPM_SHAPE_HALFSPACE) {
		const float len = sqrtf(sh->b[0] * sh->b[0] + sh->b[1] * sh->b[1] + sh->b[2] * sh->b[2]);
		for(int d = 0; d < 3; ++d) s.b[d] = sh->b[d] / len;
	}
	p = collision_pose(o, time);
}
// xyz[n*3] domain points -> out7[n*7] = {sdis, nx, ny, nz, x, y, z}: what shape_query sees and answers
extern "C" int host_shape_query(const mpm_collision_object* obj, const mpm_collision_shape* sh, float time, const float* xyz, size_t n, float* out7) {
	CollisionObject o;
	CollisionShape s;
	CollisionPose p;
	convert(obj, sh, time, o, s, p);
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
		float xmt[3], x[3], nrm[3], sdis;
		collision_material_point(o, p, X, xmt, x);
		shape_query(s, x, sdis, nrm);
		out7[7 * i] = sdis;
		for(int d = 0; d < 3; ++d) out7[7 * i + 1 + d] = nrm[d], out7[7 * i + 4 + d] = x[d];
	}
	return 0;
}
// nodes[n*3] integer node coordinates (X = (float) node * dx, as the grid kernels form it); vel[n*3] in place
extern "C" int host_shape_resolve(const mpm_collision_object* obj, const mpm_collision_shape* sh, float time, float dx, const int* nodes, size_t n, float* vel) {
	CollisionObject o;
	CollisionShape s;
	CollisionPose p;
	convert(obj, sh, time, o, s, p);
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {(float) nodes[3 * i] * dx, (float) nodes[3 * i + 1] * dx, (float) nodes[3 * i + 2] * dx};
		float v[3]		 = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
		shape_resolve(o, p, s, X, v);
		for(int d = 0; d < 3; ++d) vel[3 * i + d] = v[d];
	}
	return 0;
}
