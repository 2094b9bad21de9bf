// x86 build of the collision object's two halves (mpm_collision.hpp): the pose as the host computes it per grid update and the per-node
// part the kernels run, one node at a time.  Same call shape as the oracle's mpmo_fn_collision_resolve.
// Build: clang++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Itools/hostcheck -Iclaymore_amd/csrc -o libhostcollision.so tools/hostcheck/check_collision.cpp
struct float4 {
	float x, y, z, w;
};
#include "../../include/claymore_amd.h"
#include "mpm_collision.hpp"
using namespace mpm;
// field4: node-major {sdis, gx, gy, gz}, N^3 nodes; boundary / G in blocks as in GridCfg; nodes[n*3] global node indices; vel[n*3] in place
extern "C" int host_collision_resolve(const mpm_collision_object* obj, const float* field4, int N, float dx, int boundary, int G, const int* nodes, size_t n, float time, float* vel) {
	CollisionObject o {};
	o.type	   = obj->type;
	o.friction = obj->friction;
	o.scale	   = obj->scale;
	o.dsdt	   = obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	o.time	= time;
	o.field = reinterpret_cast<const float4*>(field4);
	const CollisionPose p = collision_pose(o, time);
	for(size_t i = 0; i < n; ++i) {
		const int node[3] = {nodes[3 * i], nodes[3 * i + 1], nodes[3 * i + 2]};
		float v[3]		  = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
		collision_resolve(o, p, node, dx, N, (float) boundary * dx * 4.f, (float) (G - boundary) * 4.f * dx, v);
		for(int d = 0; d < 3; ++d) vel[3 * i + d] = v[d];
	}
	return 0;
}
extern "C" void host_collision_pose(const mpm_collision_object* obj, float time, float* out14) {
	CollisionObject o {};
	o.scale = obj->scale;
	o.dsdt	= obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	const CollisionPose p = collision_pose(o, time);
	for(int i = 0; i < 9; ++i) out14[i] = p.rot[i];
	out14[9] = p.inv;
	for(int d = 0; d < 3; ++d) out14[10 + d] = p.shift[d];
	out14[13] = p.growth;
}
