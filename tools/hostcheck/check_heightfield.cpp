// x86 build of the heightfield collider (mpm_collision_heightfield.hpp) behind a small C interface: the table builder, the query (material
// point, signed tangent-plane distance, normal) and query + response, one domain point at a time.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Itools/hostcheck -Iclaymore_amd/csrc -o libhostheightfield.so tools/hostcheck/check_heightfield.cpp
struct float4 {
	float x, y, z, w;
};
#include <vector>
#include "../../include/claymore_amd.h"
#include "mpm_collision_heightfield.hpp"
using namespace mpm;
static bool convert(const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights, float time, CollisionObject& o, Heightfield& f, std::vector<float4>& table, CollisionPose& p) {
	o		   = CollisionObject {};
	o.type	   = obj->type;
	o.friction = obj->friction;
	o.scale	   = obj->scale;
	o.dsdt	   = obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	o.time	= time;
	o.field = nullptr;
	if(hf->nx < 2 || hf->nz < 2 || hf->nx > MPM_HEIGHTFIELD_MAX_SAMPLES || hf->nz > MPM_HEIGHTFIELD_MAX_SAMPLES) return false;
	table.resize((size_t) hf->nx * hf->nz);
	if(!heightfield_build(heights, hf->nx, hf->nz, hf->spacing, table.data())) return false;
	f.table		 = table.data();
	f.nx		 = hf->nx;
	f.nz		 = hf->nz;
	f.origin[0]	 = hf->origin[0];
	f.origin[1]	 = hf->origin[1];
	f.spacing	 = hf->spacing;
	f.inside_out = hf->inside_out ? 1 : 0;
	p			 = collision_pose(o, time);
	return true;
}
// heights[nx*nz] -> out4[nx*nz*4] = {H, gx, gz, 0}; returns 0, or 1 where an entry is not finite
extern "C" int host_heightfield_build(const float* heights, int nx, int nz, float spacing, float* out4) {
	return heightfield_build(heights, nx, nz, spacing, reinterpret_cast<float4*>(out4)) ? 0 : 1;
}
// xyz[n*3] domain points -> out7[n*7] = {sdis, nx, ny, nz, x, y, z}: what heightfield_query sees and answers
extern "C" int host_heightfield_query(const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights, float time, const float* xyz, size_t n, float* out7) {
	CollisionObject o;
	Heightfield f;
	CollisionPose p;
	std::vector<float4> table;
	if(!convert(obj, hf, heights, time, o, f, table, p)) return 1;
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
		float xmt[3], x[3], nrm[3], sdis;
		collision_material_point(o, p, X, xmt, x);
		heightfield_query(f, x, sdis, nrm);
		out7[7 * i] = sdis;
		for(int d = 0; d < 3; ++d) out7[7 * i + 1 + d] = nrm[d], out7[7 * i + 4 + d] = x[d];
	}
	return 0;
}
// nodes[n*3] integer node coordinates (X = (float) node * dx, as the grid kernels form it); vel[n*3] in place
extern "C" int host_heightfield_resolve(const mpm_collision_object* obj, const mpm_heightfield* hf, const float* heights, float time, float dx, const int* nodes, size_t n, float* vel) {
	CollisionObject o;
	Heightfield f;
	CollisionPose p;
	std::vector<float4> table;
	if(!convert(obj, hf, heights, time, o, f, table, p)) return 1;
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {(float) nodes[3 * i] * dx, (float) nodes[3 * i + 1] * dx, (float) nodes[3 * i + 2] * dx};
		float v[3]		 = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
		heightfield_resolve(o, p, f, X, v);
		for(int d = 0; d < 3; ++d) vel[3 * i + d] = v[d];
	}
	return 0;
}
