// x86 build of the volume collider (mpm_collision_volume.hpp) behind a small C interface: the query (material point, signed distance, normal)
// and query + response, one domain point at a time, the samples' positions and the auto-sized box of a mesh install.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Itools/hostcheck -Iclaymore_amd/csrc -o libhostvolume.so tools/hostcheck/check_volume.cpp
struct float4 {
	float x, y, z, w;
};
#include "../../include/claymore_amd.h"
#include "mpm_collision_volume.hpp"
using namespace mpm;
static bool convert(const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4, float time, CollisionObject& o, Volume& f, CollisionPose& p) {
	o		   = CollisionObject {};
	o.type	   = obj->type;
	o.friction = obj->friction;
	o.scale	   = obj->scale;
	o.dsdt	   = obj->dsdt;
	for(int d = 0; d < 3; ++d) o.trans[d] = obj->trans[d], o.trans_vel[d] = obj->trans_vel[d], o.omega[d] = obj->omega[d];
	for(int i = 0; i < 9; ++i) o.rot[i] = obj->rot_mat[i];
	o.time	= time;
	o.field = nullptr;
	for(int d = 0; d < 3; ++d)
		if(vol->dims[d] < kVolumeMinSamples || vol->dims[d] > MPM_VOLUME_MAX_SAMPLES) return false;
	f.table = reinterpret_cast<const float4*>(field4);
	for(int d = 0; d < 3; ++d) f.dims[d] = vol->dims[d], f.origin[d] = vol->origin[d];
	f.spacing	 = vol->spacing;
	f.inside_out = vol->inside_out ? 1 : 0;
	p			 = collision_pose(o, time);
	return true;
}
// xyz[n*3] domain points -> out7[n*7] = {sdis, nx, ny, nz, x, y, z}: what volume_query sees and answers
extern "C" int host_volume_query(const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4, float time, const float* xyz, size_t n, float* out7) {
	CollisionObject o;
	Volume f;
	CollisionPose p;
	if(!convert(obj, vol, field4, time, o, f, p)) return 1;
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
		float xmt[3], x[3], nrm[3], sdis;
		collision_material_point(o, p, X, xmt, x);
		volume_query(f, x, sdis, nrm);
		out7[7 * i] = sdis;
		for(int d = 0; d < 3; ++d) out7[7 * i + 1 + d] = nrm[d], out7[7 * i + 4 + d] = x[d];
	}
	return 0;
}
// nodes[n*3] integer node coordinates (X = (float) node * dx, as the grid kernels form it); vel[n*3] in place
extern "C" int host_volume_resolve(const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4, float time, float dx, const int* nodes, size_t n, float* vel) {
	CollisionObject o;
	Volume f;
	CollisionPose p;
	if(!convert(obj, vol, field4, time, o, f, p)) return 1;
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {(float) nodes[3 * i] * dx, (float) nodes[3 * i + 1] * dx, (float) nodes[3 * i + 2] * dx};
		float v[3]		 = {vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]};
		volume_resolve(o, p, f, X, v);
		for(int d = 0; d < 3; ++d) vel[3 * i + d] = v[d];
	}
	return 0;
}
// out[n] = origin + (float) i * spacing for i in [0, n)
extern "C" void host_volume_sample_points(float origin, float spacing, int n, float* out) {
	for(int i = 0; i < n; ++i) out[i] = volume_sample_point(origin, spacing, i);
}
// the box of a mesh install with dims == 0; returns 0, or 1 where it leaves the limits
extern "C" int host_volume_autosize(const float* verts, size_t nv, float spacing, int pad, float* origin3, int* dims3) {
	float o[3];
	int d[3]	  = {0, 0, 0};
	const bool ok = volume_autosize(verts, nv, spacing, pad, o, d);
	for(int k = 0; k < 3; ++k) origin3[k] = o[k], dims3[k] = d[k];
	return ok ? 0 : 1;
}
