// x86 build of the force fields (mpm_force_field.hpp) behind a small C interface: force_cell at arbitrary domain points with given {m, p}.
// The vortex axis and a half-space region's normal are normalised as the library does on install; nothing is validated.
// Build: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -Itools/hostcheck -Iclaymore_amd/csrc -o libhostforces.so tools/hostcheck/check_forces.cpp
struct float4 {
	float x, y, z, w;
};
#include "../../include/claymore_amd.h"
#include "mpm_force_field.hpp"
using namespace mpm;
static void unit3(const float* v, float* out) {
	const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	for(int d = 0; d < 3; ++d) out[d] = v[d] / len;
}
static ForceSlot convert(const mpm_force_field& f) {
	ForceSlot c {};
	c.kind	  = f.kind;
	c.falloff = f.falloff;
	for(int d = 0; d < 3; ++d) c.vec[d] = f.vec[d], c.centre[d] = f.centre[d];
	if(f.kind == MPM_FORCE_VORTEX) unit3(f.vec, c.vec);
	c.strength = f.strength, c.swirl = f.swirl, c.pull = f.pull, c.lift = f.lift, c.soft = f.soft, c.feather = f.feather;
	const mpm_collision_shape& r = f.region;
	c.region.kind				 = r.kind;
	c.region.inside_out			 = r.inside_out ? 1 : 0;
	for(int d = 0; d < 3; ++d) c.region.a[d] = r.a[d], c.region.b[d] = r.b[d];
	c.region.radius = r.radius;
	if(r.kind == MPM_SHAPE_HALFSPACE) unit3(r.b, c.region.b);
	return c;
}
// fields[i] sits in slot i (kind 0: empty); xyz[n*3], mp4[n*4] = {m, p} -> out4[n*4]
extern "C" int host_force_cell(const mpm_force_field* fields, int n_fields, float dt, const float* xyz, const float* mp4, size_t n, float* out4) {
	if(n_fields < 0 || n_fields > kMaxForceFields) return 1;
	ForceArgs fa {};
	for(int i = 0; i < n_fields; ++i) {
		fa.slot[i] = convert(fields[i]);
		if(fa.slot[i].kind) fa.count = i + 1;
	}
	for(size_t i = 0; i < n; ++i) {
		const float X[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
		float4 v		 = {mp4[4 * i], mp4[4 * i + 1], mp4[4 * i + 2], mp4[4 * i + 3]};
		force_cell(fa, X, dt, v);
		out4[4 * i] = v.x, out4[4 * i + 1] = v.y, out4[4 * i + 2] = v.z, out4[4 * i + 3] = v.w;
	}
	return 0;
}
