// mpm_collision_heightfield.hpp — a collision object given as a 2-D height table: terrain y = h(x, z).
//
// An extension, like the analytic shapes (mpm_collision_shapes.hpp; the reference knows level sets only), and the one collider kind of the
// slots that reads memory: one float4 {H, gx, gz, 0} per sample (i, k) at [i nz + k], built on the host at install (heightfield_build).
// It is the level-set kernel's idiom in two dimensions: one 16-byte load per stencil corner, and normals that are continuous across table
// cells because the gradient is interpolated, not derived per cell.  A node is taken to its material point by collision_material_point
// (mpm_collision.hpp), the table answers with sdis and a unit normal, and from `sdis <= 0` on the node runs through collision_respond.  Up is
// material y: obj.rot_mat, trans and trans_vel tilt and move the terrain.  query_sdf's domain box does not apply; outside the table's
// footprint the collider touches nothing.
// sdis is the distance to the TANGENT PLANE of the interpolated surface under the point ((x_1 - h) / len), not a Euclidean distance: the
// response uses its sign only.
// Builds on x86 like mpm_collision_shapes.hpp (tools/hostcheck/check_heightfield.cpp): MPM_DEV only, contraction off, plain IEEE `/` and sqrtf.
// tests/heightfield_model.py restates every function below statement for statement with numpy float32.
#pragma once
#include "mpm_collision.hpp"

namespace mpm {

enum { kHeightfieldMinSamples = 2, kHeightfieldMaxSamples = 4096 };// per axis (MPM_HEIGHTFIELD_MAX_SAMPLES)

struct Heightfield {// mpm_heightfield as installed: the table lives in device memory (in host memory for the x86 build)
	const float4* table;// nx * nz entries {H, gx, gz, 0}, sample (i, k) at [i nz + k]
	int nx, nz;
	float origin[2];// material (x, z) of sample (0, 0)
	float spacing;
	int inside_out;
};

// Host side (plain C++, no contraction): the table from the heights H(i, k) at [i nz + k].  Statement order, per sample:
//   gx = i == 0 ? (H(1,k) - H(0,k)) / spacing : i == nx-1 ? (H(nx-1,k) - H(nx-2,k)) / spacing : (H(i+1,k) - H(i-1,k)) / (2.f * spacing)
//   gz the same along k;  out(i,k) = {H(i,k), gx, gz, 0}.
// Returns false where a height or a derived entry is not finite (the table is then not to be used).  nx, nz >= 2.
inline bool heightfield_build(const float* H, int nx, int nz, float spacing, float4* out) {
#pragma clang fp contract(off)
	bool finite = true;
	for(int i = 0; i < nx; ++i)
		for(int k = 0; k < nz; ++k) {
			const size_t at = (size_t) i * nz + k;
			float gx, gz;
			if(i == 0)
				gx = (H[(size_t) nz + k] - H[k]) / spacing;
			else if(i == nx - 1)
				gx = (H[at] - H[at - nz]) / spacing;
			else
				gx = (H[at + nz] - H[at - nz]) / (2.f * spacing);
			if(k == 0)
				gz = (H[at + 1] - H[at]) / spacing;
			else if(k == nz - 1)
				gz = (H[at] - H[at - 1]) / spacing;
			else
				gz = (H[at + 1] - H[at - 1]) / (2.f * spacing);
			out[at].x = H[at];
			out[at].y = gx;
			out[at].z = gz;
			out[at].w = 0.f;
			// (x - x == 0 exactly for every finite x, NaN for an infinity or a NaN)
			if(!(H[at] - H[at] == 0.f && gx - gx == 0.f && gz - gz == 0.f)) finite = false;
		}
	return finite;
}

// Signed tangent-plane distance and unit normal of the terrain at the material point x.  Statement order:
//   u = (x_0 - origin_0) / spacing;  w = (x_2 - origin_1) / spacing
//   outside unless 0 <= u <= (float) (nx - 1) and 0 <= w <= (float) (nz - 1) (a NaN is outside): sdis = NaN, n = 0, whatever inside_out
//   says - NOTHING is loaded (the range check is what keeps the four indices inside the table)
//   i = min((int) u, nx - 2);  k = min((int) w, nz - 2);  fu = u - (float) i;  fw = w - (float) k
//   cu = 1.f - fu;  cw = 1.f - fw;  w00 = cu cw;  w10 = fu cw;  w01 = cu fw;  w11 = fu fw      (wab: sample (i + a, k + b))
//   every channel c of {h, gx, gz}: ((w00 t00.c + w10 t10.c) + w01 t01.c) + w11 t11.c
//   len = sqrtf((gx gx + 1.f) + gz gz)   (never zero);  n = (-gx / len, 1.f / len, -gz / len);  sdis = (x_1 - h) / len
//   inside_out: sdis = -sdis, n_i = -n_i   (the solid is ABOVE the surface: a ceiling)
MPM_DEV void heightfield_query(const Heightfield& f, const float (&x)[3], float& sdis, float (&n)[3]) {
#pragma clang fp contract(off)
	const float u = (x[0] - f.origin[0]) / f.spacing;
	const float w = (x[2] - f.origin[1]) / f.spacing;
	if(!(u >= 0.f && u <= (float) (f.nx - 1) && w >= 0.f && w <= (float) (f.nz - 1))) {
		sdis = __builtin_nanf("");
		n[0] = n[1] = n[2] = 0.f;
		return;
	}
	const int iu = (int) u, iw = (int) w;
	const int i = iu < f.nx - 2 ? iu : f.nx - 2;
	const int k = iw < f.nz - 2 ? iw : f.nz - 2;
	const float fu = u - (float) i, fw = w - (float) k;
	const float cu = 1.f - fu, cw = 1.f - fw;
	const float w00 = cu * cw, w10 = fu * cw, w01 = cu * fw, w11 = fu * fw;
	const float4* row = f.table + (size_t) i * f.nz + k;
	const float4 t00 = row[0], t01 = row[1], t10 = row[f.nz], t11 = row[f.nz + 1];
	const float h  = ((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x;
	const float gx = ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y;
	const float gz = ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z;
	const float len = sqrtf((gx * gx + 1.f) + gz * gz);
	n[0] = -gx / len;
	n[1] = 1.f / len;
	n[2] = -gz / len;
	sdis = (x[1] - h) / len;
	if(f.inside_out) {
		sdis = -sdis;
#pragma unroll
		for(int d = 0; d < 3; ++d) n[d] = -n[d];
	}
}

// One heightfield acting on one domain point X (a node: (float) node * dx): shape_resolve's statements around heightfield_query.
MPM_DEV void heightfield_resolve(const CollisionObject& o, const CollisionPose& p, const Heightfield& f, const float (&X)[3], float (&vel)[3]) {
#pragma clang fp contract(off)
	float xmt[3], x[3], n[3], sdis;
	collision_material_point(o, p, X, xmt, x);
	heightfield_query(f, x, sdis, n);
	if(!(sdis <= 0.f)) return;
	collision_respond(o, p, xmt, x, n, vel);
}

}// namespace mpm
