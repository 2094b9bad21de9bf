// mpm_collision_volume.hpp — a collision object given as a local level-set box: a dense table of {sdis, gx, gy, gz} samples with its own origin,
// spacing and dimensions, in one of the four slots.
//
// An extension, the 3-D version of the heightfield (mpm_collision_heightfield.hpp): the level-set object of mpm_collision.hpp keeps a float4 per
// node of the whole domain, at the grid's resolution, once per context; a volume keeps dims[0] x dims[1] x dims[2] samples `spacing` apart from
// `origin` in material coordinates (96^3 samples: 14 MiB), touches nothing outside that footprint, and up to four of them move independently.
// A node is taken to its material point by collision_material_point, the table answers with sdis and a unit normal by query_sdf's own
// statements (collision_resolve, on xl = x - origin and `spacing` for dx), and from `sdis <= 0` on the node runs through collision_respond.
// query_sdf's domain box does not apply; with origin 0, spacing dx and dims N the statements are the level-set kernel's on the same numbers.
// Three parts:
//   1. the definition - volume_query / volume_resolve / volume_sample_point / volume_autosize - MPM_DEV or plain C++, float32 in one written-down
//      order without contraction; it builds on x86 too (tools/hostcheck/check_volume.cpp; tests/collision_volume_model.py restates it in NumPy);
//   2. the install-time kernel that fills a table from a closed triangle mesh (HIP only): mpm_collision_mesh.hpp's field definition evaluated at
//      the table's samples, one wave per 4 x 4 x 4 sample tile - collision_mesh_table_kernel, in that file;
//   3. the read-back kernel of mpm_get_collision_volume (HIP only): collision_table_box_kernel, in that file too.
// The definition is in include/claymore_amd.h and INTEGRATION.md section 5.
#pragma once
// The response (volume_resolve) needs mpm_collision.hpp and with it a HIP runtime header - the real one, or tools/hostcheck's stand-in.  A plain
// host build without either (claymore_amd/host/host_selftest.cpp --volume-query) gets the query alone and provides float4 itself.
#if defined(__HIPCC__) || __has_include(<hip/hip_runtime.h>)
#include "mpm_collision.hpp"
#define MPM_VOLUME_HAS_RESPONSE 1
#else
#include <math.h>
#include <stddef.h>
#ifndef MPM_DEV
#define MPM_DEV inline
#endif
#endif

// No contraction anywhere in the definition (mpm_collision.hpp says why), spelled for the compiler at hand as mpm_collision_mesh.hpp does: clang
// (hipcc) takes the pragma per function; g++, which builds the host tools, takes the option for the whole file and knows neither clang pragma.
#if defined(__clang__)
#define MPM_VOLUME_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MPM_VOLUME_UNROLL _Pragma("unroll")
#else
#define MPM_VOLUME_NO_CONTRACT
#define MPM_VOLUME_UNROLL
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

namespace mpm {

enum { kVolumeMinSamples = 2, kVolumeMaxSamples = 1024 };// per axis (MPM_VOLUME_MAX_SAMPLES)
constexpr long long kVolumeMaxTable = 1ll << 27;		  // samples per table (2 GiB)

struct Volume {// mpm_collision_volume as installed: the table lives in device memory (in host memory for the x86 build)
	const float4* table;// dims[0] dims[1] dims[2] entries {sdis, gx, gy, gz}, sample (i, j, k) at [(i dims[1] + j) dims[2] + k]
	int dims[3];
	float origin[3];// material position of sample (0, 0, 0)
	float spacing;
	int inside_out;
};

// Material position of sample i along axis d: one multiplication, one addition.
MPM_DEV float volume_sample_point(float origin, float spacing, int i) {
	MPM_VOLUME_NO_CONTRACT
	const float s = (float) i * spacing;
	return origin + s;
}

// Signed distance and unit normal of the volume at the material point x.  Statement order, per axis d:
//   xl_d = x_d - origin_d;  u_d = xl_d / spacing
//   outside unless 0 <= u_d <= (float) (dims_d - 1) on all three axes (a NaN is outside): sdis = NaN, n = 0, whatever inside_out says -
//   NOTHING is loaded (the range check is what keeps the eight indices inside the table)
//   cid_d = min((int) u_d, dims_d - 2);  dis = xl_d - (float) cid_d * spacing;  w[d][0] = 1.f - dis / spacing;  w[d][1] = dis / spacing
//   sdis = 0, g = 0; for i, j, k in {0, 1} (i slowest): w = w[0][i] * w[1][j] * w[2][k]; v = table(cid + (i, j, k)); sdis += w * v.x; g += w * v.yzw
//   nn = sqrtf(g_0 g_0 + g_1 g_1 + g_2 g_2);  n_d = g_d / nn   (a zero gradient gives what it gives in the level set)
//   inside_out: sdis = -sdis, n_d = -n_d
MPM_DEV void volume_query(const Volume& f, const float (&x)[3], float& sdis, float (&n)[3]) {
	MPM_VOLUME_NO_CONTRACT
	float xl[3], u[3];
	MPM_VOLUME_UNROLL
	for(int d = 0; d < 3; ++d) {
		xl[d] = x[d] - f.origin[d];
		u[d]  = xl[d] / f.spacing;
	}
	if(!(u[0] >= 0.f && u[0] <= (float) (f.dims[0] - 1) && u[1] >= 0.f && u[1] <= (float) (f.dims[1] - 1) && u[2] >= 0.f && u[2] <= (float) (f.dims[2] - 1))) {
		sdis = __builtin_nanf("");
		n[0] = n[1] = n[2] = 0.f;
		return;
	}
	int cid[3];
	float w1[3][2];
	MPM_VOLUME_UNROLL
	for(int d = 0; d < 3; ++d) {
		const int iu	   = (int) u[d];
		cid[d]			   = iu < f.dims[d] - 2 ? iu : f.dims[d] - 2;
		const float dis_lb = xl[d] - ((float) cid[d] * f.spacing);
		w1[d][0]		   = 1.f - dis_lb / f.spacing;
		w1[d][1]		   = dis_lb / f.spacing;
	}
	sdis = 0.f;
	n[0] = n[1] = n[2] = 0.f;
	MPM_VOLUME_UNROLL
	for(int i = 0; i < 2; ++i)
	MPM_VOLUME_UNROLL
		for(int j = 0; j < 2; ++j)
	MPM_VOLUME_UNROLL
			for(int k = 0; k < 2; ++k) {
				const float w  = w1[0][i] * w1[1][j] * w1[2][k];
				const float4 v = f.table[((size_t) (cid[0] + i) * (size_t) f.dims[1] + (size_t) (cid[1] + j)) * (size_t) f.dims[2] + (size_t) (cid[2] + k)];
				sdis += w * v.x;
				n[0] += w * v.y;
				n[1] += w * v.z;
				n[2] += w * v.w;
			}
	const float nn = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
	MPM_VOLUME_UNROLL
	for(int d = 0; d < 3; ++d) n[d] /= nn;
	if(f.inside_out) {
		sdis = -sdis;
	MPM_VOLUME_UNROLL
		for(int d = 0; d < 3; ++d) n[d] = -n[d];
	}
}

#if defined(MPM_VOLUME_HAS_RESPONSE)
// One volume acting on one domain point X (a node: (float) node * dx): shape_resolve's statements around volume_query.
MPM_DEV void volume_resolve(const CollisionObject& o, const CollisionPose& p, const Volume& f, const float (&X)[3], float (&vel)[3]) {
	MPM_VOLUME_NO_CONTRACT
	float xmt[3], x[3], n[3], sdis;
	collision_material_point(o, p, X, xmt, x);
	volume_query(f, x, sdis, n);
	if(!(sdis <= 0.f)) return;
	collision_respond(o, p, xmt, x, n, vel);
}
#endif

// Host side (plain C++): the box of a mesh install with dims == {0, 0, 0}, from the mesh's bounding box [mn, mx] in float64 on the float32
// vertices and the float32 spacing:  origin_d = mn_d - pad * spacing;  dims_d = ceil((mx_d - mn_d) / spacing) + 2 * pad + 1;  the origin is then
// stored as float32.  Returns false where a dims entry leaves 2 .. kVolumeMaxSamples or their product kVolumeMaxTable (nv >= 1, finite vertices).
inline bool volume_autosize(const float* verts, size_t nv, float spacing, int pad, float (&origin)[3], int (&dims)[3]) {
	const double sp = (double) spacing;
	long long total = 1;
	for(int d = 0; d < 3; ++d) {
		double mn = (double) verts[d], mx = (double) verts[d];
		for(size_t i = 1; i < nv; ++i) {
			const double v = (double) verts[3 * i + d];
			mn			   = v < mn ? v : mn;
			mx			   = v > mx ? v : mx;
		}
		origin[d]	   = (float) (mn - (double) pad * sp);
		const double n = ceil((mx - mn) / sp) + 2. * (double) pad + 1.;
		if(!(n >= (double) kVolumeMinSamples && n <= (double) kVolumeMaxSamples)) return false;
		dims[d] = (int) n;
		total *= dims[d];
	}
	return total <= kVolumeMaxTable;
}

}// namespace mpm
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif

#if defined(__HIPCC__)
// Parts 2 and 3 are mpm_collision_mesh.hpp's: collision_mesh_table_kernel fills a table from a closed mesh - it is the kernel of the domain-wide
// field, given the box's origin, spacing and dimensions and inside_out 0 (a volume is flipped at the query); the argument, the partial tiles
// and the budget are written there (tests/test_collision_volume_isa.py) - and collision_table_box_kernel reads a box of a table back.
#include "mpm_collision_mesh.hpp"
#endif// __HIPCC__
