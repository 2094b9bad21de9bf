// mpm_force_field.hpp — force fields on the grid: uniform acceleration, point attractor, vortex, drag (an extension, the reference knows one
// scalar gravity only).
//
// Up to kMaxForceFields fields act on the {mass, momentum} of every grid node with mass, BEFORE the grid update turns momenta into velocities
// (walls, gravity, colliders): force_cell is one node through the slots in order 0..3, each acting on the momentum the previous one left;
// grid_force_kernel is the pass over the grid that launch_grid_update enqueues ahead of the update whenever a slot is occupied, and the
// read-only load readouts (mpm_collider_loads.hpp) call force_cell on their register copy of a cell.  The mass is never written.
// A field has an optional region, a CollisionShape in domain coordinates without pose or clock, evaluated by shape_query at the node
// position X = (float) node * dx; the weight w is 1 where region.kind == 0, else from the signed distance sdis:
//   feather == 0:  w = sdis <= 0 ? 1 : 0          feather > 0:  t = (0 - sdis) / feather;  w = sdis < 0 ? (t < 1 ? t : 1) : 0
// (a NaN sdis gives 0).  A node with w == 0 is skipped by that slot: its words keep their bits.
// Builds on x86 like mpm_collision_shapes.hpp (tools/hostcheck/check_forces.cpp): MPM_DEV only, contraction off, plain IEEE + - * / and sqrtf.
// tests/force_field_model.py restates every statement below with numpy float32.
#pragma once
#include "mpm_collision_shapes.hpp"
#if defined(__HIPCC__)
#include "mpm_kernels.hpp"// (GridCfg, for the kernels at the end)
#endif

namespace mpm {

enum { kForceUniform = 1, kForcePoint = 2, kForceVortex = 3, kForceDrag = 4 };// MPM_FORCE_*
constexpr int kMaxForceFields = 4;											  // MPM_MAX_FORCE_FIELDS

struct ForceSlot {// mpm_force_field as installed (a vortex's axis in vec and a half-space region's normal have unit length here)
	int kind;	  // 0: an empty slot
	int falloff;  // POINT: the power of the distance the pull falls off with, 0..2
	float vec[3]; // UNIFORM: the acceleration; VORTEX: the unit axis; DRAG: the target velocity
	float centre[3];
	float strength;// POINT: the pull (negative: repels); DRAG: the rate k
	float swirl, pull, lift;
	float soft;
	float feather;
	CollisionShape region;// kind 0: everywhere
};
struct ForceArgs {
	int count;// slots [0, count) are looked at; 0: no field
	ForceSlot slot[kMaxForceFields];
};

// The weight of a slot at X.
MPM_DEV float force_weight(const ForceSlot& f, const float (&X)[3]) {
#pragma clang fp contract(off)
	if(f.region.kind == 0) return 1.f;
	float sdis, n[3];
	shape_query(f.region, X, sdis, n);
	if(f.feather > 0.f) {
		const float t = (0.f - sdis) / f.feather;
		return sdis < 0.f ? (t < 1.f ? t : 1.f) : 0.f;
	}
	return sdis <= 0.f ? 1.f : 0.f;
}

// One node: v = {mass, momentum}, the momentum in place.  Statement order per slot of kind != 0 with w != 0 (m = v.x, p = momentum):
//   UNIFORM  a = vec
//   POINT    r_i = centre_i - X_i;  d2 = ((r_0 r_0 + r_1 r_1) + r_2 r_2) + soft soft;  d = sqrtf(d2)
//            falloff 0: q_i = r_i / d;   1: q_i = r_i / d2;   2: q_i = r_i / (d2 d);   a_i = d == 0 ? +0 : strength q_i
//   VORTEX   r_i = X_i - centre_i;  h = (r_0 n_0 + r_1 n_1) + r_2 n_2;  rp_i = r_i - h n_i   (n = vec)
//            c_0 = n_1 rp_2 - n_2 rp_1;  c_1 = n_2 rp_0 - n_0 rp_2;  c_2 = n_0 rp_1 - n_1 rp_0
//            a_i = (swirl c_i - pull rp_i) + lift n_i
//   these three:  g = w dt;  p_i = p_i + m (a_i g)
//   DRAG     s = w (strength dt);  p_i = (p_i + s (m vec_i)) / (1 + s)      (implicit Euler of dv/dt = -w k (v - vec))
// The kinds and the count are the same for every node of a launch (scalar branches); the slot loop is a real loop over the kernel-argument
// segment (unrolled it held four slots in scalar registers at once and spilled them: DESIGN.md 3.1).
MPM_DEV void force_cell(const ForceArgs& fa, const float (&X)[3], float dt, float4& v) {
#pragma clang fp contract(off)
#pragma nounroll
	for(int s = 0; s < fa.count; ++s) {
		const ForceSlot& f = fa.slot[s];
		if(f.kind == 0) continue;
		const float w = force_weight(f, X);
		if(w == 0.f) continue;
		const float m = v.x;
		if(f.kind == kForceDrag) {
			const float k = w * (f.strength * dt);
			v.y			  = (v.y + k * (m * f.vec[0])) / (1.f + k);
			v.z			  = (v.z + k * (m * f.vec[1])) / (1.f + k);
			v.w			  = (v.w + k * (m * f.vec[2])) / (1.f + k);
			continue;
		}
		float a[3];
		if(f.kind == kForceUniform) {
			a[0] = f.vec[0], a[1] = f.vec[1], a[2] = f.vec[2];
		} else if(f.kind == kForcePoint) {
			const float r[3] = {f.centre[0] - X[0], f.centre[1] - X[1], f.centre[2] - X[2]};
			const float d2	 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + f.soft * f.soft;
			const float d	 = sqrtf(d2);
			const float den	 = f.falloff == 0 ? d : (f.falloff == 1 ? d2 : d2 * d);
			const bool zero	 = d == 0.f;
#pragma unroll
			for(int i = 0; i < 3; ++i) a[i] = zero ? 0.f : f.strength * (r[i] / den);
		} else if(f.kind == kForceVortex) {
			const float(&n)[3] = f.vec;
			const float r[3]   = {X[0] - f.centre[0], X[1] - f.centre[1], X[2] - f.centre[2]};
			const float h	   = r[0] * n[0] + r[1] * n[1] + r[2] * n[2];
			const float rp[3]  = {r[0] - h * n[0], r[1] - h * n[1], r[2] - h * n[2]};
			const float c[3]   = {n[1] * rp[2] - n[2] * rp[1], n[2] * rp[0] - n[0] * rp[2], n[0] * rp[1] - n[1] * rp[0]};
#pragma unroll
			for(int i = 0; i < 3; ++i) a[i] = f.swirl * c[i] - f.pull * rp[i] + f.lift * n[i];
		} else
			continue;// (an unknown kind does nothing; mpm_set_force_field refuses it)
		const float g = w * dt;
		v.y			  = v.y + m * (a[0] * g);
		v.z			  = v.z + m * (a[1] * g);
		v.w			  = v.w + m * (a[2] * g);
	}
}

// The node position the collider slots see (grid_cell's node mapping).
MPM_DEV void force_node_position(int kx, int ky, int kz, int cell, float dx, float (&X)[3]) {
	X[0] = (float) (kx * 4 + (cell >> 4)) * dx;
	X[1] = (float) (ky * 4 + ((cell >> 2) & 3)) * dx;
	X[2] = (float) (kz * 4 + (cell & 3)) * dx;
}

#if defined(__HIPCC__)
// The pre-pass, in the stand-alone frame's shape: one wave per grid block, lane = cell, grid-stride over the device's block count, channel-planar.
// A cell with mass loads its momentum, runs through force_cell and stores the momentum; the mass word and cells without mass are not written.
__global__ __launch_bounds__(256) void grid_force_kernel(GridCfg cfg, const int* __restrict__ nbc_ptr, float* __restrict__ grid, const int* __restrict__ keys, float dt, ForceArgs fa) {
	const int cell	  = threadIdx.x & 63;
	const int nblocks = min(*nbc_ptr, cfg.cap);
	for(int blockno = (blockIdx.x * 256 + threadIdx.x) >> 6; blockno < nblocks; blockno += gridDim.x * 4) {
		const int kx = keys[3 * blockno], ky = keys[3 * blockno + 1], kz = keys[3 * blockno + 2];
		float* g	 = grid + (size_t) blockno * 256 + cell;
		float4 v	 = {g[0], 0.f, 0.f, 0.f};
		if(v.x > 0.0f) {
			v.y = g[64];
			v.z = g[128];
			v.w = g[192];
			float X[3];
			force_node_position(kx, ky, kz, cell, cfg.dx, X);
			force_cell(fa, X, dt, v);
			g[64]  = v.y;
			g[128] = v.z;
			g[192] = v.w;
		}
	}
}
// mpm_test_force_field: force_cell at arbitrary points with given {m, p}
__global__ void test_force_field_kernel(ForceArgs fa, float dt, size_t n, const float* __restrict__ xyz, const float* __restrict__ mp4, float* __restrict__ out4) {
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const float X[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
	float4 v		 = {mp4[4 * i], mp4[4 * i + 1], mp4[4 * i + 2], mp4[4 * i + 3]};
	force_cell(fa, X, dt, v);
	out4[4 * i] = v.x, out4[4 * i + 1] = v.y, out4[4 * i + 2] = v.z, out4[4 * i + 3] = v.w;
}
#endif// __HIPCC__

}// namespace mpm
