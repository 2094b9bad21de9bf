// mpm_collider_loads.hpp — what the next grid update will do to the material at every collider: impulses, and from them force and torque
// (an extension, the reference has no load output).
//
// A read-only readout of the grid while it holds the mass and momentum of the last P2G.  load_cell - THE walk of one cell through the colliders
// with a row per collider, for every argument type with_collider hands out, bodies included - runs the grid update's own statements:
// grid_cell_walls_gravity, then collision_resolve and per slot slot_resolve, the very device functions grid_cell inlines, in grid_cell's order - and
// hands the velocity change of every collider to a sink, row by row:
//   row 0 the level-set object, rows 1..4 slots 0..3, row 5 the domain walls (gravity belongs to no row).
// Per node and row the impulse on the MATERIAL is j = (double) m * (double) dv (exact: 24 x 24 bits), the load on the collider is -j, its
// torque about the row's pivot r x (-j) with r = (double) X - pivot, X = (float) node * dx - float64 products without contraction, so a
// float32 / float64 model has the per-node terms bit for bit.  A node is touched where any component of dv is non-zero or NaN.
//
// The sums: no floating-point atomics anywhere.  loads_frame - THE frame, behind collider_loads_kernel and, storing the velocities as well, behind
// grid_update_body_kernel (mpm_rigid_body.hpp) - runs in kLoadGroups workgroups - a CONSTANT, so which blocks a wave walks, and with it the order of
// every addition, depends on the block count alone and not on a launch sized by a host estimate - and after each collider asks the whole wave
// whether any lane was touched (one ballot; most blocks touch nothing and go on).  A touched wave reduces its 8 sums by a butterfly of shuffles
// (commutative additions: every lane ends with the same bits) and lane 0 adds them into the wave's own row of LDS partials; the workgroup adds
// its four waves in order and writes [row][8] to a scratch array; load_totals, one workgroup, adds the workgroups' partials in index order -
// collider_loads_reduce_kernel stores the totals or adds them to the gauge's accumulators, body_step_kernel steps the bodies with them.  The same
// state gives the same bits on every call.  float64 lives in the reduction alone: the per-node collider code is the grid update's float32, and a
// lane holds eight doubles at most (no private array indexed at run time, no scratch).
#pragma once
#include "mpm_kernels.hpp"
#include "mpm_force_field.hpp"

namespace mpm {

constexpr int kLoadRows	   = 6;// MPM_LOAD_ROWS
constexpr int kLoadSums	   = 8;// {n_touched, Jx, Jy, Jz, Lx, Ly, Lz, m_touched}
constexpr int kLoadWallRow = 5;
constexpr int kLoadGroups  = 1024;// workgroups of loads_frame, four waves each (a constant: see above)
constexpr int kLoadReduceThreads = 1024;// 16 waves: wave w adds the partials of workgroups [64 w, 64 w + 64) in order
// the gauge's accumulators: [kLoadRows][kLoadSums] totals, then the elapsed time, then the number of updates (as a double's worth of bits: a long long)
constexpr int kLoadAccDoubles = kLoadRows * kLoadSums + 2;

struct LoadPivots {
	double p[kLoadRows][3];
};
// The pivot of a row: the one that travels by value.  (An argument type that carries body state overloads this: mpm_rigid_body.hpp.)
template<class Collider>
MPM_DEV void row_pivot(const Collider&, const LoadPivots& piv, int row, double (&p)[3]) {
	p[0] = piv.p[row][0], p[1] = piv.p[row][1], p[2] = piv.p[row][2];
}

// One cell through the grid update's statements.  Every lane of the wave calls this (the sinks vote and shuffle): a lane without mass
// (`active` false) computes nothing and reports no change.  sink(row, touched, node, dv, vel) is called at wave-uniform places: once for the
// walls, once for the level-set object if installed, once per slot in use - vel the velocity that collider left.
template<class Collider, class Sink>
MPM_DEV void load_cell(const GridCfg& cfg, const Collider& a, int kx, int ky, int kz, int cell, float dt, bool active, const float4& v, Sink&& sink) {
#pragma clang fp contract(off)
	float vel[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
	int node[3]	 = {kx * 4 + (cell >> 4), ky * 4 + ((cell >> 2) & 3), kz * 4 + (cell & 3)};
	if(active) grid_cell_walls_gravity(cfg, kx, ky, kz, cell, dt, v, vel, node, &dv);// (with the walls' row)
	auto touched = [&]() { return active && !(dv[0] == 0.0f && dv[1] == 0.0f && dv[2] == 0.0f); };// (a NaN compares unequal: touched)
	sink(kLoadWallRow, touched(), node, dv, vel);
	auto row = [&](int r, auto&& resolve) {
		const float before[3] = {vel[0], vel[1], vel[2]};
		if(active) resolve();
#pragma unroll
		for(int d = 0; d < 3; ++d) dv[d] = vel[d] - before[d];
		sink(r, touched(), node, dv, vel);
	};
	const float bc_lo = (float) cfg.boundary * cfg.dx * 4.f, bc_hi = (float) (cfg.G - cfg.boundary) * 4.f * cfg.dx;
	if constexpr(std::is_same_v<Collider, NoCollision>) {
		(void) a;
	} else if constexpr(std::is_same_v<Collider, CollisionArgs>) {
		row(0, [&]() { collision_resolve(a.obj, a.pose, node, cfg.dx, cfg.G * 4, bc_lo, bc_hi, vel); });
	} else {// (a type with slots: one that shape_args and slot_resolve take)
		const ShapeArgs& col = shape_args(a);
		// The level-set object's 40 words are the same for every block, and left alone the compiler loads them once, ahead of the walk over the blocks,
		// where they sit in scalar registers beside the slot the loop is at - more than there are, so some were spilled.  Read through an index the
		// compiler cannot see through (a scalar 0, made anew per cell) they are loaded where they are used and dead behind it.
		int here = 0;
		asm volatile("" : "+s"(here));
		const CollisionArgs& field = (&col.field)[here];
		if(col.has_field) row(0, [&]() { collision_resolve(field.obj, field.pose, node, cfg.dx, cfg.G * 4, bc_lo, bc_hi, vel); });
		const float X[3] = {(float) node[0] * cfg.dx, (float) node[1] * cfg.dx, (float) node[2] * cfg.dx};
#pragma nounroll
		for(int s = 0; s < col.count; ++s) {
			if(col.slot[s].shape.kind == 0) continue;// (an empty slot has no row)
			row(1 + s, [&]() { slot_resolve(a, s, X, vel); });// (the slot's kind wave-uniform)
		}
	}
}

// The walk over the grid that the readouts and the body update share: one wave per grid block of the device's count, lane = cell;
// per_cell(kx, ky, kz, g, v, active) with g the cell's mass word (the momenta 64, 128, 192 floats on), v = {mass, momentum} and `active` whether the
// cell has mass (the momenta of a cell without are not read).
template<class Grid, class PerCell>
MPM_DEV void for_each_cell(const GridCfg& cfg, const int* __restrict__ nbc_ptr, Grid* grid, const int* __restrict__ keys, PerCell&& per_cell) {
	const int cell	  = threadIdx.x & 63;
	const int nblocks = min(*nbc_ptr, cfg.cap);
	for(int blockno = (blockIdx.x * 256 + threadIdx.x) >> 6; blockno < nblocks; blockno += gridDim.x * 4) {
		const int kx = keys[3 * blockno], ky = keys[3 * blockno + 1], kz = keys[3 * blockno + 2];
		Grid* g		 = grid + (size_t) blockno * 256 + cell;
		float4 v	 = {g[0], 0.f, 0.f, 0.f};
		const bool active = v.x > 0.0f;
		if(active) {
			v.y = g[64];
			v.z = g[128];
			v.w = g[192];
		}
		per_cell(kx, ky, kz, g, v, active);
	}
}

MPM_DEV double load_wave_sum(double x) {
#pragma unroll
	for(int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
	return x;
}

// The totals' first stage, a workgroup of 256: workgroup g writes its [kLoadRows][kLoadSums] partial sums to partials + g * kLoadRows * kLoadSums.
// With APPLY the pass is the grid update as well: per massed cell the velocity the last collider left is stored and the doubled |v|^2 folded into
// the max slots.  before(kx, ky, kz, cell, v, active): what happens to the register copy of a cell ahead of the walk (forced_cell for the readouts, which
// see the momenta the force fields' pass will leave; nothing for the applying pass, which runs behind that pass).
struct NoFields {
	MPM_DEV void operator()(int, int, int, int, float4&, bool) const {}
};
// The force fields on the register copy of a massed cell, behind one wave-uniform branch (mpm_force_field.hpp).
struct ForcedCell {
	const GridCfg& cfg;
	const ForceArgs& forces;
	float dt;
	MPM_DEV void operator()(int kx, int ky, int kz, int cell, float4& v, bool active) const {
		if(forces.count > 0) {
			float X[3];
			force_node_position(kx, ky, kz, cell, cfg.dx, X);
			if(active) force_cell(forces, X, dt, v);
		}
	}
};
template<bool APPLY, class Collider, class Grid, class Before = NoFields>
MPM_DEV void loads_frame(const GridCfg& cfg, const int* __restrict__ nbc_ptr, Grid* grid, const int* __restrict__ keys, float dt, const Collider& col, const LoadPivots& piv, double* __restrict__ partials, unsigned* __restrict__ max_vel_bits, const Before& before = NoFields {}) {
#pragma clang fp contract(off)
	__shared__ double s_part[4][kLoadRows][kLoadSums];
	const int cell = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for(int i = threadIdx.x; i < 4 * kLoadRows * kLoadSums; i += 256) (&s_part[0][0][0])[i] = 0.0;
	__syncthreads();
	float vel_sqr = 0.f;
	for_each_cell(cfg, nbc_ptr, grid, keys, [&](int kx, int ky, int kz, Grid* g, float4& v, bool active) {
		float fv[3] = {0.f, 0.f, 0.f};// the velocity the last collider left
		before(kx, ky, kz, cell, v, active);
		load_cell(cfg, col, kx, ky, kz, cell, dt, active, v, [&](int row, bool touched, const int (&node)[3], const float (&dv)[3], const float (&vel)[3]) {
#pragma clang fp contract(off)
			if constexpr(APPLY) fv[0] = vel[0], fv[1] = vel[1], fv[2] = vel[2];
			if(!__any(touched)) return;// (wave-uniform: most blocks touch nothing)
			// the load on the collider: -j, j = m dv in float64 (exact); its torque about the pivot: r x (-j)
			double p[3];
			row_pivot(col, piv, row, p);
			const double m	= (double) v.x;
			const double j0 = touched ? -(m * (double) dv[0]) : 0.0, j1 = touched ? -(m * (double) dv[1]) : 0.0, j2 = touched ? -(m * (double) dv[2]) : 0.0;
			const double r0 = (double) ((float) node[0] * cfg.dx) - p[0], r1 = (double) ((float) node[1] * cfg.dx) - p[1], r2 = (double) ((float) node[2] * cfg.dx) - p[2];
			const double l0 = touched ? r1 * j2 - r2 * j1 : 0.0, l1 = touched ? r2 * j0 - r0 * j2 : 0.0, l2 = touched ? r0 * j1 - r1 * j0 : 0.0;
			const double n = (double) __popcll(__ballot(touched));
			const double s1 = load_wave_sum(j0), s2 = load_wave_sum(j1), s3 = load_wave_sum(j2);
			const double s4 = load_wave_sum(l0), s5 = load_wave_sum(l1), s6 = load_wave_sum(l2);
			const double s7 = load_wave_sum(touched ? m : 0.0);
			if(cell == 0) {// (the wave's own row: no other wave writes it)
				double* q = s_part[wave][row];
				q[0] += n, q[1] += s1, q[2] += s2, q[3] += s3, q[4] += s4, q[5] += s5, q[6] += s6, q[7] += s7;
			}
		});
		if constexpr(APPLY) {
			if(active) {
				vel_sqr = fmaxf(vel_sqr, grid_cell_store_doubled_q(fv, v));
				g[64]	= v.y;
				g[128]	= v.z;
				g[192]	= v.w;
			}
		}
	});
	if constexpr(APPLY) wave_max_vel(vel_sqr, max_vel_bits);
	__syncthreads();
	if(threadIdx.x < kLoadRows * kLoadSums) {
		const double* p = &s_part[0][0][0] + threadIdx.x;
		partials[(size_t) blockIdx.x * (kLoadRows * kLoadSums) + threadIdx.x] = ((p[0] + p[kLoadRows * kLoadSums]) + p[2 * kLoadRows * kLoadSums]) + p[3 * kLoadRows * kLoadSums];
	}
}
// The readout: the frame without the stores.
template<class Collider>
__global__ __launch_bounds__(256) void collider_loads_kernel(GridCfg cfg, const int* __restrict__ nbc_ptr, const float* __restrict__ grid, const int* __restrict__ keys, float dt, Collider col, LoadPivots piv, double* __restrict__ partials, ForceArgs forces) {
	loads_frame<false>(cfg, nbc_ptr, grid, keys, dt, col, piv, partials, nullptr, ForcedCell {cfg, forces, dt});
}

// The second stage, one workgroup of kLoadReduceThreads: the partials of `groups` workgroups in index order - wave w adds its 64 workgroups one
// after the other, then entry e adds the 16 waves one after the other.  Returns entry e's total to thread e < kLoadRows * kLoadSums (0 to the rest).
MPM_DEV double load_totals(const double* __restrict__ partials, int groups) {
#pragma clang fp contract(off)
	constexpr int E = kLoadRows * kLoadSums, W = kLoadReduceThreads / 64;
	__shared__ double s_sum[W][E];
	const int e = threadIdx.x & 63, w = threadIdx.x >> 6;
	if(e < E) {
		const int per = (groups + W - 1) / W;
		double sum	  = 0.0;
		for(int g = w * per; g < min(groups, (w + 1) * per); ++g) sum += partials[(size_t) g * E + e];
		s_sum[w][e] = sum;
	}
	__syncthreads();
	double total = 0.0;
	if(threadIdx.x < E) {
		total = s_sum[0][threadIdx.x];
#pragma unroll
		for(int i = 1; i < W; ++i) total += s_sum[i][threadIdx.x];
	}
	return total;
}
// accumulate 0: out[e] = total.  accumulate 1 (the gauge): out[e] += total, out[48] += dt, and the long long behind it counts the call.
__global__ __launch_bounds__(kLoadReduceThreads) void collider_loads_reduce_kernel(const double* __restrict__ partials, int groups, double* __restrict__ out, int accumulate, double dt) {
#pragma clang fp contract(off)
	constexpr int E	   = kLoadRows * kLoadSums;
	const double total = load_totals(partials, groups);
	if(threadIdx.x < E) out[threadIdx.x] = accumulate ? out[threadIdx.x] + total : total;
	if(accumulate && threadIdx.x == E) {
		out[E] += dt;
		reinterpret_cast<long long*>(out)[E + 1] += 1;
	}
}

// The contact map: one record per touched (node, row), appended through a wave-aggregated integer counter (one atomic per touched wave and
// row); records beyond `capacity` are counted and not written.  node_row4: int32 {i, j, k, row}; rec8: float32 {m, dv[3], v_after[3], 0}.
template<class Collider>
__global__ __launch_bounds__(256) void collider_contacts_kernel(GridCfg cfg, const int* __restrict__ nbc_ptr, const float* __restrict__ grid, const int* __restrict__ keys, float dt, Collider col, unsigned long long capacity, int* __restrict__ node_row4, float* __restrict__ rec8, unsigned long long* counter, ForceArgs forces) {
	const int cell = threadIdx.x & 63;
	for_each_cell(cfg, nbc_ptr, grid, keys, [&](int kx, int ky, int kz, const float*, float4& v, bool active) {
		ForcedCell {cfg, forces, dt}(kx, ky, kz, cell, v, active);
		load_cell(cfg, col, kx, ky, kz, cell, dt, active, v, [&](int row, bool touched, const int (&node)[3], const float (&dv)[3], const float (&vel)[3]) {
			const unsigned long long mask = __ballot(touched);
			if(!mask) return;
			unsigned long long first = 0;
			if(cell == 0) first = atomicAdd(counter, (unsigned long long) __popcll(mask));
			first = __shfl(first, 0);
			const unsigned long long at = first + (unsigned long long) __popcll(mask & ((1ull << cell) - 1ull));
			if(touched && at < capacity) {
				int4* nr = reinterpret_cast<int4*>(node_row4) + at;
				*nr		 = int4 {node[0], node[1], node[2], row};
				float4* r = reinterpret_cast<float4*>(rec8) + 2 * at;
				r[0]	  = float4 {v.x, dv[0], dv[1], dv[2]};
				r[1]	  = float4 {vel[0], vel[1], vel[2], 0.f};
			}
		});
	});
}

}// namespace mpm
