// mpm_particle_remove.hpp — particle removal (mpm_count_particles_in, mpm_remove_particles): the kernels of the re-lay that takes
// particles out of a context that has been set up - emission's mirror image (mpm_particle_emit.hpp).  The substep kernels know nothing of it: the
// live particles are walked once to count the selected ones, walked again to split them into the survivors' staging columns (EmitStage) and a
// removed list, mpm_initial_setup's own kernels lay the survivors out in a fresh partition, the old grid is carried over by block key, and every
// node a removed particle's stencil reaches is rescaled: it takes the survivors' set-up mass m' and keeps its velocity, p' = p (m' / m).
// A particle is selected when shape_query (mpm_collision_shapes.hpp) of any region gives sdis <= 0 at its float32 world position - the position
// the readouts return - or when its id's bit is set in the bitmap built from the caller's id list.
//
// Group segments: sink_bitmap_kernel 0 B, sink_count_kernel 0 B, sink_gather_kernel 0 B, sink_mark_kernel 0 B, sink_carry_grid_kernel 0 B,
// sink_rescale_grid_kernel 0 B.
#pragma once
#include "mpm_collision_shapes.hpp"
#include "mpm_kernels.hpp"
#include "mpm_particle_emit.hpp"
#include "mpm_readout.hpp"

namespace mpm {

constexpr int kMaxSinkRegions = 8;// MPM_MAX_SINK_REGIONS
enum { kSinkCarryMiss = 1 };

// What selects a particle, by value: the regions as make_shape_slot leaves them (a half-space's normal has unit length), and the id bitmap of
// the one model the launch walks (null: no ids; nbits = the model's n).
struct SinkSelect {
	CollisionShape region[kMaxSinkRegions];
	int nregions;
	unsigned nbits;
	const unsigned* bitmap;
};

// One bit per id of the caller's list (the host has checked 0 <= id < n; duplicates set a bit twice).
__global__ __launch_bounds__(256) void sink_bitmap_kernel(size_t n, const int* __restrict__ ids, unsigned* bitmap) {
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n) atomicOr(&bitmap[ids[i] >> 5], 1u << (ids[i] & 31));
}

// The predicate on one live particle: x in world units, id from the side array (-1: untracked).  The region's kind is the same for every lane
// (a scalar branch per region); a NaN sdis selects nothing.
__device__ __forceinline__ bool sink_selected(const SinkSelect& q, const float (&x)[3], int id) {
	bool hit = false;
	for(int r = 0; r < q.nregions; ++r) {
		float sdis, n[3];
		shape_query(q.region[r], x, sdis, n);
		hit = hit || sdis <= 0.f;
	}
	if(q.bitmap && (unsigned) id < q.nbits) hit = hit || ((q.bitmap[id >> 5] >> (id & 31)) & 1u) != 0u;
	return hit;
}

// The walk both passes share: the particle of list slot pidib of block b, its world position and its id.  Returns the record.
__device__ __forceinline__ const float* sink_fetch(const ReadoutArgs& a, const int* list, int pidib, int kx, int ky, int kz, float4& r0, float (&x)[3], const float** row, size_t* sslot, int& id) {
	float p[3];
	const float* src = readout_position(a, list[pidib], kx, ky, kz, p, row, sslot);
	r0				 = *reinterpret_cast<const float4*>(src);
	x[0] = r0.x * a.cfg.dx, x[1] = r0.y * a.cfg.dx, x[2] = r0.z * a.cfg.dx;
	id = a.ids ? a.ids[*sslot] : -1;
	return src;
}

// readout_kernel's walk (readout_live, readout_position, a 16-byte record load) with the predicate alone: *count (zeroed by the caller) ends at
// the number of selected live particles of the model.  One workgroup per particle block; a wave sums its ballots' popcounts over its trips and
// issues one atomic.  Nothing else is written.
__global__ __launch_bounds__(kReadoutThreads) void sink_count_kernel(ReadoutArgs a, SinkSelect q, unsigned long long* count) {
	const int b = blockIdx.x;
	const int n = a.size[b];
	if(n == 0) return;
	const int kx = a.cur_keys[3 * b], ky = a.cur_keys[3 * b + 1], kz = a.cur_keys[3 * b + 2];
	const int* list = a.list + (size_t) a.row_of[b] * a.cfg.ppb;
	unsigned found	= 0;
	for(int pidib = threadIdx.x; pidib < ((n + 63) & ~63); pidib += kReadoutThreads) {
		bool sel = false;
		if(readout_live(n, pidib, a.dense)) {
			float4 r0;
			float x[3];
			const float* row = nullptr;
			size_t sslot	 = 0;
			int id;
			sink_fetch(a, list, pidib, kx, ky, kz, r0, x, &row, &sslot, id);
			sel = sink_selected(q, x, id);
		}
		found += (unsigned) __popcll(__ballot(sel));
	}
	if((threadIdx.x & 63) == 0 && found) atomicAdd(count, (unsigned long long) found);
}

// Where the gather puts the selected particles: slot o of the three columns, shared by all models of a call (*counter runs across the launches).
struct SinkRemoved {
	float* xyz;	 // 3 per slot, world units
	int* ids;	 // the particle's id, -1 in an untracked context
	int* model;	 // the model it belonged to
	unsigned long long capacity;
	unsigned long long* counter;
};

// emit_gather_kernel's one-pass column gather, split by the predicate: a survivor's position, state, log Jp and id go to one slot of the staging
// columns, a selected particle's position, id and model to one slot of the removed list.  The survivors of a block are not known up front, so a
// wave takes the slots of each trip with one global atomic per list (*kept, zeroed by the caller, ends at the number of survivors).  The
// record is fetched with 16-byte loads, as there.
__global__ __launch_bounds__(kReadoutThreads) void sink_gather_kernel(ReadoutArgs a, SinkSelect q, int model, EmitStage out, unsigned long long capacity, unsigned long long* kept, SinkRemoved gone) {
	const int b = blockIdx.x;
	const int n = a.size[b];
	if(n == 0) return;
	const int kx = a.cur_keys[3 * b], ky = a.cur_keys[3 * b + 1], kz = a.cur_keys[3 * b + 2];
	const int* list	 = a.list + (size_t) a.row_of[b] * a.cfg.ppb;
	const bool fluid = a.nch == 4;
	const int lane	 = threadIdx.x & 63;
	for(int pidib = threadIdx.x; pidib < ((n + 63) & ~63); pidib += kReadoutThreads) {
		const bool live = readout_live(n, pidib, a.dense);
		if(__ballot(live) == 0ull) continue;
		float4 r0		 = make_float4(0.f, 0.f, 0.f, 0.f);
		float x[3]		 = {0.f, 0.f, 0.f};
		const float* row = nullptr;
		const float* src = nullptr;
		size_t sslot	 = 0;
		int id			 = -1;
		bool sel		 = false;
		if(live) {
			src = sink_fetch(a, list, pidib, kx, ky, kz, r0, x, &row, &sslot, id);
			sel = sink_selected(q, x, id);
		}
		const unsigned long long gone_mask = __ballot(live && sel), keep_mask = __ballot(live && !sel);
		unsigned long long first_keep = 0, first_gone = 0;
		if(lane == 0) {
			if(keep_mask) first_keep = atomicAdd(kept, (unsigned long long) __popcll(keep_mask));
			if(gone_mask) first_gone = atomicAdd(gone.counter, (unsigned long long) __popcll(gone_mask));
		}
		first_keep = __shfl(first_keep, 0);
		first_gone = __shfl(first_gone, 0);
		if(!live) continue;
		const unsigned long long below = (1ull << lane) - 1ull;
		if(sel) {
			const unsigned long long o = first_gone + (unsigned long long) __popcll(gone_mask & below);
			if(o >= gone.capacity) continue;
			gone.xyz[3 * o] = x[0], gone.xyz[3 * o + 1] = x[1], gone.xyz[3 * o + 2] = x[2];
			gone.ids[o]	  = id;
			gone.model[o] = model;
			continue;
		}
		const unsigned long long o = first_keep + (unsigned long long) __popcll(keep_mask & below);
		if(o >= capacity) continue;
		out.xyz[3 * o] = x[0], out.xyz[3 * o + 1] = x[1], out.xyz[3 * o + 2] = x[2];
		float s[6] = {r0.w, 0.f, 0.f, 0.f, 0.f, 0.f};
		if(!fluid) {
			const float4 r1 = *reinterpret_cast<const float4*>(src + 4);
			s[1] = r1.x, s[2] = r1.y, s[3] = r1.z, s[4] = r1.w, s[5] = row[0];
		}
		emit_store_state(out.state9 + 9 * o, fluid, s);
		out.logjp[o] = a.nch - rec_floats(a.nch) == 2 ? row[1] : 0.f;
		if(out.ids) out.ids[o] = id;
	}
}

// Per removed particle: the in-domain nodes of its 27-node stencil (base = node - 1, as the rasteriser and particle_block_key form it), marked
// in the numbering of `table` - one 64-bit mask per grid block, cell 16 x + 4 y + z is the bit.  A node whose block the table does not hold
// (beyond an upper face) has no cell to mark.
__global__ __launch_bounds__(256) void sink_mark_kernel(GridCfg cfg, size_t n, const float* __restrict__ xyz, const int* __restrict__ table, int nbc, unsigned long long* marks) {
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const int bx = node_index(xyz[3 * i], cfg.dx_inv) - 1, by = node_index(xyz[3 * i + 1], cfg.dx_inv) - 1, bz = node_index(xyz[3 * i + 2], cfg.dx_inv) - 1;
#pragma unroll 1
	for(int s = 0; s < 27; ++s) {
		const int x = bx + s / 9, y = by + (s / 3) % 3, z = bz + s % 3;
		if((x | y | z) < 0) continue;
		const int bno = table_query(cfg, table, x >> 2, y >> 2, z >> 2);
		if(bno < 0 || bno >= nbc) continue;
		atomicOr(&marks[bno], 1ull << (((x & 3) << 4) | ((y & 3) << 2) | (z & 3)));
	}
}

// emit_carry_grid_kernel for a partition that shrank: an old block the new table does not hold is dropped - every cell of it that holds mass
// must then be marked (reached by a removed particle: nobody else stands there), else the flag is raised.  A block that is carried takes its
// marks along under its new number (new_marks zeroed by the caller).  One wave per old block, one 16-byte load and store per lane.
__global__ __launch_bounds__(256) void sink_carry_grid_kernel(GridCfg cfg, int old_nbc, int new_nbc, const int* __restrict__ old_keys, const float* __restrict__ old_grid, const unsigned long long* __restrict__ old_marks, const int* __restrict__ new_table, float* __restrict__ grid, unsigned long long* __restrict__ new_marks, int* flag) {
	const int lane = threadIdx.x & 63;
	for(int ob = blockIdx.x * 4 + (threadIdx.x >> 6); ob < old_nbc; ob += gridDim.x * 4) {
		const int nb				  = table_query(cfg, new_table, old_keys[3 * ob], old_keys[3 * ob + 1], old_keys[3 * ob + 2]);
		const unsigned long long mask = old_marks[ob];
		if(nb < 0 || nb >= new_nbc) {
			const bool stranded = old_grid[(size_t) ob * 256 + lane] != 0.f && !((mask >> lane) & 1ull);
			if(__any(stranded) && lane == 0) atomicOr(flag, kSinkCarryMiss);
			continue;
		}
		reinterpret_cast<float4*>(grid + (size_t) nb * 256)[lane] = reinterpret_cast<const float4*>(old_grid + (size_t) ob * 256)[lane];
		if(lane == 0) new_marks[nb] = mask;
	}
}

// The marked cells of the carried grid against the survivors' set-up mass (`mass`: channel 0 of a scratch grid in the same numbering, written by
// rasterize_blocks_kernel with v0 = 0).  One wave per grid block, lane = cell.  With m the node's old mass: !(m > 0) keeps the node's bits;
// m' == 0 leaves +0 in all four channels; else the mass becomes m' and each momentum p * r, r = m' / m as one IEEE division.  Unmarked cells
// are not written.
__global__ __launch_bounds__(256) void sink_rescale_grid_kernel(int nbc, const unsigned long long* __restrict__ marks, const float* __restrict__ mass, float* __restrict__ grid) {
#pragma clang fp contract(off)
	const int lane = threadIdx.x & 63;
	for(int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < nbc; b += gridDim.x * 4) {
		if(!((marks[b] >> lane) & 1ull)) continue;
		float* g	  = grid + (size_t) b * 256 + lane;
		const float m = g[0];
		if(!(m > 0.f)) continue;
		const float m1 = mass[(size_t) b * 256 + lane];
		if(m1 == 0.f) {
			g[0] = g[64] = g[128] = g[192] = 0.f;
			continue;
		}
		const float r = __fdiv_rn(m1, m);
		g[0]		  = m1;
		g[64]		  = g[64] * r;
		g[128]		  = g[128] * r;
		g[192]		  = g[192] * r;
	}
}

}// namespace mpm
