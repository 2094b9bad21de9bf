// mpm_particle_emit.hpp — particle emission (mpm_emit_particles): the kernels of the re-lay that adds particles to a context that has
// been set up.  The substep kernels know nothing of it: every live particle of every model is gathered into flat staging arrays, the new particles
// are appended, mpm_initial_setup's own kernels lay the merged arrays out in a fresh partition, the old grid is carried over by block key and the
// new particles alone are rasterised on top with rasterize_particles_kernel (mpm_particle_init.hpp).
//
// Group segments: emit_gather_kernel 16 B (the block's output range: one 8-byte first slot, one 4-byte counter), emit_append_kernel 0 B,
// emit_count_kernel 0 B, emit_bins_kernel 0 B, emit_fill_ids_kernel 0 B, emit_carry_grid_kernel 0 B.
#pragma once
#include "mpm_kernels.hpp"
#include "mpm_particle_init.hpp"
#include "mpm_readout.hpp"

namespace mpm {

// what the emission's checks found, one bit per reason
enum { kEmitBadPosition = 1, kEmitOutside = 2, kEmitBlockFull = 4, kEmitCarryMiss = 8 };

// The staging columns of one model, one slot per particle: what fill_bins_state_kernel reads (state9 in MPM_STATE_B's verbatim layout) and the id.
struct EmitStage {
	float* xyz;	  // 3 per slot, world units (cell units times dx: exact, dx is a power of two)
	float* state9;// 9 per slot, as mpm_retrieve_state returns it
	float* logjp; // 1 per slot
	int* ids;	  // 1 per slot; null in an untracked context
};

__device__ __forceinline__ void emit_store_state(float* __restrict__ s9, bool fluid, const float (&s)[6]) {
	// s = {b00 (marked), b11, b22, b10, b20, b21}: the full symmetric matrix, column-major (sym_expand's layout); the J-fluid keeps J in entry 0
	s9[0] = s[0];
	s9[1] = fluid ? 0.f : s[3];
	s9[2] = fluid ? 0.f : s[4];
	s9[3] = fluid ? 0.f : s[3];
	s9[4] = fluid ? 0.f : s[1];
	s9[5] = fluid ? 0.f : s[5];
	s9[6] = fluid ? 0.f : s[4];
	s9[7] = fluid ? 0.f : s[5];
	s9[8] = fluid ? 0.f : s[2];
}

// readout_kernel's walk (mpm_readout.hpp: readout_live, readout_position, the same slot hand-out) with every column written in the one pass, so
// that position, state, log Jp and id of a particle share a slot.  One workgroup per particle block; the record is fetched with 16-byte loads
// (one for the J-fluid's {x, y, z, J}, two for a solid's {x, y, z, b00, b11, b22, b10, b20}).  *counter (zeroed by the caller) ends at the number
// of live particles; slots at or beyond `capacity` are dropped.
__global__ __launch_bounds__(kReadoutThreads) void emit_gather_kernel(ReadoutArgs a, EmitStage out, unsigned long long capacity, unsigned long long* counter) {
	__shared__ unsigned long long s_first;
	__shared__ unsigned s_next;
	const int b = blockIdx.x;
	const int n = a.size[b];
	if(n == 0) return;
	const int kx = a.cur_keys[3 * b], ky = a.cur_keys[3 * b + 1], kz = a.cur_keys[3 * b + 2];
	const int* list = a.list + (size_t) a.row_of[b] * a.cfg.ppb;
	if(threadIdx.x == 0) {
		s_first = atomicAdd(counter, (unsigned long long) n);
		s_next	= 0u;
	}
	__syncthreads();
	const bool fluid = a.nch == 4;
	for(int pidib = threadIdx.x; pidib < ((n + 63) & ~63); pidib += kReadoutThreads) {
		const bool live					   = readout_live(n, pidib, a.dense);
		const unsigned long long live_mask = __ballot(live);
		if(live_mask == 0ull) continue;
		const int lane	 = threadIdx.x & 63;
		const int leader = __ffsll((long long) live_mask) - 1;
		unsigned first	 = 0;
		if(lane == leader) first = atomicAdd(&s_next, (unsigned) __popcll(live_mask));
		first = __shfl(first, leader);
		if(!live) continue;
		const unsigned rank		   = first + (unsigned) __popcll(live_mask & ((1ull << lane) - 1ull));
		const unsigned long long o = s_first + rank;
		if(rank >= (unsigned) n || o >= capacity) continue;
		float p[3];
		const float* row = nullptr;
		size_t sslot	 = 0;
		const float* src = readout_position(a, list[pidib], kx, ky, kz, p, &row, &sslot);
		const float4 r0	 = *reinterpret_cast<const float4*>(src);
		out.xyz[3 * o]	   = r0.x * a.cfg.dx;
		out.xyz[3 * o + 1] = r0.y * a.cfg.dx;
		out.xyz[3 * o + 2] = r0.z * a.cfg.dx;
		float s[6] = {r0.w, 0.f, 0.f, 0.f, 0.f, 0.f};
		if(!fluid) {
			const float4 r1 = *reinterpret_cast<const float4*>(src + 4);
			s[1] = r1.x, s[2] = r1.y, s[3] = r1.z, s[4] = r1.w, s[5] = row[0];
		}
		emit_store_state(out.state9 + 9 * o, fluid, s);
		out.logjp[o] = a.nch - rec_floats(a.nch) == 2 ? row[1] : 0.f;
		if(out.ids) out.ids[o] = a.ids[sslot];
	}
}

// The n new particles, whose positions the host has copied to slots first .. first + n - 1 of out.xyz: their state (a's state9 through
// particle_init_state, as fill_bins_state_kernel would read it; null: stress-free), their log Jp (null: log_jp0) and their ids first_id + i go
// into the staging columns; a position that is not finite, or whose block key lies outside the domain (what set-up counts as lost), raises a flag.
__global__ __launch_bounds__(256) void emit_append_kernel(GridCfg cfg, size_t n, size_t first, bool fluid, float log_jp0, int first_id, ParticleInit a, EmitStage out, int* flag) {
	int bad = 0;
	for(size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
		const size_t o = first + i;
		const float x = out.xyz[3 * o], y = out.xyz[3 * o + 1], z = out.xyz[3 * o + 2];
		if(!(isfinite(x) && isfinite(y) && isfinite(z)))
			bad |= kEmitBadPosition;
		else {
			int bx, by, bz, cx, cy, cz;
			particle_block_key(cfg, out.xyz, o, bx, by, bz, cx, cy, cz);
			if(!key_ok(cfg, bx, by, bz)) bad |= kEmitOutside;
		}
		float s[6] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f};
		if(a.state9) particle_init_state(fluid, a.state_f, a.state9 + 9 * i, s);
		emit_store_state(out.state9 + 9 * o, fluid, s);
		out.logjp[o] = a.logjp ? a.logjp[i] : log_jp0;
		if(out.ids) out.ids[o] = first_id + (int) i;
	}
	if(bad) atomicOr(flag, bad);
}

// bucket_particles_kernel's count without its list: how many of the n particles fall into each block of `table` (counts zeroed by the caller).
// A particle without a block, or one beyond the ppb list slots of its block, raises a flag - nothing of the context is written.
__global__ __launch_bounds__(256) void emit_count_kernel(GridCfg cfg, size_t n, const float* __restrict__ xyz, const int* __restrict__ table, int* counts, int* flag) {
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	int bx, by, bz, cx, cy, cz;
	particle_block_key(cfg, xyz, i, bx, by, bz, cx, cy, cz);
	const int bno = table_query(cfg, table, bx, by, bz);
	if(bno < 0) {
		atomicOr(flag, kEmitOutside);
		return;
	}
	if(atomicAdd(&counts[bno], 1) >= cfg.ppb) atomicOr(flag, kEmitBlockFull);
}

// The bins those counts need, as init_bins_kernel will hand them out: ceil(count / 64) per block, one atomic per wave.
__global__ __launch_bounds__(256) void emit_bins_kernel(int pbc, const int* __restrict__ counts, int* total) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	int nbins	= b < pbc ? (counts[b] + kBin - 1) / kBin : 0;
#pragma unroll
	for(int off = 32; off > 0; off >>= 1) nbins += __shfl_xor(nbins, off);
	if((threadIdx.x & 63) == 0 && nbins) atomicAdd(total, nbins);
}

// fill_ids_kernel (mpm_particle_ids.hpp) with one indirection: the bucketed index names a staging slot, whose id goes to the bin slot.
__global__ __launch_bounds__(256) void emit_fill_ids_kernel(int ppb, const int* __restrict__ ids_by_block, const int* __restrict__ size, const int* __restrict__ binoff, const int* __restrict__ staged_ids, int* __restrict__ ids) {
	const int b = blockIdx.x;
	const int n = size[b];
	for(int pidib = threadIdx.x; pidib < n; pidib += blockDim.x) ids[(size_t) (binoff[b] + (pidib >> 6)) * kBin + (pidib & 63)] = staged_ids[ids_by_block[(size_t) b * ppb + pidib]];
}

// The grid of the old numbering (old_nbc blocks with their keys, both kept aside) into the new one, which the caller has zeroed: one wave per old
// block, one 16-byte load and store per lane.  Every old neighbour block is a neighbour block of the merged particle set; one that the new table
// does not hold raises a flag.
__global__ __launch_bounds__(256) void emit_carry_grid_kernel(GridCfg cfg, int old_nbc, int new_nbc, const int* __restrict__ old_keys, const float* __restrict__ old_grid, const int* __restrict__ new_table, float* __restrict__ grid, int* flag) {
	const int lane = threadIdx.x & 63;
	for(int ob = blockIdx.x * 4 + (threadIdx.x >> 6); ob < old_nbc; ob += gridDim.x * 4) {
		const int nb = table_query(cfg, new_table, old_keys[3 * ob], old_keys[3 * ob + 1], old_keys[3 * ob + 2]);
		if(nb < 0 || nb >= new_nbc) {
			if(lane == 0) atomicOr(flag, kEmitCarryMiss);
			continue;
		}
		reinterpret_cast<float4*>(grid + (size_t) nb * 256)[lane] = reinterpret_cast<const float4*>(old_grid + (size_t) ob * 256)[lane];
	}
}

}// namespace mpm
