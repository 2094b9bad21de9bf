// mpm_particle_ids.hpp - persistent particle identities (an extension, opt-in: mpm_track_particle_ids).
// A tracked model carries one int32 per bin slot in a side array ids[2], double-buffered and addressed like bins[2]:
//   particle at slot s of a block whose first bin is `binoff` -> ids[(binoff + (s >> 6)) * 64 + (s & 63)]
// The value is the particle's index in the xyz array its model was added with.  G2P2G and the record formats know nothing of it: at a
// substep boundary the list record at position p of block b names its source slot (direction tag + slot in a block of the previous
// numbering), and G2P2G stores that particle at slot p of the block's destination bins - so the substep's permutation is data that
// prepare_blocks_kernel has already produced, and move_ids_kernel applies it to the side array beside every G2P2G launch.
#pragma once
#include "mpm_kernels.hpp"
#include "mpm_readout.hpp"

namespace mpm {

constexpr int kMoveIdsThreads = 256;				   // four waves: one particle block each
constexpr int kMoveIdsWaves	  = kMoveIdsThreads / 64;
constexpr int kMoveIdsUnroll  = 4;					   // 64-record slices in flight per wave

// Set-up: bucket_particles_kernel has left each block's input indices in `ids_by_block` (list[1], ppb per block), fill_bins_kernel places
// particle pidib of block b at slot pidib of the block's bins: the same index goes to the same slot of the side array.
__global__ __launch_bounds__(256) void fill_ids_kernel(int ppb, const int* __restrict__ ids_by_block, const int* __restrict__ size, const int* __restrict__ binoff, int* __restrict__ ids) {
	const int b = blockIdx.x;
	const int n = size[b];
	for(int pidib = threadIdx.x; pidib < n; pidib += blockDim.x) ids[(size_t) (binoff[b] + (pidib >> 6)) * kBin + (pidib & 63)] = ids_by_block[(size_t) b * ppb + pidib];
}

// What one G2P2G launch of a model sees (launch_g2p2g_model), and the two id buffers.
struct MoveIdsArgs {
	int ppb, pid_bits, cap;
	int dense;			  // the pair list layout (no holes), else the sliced one
	const int* size;	  // particles per current block
	const int* row_of;	  // row of list_in that belongs to current block b
	const int* list_in;	  // the advection records G2P2G reads
	const int* binoff_dst;// first destination bin of a block, current numbering
	const int* blockinfo; // [block][kInfoRow]: [0, 27) the first source bin per direction (prepare_blocks_kernel)
	const int* ids_src;
	int* ids_dst;
};

// ids_dst[binoff_dst[b] * 64 + p] = ids_src[source slot of record p], for every live list position p of every block the G2P2G launch with
// the same block_list / only_flag / nblocks_ptr / nblocks works on.  One wave per particle block, four per workgroup; a wave walks over blocks
// w, w + waves in the launch, ... of the true count (read from device memory as G2P2G reads it).  Everything addressed by the block number
// is wave-uniform (scalar loads); the block's 27 source bin offsets come from its look-up row in ONE load, lane l < 27 keeps direction l's
// in a register, and a record fetches its direction's with __shfl (ds_bpermute, no LDS space) - not 27 table probes per record.  Per record:
// a coalesced 4-B list load, a scattered 4-B id load, a coalesced 4-B store.  No atomics, no barrier: waves share nothing.  The kernel is
// bound by latency, not bytes (two dependent round trips per record), hence the four slices in flight (kMoveIdsUnroll).
__global__ __launch_bounds__(kMoveIdsThreads) void move_ids_kernel(MoveIdsArgs a, const int* __restrict__ block_list, const int* __restrict__ only_flag, const int* __restrict__ nblocks_ptr, int nblocks) {
	const int lane	= threadIdx.x & 63;
	const int wave	= __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
	const int total = nblocks_ptr ? min(*nblocks_ptr, a.cap) : nblocks;
	const int tag_shift = a.pid_bits + kKeyBits;
	for(int bid = (int) blockIdx.x * kMoveIdsWaves + wave; bid < total; bid += (int) gridDim.x * kMoveIdsWaves) {
		const int b	   = __builtin_amdgcn_readfirstlane(block_list ? block_list[bid] : bid);
		const int size = __builtin_amdgcn_readfirstlane(a.size[b]);
		const int flag = only_flag ? __builtin_amdgcn_readfirstlane(only_flag[b]) : 1;
		if(size == 0 || flag == 0) continue;
		const int row	 = __builtin_amdgcn_readfirstlane(a.row_of[b]);
		const int dst0	 = __builtin_amdgcn_readfirstlane(a.binoff_dst[b]);
		const int* list	 = a.list_in + (size_t) row * a.ppb;
		int* dst		 = a.ids_dst + (size_t) dst0 * kBin;
		const int info	 = a.blockinfo[(size_t) b * kInfoRow + lane];// (lanes 27.. hold the row's other look-ups: never asked for, a tag is < 27)
		// kMoveIdsUnroll slices per trip, stage by stage: all list loads, then all gathers, then the stores - a trip is two dependent round trips to
		// memory whatever it carries, and a block of 512 records is two trips instead of eight.  The loads are unconditional (countable for
		// s_waitcnt, no divergent control flow): a lane without a record re-reads the block's first one, which exists in both layouts.
		for(int p0 = 0; p0 < size; p0 += 64 * kMoveIdsUnroll) {// (p0 wave-uniform: every lane takes every trip, so the shuffles below see lanes 0..26)
			bool live[kMoveIdsUnroll];
			int rec[kMoveIdsUnroll], id[kMoveIdsUnroll];
#pragma unroll
			for(int u = 0; u < kMoveIdsUnroll; ++u) {
				const int q0 = p0 + 64 * u;
				live[u]		 = q0 < size ? readout_live(size, q0 + lane, a.dense) : false;
				rec[u]		 = list[live[u] ? q0 + lane : 0];
			}
#pragma unroll
			for(int u = 0; u < kMoveIdsUnroll; ++u) {
				const int sp  = rec[u] & (a.ppb - 1);
				const int tag = (rec[u] >> tag_shift) & 31;
				const int got = __shfl(info, tag);
				const int off = tag < 27 ? got : -1;
				live[u]		  = live[u] && off >= 0;// (a source block that is not there, a tag that names no direction: never for a record G2P2G may read)
				id[u]		  = a.ids_src[off >= 0 ? (size_t) (off + (sp >> 6)) * kBin + (sp & 63) : (size_t) 0];
			}
#pragma unroll
			for(int u = 0; u < kMoveIdsUnroll; ++u)
				if(live[u]) dst[p0 + 64 * u + lane] = id[u];
		}
	}
}

}// namespace mpm
