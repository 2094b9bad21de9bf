// mpm_grid_isosurface.hpp - the surface readout (an extension, the reference has none): the
// iso-contour f = iso_mass of the mass channel of grid[0] by marching tetrahedra, appended as a triangle soup to a caller-sized buffer.
//   grid_isosurface_kernel<VEL>   a workgroup per valued block; VEL adds a per-vertex velocity
// The field, the cells, the tetrahedra, the vertices and the winding are defined in include/claymore_amd.h (mpm_grid_isosurface); the
// model is tests/grid_isosurface_model.py.  In short: cell (i, j, k), i, j, k in [-1, N - 1], has the corner nodes (i, j, k) + {0, 1}^3; it
// is cut into the six Kuhn tetrahedra c0 = 0, c1 = e_a, c2 = e_a + e_b, c3 = (1, 1, 1), one per permutation (a, b, c) of the axes; an edge
// (ci, cj), i < j, with exactly one end inside (f > iso) carries the vertex ci + t (cj - ci), t = (iso - f(ci)) / (f(cj) - f(ci)).  A vertex
// depends on its edge's two nodes only - never on the cell or tetrahedron that asks - so triangles that share an edge get the same bits.
// WHO EMITS A CELL.  A workgroup stages the 6^3 nodes 4 key - 1 .. 4 key + 4 of its block (the nodes of the 26 blocks around it read +0
// where grid_block_number finds no values) and so sees the 5^3 cells whose low corner is node 4 key + {-1 .. 3}^3.  Each cell is emitted by
// ONE block: the valued block that holds the cell's corner with the smallest index 4 cx + 2 cy + cz among the corners in valued blocks.
// That is every cell whose corner 0 the block holds (4^3), and of the 61 cells on its three lower faces those whose corners of smaller
// index all lie in blocks without values - decided per cell from the 27 looked-up numbers, as the rule reads: walk the corners upward,
// stop at the first in a valued block, own the cell iff that block is this one.  (The corners below a block's own lowest can lie in any of
// the 13 blocks that precede it in (x, y, z) order - a cell on the lower x face at the upper y edge reaches block (-1, +1, 0) - not in the
// seven blocks key - {0, 1}^3 alone.)  A cell with an inside corner has a valued corner block, so it is emitted exactly once.
// Reads only: grid[0], the table and the keys.
#pragma once
#include "mpm_grid_field.hpp"

namespace mpm {

constexpr int kIsoThreads = 256;
constexpr int kIsoPitchY = 6, kIsoPitchX = 36, kIsoPitchC = 216;// the staged node box: [channel][x][y][z], 6 nodes per axis
constexpr int kIsoCells = 125, kIsoItems = 6 * kIsoCells;		 // (cell, tetrahedron) pairs of a block
constexpr int kIsoRounds = (kIsoItems + kIsoThreads - 1) / kIsoThreads;
constexpr int kIsoStageBatch = 7;							 // channel rows a wave keeps in flight while staging

struct IsoArgs {
	int lo[3], hi[3];// the half-open cell box
	float iso;
	unsigned long long capacity;// triangles the buffers hold
};

// The triangles of a tetrahedron of an EVEN permutation for the 4-bit case (bit i: corner i inside): up to six vertices, four bits each,
// an edge (i, j), i < j, as i | j << 2; vertices 0 - 2 the first triangle, 3 - 5 the second.  An odd permutation mirrors the tetrahedron:
// the same vertices with the last two of each triangle exchanged.  Derived from the rule by tests/grid_isosurface_model.py (TABLES): one
// inside corner I gives P(I, O0) P(I, O1) P(I, O2), three the mirror case, two the quad P(I0,O0) P(I0,O1) P(I1,O1) P(I1,O0) split along
// its first diagonal; the order is reversed where det[O0 - I, O1 - I, O2 - I] (for the quad: of the edge midpoints) says the normal
// would point to the inside corners.
__device__ __forceinline__ unsigned iso_case_triangles(int mask) {
	switch(mask) {
	case 1: return 0xc84u;
	case 2: return 0x9d4u;
	case 3: return 0x9d8dc8u;
	case 4: return 0xe98u;
	case 5: return 0xe94ce4u;
	case 6: return 0x8e4ed4u;
	case 7: return 0xedcu;
	case 8: return 0xdecu;
	case 9: return 0xde4e84u;
	case 10: return 0xec49e4u;
	case 11: return 0x9e8u;
	case 12: return 0xcd8d98u;
	case 13: return 0xd94u;
	case 14: return 0x8c4u;
	default: return 0u;
	}
}
constexpr unsigned kIsoOddPerms = 0x26u;// permutation p = 2 a + (b is the larger of the two other axes): (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0)

template<typename T>
__device__ __forceinline__ T iso_sel4(int i, T v0, T v1, T v2, T v3) {
	return i == 0 ? v0 : i == 1 ? v1 : i == 2 ? v2 : v3;
}

// One (cell, tetrahedron) pair of a block: item = 6 cell + p, cell = 25 lx + 5 ly + lz the cell whose low corner is node 4 key - 1 + l,
// p the permutation.  The corners c0 .. c3 sit at base + {0, off1, off2, off3} in the staged box and at l + the bits of {0, m1, m2, 7}
// (bit d: axis d); mask is the case, 0 for an item past the last or of a cell the block does not emit.
struct IsoItem {
	int p, lx, ly, lz, base, off1, off2, off3, m1, m2, mask;
	float f0, f1, f2, f3;
	__device__ __forceinline__ IsoItem(int item, const float* s_box, const unsigned char* s_cell, float iso) {
		const int cell = item / 6;
		p			   = item - 6 * cell;
		const bool live = item < kIsoItems && s_cell[min(cell, kIsoCells - 1)] != 0;
		lx = cell / 25, ly = (cell / 5) % 5, lz = cell % 5;
		const int ax = p >> 1, bx = (p & 1) ? (ax == 2 ? 1 : 2) : (ax == 0 ? 1 : 0);// the permutation's first two axes
		const int pitch_a = ax == 0 ? kIsoPitchX : ax == 1 ? kIsoPitchY : 1, pitch_b = bx == 0 ? kIsoPitchX : bx == 1 ? kIsoPitchY : 1;
		off1 = pitch_a, off2 = pitch_a + pitch_b, off3 = kIsoPitchX + kIsoPitchY + 1;
		m1 = 1 << ax, m2 = m1 | (1 << bx);
		base = lx * kIsoPitchX + ly * kIsoPitchY + lz;
		f0 = f1 = f2 = f3 = 0.f;
		if(live) {
			f0 = s_box[base];
			f1 = s_box[base + off1];
			f2 = s_box[base + off2];
			f3 = s_box[base + off3];
		}
		mask = live ? (f0 > iso ? 1 : 0) | (f1 > iso ? 2 : 0) | (f2 > iso ? 4 : 0) | (f3 > iso ? 8 : 0) : 0;
	}
};
__device__ __forceinline__ int iso_triangle_count(unsigned tris) {
	return tris == 0u ? 0 : (tris >> 12) != 0u ? 2 : 1;
}

// Stage NCH channels, from C0 on, of the 6^3 node box of a block: a wave per 256-byte channel row of one of the 27 blocks, the lanes whose
// node lies outside the box idle, kIsoStageBatch rows in flight per wave.  Every node of the box belongs to exactly one of the 27 blocks,
// so every word of the staged channels is written (+0 where the block holds no values).
template<int C0, int NCH>
__device__ __forceinline__ void iso_stage(float* s_box, const int* s_nb, const float* __restrict__ grid, int lane, int wave) {
	for(int first = 0; first < 27 * NCH; first += 4 * kIsoStageBatch) {
		float v[kIsoStageBatch];
		int at[kIsoStageBatch];
#pragma unroll
		for(int u = 0; u < kIsoStageBatch; ++u) {
			const int r = first + 4 * u + wave;
			at[u]		= -1;
			v[u]		= 0.f;
			if(r >= 27 * NCH) continue;
			const int o = r / NCH, c = C0 + r % NCH;
			const int x = 4 * (o / 9) + (lane >> 4) - 3, y = 4 * ((o / 3) % 3) + ((lane >> 2) & 3) - 3, z = 4 * (o % 3) + (lane & 3) - 3;// box index
			if((unsigned) x >= 6u || (unsigned) y >= 6u || (unsigned) z >= 6u) continue;
			at[u]		 = c * kIsoPitchC + x * kIsoPitchX + y * kIsoPitchY + z;
			const int nb = s_nb[o];
			if(nb >= 0) v[u] = grid[(size_t) nb * 256 + 64 * c + lane];
		}
#pragma unroll
		for(int u = 0; u < kIsoStageBatch; ++u)
			if(at[u] >= 0) s_box[at[u]] = v[u];
	}
}

template<bool VEL>
__global__ __launch_bounds__(kIsoThreads) void grid_isosurface_kernel(GridCfg cfg, int nbc, const int* __restrict__ keys, const int* __restrict__ table, const float* __restrict__ grid, IsoArgs a, float* __restrict__ tri_xyz, float* __restrict__ tri_vel, unsigned long long* counter) {
	constexpr int C = VEL ? 4 : 1;
	__shared__ float s_box[C * kIsoPitchC];
	__shared__ int s_nb[27];			 // the block at key + (o - 1), o = 9 ox + 3 oy + oz: its number, or -1 if it holds no values
	__shared__ unsigned char s_cell[128];// 1: a cell this block emits (owned, inside the cell box, with corners on both sides)
	__shared__ int s_sum[4 * kIsoRounds]; // the triangles of a (round, wave), then of those before it
	__shared__ unsigned long long s_first;// the block's first triangle
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for(int b = blockIdx.x; b < nbc; b += gridDim.x) {
		const int kx = keys[3 * b], ky = keys[3 * b + 1], kz = keys[3 * b + 2];
		if(threadIdx.x < 27) s_nb[threadIdx.x] = grid_block_number(cfg, table, nbc, kx + (int) threadIdx.x / 9 - 1, ky + ((int) threadIdx.x / 3) % 3 - 1, kz + (int) threadIdx.x % 3 - 1);
		__syncthreads();// (also: the previous block's reads of s_box and s_cell are done)
		// The mass of the box first; the momenta only once the block turns out to emit (most blocks lie inside the material or outside it).
		iso_stage<0, 1>(s_box, s_nb, grid, lane, wave);
		__syncthreads();
		// The cells: which of the 125 this block emits.
		bool emit = false;
		if(threadIdx.x < kIsoCells) {
			const int lx = threadIdx.x / 25, ly = (threadIdx.x / 5) % 5, lz = threadIdx.x % 5;// the low corner's box index; its node is 4 key - 1 + l
			const int gx = 4 * kx - 1 + lx, gy = 4 * ky - 1 + ly, gz = 4 * kz - 1 + lz;
			const bool in_box = gx >= a.lo[0] && gx < a.hi[0] && gy >= a.lo[1] && gy < a.hi[1] && gz >= a.lo[2] && gz < a.hi[2];
			int n_in = 0, owner = -1;
#pragma unroll
			for(int ci = 0; ci < 8; ++ci) {
				const int x = lx + (ci >> 2), y = ly + ((ci >> 1) & 1), z = lz + (ci & 1);
				n_in += s_box[x * kIsoPitchX + y * kIsoPitchY + z] > a.iso ? 1 : 0;
				const int o = 9 * ((x + 3) >> 2) + 3 * ((y + 3) >> 2) + ((z + 3) >> 2);// box index 0: the block below; 1 .. 4: this one; 5: the one above
				if(owner < 0 && s_nb[o] >= 0) owner = o;
			}
			emit				  = in_box && owner == 13 && n_in > 0 && n_in < 8;
			s_cell[threadIdx.x] = emit ? 1 : 0;
		}
		if(!__syncthreads_or(emit)) continue;
		if(VEL) iso_stage<1, 3>(s_box, s_nb, grid, lane, wave);// (visible after the barrier below)
		// The (cell, tetrahedron) pairs, a lane each, in two passes over the same items: first every lane forms its case and counts its 0, 1
		// or 2 triangles, the waves rank their lanes by ballots, and the WORKGROUP reserves its range with one atomic (atomics on one address
		// serialise at ~11 ns each: one per wave and round took 0.95 ms at C3 instead of 0.30 - profiles/grid_isosurface.txt); then each
		// lane forms the case again from LDS and writes its triangles where its range lies below the capacity.
		unsigned ranks = 0u;// the lane's rank in its wave, eight bits a round (at most 2 x 63)
		static_assert(kIsoRounds <= 4, "ranks holds four rounds");
#pragma unroll
		for(int r = 0; r < kIsoRounds; ++r) {// (whole waves: every lane meets the ballots)
			const IsoItem it(r * kIsoThreads + threadIdx.x, s_box, s_cell, a.iso);
			const int ntri = iso_triangle_count(iso_case_triangles(it.mask));
			const unsigned long long one = __ballot(ntri == 1), two = __ballot(ntri == 2), below = (1ull << lane) - 1ull;
			ranks |= (unsigned) (__popcll(one & below) + 2 * __popcll(two & below)) << (8 * r);
			if(lane == 0) s_sum[4 * r + wave] = __popcll(one) + 2 * __popcll(two);
		}
		__syncthreads();
		if(threadIdx.x == 0) {
			int total = 0;
			for(int i = 0; i < 4 * kIsoRounds; ++i) {// the triangles before each (round, wave)
				const int n = s_sum[i];
				s_sum[i]	= total;
				total += n;
			}
			s_first = atomicAdd(counter, (unsigned long long) total);// (total > 0: a cell that is emitted has a cut tetrahedron)
		}
		__syncthreads();
#pragma unroll 1
		for(int r = 0; r < kIsoRounds; ++r) {
			const IsoItem it(r * kIsoThreads + threadIdx.x, s_box, s_cell, a.iso);
			const unsigned tris = iso_case_triangles(it.mask);
			const int ntri		= iso_triangle_count(tris);
			if(ntri == 0) continue;
			const unsigned long long mine = s_first + (unsigned long long) (s_sum[4 * r + wave] + (int) ((ranks >> (8 * r)) & 255u));
			const int p = it.p, lx = it.lx, ly = it.ly, lz = it.lz, base = it.base, off1 = it.off1, off2 = it.off2, off3 = it.off3, m1 = it.m1, m2 = it.m2, m3 = 7;
			const float f0 = it.f0, f1 = it.f1, f2 = it.f2, f3 = it.f3;
			const bool odd = (kIsoOddPerms >> p) & 1u;
			const int g[3] = {4 * kx - 1 + lx, 4 * ky - 1 + ly, 4 * kz - 1 + lz};
			for(int k = 0; k < ntri; ++k) {
				const unsigned long long q = mine + (unsigned long long) k;
				if(q >= a.capacity) break;// (counted all the same: *n is the count the surface has)
#pragma unroll
				for(int v = 0; v < 3; ++v) {
					const int slot		= 3 * k + (odd && v != 0 ? 3 - v : v);
					const unsigned code = (tris >> (4 * slot)) & 15u;
					const int i = (int) (code & 3u), j = (int) (code >> 2);// the edge (ci, cj), i < j: ci <= cj componentwise
					const float fa = iso_sel4(i, f0, f1, f2, f3), fb = iso_sel4(j, f0, f1, f2, f3);
					const int ma = iso_sel4(i, 0, m1, m2, m3), mb = iso_sel4(j, 0, m1, m2, m3);
					const float t = __fdiv_rn(a.iso - fa, fb - fa);
#pragma unroll
					for(int d = 0; d < 3; ++d) {
						const float node				  = (float) (g[d] + ((ma >> d) & 1));
						tri_xyz[9ull * q + 3 * v + d] = (((ma ^ mb) >> d) & 1 ? node + t : node) * cfg.dx;
					}
					if(VEL) {
						const int oa = base + iso_sel4(i, 0, off1, off2, off3), ob = base + iso_sel4(j, 0, off1, off2, off3);
#pragma unroll
						for(int c = 1; c < 4; ++c) {
							const float pa = s_box[c * kIsoPitchC + oa], pb = s_box[c * kIsoPitchC + ob];
							tri_vel[9ull * q + 3 * v + (c - 1)] = __fdiv_rn(pa + t * (pb - pa), a.iso);
						}
					}
				}
			}
		}
	}
}

}// namespace mpm
