// mpm_grid_field.hpp - the Eulerian readouts (an extension, the reference has none): what grid[0]
// holds between two substeps - the mass m_i and momentum p_i of the last P2G on the sparse blocks of the current partition - asked for
// by position, not by particle.
//   grid_sample_kernel       sum_i W_i(x_q) {m_i, p_i} at arbitrary points: G2P's 27-node stencil, one lane per point
//   grid_volume_kernel<S>    a dense box of nodes, copied (S = 1) or summed over S^3 nodes per output cell (S = 2, 4)
//   grid_box_totals_kernel   {sum m, sum p (3), sum_{m>0} |p|^2 / (2 m)} over the nodes of a box, in float64
// Node (i, j, k), N = 4 G per axis, sits at (i, j, k) dx, in the block with key (i >> 2, j >> 2, k >> 2) at cell ((i & 3) << 4) | ((j & 3) << 2)
// | (k & 3); channel c of cell q of block number nb is grid[nb * 256 + 64 * c + q] (c = mass, px, py, pz: the layout readout_stage_cube reads).
// WHICH NODES HOLD A VALUE: those inside [0, N)^3 whose block the current table knows under a number BELOW nbc.  Numbers in [nbc, ebc) are
// exterior blocks: the table finds them, but grid[0] has no rows for them (it is cleared and written for nbc blocks only) - they read as
// +0, like every node outside the domain or in no block.  The particle readouts never meet such a block (a particle's stencil stays inside
// the neighbour blocks); these kernels do, so every look-up here goes through grid_block_number.
// All three read only: no state changes, and a context that never calls them launches none of them.
#pragma once
#include "mpm_kernels.hpp"

namespace mpm {

constexpr int kGridFieldThreads = 256;

// The number of the block with key (x, y, z) if its nodes hold values, else -1 (outside the domain, unknown to the table, or exterior).
__device__ __forceinline__ int grid_block_number(const GridCfg& cfg, const int* __restrict__ table, int nbc, int x, int y, int z) {
	const int nb = table_query(cfg, table, x, y, z);
	return nb < nbc ? nb : -1;
}

// out4[4 q ..] = sum over the stencil of point q of W {m, px, py, pz}.  The stencil is G2P's: p = x * dx_inv (one multiply, as node_index),
// base = lround_pos(p) - 1, weights bspline_weight_cells(p - base), W = w0[i] * w1[j] * w2[k].  A point with a p that is not finite, < 0 or
// >= N gets zeros.  The stencil's nodes base .. base + 2 lie in the 2 x 2 x 2 blocks at key (base >> 2) + {0, 1}^3: their eight numbers are
// looked up once per point, the 27 nodes pick theirs by selects (every index below is a constant after unrolling: no scratch).
__global__ __launch_bounds__(kGridFieldThreads) void grid_sample_kernel(GridCfg cfg, int nbc, const int* __restrict__ table, const float* __restrict__ grid, const float* __restrict__ xyz, size_t n, float* __restrict__ out4) {
	const size_t q = (size_t) blockIdx.x * kGridFieldThreads + threadIdx.x;
	if(q >= n) return;
	const float nodes = (float) (4 * cfg.G);
	int base[3];
	float w[3][3];
	bool inside = true;
#pragma unroll
	for(int d = 0; d < 3; ++d) {
		const float p = xyz[3 * q + d] * cfg.dx_inv;
		inside		  = inside && p >= 0.f && p < nodes;// (false for a NaN and for either infinity)
		const float pc = inside ? p : 0.f;
		base[d]		  = lround_pos(pc) - 1;// -1 .. N - 1
		bspline_weight_cells(pc - (float) base[d], w[d]);
	}
	float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
	if(inside) {
		const int kx = base[0] >> 2, ky = base[1] >> 2, kz = base[2] >> 2;// (arithmetic shift: base -1 is block -1, which no table holds)
		int nb[2][2][2];
#pragma unroll
		for(int a = 0; a < 2; ++a)
#pragma unroll
			for(int b = 0; b < 2; ++b)
#pragma unroll
				for(int c = 0; c < 2; ++c) nb[a][b][c] = grid_block_number(cfg, table, nbc, kx + a, ky + b, kz + c);
#pragma unroll
		for(int i = 0; i < 3; ++i) {
			const int x	  = base[0] + i;
			const bool hx = (x >> 2) != kx;
			const int n4[2][2] = {{hx ? nb[1][0][0] : nb[0][0][0], hx ? nb[1][0][1] : nb[0][0][1]}, {hx ? nb[1][1][0] : nb[0][1][0], hx ? nb[1][1][1] : nb[0][1][1]}};
#pragma unroll
			for(int j = 0; j < 3; ++j) {
				const int y		= base[1] + j;
				const bool hy	= (y >> 2) != ky;
				const int n2[2] = {hy ? n4[1][0] : n4[0][0], hy ? n4[1][1] : n4[0][1]};
				const float wij = w[0][i] * w[1][j];
#pragma unroll
				for(int k = 0; k < 3; ++k) {
					const int z	  = base[2] + k;
					const int blk = (z >> 2) != kz ? n2[1] : n2[0];
					if(blk < 0) continue;
					const float* g = grid + (size_t) blk * 256 + (((x & 3) << 4) | ((y & 3) << 2) | (z & 3));
					const float W  = wij * w[2][k];
					acc.x += W * g[0];
					acc.y += W * g[64];
					acc.z += W * g[128];
					acc.w += W * g[192];
				}
			}
		}
	}
	reinterpret_cast<float4*>(out4)[q] = acc;
}

// The dense box.  A workgroup takes one TILE of the output at a time: the output cells that cover 4 x 4 x 32 nodes (z longest: the output is
// z-fastest), i.e. (4 / S) x (4 / S) x (32 / S) cells.  It looks up the blocks under the tile once (8 when the tile's first node is block
// aligned, up to 2 x 2 x 9 when it is not), stages them in LDS as a dense node box - every block read as its whole 1 KiB, four 256-byte
// channel rows, by the 256 lanes at once, eight blocks in flight - and then one lane per (channel, output cell) reads its S^3 nodes from
// LDS and writes one word: runs of 32 / S consecutive floats along z.  S = 1 moves the word's bits; S = 2, 4 add in float32, acc = +0 then
// x slowest, z fastest (the model's order; there is no multiply to contract and nothing is reassociated).  A tile with no valued block
// under it (most of a sparse domain) stages nothing and writes zeros.  The tiles are walked with a grid-stride loop, so the launch is
// bounded whatever the box.
constexpr int kVolTileX = 4, kVolTileY = 4, kVolTileZ = 32;					// nodes per tile
constexpr int kVolBlocksX = 2, kVolBlocksY = 2, kVolBlocksZ = kVolTileZ / 4 + 1;// blocks a tile can touch per axis
constexpr int kVolBlocks  = kVolBlocksX * kVolBlocksY * kVolBlocksZ;			// 36
constexpr int kVolPitchY  = 4 * kVolBlocksZ;									// 36 words: a z row of the staged box
constexpr int kVolPitchX  = 4 * kVolBlocksY * kVolPitchY + 16;					// (+16 words: the two x planes a half-wave stages fall on different banks)
constexpr int kVolPitchC  = 4 * kVolBlocksX * kVolPitchX;

struct VolumeArgs {
	long long origin[3];// first node of the box (may be negative)
	long long dims[3];	// output cells per axis
	long long tiles[3]; // tiles per axis
};

template<int S>
__global__ __launch_bounds__(kGridFieldThreads) void grid_volume_kernel(GridCfg cfg, int nbc, const int* __restrict__ table, const float* __restrict__ grid, VolumeArgs a, float* __restrict__ out) {
	constexpr int CX = kVolTileX / S, CY = kVolTileY / S, CZ = kVolTileZ / S;// output cells per tile
	constexpr int kItems = 4 * CX * CY * CZ;
	__shared__ unsigned s_box[4 * kVolPitchC];
	__shared__ int s_nb[kVolBlocks];// >= 0: block number; -1: a block of the tile without values; -2: not under the tile
	const long long ntiles = a.tiles[0] * a.tiles[1] * a.tiles[2];
	unsigned* const out_bits = reinterpret_cast<unsigned*>(out);
	for(long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const long long tz = t % a.tiles[2], ty = (t / a.tiles[2]) % a.tiles[1], tx = t / (a.tiles[2] * a.tiles[1]);
		const long long n0[3] = {a.origin[0] + tx * kVolTileX, a.origin[1] + ty * kVolTileY, a.origin[2] + tz * kVolTileZ};// the tile's first node
		const int off[3]	  = {(int) (n0[0] & 3), (int) (n0[1] & 3), (int) (n0[2] & 3)};									// ... inside its first block
		bool mine = false;
		if(threadIdx.x < kVolBlocks) {
			const int bx = threadIdx.x / (kVolBlocksY * kVolBlocksZ), by = (threadIdx.x / kVolBlocksZ) % kVolBlocksY, bz = threadIdx.x % kVolBlocksZ;
			int nb = -2;
			if(bx < ((off[0] + kVolTileX + 3) >> 2) && by < ((off[1] + kVolTileY + 3) >> 2) && bz < ((off[2] + kVolTileZ + 3) >> 2)) {
				const long long kx = (n0[0] >> 2) + bx, ky = (n0[1] >> 2) + by, kz = (n0[2] >> 2) + bz;// (floor: the shift is arithmetic)
				nb = -1;
				if(kx >= 0 && kx < cfg.G && ky >= 0 && ky < cfg.G && kz >= 0 && kz < cfg.G) nb = grid_block_number(cfg, table, nbc, (int) kx, (int) ky, (int) kz);
			}
			s_nb[threadIdx.x] = nb;
			mine			  = nb >= 0;
		}
		const bool any = __syncthreads_or(mine) != 0;// (also: s_nb is visible, and the previous tile's reads of s_box are done)
		if(any) {
			// (eight blocks' loads are issued before the first is used: one block per trip left a workgroup waiting out one memory latency per
			//  KiB, and the kernel at a fifth of the copy rate - profiles/grid_field.txt)
			for(int first = 0; first < kVolBlocks; first += 8) {
				unsigned v[8];
#pragma unroll
				for(int u = 0; u < 8; ++u) {
					const int nb = first + u < kVolBlocks ? s_nb[first + u] : -2;// (uniform over the workgroup)
					v[u]		 = nb >= 0 ? __float_as_uint(grid[(size_t) nb * 256 + threadIdx.x]) : 0u;
				}
				const int c = threadIdx.x >> 6, cell = threadIdx.x & 63;
				const int in_block = c * kVolPitchC + (cell >> 4) * kVolPitchX + ((cell >> 2) & 3) * kVolPitchY + (cell & 3);
#pragma unroll
				for(int u = 0; u < 8; ++u) {
					const int lb = first + u;
					if(lb >= kVolBlocks || s_nb[lb] == -2) continue;
					const int bx = lb / (kVolBlocksY * kVolBlocksZ), by = (lb / kVolBlocksZ) % kVolBlocksY, bz = lb % kVolBlocksZ;
					s_box[in_block + 4 * bx * kVolPitchX + 4 * by * kVolPitchY + 4 * bz] = v[u];
				}
			}
			__syncthreads();
		}
		for(int item = threadIdx.x; item < kItems; item += kGridFieldThreads) {
			const int cz = item % CZ, cy = (item / CZ) % CY, cx = (item / (CZ * CY)) % CX, c = item / (CZ * CY * CX);
			const long long X = tx * CX + cx, Y = ty * CY + cy, Z = tz * CZ + cz;
			if(X >= a.dims[0] || Y >= a.dims[1] || Z >= a.dims[2]) continue;
			unsigned bits = 0u;
			if(any) {
				const unsigned* src = s_box + c * kVolPitchC + (off[0] + S * cx) * kVolPitchX + (off[1] + S * cy) * kVolPitchY + off[2] + S * cz;
				if(S == 1)
					bits = src[0];
				else {
					float acc = 0.f;
#pragma unroll
					for(int i = 0; i < S; ++i)
#pragma unroll
						for(int j = 0; j < S; ++j)
#pragma unroll
							for(int k = 0; k < S; ++k) acc += __uint_as_float(src[i * kVolPitchX + j * kVolPitchY + k]);
					bits = __float_as_uint(acc);
				}
			}
			out_bits[(((size_t) c * (size_t) a.dims[0] + (size_t) X) * (size_t) a.dims[1] + (size_t) Y) * (size_t) a.dims[2] + (size_t) Z] = bits;
		}
	}
}

// Totals over the nodes of the half-open node box [lo, hi) (already clipped to the domain by the caller): grid_totals_kernel's walk - a
// wave per block, a lane per cell, all nbc blocks - with the nodes outside the box masked, and kReadMomentum's reduction: each lane sums in
// float64, a wave folds its 64 lanes with __shfl_xor, the 4 waves meet in LDS, ONE set of five float64 atomics per workgroup (their order
// is unspecified: the last bits may differ from run to run).  out[4] = sum over nodes with m > 0 of |p|^2 / (2 m), formed in float64 from
// the float32 node values.
constexpr int kBoxSums = 5;
struct BoxArgs {
	int lo[3], hi[3];
};
__global__ __launch_bounds__(kGridFieldThreads) void grid_box_totals_kernel(int nbc, const int* __restrict__ keys, const float* __restrict__ grid, BoxArgs box, double* out) {
	__shared__ double s_red[kGridFieldThreads / 64][kBoxSums];
	const int lane = threadIdx.x & 63;
	double acc[kBoxSums] = {};
	for(int b = blockIdx.x * (kGridFieldThreads / 64) + (threadIdx.x >> 6); b < nbc; b += gridDim.x * (kGridFieldThreads / 64)) {
		const int x = 4 * keys[3 * b] + (lane >> 4), y = 4 * keys[3 * b + 1] + ((lane >> 2) & 3), z = 4 * keys[3 * b + 2] + (lane & 3);
		if(x < box.lo[0] || x >= box.hi[0] || y < box.lo[1] || y >= box.hi[1] || z < box.lo[2] || z >= box.hi[2]) continue;
		const float* g = grid + (size_t) b * 256 + lane;
		const double m = (double) g[0], px = (double) g[64], py = (double) g[128], pz = (double) g[192];
		acc[0] += m;
		acc[1] += px;
		acc[2] += py;
		acc[3] += pz;
		if(m > 0.0) acc[4] += (px * px + py * py + pz * pz) / (2.0 * m);
	}
#pragma unroll
	for(int d = 0; d < kBoxSums; ++d)
#pragma unroll
		for(int off = 32; off > 0; off >>= 1) acc[d] += __shfl_xor(acc[d], off);
	if(lane == 0)
		for(int d = 0; d < kBoxSums; ++d) s_red[threadIdx.x >> 6][d] = acc[d];
	__syncthreads();
	if(threadIdx.x < kBoxSums) {
		double t = 0.0;
		for(int w = 0; w < kGridFieldThreads / 64; ++w) t += s_red[w][threadIdx.x];
		atomicAdd(out + threadIdx.x, t);
	}
}

}// namespace mpm
