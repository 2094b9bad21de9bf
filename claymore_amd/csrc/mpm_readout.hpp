// mpm_readout.hpp — per-particle velocity output (an extension: the reference's output_model, mgmpm_kernels.cuh:1087-1122, copies
// positions only).  G2P2G is fused, so a particle's velocity v_p and affine matrix C_p exist only in registers of the substep kernels;
// this kernel gathers them again, the way G2P does, from the grid a public call leaves behind: grid[0] holds each node's mass m_i and
// momentum p_i of the last P2G.
//   v_i = p_i / m_i (m_i > 0, else 0)   - the state BEFORE the next grid update: no gravity, walls or collision object
//   v_p = sum_i w_ip v_i                - 27-node quadratic B-spline stencil, base node and weights those of G2P (lround_pos, bspline_weight_cells)
//   C_p = D^-1 sum_i w_ip v_i (x_i - x_p)^T, D^-1 = 4 / dx^2, column-major: C[3 * c + r] = C_rc (G2P2G's A, mpm_g2p2g.hpp)
// Layout: one workgroup (256 lanes) per particle block, walking the block's list as retrieve_kernel does (sliced holes, pair layout,
// row_of, binoff, the neighbour direction in the record).  The 2x2x2 grid blocks the block's stencils reach are staged once in LDS as
// velocities: 8^3 nodes x 16 B = 8 KiB; a block that is not registered (or beyond an upper face) stages zero.  Each particle then reads
// its 27 nodes from LDS at the cube-local stencil base ((base - 1) & 3) + 1 - G2P's, which also gives particles of cells -2 / -1 the
// reference's wrapped key.  Output slots: ONE global atomic per workgroup reserves the block's n slots, its waves take theirs from an LDS
// counter (the block's list holds exactly n records).  Per-wave global atomics on the one counter - what retrieve_kernel amounts to after
// the compiler's wave aggregation - serialise at ~12 ns each: 7.5 ms for C3's 626 k waves; this kernel takes 1.10 ms, and so does the
// reduction below, which has no counter at all (profiles/c3_velocity_readout.txt, c3_particle_momentum.txt).  Position,
// velocity and C of a particle go to the same slot.  particle_momentum_kernel sums the same readout instead of writing it.
#pragma once
#include "mpm_kernels.hpp"

namespace mpm {

constexpr int kReadoutThreads = 256;

// The pieces both readout kernels share - the cube staging, the record fetch and the 27-node gather - so that the stencil, tie and
// face rules live in one place.
// Stage the 2x2x2 grid blocks at (kx, ky, kz) + {0, 1}^3 as velocities: node (x, y, z) of the 8^3 cube at (x << 6) | (y << 3) | z.
// The eight table look-ups are done once, by eight lanes, into s_nb (not once per node: 64 hash probes per block).
__device__ __forceinline__ void readout_stage_cube(const GridCfg& cfg, const int* __restrict__ cur_table, const float* __restrict__ grid, int kx, int ky, int kz, float4* s_v) {
	__shared__ int s_nb[8];
	if(threadIdx.x < 8) s_nb[threadIdx.x] = table_query(cfg, cur_table, kx + ((threadIdx.x >> 2) & 1), ky + ((threadIdx.x >> 1) & 1), kz + (threadIdx.x & 1));
	__syncthreads();
	for(int i = threadIdx.x; i < 512; i += kReadoutThreads) {
		const int lb = i >> 6, c = i & 63;// grid block of the cube (x, y, z bits 2, 1, 0) and its cell, as grid blocks are laid out
		const int nb = s_nb[lb];
		float4 v	 = make_float4(0.f, 0.f, 0.f, 0.f);
		if(nb >= 0) {
			const float* g = grid + (size_t) nb * 256 + c;
			const float m  = g[0];
			if(m > 0.f) v = make_float4(g[64] / m, g[128] / m, g[192] / m, 0.f);
		}
		const int x = ((lb >> 2) & 1) * 4 + (c >> 4), y = ((lb >> 1) & 1) * 4 + ((c >> 2) & 3), z = (lb & 1) * 4 + (c & 3);
		s_v[(x << 6) | (y << 3) | z] = v;
	}
}
// Whether slot pidib of a list of n records holds a particle (a hole of the sliced list layout does not; the pair layout has none).
__device__ __forceinline__ bool readout_live(int n, int pidib, int dense) {
	return dense ? pidib < n : (pidib & 63) < slice_records_at(n, pidib & ~63);
}
// Position (cell units) of the particle in record `rec` of block (kx, ky, kz): the source bin the record's neighbour direction names.
__device__ __forceinline__ void readout_position(const GridCfg& cfg, int nch, int rec, int kx, int ky, int kz, const int* __restrict__ prev_table, const int* __restrict__ binoff_src, const float* __restrict__ bins_src, float p[3]) {
	int ox, oy, oz;
	dir_components((rec >> (cfg.pid_bits + kKeyBits)) & 31, ox, oy, oz);
	const int sp	 = rec & (cfg.ppb - 1);
	const int srcno	 = table_query(cfg, prev_table, kx + ox, ky + oy, kz + oz);
	const float* src = bins_src + (size_t) (binoff_src[srcno] + (sp >> 6)) * (kBin * nch) + (sp & 63) * rec_floats(nch);
	p[0] = src[0], p[1] = src[1], p[2] = src[2];
}
// G2P's gather at p (cell units) from the staged cube: v_p, and with kAffine A = sum_i w_ip v_i (x_i - x_p)^T in cell units (column-major).
template<bool kAffine>
__device__ __forceinline__ void readout_gather(const float4* s_v, const float p[3], float v[3], float A[9]) {
	int l[3];
	float w[3][3], fd[3];
#pragma unroll
	for(int d = 0; d < 3; ++d) {
		const int base = lround_pos(p[d]) - 1;
		fd[d]		   = p[d] - (float) base;
		bspline_weight_cells(fd[d], w[d]);
		l[d] = ((base - 1) & 3) + 1;// stencil base in the cube, as G2P forms it (1..4)
	}
	v[0] = v[1] = v[2] = 0.f;
	if(kAffine)
		for(int d = 0; d < 9; ++d) A[d] = 0.f;
#pragma unroll 1// (one x-slab of 9 nodes in flight at a time: 136 VGPRs fully unrolled, three waves per SIMD)
	for(int i = 0; i < 3; ++i)
#pragma unroll
		for(int j = 0; j < 3; ++j)
#pragma unroll
			for(int k = 0; k < 3; ++k) {
				const float4 nv = s_v[((l[0] + i) << 6) | ((l[1] + j) << 3) | (l[2] + k)];
				const float W	= w[0][i] * w[1][j] * w[2][k];
				const float r[3] = {(float) i - fd[0], (float) j - fd[1], (float) k - fd[2]};
				const float wv[3] = {W * nv.x, W * nv.y, W * nv.z};
#pragma unroll
				for(int a = 0; a < 3; ++a) {
					v[a] += wv[a];
					if(kAffine)
#pragma unroll
						for(int c = 0; c < 3; ++c) A[3 * c + a] = fmaf(wv[a], r[c], A[3 * c + a]);
				}
			}
}

__global__ __launch_bounds__(kReadoutThreads) void retrieve_velocity_kernel(GridCfg cfg, int nch, const int* __restrict__ cur_keys, const int* __restrict__ cur_table, const int* __restrict__ prev_table, const int* __restrict__ size, const int* __restrict__ row_of, const int* __restrict__ list_in, const int* __restrict__ binoff_src, const float* __restrict__ bins_src, const float* __restrict__ grid, float* xyz, float* vel, float* affine9, unsigned long long capacity, unsigned long long* counter, int dense) {
	__shared__ float4 s_v[512];// node (x, y, z) of the 8^3 cube at (x << 6) | (y << 3) | z, {vx, vy, vz, 0}
	__shared__ unsigned long long s_first;// the block's output range [s_first, s_first + n)
	__shared__ unsigned s_next;			  // slots of that range handed out so far
	const int b = blockIdx.x;
	const int n = size[b];
	if(n == 0) return;
	if(threadIdx.x == 0) {
		s_first = atomicAdd(counter, (unsigned long long) n);
		s_next	= 0u;
	}
	const int kx = cur_keys[3 * b], ky = cur_keys[3 * b + 1], kz = cur_keys[3 * b + 2];
	readout_stage_cube(cfg, cur_table, grid, kx, ky, kz, s_v);
	__syncthreads();
	const int* list	 = list_in + (size_t) row_of[b] * cfg.ppb;
	const float cdinv = cfg.d_inv * cfg.dx;// A is gathered in cell units: C = D^-1 A dx
	const int lane	 = threadIdx.x & 63;
	for(int pidib = threadIdx.x; pidib < ((n + 63) & ~63); pidib += kReadoutThreads) {
		// (the loop bound is a multiple of 64 and the stride of 256: every lane of a wave takes the same trips - the slot atomic below is per wave)
		const bool live = readout_live(n, pidib, dense);
		float p[3] = {0.f, 0.f, 0.f};
		if(live) readout_position(cfg, nch, list[pidib], kx, ky, kz, prev_table, binoff_src, bins_src, p);
		const unsigned long long live_mask = __ballot(live);
		if(live_mask == 0ull) continue;
		const int leader = __ffsll((long long) live_mask) - 1;
		unsigned first	 = 0;
		if(lane == leader) first = atomicAdd(&s_next, (unsigned) __popcll(live_mask));
		first = __shfl(first, leader);
		if(!live) continue;
		const unsigned rank = first + (unsigned) __popcll(live_mask & ((1ull << lane) - 1ull));
		const unsigned long long o = s_first + rank;
		if(rank >= (unsigned) n || o >= capacity) continue;// (the first never happens: the list holds n records)
		float v[3], A[9];
		readout_gather<true>(s_v, p, v, A);
		xyz[3 * o]	   = p[0] * cfg.dx;
		xyz[3 * o + 1] = p[1] * cfg.dx;
		xyz[3 * o + 2] = p[2] * cfg.dx;
		vel[3 * o]	   = v[0];
		vel[3 * o + 1] = v[1];
		vel[3 * o + 2] = v[2];
		if(affine9)
			for(int d = 0; d < 9; ++d) affine9[9 * o + d] = A[d] * cdinv;
	}
}

// Totals of the readout without per-particle output (mpm_particle_momentum): out[0..4] += {count, sum m v_p (3), sum 1/2 m |v_p|^2}
// over the model's particles, m = the model's particle mass.  Same walk, cube and gather as retrieve_velocity_kernel; each lane sums in
// float64, a wave folds its 64 lanes with __shfl_xor (DPP / ds_swizzle), the 4 waves meet in LDS, and ONE set of five float64 atomics
// per workgroup goes to global memory (global_atomic_add_f64; per-wave global atomics serialise, see above).  out must be zeroed by the
// caller; the order of the workgroups' atomics is unspecified, so the last bits of the sums may differ from run to run.
constexpr int kMomentumSums = 5;
__global__ __launch_bounds__(kReadoutThreads) void particle_momentum_kernel(GridCfg cfg, int nch, const int* __restrict__ cur_keys, const int* __restrict__ cur_table, const int* __restrict__ prev_table, const int* __restrict__ size, const int* __restrict__ row_of, const int* __restrict__ list_in, const int* __restrict__ binoff_src, const float* __restrict__ bins_src, const float* __restrict__ grid, double mass, double* out, int dense) {
	__shared__ float4 s_v[512];
	__shared__ double s_red[kReadoutThreads / 64][kMomentumSums];
	const int b = blockIdx.x;
	const int n = size[b];
	if(n == 0) return;
	const int kx = cur_keys[3 * b], ky = cur_keys[3 * b + 1], kz = cur_keys[3 * b + 2];
	readout_stage_cube(cfg, cur_table, grid, kx, ky, kz, s_v);
	__syncthreads();
	const int* list = list_in + (size_t) row_of[b] * cfg.ppb;
	double acc[kMomentumSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
	for(int pidib = threadIdx.x; pidib < ((n + 63) & ~63); pidib += kReadoutThreads) {
		if(!readout_live(n, pidib, dense)) continue;
		float p[3], v[3];
		readout_position(cfg, nch, list[pidib], kx, ky, kz, prev_table, binoff_src, bins_src, p);
		readout_gather<false>(s_v, p, v, nullptr);
		acc[0] += 1.0;
		acc[1] += (double) v[0];
		acc[2] += (double) v[1];
		acc[3] += (double) v[2];
		acc[4] += (double) v[0] * v[0] + (double) v[1] * v[1] + (double) v[2] * v[2];
	}
#pragma unroll
	for(int d = 0; d < kMomentumSums; ++d)
#pragma unroll
		for(int off = 32; off > 0; off >>= 1) acc[d] += __shfl_xor(acc[d], off);
	const int wave = threadIdx.x >> 6;
	if((threadIdx.x & 63) == 0)
		for(int d = 0; d < kMomentumSums; ++d) s_red[wave][d] = acc[d];
	__syncthreads();
	if(threadIdx.x < kMomentumSums) {
		double t = 0.0;
		for(int w = 0; w < kReadoutThreads / 64; ++w) t += s_red[w][threadIdx.x];
		const double scale = threadIdx.x == 0 ? 1.0 : threadIdx.x < 4 ? mass : 0.5 * mass;
		atomicAdd(out + threadIdx.x, t * scale);
	}
}

}// namespace mpm
