// mpm_readout.hpp - every readout of a model's particles, one walk of each particle block's list (readout_kernel<K>):
//   kReadState     x, the 9-float state and log Jp (output_model, gmpm_simulator.cuh:594-634; the reference's retrieve_particle_buffer,
//                  mgmpm_kernels.cuh:1087-1122, copies x only) - from the record and row alone, whatever the grid holds
//   kReadVelocity  x, v_p and C_p (an extension: G2P2G is fused, so they exist only in registers of the substep kernels), gathered again the
//                  way G2P does from grid[0], the mass m_i and momentum p_i of the last P2G
//   kReadMomentum  {count, sum m v_p, sum 1/2 m |v_p|^2} of the same gather, summed instead of written
//   v_i = p_i / m_i (m_i > 0, else 0)   - the state BEFORE the next grid update: no gravity, walls or collision object
//   v_p = sum_i w_ip v_i                - 27-node quadratic B-spline stencil, base node and weights those of G2P (lround_pos, bspline_weight_cells)
//   C_p = D^-1 sum_i w_ip v_i (x_i - x_p)^T, D^-1 = 4 / dx^2, column-major: C[3 * c + r] = C_rc (G2P2G's A, mpm_g2p2g.hpp)
//   kReadStress    x, the Cauchy stress and {J, pressure, von Mises} (an extension: the stress exists only in registers of the substep
//                  kernels): the model's stress function on the stored state with a zero velocity gradient (readout_stress below,
//                  INTEGRATION.md section 5) - from the record and row alone, like kReadState; it writes no bin
//   kReadStressTotals  {count, sum V0 tau (6), max von Mises} of the same evaluation, reduced instead of written
//   kReadIds       x and the particle's identity (an extension, tracked contexts only: mpm_particle_ids.hpp): kReadState's walk, the id read
//                  from the side array at the record's source slot
// One workgroup (256 lanes) per particle block.  The gathers stage the 2x2x2 grid blocks the block's stencils reach once in LDS as
// velocities (8 KiB; a block that is not registered, or beyond an upper face, stages zero) and read each particle's 27 nodes from there at
// G2P's cube-local stencil base ((base - 1) & 3) + 1, which also gives particles of cells -2 / -1 the reference's wrapped key.  Output
// slots: ONE global atomic per workgroup reserves the block's n slots (its list holds exactly n records), its waves take theirs from an
// LDS counter; all outputs of a particle share its slot, and the slot order is unspecified.
#pragma once
#include "mpm_kernels.hpp"

namespace mpm {

constexpr int kReadoutThreads = 256;
constexpr int kMomentumSums	  = 5;
constexpr int kStressSums	  = 7;// count and the six sums; the maximum is an eighth word of its own

enum ReadoutKind { kReadState, kReadVelocity, kReadMomentum, kReadStress, kReadStressTotals, kReadIds };

// What every readout reads of a model: the block numberings, the list and the bins (make_readout_args, claymore_hip.hip).
struct ReadoutArgs {
	GridCfg cfg;
	int nch;			  // floats per particle in a bin
	int dense;			  // the pair list layout (no holes), else the sliced one
	const int* cur_keys;  // [block][3], current numbering
	const int* cur_table; // current numbering (the staged grid blocks)
	const int* prev_table;// the numbering the bins are laid out in
	const int* size;	  // particles per current block
	const int* row_of;	  // row of `list` that belongs to current block b
	const int* list;	  // advection records, cfg.ppb per row
	const int* binoff;	  // first bin of a block, previous numbering
	const float* bins;
	const int* ids;		  // kReadIds: one id per bin slot, addressed like the bins (null in an untracked context)
};

// Where a readout puts its result.  kReadState / kReadVelocity / kReadStress: slot o of col[c] holds kReadoutWidth[K][c] floats of one
// particle - col[0] x (never null), then state9 and log Jp, or v and C, or stress6 and scalars3; a null column is not written -, slots at or
// beyond `capacity` are dropped, and *counter (zeroed by the caller) ends at the number of particles.  kReadMomentum: sums[0..4] (zeroed by
// the caller) += the totals, weight = the particle mass.  kReadStressTotals: sums[0..6] += {count, sum V0 tau}, weight = the particle volume
// V0, and the first 32 bits of sums[7] (zeroed too) take the float32 bit pattern of the largest von Mises stress by an integer atomicMax
// (q >= 0: the patterns order as the values do).  The stress kinds read the model's material and constants from here.
struct ReadoutOut {
	float* col[3];
	unsigned long long capacity;
	unsigned long long* counter;
	double weight;
	double* sums;
	int material;
	MaterialConst mc;
	int* ids = nullptr;// kReadIds: slot o takes the particle's id
};
constexpr int kReadoutWidth[6][3] = {{3, 9, 1}, {3, 3, 9}, {0, 0, 0}, {3, 6, 3}, {0, 0, 0}, {3, 1, 0}};// (kReadIds: column 1 is the int32 id, ReadoutOut::ids)

// The pieces the readouts share - the list walk's liveness test, the record fetch, the cube staging and the 27-node gather - so that the
// list layouts, the record format and the stencil, tie and face rules live in one place.
// Whether slot pidib of a list of n records holds a particle (a hole of the sliced list layout does not; the pair layout has none).
__device__ __forceinline__ bool readout_live(int n, int pidib, int dense) {
	return dense ? pidib < n : (pidib & 63) < slice_records_at(n, pidib & ~63);
}
// Position (cell units) of the particle in record `rec` of block (kx, ky, kz), from the source bin the record's neighbour direction names.
// Returns the particle's record (x, y, z, then J or five entries of b) and sets *row to its row (b21, log Jp; mpm_g2p2g.hpp); *slot (if
// asked for): the particle's slot in the source bins, 64 per bin.
__device__ __forceinline__ const float* readout_position(const ReadoutArgs& a, int rec, int kx, int ky, int kz, float p[3], const float** row, size_t* slot = nullptr) {
	int ox, oy, oz;
	dir_components((rec >> (a.cfg.pid_bits + kKeyBits)) & 31, ox, oy, oz);
	const int sp	 = rec & (a.cfg.ppb - 1);
	const int srcno	 = table_query(a.cfg, a.prev_table, kx + ox, ky + oy, kz + oz);
	const int recf	 = rec_floats(a.nch);
	const float* bin = a.bins + (size_t) (a.binoff[srcno] + (sp >> 6)) * (kBin * a.nch);
	const float* src = bin + (sp & 63) * recf;
	*row			 = bin + kBin * recf + (sp & 63) * (a.nch - recf);
	if(slot) *slot = (size_t) (a.binoff[srcno] + (sp >> 6)) * kBin + (sp & 63);
	p[0] = src[0], p[1] = src[1], p[2] = src[2];
	return src;
}
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

// What the stress readouts report of one stored particle (record `src`, row `row` of readout_position): tau = P F^T per unit reference
// volume as {xx, yy, zz, xy, xz, yz} (sym_expand's six-vector) and J = det F of the state tau belongs to.
//   solids   the model's stress function (mpm_device_math.hpp) with StressScale {2 mu, lambda, 1} on b decoded as G2P2G decodes it (|b00|,
//            the reflection mark in its sign, log Jp from the row) - i.e. compute_stress with a zero velocity gradient.  The projected b and
//            log Jp that SAND and NACC hand back stay in registers and are dropped: J is the one of the projected state, as tau is.
//   J-fluid  p = bulk (J^-gamma - 1), tau = -J p I: the Tait pressure alone.  The viscous part, viscosity (C_p + C_p^T), needs the velocity
//            gradient, which lives on the grid (kReadVelocity's C_p and its preconditions).
// The material is uniform over the launch: a scalar branch, each arm with its own register allocation (the kernel gets the largest).
// The stress functions vote across the wave (the undeformed early exit, __any(refl), the sweeps of sym_eig3): this is called after the walk
// has dropped its dead lanes, so the votes run over live lanes only, and a live lane's result does not depend on its neighbours - the
// early exits return exactly what the general path gives for b = I, and sym_eig3 rotates a lane by the lane's own verdict.
__device__ __forceinline__ void readout_stress(int material, const MaterialConst& mc, const float* src, const float* row, float (&tau)[6], float& J) {
	float txx, tyy, tzz, txy = 0.f, txz = 0.f, tyz = 0.f, det;// (scalars, not tau[]: see readout_cauchy)
	if(material == 0) {
		det			  = src[3];
		const float p = mc.bulk * (__builtin_amdgcn_exp2f(-mc.gamma * __builtin_amdgcn_logf(det)) - 1.f);// J^-gamma as stress_jfluid forms it
		txx = tyy = tzz = -det * p;
	} else {
		const StressScale ss {2.0f * mc.mu, mc.lambda, 1.0f};
		NoHook nh;
		float b[6] = {fabsf(src[3]), src[4], src[5], src[6], src[7], row[0]}, PF[9];
		bool refl  = (__float_as_uint(src[3]) & kReflBit) != 0u;
		if(material == 1) {
			stress_fixed_corotated<0>(ss, b, refl, PF, nh, &det);
		} else {
			float lj = row[1];
			if(material == 2)
				stress_sand<0>(mc, ss, b, refl, lj, PF, nh, &det);
			else
				stress_nacc<0>(mc, ss, b, refl, lj, PF, nh, &det);
		}
		txx = PF[0], tyy = PF[4], tzz = PF[8], txy = PF[1], txz = PF[2], tyz = PF[5];
	}
	tau[0] = txx, tau[1] = tyy, tau[2] = tzz, tau[3] = txy, tau[4] = txz, tau[5] = tyz;
	J = det;
}
// Cauchy stress sigma = tau / J and {J, pressure = -tr sigma / 3, von Mises q = sqrt(3/2 dev sigma : dev sigma)}.  Both stress kinds call
// this, and the largest q of kReadStressTotals equals the largest q kReadStress wrote bit for bit: so the roundings are spelled out
// (IEEE division, no contraction the compiler could choose differently in two kernels).  (tau[] is written once, after the material branch,
// and the arrays of the stress readouts are indexed by constants only: written in each arm, the compiler merged the arms' stores into one
// with a variable index and kept three entries of tau in scratch.)
__device__ __forceinline__ void readout_cauchy(const float (&tau)[6], float J, float (&sigma)[6], float (&scal)[3]) {
#pragma clang fp contract(off)
	sigma[0] = __fdiv_rn(tau[0], J), sigma[1] = __fdiv_rn(tau[1], J), sigma[2] = __fdiv_rn(tau[2], J);
	sigma[3] = __fdiv_rn(tau[3], J), sigma[4] = __fdiv_rn(tau[4], J), sigma[5] = __fdiv_rn(tau[5], J);
	const float mean = (sigma[0] + sigma[1] + sigma[2]) * (1.0f / 3.0f);
	const float d0 = sigma[0] - mean, d1 = sigma[1] - mean, d2 = sigma[2] - mean;
	const float dd = (d0 * d0 + d1 * d1 + d2 * d2) + 2.0f * (sigma[3] * sigma[3] + sigma[4] * sigma[4] + sigma[5] * sigma[5]);
	scal[0]		   = J;
	scal[1]		   = -mean;
	scal[2]		   = __fsqrt_rn(1.5f * dd);
}

// One workgroup per particle block; the walk's bound is a multiple of 64 and its stride 256, so every lane of a wave takes the same trips
// (the slot counter is taken per wave).  kReadMomentum: each lane sums in float64, a wave folds its 64 lanes with __shfl_xor (DPP /
// ds_swizzle), the 4 waves meet in LDS, and ONE set of five float64 atomics per workgroup goes to global memory (global_atomic_add_f64);
// the order of the workgroups' atomics is unspecified, so the last bits of the sums may differ from run to run.  kReadStressTotals sums
// the same way (seven float64) and carries the largest q as a float32 bit pattern: wave fold, integer atomicMax in LDS, one in global memory.
template<ReadoutKind K>
__global__ __launch_bounds__(kReadoutThreads) void readout_kernel(ReadoutArgs a, const float* __restrict__ grid, ReadoutOut out) {
	constexpr bool kGrid  = K == kReadVelocity || K == kReadMomentum;// (the state and stress readouts neither stage nor read the grid)
	constexpr bool kSlots = K != kReadMomentum && K != kReadStressTotals;// per-particle output (else: totals)
	constexpr int kSums	  = K == kReadStressTotals ? kStressSums : kMomentumSums;
	__shared__ float4 s_v[kGrid ? 512 : 1];// node (x, y, z) of the 8^3 cube at (x << 6) | (y << 3) | z, {vx, vy, vz, 0}
	__shared__ unsigned long long s_first;// the block's output range [s_first, s_first + n)
	__shared__ unsigned s_next;			  // slots of that range handed out so far
	__shared__ double s_red[kReadoutThreads / 64][kSums];
	__shared__ unsigned s_qmax;// kReadStressTotals: the block's largest q (bit pattern)
	const int b = blockIdx.x;
	const int n = a.size[b];
	if(n == 0) return;
	// (the block's scalars are loaded before the first global store, the slot atomic: so the compiler knows them uniform and unclobbered)
	const int kx = a.cur_keys[3 * b], ky = a.cur_keys[3 * b + 1], kz = a.cur_keys[3 * b + 2];
	const int* list = a.list + (size_t) a.row_of[b] * a.cfg.ppb;
	if(kSlots && threadIdx.x == 0) {
		s_first = atomicAdd(out.counter, (unsigned long long) n);
		s_next	= 0u;
	}
	if(K == kReadStressTotals && threadIdx.x == 0) s_qmax = 0u;
	if constexpr(kGrid) readout_stage_cube(a.cfg, a.cur_table, grid, kx, ky, kz, s_v);
	__syncthreads();
	double acc[kSums] = {};
	float qmax		  = 0.f;
	for(int pidib = threadIdx.x; pidib < ((n + 63) & ~63); pidib += kReadoutThreads) {
		const bool live = readout_live(n, pidib, a.dense);
		if(!kSlots && !live) continue;// (no slots: the lanes of a wave need not agree)
		float p[3]		 = {0.f, 0.f, 0.f};
		const float *src = nullptr, *row = nullptr;
		size_t sslot	 = 0;
		if(live) src = readout_position(a, list[pidib], kx, ky, kz, p, &row, K == kReadIds ? &sslot : nullptr);
		if constexpr(K == kReadMomentum) {
			float v[3];
			readout_gather<false>(s_v, p, v, nullptr);
			acc[0] += 1.0;
			acc[1] += (double) v[0];
			acc[2] += (double) v[1];
			acc[3] += (double) v[2];
			acc[4] += (double) v[0] * v[0] + (double) v[1] * v[1] + (double) v[2] * v[2];
		} else if constexpr(K == kReadStressTotals) {
			float tau[6], sigma[6], scal[3], J;
			readout_stress(out.material, out.mc, src, row, tau, J);
			readout_cauchy(tau, J, sigma, scal);
			acc[0] += 1.0;
			acc[1] += (double) tau[0], acc[2] += (double) tau[1], acc[3] += (double) tau[2];
			acc[4] += (double) tau[3], acc[5] += (double) tau[4], acc[6] += (double) tau[5];
			qmax = fmaxf(qmax, scal[2]);
		} else {
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
			if(rank >= (unsigned) n || o >= out.capacity) continue;// (the first never happens: the list holds n records)
			float* xyz	   = out.col[0];
			xyz[3 * o]	   = p[0] * a.cfg.dx;// (stored in cell units)
			xyz[3 * o + 1] = p[1] * a.cfg.dx;
			xyz[3 * o + 2] = p[2] * a.cfg.dx;
			if constexpr(K == kReadState) {
				float *state9 = out.col[1], *logjp = out.col[2];
				if(state9) {
					if(a.nch == 4) {
						state9[9 * o] = src[3];
						for(int d = 1; d < 9; ++d) state9[9 * o + d] = 0.f;
					} else {// b = F F^T as a full symmetric matrix (the sign of b00 marks a reflected F: reported as it is stored)
						const float s6[6] = {src[3], src[4], src[5], src[6], src[7], row[0]};
						float m[9];
						sym_expand(s6, m);
						for(int d = 0; d < 9; ++d) state9[9 * o + d] = m[d];
					}
				}
				if(logjp) logjp[o] = a.nch - rec_floats(a.nch) == 2 ? row[1] : 0.f;
			} else if constexpr(K == kReadIds) {
				out.ids[o] = a.ids[sslot];
			} else if constexpr(K == kReadStress) {
				float *stress6 = out.col[1], *scalars3 = out.col[2];
				float tau[6], sigma[6], scal[3], J;
				readout_stress(out.material, out.mc, src, row, tau, J);
				readout_cauchy(tau, J, sigma, scal);
				if(stress6) {
					float* s = stress6 + 6 * o;
					s[0] = sigma[0], s[1] = sigma[1], s[2] = sigma[2], s[3] = sigma[3], s[4] = sigma[4], s[5] = sigma[5];
				}
				if(scalars3) {
					float* s = scalars3 + 3 * o;
					s[0] = scal[0], s[1] = scal[1], s[2] = scal[2];
				}
			} else {
				float *vel = out.col[1], *affine9 = out.col[2];
				const float cdinv = a.cfg.d_inv * a.cfg.dx;// A is gathered in cell units: C = D^-1 A dx
				float v[3], A[9];
				readout_gather<true>(s_v, p, v, A);
				vel[3 * o]	   = v[0];
				vel[3 * o + 1] = v[1];
				vel[3 * o + 2] = v[2];
				if(affine9)
					for(int d = 0; d < 9; ++d) affine9[9 * o + d] = A[d] * cdinv;
			}
		}
	}
	if constexpr(!kSlots) {
#pragma unroll
		for(int d = 0; d < kSums; ++d)
#pragma unroll
			for(int off = 32; off > 0; off >>= 1) acc[d] += __shfl_xor(acc[d], off);
		if constexpr(K == kReadStressTotals) {
#pragma unroll
			for(int off = 32; off > 0; off >>= 1) qmax = fmaxf(qmax, __shfl_xor(qmax, off));
		}
		if((threadIdx.x & 63) == 0) {
			for(int d = 0; d < kSums; ++d) s_red[threadIdx.x >> 6][d] = acc[d];
			if(K == kReadStressTotals) atomicMax(&s_qmax, __float_as_uint(qmax));
		}
		__syncthreads();
		if(threadIdx.x < kSums) {
			double t = 0.0;
			for(int w = 0; w < kReadoutThreads / 64; ++w) t += s_red[w][threadIdx.x];
			const double scale = threadIdx.x == 0 ? 1.0 : K == kReadStressTotals || threadIdx.x < 4 ? out.weight : 0.5 * out.weight;
			atomicAdd(out.sums + threadIdx.x, t * scale);
		}
		if(K == kReadStressTotals && threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(out.sums + kStressSums), s_qmax);
	}
}

}// namespace mpm
