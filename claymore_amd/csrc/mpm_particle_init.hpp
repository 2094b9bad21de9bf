// mpm_particle_init.hpp — per-particle initial conditions (mpm_add_model_particles, mpm_set_model_velocity_field): the set-up kernels of a model
// that starts with its own velocity, APIC matrix or material state.  A model with none of these never comes here: mpm_initial_setup launches
// fill_bins_kernel and rasterize_blocks_kernel (mpm_kernels.hpp) for it exactly as before.  Nothing of the substep loop is touched.
//
// Group segments: validate_particle_init_kernel 0 B, fill_bins_state_kernel 0 B, rasterize_particles_kernel 8192 B (4 x 512 floats).
#pragma once
#include "mpm_kernels.hpp"

namespace mpm {

// what validate_particle_init_kernel found, one bit per reason
enum { kInitBadVelocity = 1, kInitBadAffine = 2, kInitBadState = 4, kInitBadLogJp = 8, kInitNotPositive = 16 };

// The per-particle arrays of a model, on the device (null: not given), in the order of the model's positions.
struct ParticleInit {
	const float* velocity = nullptr;// n * 3, world units
	const float* affine9  = nullptr;// n * 9, C_p column-major: [3 c + r] = C_rc (mpm_retrieve_velocity's layout)
	const float* state9	  = nullptr;// n * 9: b (state_f == 0, as mpm_retrieve_state returns it) or F (state_f == 1, mpm_test_stress's layout)
	const float* logjp	  = nullptr;// n
	int state_f			  = 0;
};
// v_p = v0 + G (x_p - pivot), C_p = G (column-major)
struct VelocityField {
	float v0[3], G[9], pivot[3];
};

// One row of state9 as the bins hold it: s = {b00 with the reflection mark in its sign, b11, b22, b10, b20, b21} for a solid, s[0] = J for the J-fluid.
__device__ __forceinline__ void particle_init_state(bool fluid, int state_f, const float* __restrict__ in, float (&s)[6]) {
	if(!state_f) {// stored verbatim: readout -> re-seed -> readout is bit for bit
		s[0] = in[0], s[1] = in[4], s[2] = in[8], s[3] = in[1], s[4] = in[2], s[5] = in[5];
		return;
	}
	float F[9];
#pragma unroll
	for(int d = 0; d < 9; ++d) F[d] = in[d];
	const float det = det3(F);
	if(fluid) {
		s[0] = det;
		s[1] = s[2] = s[3] = s[4] = s[5] = 0.f;
		return;
	}
	left_cauchy_green(F, s);
	if(det < 0.f) s[0] = -s[0];
}

// Finiteness of every array and positivity of the state: one pass, one flag word.  A wave that finds nothing writes nothing.
__global__ __launch_bounds__(256) void validate_particle_init_kernel(size_t n, bool fluid, ParticleInit a, int* flag) {
	int bad = 0;
	for(size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
		if(a.velocity)
			for(int d = 0; d < 3; ++d)
				if(!isfinite(a.velocity[3 * i + d])) bad |= kInitBadVelocity;
		if(a.affine9)
			for(int d = 0; d < 9; ++d)
				if(!isfinite(a.affine9[9 * i + d])) bad |= kInitBadAffine;
		if(a.logjp && !isfinite(a.logjp[i])) bad |= kInitBadLogJp;
		if(a.state9) {
			bool fin = true;
			for(int d = 0; d < 9; ++d) fin = fin && isfinite(a.state9[9 * i + d]);
			if(!fin)
				bad |= kInitBadState;
			else {
				float s[6];
				particle_init_state(fluid, a.state_f, a.state9 + 9 * i, s);
				const bool pos = fluid ? s[0] > 0.f : (fabsf(s[0]) > 0.f && s[1] > 0.f && s[2] > 0.f);
				if(!pos) bad |= kInitNotPositive;
			}
		}
	}
	if(bad) atomicOr(flag, bad);
}

// fill_bins_kernel's body (mpm_kernels.hpp: same record and row layout, same list records; the ids follow through fill_ids_kernel as there) with the
// material state taken from the arrays.  state9 null: the stress-free state; logjp null: log_jp0.
__global__ __launch_bounds__(256) void fill_bins_state_kernel(GridCfg cfg, int nch, float log_jp0, const float* __restrict__ xyz, const int* __restrict__ ids, const int* __restrict__ size, const int* __restrict__ binoff, float* bins, int* list_in, ParticleInit a) {
	const int b = blockIdx.x;
	const int n = size[b];
	for(int pidib = threadIdx.x; pidib < n; pidib += blockDim.x) {
		const size_t pid = (size_t) ids[(size_t) b * cfg.ppb + pidib];
		const int rec = rec_floats(nch), row = nch - rec;
		float* bin = bins + (size_t) (binoff[b] + (pidib >> 6)) * (kBin * nch);
		float* dst = bin + (pidib & 63) * rec;
		float s[6] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f};
		if(a.state9) particle_init_state(nch == 4, a.state_f, a.state9 + 9 * pid, s);
		dst[0] = xyz[3 * pid] * cfg.dx_inv;
		dst[1] = xyz[3 * pid + 1] * cfg.dx_inv;
		dst[2] = xyz[3 * pid + 2] * cfg.dx_inv;
		dst[3] = s[0];// J, or b00
		if(nch != 4) {
			dst[4] = s[1];// b11
			dst[5] = s[2];// b22
			dst[6] = s[3];// b10
			dst[7] = s[4];// b20
			bin[kBin * rec + (pidib & 63) * row] = s[5];// b21
			if(row == 2) bin[kBin * rec + (pidib & 63) * row + 1] = a.logjp ? a.logjp[pid] : log_jp0;
		}
		const int cx = node_index(xyz[3 * pid], cfg.dx_inv) - 2, cy = node_index(xyz[3 * pid + 1], cfg.dx_inv) - 2, cz = node_index(xyz[3 * pid + 2], cfg.dx_inv) - 2;
		const int key = (((cy & 3) + 1) * 6 + ((cx & 3) + 1)) * 6 + ((cz & 3) + 1);
		list_in[(size_t) b * cfg.ppb + pidib] = (kStay << (cfg.pid_bits + kKeyBits)) | (key << cfg.pid_bits) | pidib;
	}
}

// The per-particle counterpart of rasterize_blocks_kernel (mpm_kernels.hpp; the comment above it explains the node cube, node -1 of the lower faces
// and the blocks beyond the upper faces): one workgroup per particle block, FOUR LDS images of the 8^3 node cube - mass and the three momenta -,
// every touched node written back with one global atomic per channel.  A particle gives node i
//     m w_ip                           to the mass image and
//     m w_ip (v_p + C_p (x_i - x_p))   to the momentum images, x_i - x_p in world units.
// FIELD: v_p = v0 + G (x_p - pivot) and C_p = G come from the kernel argument (a second instantiation: the node loop holds no such branch); else from
// the arrays (velocity null: f.v0 for every particle; affine9 null: 0).
// Roundings of one momentum term, for the tests' bound (tests/test_particle_init_gpu.py counts the same statements):
//   d = (float) node - p: one rounding per axis, relative to d (both operands are exact), times dx (exact);
//   C d: three products, two additions; + v_p: one addition                                        -> 7 with d, relative to |v| + sum |C d|
//   w = w0 w1 w2: two products; m w: one; times the bracket: one                                   -> 4
//   each axis weight: the square and, for the middle one, 0.75 - square (at most 2 roundings relative to w >= 0.5); below node 1 of a lower face
//   p - base = p + 1 rounds too (node -1 is dropped, the other two weights then carry at most 5)    -> 3 x 5
// FIELD adds x_p - pivot (1), the three products and three additions of v0 + G (..)                 -> 7 more, relative to |v0| + sum |G (x - pivot)|.
template<bool FIELD>
__global__ __launch_bounds__(256) void rasterize_particles_kernel(GridCfg cfg, const float* __restrict__ xyz, const int* __restrict__ ids, const int* __restrict__ size, const int* __restrict__ keys, const int* __restrict__ table, float* grid, float mass, ParticleInit a, VelocityField f) {
	__shared__ float s_g[4][512];
	const int b = blockIdx.x;
	const int n = size[b];
	if(n == 0) return;
	const int kx = keys[3 * b], ky = keys[3 * b + 1], kz = keys[3 * b + 2];
	for(int i = threadIdx.x; i < 2048; i += 256) (&s_g[0][0])[i] = 0.f;
	__syncthreads();
	for(int pidib = threadIdx.x; pidib < n; pidib += 256) {
		const size_t pid = (size_t) ids[(size_t) b * cfg.ppb + pidib];
		int base[3];
		float w[3][3], dd[3][3], v[3], C[9];
#pragma unroll
		for(int d = 0; d < 3; ++d) {
			const float p = xyz[3 * pid + d] * cfg.dx_inv;
			base[d]		  = lround_pos(p) - 1;
			bspline_weight_cells(p - (float) base[d], w[d]);
#pragma unroll
			for(int i = 0; i < 3; ++i) dd[d][i] = ((float) (base[d] + i) - p) * cfg.dx;
		}
		if constexpr(FIELD) {
			const float r0 = xyz[3 * pid] - f.pivot[0], r1 = xyz[3 * pid + 1] - f.pivot[1], r2 = xyz[3 * pid + 2] - f.pivot[2];
#pragma unroll
			for(int r = 0; r < 3; ++r) v[r] = f.v0[r] + (f.G[r] * r0 + f.G[3 + r] * r1 + f.G[6 + r] * r2);
#pragma unroll
			for(int d = 0; d < 9; ++d) C[d] = f.G[d];
		} else {
#pragma unroll
			for(int r = 0; r < 3; ++r) v[r] = a.velocity ? a.velocity[3 * pid + r] : f.v0[r];
#pragma unroll
			for(int d = 0; d < 9; ++d) C[d] = a.affine9 ? a.affine9[9 * pid + d] : 0.f;
		}
		const int lx = base[0] - 4 * kx, ly = base[1] - 4 * ky, lz = base[2] - 4 * kz;// 1..4 inside the domain, -1 / 0 for cells -2 / -1
#pragma unroll
		for(int i = 0; i < 3; ++i)
#pragma unroll
			for(int j = 0; j < 3; ++j)
#pragma unroll
				for(int k = 0; k < 3; ++k)
					if((unsigned) (lx + i) < 8u && (unsigned) (ly + j) < 8u && (unsigned) (lz + k) < 8u) {
						const int at   = ((lx + i) << 6) | ((ly + j) << 3) | (lz + k);
						const float wm = mass * (w[0][i] * w[1][j] * w[2][k]);
						atomicAdd(&s_g[0][at], wm);
#pragma unroll
						for(int r = 0; r < 3; ++r) atomicAdd(&s_g[1 + r][at], wm * (v[r] + (C[r] * dd[0][i] + C[3 + r] * dd[1][j] + C[6 + r] * dd[2][k])));
					}
	}
	__syncthreads();
	for(int i = threadIdx.x; i < 512; i += 256) {
		const float m = s_g[0][i];
		if(m == 0.f) continue;
		const int x = i >> 6, y = (i >> 3) & 7, z = i & 7;
		const int bno = table_query(cfg, table, kx + (x >> 2), ky + (y >> 2), kz + (z >> 2));
		if(bno < 0) continue;
		float* g = grid + (size_t) bno * 256 + (x & 3) * 16 + (y & 3) * 4 + (z & 3);
		unsafeAtomicAdd(g, m);
#pragma unroll
		for(int r = 0; r < 3; ++r) {
			const float q = s_g[1 + r][i];
			if(q != 0.f) unsafeAtomicAdd(g + 64 * (1 + r), q);
		}
	}
}

}// namespace mpm
