// mpm_mesh_fill.hpp — a closed triangle mesh filled with particles on the reference's lattice (mpm_sample_mesh, mpm_add_model_mesh).
//
// "Inside the mesh" is the sign of the field mpm_collision_mesh.hpp defines, evaluated at the lattice's candidates instead of at the nodes;
// the hits are compacted in a fixed order - it is the particle's id - without atomics.  Three parts, as in mpm_collision_mesh.hpp:
//   1. the definition - the candidate lattice, the clip rule mesh_fill_range, the order - in plain C++ that builds on x86 too;
//      mesh_fill_host restates the whole sampler per point (claymore_amd/host/host_selftest.cpp --mesh-fill, tests/mesh_fill_model.py in NumPy);
//   2. the kernels (HIP only): classify (one wave per 4 x 4 x 4 node tile, on mpm_collision_mesh.hpp's tile walk), an exclusive scan of the
//      tile counts, emit;
//   3. the host routine is in claymore_hip.hip (mesh_fill_count / mesh_fill_emit): both entry points run the same kernels.
// The definition is in include/claymore_amd.h and INTEGRATION.md section 5.
#pragma once
#include "mpm_collision_mesh.hpp"

namespace mpm {

// The candidate lattice: node i carries, per axis, the coordinates ((float) i -+ 0.25f) dx - exact in float32, dx being a power of two and
// i < 2^10 -, so 8 candidates per node, numbered k = 4 a + 2 b + c with a / b / c = 0 for -0.25 and 1 for +0.25 on x / y / z.
MPM_DEV float mesh_fill_coord(int node, int plus, float dx) {
	return ((float) node + (plus ? 0.25f : -0.25f)) * dx;
}

// The nodes that are looked at: lo <= (i, j, k) < hi, the caller's box (default [0, N)^3) cut down to the nodes that can carry a candidate
// within the mesh's bounding box [mn, mx]: a coordinate (i -+ 0.25) dx lies in it only if (i + 0.25) dx >= mn and (i - 0.25) dx <= mx,
// so only if floor(mn N) <= i <= floor(mx N) + 1 (float64 on the float32 vertices: exact).  The cut changes no result - a point
// outside the bounding box is outside the mesh - only the work.  Tiles are those of the domain (node >> 2), tlo + [0, tn) per axis.
struct MeshFillRange {
	int lo[3], hi[3];
	int tlo[3], tn[3];
};
// false: the caller's box leaves [0, N] (the call is refused)
inline bool mesh_fill_range(int N, const float* verts, size_t nv, const int* box_lo, const int* box_hi, MeshFillRange& r) {
	for(int d = 0; d < 3; ++d) {
		int lo = box_lo ? box_lo[d] : 0, hi = box_hi ? box_hi[d] : N;
		if(lo < 0 || lo > N || hi < 0 || hi > N) return false;
		double mn = INFINITY, mx = -INFINITY;
		for(size_t i = 0; i < nv; ++i) {
			mn = std::min(mn, (double) verts[3 * i + d]);
			mx = std::max(mx, (double) verts[3 * i + d]);
		}
		const double a = std::floor(mn * (double) N), b = std::floor(mx * (double) N) + 2.;
		lo = std::max(lo, (int) std::min(std::max(a, 0.), (double) N));
		hi = std::min(hi, (int) std::min(std::max(b, 0.), (double) N));
		if(hi < lo) hi = lo;
		r.lo[d]	 = lo;
		r.hi[d]	 = hi;
		r.tlo[d] = lo >> 2;
		r.tn[d]	 = hi > lo ? ((hi + 3) >> 2) - (lo >> 2) : 0;
	}
	if(!r.tn[0] || !r.tn[1] || !r.tn[2]) r.tn[0] = r.tn[1] = r.tn[2] = 0;
	return true;
}

#if !defined(__HIPCC__)
// x86 builds only: the sampler per point, no tiles culled and nothing taken from a tile's centre.  Order: tiles ascending (x slowest, z
// fastest), nodes of a tile in lane order (x 4 + y) 4 + z, candidates k = 0 .. 7; inside(p) <=> sdis(p) < -margin.
inline void mesh_fill_host(const std::vector<MeshTri>& rec, const std::vector<MeshPseudo>& pseudo, int N, const MeshFillRange& r, float margin, std::vector<float>& xyz) {
	const float dx = 1.f / (float) N;
	xyz.clear();
	for(int tx = r.tlo[0]; tx < r.tlo[0] + r.tn[0]; ++tx)
		for(int ty = r.tlo[1]; ty < r.tlo[1] + r.tn[1]; ++ty)
			for(int tz = r.tlo[2]; tz < r.tlo[2] + r.tn[2]; ++tz)
				for(int lane = 0; lane < 64; ++lane) {
					const int node[3] = {4 * tx + (lane >> 4), 4 * ty + ((lane >> 2) & 3), 4 * tz + (lane & 3)};
					bool live		  = true;
					for(int d = 0; d < 3; ++d) live = live && node[d] >= r.lo[d] && node[d] < r.hi[d];
					if(!live) continue;
					for(int k = 0; k < 8; ++k) {
						const float p[3] = {mesh_fill_coord(node[0], k & 4, dx), mesh_fill_coord(node[1], k & 2, dx), mesh_fill_coord(node[2], k & 1, dx)};
						float out[4], q;
						int feature;
						mesh_point_query(rec, pseudo, p, 0, out, feature, q);
						if(out[0] < -margin) xyz.insert(xyz.end(), p, p + 3);
					}
				}
}
#endif

#if defined(__HIPCC__)
// ---- the kernels -----------------------------------------------------------------------------------------------------------------------
struct MeshFillArgs {
	float dx, slack, margin;
	int lo[3], hi[3];  // the clipped node range
	int tlo[3], tn[3]; // its tiles
};

// Classify.  One wave (a 64-thread block) per tile of the clipped range, one node per lane as in collision_mesh_table_kernel, and the same
// three steps - mpm_collision_mesh.hpp's walk: mesh_centre_bound, mesh_sweep_candidates, mesh_walk_chunk; the argument is written there -
// with the node replaced by its 8 candidates:
//   1. Bound.  q at the tile's centre over all triangles, a wave-min with the lowest index among equals: D = sqrtf(min q) and T(centre).
//      Every candidate of the tile is within r = (1.5 + 0.25) sqrt(3) dx of the centre: the nodes' half diagonal plus the candidates' offset.
//   2. Candidates, once per tile.  A triangle nearest to a candidate is within D + 2 r of the centre; the test, its float32 safety margin
//      (thr = (D + 2 r) (1 + 2^-6) + slack) and the index-ordered compaction into an LDS chunk are the field kernel's.  Each lane walks the
//      chunk for its 8 candidates in turn (k is a run-time loop: the walk's code exists once) and keeps 8 (q, T) pairs in registers - read
//      and written through select chains, never by a run-time index, so nothing goes to scratch.
//   3. Rule.  mesh_field_value at each candidate with its winner; bit k of the lane's mask = sdis < -margin.  A node outside the clip
//      range keeps mask 0.  The 64 masks (one byte a lane) and their popcount's wave sum go to global memory.
// Shortcut for tiles away from the surface.  If D > r + margin, no candidate p of the tile is within margin of the surface
// (dist(p) >= D - |p - centre| >= D - r > margin), and the segment from the centre to p stays at distance > 0 from it, so p lies on the
// centre's side: inside(p) = inside(centre) for all 512 candidates, and because |sdis(p)| > margin, sdis(p) < -margin <=> p is inside.  The tile then
// takes one mesh_field_value at the centre with T(centre) of step 1 and skips steps 2 and 3.  The test is made on float32 values with
// the field kernel's style of margin: D > (r + margin) (1 + 2^-6) + slack, slack = max(dx / 4, 2^-12 max |coordinate|) - the walk's error
// is a few ulps of a coordinate, the slack thousands.  The sign at the centre is the pseudonormal's, as everywhere; D > 3 dx away from the
// surface it is decided by a wide margin for any mesh whose candidates' signs are.
// Budget.  LDS: kMeshChunk x (48 B record + 4 B index) = 6.5 KiB per block, no scratch (tests/test_mesh_fill_isa.py checks both).  One
// atomic per shortcut tile, on a statistics counter only: placement uses none.
constexpr float kMeshFillRadius = 3.031088913f;// 1.75 sqrt(3), in cells

__global__ __launch_bounds__(64) void mesh_fill_classify_kernel(const MeshTri* __restrict__ tris, const MeshPseudo* __restrict__ pseudo, int nt, MeshFillArgs a, unsigned char* __restrict__ masks,
																 unsigned* __restrict__ counts, unsigned long long* __restrict__ shortcuts) {
	__shared__ float4 s_rec[kMeshChunk * 3];
	__shared__ int s_idx[kMeshChunk];
	const int lane	= (int) threadIdx.x;
	const float dx	= a.dx;
	const unsigned tz = blockIdx.x % (unsigned) a.tn[2], ty = (blockIdx.x / (unsigned) a.tn[2]) % (unsigned) a.tn[1], tx = blockIdx.x / ((unsigned) a.tn[2] * (unsigned) a.tn[1]);
	const int base3[3] = {4 * (a.tlo[0] + (int) tx), 4 * (a.tlo[1] + (int) ty), 4 * (a.tlo[2] + (int) tz)};
	const int node[3]  = {base3[0] + (lane >> 4), base3[1] + ((lane >> 2) & 3), base3[2] + (lane & 3)};
	const bool live	   = node[0] >= a.lo[0] && node[0] < a.hi[0] && node[1] >= a.lo[1] && node[1] < a.hi[1] && node[2] >= a.lo[2] && node[2] < a.hi[2];
	const float centre[3] = {((float) base3[0] + 1.5f) * dx, ((float) base3[1] + 1.5f) * dx, ((float) base3[2] + 1.5f) * dx};
	const float px0 = mesh_fill_coord(node[0], 0, dx), px1 = mesh_fill_coord(node[0], 1, dx);
	const float py0 = mesh_fill_coord(node[1], 0, dx), py1 = mesh_fill_coord(node[1], 1, dx);
	const float pz0 = mesh_fill_coord(node[2], 0, dx), pz1 = mesh_fill_coord(node[2], 1, dx);
	const float4* tris4 = reinterpret_cast<const float4*>(tris);
	unsigned mask = 0;
	// 1. bound, and the centre's nearest triangle
	int tmin;
	const float D = sqrtf(mesh_centre_bound(tris4, nt, lane, centre, tmin));
	const float r = kMeshFillRadius * dx;
	if(D > (r + a.margin) * 1.015625f + a.slack) {// wave-uniform: the tile is all in or all out
		MeshTri win;
		mesh_load_tri(tris4 + 3 * (size_t) tmin, win);
		float out[4], q;
		int feature;
		mesh_field_value(win, pseudo[tmin], centre, 0, out, feature, q);
		mask = live && out[0] < -a.margin ? 0xFFu : 0u;
		if(lane == 0) atomicAdd(shortcuts, 1ull);
	} else {
		// 2. candidates
		float best_q[8];
		int best_t[8];
		MPM_MESH_UNROLL
		for(int j = 0; j < 8; ++j) best_q[j] = INFINITY, best_t[j] = 0;
		mesh_sweep_candidates(tris4, nt, lane, centre, mesh_threshold2(D, r, a.slack), s_rec, s_idx, [&](int fill) {
			_Pragma("unroll 1") for(int k = 0; k < 8; ++k) {
				const float p[3] = {k & 4 ? px1 : px0, k & 2 ? py1 : py0, k & 1 ? pz1 : pz0};
				float bq		 = best_q[0];
				int bt			 = best_t[0];
				MPM_MESH_UNROLL
				for(int j = 1; j < 8; ++j) bq = k == j ? best_q[j] : bq, bt = k == j ? best_t[j] : bt;
				mesh_walk_chunk(s_rec, s_idx, fill, p, bq, bt);
				MPM_MESH_UNROLL
				for(int j = 0; j < 8; ++j) best_q[j] = k == j ? bq : best_q[j], best_t[j] = k == j ? bt : best_t[j];
			}
		});
		// 3. rule
		_Pragma("unroll 1") for(int k = 0; k < 8; ++k) {
			const float p[3] = {k & 4 ? px1 : px0, k & 2 ? py1 : py0, k & 1 ? pz1 : pz0};
			int bt			 = best_t[0];
			MPM_MESH_UNROLL
			for(int j = 1; j < 8; ++j) bt = k == j ? best_t[j] : bt;
			MeshTri win;
			mesh_load_tri(tris4 + 3 * (size_t) bt, win);
			float out[4], q;
			int feature;
			mesh_field_value(win, pseudo[bt], p, 0, out, feature, q);
			if(live && out[0] < -a.margin) mask |= 1u << k;
		}
	}
	masks[(size_t) blockIdx.x * 64 + (size_t) lane] = (unsigned char) mask;
	unsigned n = (unsigned) __popc(mask);
	for(int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
	if(lane == 0) counts[blockIdx.x] = n;
}

// Scan of the tile counts, exclusive, in two levels; no atomics, so the offsets are the order.
//   block level: 256 threads x 4 tiles; counts[] becomes each tile's offset within its group of kMeshFillGroup tiles (at most 2^19, 32 bits),
//     bsum[] the group's total.  LDS: one word per wave, 16 B.
//   top level: one block of 1024 threads walks bsum[] 1024 groups at a time with a running carry; boff[g] is the group's offset in 64 bits
//     (bits 10: up to 2^33 points), boff[ngroups] the total - the one value the host reads before it allocates.  LDS: 16 x 8 B = 128 B.
constexpr int kMeshFillGroup = 1024;

__global__ __launch_bounds__(256) void mesh_fill_scan_block_kernel(unsigned* __restrict__ counts, unsigned ntiles, unsigned* __restrict__ bsum) {
	__shared__ unsigned s_wave[4];
	const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned base = (blockIdx.x * 256u + threadIdx.x) * 4u;
	unsigned c[4], sum = 0;
	MPM_MESH_UNROLL
	for(unsigned j = 0; j < 4; ++j) {
		c[j] = base + j < ntiles ? counts[base + j] : 0u;
		sum += c[j];
	}
	unsigned inc = sum;
	for(unsigned off = 1; off < 64; off <<= 1) {
		const unsigned v = __shfl_up(inc, off);
		if(lane >= off) inc += v;
	}
	if(lane == 63) s_wave[wave] = inc;
	__syncthreads();
	unsigned before = 0;
	MPM_MESH_UNROLL
	for(unsigned w = 0; w < 4; ++w) before += w < wave ? s_wave[w] : 0u;
	unsigned ex = before + inc - sum;
	MPM_MESH_UNROLL
	for(unsigned j = 0; j < 4; ++j) {
		if(base + j < ntiles) counts[base + j] = ex;
		ex += c[j];
	}
	if(threadIdx.x == 255) bsum[blockIdx.x] = before + inc;
}

__global__ __launch_bounds__(1024) void mesh_fill_scan_top_kernel(const unsigned* __restrict__ bsum, unsigned ngroups, unsigned long long* __restrict__ boff) {
	__shared__ unsigned long long s_wave[16];
	const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	unsigned long long carry = 0;// the same in every thread
	for(unsigned base = 0; base < ngroups; base += 1024) {
		const unsigned i		   = base + threadIdx.x;
		const unsigned long long v = i < ngroups ? (unsigned long long) bsum[i] : 0ull;
		unsigned long long inc	   = v;
		for(unsigned off = 1; off < 64; off <<= 1) {
			const unsigned long long u = __shfl_up(inc, off);
			if(lane >= off) inc += u;
		}
		if(lane == 63) s_wave[wave] = inc;
		__syncthreads();
		unsigned long long before = 0, all = 0;
		MPM_MESH_UNROLL
		for(unsigned w = 0; w < 16; ++w) {
			before += w < wave ? s_wave[w] : 0ull;
			all += s_wave[w];
		}
		if(i < ngroups) boff[i] = carry + before + inc - v;
		carry += all;
		__syncthreads();
	}
	if(threadIdx.x == 0) boff[ngroups] = carry;
}

// Emit.  One wave per tile: a wave prefix sum of the lanes' popcounts, then each lane writes its up to 8 candidates consecutively from
// boff[group] + counts[tile] + prefix, k ascending.  capacity (points) is the size of xyz: the host passes the scanned total, and no write
// goes past it whatever the buffers hold.  No LDS.
__global__ __launch_bounds__(64) void mesh_fill_emit_kernel(const unsigned char* __restrict__ masks, const unsigned* __restrict__ offs, const unsigned long long* __restrict__ boff, MeshFillArgs a,
															 float* __restrict__ xyz, unsigned long long capacity) {
	const int lane		= (int) threadIdx.x;
	const unsigned mask = masks[(size_t) blockIdx.x * 64 + (size_t) lane];
	const unsigned n	= (unsigned) __popc(mask);
	unsigned inc		= n;
	for(int off = 1; off < 64; off <<= 1) {
		const unsigned v = __shfl_up(inc, off);
		if(lane >= off) inc += v;
	}
	if(!n) return;
	const unsigned tz = blockIdx.x % (unsigned) a.tn[2], ty = (blockIdx.x / (unsigned) a.tn[2]) % (unsigned) a.tn[1], tx = blockIdx.x / ((unsigned) a.tn[2] * (unsigned) a.tn[1]);
	const int node[3] = {4 * (a.tlo[0] + (int) tx) + (lane >> 4), 4 * (a.tlo[1] + (int) ty) + ((lane >> 2) & 3), 4 * (a.tlo[2] + (int) tz) + (lane & 3)};
	unsigned long long o = boff[blockIdx.x / (unsigned) kMeshFillGroup] + (unsigned long long) offs[blockIdx.x] + (unsigned long long) (inc - n);
	for(int k = 0; k < 8; ++k)
		if(mask >> k & 1u) {
			if(o < capacity) {
				xyz[3 * o]	   = mesh_fill_coord(node[0], k & 4, a.dx);
				xyz[3 * o + 1] = mesh_fill_coord(node[1], k & 2, a.dx);
				xyz[3 * o + 2] = mesh_fill_coord(node[2], k & 1, a.dx);
			}
			++o;
		}
}
#endif// __HIPCC__

}// namespace mpm
