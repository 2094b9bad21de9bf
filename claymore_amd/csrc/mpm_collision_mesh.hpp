// mpm_collision_mesh.hpp — the level-set collision object built from a closed triangle mesh (mpm_set_collision_mesh).
//
// An install-time kernel fills the field collision_resolve reads (mpm_collision.hpp: one float4 {sdis, gx, gy, gz} per node of the whole
// domain) straight from the mesh: exact point-triangle distance, a sign from angle-weighted pseudonormals (Baerentzen & Aanaes), a gradient.
// The substep path is untouched.  Three parts:
//   1. the definition - mesh_closest / mesh_field_value - MPM_DEV, float32 in one written-down order without contraction; it builds on x86
//      too (claymore_amd/host/host_selftest.cpp --mesh-closest, tests/collision_mesh_model.py restates it in NumPy);
//   2. the host side of an install - mesh_build: validation, adjacency, the per-triangle records - plain C++, no HIP;
//   3. the tile walk (HIP only) - one wave per 4 x 4 x 4 tile of points, triangles culled per tile - as device functions, and the two kernels
//      on it that every mesh-built table shares: collision_mesh_table_kernel (this field, and a volume's table: mpm_collision_volume.hpp) and
//      the box read-back collision_table_box_kernel.  mpm_mesh_fill.hpp's classify kernel is the walk's third caller.
// The definition is in include/claymore_amd.h and INTEGRATION.md section 5.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>
#ifndef MPM_DEV
#if defined(__HIPCC__)
#define MPM_DEV __device__ __forceinline__
#else
#define MPM_DEV inline
#endif
#endif

// No contraction anywhere in this file (mpm_collision.hpp says why), spelled for the compiler at hand: clang (hipcc) takes the pragma per
// function; g++, which builds the host tools, takes the option for the whole file and knows neither clang pragma.
#if defined(__clang__)
#define MPM_MESH_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MPM_MESH_UNROLL _Pragma("unroll")
#else
#define MPM_MESH_NO_CONTRACT
#define MPM_MESH_UNROLL
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

namespace mpm {

// What the kernel reads of a triangle (a, b, c): 12 defined floats ...
struct MeshTri {
	float a[3], ab[3], ac[3];// a, b - a, c - a: one float32 subtraction each
	float nh[3];			 // n / sqrtf(n . n), n = ab x ac
};
// ... and, for the sign only, the pseudonormal of each feature (float64 arithmetic, stored as float32; not bit-defined)
struct MeshPseudo {
	float m[6][3];// [feature]: corners a, b, c (sum over the triangles around the vertex of interior angle x n^), edges ab, ac, bc (n^ + n^ across)
};
enum { kMeshCornerA = 0, kMeshCornerB = 1, kMeshCornerC = 2, kMeshEdgeAB = 3, kMeshEdgeAC = 4, kMeshEdgeBC = 5, kMeshFace = 6 };

MPM_DEV float mesh_dot(const float (&a)[3], const float (&b)[3]) {
	MPM_MESH_NO_CONTRACT
	return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// Closest point c of the triangle to p by the Voronoi-region walk (Ericson, Real-Time Collision Detection 5.1.5: d1 .. d6, va / vb / vc), on
// the record: bp = ap - ab and cp = ap - ac stand for p - b and p - c.  The region gives the barycentric pair (v, w) as num / den - corners
// 0 / 1 and 1 / 1, so every region goes through the same two correctly rounded divisions -, on edge bc v = 1 - w, and
// c = (a + ab v) + ac w per axis.  Returns q = |p - c|^2 as ((dx^2 + dy^2) + dz^2); a NaN anywhere ends in the face branch.
MPM_DEV float mesh_closest(const MeshTri& t, const float (&p)[3], float (&c)[3], int& feature) {
	MPM_MESH_NO_CONTRACT
	float ap[3], bp[3], cp[3];
	MPM_MESH_UNROLL
	for(int d = 0; d < 3; ++d) {
		ap[d] = p[d] - t.a[d];
		bp[d] = ap[d] - t.ab[d];
		cp[d] = ap[d] - t.ac[d];
	}
	const float d1 = mesh_dot(t.ab, ap), d2 = mesh_dot(t.ac, ap);
	const float d3 = mesh_dot(t.ab, bp), d4 = mesh_dot(t.ac, bp);
	const float d5 = mesh_dot(t.ab, cp), d6 = mesh_dot(t.ac, cp);
	const float vc = d1 * d4 - d3 * d2;
	const float vb = d5 * d2 - d1 * d6;
	const float va = d3 * d6 - d5 * d4;
	const float e43 = d4 - d3, e56 = d5 - d6;
	float nv = 0.f, nw = 0.f, den = 1.f;
	if(d1 <= 0.f && d2 <= 0.f) {
		feature = kMeshCornerA;
	} else if(d3 >= 0.f && d4 <= d3) {
		feature = kMeshCornerB;
		nv		= 1.f;
	} else if(vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
		feature = kMeshEdgeAB;
		nv		= d1;
		den		= d1 - d3;
	} else if(d6 >= 0.f && d5 <= d6) {
		feature = kMeshCornerC;
		nw		= 1.f;
	} else if(vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
		feature = kMeshEdgeAC;
		nw		= d2;
		den		= d2 - d6;
	} else if(va <= 0.f && e43 >= 0.f && e56 >= 0.f) {
		feature = kMeshEdgeBC;
		nw		= e43;
		den		= e43 + e56;
	} else {
		feature = kMeshFace;
		nv		= vb;
		nw		= vc;
		den		= (va + vb) + vc;
	}
	float v		  = nv / den;
	const float w = nw / den;
	if(feature == kMeshEdgeBC) v = 1.f - w;
	float diff[3];
	MPM_MESH_UNROLL
	for(int d = 0; d < 3; ++d) {
		c[d]	= (t.a[d] + t.ab[d] * v) + t.ac[d] * w;
		diff[d] = p[d] - c[d];
	}
	return (diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2];
}

// The node's four words from its nearest triangle T (the lowest index among the smallest q - the caller's search).  Plane rule where T's
// feature is the face or q < 2^-40 (the node on, or numerically on, the surface: (p - c) / |p - c| would be rounding noise):
// sdis = (p - a) . n^, g = n^.  Radial rule elsewhere: d = sqrtf(q), s = +1 if (p - c) . m >= 0 else -1 with m the feature's pseudonormal,
// sdis = s d, g = s (p - c) / d.  inside_out negates all four.  Also hands back the feature and q (the host tools print them).
MPM_DEV void mesh_field_value(const MeshTri& t, const MeshPseudo& ps, const float (&p)[3], int inside_out, float (&out)[4], int& feature, float& q) {
	MPM_MESH_NO_CONTRACT
	float c[3];
	q = mesh_closest(t, p, c, feature);
	if(feature == kMeshFace || q < 0x1p-40f) {
		float ap[3];
	MPM_MESH_UNROLL
		for(int d = 0; d < 3; ++d) ap[d] = p[d] - t.a[d];
		out[0] = mesh_dot(ap, t.nh);
	MPM_MESH_UNROLL
		for(int d = 0; d < 3; ++d) out[1 + d] = t.nh[d];
	} else {
		const float dist = sqrtf(q);
		float diff[3], m[3];
	MPM_MESH_UNROLL
		for(int d = 0; d < 3; ++d) {
			diff[d] = p[d] - c[d];
			m[d]	= (&ps.m[0][0])[3 * feature + d];
		}
		const float s = mesh_dot(diff, m) >= 0.f ? 1.f : -1.f;
		out[0]		  = s * dist;
	MPM_MESH_UNROLL
		for(int d = 0; d < 3; ++d) out[1 + d] = (s * diff[d]) / dist;
	}
	if(inside_out) {
	MPM_MESH_UNROLL
		for(int d = 0; d < 4; ++d) out[d] = -out[d];
	}
}

// ---- host side of an install -----------------------------------------------------------------------------------------------------------
struct MeshReport {
	std::string reason;// empty: the mesh is accepted; else the first failed check, in the order of include/claymore_amd.h
	bool closed = false;// every directed edge once, its reverse once
	double volume = 0.; // sum a . (b x c) / 6 in float64 (0 unless the indices and vertices passed)
};

// Validation, adjacency and records of a mesh.  The records are built whenever the indices and vertices are usable, accepted or not (an open
// mesh's free edges get their own triangle's normal as pseudonormal), so that the host tools can query any mesh; an install goes on only
// with an empty report.reason.  limit_t / limit_v: MPM_MESH_MAX_TRIANGLES / _VERTICES.
inline void mesh_build(const float* verts, size_t nv, const int32_t* tris, size_t nt, size_t limit_v, size_t limit_t, std::vector<MeshTri>& rec,
					   std::vector<MeshPseudo>& pseudo, MeshReport& rep) {
	MPM_MESH_NO_CONTRACT
	rec.clear();
	pseudo.clear();
	rep = MeshReport {};
	auto refuse = [&](const std::string& why) {
		if(rep.reason.empty()) rep.reason = why;
	};
	if(nt < 4) refuse("collision mesh: fewer than 4 triangles");
	if(nt > limit_t) refuse("collision mesh: more than " + std::to_string(limit_t) + " triangles");
	if(nv > limit_v) refuse("collision mesh: more than " + std::to_string(limit_v) + " vertices");
	if(nt > limit_t || nv > limit_v) return;
	for(size_t i = 0; i < 3 * nt; ++i)
		if(tris[i] < 0 || (size_t) tris[i] >= nv) {
			refuse("collision mesh: triangle " + std::to_string(i / 3) + " has an index outside [0, nv)");
			return;
		}
	for(size_t i = 0; i < 3 * nv; ++i)
		if(!std::isfinite(verts[i])) {
			refuse("collision mesh: vertex " + std::to_string(i / 3) + " is not finite");
			return;
		}
	// records (float32) and unit normals (float64, for the pseudonormals)
	rec.resize(nt);
	pseudo.resize(nt);
	std::vector<double> nh64(3 * nt), vsum(3 * nv, 0.);
	double vol = 0.;
	for(size_t t = 0; t < nt; ++t) {
		const float *a = verts + 3 * (size_t) tris[3 * t], *b = verts + 3 * (size_t) tris[3 * t + 1], *c = verts + 3 * (size_t) tris[3 * t + 2];
		MeshTri& r = rec[t];
		for(int d = 0; d < 3; ++d) {
			r.a[d]	= a[d];
			r.ab[d] = b[d] - a[d];
			r.ac[d] = c[d] - a[d];
		}
		float n[3];
		n[0]		   = r.ab[1] * r.ac[2] - r.ab[2] * r.ac[1];
		n[1]		   = r.ab[2] * r.ac[0] - r.ab[0] * r.ac[2];
		n[2]		   = r.ab[0] * r.ac[1] - r.ab[1] * r.ac[0];
		const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
		if(!(nn > 0.f) || !std::isfinite(nn)) refuse("collision mesh: triangle " + std::to_string(t) + " is degenerate (n . n is zero or not finite)");
		const float len = sqrtf(nn);
		for(int d = 0; d < 3; ++d) r.nh[d] = n[d] / len;
		// float64: normal, interior angles, volume
		const double A[3] = {a[0], a[1], a[2]}, B[3] = {b[0], b[1], b[2]}, C[3] = {c[0], c[1], c[2]};
		const double* P[3] = {A, B, C};
		double e1[3], e2[3], N[3];
		for(int d = 0; d < 3; ++d) e1[d] = B[d] - A[d], e2[d] = C[d] - A[d];
		N[0]			= e1[1] * e2[2] - e1[2] * e2[1];
		N[1]			= e1[2] * e2[0] - e1[0] * e2[2];
		N[2]			= e1[0] * e2[1] - e1[1] * e2[0];
		const double nl = std::sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
		for(int d = 0; d < 3; ++d) nh64[3 * t + d] = nl > 0. ? N[d] / nl : 0.;
		vol += A[0] * (B[1] * C[2] - B[2] * C[1]) + A[1] * (B[2] * C[0] - B[0] * C[2]) + A[2] * (B[0] * C[1] - B[1] * C[0]);
		for(int k = 0; k < 3; ++k) {// interior angle at corner k
			const double *o = P[k], *u = P[(k + 1) % 3], *w = P[(k + 2) % 3];
			double x[3], y[3], cr[3];
			for(int d = 0; d < 3; ++d) x[d] = u[d] - o[d], y[d] = w[d] - o[d];
			cr[0]			   = x[1] * y[2] - x[2] * y[1];
			cr[1]			   = x[2] * y[0] - x[0] * y[2];
			cr[2]			   = x[0] * y[1] - x[1] * y[0];
			const double angle = std::atan2(std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), x[0] * y[0] + x[1] * y[1] + x[2] * y[2]);
			for(int d = 0; d < 3; ++d) vsum[3 * (size_t) tris[3 * t + k] + d] += angle * nh64[3 * t + d];
		}
	}
	rep.volume = vol / 6.;
	// directed edges: (u, v) -> triangle 3 t + e, e = 0: ab, 1: bc, 2: ca
	struct Edge {
		uint64_t key;
		uint32_t id;
	};
	std::vector<Edge> edges(3 * nt);
	for(size_t t = 0; t < nt; ++t)
		for(int e = 0; e < 3; ++e) edges[3 * t + e] = Edge {((uint64_t) (uint32_t) tris[3 * t + e] << 32) | (uint32_t) tris[3 * t + (e + 1) % 3], (uint32_t) (3 * t + e)};
	std::sort(edges.begin(), edges.end(), [](const Edge& x, const Edge& y) { return x.key < y.key || (x.key == y.key && x.id < y.id); });
	bool closed = true;
	std::vector<int64_t> across(3 * nt, -1);// triangle across each directed edge
	for(size_t i = 0; i < edges.size(); ++i) {
		if(i && edges[i].key == edges[i - 1].key) closed = false;// a directed edge twice: a duplicated or flipped triangle
		const uint64_t rev = (edges[i].key << 32) | (edges[i].key >> 32);
		auto lo = std::lower_bound(edges.begin(), edges.end(), rev, [](const Edge& x, uint64_t k) { return x.key < k; });
		if(lo == edges.end() || lo->key != rev)
			closed = false;// a free edge
		else {
			across[edges[i].id] = lo->id / 3;
			if(lo + 1 != edges.end() && (lo + 1)->key == rev) closed = false;
		}
	}
	rep.closed = closed;
	if(!closed) refuse("collision mesh: not a closed, consistently oriented manifold (every directed edge must occur once and its reverse once)");
	if(!(rep.volume > 0.)) refuse("collision mesh: signed volume " + std::to_string(rep.volume) + " <= 0: flip the winding (counter-clockwise seen from outside) or use inside_out");
	for(size_t t = 0; t < nt; ++t) {
		static const int edge_of_feature[3] = {0, 2, 1};// features ab, ac, bc <- directed edges ab (0), ca (2), bc (1)
		for(int k = 0; k < 3; ++k)
			for(int d = 0; d < 3; ++d) pseudo[t].m[k][d] = (float) vsum[3 * (size_t) tris[3 * t + k] + d];
		for(int f = 0; f < 3; ++f) {
			const int64_t o = across[3 * t + edge_of_feature[f]];
			for(int d = 0; d < 3; ++d) pseudo[t].m[3 + f][d] = (float) (nh64[3 * t + d] + (o >= 0 ? nh64[3 * (size_t) o + d] : 0.));
		}
	}
}

#if !defined(__HIPCC__)
// x86 builds only (there MPM_DEV functions are plain inline ones): the field value of one point by exhaustive search, T = the lowest index
// among the smallest q (strict < in index order).
inline int mesh_point_query(const std::vector<MeshTri>& rec, const std::vector<MeshPseudo>& pseudo, const float (&p)[3], int inside_out, float (&out)[4], int& feature, float& q) {
	int best  = 0;
	float bq  = INFINITY;
	for(size_t t = 0; t < rec.size(); ++t) {
		float c[3];
		int f;
		const float qt = mesh_closest(rec[t], p, c, f);
		if(qt < bq) bq = qt, best = (int) t;
	}
	mesh_field_value(rec[(size_t) best], pseudo[(size_t) best], p, inside_out, out, feature, q);
	return best;
}
#endif

#if defined(__HIPCC__)
// ---- the tile walk and its kernels -------------------------------------------------------------------------------------------------------
// One wave (a 64-thread block) per 4 x 4 x 4 node tile, one node per lane (lane = (x 4 + y) 4 + z: four 64-byte runs of the field).
//   1. Bound.  The lanes stride over the triangles and evaluate q at the tile's centre; a wave-min gives D = sqrtf(min q).  With r the
//      half diagonal of the tile's nodes (1.5 sqrt(3) dx) every node is within D + r of the mesh.
//   2. Candidates.  A triangle nearest to some node p of the tile is within D + r of p, so within D + 2 r of the centre.  The triangles
//      are tested again 64 at a time in index order; those that pass are compacted, in index order (ballot + prefix count), into an LDS
//      chunk of kMeshChunk records.  Whenever another 64 might not fit, and at the end, every lane walks the chunk in order with strict <
//      against its own node.  Chunks are consumed in index order, so "the lowest index among equals" survives the culling.
//   3. Rule and store.  The winner's record is read again, mesh_field_value gives the four words, one 16-byte store per node.
// Safety margin of the test.  The argument above is about exact distances; the kernel compares float32 values of the walk, each off by
// some eps.  Going through it with computed distances costs 4 eps: q_T(centre) <= (D + 2 r + 4 eps)^2.  The test uses
//     thr = (D + 2 r) (1 + 2^-6) + slack,   slack = max(dx / 4, 2^-12 max |coordinate|),   q <= thr^2,
// i.e. eps up to 2^-8 (D + 2 r) + slack / 4 - where a coordinate's float32 ulp is 2^-24 of it and the walk's error is a few of those
// for triangles that are not slivers; the squaring's own rounding (2^-23 relative) disappears in the 2^-6.  The margin costs a few
// candidates per tile and nothing else: a triangle that passes needlessly loses the strict < comparison.
// Budget.  LDS: kMeshChunk x (48 B record + 4 B index) = 6.5 KiB per block, stated here and checked by tests/test_collision_mesh_isa.py with the
// kernel's scratch (none: every array is indexed by constants).  No atomics.
// The walk exists once, as the functions below; its callers are collision_mesh_table_kernel (one point per lane) and
// mesh_fill_classify_kernel (mpm_mesh_fill.hpp: eight points per lane, a larger r).  Both declare the chunk themselves and pass it in.
constexpr int kMeshChunk = 128;

// A record as the kernels fetch it: three 16-byte loads, from global memory or from the chunk
MPM_DEV void mesh_load_tri(const float4* src, MeshTri& t) {
	const float4 r0 = src[0], r1 = src[1], r2 = src[2];
	t.a[0] = r0.x, t.a[1] = r0.y, t.a[2] = r0.z, t.ab[0] = r0.w;
	t.ab[1] = r1.x, t.ab[2] = r1.y, t.ac[0] = r1.z, t.ac[1] = r1.w;
	t.ac[2] = r2.x, t.nh[0] = r2.y, t.nh[1] = r2.z, t.nh[2] = r2.w;
}

// 1. Bound: min q at the tile's centre over all triangles, the same in every lane, and in tmin the lowest index that attains it (a caller
// that ignores tmin pays nothing for it: qmin does not depend on it).  The lanes past the end of the last 64 repeat triangle nt - 1.
MPM_DEV float mesh_centre_bound(const float4* __restrict__ tris4, int nt, int lane, const float (&centre)[3], int& tmin) {
	float qmin = INFINITY;
	tmin	   = 0;
	for(int base = 0; base < nt; base += 64) {
		const int t = min(base + lane, nt - 1);
		MeshTri tri;
		mesh_load_tri(tris4 + 3 * (size_t) t, tri);
		float c[3];
		int f;
		const float q = mesh_closest(tri, centre, c, f);
		if(q < qmin) qmin = q, tmin = t;
	}
	for(int off = 32; off > 0; off >>= 1) {
		const float oq = __shfl_xor(qmin, off);
		const int ot   = __shfl_xor(tmin, off);
		tmin		   = oq < qmin || (oq == qmin && ot < tmin) ? ot : tmin;
		qmin		   = oq < qmin ? oq : qmin;
	}
	return qmin;
}

// The test's threshold on q(centre), squared: D = sqrtf(min q), r the half diagonal of the tile's points about the centre
MPM_DEV float mesh_threshold2(float D, float r, float slack) {
	const float thr = (D + 2.f * r) * 1.015625f + slack;
	return thr * thr;
}

// 2. Candidates: the triangles with q(centre) <= thr2, 64 at a time in index order, compacted in that order into the chunk s_rec / s_idx
// (kMeshChunk records); consume(fill) runs between two barriers whenever another 64 might not fit, and at the end.  Every lane of the
// block calls this (fill is wave-uniform).  consume is taken by value: behind a reference, the arrays a lambda captures went to scratch.
template<typename Consume>
MPM_DEV void mesh_sweep_candidates(const float4* __restrict__ tris4, int nt, int lane, const float (&centre)[3], float thr2, float4* s_rec, int* s_idx, Consume consume) {
	int fill = 0;
	for(int base = 0; base < nt; base += 64) {
		const int t	  = base + lane;
		const bool in = t < nt;
		MeshTri tri;
		mesh_load_tri(tris4 + 3 * (size_t) (in ? t : nt - 1), tri);
		float c[3];
		int f;
		const float qc				  = mesh_closest(tri, centre, c, f);
		const bool cand				  = in && qc <= thr2;
		const unsigned long long mask = __ballot(cand);
		if(cand) {
			const int pos = fill + (int) __popcll(mask & ((1ull << lane) - 1ull));// < fill + 64 <= kMeshChunk
			const float4* src  = tris4 + 3 * (size_t) t;
			s_rec[3 * pos]	   = src[0];
			s_rec[3 * pos + 1] = src[1];
			s_rec[3 * pos + 2] = src[2];
			s_idx[pos]		   = t;
		}
		fill += (int) __popcll(mask);
		if(fill > kMeshChunk - 64 || base + 64 >= nt) {
			__syncthreads();
			consume(fill);
			__syncthreads();
			fill = 0;
		}
	}
}

// One point against the chunk, in order, strict <: (best_q, best_t) carry over from chunk to chunk
MPM_DEV void mesh_walk_chunk(const float4* s_rec, const int* s_idx, int fill, const float (&p)[3], float& best_q, int& best_t) {
	for(int i = 0; i < fill; ++i) {
		MeshTri ct;
		mesh_load_tri(s_rec + 3 * i, ct);
		float c[3];
		int f;
		const float qt = mesh_closest(ct, p, c, f);
		if(qt < best_q) best_q = qt, best_t = s_idx[i];
	}
}

// Position of sample i along an axis: volume_sample_point's two statements (mpm_collision_volume.hpp, which includes this file)
MPM_DEV float mesh_table_point(float origin, float spacing, int i) {
	MPM_MESH_NO_CONTRACT
	const float s = (float) i * spacing;
	return origin + s;
}

// A table of d0 x d1 x d2 samples `spacing` apart from (o0, o1, o2), sample (i, j, k) at [(i d1 + j) d2 + k] and p_d = origin_d +
// (float) i_d * spacing: the three steps above with `spacing` for dx and the samples for the nodes.  Both mesh-built colliders are this kernel:
//   the level-set field (mpm_set_collision_mesh): dims {N, N, N}, origin 0, spacing dx - p is (float) node * dx exactly -, inside_out baked
//     into the words by mesh_field_value;
//   a volume's table (mpm_set_collision_volume_mesh): the box's own numbers, inside_out 0 - a volume is flipped at the query -, slack taken
//     over the vertices and the box's corners.
// dims need not be multiples of 4: the lanes of a partial tile whose sample lies outside the table take part in the culling (their point
// is still within r of the centre) and do not store.
__global__ __launch_bounds__(64) void collision_mesh_table_kernel(const MeshTri* __restrict__ tris, const MeshPseudo* __restrict__ pseudo, int nt, int d0, int d1, int d2, float o0, float o1,
																   float o2, float spacing, float slack, int inside_out, float4* __restrict__ table) {
	__shared__ float4 s_rec[kMeshChunk * 3];
	__shared__ int s_idx[kMeshChunk];
	const int lane	  = (int) threadIdx.x;
	const unsigned t1 = (unsigned) ((d1 + 3) >> 2), t2 = (unsigned) ((d2 + 3) >> 2);
	const int bz = (int) (blockIdx.x % t2), by = (int) ((blockIdx.x / t2) % t1), bx = (int) (blockIdx.x / (t2 * t1));
	const int idx[3]	  = {4 * bx + (lane >> 4), 4 * by + ((lane >> 2) & 3), 4 * bz + (lane & 3)};
	const bool stores	  = idx[0] < d0 && idx[1] < d1 && idx[2] < d2;
	const float p[3]	  = {mesh_table_point(o0, spacing, idx[0]), mesh_table_point(o1, spacing, idx[1]), mesh_table_point(o2, spacing, idx[2])};
	const float centre[3] = {o0 + ((float) (4 * bx) + 1.5f) * spacing, o1 + ((float) (4 * by) + 1.5f) * spacing, o2 + ((float) (4 * bz) + 1.5f) * spacing};
	const float4* tris4	  = reinterpret_cast<const float4*>(tris);
	int tmin;
	const float D = sqrtf(mesh_centre_bound(tris4, nt, lane, centre, tmin));
	float best_q  = INFINITY;
	int best_t	  = 0;
	mesh_sweep_candidates(tris4, nt, lane, centre, mesh_threshold2(D, 2.598076211f * spacing, slack), s_rec, s_idx, [&](int fill) { mesh_walk_chunk(s_rec, s_idx, fill, p, best_q, best_t); });
	// 3. rule and store
	MeshTri win;
	mesh_load_tri(tris4 + 3 * (size_t) best_t, win);
	float out[4], q;
	int feature;
	mesh_field_value(win, pseudo[best_t], p, inside_out, out, feature, q);
	if(stores) table[((size_t) idx[0] * (size_t) d1 + (size_t) idx[1]) * (size_t) d2 + (size_t) idx[2]] = make_float4(out[0], out[1], out[2], out[3]);
}

// mpm_get_collision_field, mpm_get_collision_volume: the box lo + [0, b) of a table of (., d1, d2) entries, x slowest, z fastest (bounds
// are the host's to check)
__global__ void collision_table_box_kernel(const float4* __restrict__ table, int d1, int d2, int lo0, int lo1, int lo2, int b0, int b1, int b2, float4* __restrict__ out) {
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= (size_t) b0 * (size_t) b1 * (size_t) b2) return;
	const int z = (int) (i % (size_t) b2), y = (int) ((i / (size_t) b2) % (size_t) b1), x = (int) (i / ((size_t) b2 * (size_t) b1));
	out[i]		= table[((size_t) (lo0 + x) * (size_t) d1 + (size_t) (lo1 + y)) * (size_t) d2 + (size_t) (lo2 + z)];
}
#endif// __HIPCC__

}// namespace mpm
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC pop_options
#endif
