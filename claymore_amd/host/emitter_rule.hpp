// emitter_rule.hpp — the layer rule of a particle source (an entry of a scene file's "emitters"; scenes.Emitter states the same rule in Python):
//   {"model": 0, "shape": "box", "lo": [..], "hi": [..] | "shape": "disc", "center": [..], "radius": r, "normal": [..],
//    "velocity": [x, y, z], "start": t0, "end": t1}
// The velocity lies along one principal axis, the flow axis (a disc's normal names the same axis).  The particles are the reference's lattice -
// 8 per cell at node -+ 0.25 dx, the odd multiples of dx / 4 - cut by the nozzle's cross-section (a box's extent on the two axes across the flow,
// bounds included; a disc's radius about its centre), in the lattice plane nearest the nozzle's centre (a tie goes to the lower one).  One layer
// is due every (dx / 2) / |v| seconds: t_k = start + k (dx / 2) / |v| for every t_k < end.  A layer due at t_k is handed out by the first due(t)
// with t >= t_k, at x + v (t - t_k), so the stream is the same lattice whatever the substep sizes are.  All in float64, the points rounded to
// float32 once.  Shared by gmpm.cpp, which emits what is due between two mpm_substep calls, and host_selftest.cpp (--emitter), which needs no GPU.
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mini_json.hpp"

namespace pio {

struct Emitter {
	int model = 0, axis = 0;
	double velocity[3] = {0, 0, 0};
	double start = 0.0, end = std::numeric_limits<double>::infinity(), period = 0.0;
	std::vector<double> layer;// 3 per lattice point of the nozzle's plane
	long next_layer = 0;

	// The positions to emit at the substep boundary t (3 floats a point): every layer that is due and has not been handed out.
	std::vector<float> due(double t) {
		std::vector<float> out;
		for(;;) {
			const double tk = start + (double) next_layer * period;
			if(!(tk < end && tk <= t)) break;
			for(size_t i = 0; i < layer.size(); ++i) out.push_back((float) (layer[i] + velocity[i % 3] * (t - tk)));
			++next_layer;
		}
		return out;
	}
};

// false: malformed (a message has been printed)
inline bool parse_emitter(const mj::Value& e, int bits, Emitter& em) {
	auto vec = [&](const char* k, double (&out)[3]) {
		if(!e.has(k) || e[k].arr.size() != 3) return false;
		for(int d = 0; d < 3; ++d) out[d] = e[k][d].number();
		return true;
	};
	if(!vec("velocity", em.velocity)) {
		std::fprintf(stderr, "gmpm: an emitter needs \"velocity\": [x, y, z]\n");
		return false;
	}
	int nonzero = 0;
	for(int d = 0; d < 3; ++d)
		if(em.velocity[d] != 0.0) em.axis = d, ++nonzero;
	if(nonzero != 1 || !std::isfinite(em.velocity[em.axis])) {
		std::fprintf(stderr, "gmpm: an emitter's velocity must lie along one principal axis\n");
		return false;
	}
	em.model = e.has("model") ? (int) e["model"].number() : 0;
	em.start = e.has("start") ? e["start"].number() : 0.0;
	if(e.has("end")) em.end = e["end"].number();
	const int n	   = 1 << bits;
	const double h = 0.5 / (double) n;// the lattice spacing, dx / 2
	em.period	   = h / std::fabs(em.velocity[em.axis]);
	const std::string shape = e.has("shape") ? e["shape"].string() : "";
	double c[3], lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, radius = 0.0;
	if(shape == "disc") {
		if(!vec("center", c) || !e.has("radius")) {
			std::fprintf(stderr, "gmpm: emitter 'disc' needs \"center\" and \"radius\"\n");
			return false;
		}
		radius = e["radius"].number();
		double nrm[3];
		if(vec("normal", nrm)) {
			int nz = 0, at = 0;
			for(int d = 0; d < 3; ++d)
				if(nrm[d] != 0.0) at = d, ++nz;
			if(nz != 1 || at != em.axis) {
				std::fprintf(stderr, "gmpm: a disc emitter's normal must lie along its velocity's axis\n");
				return false;
			}
		}
	} else if(shape == "box") {
		if(!vec("lo", lo) || !vec("hi", hi)) {
			std::fprintf(stderr, "gmpm: emitter 'box' needs \"lo\" and \"hi\"\n");
			return false;
		}
		for(int d = 0; d < 3; ++d) c[d] = (lo[d] + hi[d]) / 2;
	} else {
		std::fprintf(stderr, "gmpm: unknown emitter shape '%s' (expected box or disc)\n", shape.c_str());
		return false;
	}
	long j = (long) std::floor(c[em.axis] / h);
	j	   = j < 0 ? 0 : j > 2 * n - 1 ? 2 * n - 1 : j;
	if(j > 0 && c[em.axis] == (double) j * h) --j;
	const int t0 = em.axis == 0 ? 1 : 0, t1 = em.axis == 2 ? 1 : 2;
	em.layer.clear();
	for(int a = 0; a < 2 * n; ++a)
		for(int b = 0; b < 2 * n; ++b) {
			const double A = ((double) a + 0.5) * h, B = ((double) b + 0.5) * h;
			const bool keep = shape == "disc" ? (A - c[t0]) * (A - c[t0]) + (B - c[t1]) * (B - c[t1]) <= radius * radius : (A >= lo[t0] && A <= hi[t0] && B >= lo[t1] && B <= hi[t1]);
			if(!keep) continue;
			double p[3];
			p[em.axis] = ((double) j + 0.5) * h, p[t0] = A, p[t1] = B;
			em.layer.insert(em.layer.end(), p, p + 3);
		}
	em.next_layer = 0;
	return true;
}

}// namespace pio
