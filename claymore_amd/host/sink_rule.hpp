// sink_rule.hpp — the sweep rule of a particle sink (an entry of a scene file's "sinks"; scenes.Sink states the same rule in Python):
//   {"shape": "halfspace" ("point", "normal") | "sphere" ("center", "radius") | "box" ("center", "half_extents") | "capsule" ("a", "b", "radius"),
//    "inside_out": false, "model": -1, "start": t0, "end": t1, "period": T}
// The shape keys are those of "colliders", in domain coordinates and without a pose.  Sweep k is due at t_k = start + k period for every
// t_k < end; it is served by the first substep boundary t >= t_k, and several sweeps that are due at one boundary make one call.  "period" is
// required and must be > 0.  All in float64.  Shared by gmpm.cpp, which sweeps what is due between two mpm_substep calls - before it serves the
// emitters -, and host_selftest.cpp (--sink), which needs no GPU.
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>

#include "mini_json.hpp"

namespace pio {

struct Sink {
	int model = -1;
	double start = 0.0, end = std::numeric_limits<double>::infinity(), period = 0.0;
	long next_sweep = 0;

	// How many sweeps the substep boundary t serves: every sweep that is due and has not been served (0: no call).
	long due(double t) {
		long k = 0;
		for(;;) {
			const double tk = start + (double) next_sweep * period;
			if(!(tk < end && tk <= t)) break;
			++next_sweep;
			++k;
		}
		return k;
	}
};

// The times of a sink entry; the region is the caller's to parse (gmpm.cpp: the collider's shape keys).  false: malformed (a message has been printed)
inline bool parse_sink(const mj::Value& e, Sink& sk) {
	if(!e.has("period") || !(e["period"].number() > 0.0) || !std::isfinite(e["period"].number())) {
		std::fprintf(stderr, "gmpm: a sink needs \"period\" > 0\n");
		return false;
	}
	sk.period = e["period"].number();
	sk.model  = e.has("model") ? (int) e["model"].number() : -1;
	sk.start  = e.has("start") ? e["start"].number() : 0.0;
	if(e.has("end")) sk.end = e["end"].number();
	sk.next_sweep = 0;
	return true;
}

}// namespace pio
