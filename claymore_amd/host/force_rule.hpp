// force_rule.hpp — when a force field of a scene is installed and removed (an entry of a scene file's "forces"; scenes.ForceEntry states the
// same rule in Python):
//   {"kind": "uniform" ("vec") | "point" ("centre", "strength", "falloff", "soft") | "vortex" ("vec": the axis, "centre", "swirl", "pull", "lift") |
//    "drag" ("vec": the target velocity, "strength"), "feather": w, "region": {the shape keys of "colliders", at rest}, "start": t0, "end": t1}
// Entry i of the array lives in slot i.  The rule: the entry is installed at the first substep boundary t where start <= t < end holds and
// removed at the first boundary where it no longer holds (start == end: never installed; a window no boundary falls into: never installed).
// All in float64.  Shared by gmpm.cpp, which serves the forces at every substep boundary before the sinks and the emitters, and
// host_selftest.cpp (--force), which needs no GPU.
#pragma once
#include <limits>

#include "mini_json.hpp"

namespace pio {

struct ForceRule {
	double start = 0.0, end = std::numeric_limits<double>::infinity();
	bool installed = false;

	// What the substep boundary t asks for: +1 install, -1 remove, 0 nothing.
	int due(double t) {
		const bool want = start <= t && t < end;
		const int act	= (int) want - (int) installed;
		installed		= want;
		return act;
	}
};

// The times of a force entry; the field itself is the caller's to parse (gmpm.cpp).
inline void parse_force_rule(const mj::Value& e, ForceRule& r) {
	r = ForceRule {};
	if(e.has("start")) r.start = e["start"].number();
	if(e.has("end")) r.end = e["end"].number();
}

}// namespace pio
