// model_field.hpp — the initial velocity field of a model object of a gmpm scene file (mpm_set_model_velocity_field):
//   "velocity": [x, y, z]                       v0, as before: the velocity at the pivot
//   "omega": [x, y, z]                          a rigid rotation about the pivot, rad/s: v = v0 + omega x (x - pivot)
//   "velocity_gradient": [9 numbers]            G row-major, G[3 r + c] = dv_r / dx_c: v = v0 + G (x - pivot); with "omega" the two are added
//   "pivot": [x, y, z]                          optional, default the origin
// Shared by gmpm.cpp and host_selftest.cpp (which parses one such model without a device).
#pragma once
#include <cmath>
#include <cstdio>

#include "mini_json.hpp"

namespace pio {

struct ModelField {
	float v0[3]	   = {0.f, 0.f, 0.f};
	float grad9[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};// column-major, as the C ABI takes it: grad9[3 c + r] = G_rc
	float pivot[3] = {0.f, 0.f, 0.f};
	// the velocity of a particle at x, in float64 (frame 0's "v" attribute, the first dt)
	void at(const float* x, double (&v)[3]) const {
		for(int r = 0; r < 3; ++r) {
			v[r] = v0[r];
			for(int c = 0; c < 3; ++c) v[r] += (double) grad9[3 * c + r] * ((double) x[c] - (double) pivot[c]);
		}
	}
};

// 0: the model carries no field ("velocity" alone); 1: f holds it; -1: malformed (a message has been printed)
inline int parse_model_field(const mj::Value& m, ModelField& f) {
	if(m.has("velocity"))
		for(int d = 0; d < 3; ++d) f.v0[d] = (float) m["velocity"][d].number();
	const bool has_omega = m.has("omega"), has_grad = m.has("velocity_gradient");
	if(!has_omega && !has_grad) return 0;
	if(has_grad) {
		if(m["velocity_gradient"].arr.size() != 9) {
			std::fprintf(stderr, "gmpm: \"velocity_gradient\" takes 9 numbers (row-major), got %zu\n", m["velocity_gradient"].arr.size());
			return -1;
		}
		for(int r = 0; r < 3; ++r)
			for(int c = 0; c < 3; ++c) f.grad9[3 * c + r] = (float) m["velocity_gradient"][3 * r + c].number();
	}
	if(has_omega) {
		if(m["omega"].arr.size() != 3) {
			std::fprintf(stderr, "gmpm: \"omega\" takes 3 numbers, got %zu\n", m["omega"].arr.size());
			return -1;
		}
		const float w[3] = {(float) m["omega"][0].number(), (float) m["omega"][1].number(), (float) m["omega"][2].number()};
		// W x = omega x x: W = [[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]]
		f.grad9[3 * 1 + 0] += -w[2], f.grad9[3 * 2 + 0] += w[1];
		f.grad9[3 * 0 + 1] += w[2], f.grad9[3 * 2 + 1] += -w[0];
		f.grad9[3 * 0 + 2] += -w[1], f.grad9[3 * 1 + 2] += w[0];
	}
	if(m.has("pivot"))
		for(int d = 0; d < 3; ++d) f.pivot[d] = (float) m["pivot"][d].number();
	for(float x: f.grad9)
		if(!std::isfinite(x)) {
			std::fprintf(stderr, "gmpm: the model's velocity field is not finite\n");
			return -1;
		}
	return 1;
}

}// namespace pio
