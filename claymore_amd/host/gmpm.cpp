// gmpm.cpp — host driver with the surface of claymore's `gmpm` executable (Projects/GMPM/gmpm.cu:168-209):
//     gmpm -f scene.json
// parses the same scene schema (gmpm.cu:60-165), samples the models, runs GmpmSimulator::main_loop
// (gmpm_simulator.cuh:303-592) through the C ABI of include/claymore_amd.h and writes position-only BGEO frames
// `model_id[i]_frame[f].bgeo` (gmpm_simulator.cuh:204,626-631).  All kernels live behind libclaymore_hip.so.
//
// Schema additions (the reference hard-codes them at compile time, Projects/GMPM/settings.h): simulation.domain_bits
// (default 8), simulation.max_ppc, simulation.gravity, simulation.output_dir; model.file may be "sphere" or "box"
// (analytic shapes on the reference's 8-per-node lattice, offset = min corner, span = extent) besides "*.sdf"
// (text level set; sampled on the same lattice where phi < 0 - deterministic, unlike the reference's rand()-based
// Poisson sampling, Library/MnSystem/IO/PoissonDisk/SampleGenerator.h:112-176).  simulation.output_velocity (default false):
// every frame also carries a 3-float point attribute "v" (mpm_retrieve_velocity; frame 0: the model's initial velocity);
// without it the frames are byte for byte the position-only ones.  simulation.output_stress (default false): every frame also carries the
// point attributes "stress" (6 floats: the Cauchy stress {xx, yy, zz, xy, xz, yz}), "J", "pressure" and "vonmises" (1 float each) of
// mpm_retrieve_stress (frame 0: the stress-free initial state, J = 1).  With both keys the two readouts come back in different particle
// orders: each is sorted on the bits of its positions (which are the same bits in both) and the stress rows are written in the order of the
// velocity readout.  simulation.output_ids (default false): the context tracks particle ids (mpm_track_particle_ids) and every frame also carries
// the INT point attribute "id" - the particle's index among the model's sampled points - with the frame's points written in ascending id
// order, so the point order is the same in every frame; the other attributes are joined to the ids on the position bits.  A top-level "colliders" array installs analytic collision shapes (parse_collider below).
// A top-level "collision_mesh" object installs the level-set collision object from an OBJ file (mpm_set_collision_mesh; in main below).
// "body": {...} in an entry of "colliders" makes it a rigid body (install_body below); simulation.output_bodies (default false) writes
// `bodies_frame[f].json` beside each frame: every body's pose, velocities and last impulse (mpm_get_collider_body).
// simulation.output_loads (default false): the load gauge runs (mpm_load_gauge) and `loads_frame[f].json` beside each frame holds, per row (the
// level-set object, the four slots, the domain walls), the force and torque on the collider averaged over the frame, the touched-node count and
// the elapsed time (mpm_load_gauge_read at the frame's end).  A model object may carry "omega": [x, y, z] or "velocity_gradient": [9 numbers, row-major] with an
// optional "pivot": the model starts in the linear velocity field v = velocity + G (x - pivot) (model_field.hpp, mpm_set_model_velocity_field).
// A top-level "emitters" array holds particle sources (emitter_rule.hpp: a box or disc nozzle, a velocity, a start and an end time, a model):
// what is due is added to its model between two mpm_substep calls (mpm_emit_particles), so later frames of that model carry more points; with
// simulation.output_ids the new points have the largest ids and the ascending-id order of the older ones stays as it was.
// A top-level "sinks" array holds particle sinks (sink_rule.hpp: the shape keys of "colliders" - halfspace, sphere, box or capsule, at rest -
// plus "model" (default -1: all), "start", "end" and "period"): a sink with a sweep due takes the particles in its region out between two
// mpm_substep calls (mpm_remove_particles), before the emitters are served, so later frames carry fewer points.  simulation.output_removed
// (default false) writes `removed_frame[f].json` beside each frame: per-model counts, mass and momentum removed since the last frame.
// A top-level "forces" array holds up to four force fields (force_rule.hpp: "kind" uniform | point | vortex | drag with "vec", "centre", "strength",
// "swirl", "pull", "lift", "soft", "falloff", "feather", an optional "region" with the shape keys of "colliders", at rest, and "start" / "end"):
// entry i is installed in slot i (mpm_set_force_field) at the first substep boundary inside [start, end) and removed at the first one outside,
// before sinks and emitters are served.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/claymore_amd.h"
#include "mini_json.hpp"
#include "particle_io.hpp"
#include "model_field.hpp"
#include "emitter_rule.hpp"
#include "sink_rule.hpp"
#include "force_rule.hpp"

namespace {

struct ModelSpec {
	int material = MPM_FIXED_COROTATED;
	mpm_material_params p {};
	pio::Points pts;
	float v0[3] = {0, 0, 0};
};

[[noreturn]] void die(mpm_ctx* ctx, int rc) {
	// check_cuda_errors / std::abort behaviour of the reference: print and leave (HostUtils.hpp:33-44)
	std::fprintf(stderr, "gmpm: status %d: %s\n", rc, ctx ? mpm_last_error(ctx) : "(no context)");
	std::exit(EXIT_FAILURE);
}

int material_of(const std::string& s) {
	if(s == "jfluid") return MPM_J_FLUID;
	if(s == "fixed_corotated") return MPM_FIXED_COROTATED;
	if(s == "sand") return MPM_SAND;
	if(s == "nacc") return MPM_NACC;
	return -1;
}

float num(const mj::Value& v, const char* k, float dflt) {
	return v.has(k) ? (float) v[k].number() : dflt;
}

pio::Points sample_model(const mj::Value& model, int bits, const std::string& scene_dir) {
	const float dx = 1.f / (float) (1 << bits);
	float offset[3], span[3];
	for(int d = 0; d < 3; ++d) {
		offset[d] = (float) model["offset"][d].number();
		span[d]	  = (float) model["span"][d].number();
	}
	int lo[3], hi[3];
	for(int d = 0; d < 3; ++d) {
		lo[d] = (int) std::floor(offset[d] / dx) - 1;
		hi[d] = (int) std::ceil((offset[d] + span[d]) / dx) + 2;
	}
	const std::string file = model["file"].string();
	if(file == "box") {
		return pio::sample_lattice(dx, lo, hi, [&](const std::array<float, 3>& p) {
			for(int d = 0; d < 3; ++d)
				if(p[d] < offset[d] || p[d] >= offset[d] + span[d]) return false;
			return true;
		});
	}
	if(file == "sphere") {
		const float c[3] = {offset[0] + 0.5f * span[0], offset[1] + 0.5f * span[1], offset[2] + 0.5f * span[2]};
		const float r	 = 0.5f * std::min(span[0], std::min(span[1], span[2]));
		return pio::sample_lattice(dx, lo, hi, [&](const std::array<float, 3>& p) {
			const float a = p[0] - c[0], b = p[1] - c[1], e = p[2] - c[2];
			return a * a + b * b + e * e <= r * r;
		});
	}
	if(file.size() > 4 && file.substr(file.size() - 4) == ".sdf") {
		pio::Sdf sdf;
		std::string path = file;
		if(!sdf.load(path)) path = scene_dir + "/" + file;
		if(sdf.phi.empty() && !sdf.load(path)) {
			std::fprintf(stderr, "cannot read level set %s\n", file.c_str());
			std::exit(EXIT_FAILURE);
		}
		// read_sdf (ParticleIO.hpp:32-70): the level set box is scaled uniformly into `span` and moved to `offset`
		float ext[3], scale = 1e30f;
		for(int d = 0; d < 3; ++d) {
			ext[d] = (float) sdf.n[d] * sdf.dx - sdf.mn[d];
			scale  = std::min(scale, span[d] / ext[d]);
		}
		return pio::sample_lattice(dx, lo, hi, [&](const std::array<float, 3>& p) {
			const float q[3] = {(p[0] - offset[0]) / scale + sdf.mn[0], (p[1] - offset[1]) / scale + sdf.mn[1], (p[2] - offset[2]) / scale + sdf.mn[2]};
			return sdf.sample(q[0], q[1], q[2]) < 0.f;
		});
	}
	std::fprintf(stderr, "unknown model file '%s' (expected *.sdf, *.obj, sphere or box)\n", file.c_str());
	std::exit(EXIT_FAILURE);
}

bool vec3(const mj::Value& v, const char* k, float (&out)[3]) {
	if(!v.has(k)) return false;
	for(int d = 0; d < 3; ++d) out[d] = (float) v[k][d].number();
	return true;
}

// The fields every entry of "colliders" shares: "type": "sticky|slip|separate", "friction", "velocity", "omega" (either of the last two makes it move).
bool parse_collider_motion(const mj::Value& c, mpm_collision_object& obj, bool& moving) {
	const std::string type = c.has("type") ? c["type"].string() : "sticky";
	obj.type			   = type == "sticky" ? MPM_BOUNDARY_STICKY : type == "slip" ? MPM_BOUNDARY_SLIP : type == "separate" ? MPM_BOUNDARY_SEPARATE : -1;
	if(obj.type < 0) {
		std::fprintf(stderr, "gmpm: unknown collider type '%s' (expected sticky, slip or separate)\n", type.c_str());
		return false;
	}
	obj.friction = num(c, "friction", obj.friction);
	if(vec3(c, "velocity", obj.trans_vel)) moving = true;
	if(vec3(c, "omega", obj.omega)) moving = true;
	return true;
}

// The two entries of "colliders" that install a volume - a local level-set box (mpm_set_collision_volume_mesh / mpm_set_collision_volume):
// {"shape": "mesh", "file": "body.obj", "spacing": s, "pad": 2, "scale": .., "offset": [..]}: the OBJ file's vertices, times the uniform scale,
//   plus the offset, sampled `spacing` apart in a box sized from the mesh with `pad` cells of margin; fills verts / tris;
// {"shape": "volume", "dims": [d0, d1, d2], "origin": [x, y, z], "spacing": s, "file": "body.f32"}: d0 d1 d2 samples {sdis, gx, gy, gz} of raw
//   little-endian float32, sample (i, j, k) at (i d1 + j) d2 + k; fills field4;
// both with the shared "type", "friction", "velocity", "omega" and "inside_out"; files are relative to the scene file.  They turn about the origin.
bool parse_volume_collider(const mj::Value& c, const std::string& shape, mpm_collision_object& obj, mpm_collision_volume& vol, bool& moving, std::vector<float>& verts, std::vector<int32_t>& tris,
						   std::vector<float>& field4, const std::string& scene_dir) {
	mpm_default_collision_object(&obj);
	std::memset(&vol, 0, sizeof(vol));
	if(!c.has("file") || !c.has("spacing")) {
		std::fprintf(stderr, "gmpm: collider '%s' lacks a field (file, spacing)\n", shape.c_str());
		return false;
	}
	const std::string name = c["file"].string();
	const std::string path = !name.empty() && name[0] == '/' ? name : scene_dir + "/" + name;
	vol.spacing			   = num(c, "spacing", 0.f);
	vol.inside_out		   = c.has("inside_out") && c["inside_out"].type == mj::Value::Bool && c["inside_out"].b;
	if(shape == "mesh") {
		if(!pio::read_obj_mesh(path, verts, tris) || verts.empty()) {
			std::fprintf(stderr, "gmpm: collider mesh file '%s' cannot be read as an OBJ mesh\n", path.c_str());
			return false;
		}
		const float scale = num(c, "scale", 1.f);
		float offset[3]	  = {0.f, 0.f, 0.f};
		vec3(c, "offset", offset);
		for(size_t i = 0; i < verts.size(); ++i) verts[i] = verts[i] * scale + offset[i % 3];
		vol.pad = (int) num(c, "pad", 2.f);
	} else {
		if(!c.has("dims") || c["dims"].type != mj::Value::Array || c["dims"].arr.size() != 3 || !vec3(c, "origin", vol.origin)) {
			std::fprintf(stderr, "gmpm: collider 'volume' needs \"dims\": [d0, d1, d2] and \"origin\": [x, y, z]\n");
			return false;
		}
		size_t n = 4;
		for(int d = 0; d < 3; ++d) {
			const double v = c["dims"][d].number();
			vol.dims[d]	   = (int) v;
			if((double) vol.dims[d] != v || vol.dims[d] < 2 || vol.dims[d] > MPM_VOLUME_MAX_SAMPLES) {
				std::fprintf(stderr, "gmpm: volume dims must be whole numbers 2 .. %d\n", (int) MPM_VOLUME_MAX_SAMPLES);
				return false;
			}
			n *= (size_t) vol.dims[d];
		}
		field4.assign(n, 0.f);
		std::ifstream f(path, std::ios::binary);
		if(!f || !f.read(reinterpret_cast<char*>(field4.data()), (std::streamsize) (n * sizeof(float))) || f.peek() != std::ifstream::traits_type::eof()) {
			std::fprintf(stderr, "gmpm: volume file '%s' does not hold exactly %zu float32 values\n", path.c_str(), n);
			return false;
		}
	}
	return parse_collider_motion(c, obj, moving);
}

// "body": {...} inside an entry of "colliders" makes that collider a rigid body (mpm_set_collider_body) once it is installed: "mass", "inertia"
// [xx, yy, zz, xy, xz, yz] and "com" [x, y, z], or "density" - which fills those not given from the analytic shape (sh) or the OBJ mesh (verts, tris)
// through mpm_shape_mass_properties / mpm_mesh_mass_properties -, "gravity" (default true), "lock": "x z rx ry", "force", "torque".  The entry's
// "velocity" and "omega" are the body's v0 and (true) angular velocity.
bool install_body(mpm_ctx* ctx, int slot, const mj::Value& b, const mpm_collision_shape* sh, const std::vector<float>& verts, const std::vector<int32_t>& tris) {
	mpm_rigid_body body;
	std::memset(&body, 0, sizeof(body));
	body.gravity = 1;
	if(b.has("density")) {
		const float rho = num(b, "density", 0.f);
		const int rc	= sh ? mpm_shape_mass_properties(sh, rho, &body) : mpm_mesh_mass_properties(verts.data(), verts.size() / 3, tris.data(), tris.size() / 3, rho, &body);
		if(rc) {
			std::fprintf(stderr, "gmpm: collider %d: \"density\" needs a sphere, a box, a capsule or a closed mesh, and a density > 0\n", slot);
			return false;
		}
	} else if(!b.has("mass") || !b.has("inertia") || !b.has("com")) {
		std::fprintf(stderr, "gmpm: collider %d: a body needs \"density\", or \"mass\", \"inertia\" and \"com\"\n", slot);
		return false;
	}
	body.mass = num(b, "mass", body.mass);
	if(b.has("inertia")) {
		if(b["inertia"].type != mj::Value::Array || b["inertia"].arr.size() != 6) {
			std::fprintf(stderr, "gmpm: collider %d: body \"inertia\" must be [xx, yy, zz, xy, xz, yz]\n", slot);
			return false;
		}
		for(int i = 0; i < 6; ++i) body.inertia[i] = (float) b["inertia"][i].number();
	}
	vec3(b, "com", body.com);
	vec3(b, "force", body.force);
	vec3(b, "torque", body.torque);
	if(b.has("gravity") && b["gravity"].type == mj::Value::Bool) body.gravity = b["gravity"].b ? 1 : 0;
	if(b.has("lock")) {
		std::istringstream words(b["lock"].string());
		for(std::string w; words >> w;) {
			static const char* names[6] = {"x", "y", "z", "rx", "ry", "rz"};
			int bit = -1;
			for(int i = 0; i < 6; ++i)
				if(w == names[i]) bit = i;
			if(bit < 0) {
				std::fprintf(stderr, "gmpm: collider %d: unknown body lock '%s' (expected x y z rx ry rz)\n", slot, w.c_str());
				return false;
			}
			body.lock |= 1 << bit;
		}
	}
	const int rc = mpm_set_collider_body(ctx, slot, &body);
	if(rc) die(ctx, rc);
	return true;
}

// One entry of "colliders": {"shape": "halfspace" ("point", "normal") | "sphere" ("center", "radius") | "box" ("center", "half_extents") |
// "capsule" ("a", "b", "radius") | "heightfield" (below) | "mesh" | "volume" (parse_volume_collider above), "type": "sticky|slip|separate", "friction", "velocity", "omega", "inside_out"}.  A collider with
// "velocity" or "omega" moves: it translates, and turns about its point / center / a, with the context's clock, which then starts at 0.
// {"shape": "heightfield", "nx", "nz", "origin": [x, z], "spacing", "heights": [nx nz numbers, sample (i, k) at i nz + k] | "file": "name.f32"
// (raw little-endian float32, nx nz values, relative to the scene file)} with the same "type", "friction", "velocity", "omega", "inside_out"
// installs a heightfield (mpm_set_collision_heightfield): `heights` is filled and hf.nx > 0 says so.  It turns about (origin x, 0, origin z).
bool parse_collider(const mj::Value& c, mpm_collision_object& obj, mpm_collision_shape& sh, bool& moving, mpm_heightfield& hf, std::vector<float>& heights, const std::string& scene_dir) {
	mpm_default_collision_object(&obj);
	std::memset(&sh, 0, sizeof(sh));
	std::memset(&hf, 0, sizeof(hf));
	const std::string shape = c.has("shape") ? c["shape"].string() : "";
	bool ok = true;
	if(shape == "heightfield") {
		if(!c.has("nx") || !c.has("nz") || !c.has("spacing") || (!c.has("heights") && !c.has("file"))) {
			std::fprintf(stderr, "gmpm: collider 'heightfield' lacks a field (nx, nz, spacing, heights or file)\n");
			return false;
		}
		const float fx = num(c, "nx", 0.f), fz = num(c, "nz", 0.f);
		hf.nx	   = (int) fx;
		hf.nz	   = (int) fz;
		hf.spacing = num(c, "spacing", 0.f);
		if((float) hf.nx != fx || (float) hf.nz != fz) {
			std::fprintf(stderr, "gmpm: heightfield nx, nz must be whole numbers\n");
			return false;
		}
		if(c.has("origin")) {
			if(c["origin"].type != mj::Value::Array || c["origin"].arr.size() != 2) {
				std::fprintf(stderr, "gmpm: heightfield 'origin' must be [x, z]\n");
				return false;
			}
			for(int d = 0; d < 2; ++d) hf.origin[d] = (float) c["origin"][d].number();
		}
		if(hf.nx < 2 || hf.nz < 2 || hf.nx > MPM_HEIGHTFIELD_MAX_SAMPLES || hf.nz > MPM_HEIGHTFIELD_MAX_SAMPLES) {
			std::fprintf(stderr, "gmpm: heightfield nx, nz must be 2 .. %d\n", (int) MPM_HEIGHTFIELD_MAX_SAMPLES);
			return false;
		}
		const size_t n = (size_t) hf.nx * hf.nz;
		heights.assign(n, 0.f);
		if(c.has("heights")) {
			if(c["heights"].arr.size() != n) {
				std::fprintf(stderr, "gmpm: heightfield 'heights' has %zu values, nx nz = %zu\n", c["heights"].arr.size(), n);
				return false;
			}
			for(size_t i = 0; i < n; ++i) heights[i] = (float) c["heights"][i].number();
		} else {
			const std::string name = c["file"].string();
			const std::string path = !name.empty() && name[0] == '/' ? name : scene_dir + "/" + name;
			std::ifstream f(path, std::ios::binary);
			if(!f || !f.read(reinterpret_cast<char*>(heights.data()), (std::streamsize) (n * sizeof(float))) || f.peek() != std::ifstream::traits_type::eof()) {
				std::fprintf(stderr, "gmpm: heightfield file '%s' does not hold exactly %zu float32 values\n", path.c_str(), n);
				return false;
			}
		}
		sh.a[0] = hf.origin[0];// the pivot of omega
		sh.a[2] = hf.origin[1];
		hf.inside_out = c.has("inside_out") && c["inside_out"].type == mj::Value::Bool && c["inside_out"].b;
	} else if(shape == "halfspace") {
		sh.kind = MPM_SHAPE_HALFSPACE;
		ok		= vec3(c, "point", sh.a) && vec3(c, "normal", sh.b);
	} else if(shape == "sphere") {
		sh.kind = MPM_SHAPE_SPHERE;
		ok		= vec3(c, "center", sh.a) && c.has("radius");
	} else if(shape == "box") {
		sh.kind = MPM_SHAPE_BOX;
		ok		= vec3(c, "center", sh.a) && vec3(c, "half_extents", sh.b);
	} else if(shape == "capsule") {
		sh.kind = MPM_SHAPE_CAPSULE;
		ok		= vec3(c, "a", sh.a) && vec3(c, "b", sh.b) && c.has("radius");
	} else {
		std::fprintf(stderr, "gmpm: unknown collider shape '%s' (expected halfspace, sphere, box, capsule, heightfield, mesh or volume)\n", shape.c_str());
		return false;
	}
	if(!ok) {
		std::fprintf(stderr, "gmpm: collider '%s' lacks a field\n", shape.c_str());
		return false;
	}
	sh.radius			   = num(c, "radius", 0.f);
	sh.inside_out		   = c.has("inside_out") && c["inside_out"].type == mj::Value::Bool && c["inside_out"].b;
	for(int d = 0; d < 3; ++d) obj.trans[d] = sh.a[d];// the pivot of omega
	return parse_collider_motion(c, obj, moving);
}

// The rows of xyz (n x 3 floats) in ascending order of their bits (x, then y, then z, as unsigned integers): two readouts of one state hold
// the same position bits, so equal ranks are the same particle.
std::vector<size_t> order_by_position_bits(const float* xyz, size_t n) {
	std::vector<size_t> order(n);
	for(size_t i = 0; i < n; ++i) order[i] = i;
	std::sort(order.begin(), order.end(), [xyz](size_t a, size_t b) {
		uint32_t ka[3], kb[3];
		std::memcpy(ka, xyz + 3 * a, sizeof(ka));
		std::memcpy(kb, xyz + 3 * b, sizeof(kb));
		return ka[0] != kb[0] ? ka[0] < kb[0] : ka[1] != kb[1] ? ka[1] < kb[1] : ka[2] < kb[2];
	});
	return order;
}

// The rows of a readout (xyz, n) in ascending id order: row src[j] of the readout is the particle with the j-th smallest id, which ids_sorted[j]
// then holds.  (ixyz, ids, ni): mpm_retrieve_ids of the same state - the same position bits.  Bit-identical positions are handed out in id order.
bool rows_by_id(const float* xyz, size_t n, const float* ixyz, const int32_t* ids, size_t ni, std::vector<size_t>& src, std::vector<int32_t>& ids_sorted) {
	if(n != ni) return false;
	auto less_bits = [](const float* a, const float* b) {
		uint32_t ka[3], kb[3];
		std::memcpy(ka, a, sizeof(ka));
		std::memcpy(kb, b, sizeof(kb));
		return ka[0] != kb[0] ? ka[0] < kb[0] : ka[1] != kb[1] ? ka[1] < kb[1] : ka[2] < kb[2];
	};
	std::vector<size_t> oa(n), ob(n);
	for(size_t i = 0; i < n; ++i) oa[i] = ob[i] = i;
	std::sort(oa.begin(), oa.end(), [&](size_t a, size_t b) {
		if(less_bits(ixyz + 3 * a, ixyz + 3 * b)) return true;
		if(less_bits(ixyz + 3 * b, ixyz + 3 * a)) return false;
		return ids[a] < ids[b];
	});
	std::stable_sort(ob.begin(), ob.end(), [&](size_t a, size_t b) { return less_bits(xyz + 3 * a, xyz + 3 * b); });
	std::vector<std::pair<int32_t, size_t>> pairs(n);
	for(size_t k = 0; k < n; ++k) {
		if(std::memcmp(ixyz + 3 * oa[k], xyz + 3 * ob[k], 3 * sizeof(float)) != 0) return false;
		pairs[k] = {ids[oa[k]], ob[k]};
	}
	std::sort(pairs.begin(), pairs.end());
	src.resize(n);
	ids_sorted.resize(n);
	for(size_t k = 0; k < n; ++k) ids_sorted[k] = pairs[k].first, src[k] = pairs[k].second;
	return true;
}
template<typename T>
void take_rows(std::vector<T>& a, int width, const std::vector<size_t>& src) {
	if(a.empty()) return;
	std::vector<T> out(src.size() * (size_t) width);
	for(size_t k = 0; k < src.size(); ++k)
		for(int d = 0; d < width; ++d) out[(size_t) width * k + d] = a[(size_t) width * src[k] + d];
	a.swap(out);
}
}// namespace

int main(int argc, char** argv) {
	std::string scene = "scene.json";
	for(int i = 1; i < argc; ++i) {
		if((!std::strcmp(argv[i], "-f") || !std::strcmp(argv[i], "--file")) && i + 1 < argc) scene = argv[++i];
	}
	std::ifstream in(scene);
	if(!in) {
		std::printf("file not exist %s\n", scene.c_str());
		return 1;
	}
	std::stringstream ss;
	ss << in.rdbuf();
	mj::ValuePtr doc;
	try {
		doc = mj::parse(ss.str());
	} catch(const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	const std::string scene_dir = scene.find('/') == std::string::npos ? "." : scene.substr(0, scene.rfind('/'));
	std::printf("load the scene file of size %zu\n", ss.str().size());

	const mj::Value& sim = (*doc)["simulation"];
	const int gpuid		 = (int) num(sim, "gpuid", 0);
	const int fps		 = (int) num(sim, "fps", 24);	   // DEFAULT_FPS, gmpm_simulator.cuh:27
	const int frames	 = (int) num(sim, "frames", 60);   // DEFAULT_FRAMES :28
	const float dt_def	 = num(sim, "default_dt", 1e-4f);// DEFAULT_DT :26
	const int bits		 = (int) num(sim, "domain_bits", 8);
	const std::string out_dir = sim.has("output_dir") ? sim["output_dir"].string() : ".";
	const bool out_vel		  = sim.has("output_velocity") && sim["output_velocity"].type == mj::Value::Bool && sim["output_velocity"].b;
	const bool out_stress	  = sim.has("output_stress") && sim["output_stress"].type == mj::Value::Bool && sim["output_stress"].b;
	const bool out_ids		  = sim.has("output_ids") && sim["output_ids"].type == mj::Value::Bool && sim["output_ids"].b;
	const bool out_loads	  = sim.has("output_loads") && sim["output_loads"].type == mj::Value::Bool && sim["output_loads"].b;
	const bool out_bodies	  = sim.has("output_bodies") && sim["output_bodies"].type == mj::Value::Bool && sim["output_bodies"].b;
	int grid_stride			  = 0;// simulation.output_grid: 0 = no grid files
	if(sim.has("output_grid")) {
		const mj::Value& og = sim["output_grid"];
		const float fs		= og.type == mj::Value::Object ? num(og, "stride", 1.f) : 0.f;
		grid_stride			= (int) fs;
		if((float) grid_stride != fs || (grid_stride != 1 && grid_stride != 2 && grid_stride != 4)) {
			std::fprintf(stderr, "gmpm: simulation.output_grid must be {\"stride\": 1, 2 or 4}\n");
			return 1;
		}
	}
	float surface_iso = 0.f;// simulation.output_surface: the iso value as a node mass, density * dx^3; 0 = no surface files
	if(sim.has("output_surface")) {
		const mj::Value& os = sim["output_surface"];
		const double rho	= os.type == mj::Value::Object ? (double) num(os, "density", 0.f) : 0.0;
		const double dx		= 1.0 / (double) (1 << bits);
		surface_iso			= (float) (rho * dx * dx * dx);
		if(!(surface_iso > 0.f) || !std::isfinite(surface_iso)) {
			std::fprintf(stderr, "gmpm: simulation.output_surface must be {\"density\": a positive number}\n");
			return 1;
		}
	}
	std::printf("simulation: gpuid[%d], defaultDt[%g], fps[%d], frames[%d]\n", gpuid, dt_def, fps, frames);

	mpm_config cfg;
	if(mpm_default_config(bits, &cfg)) die(nullptr, MPM_ERR_INVALID);
	cfg.max_ppc = (int) num(sim, "max_ppc", 128);
	cfg.gravity = num(sim, "gravity", cfg.gravity);
	mpm_ctx* ctx = nullptr;
	int rc		 = mpm_create(&cfg, gpuid, &ctx);
	if(rc) die(nullptr, rc);
	if(out_ids && (rc = mpm_track_particle_ids(ctx, 1))) die(ctx, rc);

	const mj::Value& models = (*doc)["models"];
	std::printf("has %zu models\n", models.arr.size());
	std::vector<size_t> counts;
	float max_v0 = 0.f;
	for(size_t mi = 0; mi < models.arr.size(); ++mi) {
		const mj::Value& m = models[mi];
		const int mat	   = material_of(m["constitutive"].string());
		if(mat < 0) {
			std::printf("Unknown constitutive: %s", m["constitutive"].string().c_str());
			continue;
		}
		std::printf("model constitutive[%s], file[%s]\n", m["constitutive"].string().c_str(), m["file"].string().c_str());
		mpm_material_params p;
		mpm_default_material(mat, bits, &p);
		// update_*_parameters, gmpm_simulator.cuh:211-254 (sand has no updater in the reference, gmpm.cu:134-135)
		if(mat != MPM_SAND) {
			p.rho	 = num(m, "rho", p.rho);
			p.volume = num(m, "volume", p.volume);
		}
		if(mat == MPM_FIXED_COROTATED || mat == MPM_NACC) {
			p.youngs_modulus = num(m, "youngs_modulus", p.youngs_modulus);
			p.poisson_ratio	 = num(m, "poisson_ratio", p.poisson_ratio);
		}
		if(mat == MPM_J_FLUID) {
			p.bulk		= num(m, "bulk_modulus", p.bulk);
			p.gamma		= num(m, "gamma", p.gamma);
			p.viscosity = num(m, "viscosity", p.viscosity);
		}
		if(mat == MPM_NACC) {
			p.beta = num(m, "beta", p.beta);
			p.xi   = num(m, "xi", p.xi);
		}
		// "velocity" is v0; "omega" / "velocity_gradient" (with an optional "pivot") make it the linear field of model_field.hpp
		pio::ModelField field;
		const int has_field = pio::parse_model_field(m, field);
		if(has_field < 0) return 1;
		float v0[3];
		for(int d = 0; d < 3; ++d) v0[d] = field.v0[d];
		if(!has_field) max_v0 = std::max(max_v0, std::sqrt(v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2]));
		int id = -1;
		pio::Points pts;
		const std::string file = m["file"].string();
		if(file.size() > 4 && file.substr(file.size() - 4) == ".obj") {
			// "file": "name.obj" (relative to the scene file), optional "margin": a closed triangle mesh filled with lattice particles on the device
			// (mpm_add_model_mesh).  As for a level set, the mesh's bounding box is scaled uniformly into `span` and moved to `offset`:
			// v' = (v - mn) s + offset per axis in float32, s = min over the axes of span / (mx - mn).
			const std::string path = !file.empty() && file[0] == '/' ? file : scene_dir + "/" + file;
			std::vector<float> verts;
			std::vector<int32_t> tris;
			if(!pio::read_obj_mesh(path, verts, tris) || verts.empty()) {
				std::fprintf(stderr, "gmpm: model file '%s' cannot be read as an OBJ mesh\n", path.c_str());
				return 1;
			}
			float mn[3] = {verts[0], verts[1], verts[2]}, mx[3] = {verts[0], verts[1], verts[2]}, scale = 1e30f;
			for(size_t i = 0; i < verts.size(); ++i) mn[i % 3] = std::min(mn[i % 3], verts[i]), mx[i % 3] = std::max(mx[i % 3], verts[i]);
			for(int d = 0; d < 3; ++d) scale = std::min(scale, (float) m["span"][d].number() / (mx[d] - mn[d]));
			for(size_t i = 0; i < verts.size(); ++i) {
				const float rel = verts[i] - mn[i % 3], scaled = rel * scale;
				verts[i]		= scaled + (float) m["offset"][i % 3].number();
			}
			mpm_mesh_fill opt;
			std::memset(&opt, 0, sizeof(opt));
			opt.margin = num(m, "margin", 0.f);
			size_t n   = 0;
			rc		   = mpm_add_model_mesh(ctx, mat, &p, verts.data(), verts.size() / 3, tris.data(), tris.size() / 3, &opt, v0, &id, &n);
			if(rc) die(ctx, rc);
			pts.resize(n);// frame 0 is written from the same sampler's points: the model's own array stays on the device
			if(n && (rc = mpm_sample_mesh(bits, verts.data(), verts.size() / 3, tris.data(), tris.size() / 3, &opt, pts[0].data(), &n, gpuid))) die(nullptr, rc);
		} else {
			pts = sample_model(m, bits, scene_dir);
			rc	= mpm_add_model(ctx, mat, &p, pts.empty() ? nullptr : pts[0].data(), pts.size(), v0, &id);
			if(rc) die(ctx, rc);
		}
		if(has_field) {
			if((rc = mpm_set_model_velocity_field(ctx, id, field.v0, field.grad9, field.pivot))) die(ctx, rc);
			for(const auto& x: pts) {// (the first dt follows the fastest particle)
				double v[3];
				field.at(x.data(), v);
				max_v0 = std::max(max_v0, (float) std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
			}
		}
		std::printf("init %d-th model with %zu particles\n", id, pts.size());
		const std::string frame0 = out_dir + "/model_id[" + std::to_string(id) + "]_frame[0].bgeo";
		if(out_vel || out_stress || out_ids) {
			std::vector<float> v(out_vel ? 3 * pts.size() : 0), s9(out_stress ? 9 * pts.size() : 0, 0.f);
			std::vector<int32_t> id0(out_ids ? pts.size() : 0);// (the sampled points are the input array: id = index)
			for(size_t i = 0; i < id0.size(); ++i) id0[i] = (int32_t) i;
			for(size_t i = 0; i < pts.size(); ++i) {
				double vi[3] = {v0[0], v0[1], v0[2]};
				if(has_field && out_vel) field.at(pts[i].data(), vi);
				for(int d = 0; d < 3 && out_vel; ++d) v[3 * i + d] = (float) vi[d];
				if(out_stress) s9[9 * i + 6] = 1.f;// J
			}
			pio::write_bgeo_frame(frame0, pts.empty() ? nullptr : pts[0].data(), pts.size(), out_vel ? v.data() : nullptr, out_stress ? s9.data() : nullptr, out_ids && !id0.empty() ? id0.data() : nullptr);
		} else
			pio::write_bgeo(frame0, pts.empty() ? nullptr : pts[0].data(), pts.size());
		counts.push_back(pts.size());
	}

	// "collision_mesh": {"file": "body.obj", "type": "sticky|slip|separate", "friction", "velocity", "omega", "inside_out", "scale": s, "offset": [x, y, z]}
	// installs the level-set collision object from a closed triangle mesh (mpm_set_collision_mesh): the OBJ file's vertices, times the uniform
	// scale, plus the offset.  It is a key of its own, not a collider: the mesh occupies the level-set object, not a slot.  It moves - about
	// the origin - with "velocity" or "omega", which start the clock as a moving collider does.
	bool mesh_moving = false;
	if(doc->has("collision_mesh")) {
		const mj::Value& cm = (*doc)["collision_mesh"];
		if(cm.type != mj::Value::Object || !cm.has("file")) {
			std::fprintf(stderr, "gmpm: collision_mesh must be an object with a \"file\"\n");
			return 1;
		}
		const std::string path = scene_dir + "/" + cm["file"].string();
		std::vector<float> verts;
		std::vector<int32_t> tris;
		if(!pio::read_obj_mesh(path, verts, tris)) {
			std::fprintf(stderr, "gmpm: collision_mesh file '%s' cannot be read as an OBJ mesh\n", path.c_str());
			return 1;
		}
		const float scale = num(cm, "scale", 1.f);
		float offset[3]	  = {0.f, 0.f, 0.f};
		vec3(cm, "offset", offset);
		for(size_t i = 0; i < verts.size(); ++i) verts[i] = verts[i] * scale + offset[i % 3];
		mpm_collision_object obj;
		mpm_default_collision_object(&obj);
		const std::string type = cm.has("type") ? cm["type"].string() : "sticky";
		obj.type			   = type == "sticky" ? MPM_BOUNDARY_STICKY : type == "slip" ? MPM_BOUNDARY_SLIP : type == "separate" ? MPM_BOUNDARY_SEPARATE : -1;
		if(obj.type < 0) {
			std::fprintf(stderr, "gmpm: unknown collision_mesh type '%s' (expected sticky, slip or separate)\n", type.c_str());
			return 1;
		}
		obj.friction = num(cm, "friction", obj.friction);
		if(vec3(cm, "velocity", obj.trans_vel)) mesh_moving = true;
		if(vec3(cm, "omega", obj.omega)) mesh_moving = true;
		mpm_collision_mesh opt;
		std::memset(&opt, 0, sizeof(opt));
		opt.inside_out = cm.has("inside_out") && cm["inside_out"].type == mj::Value::Bool && cm["inside_out"].b;
		if((rc = mpm_set_collision_mesh(ctx, &obj, &opt, verts.data(), verts.size() / 3, tris.data(), tris.size() / 3))) die(ctx, rc);
		std::printf("has a collision mesh of %zu triangles%s\n", tris.size() / 3, mesh_moving ? ", clock running" : "");
	}

	// "colliders": analytic collision shapes (mpm_set_collision_shape), at most MPM_MAX_COLLISION_SHAPES, slot = position in the array
	int bodies = 0;// bit s: slot s is a rigid body ("body": {...} in its entry)
	if(doc->has("colliders")) {
		const mj::Value& cols = (*doc)["colliders"];
		if(cols.arr.size() > (size_t) MPM_MAX_COLLISION_SHAPES) {
			std::fprintf(stderr, "gmpm: %zu colliders, at most %d\n", cols.arr.size(), (int) MPM_MAX_COLLISION_SHAPES);
			return 1;
		}
		bool moving = false;
		for(size_t ci = 0; ci < cols.arr.size(); ++ci) {
			mpm_collision_object obj;
			mpm_collision_shape sh;
			mpm_heightfield hf;
			std::vector<float> heights;
			const std::string shape = cols[ci].has("shape") ? cols[ci]["shape"].string() : "";
			if(shape == "mesh" || shape == "volume") {// a volume in this slot, built from an OBJ mesh or given as samples
				mpm_collision_volume vol;
				std::vector<float> verts, field4;
				std::vector<int32_t> tris;
				if(!parse_volume_collider(cols[ci], shape, obj, vol, moving, verts, tris, field4, scene_dir)) return 1;
				rc = shape == "mesh" ? mpm_set_collision_volume_mesh(ctx, (int) ci, &obj, &vol, verts.data(), verts.size() / 3, tris.data(), tris.size() / 3)
									 : mpm_set_collision_volume(ctx, (int) ci, &obj, &vol, field4.data());
				if(rc) die(ctx, rc);
				if(cols[ci].has("body")) {
					if(!install_body(ctx, (int) ci, cols[ci]["body"], nullptr, verts, tris)) return 1;
					bodies |= 1 << ci;
				}
				continue;
			}
			if(!parse_collider(cols[ci], obj, sh, moving, hf, heights, scene_dir)) return 1;
			rc = hf.nx ? mpm_set_collision_heightfield(ctx, (int) ci, &obj, &hf, heights.data()) : mpm_set_collision_shape(ctx, (int) ci, &obj, &sh);
			if(rc) die(ctx, rc);
			if(cols[ci].has("body")) {
				if(!install_body(ctx, (int) ci, cols[ci]["body"], hf.nx ? nullptr : &sh, {}, {})) return 1;
				bodies |= 1 << ci;
			}
		}
		std::printf("has %zu colliders%s\n", cols.arr.size(), moving ? ", clock running" : "");
		if(moving && (rc = mpm_set_collision_clock(ctx, 1, 0.f))) die(ctx, rc);// one clock for all of them, started after the last install
	}
	if(mesh_moving && (rc = mpm_set_collision_clock(ctx, 1, 0.f))) die(ctx, rc);// (every install above stopped it)

	// main_loop, gmpm_simulator.cuh:303-592
	const float spf = 1.f / (float) fps;
	float dt		= mpm_compute_dt(ctx, max_v0, 0.f, spf, dt_def);
	rc				= mpm_initial_setup(ctx);
	if(rc) die(ctx, rc);
	mpm_counts c;
	mpm_get_counts(ctx, &c);
	std::printf("block count on device %d: %d, %d, %d\n", gpuid, c.particle_blocks, c.neighbor_blocks, c.exterior_blocks);
	float cur_time = 0.f;
	long steps	   = 0;
	// "emitters": particle sources (emitter_rule.hpp), served at every substep boundary - after set-up and after each mpm_substep: what is due goes
	// to its model through mpm_emit_particles with the emitter's velocity, and the frames of that model carry more points from then on
	std::vector<pio::Emitter> emitters;
	if(doc->has("emitters")) {
		const mj::Value& list = (*doc)["emitters"];
		for(size_t ei = 0; ei < list.arr.size(); ++ei) {
			pio::Emitter em;
			if(!pio::parse_emitter(list[ei], bits, em)) return 1;
			if(em.model < 0 || em.model >= (int) counts.size()) {
				std::fprintf(stderr, "gmpm: an emitter names model %d, the scene has %zu\n", em.model, counts.size());
				return 1;
			}
			emitters.push_back(std::move(em));
		}
		std::printf("has %zu emitters\n", emitters.size());
	}
	auto serve_emitters = [&](double t) {
		for(auto& em: emitters) {
			const std::vector<float> pts = em.due(t);
			if(pts.empty()) continue;
			const float v[3] = {(float) em.velocity[0], (float) em.velocity[1], (float) em.velocity[2]};
			const int re	 = mpm_emit_particles(ctx, em.model, pts.data(), pts.size() / 3, v, nullptr, nullptr);
			if(re) die(ctx, re);
			counts[em.model] += pts.size() / 3;
		}
	};
	// "sinks": particle sinks (sink_rule.hpp), swept at every substep boundary before the emitters are served: a sink with a sweep due takes the
	// particles of its model(s) that lie in its region out through mpm_remove_particles, and the frames carry fewer points from then on.
	// simulation.output_removed: removed_frame[f].json holds what the sinks took since the last frame - per-model counts, mass and momentum
	struct SceneSink {
		pio::Sink rule;
		mpm_collision_shape region;
	};
	std::vector<SceneSink> sinks;
	const bool out_removed = sim.has("output_removed") && sim["output_removed"].type == mj::Value::Bool && sim["output_removed"].b;
	if(doc->has("sinks")) {
		const mj::Value& list = (*doc)["sinks"];
		for(size_t si = 0; si < list.arr.size(); ++si) {
			SceneSink sk;
			mpm_collision_object obj;
			mpm_heightfield hf;
			std::vector<float> heights;
			bool moving = false;
			if(!pio::parse_sink(list[si], sk.rule) || !parse_collider(list[si], obj, sk.region, moving, hf, heights, scene_dir)) return 1;
			if(hf.nx > 0 || moving) {
				std::fprintf(stderr, "gmpm: a sink is a halfspace, sphere, box or capsule at rest\n");
				return 1;
			}
			if(sk.rule.model < -1 || sk.rule.model >= (int) counts.size()) {
				std::fprintf(stderr, "gmpm: a sink names model %d, the scene has %zu\n", sk.rule.model, counts.size());
				return 1;
			}
			sinks.push_back(sk);
		}
		std::printf("has %zu sinks\n", sinks.size());
	}
	long long removed_since[8] = {0};
	double removed_mass = 0.0, removed_momentum[3] = {0.0, 0.0, 0.0};
	auto serve_sinks = [&](double t) {
		for(auto& sk: sinks) {
			if(!sk.rule.due(t)) continue;
			mpm_removal what;
			std::memset(&what, 0, sizeof(what));
			what.regions  = &sk.region;
			what.nregions = 1;
			mpm_removal_result res;
			const int rr = mpm_remove_particles(ctx, sk.rule.model, &what, &res);
			if(rr) die(ctx, rr);
			for(size_t mi = 0; mi < counts.size(); ++mi) removed_since[mi] += (long long) res.removed[mi];
			removed_mass += res.mass;
			for(int d = 0; d < 3; ++d) removed_momentum[d] += res.momentum[d];
		}
	};
	auto write_removed = [&](int frame) {
		FILE* f = std::fopen((out_dir + "/removed_frame[" + std::to_string(frame) + "].json").c_str(), "w");
		if(!f) {
			std::fprintf(stderr, "gmpm: cannot write the removed particles of frame %d\n", frame);
			std::exit(1);
		}
		std::fprintf(f, "{\"frame\": %d, \"removed\": [", frame);
		for(size_t mi = 0; mi < counts.size(); ++mi) std::fprintf(f, "%s%lld", mi ? ", " : "", removed_since[mi]);
		std::fprintf(f, "], \"mass\": %.17g, \"momentum\": [%.17g, %.17g, %.17g]}\n", removed_mass, removed_momentum[0], removed_momentum[1], removed_momentum[2]);
		std::fclose(f);
		for(auto& k: removed_since) k = 0;
		removed_mass = removed_momentum[0] = removed_momentum[1] = removed_momentum[2] = 0.0;
	};
	// "forces": force fields (force_rule.hpp), entry i in slot i: installed and removed through mpm_set_force_field at the substep boundaries, before
	// the sinks and the emitters are served.  "region" holds the shape keys of "colliders" (halfspace, sphere, box or capsule, at rest).
	struct SceneForce {
		pio::ForceRule rule;
		mpm_force_field field;
	};
	std::vector<SceneForce> forces;
	if(doc->has("forces")) {
		const mj::Value& list = (*doc)["forces"];
		if(list.arr.size() > MPM_MAX_FORCE_FIELDS) {
			std::fprintf(stderr, "gmpm: a scene holds at most %d forces\n", (int) MPM_MAX_FORCE_FIELDS);
			return 1;
		}
		for(size_t fi = 0; fi < list.arr.size(); ++fi) {
			const mj::Value& e = list[fi];
			SceneForce sf;
			std::memset(&sf.field, 0, sizeof(sf.field));
			pio::parse_force_rule(e, sf.rule);
			const std::string kind = e.has("kind") ? e["kind"].string() : "";
			sf.field.kind = kind == "uniform" ? MPM_FORCE_UNIFORM : kind == "point" ? MPM_FORCE_POINT : kind == "vortex" ? MPM_FORCE_VORTEX : kind == "drag" ? MPM_FORCE_DRAG : 0;
			if(!sf.field.kind) {
				std::fprintf(stderr, "gmpm: unknown force kind '%s' (expected uniform, point, vortex or drag)\n", kind.c_str());
				return 1;
			}
			vec3(e, "vec", sf.field.vec);
			vec3(e, "centre", sf.field.centre);
			sf.field.falloff  = (int) num(e, "falloff", 0.f);
			sf.field.strength = num(e, "strength", 0.f);
			sf.field.swirl	  = num(e, "swirl", 0.f);
			sf.field.pull	  = num(e, "pull", 0.f);
			sf.field.lift	  = num(e, "lift", 0.f);
			sf.field.soft	  = num(e, "soft", 0.f);
			sf.field.feather  = num(e, "feather", 0.f);
			if(e.has("region")) {
				mpm_collision_object obj;
				mpm_heightfield hf;
				std::vector<float> heights;
				bool moving = false;
				if(!parse_collider(e["region"], obj, sf.field.region, moving, hf, heights, scene_dir)) return 1;
				if(hf.nx > 0 || moving) {
					std::fprintf(stderr, "gmpm: a force's region is a halfspace, sphere, box or capsule at rest\n");
					return 1;
				}
			}
			forces.push_back(sf);
		}
		std::printf("has %zu forces\n", forces.size());
	}
	auto serve_forces = [&](double t) {
		for(size_t fi = 0; fi < forces.size(); ++fi) {
			const int act = forces[fi].rule.due(t);
			if(!act) continue;
			const int rf = mpm_set_force_field(ctx, (int) fi, act > 0 ? &forces[fi].field : nullptr);
			if(rf) die(ctx, rf);
		}
	};
	if(!forces.empty()) serve_forces(0.0);
	if(!sinks.empty()) serve_sinks(0.0);
	serve_emitters(0.0);
	std::vector<float> buf, vbuf, sbuf;
	pio::AsyncWriter io;
	// simulation.output_surface: the iso-surface of the mass grid beside the frame (frame 0: the grid of the set-up's P2G): count, then fetch
	auto write_surface = [&](int frame) {
		size_t nt = 0;
		int rs	  = mpm_grid_isosurface(ctx, surface_iso, nullptr, nullptr, nullptr, nullptr, &nt);
		if(rs) die(ctx, rs);
		std::vector<float> tris(9 * nt);
		if(nt && (rs = mpm_grid_isosurface(ctx, surface_iso, nullptr, nullptr, tris.data(), nullptr, &nt))) die(ctx, rs);
		io.write_obj_surface_async(out_dir + "/surface_frame[" + std::to_string(frame) + "].obj", std::move(tris));
	};
	if(surface_iso > 0.f) write_surface(0);
	// simulation.output_loads: the load gauge (mpm_load_gauge) runs over every frame; loads_frame[f].json holds, per row, the force and torque on the
	// collider averaged over the frame's substeps, the touched-node count summed over them and the elapsed time, read and zeroed at the frame's end
	if(out_loads && (rc = mpm_load_gauge(ctx, 1, nullptr))) die(ctx, rc);
	auto write_loads = [&](int frame) {
		double rows[MPM_LOAD_ROWS][8], elapsed = 0.0;
		int updates = 0;
		int rs		= mpm_load_gauge_read(ctx, rows, &elapsed, &updates, 1);
		if(rs) die(ctx, rs);
		static const char* names[MPM_LOAD_ROWS] = {"field", "slot0", "slot1", "slot2", "slot3", "walls"};
		FILE* f = std::fopen((out_dir + "/loads_frame[" + std::to_string(frame) + "].json").c_str(), "w");
		if(!f) {
			std::fprintf(stderr, "gmpm: cannot write the loads of frame %d\n", frame);
			std::exit(1);
		}
		std::fprintf(f, "{\"frame\": %d, \"elapsed\": %.17g, \"updates\": %d, \"rows\": {", frame, elapsed, updates);
		for(int r = 0; r < MPM_LOAD_ROWS; ++r) {
			const double* a = rows[r];
			auto per = [&](double x) { return elapsed > 0.0 ? x / elapsed : 0.0; };
			std::fprintf(f, "%s\n  \"%s\": {\"count\": %.17g, \"mass\": %.17g, \"impulse\": [%.17g, %.17g, %.17g], \"angular_impulse\": [%.17g, %.17g, %.17g], \"force\": [%.17g, %.17g, %.17g], \"torque\": [%.17g, %.17g, %.17g]}", r ? "," : "",
						 names[r], a[0], a[7], a[1], a[2], a[3], a[4], a[5], a[6], per(a[1]), per(a[2]), per(a[3]), per(a[4]), per(a[5]), per(a[6]));
		}
		std::fprintf(f, "\n}}\n");
		std::fclose(f);
	};
	// simulation.output_bodies: bodies_frame[f].json beside each frame holds every rigid body's pose, velocities and last impulse (mpm_get_collider_body)
	auto write_bodies = [&](int frame) {
		FILE* f = std::fopen((out_dir + "/bodies_frame[" + std::to_string(frame) + "].json").c_str(), "w");
		if(!f) {
			std::fprintf(stderr, "gmpm: cannot write the bodies of frame %d\n", frame);
			std::exit(1);
		}
		std::fprintf(f, "{\"frame\": %d, \"bodies\": {", frame);
		bool first = true;
		for(int s = 0; s < MPM_MAX_COLLISION_SHAPES; ++s) {
			if(!((bodies >> s) & 1)) continue;
			mpm_rigid_body_state st;
			int rs = mpm_get_collider_body(ctx, s, nullptr, &st);
			if(rs) die(ctx, rs);
			std::fprintf(f, "%s\n  \"slot%d\": {\"position\": [%.17g, %.17g, %.17g], \"orientation\": [%.17g, %.17g, %.17g, %.17g], \"velocity\": [%.17g, %.17g, %.17g], \"omega\": [%.17g, %.17g, %.17g], "
					"\"angular_momentum\": [%.17g, %.17g, %.17g], \"last_impulse\": [%.17g, %.17g, %.17g], \"last_angular_impulse\": [%.17g, %.17g, %.17g], \"last_touched_mass\": %.17g, "
					"\"max_mass_ratio\": %.17g, \"last_touched_nodes\": %lld, \"updates\": %lld}",
					first ? "" : ",", s, st.position[0], st.position[1], st.position[2], st.orientation[0], st.orientation[1], st.orientation[2], st.orientation[3], st.velocity[0], st.velocity[1],
					st.velocity[2], st.omega[0], st.omega[1], st.omega[2], st.angular_momentum[0], st.angular_momentum[1], st.angular_momentum[2], st.last_impulse[0], st.last_impulse[1],
					st.last_impulse[2], st.last_angular_impulse[0], st.last_angular_impulse[1], st.last_angular_impulse[2], st.last_touched_mass, st.max_mass_ratio,
					(long long) st.last_touched_nodes, (long long) st.updates);
			first = false;
		}
		std::fprintf(f, "\n}}\n");
		std::fclose(f);
	};
	const auto wall0 = std::chrono::steady_clock::now();
	for(int frame = 1; frame <= frames; ++frame) {
		for(float t = 0.f; t < spf;) {
			float next_dt = dt, max_vel = 0.f;
			rc = mpm_substep(ctx, dt, t, spf, dt_def, &next_dt, &max_vel);
			if(rc == MPM_ERR_NONFINITE) {
				std::cout << "Maximum velocity is infinity" << std::endl;
				frame = frames + 1;
				break;
			}
			if(rc) die(ctx, rc);
			t += dt;
			cur_time += dt;
			dt = next_dt;
			++steps;
			if(!forces.empty()) serve_forces((double) cur_time);
			if(!sinks.empty()) serve_sinks((double) cur_time);
			if(!emitters.empty()) serve_emitters((double) cur_time);
		}
		if(frame > frames) break;
		mpm_get_counts(ctx, &c);
		mpm_timers tm;
		mpm_get_timers(ctx, &tm);
		std::printf("frame %d: t %.6f, %ld substeps, blocks %d/%d/%d, last substep: grid %.3f ms g2p2g %.3f ms partition %.3f ms\n", frame, cur_time, steps, c.particle_blocks, c.neighbor_blocks, c.exterior_blocks, tm.grid_update_ms, tm.g2p2g_ms, tm.partition_ms);
		if(grid_stride) {// the Eulerian side of the frame: the whole domain at the asked stride
			const int origin[3] = {0, 0, 0};
			const int cells		= (1 << bits) / grid_stride;
			const int dims[3]	= {cells, cells, cells};
			std::vector<float> vol((size_t) 4 * cells * cells * cells);
			rc = mpm_grid_volume(ctx, origin, dims, grid_stride, vol.data());
			if(rc) die(ctx, rc);
			io.write_npy_f32_async(out_dir + "/grid_frame[" + std::to_string(frame) + "].npy", std::move(vol), {4, (size_t) cells, (size_t) cells, (size_t) cells});
		}
		if(surface_iso > 0.f) write_surface(frame);
		if(out_loads) write_loads(frame);
		if(out_bodies) write_bodies(frame);
		if(out_removed) write_removed(frame);
		for(size_t mi = 0; mi < counts.size(); ++mi) {// output_model, :594-634
			buf.resize(3 * counts[mi]);
			vbuf.clear();
			sbuf.clear();
			size_t n = counts[mi];
			if(out_vel) {
				vbuf.resize(3 * counts[mi]);
				rc = mpm_retrieve_velocity(ctx, (int) mi, buf.data(), vbuf.data(), nullptr, &n);
			} else if(!out_stress && !out_ids)
				rc = mpm_retrieve_positions(ctx, (int) mi, buf.data(), &n);
			if(rc) die(ctx, rc);
			if(out_stress) {
				std::vector<float> sx(3 * counts[mi]), s6(6 * counts[mi]), sc(3 * counts[mi]);
				size_t ns = counts[mi];
				rc		  = mpm_retrieve_stress(ctx, (int) mi, sx.data(), s6.data(), sc.data(), &ns);
				if(rc) die(ctx, rc);
				// row k of the stress readout goes where the velocity readout has the same position bits (alone: its own order)
				std::vector<size_t> to(ns);
				if(out_vel) {
					const std::vector<size_t> ov = order_by_position_bits(buf.data(), n), os = order_by_position_bits(sx.data(), ns);
					bool same = n == ns;
					for(size_t k = 0; same && k < ns; ++k) {
						same  = std::memcmp(&buf[3 * ov[k]], &sx[3 * os[k]], 3 * sizeof(float)) == 0;
						to[os[k]] = ov[k];
					}
					if(!same) {
						std::fprintf(stderr, "gmpm: the velocity and stress readouts of model %zu do not hold the same positions\n", mi);
						die(ctx, MPM_ERR_INTERNAL);
					}
				} else {
					for(size_t k = 0; k < ns; ++k) to[k] = k;
					buf.swap(sx);
					n = ns;
				}
				sbuf.resize(9 * ns);
				for(size_t k = 0; k < ns; ++k) {
					for(int d = 0; d < 6; ++d) sbuf[9 * to[k] + d] = s6[6 * k + d];
					for(int d = 0; d < 3; ++d) sbuf[9 * to[k] + 6 + d] = sc[3 * k + d];
				}
			}
			std::vector<int32_t> ibuf;
			if(out_ids) {// the frame's rows in ascending id order
				std::vector<float> ix(3 * counts[mi]);
				std::vector<int32_t> ids(counts[mi]);
				size_t ni = counts[mi];
				rc		  = mpm_retrieve_ids(ctx, (int) mi, ix.data(), ids.data(), &ni);
				if(rc) die(ctx, rc);
				if(!out_vel && !out_stress) {
					buf = ix;
					n	= ni;
				}
				std::vector<size_t> src;
				if(!rows_by_id(buf.data(), n, ix.data(), ids.data(), ni, src, ibuf)) {
					std::fprintf(stderr, "gmpm: the id readout of model %zu does not hold the positions of the frame\n", mi);
					die(ctx, MPM_ERR_INTERNAL);
				}
				buf.resize(3 * n);
				take_rows(buf, 3, src);
				if(!vbuf.empty()) vbuf.resize(3 * n);
				take_rows(vbuf, 3, src);
				take_rows(sbuf, 9, src);
			}
			std::printf("total number of particles %zu\n", n);
			// IO::insert_job (gmpm_simulator.cuh:626-632): the frame is written by the IO thread while the next frame is computed
			const std::string fn = out_dir + "/model_id[" + std::to_string(mi) + "]_frame[" + std::to_string(frame) + "].bgeo";
			if(out_vel || out_stress || out_ids)
				io.write_bgeo_frame_async(fn, buf, vbuf, sbuf, n, ibuf);
			else
				io.write_bgeo_async(fn, buf, n);
		}
	}
	io.flush();// IO::flush() at the end of main_loop (gmpm_simulator.cuh:591)
	const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
	std::printf("done: %ld substeps in %.3f s\n", steps, wall);
	mpm_destroy(ctx);
	return 0;
}
