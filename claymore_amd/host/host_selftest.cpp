// host_selftest.cpp — exercises the pieces of the host drivers that need no GPU (JSON reader, lattice sampler, BGEO
// writer, NumPy writer, OBJ reader, the collision mesh's validation and closest-point functions, the mesh-sampled model per point, the volume collider's query per point).  usage: host_selftest <out.bgeo>  -> prints "json_ok <n_models> <dt>", "sphere <count>", "bgeo <bytes>"
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "mini_json.hpp"
#include "particle_io.hpp"
#include "model_field.hpp"
#include "emitter_rule.hpp"
#include "sink_rule.hpp"
#include "force_rule.hpp"
#include "../csrc/mpm_collision_mesh.hpp"
#include "../csrc/mpm_mesh_fill.hpp"
#if !defined(__HIPCC__)
struct float4 {
	float x, y, z, w;
};
#endif
#include "../csrc/mpm_collision_volume.hpp"

int main(int argc, char** argv) {
	if(argc == 3 && !std::strcmp(argv[1], "--model-field")) {// host_selftest --model-field '{"velocity": .., "omega": .., "pivot": ..}': a scene file's model object ->
		// "field|none", then v0 (3), grad9 column-major (9), pivot (3) as gmpm hands them to mpm_set_model_velocity_field, and the velocity at (1, 2, 3)
		mj::ValuePtr m;
		try {
			m = mj::parse(argv[2]);
		} catch(const std::exception& e) {
			std::cerr << "cannot parse the model object: " << e.what() << "\n";
			return 2;
		}
		pio::ModelField f;
		const int rc = pio::parse_model_field(*m, f);
		if(rc < 0) return 1;
		std::cout << (rc ? "field" : "none");
		for(float x: f.v0) std::cout << " " << x;
		for(float x: f.grad9) std::cout << " " << x;
		for(float x: f.pivot) std::cout << " " << x;
		const float at[3] = {1.f, 2.f, 3.f};
		double v[3];
		f.at(at, v);
		std::cout << " " << v[0] << " " << v[1] << " " << v[2] << "\n";
		return 0;
	}
	if(argc >= 5 && !std::strcmp(argv[1], "--emitter")) {// host_selftest --emitter '{"shape": .., "velocity": .., ..}' BITS T1 [T2 ..]: an entry of a scene file's "emitters" ->
		// per substep boundary (ascending times, as decimal or hex floats) "due N", then the N points gmpm would emit there, "x y z" as float32 bits in hex
		mj::ValuePtr e;
		try {
			e = mj::parse(argv[2]);
		} catch(const std::exception& ex) {
			std::cerr << "cannot parse the emitter object: " << ex.what() << "\n";
			return 2;
		}
		pio::Emitter em;
		if(!pio::parse_emitter(*e, std::atoi(argv[3]), em)) return 1;
		for(int i = 4; i < argc; ++i) {
			const std::vector<float> pts = em.due(std::strtod(argv[i], nullptr));
			std::printf("due %zu\n", pts.size() / 3);
			for(size_t p = 0; p < pts.size(); p += 3) {
				uint32_t b[3];
				std::memcpy(b, &pts[p], sizeof(b));
				std::printf("%08x %08x %08x\n", b[0], b[1], b[2]);
			}
		}
		return 0;
	}
	if(argc >= 4 && !std::strcmp(argv[1], "--sink")) {// host_selftest --sink '{"period": .., "start": .., "end": .., "model": ..}' T1 [T2 ..]: an entry of a scene file's "sinks" ->
		// "model M", then per substep boundary (ascending times, as decimal or hex floats) "due K": the sweeps gmpm's one call there serves
		mj::ValuePtr e;
		try {
			e = mj::parse(argv[2]);
		} catch(const std::exception& ex) {
			std::cerr << "cannot parse the sink object: " << ex.what() << "\n";
			return 2;
		}
		pio::Sink sk;
		if(!pio::parse_sink(*e, sk)) return 1;
		std::printf("model %d\n", sk.model);
		for(int i = 3; i < argc; ++i) std::printf("due %ld\n", sk.due(std::strtod(argv[i], nullptr)));
		return 0;
	}
	if(argc >= 4 && !std::strcmp(argv[1], "--force")) {// host_selftest --force '{"start": .., "end": ..}' T1 [T2 ..]: the times of an entry of a scene file's "forces" ->
		// per substep boundary (ascending times) what gmpm does there: 1 install, -1 remove, 0 nothing
		mj::ValuePtr e;
		try {
			e = mj::parse(argv[2]);
		} catch(const std::exception& ex) {
			std::cerr << "cannot parse the force object: " << ex.what() << "\n";
			return 2;
		}
		pio::ForceRule fr;
		pio::parse_force_rule(*e, fr);
		for(int i = 3; i < argc; ++i) std::printf("%d\n", fr.due(std::strtod(argv[i], nullptr)));
		return 0;
	}
	if(argc == 4 && !std::strcmp(argv[1], "--bgeo-from")) {// host_selftest --bgeo-from points.f32 out.bgeo: raw float32 xyz -> BGEO frame
		std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
		if(!in) return 3;
		const size_t bytes = (size_t) in.tellg();
		std::vector<float> xyz(bytes / sizeof(float));
		in.seekg(0);
		in.read(reinterpret_cast<char*>(xyz.data()), (std::streamsize) bytes);
		return pio::write_bgeo(argv[3], xyz.data(), xyz.size() / 3) ? 0 : 4;
	}
	if(argc == 5 && !std::strcmp(argv[1], "--bgeo-v-from")) {// host_selftest --bgeo-v-from points.f32 vel.f32 out.bgeo: the same with the "v" attribute
		std::vector<float> arr[2];
		for(int a = 0; a < 2; ++a) {
			std::ifstream in(argv[2 + a], std::ios::binary | std::ios::ate);
			if(!in) return 3;
			const size_t bytes = (size_t) in.tellg();
			arr[a].resize(bytes / sizeof(float));
			in.seekg(0);
			in.read(reinterpret_cast<char*>(arr[a].data()), (std::streamsize) bytes);
		}
		if(arr[0].size() != arr[1].size()) return 5;
		return pio::write_bgeo(argv[4], arr[0].data(), arr[0].size() / 3, arr[1].data()) ? 0 : 4;
	}
	if(argc == 5 && !std::strcmp(argv[1], "--bgeo-stress-from")) {// host_selftest --bgeo-stress-from points.f32 stress9.f32 out.bgeo: "stress", "J", "pressure", "vonmises"
		std::vector<float> arr[2];
		for(int a = 0; a < 2; ++a) {
			std::ifstream in(argv[2 + a], std::ios::binary | std::ios::ate);
			if(!in) return 3;
			const size_t bytes = (size_t) in.tellg();
			arr[a].resize(bytes / sizeof(float));
			in.seekg(0);
			in.read(reinterpret_cast<char*>(arr[a].data()), (std::streamsize) bytes);
		}
		if(arr[0].size() * 3 != arr[1].size()) return 5;
		return pio::write_bgeo_frame(argv[4], arr[0].data(), arr[0].size() / 3, nullptr, arr[1].data()) ? 0 : 4;
	}
	if(argc == 7 && !std::strcmp(argv[1], "--npy-from")) {// host_selftest --npy-from raw.f32 d0 d1 d2 out.npy: 4 d0 d1 d2 raw float32 values -> a grid volume's NumPy file, shape (4, d0, d1, d2)
		std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
		if(!in) return 3;
		const size_t bytes = (size_t) in.tellg();
		std::vector<float> v(bytes / sizeof(float));
		in.seekg(0);
		in.read(reinterpret_cast<char*>(v.data()), (std::streamsize) bytes);
		std::vector<size_t> shape {4};
		for(int a = 3; a < 6; ++a) shape.push_back((size_t) std::strtoull(argv[a], nullptr, 10));
		if(4 * shape[1] * shape[2] * shape[3] != v.size()) return 5;
		return pio::write_npy_f32(argv[6], v.data(), shape) ? 0 : 4;
	}
	if(argc == 4 && !std::strcmp(argv[1], "--obj-from")) {// host_selftest --obj-from soup.f32 out.obj: 9 raw float32 values a triangle -> the welded OBJ file of a surface
		std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
		if(!in) return 3;
		const size_t bytes = (size_t) in.tellg();
		std::vector<float> v(bytes / sizeof(float));
		in.seekg(0);
		in.read(reinterpret_cast<char*>(v.data()), (std::streamsize) bytes);
		if(v.size() % 9) return 5;
		return pio::write_obj_surface(argv[3], v.data(), v.size() / 9) ? 0 : 4;
	}
	if(argc == 3 && !std::strcmp(argv[1], "--mesh-check")) {// host_selftest --mesh-check FILE.obj: what mpm_set_collision_mesh's validation says about a mesh
		std::vector<float> verts;
		std::vector<int32_t> tris;
		if(!pio::read_obj_mesh(argv[2], verts, tris)) return 3;
		std::vector<mpm::MeshTri> rec;
		std::vector<mpm::MeshPseudo> pseudo;
		mpm::MeshReport rep;
		mpm::mesh_build(verts.data(), verts.size() / 3, tris.data(), tris.size() / 3, (size_t) 1 << 22, (size_t) 1 << 22, rec, pseudo, rep);
		std::printf("nv %zu\nnt %zu\nclosed %d\nvolume %.17g\nverdict %s\n", verts.size() / 3, tris.size() / 3, rep.closed ? 1 : 0, rep.volume, rep.reason.empty() ? "ok" : rep.reason.c_str());
		return 0;
	}
	if(argc == 4 && !std::strcmp(argv[1], "--mesh-closest")) {// host_selftest --mesh-closest FILE.obj POINTS.f32: per point "T feature q sdis gx gy gz" (the floats as
		std::vector<float> verts;								// their bits in hex) from the x86 build of the kernel's own functions; any mesh, closed or not
		std::vector<int32_t> tris;
		if(!pio::read_obj_mesh(argv[2], verts, tris)) return 3;
		std::ifstream in(argv[3], std::ios::binary | std::ios::ate);
		if(!in) return 3;
		const size_t bytes = (size_t) in.tellg();
		std::vector<float> pts(bytes / sizeof(float));
		in.seekg(0);
		in.read(reinterpret_cast<char*>(pts.data()), (std::streamsize) bytes);
		if(pts.size() % 3) return 5;
		std::vector<mpm::MeshTri> rec;
		std::vector<mpm::MeshPseudo> pseudo;
		mpm::MeshReport rep;
		mpm::mesh_build(verts.data(), verts.size() / 3, tris.data(), tris.size() / 3, (size_t) 1 << 22, (size_t) 1 << 22, rec, pseudo, rep);
		if(rec.empty()) return 6;
		for(size_t i = 0; i < pts.size() / 3; ++i) {
			const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
			float out[4], q;
			int feature;
			const int T = mpm::mesh_point_query(rec, pseudo, p, 0, out, feature, q);
			uint32_t w[5];
			std::memcpy(&w[0], &q, 4);
			std::memcpy(&w[1], out, 16);
			std::printf("%d %d %08x %08x %08x %08x %08x\n", T, feature, w[0], w[1], w[2], w[3], w[4]);
		}
		return 0;
	}
	if(argc == 12 && !std::strcmp(argv[1], "--volume-query")) {// host_selftest --volume-query TABLE.f32 d0 d1 d2 o0 o1 o2 SPACING INSIDE_OUT POINTS.f32: per material
		mpm::Volume f {};										 // point "sdis nx ny nz" (their bits in hex) from the x86 build of the kernels' own volume_query
		for(int d = 0; d < 3; ++d) {
			f.dims[d]	= std::atoi(argv[3 + d]);
			f.origin[d] = std::strtof(argv[6 + d], nullptr);
			if(f.dims[d] < mpm::kVolumeMinSamples || f.dims[d] > mpm::kVolumeMaxSamples) return 5;
		}
		f.spacing	 = std::strtof(argv[9], nullptr);
		f.inside_out = std::atoi(argv[10]) ? 1 : 0;
		std::vector<float> arr[2];
		for(int a = 0; a < 2; ++a) {
			std::ifstream in(argv[a ? 11 : 2], std::ios::binary | std::ios::ate);
			if(!in) return 3;
			const size_t bytes = (size_t) in.tellg();
			arr[a].resize(bytes / sizeof(float));
			in.seekg(0);
			in.read(reinterpret_cast<char*>(arr[a].data()), (std::streamsize) bytes);
		}
		if(arr[0].size() != 4 * (size_t) f.dims[0] * (size_t) f.dims[1] * (size_t) f.dims[2] || arr[1].size() % 3) return 5;
		f.table = reinterpret_cast<const float4*>(arr[0].data());
		for(size_t i = 0; i < arr[1].size() / 3; ++i) {
			const float x[3] = {arr[1][3 * i], arr[1][3 * i + 1], arr[1][3 * i + 2]};
			float w[4], n[3];
			mpm::volume_query(f, x, w[0], n);
			std::memcpy(&w[1], n, 12);
			uint32_t b[4];
			std::memcpy(b, w, 16);
			std::printf("%08x %08x %08x %08x\n", b[0], b[1], b[2], b[3]);
		}
		return 0;
	}
	if((argc == 4 || argc == 5 || argc == 11) && !std::strcmp(argv[1], "--mesh-fill")) {// host_selftest --mesh-fill FILE.obj BITS [MARGIN [lo0 lo1 lo2 hi0 hi1 hi2]]: the mesh-sampled
		std::vector<float> verts;														  // model per point (mesh_fill_host): "count N" or "refused WHY", then per point "x y z" as bits in hex
		std::vector<int32_t> tris;
		if(!pio::read_obj_mesh(argv[2], verts, tris)) return 3;
		const int bits	   = std::atoi(argv[3]);
		const float margin = argc >= 5 ? std::strtof(argv[4], nullptr) : 0.f;
		if(bits < 4 || bits > 10) return 5;
		int box[6];
		for(int i = 0; argc == 11 && i < 6; ++i) box[i] = std::atoi(argv[5 + i]);
		std::vector<mpm::MeshTri> rec;
		std::vector<mpm::MeshPseudo> pseudo;
		mpm::MeshReport rep;
		mpm::mesh_build(verts.data(), verts.size() / 3, tris.data(), tris.size() / 3, (size_t) 1 << 22, (size_t) 1 << 22, rec, pseudo, rep);
		mpm::MeshFillRange r;
		if(rep.reason.empty() && (!(margin >= 0.f) || !std::isfinite(margin))) rep.reason = "margin must be finite and >= 0";
		if(rep.reason.empty() && !mpm::mesh_fill_range(1 << bits, verts.data(), verts.size() / 3, argc == 11 ? box : nullptr, argc == 11 ? box + 3 : nullptr, r)) rep.reason = "lo / hi outside [0, N]";
		if(!rep.reason.empty()) {
			std::printf("refused %s\n", rep.reason.c_str());
			return 0;
		}
		std::vector<float> xyz;
		mpm::mesh_fill_host(rec, pseudo, 1 << bits, r, margin, xyz);
		std::printf("count %zu\n", xyz.size() / 3);
		for(size_t i = 0; i < xyz.size() / 3; ++i) {
			uint32_t w[3];
			std::memcpy(w, &xyz[3 * i], 12);
			std::printf("%08x %08x %08x\n", w[0], w[1], w[2]);
		}
		return 0;
	}
	const char* text = R"({"simulation": {"gpuid": 0, "fps": 1200, "frames": 2, "default_dt": 5e-6},
	  "models": [{"type": "particle", "file": "two_dragons.sdf", "constitutive": "jfluid", "offset": [0.1, 0.1, 0.1],
	              "span": [1.0, 1.0, 1.0], "velocity": [0.0, -1.0, 0.0], "nested": {"a": [true, false, null, "s\"q"]}},
	             {"file": "sphere", "constitutive": "sand", "offset": [0.2, 0.1, 0.2], "span": [1, 1, 1], "velocity": [0, -1e0, 0]}]})";
	auto doc = mj::parse(text);
	std::cout << "json_ok " << (*doc)["models"].arr.size() << " " << (*doc)["simulation"]["default_dt"].number() << " "
			  << (*doc)["models"][0]["nested"]["a"][3].string() << " " << (*doc)["models"][1]["velocity"][1].number() << "\n";
	bool threw = false;
	try {
		mj::parse("{\"a\": [1, 2}");
	} catch(const std::exception&) {
		threw = true;
	}
	std::cout << "json_bad " << (threw ? "rejected" : "accepted") << "\n";
	const float dx = 1.f / 64.f;
	const int lo[3] = {20, 20, 20}, hi[3] = {44, 44, 44};
	auto pts = pio::sample_lattice(dx, lo, hi, [&](const std::array<float, 3>& p) {
		const float a = p[0] - 0.5f, b = p[1] - 0.5f, c = p[2] - 0.5f;
		return a * a + b * b + c * c <= (5 * dx) * (5 * dx);
	});
	std::cout << "sphere " << pts.size() << "\n";
	if(argc > 1) {
		const float xyz[6] = {0.25f, 0.5f, 0.75f, -1.5f, 2.0f, 3.25f};
		std::cout << "bgeo " << (pio::write_bgeo(argv[1], xyz, 2) ? "written" : "failed") << "\n";
		{// the IO worker: 8 frames queued, flush() returns only when all of them are on disk
			pio::AsyncWriter io;
			for(int f = 0; f < 8; ++f) io.write_bgeo_async(std::string(argv[1]) + ".async" + std::to_string(f), std::vector<float>(xyz, xyz + 6), 2);
			io.flush();
			int ok = 0;
			for(int f = 0; f < 8; ++f) {
				std::ifstream in(std::string(argv[1]) + ".async" + std::to_string(f), std::ios::binary | std::ios::ate);
				ok += in && in.tellg() == std::ifstream::pos_type(41 + 2 * 16 + 2);
			}
			std::cout << "async " << ok << "\n";
		}
	}
	return 0;
}
