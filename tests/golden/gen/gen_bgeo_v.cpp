// gen_bgeo_v.cpp — golden BGEO frame with a velocity point attribute, written by the reference's OWN partio (Externals/partio,
// compiled from its sources where they lie; see gen_bgeo_v.sh).  The calls of gen_bgeo.cpp plus a second VECTOR attribute "v" of
// 3 floats, added after "position" - the frame gmpm writes with simulation.output_velocity.  Points and velocities come from
// raw float32 files so that the test can feed the very same numbers to claymore_amd/host/particle_io.hpp.
#include <Partio.h>

#include <cstdio>
#include <vector>

static std::vector<float> read_f32(const char* fn) {
	std::vector<float> out;
	std::FILE* f = std::fopen(fn, "rb");
	if(!f) return out;
	float buf[3];
	while(std::fread(buf, sizeof(float), 3, f) == 3) out.insert(out.end(), buf, buf + 3);
	std::fclose(f);
	return out;
}

int main(int argc, char** argv) {
	if(argc < 4) return 2;
	const std::vector<float> xyz = read_f32(argv[1]), vel = read_f32(argv[2]);
	if(xyz.empty() || xyz.size() != vel.size()) return 3;
	const int n = (int) (xyz.size() / 3);
	Partio::ParticlesDataMutable* parts = Partio::create();
	Partio::ParticleAttribute pos		= parts->addAttribute("position", Partio::VECTOR, 3);
	Partio::ParticleAttribute v			= parts->addAttribute("v", Partio::VECTOR, 3);
	parts->addParticles(n);
	for(int idx = 0; idx < n; ++idx) {
		float* p = parts->dataWrite<float>(pos, idx);
		float* q = parts->dataWrite<float>(v, idx);
		for(int k = 0; k < 3; k++) {
			p[k] = xyz[3 * idx + k];
			q[k] = vel[3 * idx + k];
		}
	}
	Partio::write(argv[3], *parts);
	parts->release();
	return 0;
}
