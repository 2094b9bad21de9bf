// gen_bgeo_stress.cpp — golden BGEO frame with the stress point attributes, written by the reference's OWN partio (Externals/partio,
// compiled from its sources where they lie; see gen_bgeo_stress.sh).  The calls of gen_bgeo.cpp plus four FLOAT attributes added after
// "position": "stress" of 6 floats, "J", "pressure" and "vonmises" of 1 - the frame gmpm writes with simulation.output_stress.  Points and
// values (9 floats a point: stress6, J, pressure, von Mises) come from raw float32 files so that the test can feed the very same numbers
// to claymore_amd/host/particle_io.hpp.
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
	const std::vector<float> xyz = read_f32(argv[1]), val = read_f32(argv[2]);
	if(xyz.empty() || xyz.size() * 3 != val.size()) return 3;
	const int n = (int) (xyz.size() / 3);
	Partio::ParticlesDataMutable* parts = Partio::create();
	Partio::ParticleAttribute pos		= parts->addAttribute("position", Partio::VECTOR, 3);
	Partio::ParticleAttribute stress	= parts->addAttribute("stress", Partio::FLOAT, 6);
	Partio::ParticleAttribute scalar[3] = {parts->addAttribute("J", Partio::FLOAT, 1), parts->addAttribute("pressure", Partio::FLOAT, 1), parts->addAttribute("vonmises", Partio::FLOAT, 1)};
	parts->addParticles(n);
	for(int idx = 0; idx < n; ++idx) {
		float* p = parts->dataWrite<float>(pos, idx);
		for(int k = 0; k < 3; k++) p[k] = xyz[3 * idx + k];
		float* s = parts->dataWrite<float>(stress, idx);
		for(int k = 0; k < 6; k++) s[k] = val[9 * idx + k];
		for(int k = 0; k < 3; k++) *parts->dataWrite<float>(scalar[k], idx) = val[9 * idx + 6 + k];
	}
	Partio::write(argv[3], *parts);
	parts->release();
	return 0;
}
