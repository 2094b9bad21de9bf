// bgeo_ids_selftest.cpp - the BGEO writer's INT point attribute without a GPU (tests/test_particle_ids_bgeo_cpu.py):
//   bgeo_ids_selftest points.f32 ids.i32 out.bgeo [vel.f32]   raw float32 xyz and raw int32 ids -> a frame with "id" (behind "v", if given)
#include <cstdint>
#include <fstream>
#include <vector>

#include "particle_io.hpp"

template<typename T>
static bool slurp(const char* fn, std::vector<T>& out) {
	std::ifstream in(fn, std::ios::binary | std::ios::ate);
	if(!in) return false;
	const std::streamsize bytes = in.tellg();
	in.seekg(0);
	out.resize((size_t) bytes / sizeof(T));
	return (bool) in.read(reinterpret_cast<char*>(out.data()), bytes);
}

int main(int argc, char** argv) {
	if(argc != 4 && argc != 5) return 2;
	std::vector<float> xyz, vel;
	std::vector<int32_t> ids;
	if(!slurp(argv[1], xyz) || !slurp(argv[2], ids) || (argc == 5 && !slurp(argv[4], vel))) return 3;
	const size_t n = xyz.size() / 3;
	if(ids.size() != n || (argc == 5 && vel.size() != 3 * n)) return 3;
	return pio::write_bgeo_frame(argv[3], xyz.data(), n, argc == 5 ? vel.data() : nullptr, nullptr, ids.data()) ? 0 : 4;
}
