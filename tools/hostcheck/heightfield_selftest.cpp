// Stand-alone check of the heightfield's index arithmetic for a sanitizer: it includes only the header, builds the smallest tables (2 x 2,
// 2 x 9, 9 x 2) in heap blocks of exactly nx * nz entries, and queries the footprint's corners, edges and interior and the points one
// float beyond every edge.  Inside: finite answers that reproduce the height at the samples; outside and NaN: sdis = NaN, n = 0, nothing
// loaded.  Exit 0 = all held; under -fsanitize=address,undefined an index outside a table aborts instead.
// Build: g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/hostcheck -Iclaymore_amd/csrc
//        -o heightfield_selftest tools/hostcheck/heightfield_selftest.cpp
struct float4 {
	float x, y, z, w;
};
#include "mpm_collision_heightfield.hpp"
#include <cmath>
#include <cstdio>
#include <memory>
using namespace mpm;

static int failures = 0;
static void expect(bool ok, const char* what, int nx, int nz, float x, float z) {
	if(!ok) {
		std::fprintf(stderr, "heightfield_selftest: %s at table %d x %d, point (%.9g, %.9g)\n", what, nx, nz, x, z);
		++failures;
	}
}

static void run(int nx, int nz, float origin_x, float origin_z, float spacing, int inside_out) {
	const size_t n = (size_t) nx * nz;
	std::unique_ptr<float[]> H(new float[n]);
	std::unique_ptr<float4[]> T(new float4[n]);
	for(int i = 0; i < nx; ++i)
		for(int k = 0; k < nz; ++k) H[(size_t) i * nz + k] = 0.25f + 0.03125f * (float) i - 0.015625f * (float) k + 0.0078125f * (float) ((i * k) % 3);
	expect(heightfield_build(H.get(), nx, nz, spacing, T.get()), "a finite table was refused", nx, nz, 0.f, 0.f);
	const Heightfield f {T.get(), nx, nz, {origin_x, origin_z}, spacing, inside_out};
	const float x_hi = origin_x + (float) (nx - 1) * spacing, z_hi = origin_z + (float) (nz - 1) * spacing;
	// every sample, every cell centre, every edge midpoint
	for(int i2 = 0; i2 <= 2 * (nx - 1); ++i2)
		for(int k2 = 0; k2 <= 2 * (nz - 1); ++k2) {
			const float x[3] = {origin_x + 0.5f * (float) i2 * spacing, 0.5f, origin_z + 0.5f * (float) k2 * spacing};
			float sdis, nrm[3];
			heightfield_query(f, x, sdis, nrm);
			const float u = (x[0] - origin_x) / spacing, w = (x[2] - origin_z) / spacing;
			const bool in = u >= 0.f && u <= (float) (nx - 1) && w >= 0.f && w <= (float) (nz - 1);
			if(in) {
				expect(std::isfinite(sdis) && std::isfinite(nrm[0]) && std::isfinite(nrm[2]), "no finite answer inside the footprint", nx, nz, x[0], x[2]);
				expect(inside_out ? nrm[1] < 0.f : nrm[1] > 0.f, "the normal does not point away from the solid", nx, nz, x[0], x[2]);
				if(i2 % 2 == 0 && k2 % 2 == 0 && u == (float) (i2 / 2) && w == (float) (k2 / 2)) {// on a sample: h is the sample's height
					const float len = std::sqrt((T[(size_t) (i2 / 2) * nz + k2 / 2].y * T[(size_t) (i2 / 2) * nz + k2 / 2].y + 1.f) + T[(size_t) (i2 / 2) * nz + k2 / 2].z * T[(size_t) (i2 / 2) * nz + k2 / 2].z);
					const float want = (0.5f - H[(size_t) (i2 / 2) * nz + k2 / 2]) / len;
					expect(sdis == (inside_out ? -want : want), "the height at a sample is not the sample", nx, nz, x[0], x[2]);
				}
			} else
				expect(sdis != sdis && nrm[0] == 0.f && nrm[1] == 0.f && nrm[2] == 0.f, "a point outside the footprint was answered", nx, nz, x[0], x[2]);
		}
	// one float beyond every edge, at the corners and in the middle of the edges; far away; NaN
	const float xs[5] = {std::nextafter(origin_x, -INFINITY), origin_x, 0.5f * (origin_x + x_hi), x_hi, std::nextafter(x_hi, INFINITY)};
	const float zs[5] = {std::nextafter(origin_z, -INFINITY), origin_z, 0.5f * (origin_z + z_hi), z_hi, std::nextafter(z_hi, INFINITY)};
	for(int a = 0; a < 5; ++a)
		for(int b = 0; b < 5; ++b) {
			const float x[3] = {xs[a], 0.5f, zs[b]};
			float sdis, nrm[3];
			heightfield_query(f, x, sdis, nrm);
			const float u = (x[0] - origin_x) / spacing, w = (x[2] - origin_z) / spacing;
			const bool in = u >= 0.f && u <= (float) (nx - 1) && w >= 0.f && w <= (float) (nz - 1);
			expect(in ? std::isfinite(sdis) : (sdis != sdis && nrm[1] == 0.f), "a point at the footprint's rim was answered wrongly", nx, nz, x[0], x[2]);
		}
	const float far[6][3] = {{-1e30f, 0.f, 0.f}, {1e30f, 0.f, 1e30f}, {INFINITY, 0.f, 0.f}, {0.f, 0.f, -INFINITY}, {NAN, 0.f, origin_z}, {origin_x, NAN, NAN}};
	for(const auto& x: far) {
		float sdis, nrm[3];
		heightfield_query(f, x, sdis, nrm);
		expect(sdis != sdis && nrm[0] == 0.f && nrm[1] == 0.f && nrm[2] == 0.f, "a far or NaN point was answered", nx, nz, x[0], x[2]);
	}
}

int main() {
	const int dims[3][2] = {{2, 2}, {2, 9}, {9, 2}};
	for(const auto& d: dims)
		for(int io = 0; io < 2; ++io) {
			run(d[0], d[1], 0.f, 0.f, 0.015625f, io);
			run(d[0], d[1], -0.1f, 0.3f, 0.013f, io);
		}
	// the builder refuses what is not finite
	float bad[4] = {0.f, 1.f, INFINITY, 0.f};
	float4 out[4];
	if(heightfield_build(bad, 2, 2, 1.f, out)) ++failures, std::fprintf(stderr, "heightfield_selftest: an infinite height was accepted\n");
	bad[2] = 3e38f, bad[0] = -3e38f;
	if(heightfield_build(bad, 2, 2, 1.f, out)) ++failures, std::fprintf(stderr, "heightfield_selftest: an overflowing difference was accepted\n");
	if(failures) return 1;
	std::printf("heightfield_selftest ok\n");
	return 0;
}
