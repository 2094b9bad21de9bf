// x86 build of the node-cube lane mapping (mpm_cube_lane.hpp) behind a C interface: out5 = {on, octant, cell, gather-arena node, scatter-arena node}.
// Build: g++ -O2 -std=c++17 -fPIC -shared -Iclaymore_amd/csrc -o libhostcube.so tools/hostcheck/check_cube.cpp   (tests/test_cube_lane_model.py does)
#include "mpm_cube_lane.hpp"
extern "C" void host_cube_lane(int pass, int lane, int* out5) {
	const mpm::CubeLane c = mpm::cube_lane(pass, lane);
	out5[0] = c.on ? 1 : 0;
	out5[1] = c.octant;
	out5[2] = c.cell;
	out5[3] = c.g2p;
	out5[4] = c.p2g;
}
